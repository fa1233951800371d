#!/usr/bin/env python3
"""K2 soft votes against the hard-vote row-major multiclass kernel, same pool,
one process.

For each BASELINE shape (config 2: 100,000 x 64, T = 10; config 3: 284,807 x
30, T = 100; config 4: 2,000,000 x 256, T = 10; depth 4) and for C = 2 and
C = 10 the two entry points are launched alternately and timed with HIP
events:

  dal_forest_score_multiclass  the soft forest's hard() (arg-max leaves, the same
                               inner nodes), entropy, counts and pred written
  dal_forest_score_soft        the ProbabilityForest, entropy, sums and pred written

and the medians (and minima) of ROUNDS launches each, their ratio, and the
bytes each launch moves (the pool once, N d 4, plus its outputs) over its
median time as a share of the 6.3 TB/s the project takes as achievable go to
profiles/soft/config<N>.json.  Without --config every shape runs in a fresh
child process under its own time limit, and the run stops at the first child
that fails; profiles/soft/summary.json collects the ratios.

    python scripts/bench_soft.py [--config 2|3|4] [--rounds 30] [--out DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "distributed-active-learning_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

# config -> (rows, features, trees, pool distribution)
SHAPES = {2: (100_000, 64, 10, "uniform"), 3: (284_807, 30, 100, "normal"), 4: (2_000_000, 256, 10, "uniform")}
DEPTH, CLASSES, CHILD_TIMEOUT_S = 4, (2, 10), 240
ACHIEVABLE_GB_PER_S = 6300.0
SUMMARY_KEYS = ("hard_us_median", "soft_us_median", "ratio_median", "soft_gb_per_s", "soft_share_of_achievable",
                "hard_gb_per_s", "hard_share_of_achievable")


def run_config(cfg: int, rounds: int, out_dir: str) -> dict:
    import torch

    from dal import _lib, engine
    from dal.forest import ProbabilityForest

    n, d, T, dist = SHAPES[cfg]
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    x = (torch.rand if dist == "uniform" else torch.randn)((n, d), generator=gen, device=dev, dtype=torch.float32)
    state = engine.PoolState(x, device=dev)
    del x
    flags = torch.ones(n, dtype=torch.uint8, device=dev)
    lut = engine.device_multiclass_lut("entropy", T, dev)
    res = {"config": cfg, "rows": n, "features": d, "trees": T, "depth": DEPTH, "rounds": rounds,
           "device": torch.cuda.get_device_name(dev), "achievable_gb_per_s": ACHIEVABLE_GB_PER_S, "classes": {}}
    for C in CLASSES:
        fs = ProbabilityForest.synthetic(T, DEPTH, d, C, seed=1, dist=dist)
        fh = fs.hard()

        def hard():
            return engine.forest_score_multiclass(state, fh, lut, flags, _lib.DAL_DESCENDING, _lib.DAL_MC_ENTROPY)

        def soft():
            return engine.forest_score_soft(state, fs, flags, _lib.DAL_DESCENDING, _lib.DAL_SOFT_ENTROPY)

        for _ in range(3):
            hard()
            soft()
        torch.cuda.synchronize(dev)
        events = {"hard": [], "soft": []}
        for _ in range(rounds):
            for name, fn in (("hard", hard), ("soft", soft)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda._sleep(400_000)  # the launch is queued before the GPU reaches the start event
                a.record()
                fn()
                b.record()
                events[name].append((a, b))
        torch.cuda.synchronize(dev)
        times = {k: [a.elapsed_time(b) * 1e3 for a, b in v] for k, v in events.items()}  # us
        med = {k: statistics.median(v) for k, v in times.items()}
        # the pool and the row flags read once; sums (8 C) or counts (C), pred, score and key written
        nbytes = {"soft": n * (d * 4 + 1 + 8 * C + 1 + 16), "hard": n * (d * 4 + 1 + C + 1 + 16)}
        r = {"classes": C, "leaves": fs.n_leaves}
        for k in ("hard", "soft"):
            gbs = nbytes[k] / med[k] / 1e3
            r.update({f"{k}_us_median": med[k], f"{k}_us_min": min(times[k]), f"{k}_bytes": nbytes[k],
                      f"{k}_gb_per_s": gbs, f"{k}_share_of_achievable": gbs / ACHIEVABLE_GB_PER_S, f"{k}_us": times[k]})
        r["ratio_median"] = med["soft"] / med["hard"]
        res["classes"][str(C)] = r
        print(json.dumps({"config": cfg, "classes": C, **{k: r[k] for k in SUMMARY_KEYS}}), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"config{cfg}.json"), "w") as f:
        json.dump(res, f, indent=1)
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", type=int, choices=sorted(SHAPES))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "soft"))
    a = ap.parse_args()
    if a.rounds < 20:
        ap.error("--rounds must be at least 20")
    if a.config is not None:
        run_config(a.config, a.rounds, a.out)
        return 0
    summary = {}
    for cfg in sorted(SHAPES):
        # a fresh process per shape, each under its own time limit; nothing
        # more is started on the GPU after a child fails or runs out of time
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", str(cfg), "--rounds",
                                 str(a.rounds), "--out", a.out], timeout=CHILD_TIMEOUT_S).returncode
        except subprocess.TimeoutExpired:
            print(f"config {cfg}: no result within {CHILD_TIMEOUT_S} s; stopping", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"config {cfg}: exit status {rc}; stopping", file=sys.stderr)
            return rc if rc > 0 else 1
        with open(os.path.join(a.out, f"config{cfg}.json")) as f:
            r = json.load(f)
        summary[f"config{cfg}"] = {"rows": r["rows"], "features": r["features"], "trees": r["trees"],
                                   **{f"C{c}": {k: v[k] for k in SUMMARY_KEYS} for c, v in r["classes"].items()}}
    with open(os.path.join(a.out, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
