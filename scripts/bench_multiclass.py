#!/usr/bin/env python3
"""K2 multiclass against the binary row-major kernel, same pool, one process.

For each BASELINE shape (config 2: 100,000 x 64, T = 10; config 3: 284,807 x
30, T = 100; config 4: 2,000,000 x 256, T = 10; depth 4) the two entry points
are launched alternately and timed with HIP events:

  dal_forest_score             binary forest, row-major, uncertainty mode (the yardstick)
  dal_forest_score_multiclass  C = 10, entropy, counts and pred written

and the medians (and minima) of ROUNDS launches each, with their ratio, go to
profiles/multiclass/config<N>.json.  Without --config every shape runs in a
fresh child process under its own time limit, and the run stops at the first
child that fails; profiles/multiclass/summary.json collects the ratios.

    python scripts/bench_multiclass.py [--config 2|3|4] [--rounds 30] [--out DIR]
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
DEPTH, CLASSES, CHILD_TIMEOUT_S = 4, 10, 240


def run_config(cfg: int, rounds: int, out_dir: str) -> dict:
    import torch

    from dal import _lib, engine
    from dal.forest import Forest

    n, d, T, dist = SHAPES[cfg]
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    x = (torch.rand if dist == "uniform" else torch.randn)((n, d), generator=gen, device=dev, dtype=torch.float32)
    state = engine.PoolState(x, device=dev)
    del x
    fb = Forest.synthetic(T, DEPTH, d, seed=1, dist=dist)
    fm = Forest.synthetic(T, DEPTH, d, seed=1, dist=dist, n_classes=CLASSES)
    flags = torch.ones(n, dtype=torch.uint8, device=dev)
    lut_b = engine.device_lut("entropy", T, dev)
    lut_m = engine.device_multiclass_lut("entropy", T, dev)

    def binary():
        return engine.forest_score(state, fb, lut_b, flags, _lib.DAL_DESCENDING)

    def multi():
        return engine.forest_score_multiclass(state, fm, lut_m, flags, _lib.DAL_DESCENDING, _lib.DAL_MC_ENTROPY)

    for _ in range(3):
        binary()
        multi()
    torch.cuda.synchronize(dev)
    events = {"binary": [], "multiclass": []}
    for _ in range(rounds):
        for name, fn in (("binary", binary), ("multiclass", multi)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(400_000)  # the launch is queued before the GPU reaches the start event
            a.record()
            fn()
            b.record()
            events[name].append((a, b))
    torch.cuda.synchronize(dev)
    times = {k: [a.elapsed_time(b) * 1e3 for a, b in v] for k, v in events.items()}  # us
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {
        "config": cfg, "rows": n, "features": d, "trees": T, "depth": DEPTH, "classes": CLASSES, "rounds": rounds,
        "device": torch.cuda.get_device_name(dev),
        "binary_us_median": med["binary"], "binary_us_min": min(times["binary"]),
        "multiclass_us_median": med["multiclass"], "multiclass_us_min": min(times["multiclass"]),
        "ratio_median": med["multiclass"] / med["binary"],
        "pool_gb_per_s_binary": n * d * 4 / med["binary"] / 1e3,
        "pool_gb_per_s_multiclass": n * d * 4 / med["multiclass"] / 1e3,
        "binary_us": times["binary"], "multiclass_us": times["multiclass"],
    }
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"config{cfg}.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("config", "binary_us_median", "multiclass_us_median", "ratio_median")}),
          flush=True)
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", type=int, choices=sorted(SHAPES))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multiclass"))
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
        summary[f"config{cfg}"] = {k: r[k] for k in ("rows", "features", "trees", "classes", "binary_us_median",
                                                      "multiclass_us_median", "ratio_median")}
    with open(os.path.join(a.out, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
