#!/usr/bin/env python3
"""K2 soft-vote BALD against the soft-vote entropy kernel, same pool, one
process.

For config 4 (2,000,000 x 256, T = 10) and config 3 (284,807 x 30, T = 100),
depth 4, and for C = 2 and C = 10, three launches alternate and are timed with
HIP events:

  entropy    dal_forest_score_soft(DAL_SOFT_ENTROPY), sums and pred written:
             the yardstick (the code the parent commit has)
  bald       dal_forest_score_soft_bald, every output written (16 more bytes
             per row: hsum and entropy)
  bald_lean  dal_forest_score_soft_bald with hsum and entropy null (the bytes of
             the yardstick)

Every launch writes into buffers allocated once.  Per launch the medians and
minima of ROUNDS timings, the ratio of the medians to the yardstick's, the
byte ratio (the pool once, N d 4, plus the outputs), the yardstick's own spread
((p90 - p10) / median of its timings) and the bytes over the median time as a
share of the 6.3 TB/s the project takes as achievable go to
profiles/bald/config<N>.json.  Without --config every shape runs in a fresh
child process under its own time limit, and the run stops at the first child
that fails; profiles/bald/summary.json collects the ratios.

    python scripts/bench_bald.py [--config 3|4] [--rounds 30] [--out DIR]
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
SHAPES = {3: (284_807, 30, 100, "normal"), 4: (2_000_000, 256, 10, "uniform")}
DEPTH, CLASSES, CHILD_TIMEOUT_S = 4, (2, 10), 240
ACHIEVABLE_GB_PER_S = 6300.0
KINDS = ("entropy", "bald", "bald_lean")
SUMMARY_KEYS = ("entropy_us_median", "bald_us_median", "bald_lean_us_median", "ratio_bald", "ratio_bald_lean",
                "byte_ratio_bald", "entropy_spread", "bald_share_of_achievable", "entropy_share_of_achievable")


def _spread(v):
    q = statistics.quantiles(v, n=10)
    return (q[8] - q[0]) / statistics.median(v)


def run_config(cfg: int, rounds: int, out_dir: str) -> dict:
    import torch

    from dal import _lib
    from dal.forest import ProbabilityForest

    n, d, T, dist = SHAPES[cfg]
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    x = (torch.rand if dist == "uniform" else torch.randn)((n, d), generator=gen, device=dev, dtype=torch.float32)
    flags = torch.ones(n, dtype=torch.uint8, device=dev)
    pred = torch.empty(n, dtype=torch.uint8, device=dev)
    hsum = torch.empty(n, dtype=torch.int64, device=dev)
    entropy = torch.empty(n, dtype=torch.float64, device=dev)
    scores = torch.empty(n, dtype=torch.float64, device=dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = {"config": cfg, "rows": n, "features": d, "trees": T, "depth": DEPTH, "rounds": rounds,
           "device": torch.cuda.get_device_name(dev), "achievable_gb_per_s": ACHIEVABLE_GB_PER_S, "classes": {}}
    for C in CLASSES:
        F = ProbabilityForest.synthetic(T, DEPTH, d, C, seed=1, dist=dist)
        inner, leaf_id, leaf_q = F.device(dev)
        leaf_h = F.device_leaf_h(dev)
        sums = torch.empty((n, C), dtype=torch.int64, device=dev)
        forest = (inner.data_ptr(), leaf_id.data_ptr(), leaf_q.data_ptr())
        shape = (F.n_leaves, T, DEPTH, C)

        def entropy_kernel():
            _lib.call("dal_forest_score_soft", x.data_ptr(), n, d, d, *forest, *shape, _lib.DAL_SOFT_ENTROPY,
                      flags.data_ptr(), _lib.DAL_DESCENDING, sums.data_ptr(), pred.data_ptr(), scores.data_ptr(),
                      keys.data_ptr(), stream)

        def bald(lean=False):
            _lib.call("dal_forest_score_soft_bald", x.data_ptr(), n, d, d, *forest, leaf_h.data_ptr(), *shape,
                      flags.data_ptr(), _lib.DAL_DESCENDING, sums.data_ptr(), pred.data_ptr(),
                      0 if lean else hsum.data_ptr(), 0 if lean else entropy.data_ptr(), scores.data_ptr(),
                      keys.data_ptr(), stream)

        fns = {"entropy": entropy_kernel, "bald": bald, "bald_lean": lambda: bald(lean=True)}
        for _ in range(3):
            for k in KINDS:
                fns[k]()
        torch.cuda.synchronize(dev)
        # the two forms score the same rows: the entropy BALD returns is the yardstick's score
        entropy_kernel()
        ref = scores.clone()
        bald()
        if not torch.equal(ref.view(torch.int64), entropy.view(torch.int64)):
            raise SystemExit("the entropy of the BALD kernel is not the entropy kernel's")
        events = {k: [] for k in KINDS}
        for _ in range(rounds):
            for k in KINDS:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda._sleep(400_000)  # the launch is queued before the GPU reaches the start event
                a.record()
                fns[k]()
                b.record()
                events[k].append((a, b))
        torch.cuda.synchronize(dev)
        times = {k: [a.elapsed_time(b) * 1e3 for a, b in v] for k, v in events.items()}  # us
        med = {k: statistics.median(v) for k, v in times.items()}
        # the pool and the row flags read once; sums (8 C), pred, score and key written; bald: hsum and entropy too
        base = n * (d * 4 + 1 + 8 * C + 1 + 16)
        nbytes = {"entropy": base, "bald": base + n * 16, "bald_lean": base}
        r = {"classes": C, "leaves": F.n_leaves}
        for k in KINDS:
            gbs = nbytes[k] / med[k] / 1e3
            r.update({f"{k}_us_median": med[k], f"{k}_us_min": min(times[k]), f"{k}_bytes": nbytes[k],
                      f"{k}_gb_per_s": gbs, f"{k}_share_of_achievable": gbs / ACHIEVABLE_GB_PER_S,
                      f"{k}_spread": _spread(times[k]), f"{k}_us": times[k]})
        r["ratio_bald"] = med["bald"] / med["entropy"]
        r["ratio_bald_lean"] = med["bald_lean"] / med["entropy"]
        r["byte_ratio_bald"] = nbytes["bald"] / nbytes["entropy"]
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bald"))
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
