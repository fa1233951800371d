#!/usr/bin/env python3
"""K2 multiclass over the blocked pool copy against the row-major kernel, same
pool, one process.

For each BASELINE shape (config 2: 100,000 x 64, T = 10; config 3: 284,807 x
30, T = 100; config 4: 2,000,000 x 256, T = 10; depth 4; forest of C = 10
classes, entropy, counts and pred written) the two entry points are launched
alternately and timed with HIP events:

  dal_forest_score_multiclass          row-major (the yardstick)
  dal_forest_score_multiclass_blocked  the pool's blocked copy + the prepared forest

and at config 4 also the density-weighted pair at beta = 1 over the pool's
Gram density (dal_forest_score_multiclass_dw / _dw_blocked).  The blocked copy
and the prepared forest are built before any timing; their one-off times are
recorded on their own.  Medians, minima, the row-major samples' interquartile
range and every sample go to profiles/multiclass/blocked_config<N>.json.
Without --config every shape runs in a fresh child process under its own time
limit, and the run stops at the first child that fails;
profiles/multiclass/blocked_summary.json collects the medians.

    python scripts/bench_multiclass_blocked.py [--config 2|3|4] [--rounds 30] [--out DIR]
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
DEPTH, CLASSES, WARMUPS, CHILD_TIMEOUT_S = 4, 10, 3, 300
DW_CONFIGS = (4,)


def _timed_once(torch, dev, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize(dev)
    return out, a.elapsed_time(b) * 1e3


def _pair(torch, dev, rounds, row_major, blocked):
    """Alternate launches: WARMUPS each, then ``rounds`` timed ones each (us)."""
    for _ in range(WARMUPS):
        row_major()
        blocked()
    torch.cuda.synchronize(dev)
    events = {"row_major": [], "blocked": []}
    for _ in range(rounds):
        for name, fn in (("row_major", row_major), ("blocked", blocked)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(400_000)  # the launch is queued before the GPU reaches the start event
            a.record()
            fn()
            b.record()
            events[name].append((a, b))
    torch.cuda.synchronize(dev)
    t = {k: [a.elapsed_time(b) * 1e3 for a, b in v] for k, v in events.items()}
    q = statistics.quantiles(t["row_major"], n=4)
    med = {k: statistics.median(v) for k, v in t.items()}
    diff = med["blocked"] - med["row_major"]
    iqr = q[2] - q[0]
    return {
        "row_major_us_median": med["row_major"], "row_major_us_min": min(t["row_major"]),
        "blocked_us_median": med["blocked"], "blocked_us_min": min(t["blocked"]),
        "row_major_us_iqr": iqr, "ratio_median": med["blocked"] / med["row_major"],
        "verdict": "blocked faster" if diff < -iqr else "blocked slower" if diff > iqr else "within the iqr",
        "row_major_us": t["row_major"], "blocked_us": t["blocked"],
    }


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
    fm = Forest.synthetic(T, DEPTH, d, seed=1, dist=dist, n_classes=CLASSES)
    rule = int(_lib.load().dal_forest_multiclass_blocked_rows(d, T, DEPTH, CLASSES))
    if rule != 64:
        raise SystemExit(f"config {cfg}: dal_forest_multiclass_blocked_rows is {rule}: nothing to compare")
    flags = torch.ones(n, dtype=torch.uint8, device=dev)
    lut = engine.device_multiclass_lut("entropy", T, dev)
    fm.device(dev)
    torch.cuda.synchronize(dev)
    xb, copy_us = _timed_once(torch, dev, lambda: state.blocked_pool(fm, multiclass=True))
    prep, prep_us = _timed_once(torch, dev, lambda: fm.blocked_prep(dev, d))
    if xb is None or prep is None:
        raise SystemExit(f"config {cfg}: no blocked copy or prepared forest")
    features_used = int(prep[:4].view(torch.int32).item())

    def us(xb_):
        return lambda: engine.forest_score_multiclass(state, fm, lut, flags, _lib.DAL_DESCENDING,
                                                      _lib.DAL_MC_ENTROPY, xb=xb_)

    res = {
        "config": cfg, "rows": n, "features": d, "trees": T, "depth": DEPTH, "classes": CLASSES, "rounds": rounds,
        "warmups": WARMUPS, "device": torch.cuda.get_device_name(dev), "features_used": features_used,
        "pool_blocked_us_once": copy_us, "forest_prepare_us_once": prep_us,
        "uncertainty": _pair(torch, dev, rounds, us(None), us(xb)),
    }
    if cfg in DW_CONFIGS:
        dens, derr = state.density_fixed(), engine.density_error(state)

        def dw(xb_):
            return lambda: engine.forest_score_multiclass_dw(state, fm, flags, dens, _lib.DAL_DENSITY_FIXED, derr, 1.0,
                                                             True, xb=xb_)

        res["density_weighted"] = _pair(torch, dev, rounds, dw(None), dw(xb))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"blocked_config{cfg}.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"config": cfg, **{k: {m: v[m] for m in SUMMARY_KEYS} for k, v in res.items()
                                        if isinstance(v, dict)}}), flush=True)
    return res


SUMMARY_KEYS = ("row_major_us_median", "blocked_us_median", "row_major_us_iqr", "ratio_median", "verdict")


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
        with open(os.path.join(a.out, f"blocked_config{cfg}.json")) as f:
            r = json.load(f)
        summary[f"config{cfg}"] = {"rows": r["rows"], "features": r["features"], "trees": r["trees"],
                                   "classes": r["classes"], "features_used": r["features_used"],
                                   "pool_blocked_us_once": r["pool_blocked_us_once"],
                                   "forest_prepare_us_once": r["forest_prepare_us_once"],
                                   **{k: {m: v[m] for m in SUMMARY_KEYS} for k, v in r.items() if isinstance(v, dict)}}
    with open(os.path.join(a.out, "blocked_summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
