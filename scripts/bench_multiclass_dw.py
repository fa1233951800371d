#!/usr/bin/env python3
"""K2 multiclass, density-weighted, against the uncertainty form: same pool,
same forest, one process.

For each shape (config 2: 100,000 x 64, T = 10; config 3: 284,807 x 30,
T = 100; config 4: 2,000,000 x 256 at T = 10 and T = 100; depth 4, C = 10) the
two entry points are launched alternately and timed with HIP events:

  dal_forest_score_multiclass     entropy, counts and pred written (the yardstick)
  dal_forest_score_multiclass_dw  DAL_DENSITY_FIXED, keys_hi, counts and pred written

The DW form moves 28 more bytes per row (density 8, keys_hi 8, entropy 8,
index 4); both algorithmic byte counts are recorded with the medians and
[min, max] of ROUNDS launches each.  The density words are seeded fixed-point
values, not a Gram (the kernel's time does not depend on them, and a 2M-row
Gram has no place in a kernel benchmark).  The check recorded per shape: the
DW / uncertainty time ratio against the byte ratio plus the uncertainty form's
own (max - min) / median spread in this run.

With --select (config 2's shape) one cold density_weighting.select_multiclass
is timed against the binary density_weighting.select on its unfused branch
(per-kernel events on), each on a fresh PoolState, for orientation.

Without --case every case runs in a fresh child process under its own time
limit, and the run stops at the first child that fails.

    python scripts/bench_multiclass_dw.py [--case NAME] [--rounds 30] [--out DIR]
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

# case -> (rows, features, trees, pool distribution)
CASES = {"config2": (100_000, 64, 10, "uniform"), "config3": (284_807, 30, 100, "normal"),
         "config4": (2_000_000, 256, 10, "uniform"), "config4_T100": (2_000_000, 256, 100, "uniform")}
DEPTH, CLASSES, CHILD_TIMEOUT_S = 4, 10, 240


def _pool(n, d, dist, dev):
    import torch

    gen = torch.Generator(device=dev).manual_seed(0)
    return (torch.rand if dist == "uniform" else torch.randn)((n, d), generator=gen, device=dev, dtype=torch.float32)


def run_case(name: str, rounds: int, out_dir: str) -> dict:
    import torch

    from dal import _lib, engine
    from dal.forest import Forest

    n, d, T, dist = CASES[name]
    dev = torch.device("cuda:0")
    state = engine.PoolState(_pool(n, d, dist, dev), device=dev)
    F = Forest.synthetic(T, DEPTH, d, seed=1, dist=dist, n_classes=CLASSES)
    flags = torch.ones(n, dtype=torch.uint8, device=dev)
    lut = engine.device_multiclass_lut("entropy", T, dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    dens = (torch.rand(n, generator=gen, device=dev, dtype=torch.float64) * (0.7 * n) * _lib.DAL_FIXED_SCALE).to(
        torch.int64)
    derr = engine.density_error(state)

    def uncertainty():
        return engine.forest_score_multiclass(state, F, lut, flags, _lib.DAL_DESCENDING, _lib.DAL_MC_ENTROPY)

    def dw():
        return engine.forest_score_multiclass_dw(state, F, flags, dens, _lib.DAL_DENSITY_FIXED, derr, 1.0, True)

    for _ in range(3):
        uncertainty()
        dw()
    torch.cuda.synchronize(dev)
    events = {"uncertainty": [], "dw": []}
    for _ in range(rounds):
        for key, fn in (("uncertainty", uncertainty), ("dw", dw)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(400_000)  # the launch is queued before the GPU reaches the start event
            a.record()
            fn()
            b.record()
            events[key].append((a, b))
    torch.cuda.synchronize(dev)
    times = {k: [a.elapsed_time(b) * 1e3 for a, b in v] for k, v in events.items()}  # us
    med = {k: statistics.median(v) for k, v in times.items()}
    bytes_u = 4 * d + 1 + CLASSES + 1 + 8 + 8  # pool row, flags, counts, pred, score, key
    bytes_dw = bytes_u + 28                    # + density, keys_hi, entropy, index
    spread = (max(times["uncertainty"]) - min(times["uncertainty"])) / med["uncertainty"]
    ratio, byte_ratio = med["dw"] / med["uncertainty"], bytes_dw / bytes_u
    res = {
        "case": name, "rows": n, "features": d, "trees": T, "depth": DEPTH, "classes": CLASSES, "rounds": rounds,
        "device": torch.cuda.get_device_name(dev),
        "uncertainty_us_median": med["uncertainty"],
        "uncertainty_us_min_max": [min(times["uncertainty"]), max(times["uncertainty"])],
        "dw_us_median": med["dw"], "dw_us_min_max": [min(times["dw"]), max(times["dw"])],
        "bytes_per_row_uncertainty": bytes_u, "bytes_per_row_dw": bytes_dw,
        "byte_ratio": byte_ratio, "time_ratio_median": ratio, "uncertainty_spread": spread,
        "within_byte_ratio_plus_spread": bool(ratio <= byte_ratio + spread),
        "gb_per_s_uncertainty": n * bytes_u / med["uncertainty"] / 1e3,
        "gb_per_s_dw": n * bytes_dw / med["dw"] / 1e3,
        "uncertainty_us": times["uncertainty"], "dw_us": times["dw"],
    }
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"dw_{name}.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("case", "uncertainty_us_median", "dw_us_median", "time_ratio_median",
                                          "byte_ratio", "uncertainty_spread")}), flush=True)
    return res


def run_select(rounds: int, out_dir: str) -> dict:
    """One cold selection, k = 100, E = range(100), at config 2's shape: the
    multiclass step against the binary step's unfused branch."""
    import numpy as np
    import torch

    from dal import density_weighting as dwm
    from dal import engine
    from dal.forest import Forest

    n, d, T, dist = CASES["config2"]
    dev = torch.device("cuda:0")
    x = _pool(n, d, dist, dev)
    fb = Forest.synthetic(T, DEPTH, d, seed=1, dist=dist)
    fm = Forest.synthetic(T, DEPTH, d, seed=1, dist=dist, n_classes=CLASSES)
    unl = torch.arange(100, n, dtype=torch.int64, device=dev)
    E = np.arange(100)

    def binary():
        st = engine.PoolState(x, excluded=E, device=dev)
        st.forest_events, st.select_events = [], []  # per-kernel events: the unfused branch
        return st, lambda: dwm.select(st, unl, fb, 100)

    def multi():
        st = engine.PoolState(x, excluded=E, device=dev)
        return st, lambda: dwm.select_multiclass(st, unl, fm, 100)

    times = {"binary_unfused": [], "multiclass": []}
    reps = max(3, rounds // 10)
    for i in range(reps + 1):  # (the first pair loads the code objects)
        for key, make in (("binary_unfused", binary), ("multiclass", multi)):
            st, fn = make()
            torch.cuda.synchronize(dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize(dev)
            if i:
                times[key].append(a.elapsed_time(b) * 1e3)
    res = {"rows": n, "features": d, "trees": T, "classes": CLASSES, "k": 100, "calls": reps,
           "device": torch.cuda.get_device_name(dev),
           "note": "whole cold call between two HIP events, host time included (the call reads the status word)"}
    for key, v in times.items():
        res[f"{key}_us_median"] = statistics.median(v)
        res[f"{key}_us_min_max"] = [min(v), max(v)]
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "dw_select_config2.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--case", choices=sorted(CASES) + ["select"])
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "multiclass"))
    a = ap.parse_args()
    if a.rounds < 20:
        ap.error("--rounds must be at least 20")
    if a.case == "select":
        run_select(a.rounds, a.out)
        return 0
    if a.case is not None:
        run_case(a.case, a.rounds, a.out)
        return 0
    summary = {}
    for name in list(CASES) + ["select"]:
        # a fresh process per case, each under its own time limit; nothing
        # more is started on the GPU after a child fails or runs out of time
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--rounds",
                                 str(a.rounds), "--out", a.out], timeout=CHILD_TIMEOUT_S).returncode
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {CHILD_TIMEOUT_S} s; stopping", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"{name}: exit status {rc}; stopping", file=sys.stderr)
            return rc if rc > 0 else 1
        fn = "dw_select_config2.json" if name == "select" else f"dw_{name}.json"
        with open(os.path.join(a.out, fn)) as f:
            r = json.load(f)
        summary[name] = {k: v for k, v in r.items() if not isinstance(v, list) or len(v) <= 2}
    with open(os.path.join(a.out, "dw_summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
