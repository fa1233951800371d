#!/usr/bin/env python3
"""GPU training of regression forests (dal.random_forest.train_regressor,
csrc/rf_train_regress.hip) at the LAL model's shape, next to scikit-learn on
the same box.

Shapes (rows x features, trees; depth 4, 32 bins, "auto" = onethird features):
  5,000 x 5, T = 2,000 and 20,000 x 5, T = 2,000   the LAL regressor of
      active_learner.py:354-363 (five features, 2,000 trees); the reference's
      table is not part of this repository, so the row count is a parameter
      and the rows are synthetic: fp64 features shaped like the LAL columns,
      a smooth label with noise
  5,000 x 30, T = 100                                a wider, smaller forest

Timed per fit, wall clock around train_regressor with the rows on the device
(the host's Poisson and subset draws excluded: weights and subsets are passed
in; the exact-sum format of the labels, the uploads of the weights and the
model's copy back included), synchronised after each fit: REPS fits after a
warm-up, median and [min, max].  One further fit runs under torch.profiler and
its device time is split by kernel.  The GPU part runs in one child process
under its own time limit; scikit-learn's
RandomForestRegressor(max_depth=4, max_features=1/3, n_jobs=16).fit of the
same rows is timed on the host in the parent.  No ratio is asserted: the
numbers are recorded in profiles/rf_regress/bench.json.

--ab-lib PATH   time the fits with the library at PATH (a build of another
                commit: scripts/ab_build.sh in that checkout) and with this
                tree's -- or, with --lib PATH2, the one at PATH2: PATH against
                itself gives the spread of the measurement -- in alternating
                child processes, ALTERNATIONS each; no kernel split, no
                scikit-learn.  Written to regress_ab.json (--out-name) in --out.

    python scripts/bench_rf_regress.py [--reps 5] [--out profiles/rf_regress] [--ab-lib PATH [--lib PATH2]]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "distributed-active-learning_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = ((5000, 5, 2000), (20000, 5, 2000), (5000, 30, 100))  # n, d, T
DEPTH = 4
CHILD_TIMEOUT_S, ALTERNATIONS = 420, 3


def _rows(n, d):
    import numpy as np

    rng = np.random.default_rng(11)
    X = rng.random((n, d))
    v = rng.integers(0, 11, n)
    X[:, 0] = v / 10.0
    X[:, 1] = np.sqrt(v / 10.0 * (1 - v / 10.0) * 10.0 / 9.0)
    y = 0.3 * X[:, 1] - 0.1 * np.abs(X[:, 0] - 0.5) + 0.2 * X[:, 2] * X[:, 3] + 0.02 * rng.standard_normal(n)
    return X, y


def _summary(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "fits": len(ts)}


def _kernel_split(fit):
    """Device time of one fit by kernel name (torch.profiler), ms."""
    import torch
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fit()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        dev_us = getattr(ev, "device_time_total", None)
        if dev_us is None:
            dev_us = getattr(ev, "cuda_time_total", 0.0)
        m = re.search(r"rf_\w+_kernel(<\w+>)?", ev.key)
        name = m.group(0) if m else ev.key.strip() if ("Memset" in ev.key or "Memcpy" in ev.key) else None
        if dev_us and name:
            rec = out.setdefault(name, {"calls": 0, "ms": 0.0})
            rec["calls"] += ev.count
            rec["ms"] += dev_us / 1e3
    return out


def child(reps: int, lib_path=None, split=True) -> dict:
    import torch

    if lib_path:  # another build: keep the symbols it has
        import ctypes

        from dal import _lib

        _lib.LIB_PATH = os.path.abspath(lib_path)
        probe = ctypes.CDLL(_lib.LIB_PATH)
        for missing in [name for name in _lib.SIGNATURES if not hasattr(probe, name)]:
            del _lib.SIGNATURES[missing]
    from dal.random_forest import bagging_inputs, check_regression_labels, train_regressor

    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(dev), "reps": reps, "shapes": {}}
    for n, d, T in SHAPES:
        X, y = _rows(n, d)
        w, s = bagging_inputs(n, d, T, DEPTH, seed=1, feature_subset_strategy="onethird")
        xd = torch.from_numpy(X).to(dev)
        _, (q_y, k_y), (q_sq, k_sq) = check_regression_labels(y, n)

        def fit():
            return train_regressor(xd, y, T, max_depth=DEPTH, weights=w, feature_subsets=s, device=dev)

        fit()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fit()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        rec = _summary(ts)
        rec["label_limbs"] = {"k_y": k_y, "k_sq": k_sq, "words_per_cell": 1 + k_y + k_sq}
        rec["features_per_node"] = int(s.shape[2])
        if split:
            try:
                rec["kernels"] = _kernel_split(fit)
            except Exception as e:  # the timing above stands without the split
                rec["kernels"] = {"error": repr(e)[:200]}
        out["shapes"][f"{n}x{d}_T{T}"] = rec
    return out


def sklearn_fit() -> dict:
    from sklearn.ensemble import RandomForestRegressor

    cores = min(16, len(os.sched_getaffinity(0)))
    out = {"cores": cores}
    for n, d, T in SHAPES:
        X, y = _rows(n, d)
        ts = []
        for _ in range(2):
            t0 = time.perf_counter()
            RandomForestRegressor(n_estimators=T, max_depth=DEPTH, max_features=1 / 3, bootstrap=True,
                                  random_state=0, n_jobs=cores).fit(X, y)
            ts.append((time.perf_counter() - t0) * 1e3)
        out[f"{n}x{d}_T{T}"] = _summary(ts)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rf_regress"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--ab-lib", default=None)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out-name", default=None)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child(args.reps, args.lib, split=not args.lib)))
        return

    def run_child(lib_path):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)]
        res = subprocess.run(cmd + (["--lib", lib_path] if lib_path else []), capture_output=True, text=True,
                             timeout=CHILD_TIMEOUT_S)
        if res.returncode != 0:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
            raise SystemExit(f"child failed with status {res.returncode}")
        return json.loads(res.stdout.strip().splitlines()[-1])

    if args.ab_lib:
        this_lib = args.lib or os.path.join(REPO, "distributed-active-learning_amd", "dal", "libdal.so")
        runs = {}
        for _ in range(ALTERNATIONS):  # a failed child ends the run: nothing more is started
            for side, lib in (("other", args.ab_lib), ("this", this_lib)):
                for shape, rec in run_child(lib)["shapes"].items():
                    runs.setdefault(shape, {"other": [], "this": []})[side].append(rec["median_ms"])
        out = {"what": "train_regressor per fit, two library builds, alternating processes", "reps": args.reps,
               "other_lib": args.ab_lib, "this_lib": os.path.relpath(this_lib, REPO), "median_ms_per_process": runs,
               "this_over_other": {shape: statistics.median(r["this"]) / statistics.median(r["other"])
                                   for shape, r in runs.items()}}
        name = args.out_name or "regress_ab.json"
    else:
        out = {"what": "train_regressor (exact variance histograms) per fit, and scikit-learn on the same host",
               "depth": DEPTH, "max_bins": 32, "gpu": run_child(None), "sklearn_host": sklearn_fit()}
        name = "bench.json"
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, name), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
