#!/usr/bin/env python3
"""C-class GPU forest training against the binary fit: same rows, same bagging
draws, one process.

Shape: bench.py's bench_rf_train (5,000 x 64 labeled rows, T = 10, depth 4,
32 bins, sqrt features).  Timed per fit, wall clock around
dal.random_forest.train_classifier (host draws excluded: weights and subsets
are passed in; the forest's copy back included), synchronised after each fit:

  binary   train_classifier(num_classes=2)   dal_rf_train, the yardstick
  C = 3, 10, 32                              dal_rf_train_multiclass, labels
           min(floor(x0 * C) + (x1 > 0.8), C - 1) with 10 % relabelled uniformly

The variants run interleaved, ROUNDS rounds of REPS fits each after a warm-up;
per variant the median of each round is kept, and the report gives the median
of those medians, their [min, max] and (max - min) / median as the run-to-run
spread, then each C-class median over the binary one next to the model's C / 2
(histogram and prefix-sum volume; the launches per level are the same).

The GPU part runs in one child process under its own time limit; the
scikit-learn fit of the same shape is timed on the host in the parent, with
the core count it used.

--ab-lib PATH   time only the binary fit with the library at PATH (a build of
                an older commit: scripts/ab_build.sh in that checkout) and with
                this tree's, in alternating child processes, ALTERNATIONS each.
                With --lib PATH2 the second side is the library at PATH2
                instead of this tree's (PATH against itself: the spread of
                the measurement).  With --ab-all the C-class fits are timed
                on both sides as well.
--n ROWS        labeled rows instead of 5,000 (200,000: the histogram kernel
                is no longer launch-bound).

    python scripts/bench_rf_multiclass.py [--rounds 5] [--reps 20] [--n ROWS] [--out DIR] [--ab-lib PATH [--lib PATH2]]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "distributed-active-learning_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

N, D, TREES, DEPTH = 5000, 64, 10, 4
CLASSES = (3, 10, 32)
CHILD_TIMEOUT_S, ALTERNATIONS = 240, 3


def _rows():
    import numpy as np

    rng = np.random.default_rng(7)
    X = rng.random((N, D), dtype=np.float32)
    y2 = (X[:, : D // 8].sum(axis=1) > D // 16).astype(np.int64)  # bench_rf_train's labels
    ys = {2: y2}
    for C in CLASSES:
        y = np.minimum(np.floor(X[:, 0] * C).astype(np.int64) + (X[:, 1] > 0.8), C - 1)
        noisy = rng.random(N) < 0.1
        y[noisy] = rng.integers(0, C, int(noisy.sum()))
        ys[C] = y
    return X, ys


def _summary(round_medians):
    med = statistics.median(round_medians)
    lo, hi = min(round_medians), max(round_medians)
    return {"median_ms": med, "min_ms": lo, "max_ms": hi, "spread": (hi - lo) / med, "round_medians_ms": round_medians}


def child(rounds: int, reps: int, lib_path, variants) -> dict:
    import torch

    from dal import _lib

    if lib_path:  # another build: keep the symbols it has (an older one lacks the C-class entries)
        import ctypes

        _lib.LIB_PATH = os.path.abspath(lib_path)
        probe = ctypes.CDLL(_lib.LIB_PATH)
        for missing in [name for name in _lib.SIGNATURES if not hasattr(probe, name)]:
            del _lib.SIGNATURES[missing]
    from dal.random_forest import bagging_inputs, train_classifier

    dev = torch.device("cuda:0")
    X, ys = _rows()
    w, s = bagging_inputs(N, D, TREES, DEPTH, seed=1)
    xd = torch.from_numpy(X).to(dev)

    def fit(C):
        kw = {} if C == 2 else {"num_classes": C}
        return train_classifier(xd, ys[C], TREES, max_depth=DEPTH, weights=w, feature_subsets=s, device=dev, **kw)

    for C in variants:
        for _ in range(3):
            fit(C)
    torch.cuda.synchronize()
    per_round = {C: [] for C in variants}
    for _ in range(rounds):
        for C in variants:
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fit(C)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            per_round[C].append(statistics.median(ts))
    out = {"device": torch.cuda.get_device_name(dev), "lib": os.path.relpath(_lib.LIB_PATH, REPO), "rounds": rounds, "reps": reps,
           "fits": {("binary" if C == 2 else f"C{C}"): _summary(per_round[C]) for C in variants}}
    base = out["fits"].get("binary")
    if base:
        for C in variants:
            if C != 2:
                f = out["fits"][f"C{C}"]
                f["ratio_to_binary"] = f["median_ms"] / base["median_ms"]
                f["model_C_over_2"] = C / 2
    return out


def run_child(args, lib_path=None, binary_only=False) -> dict:
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(args.rounds), "--reps",
           str(args.reps), "--n", str(N)]
    if lib_path:
        cmd += ["--lib", lib_path]
    if binary_only:
        cmd += ["--binary-only"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    if res.returncode != 0:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        raise SystemExit(f"child failed with status {res.returncode}")
    return json.loads(res.stdout.strip().splitlines()[-1])


def sklearn_fit() -> dict:
    from sklearn.ensemble import RandomForestClassifier

    X, ys = _rows()
    cores = min(16, len(os.sched_getaffinity(0)))
    out = {"cores": cores}
    for C in (2,) + CLASSES:
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            RandomForestClassifier(n_estimators=TREES, max_depth=DEPTH, max_features="sqrt", bootstrap=True,
                                   random_state=0, n_jobs=cores).fit(X, ys[C])
            ts.append((time.perf_counter() - t0) * 1e3)
        out["binary" if C == 2 else f"C{C}"] = {"median_ms": statistics.median(ts)}
    return out


def main():
    global N
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab-lib", default=None)
    ap.add_argument("--out-name", default=None)
    ap.add_argument("--ab-all", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--binary-only", action="store_true")
    ap.add_argument("--n", type=int, default=N)
    args = ap.parse_args()
    N = args.n
    if args.child:
        print(json.dumps(child(args.rounds, args.reps, args.lib, (2,) if args.binary_only else (2,) + CLASSES)))
        return
    shape = f"{N} x {D} labeled rows, T={TREES}, depth {DEPTH}, 32 bins, sqrt features"
    if args.ab_lib:
        sides = (("other", args.ab_lib), ("this", args.lib))
        runs = {}
        for _ in range(ALTERNATIONS):  # a failed child ends the run: nothing more is started
            for side, lib in sides:
                for fit, rec in run_child(args, lib, not args.ab_all)["fits"].items():
                    runs.setdefault(fit, {"other": [], "this": []})[side].append(rec["median_ms"])
        ratio = {fit: statistics.median(r["this"]) / statistics.median(r["other"]) for fit, r in runs.items()}
        out = {"what": "fits per entry (binary: dal_rf_train), two library builds, alternating processes",
               "shape": shape, "other_lib": args.ab_lib, "this_lib": args.lib or "this tree's",
               "median_ms_per_process": runs, "this_over_other": ratio}
        name = args.out_name or "binary_ab.json"
    else:
        out = {"what": "C-class fit against the binary fit, one process", "shape": shape, "gpu": run_child(args),
               "sklearn_host": sklearn_fit()}
        name = "fit_ratios.json"
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, name), "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
