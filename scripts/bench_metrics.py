#!/usr/bin/env python3
"""Test-set evaluation: the fused dal_forest_evaluate beside what the library
offered before it, and the share of the two squared-error kernels in
mean_squared_error -- one process per part, the variants of a part alternating.

Part "evaluate" (device spans, HIP events behind a queued GPU spin; the blocked
copy and the prepared forest are built beforehand), per shape:

  fused        dal_forest_evaluate over the blocked copy: the joint table, no
               per-row store
  fused_no_rows  the same call with row flags that count no row: every walk
               runs, no cell is occupied, so no block issues a global atomic
               (what the tables' flush costs)
  score        dal_forest_score_blocked alone: votes, scores and keys, 20 B
               stored per row
  score_hist   dal_forest_score_blocked, then dal_vote_histogram of its votes:
               the composition the library already offered (a vote histogram,
               not yet the joint table)
  host_path    host wall of run_loop's accuracy: random_forest.predict, the
               download, 1 - mean(pred != y) in NumPy

  shapes       2,000,000 x 256 at T = 10 and T = 100; 284,807 x 30 at T = 100,
               and four times those rows (which part of a difference is a cost
               per launch and which a cost per row) -- depth-4 forests, random
               labels
  hbm          the fused kernel's fraction of the HBM peak over the bytes it
               must read: rows x (4 B x distinct tested features + 1 label byte)

Part "mse" (2,000,000 x 5 fp32 rows, a 2,000-tree depth-4 regressor):
dal_forest_regress, dal_sq_error_format and dal_sq_error_accumulate, device
spans, and the two new kernels' share of the three.

Medians, interquartile ranges and every sample go to
profiles/metrics/<part>.json; without --part each part runs in a fresh child
process under its own time limit, and the run stops at the first child that
fails.

    python scripts/bench_metrics.py [--part evaluate|mse] [--rounds 30] [--out DIR]
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

PARTS = ("evaluate", "mse")
DEPTH, WARMUPS, CHILD_TIMEOUT_S = 4, 3, 420
SHAPES = ((2_000_000, 256, 10), (2_000_000, 256, 100), (284_807, 30, 100), (4 * 284_807, 30, 100))
HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X HBM3E, specification
MSE_ROWS, MSE_TREES = 2_000_000, 2000


def _stats(samples):
    q = statistics.quantiles(samples, n=4)
    return {"median": statistics.median(samples), "min": min(samples), "iqr": q[2] - q[0], "samples": samples}


def _alternate(rounds, variants, timed):
    """WARMUPS of every variant, then ``rounds`` rounds of one timed run each."""
    for _ in range(WARMUPS):
        for fn in variants.values():
            fn()
    out = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            out[name].append(timed(fn))
    return out


def _span(torch, dev, lead_cycles=600_000):
    """The device span of fn's launches: a GPU spin is queued first, so that
    they are all submitted before the GPU reaches the start event."""
    def span(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(lead_cycles)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) * 1e3
    return span


def run_evaluate(rounds: int, out_dir: str) -> dict:
    import numpy as np
    import torch

    from dal import _lib, engine, metrics
    from dal import random_forest as rf
    from dal.engine import _ptr, _stream
    from dal.forest import Forest

    dev = torch.device("cuda:0")
    lib = _lib.load()
    span = _span(torch, dev)
    shapes = {}
    state = None
    for n, d, T in SHAPES:
        if state is None or (state.n, state.d) != (n, d):
            state = None  # (free the previous pool first)
            gen = torch.Generator(device=dev).manual_seed(0)
            state = engine.PoolState(torch.rand((n, d), generator=gen, device=dev, dtype=torch.float32), device=dev)
        forest = Forest.synthetic(T, DEPTH, d, seed=1)
        if not lib.dal_forest_evaluate_blocked_rows(d, T, DEPTH, 2):
            raise SystemExit(f"{n} x {d}, T = {T}: the blocked rule does not hold")
        xb = state.blocked_pool(forest)
        prep = forest.blocked_prep(dev, d)
        if xb is None or prep is None:
            raise SystemExit(f"{n} x {d}, T = {T}: no blocked copy")
        y = np.random.default_rng(2).integers(0, 2, n).astype(np.uint8)
        labels = torch.from_numpy(y).to(dev)
        inner, leaf = forest.device(dev)
        lut = engine.device_lut("least_confidence", T, dev)
        hist = torch.zeros((T + 1, 2), dtype=torch.int64, device=dev)
        vhist = torch.zeros(T + 1, dtype=torch.int64, device=dev)
        votes = torch.empty(n, dtype=torch.int32, device=dev)
        scores = torch.empty(n, dtype=torch.float64, device=dev)
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        S = _stream(dev)

        def fused():
            _lib.call("dal_forest_evaluate", _ptr(state.x), _ptr(xb), _ptr(prep), n, d, d, _ptr(inner), _ptr(leaf), T,
                      DEPTH, 2, _ptr(labels), 0, _ptr(hist), S)

        no_rows = torch.zeros(n, dtype=torch.uint8, device=dev)

        def fused_no_rows():
            _lib.call("dal_forest_evaluate", _ptr(state.x), _ptr(xb), _ptr(prep), n, d, d, _ptr(inner), _ptr(leaf), T,
                      DEPTH, 2, _ptr(labels), _ptr(no_rows), _ptr(hist), S)

        def score():
            _lib.call("dal_forest_score_blocked", _ptr(state.x), _ptr(xb), _ptr(prep), n, d, d, _ptr(inner),
                      _ptr(leaf), T, DEPTH, _ptr(lut), 0, _lib.DAL_DENSITY_NONE, 0.0, 0, 1.0, _lib.DAL_ASCENDING,
                      _ptr(votes), _ptr(scores), _ptr(keys), 0, S)

        def score_hist():
            score()
            _lib.call("dal_vote_histogram", _ptr(votes), 0, n, T, _ptr(vhist), S)

        last = {}

        def host_path():
            pred, _ = rf.predict(forest, state)
            last["acc"] = (1 - np.mean(pred.cpu().numpy() != y)) * 100

        def wall(fn):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e6

        # one checked call first: the fused table gives run_loop's accuracy
        hist.zero_()
        fused()
        host_path()
        m = metrics.finish(hist.cpu().numpy(), T, 2, ("accuracy", "auc"))
        if abs(m["accuracy"] * 100 - last["acc"]) > 1e-9:
            raise SystemExit(f"{n} x {d}, T = {T}: accuracy {m['accuracy'] * 100} vs {last['acc']}")
        us = _alternate(rounds, {"fused": fused, "fused_no_rows": fused_no_rows, "score": score,
                                 "score_hist": score_hist}, span)
        host = _alternate(rounds, {"host_path": host_path}, wall)
        D = {k: _stats(v) for k, v in us.items()}
        D["host_path"] = _stats(host["host_path"])
        fu = int(prep[:4].view(torch.int32).item())
        must_read = n * (4 * fu + 1)
        shapes[f"{n}x{d}_T{T}"] = {
            "rows": n, "features": d, "trees": T, "tested_features": fu, "us": D,
            "fused_over_score": D["fused"]["median"] / D["score"]["median"],
            "bytes_must_read": must_read,
            "fused_hbm_fraction": must_read / (D["fused"]["median"] * 1e-6) / HBM_PEAK_BYTES_PER_S,
            "accuracy": m["accuracy"], "auc": m["auc"]}
    res = {"part": "evaluate", "device": torch.cuda.get_device_name(dev), "rounds": rounds, "warmups": WARMUPS,
           "depth": DEPTH, "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "shapes": shapes}
    _write(res, out_dir, "evaluate")
    print(json.dumps({"part": "evaluate",
                      "us": {k: {v: [round(s["us"][v]["median"], 1), round(s["us"][v]["iqr"], 1)] for v in s["us"]}
                             for k, s in shapes.items()},
                      "fused_hbm_fraction": {k: round(s["fused_hbm_fraction"], 3) for k, s in shapes.items()}}),
          flush=True)
    return res


def run_mse(rounds: int, out_dir: str) -> dict:
    import numpy as np
    import torch

    from dal import _lib, metrics
    from dal.engine import _ptr, _stream
    from dal.forest import RegressionForest

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    model = RegressionForest.synthetic(MSE_TREES, DEPTH, 5, seed=1)
    x = torch.rand((MSE_ROWS, 5), generator=gen, device=dev, dtype=torch.float32)
    y = torch.randn(MSE_ROWS, generator=gen, device=dev, dtype=torch.float64)
    feat, thr, leaf = model.device(dev)
    pred = torch.empty(MSE_ROWS, dtype=torch.float64, device=dev)
    S = _stream(dev)

    def regress():
        _lib.call("dal_forest_regress", _ptr(x), _lib.DAL_X_F32, MSE_ROWS, 5, 5, _ptr(feat), _ptr(thr), _ptr(leaf),
                  model.n_trees, model.depth, _ptr(pred), S)

    regress()
    words, q = metrics.sq_error_cells(pred, y)
    k = len(words)
    fmt = torch.tensor([np.iinfo(np.int32).max, np.iinfo(np.int32).min, 0], dtype=torch.int32, device=dev)
    cells = torch.zeros(k, dtype=torch.int64, device=dev)

    def sq_format():
        _lib.call("dal_sq_error_format", _ptr(pred), _ptr(y), MSE_ROWS, fmt.data_ptr(), fmt.data_ptr() + 4,
                  fmt.data_ptr() + 8, S)

    def sq_accumulate():
        _lib.call("dal_sq_error_accumulate", _ptr(pred), _ptr(y), MSE_ROWS, q, k, _ptr(cells), S)

    us = _alternate(rounds, {"regress": regress, "sq_format": sq_format, "sq_accumulate": sq_accumulate},
                    _span(torch, dev))
    D = {name: _stats(v) for name, v in us.items()}
    new = D["sq_format"]["median"] + D["sq_accumulate"]["median"]
    res = {"part": "mse", "device": torch.cuda.get_device_name(dev), "rounds": rounds, "warmups": WARMUPS,
           "rows": MSE_ROWS, "features": 5, "trees": MSE_TREES, "depth": DEPTH, "limbs": k, "quantum_exponent": q,
           "mse": metrics.mse_from_cells(words, q, MSE_ROWS), "device_span_us": D,
           "new_kernels_share": new / (new + D["regress"]["median"])}
    _write(res, out_dir, "mse")
    print(json.dumps({"part": "mse", "device_span_us": {n: [round(v["median"], 1), round(v["iqr"], 1)]
                                                        for n, v in D.items()},
                      "new_kernels_share": round(res["new_kernels_share"], 4)}), flush=True)
    return res


def _write(res, out_dir, name):
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"{name}.json"), "w") as f:
        json.dump(res, f, indent=1)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--part", choices=PARTS)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "metrics"))
    a = ap.parse_args()
    if a.rounds < 30:
        ap.error("--rounds must be at least 30")
    runners = {"evaluate": run_evaluate, "mse": run_mse}
    if a.part is not None:
        runners[a.part](a.rounds, a.out)
        return 0
    for part in PARTS:
        # a fresh process per part, each under its own time limit; nothing
        # more is started on the GPU after a child fails or runs out of time
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part, "--rounds",
                                 str(a.rounds), "--out", a.out], timeout=CHILD_TIMEOUT_S).returncode
        except subprocess.TimeoutExpired:
            print(f"part {part}: no result within {CHILD_TIMEOUT_S} s; stopping", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"part {part}: exit status {rc}; stopping", file=sys.stderr)
            return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
