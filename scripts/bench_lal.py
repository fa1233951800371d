#!/usr/bin/env python3
"""LAL query selection: the regression-forest kernel on its own, the LAL step
beside the uncertainty step it extends, and the kernel's node-visit rate
beside the binary blocked score kernel's -- one process per part, the variants
of a part alternating.

Part "regress" (device spans, HIP events behind a queued GPU spin):

  lal_lut       dal_forest_regress, 256 x 5 fp64 rows, 2,000 depth-4 trees: the
                LAL step's one-block launch (T + 1 <= 256 rows)
  pool          dal_forest_regress, 2,000,000 x 5 fp32 rows, 200 depth-4 trees:
                random_forest.predict_regression on a pool

Part "step" (the config-4 pool, 2,000,000 x 256 fp32, depth-4 forests, k = 10,
every row but the first 10 unlabeled; warm: the blocked copy is built):

  us / lal      host wall of uncertainty_sampling.select and of
                active_learner.select_lal (2,000-tree regressor) on the same
                PoolState, T = 10 and T = 50, the status read included
                (time.perf_counter around the call, which ends in a blocking
                read), and the device span of the same calls.  lal - us is
                what the histogram, rows, regress and rescore launches add.
  unchanged     uncertainty_sampling.select returns the same indices before
                and after the LAL steps ran on the pool
  visits        node visits per second (rows x trees x depth over the device
                span) of dal_forest_regress (2,000,000 x 5 fp32, 200 trees)
                and of dal_forest_score_blocked at T = 100 on the pool

Medians, interquartile ranges and every sample go to profiles/lal/<part>.json;
without --part each part runs in a fresh child process under its own time
limit, and the run stops at the first child that fails.

    python scripts/bench_lal.py [--part regress|step] [--rounds 30] [--out DIR]
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

PARTS = ("regress", "step")
DEPTH, K, WARMUPS, CHILD_TIMEOUT_S = 4, 10, 3, 420
LAL_TREES, POOL_TREES, POOL_ROWS = 2000, 200, 2_000_000


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


def _regress_call(torch, dev, model, x, f64):
    from dal import _lib
    from dal.engine import _ptr, _stream

    feat, thr, leaf = model.device(dev)
    n, d = int(x.shape[0]), int(x.shape[1])
    out = torch.empty(n, dtype=torch.float64, device=dev)

    def call():
        _lib.call("dal_forest_regress", _ptr(x), _lib.DAL_X_F64 if f64 else _lib.DAL_X_F32, n, d, d, _ptr(feat),
                  _ptr(thr), _ptr(leaf), model.n_trees, model.depth, _ptr(out), _stream(dev))
    return call, out


def run_regress(rounds: int, out_dir: str) -> dict:
    import torch

    from dal import _lib
    from dal.forest import RegressionForest

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lal_model = RegressionForest.synthetic(LAL_TREES, DEPTH, 5, seed=1)
    pool_model = RegressionForest.synthetic(POOL_TREES, DEPTH, 5, seed=2)
    x_lut = torch.rand((256, 5), generator=gen, device=dev, dtype=torch.float64)
    x_pool = torch.rand((POOL_ROWS, 5), generator=gen, device=dev, dtype=torch.float32)
    lal_lut, _ = _regress_call(torch, dev, lal_model, x_lut, True)
    pool, _ = _regress_call(torch, dev, pool_model, x_pool, False)
    us = _alternate(rounds, {"lal_lut": lal_lut, "pool": pool}, _span(torch, dev))
    D = {k: _stats(v) for k, v in us.items()}
    res = {"part": "regress", "device": torch.cuda.get_device_name(dev), "rounds": rounds, "warmups": WARMUPS,
           "depth": DEPTH, "chunk_trees": int(_lib.load().dal_forest_regress_chunk_trees(DEPTH)),
           "lal_lut": {"rows": 256, "features": 5, "dtype": "fp64", "trees": LAL_TREES},
           "pool": {"rows": POOL_ROWS, "features": 5, "dtype": "fp32", "trees": POOL_TREES},
           "device_span_us": D,
           "node_visits_per_s": {"lal_lut": 256 * LAL_TREES * DEPTH / (D["lal_lut"]["median"] * 1e-6),
                                 "pool": POOL_ROWS * POOL_TREES * DEPTH / (D["pool"]["median"] * 1e-6)}}
    _write(res, out_dir, "regress")
    print(json.dumps({"part": "regress",
                      "device_span_us": {k: [round(v["median"], 1), round(v["iqr"], 1)] for k, v in D.items()},
                      "node_visits_per_s": {k: float(f"{v:.3g}") for k, v in res["node_visits_per_s"].items()}}),
          flush=True)
    return res


def run_step(rounds: int, out_dir: str) -> dict:
    import torch

    from dal import _lib, engine
    from dal import uncertainty_sampling as us_mod
    from dal.active_learner import select_lal
    from dal.forest import Forest, RegressionForest

    dev = torch.device("cuda:0")
    n, d = POOL_ROWS, 256
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand((n, d), generator=gen, device=dev, dtype=torch.float32)
    state = engine.PoolState(x, device=dev)
    del x
    unl = torch.arange(10, n, dtype=torch.int64, device=dev)
    lal_model = RegressionForest.synthetic(LAL_TREES, DEPTH, 5, seed=1)
    # thresholds where the five features lie (f2 <= 0.71, f6 <= 0.5, f8 = 10), so the regressor's branches vary
    scale = {1: 0.7, 3: 0.5, 4: 20.0}
    for f, s in scale.items():
        lal_model.inner_threshold[lal_model.inner_feature == f] *= s
    span = _span(torch, dev)
    last = {}

    def wall(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        last[fn.__name__] = fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize(dev)
        return (t1 - t0) * 1e6

    steps = {}
    for T in (10, 50):
        forest = Forest.synthetic(T, DEPTH, d, seed=1)

        def us():
            return us_mod.select(state, unl, forest, K).indices

        def lal():
            return select_lal(state, unl, forest, lal_model, K, n_labeled=10, n_positive=4).indices

        before = us().cpu().tolist()
        us()  # the pool's second step builds the blocked copy: everything below is warm
        if state.blocked_pool(forest, build=False) is None:
            raise SystemExit(f"T = {T}: no blocked copy")
        host = _alternate(rounds, {"us": us, "lal": lal}, wall)
        device = _alternate(rounds, {"us": us, "lal": lal}, _span(torch, dev, 3_000_000))
        after = us().cpu().tolist()
        H = {k: _stats(v) for k, v in host.items()}
        Dv = {k: _stats(v) for k, v in device.items()}
        steps[f"T{T}"] = {"trees": T, "host_wall_us": H, "device_span_us": Dv,
                          "lal_minus_us_host_us": H["lal"]["median"] - H["us"]["median"],
                          "lal_minus_us_device_us": Dv["lal"]["median"] - Dv["us"]["median"],
                          "us_selection_unchanged": before == after,
                          "lal_selection": last["lal"].cpu().tolist()}
        if before != after:
            raise SystemExit(f"T = {T}: the uncertainty selection changed")

    # node visits per second: the regress kernel and the binary blocked kernel at T = 100
    T = 100
    forest = Forest.synthetic(T, DEPTH, d, seed=1)
    xb = state.blocked_pool(forest)
    if xb is None:
        raise SystemExit("T = 100: no blocked copy")
    flags = state.row_flags(unl)[0]
    lut = engine.device_lut("least_confidence", T, dev)

    def blocked():
        engine.forest_score(state, forest, lut, flags, _lib.DAL_ASCENDING, xb=xb)

    pool_model = RegressionForest.synthetic(POOL_TREES, DEPTH, 5, seed=2)
    x5 = torch.rand((n, 5), generator=gen, device=dev, dtype=torch.float32)
    regress, _ = _regress_call(torch, dev, pool_model, x5, False)
    vis = _alternate(rounds, {"regress": regress, "blocked": blocked}, span)
    V = {k: _stats(v) for k, v in vis.items()}
    visits = {"regress": {"rows": n, "trees": POOL_TREES, "depth": DEPTH, "device_span_us": V["regress"],
                          "node_visits_per_s": n * POOL_TREES * DEPTH / (V["regress"]["median"] * 1e-6)},
              "blocked": {"rows": n, "trees": T, "depth": DEPTH, "device_span_us": V["blocked"],
                          "node_visits_per_s": n * T * DEPTH / (V["blocked"]["median"] * 1e-6)}}
    res = {"part": "step", "device": torch.cuda.get_device_name(dev), "rounds": rounds, "warmups": WARMUPS,
           "rows": n, "features": d, "depth": DEPTH, "k": K, "lal_trees": LAL_TREES, "steps": steps, "visits": visits}
    _write(res, out_dir, "step")
    brief = {"part": "step"}
    for name, s in steps.items():
        brief[name] = {"host_us": {k: [round(v["median"], 1), round(v["iqr"], 1)] for k, v in s["host_wall_us"].items()},
                       "device_us": {k: [round(v["median"], 1), round(v["iqr"], 1)]
                                     for k, v in s["device_span_us"].items()},
                       "unchanged": s["us_selection_unchanged"]}
    brief["visits_per_s"] = {k: float(f"{v['node_visits_per_s']:.3g}") for k, v in visits.items()}
    print(json.dumps(brief), flush=True)
    return res


def _write(res, out_dir, name):
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"{name}.json"), "w") as f:
        json.dump(res, f, indent=1)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--part", choices=PARTS)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lal"))
    a = ap.parse_args()
    if a.rounds < 30:
        ap.error("--rounds must be at least 30")
    if a.part is not None:
        (run_regress if a.part == "regress" else run_step)(a.rounds, a.out)
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
