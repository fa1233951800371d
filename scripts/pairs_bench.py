"""Thresholded cosine pairs (column_similarities(threshold=)) at pool scale:
filter, resolve and end-to-end times against the density Gram on the same
PoolState in the same process.

One process, HIP events, one warm-up, medians of 5 rounds with min-max.  Per
shape tau = mean + 5 sd of the cosine over a CPU sample of 10^6 random pairs (a
selective threshold, the intended use).  The yardstick is the density Gram's
MFMA launches (PoolState.gram_accumulate: gram_csym_kernel, the same H.H
products on the same number of block pairs with a row-sum epilogue),
alternated with the filter round by round; the filter / Gram ratio is what
the threshold epilogue and the K-loop structure cost.

usage: python scripts/pairs_bench.py [--out FILE.json] [--dense N] [NxD ...]
       (d = 30: config 3's N(0,1) pool; default shapes: the benchmark
       configs' pools; --dense N: also time the dense path at N x 64, 0 = skip)"""
import json
import os
import statistics
import sys
import time

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "distributed-active-learning_amd"))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from dal import _lib  # noqa: E402
from dal import similarity as sim  # noqa: E402
from dal.engine import PoolState, _ptr, _stream  # noqa: E402

ROUNDS = 5
PEAK_F16 = 2.5e15  # dense fp16 MFMA flop/s of the device


def sample_threshold(xh, pairs=1_000_000, seed=1):
    """mean + 5 sd of the cosine over random pairs i != j (fp64, on the CPU)."""
    rng = np.random.default_rng(seed)
    n = xh.shape[0]
    vals = []
    for _ in range(10):
        i = rng.integers(0, n, pairs // 10)
        j = rng.integers(0, n, pairs // 10)
        keep = i != j
        a = xh[i[keep]].astype(np.float64)
        b = xh[j[keep]].astype(np.float64)
        vals.append(np.einsum("ij,ij->i", a, b) / np.sqrt(np.einsum("ij,ij->i", a, a) * np.einsum("ij,ij->i", b, b)))
    v = np.concatenate(vals)
    return float(v.mean() + 5.0 * v.std()), float(v.mean()), float(v.std())


def med(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run_shape(n, d, dev):
    dist = "normal" if d == 30 else "uniform"
    xh = bench.host_pool(0, n, d, dist)
    tau, mean, sd = sample_threshold(xh)
    st = PoolState(bench.upload(xh, dev), device=dev)
    op = st.gram_operand()
    st.check_status()
    nb = st.n_pad // 256

    # sizes from one call through the public entry point (also the warm-up)
    i, _, _ = sim.column_similarities(st, threshold=tau)
    kept = int(i.shape[0])
    cap = min(n * (n - 1) // 2, max(1 << 20, 8 * n))
    keys = torch.empty(cap, dtype=torch.int64, device=dev)
    approx = torch.empty(cap, dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    acc = torch.zeros(st.n_pad, dtype=torch.int64, device=dev)

    def filt():
        _lib.call("dal_cosine_pairs", _ptr(op), 0, nb, _ptr(op), 0, 0, nb, n, st.d_pad, 0, tau, cap, _ptr(keys),
                  _ptr(approx), _ptr(count), _ptr(status), _stream(dev))

    def gram():
        st.gram_accumulate(acc, op, st.n_pad)

    filt()
    gram()
    torch.cuda.synchronize()
    n_cand = int(count.item())
    if int(status.item()):
        cap = n_cand
        keys = torch.empty(cap, dtype=torch.int64, device=dev)
        approx = torch.empty(cap, dtype=torch.float32, device=dev)
    values = torch.empty(n_cand, dtype=torch.float64, device=dev)

    def resolve():
        if n_cand == 0:  # (nothing reached tau - bound)
            return
        _lib.call("dal_cosine_pairs_resolve", _ptr(st.x), n, d, d, _ptr(st.norms()), _ptr(keys), n_cand,
                  _ptr(values), _stream(dev))

    t_f, t_g, t_r, t_res, t_e2e = [], [], [], [], []
    for _ in range(ROUNDS):  # filter and Gram alternate
        count.zero_()
        status.zero_()
        t_f.append(timed(filt))
        acc.zero_()
        t_g.append(timed(gram))
        t_r.append(timed(resolve))
        acc.zero_()
        t_res.append(timed(lambda: st.gram_residual(acc, op)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sim.column_similarities(st, threshold=tau)
        torch.cuda.synchronize()
        t_e2e.append((time.perf_counter() - t0) * 1e3)
    flops = float(n) * n / 2.0 * st.d_pad * 2.0
    f, g = med(t_f), med(t_g)
    out = {
        "shape": f"{n}x{d}", "dist": dist, "d_pad": st.d_pad, "tau": tau, "sample_mean": mean, "sample_sd": sd,
        "candidates": n_cand, "kept": kept, "candidates_per_kept": n_cand / max(kept, 1),
        "filter": f, "gram_mfma": g, "gram_residual": med(t_res), "resolve": med(t_r), "end_to_end": med(t_e2e),
        "filter_fraction_of_f16_peak": flops / (f["median_ms"] * 1e-3) / PEAK_F16,
        "gram_fraction_of_f16_peak": flops / (g["median_ms"] * 1e-3) / PEAK_F16,
        "filter_over_gram": f["median_ms"] / g["median_ms"],
        "filter_over_gram_range": [min(a / b for a, b in zip(t_f, t_g)), max(a / b for a, b in zip(t_f, t_g))],
    }
    print(json.dumps(out), flush=True)
    return out


def run_dense(n, dev):
    """The "before": dense column_similarities(pool) + a torch filter, against
    the thresholded call.  Larger n is not comparable: the dense path's matrix
    and index arrays no longer fit (100,000 rows: 40 GB + 80 GB)."""
    xh = bench.host_pool(0, n, 64, "uniform")
    tau, _, _ = sample_threshold(xh)
    x = bench.upload(xh, dev)

    def dense():
        i, j, v = sim.column_similarities(x)
        keep = v >= tau
        return i[keep], j[keep], v[keep]

    def thresholded():
        return sim.column_similarities(x, threshold=tau)

    res = {}
    for name, fn in (("dense_then_filter", dense), ("thresholded", thresholded)):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(ROUNDS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        res[name] = med(ts)
        res[name + "_pairs"] = int(r[0].shape[0])
        del r
        torch.cuda.empty_cache()
    out = {"shape": f"{n}x64", "tau": tau, "note": "whole calls from a device array, pool preparation included", **res}
    print(json.dumps(out), flush=True)
    return out


def main():
    argv = sys.argv[1:]
    out_path, dense_n = None, 16384
    if "--out" in argv:
        k = argv.index("--out")
        out_path = argv[k + 1]
        del argv[k:k + 2]
    if "--dense" in argv:
        k = argv.index("--dense")
        dense_n = int(argv[k + 1])
        del argv[k:k + 2]
    shapes = argv or ["100000x64", "284807x30", "500000x256", "2000000x256"]
    dev = torch.device("cuda:0")
    results = {"device": torch.cuda.get_device_name(dev), "rounds": ROUNDS, "shapes": [], "dense": None}
    for sh in shapes:
        n, d = (int(v) for v in sh.split("x"))
        results["shapes"].append(run_shape(n, d, dev))
        torch.cuda.empty_cache()
    if dense_n:
        results["dense"] = run_dense(dense_n, dev)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
