#!/usr/bin/env python3
"""The exact StandardScaler (dal.dataset, csrc/scaler.hip) next to torch's fp64
path on the same GPU in the same process, and numpy on 16 host threads.

Shapes (rows x features): 2,000,000 x 256 (the flagship pool), 284,807 x 30 and
1,000 x 2 (the reference's checkerboard split).  Rows are U[0,1) fp32 from a
seeded generator on the device.

Timed, after WARMUP untimed runs, as the median of REPS runs with [min, max]:
  fit            wall clock around StandardScaler.fit, which ends in the host
                 finish (two syncs: the format words, then the cells)
  format, accumulate, transform_f32, transform_f64
                 each call alone between two device events
  torch_fit      torch.var_mean(x.double(), 0, unbiased=True) + sqrt, synchronised
  torch_transform_f32
                 ((x.double() - mean) * (1 / std)).float(), synchronised
  numpy          two-pass fp64 mean / std(ddof=1) over 16 row blocks on 16
                 host threads, and the same transform (one run at the large shape)
HBM fractions are bytes the algorithm needs (n d 4 per pass of the fit; 8 or 12
per element of the transform) over the event time, against the 8.0 TB/s peak.
Nothing is asserted; the numbers go to profiles/scaler/bench.json.

    python scripts/bench_scaler.py [--reps 10] [--out profiles/scaler]
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "distributed-active-learning_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = ((2_000_000, 256), (284_807, 30), (1_000, 2))
WARMUP = 2
HBM_PEAK = 8.0e12
HOST_THREADS = 16


def _summary(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": len(ts)}


def _events(torch, fn, reps):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return _summary(ts)


def _wall(torch, fn, reps):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return _summary(ts)


def _numpy_host(x, reps):
    import numpy as np

    n = x.shape[0]
    cuts = [n * i // HOST_THREADS for i in range(HOST_THREADS + 1)]
    blocks = [x[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]

    def fit(pool):
        s = sum(pool.map(lambda b: b.sum(axis=0, dtype=np.float64), blocks))
        mean = s / n
        ss = sum(pool.map(lambda b: ((b.astype(np.float64) - mean) ** 2).sum(axis=0), blocks))
        return mean, np.sqrt(ss / max(n - 1, 1))

    def transform(pool, mean, std):
        f = 1.0 / std
        return list(pool.map(lambda b: ((b.astype(np.float64) - mean) * f).astype(np.float32), blocks))

    with ThreadPoolExecutor(HOST_THREADS) as pool:
        tf, tt = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            mean, std = fit(pool)
            tf.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            transform(pool, mean, std)
            tt.append((time.perf_counter() - t0) * 1e3)
    return {"threads": HOST_THREADS, "fit": _summary(tf), "transform_f32": _summary(tt)}, mean, std


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scaler"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from dal import dataset as ds

    assert torch.cuda.is_available(), "bench_scaler.py needs a GPU"
    dev = torch.device("cuda:0")
    out = {"what": "exact StandardScaler fit / transform, torch fp64 on the same GPU, numpy on host threads",
           "device": torch.cuda.get_device_name(dev), "reps": args.reps, "warmup": WARMUP, "shapes": {}}
    for n, d in SHAPES:
        g = torch.Generator(device=dev).manual_seed(n + d)
        x = torch.rand((n, d), dtype=torch.float32, device=dev, generator=g)
        scaler = ds.StandardScaler()
        model = scaler.fit(x)
        low, top, status = ds.device_format(x, n, d, d)
        k1, k2, q = ds.check_format(low.cpu().numpy(), top.cpu().numpy(), status.item())
        q_dev = torch.from_numpy(q).to(dev)
        cells = torch.zeros((d, k1 + k2), dtype=torch.int64, device=dev)
        rec = {"k1": k1, "k2": k2, "fit_wall": _wall(torch, lambda: scaler.fit(x), args.reps)}
        rec["format"] = _events(torch, lambda: ds.device_format(x, n, d, d), args.reps)
        rec["accumulate"] = _events(torch, lambda: ds.device_accumulate(x, n, d, d, q_dev, k1, k2, cells=cells),
                                    args.reps)
        rec["transform_f32"] = _events(torch, lambda: model.transform(x), args.reps)
        rec["transform_f64"] = _events(torch, lambda: model.transform(x, dtype=np.float64), args.reps)
        for name, per_el in (("format", 4), ("accumulate", 4), ("transform_f32", 8), ("transform_f64", 12)):
            t = rec[name]["median_ms"] * 1e-3
            rec[name]["bytes"] = n * d * per_el
            rec[name]["tb_per_s"] = n * d * per_el / t / 1e12
            rec[name]["hbm_fraction"] = n * d * per_el / t / HBM_PEAK

        def torch_fit():
            var, mean = torch.var_mean(x.double(), dim=0, unbiased=True)
            return mean, var.sqrt()

        tm, tsd = torch_fit()
        rec["torch_fit"] = _wall(torch, torch_fit, args.reps)
        rec["torch_transform_f32"] = _wall(torch, lambda: ((x.double() - tm) * (1.0 / tsd)).float(), args.reps)
        rec["torch_vs_exact"] = {"max_abs_mean_diff": float((tm.cpu() - torch.from_numpy(model.mean)).abs().max()),
                                 "max_abs_std_diff": float((tsd.cpu() - torch.from_numpy(model.std)).abs().max())}
        host, hm, hs = _numpy_host(x.cpu().numpy(), 1 if n * d > 10_000_000 else 3)
        rec["numpy_host"] = host
        rec["numpy_vs_exact"] = {"max_abs_mean_diff": float(np.abs(hm - model.mean).max()),
                                 "max_abs_std_diff": float(np.abs(hs - model.std).max())}
        out["shapes"][f"{n}x{d}"] = rec
        del x, cells
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench.json"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
