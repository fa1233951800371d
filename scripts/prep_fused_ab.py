"""A/B of the fp4 form's preparation: the separate entries (dal_prep_split with
partials, dal_quant_fp4, and launch 1 of dal_gram_sym_residual_fp4, timed as the
difference between that entry and dal_gram_sym_residual_fp4_pre) against the
one-pass dal_prep_split_fp4, in one process, interleaved, per pool size.

    python scripts/prep_fused_ab.py [ROWSxFEATURES ...] [--reps 7] [--lib ab/NAME/libdal.so]

Prints one line per shape: medians [min, max] in ms of
  split    dal_prep_split (two launches)
  quant    dal_quant_fp4
  res      dal_gram_sym_residual_fp4 (memset, sigma, scan, rows)
  res_pre  dal_gram_sym_residual_fp4_pre (scan, rows)
  fused    dal_prep_split_fp4 (two launches)
and separate = split + quant + (res - res_pre) against fused.  Outputs of the
two paths are compared once per shape (operand, codes, partials, accumulator)."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "distributed-active-learning_amd"))


def main():
    import torch

    from dal import _lib
    from dal.engine import workspace

    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["36000x256", "131072x256", "262144x256", "524288x256",
                                                  "1000000x256", "2000000x256"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lib", default=None, help="another build of libdal.so (scripts/ab_build.sh)")
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
        print(f"lib {a.lib}")
    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev).cuda_stream
    for shape in a.shapes:
        n, d = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.rand((n, d), dtype=torch.float32, device=dev, generator=g)
        n_pad, d_pad = int(lib.dal_pad_rows(n)), int(lib.dal_pad_features(d))
        nb, chunks = n_pad // 256, (n + 255) // 256
        flags = torch.zeros(n, dtype=torch.uint8, device=dev)
        flags[:10] = _lib.DAL_ROW_EXCLUDED
        status = torch.zeros(1, dtype=torch.int32, device=dev)

        def bufs():
            return dict(ops=torch.empty((n_pad, 2 * d_pad), dtype=torch.int16, device=dev),
                        norm=torch.empty(n, dtype=torch.float64, device=dev),
                        parts=torch.empty((chunks, d), dtype=torch.float64, device=dev),
                        acc=torch.empty(n_pad, dtype=torch.int64, device=dev),
                        codes=torch.empty((n_pad, d_pad // 2), dtype=torch.uint8, device=dev))

        A, B = bufs(), bufs()
        sig = torch.empty((n_pad // 512, d_pad), dtype=torch.int64, device=dev)
        s_l = torch.empty(d_pad, dtype=torch.int64, device=dev)
        rb = int(lib.dal_gram_sym_residual_workspace_bytes(nb, nb, d_pad))
        rws, rwsp = workspace(rb, dev)
        pb = int(lib.dal_prep_split_fp4_workspace_bytes(n_pad, d_pad))
        pws, pwsp = workspace(pb, dev)
        p = lambda t: t.data_ptr()  # noqa: E731
        calls = {
            "split": lambda: _lib.call("dal_prep_split", p(x), n, d, d, p(flags), n_pad, d_pad, p(A["ops"]),
                                       p(A["norm"]), p(A["parts"]), p(A["acc"]), p(status), stream),
            "quant": lambda: _lib.call("dal_quant_fp4", p(A["ops"]), n_pad, d_pad, p(A["codes"]), stream),
            "res": lambda: _lib.call("dal_gram_sym_residual_fp4", p(A["ops"]), nb, 0, nb, d_pad, p(A["acc"]), rwsp, rb,
                                     stream),
            "fused": lambda: _lib.call("dal_prep_split_fp4", p(x), n, d, d, p(flags), n_pad, d_pad, p(B["ops"]),
                                       p(B["norm"]), p(B["parts"]), p(B["acc"]), p(B["codes"]), p(sig), p(s_l), pwsp,
                                       pb, p(status), stream),
            "res_pre": lambda: _lib.call("dal_gram_sym_residual_fp4_pre", p(B["ops"]), nb, 0, nb, d_pad, p(B["acc"]),
                                         p(sig), p(s_l), rwsp, rb, stream),
        }
        order = ["split", "quant", "res", "fused", "res_pre"]
        for name in order:  # warm up, and the one comparison
            calls[name]()
        torch.cuda.synchronize(dev)
        same = all(torch.equal(A[k], B[k]) for k in ("ops", "codes", "acc")) and \
            A["parts"].cpu().numpy().tobytes() == B["parts"].cpu().numpy().tobytes()
        ms = {name: [] for name in order}
        for _ in range(a.reps):
            for name in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                calls[name]()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        med = {k: statistics.median(v) for k, v in ms.items()}
        sep = med["split"] + med["quant"] + med["res"] - med["res_pre"]
        cells = "  ".join(f"{k} {med[k]:.4f} [{min(ms[k]):.4f}, {max(ms[k]):.4f}]" for k in order)
        print(f"{n} x {d} ({chunks} chunks): {cells}  separate {sep:.4f}  fused {med['fused']:.4f}  "
              f"same_bytes {same}", flush=True)
        del A, B, x, sig, rws, pws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
