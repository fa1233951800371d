"""Pair-boundary timing of the wide density Gram (gram_csym_kernel<128, 8, 4>):
a timing-only build (scripts/patches/stamp_gram_pair.patch through
scripts/variant_build.py; the product source carries no stamp) records, for
wave 0 of every block (or, built with -DDAL_STAMP_WAVE=4, its SIMD partner,
which runs its look-ahead later in the pair) and its first 2,048 acting pairs, s_memtime when the
pair's first B fragment has landed (c), behind the pair's barrier (b) and
behind its last MFMA issue (a).  After >= 2.5 s of back-to-back launches on
the workload's data one more launch is stamped.  Over records of consecutive
pairs of a block:
  gap    = c[i + 1] - a[i]   last MFMA issue of a pair -> first MFMA of the next
  drain  = b[i + 1] - a[i]   ... of which up to the barrier's release (the fold)
  period = c[i + 1] - c[i]   pair start -> pair start
in shader cycles, p10 / p50 / p90, for every boundary and for those without /
with an A reload between; the in-kernel clock as scripts/clock_probe.py.

usage: python scripts/gram_pair_stamps.py LIB.so NxD[:normal] [NxD ...]"""
import ctypes
import json
import os
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "distributed-active-learning_amd"))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from dal import _lib  # noqa: E402
from clock_probe import bind, stamped  # noqa: E402


def pct(v):
    return [round(float(np.percentile(v, q)), 1) for q in (10, 50, 90)] if len(v) else None


def boundaries(rec):
    """rec [G, N, 4] -> per boundary between consecutive pairs of a block:
    gap, drain, period, reload flag of the later pair."""
    c, b, a = (rec[:, :, k].astype(np.int64) for k in range(3))
    seq = (rec[:, :, 3] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    reload = (rec[:, :, 3] >> np.uint64(32)).astype(np.int64)
    ok = (c[:, :-1] > 0) & (c[:, 1:] > 0) & (seq[:, 1:] == seq[:, :-1] + 1) & (c[:, 1:] > a[:, :-1])
    gap = (c[:, 1:] - a[:, :-1])[ok]
    drain = (b[:, 1:] - a[:, :-1])[ok]
    period = (c[:, 1:] - c[:, :-1])[ok]
    return gap, drain, period, reload[:, 1:][ok]


def main():
    path = sys.argv[1]
    lib = bind(path if os.path.isabs(path) else os.path.join(REPO, path))
    lib.dal_diag_stamp_read.restype = ctypes.c_int
    lib.dal_diag_stamp_read.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    n_st, g_st = ctypes.c_int(), ctypes.c_int()
    assert lib.dal_diag_stamp_dims(ctypes.byref(n_st), ctypes.byref(g_st)) == 0
    n_st, g_st = n_st.value, g_st.value
    _lib._lib = lib
    dev = torch.device("cuda:0")
    from dal.engine import PoolState

    for spec in sys.argv[2:]:
        parts = spec.split(":")
        n, d = (int(v) for v in parts[0].split("x"))
        x = bench.upload(bench.host_pool(0, n, d, parts[1] if len(parts) > 1 else "uniform"), dev)
        st = PoolState(x, excluded=np.arange(bench.N_EXCLUDED), device=dev)
        op = st.gram_operand()
        acc = torch.zeros(st.n_pad, dtype=torch.int64, device=dev)

        def launch():
            st.gram_accumulate(acc, op, st.n_pad)

        r = stamped(lib, launch, 16384)  # warm, 10 timed launches, the clock of the last
        assert lib.dal_diag_clock_clear() == 0  # (clears the pair stamps too)
        launch()
        torch.cuda.synchronize()
        buf = np.zeros(4 * n_st * g_st, dtype=np.uint64)
        assert lib.dal_diag_stamp_read(buf.ctypes.data, buf.size) == 0
        gap, drain, period, reload = boundaries(buf.reshape(g_st, n_st, 4))
        out = {"shape": spec, "launch_ms": round(r["launch_ms"], 3), "clock_ghz_median": round(r["clock_ghz_median"], 4),
               "clock_ghz_p10": round(r["clock_ghz_p10"], 4), "clock_ghz_p90": round(r["clock_ghz_p90"], 4),
               "blocks": r["blocks"], "boundaries": int(gap.size)}
        for name, m in (("all", np.ones_like(reload, dtype=bool)), ("same_rows", reload == 0),
                        ("a_reload", reload == 1)):
            out[name] = {"count": int(m.sum()), "gap_p10_p50_p90": pct(gap[m]), "drain_p10_p50_p90": pct(drain[m]),
                         "period_p10_p50_p90": pct(period[m])}
        if gap.size:
            out["median_gap_over_median_period"] = round(float(np.median(gap) / np.median(period)), 4)
            out["sum_gap_over_sum_period"] = round(float(gap.sum() / period.sum()), 4)
        print(json.dumps(out), flush=True)
        del st, x, op, acc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
