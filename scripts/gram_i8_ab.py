"""Same-process A/B of the density Gram call (gram_accumulate + gram_residual,
through PoolState) between the fp16 form (gram_i8=False: the kernels every
pool ran before round 13), the int8 form (gram_i8=True) and, where the pool's
rule picks it (d_pad a multiple of 256), the fp4 form (gram_fp4=True: round
14) of one library, in the style of scripts/gram_multi_ab.py: interleaved HIP-event timing of whole
calls, medians of AB_ROUNDS (5) with min and max; the two densities'
largest differences against the bound.  The int8 and fp4 calls include what
the form adds per cold step: the quantisation of the pool's operand
(dal_quant_i8, dal_quant_fp4).  AB_FORMS=i8,fp4 times a subset of the forms.
Shapes the rule leaves on the fp16 form (100000x64, 284807x30) are timed with
the default rule only, for the record that they run what they ran.

usage: python scripts/gram_i8_ab.py [NxD ...]   (d = 30: config 3's N(0,1) pool)"""
import os
import statistics
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "distributed-active-learning_amd"))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from dal import _lib  # noqa: E402
from dal.engine import PoolState  # noqa: E402


def main():
    shapes = sys.argv[1:] or ["2000000x256", "1000000x256", "70000x128", "100000x64", "284807x30"]
    rounds = int(os.environ.get("AB_ROUNDS", "5"))
    dev = torch.device("cuda:0")
    for sh in shapes:
        n, d = (int(v) for v in sh.split("x"))
        x = bench.upload(bench.host_pool(0, n, d, "normal" if d == 30 else "uniform"), dev)
        default = PoolState(x, excluded=np.arange(10), device=dev)
        forms = {"default(f16)": {}}
        if default.gram_i8 or default.gram_fp4:
            forms = {"f16": {"gram_i8": False}, "i8": {"gram_i8": True}}
            if default.gram_fp4:
                forms["fp4"] = {"gram_fp4": True}
            only = os.environ.get("AB_FORMS")
            if only:
                forms = {k: v for k, v in forms.items() if k in only.split(",")}
        pools = {k: PoolState(x, excluded=np.arange(10), device=dev, **v) for k, v in forms.items()}
        accs = {k: torch.zeros(st.n_pad, dtype=torch.int64, device=dev) for k, st in pools.items()}

        def run(k):
            st = pools[k]
            st._split_i8 = st._split_fp4 = None  # a cold step quantises the operand anew
            op = st.gram_operand()
            accs[k].zero_()
            st.gram_accumulate(accs[k], op, st.n_pad)
            st.gram_residual(accs[k], op)

        for k in pools:
            run(k)
        torch.cuda.synchronize()
        note = ""
        if len(pools) >= 2:
            keys = list(pools)
            diffs = [f"{a} - {b} <= {float((accs[a] - accs[b]).abs().max().item()) / 2.0 ** 32:.3g}"
                     for i, a in enumerate(keys) for b in keys[i + 1:]]
            bound = float(_lib.load().dal_density_error_bound_sym_d(n - 10, default.d_pad))
            note = f"  [densities differ by: {', '.join(diffs)}; bound {bound:.3g}]"
        reps = 5 if n * d < 5e7 else 1
        t = {k: [] for k in pools}
        for _ in range(rounds):
            for k in pools:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    run(k)
                e1.record()
                torch.cuda.synchronize()
                t[k].append(e0.elapsed_time(e1) / reps)
        parts = [f"{k} {statistics.median(v):.4f} ms (min {min(v):.4f}, max {max(v):.4f})" for k, v in t.items()]
        for a, b in (("i8", "f16"), ("fp4", "i8")):
            if a in t and b in t:
                parts.append(f"{a} / {b} {statistics.median(t[a]) / statistics.median(t[b]):.4f}")
        print(f"{n} x {d}: " + " | ".join(parts) + note, flush=True)
        del default, pools, accs, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
