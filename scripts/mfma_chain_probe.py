"""Does v_mfma_scale_f32_16x16x128_f8f6f4 (fp4 e2m1 on both sides, E8M0 scale
128) still add exact integers on chains that run over R pairs of the density
Gram instead of one?  scripts/mfma_rate_probe.py checked chains of 32 MFMAs
(16 column tiles x 2 k-steps, values up to 589,824); with the fold of the
integer forms deferred to once per R pairs (round 15) a chain is 32 R MFMAs
and reaches R x 589,824 -- 16,515,072 at R = 28, just below 2^24.  Same probe
kernel (mfma_fp4_exact of scripts/mfma_rate_probe.hip, one wave per chain, the
chain length a launch argument), every accumulator element against the int64
value from the host, for each R of the sweep:

 a_max_aligned   every operand +-12, signs aligned per row and column: every
                 element at +-R x 589,824
 a_max_random    every operand +-12, random signs, 4 chains
 b_toward_cap    a C input of +-(cap - 128) and one unit product per MFMA of
                 C's sign on the first 120 MFMAs (the chain ends 8 below the
                 cap), both signs of C in the columns
 b_away          the same C, one unit product per MFMA of the other sign on
                 every MFMA
 b_mixed         C = cap - 4096 R, unit products of random sign in every
                 position, 4 chains
 c_config4_rows  the config-4 rows: chains of 256 R columns against 16
                 resident rows

An R with an inexact element is not used by the kernel.  (The fold's own fp32
add of a lane's four elements is VALU arithmetic, exact below 2^24 by the
format; tests/test_gpu_gram_fold.py drives it to 4 x 7 x 589,824.)

usage: python scripts/mfma_chain_probe.py [out.json] [R ...]   (default R: 1 2 4 7 8 16 28)"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from mfma_rate_probe import ROWS, frags, operands  # noqa: E402

CHAIN_MAX = 589824  # kFp4ChainMax: one chain element per pair


def cases(a4, R):
    rng = np.random.default_rng(100 + R)
    steps, cap = 32 * R, R * CHAIN_MAX
    z = np.zeros((1, 16, 16), dtype=np.int64)
    out = []
    sk = rng.choice([-1, 1], size=(1, steps, 1, 128))
    ri, cj = rng.choice([-1, 1], size=(1, 1, 16, 1)), rng.choice([-1, 1], size=(1, 1, 16, 1))
    out.append(("a_max_aligned", 12 * sk * ri, 12 * sk * cj, z))
    out.append(("a_max_random", 12 * rng.choice([-1, 1], size=(4, steps, 16, 128)),
                12 * rng.choice([-1, 1], size=(4, steps, 16, 128)), np.repeat(z, 4, 0)))
    # C[i][j] = sj (cap - 128): the sign by the second operand's row j
    sj = rng.choice([-1, 1], size=16)
    sj[:2] = (1, -1)
    c_near = z + (sj * (cap - 128))[None, None, :]
    one_hot = np.zeros((1, steps, 16, 128), dtype=np.int64)
    one_hot[0, np.arange(steps), :, (np.arange(steps) * 37) % 128] = 1
    toward = one_hot.copy()
    toward[0, 120:] = 0
    y = np.ones((1, steps, 16, 128), dtype=np.int64) * sj[None, None, :, None]
    out.append(("b_toward_cap", toward, y, c_near))
    out.append(("b_away", one_hot, -y, c_near))
    out.append(("b_mixed", rng.choice([-1, 1], size=(4, steps, 16, 128)), rng.choice([-1, 1], size=(4, steps, 16, 128)),
                np.repeat(z, 4, 0) + cap - 4096 * R))
    nb = ROWS // (256 * R)
    if nb >= 1:
        xs = a4[:nb * 256 * R].reshape(nb, 16 * R, 16, 2, 128).transpose(0, 1, 3, 2, 4).reshape(nb, steps, 16, 128)
        res = a4[::-1][:16 * nb].reshape(nb, 16, 2, 128)  # resident rows: from the pool's end
        ys = np.broadcast_to(res.transpose(0, 2, 1, 3)[:, None], (nb, 16 * R, 2, 16, 128)).reshape(nb, steps, 16, 128)
        out.append(("c_config4_rows", xs, ys, np.repeat(z, nb, 0)))
    return out


def run(lib, a4, R):
    rows = []
    for name, x, y, c in cases(a4, R):
        shape = np.broadcast_shapes(x.shape, y.shape)
        x, y = np.broadcast_to(x, shape), np.broadcast_to(y, shape)
        ch, st = shape[:2]
        want = c + np.einsum("csik,csjk->cij", x, y)  # int64: [chain][first operand's row][second's row]
        assert np.abs(want).max() < 1 << 24 and np.abs(c).max() < 1 << 24
        # C / D: lane 16 q + j, register r = element [row 4 q + r][column j]; scale 128: the integer itself
        cin = np.ascontiguousarray(c.astype(np.float32).reshape(ch, 4, 4, 16).transpose(0, 1, 3, 2))
        got = np.zeros((ch, 4, 16, 4), dtype=np.float32)
        fx, fy = frags(x), frags(y)
        rc = lib.mfma_fp4_exact(fx.ctypes.data, fy.ctypes.data, cin.ctypes.data, got.ctypes.data, ch, st,
                                128 * 0x01010101)
        assert rc == 0, rc
        d = got.transpose(0, 1, 3, 2).reshape(ch, 16, 16).astype(np.float64)
        r = {"R": R, "case": name, "chains": int(ch), "mfmas_per_chain": int(st), "elements": int(want.size),
             "inexact": int((d != want).sum()), "max_abs_expected": int(np.abs(want).max()),
             "max_abs_difference": float(np.abs(d - want).max())}
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    sweep = [int(v) for v in sys.argv[2:]] or [1, 2, 4, 7, 8, 16, 28]
    lib = ctypes.CDLL(os.path.join(HERE, "libmfma_rate_probe.so"))
    p = ctypes.c_void_p
    lib.mfma_fp4_exact.argtypes = [p, p, p, p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    a4 = operands()[2]
    res = {"scale_e8m0": 128, "chain_max_per_pair": CHAIN_MAX, "cases": []}
    for R in sweep:
        res["cases"] += run(lib, a4, R)
    res["inexact_by_R"] = {str(R): sum(r["inexact"] for r in res["cases"] if r["R"] == R) for R in sweep}
    print(json.dumps({"inexact_by_R": res["inexact_by_R"]}), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
