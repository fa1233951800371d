"""What do the int8 and the fp4 matrix instructions buy the density Gram?  Bare
loops of v_mfma_f32_16x16x32_f16, v_mfma_i32_16x16x64_i8 and
v_mfma_scale_f32_16x16x128_f8f6f4 (fp4 e2m1 on both sides, cbsz:4 blgp:4) in
the wide form's shape (scripts/mfma_rate_probe.hip: two waves per SIMD, B
fragments re-read from LDS by ds_read_b128) on operands of the config-4 pool:
H = fp16(2^12 u) of its first rows for fp16, a(H) = clamp(rint(H / 32), -127,
127) for int8, a4(H) = the element of +-{0, 1, 2, 3, 4, 6, 8, 12} nearest to
H / 32 (ties to the smaller magnitude) as e2m1 codes for fp4.

Per form: >= 2 s of back-to-back launches, then timed launches; cycles per
MFMA on one SIMD (stamped and from the wall time), the in-kernel clock of the last launch
(d s_memtime / d s_memrealtime x 100 MHz, median over blocks) and MFMAs per
second and SIMD.  The ratios: int8 MFMAs per second for each fp16 one (an int8
MFMA covers twice the features, so 1.0 would halve the kernel and 0.5 leave it
as it is), and fp4 MFMAs per second for each int8 one (twice the features
again; the stop line is 0.6).

Exactness of the scaled instruction's fp32 accumulation on integers: chains of
the Gram kernel's length (16 column tiles x 2 k-steps into one accumulator),
every accumulator element against the int64 value -- (a) every operand +-12,
signs aligned (every element at the chain's maximum 589,824) and random; (b)
products of the smallest unit added onto a C input near the maximum; (c) the
config-4 rows; and the operand lane map by a one-hot A against a B with
distinct columns.  Both scale choices (E8M0 127: the accumulator holds a
quarter of the integer; 128 on both sides: the integer itself) are checked.

usage: python scripts/mfma_rate_probe.py [out.json] [rounds]"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS, D = 4096, 256


def operands():
    x = np.random.default_rng(0).random((ROWS, D), dtype=np.float32)  # the first rows of the config-4 pool
    u = x / np.sqrt((x.astype(np.float64) ** 2).sum(1, keepdims=True)).astype(np.float32)
    h = (u * np.float32(4096)).astype(np.float16)
    a = np.clip(np.rint(h.astype(np.float32) / np.float32(32)), -127, 127).astype(np.int8)
    return np.ascontiguousarray(h), np.ascontiguousarray(a), a4_of(h)


GRID = np.array([0, 1, 2, 3, 4, 6, 8, 12])  # twice the e2m1 magnitudes; the index is the 3-bit value code


def a4_of(h):
    """fp16 H -> the signed grid integer nearest to H / 32 (ties to the smaller magnitude, clamp at 12)."""
    m = np.abs(h.astype(np.float64)) / 32.0
    idx = np.abs(m[..., None] - GRID).argmin(-1)  # (argmin takes the first, i.e. the smaller, of a tie)
    return (np.sign(h.astype(np.float64)) * GRID[idx]).astype(np.int64)


def codes_fp4(g):
    """grid integers [..., K] -> packed e2m1 codes [..., K / 2] (even feature in the low nibble, no -0)."""
    idx = np.abs(np.abs(g)[..., None] - GRID).argmin(-1)
    assert (GRID[idx] == np.abs(g)).all()
    c = (idx | ((g < 0) << 3)).astype(np.uint8)
    return np.ascontiguousarray(c[..., 0::2] | (c[..., 1::2] << 4))


def frags(m):
    """[chains][steps][16][128] grid integers -> [chains][steps][64 lanes][16 B]: lane 16 q + i holds
    row i, k = 32 q .. 32 q + 31 (the int8 form's row / column placement)."""
    b = codes_fp4(m)  # [chains][steps][16][64]
    ch, st = b.shape[:2]
    return np.ascontiguousarray(b.reshape(ch, st, 16, 4, 16).transpose(0, 1, 3, 2, 4))


def exact_cases(a4):
    rng = np.random.default_rng(1)
    steps, cases = 32, []
    z = np.zeros((1, 16, 16), dtype=np.int64)
    # (a) every operand +-12: signs aligned per row and column, and random
    sk = rng.choice([-1, 1], size=(1, steps, 1, 128))
    ri, cj = rng.choice([-1, 1], size=(1, 1, 16, 1)), rng.choice([-1, 1], size=(1, 1, 16, 1))
    cases.append(("a_max_aligned", 12 * sk * ri, 12 * sk * cj, z))
    cases.append(("a_max_random", 12 * rng.choice([-1, 1], size=(4, steps, 16, 128)),
                  12 * rng.choice([-1, 1], size=(4, steps, 16, 128)), np.repeat(z, 4, 0)))
    # (b) unit products onto a C near the maximum: all 4,096 of them +1, and one per MFMA
    one = np.ones((1, steps, 16, 128), dtype=np.int64)
    cases.append(("b_unit_all", one, one, z + 589824 - 4096))
    x = np.zeros((1, steps, 16, 128), dtype=np.int64)
    x[0, np.arange(steps), :, (np.arange(steps) * 37) % 128] = 1
    cases.append(("b_unit_one_per_mfma", x, one * rng.choice([-1, 1], size=(1, 1, 16, 1)), z + 589824 - 40))
    cases.append(("b_unit_mixed_signs", rng.choice([-1, 1], size=(4, steps, 16, 128)),
                  rng.choice([-1, 1], size=(4, steps, 16, 128)), np.repeat(z, 4, 0) + 589824 - 4096))
    # (c) the config-4 rows: chain b = 256 columns (rows 256 b ..) against 16 resident rows
    nb = ROWS // 256
    xs = a4.reshape(nb, 16, 16, 2, 128).transpose(0, 1, 3, 2, 4).reshape(nb, steps, 16, 128)
    res = a4[::-1][:16 * nb].reshape(nb, 16, 2, 128)  # resident rows: from the pool's end
    ys = np.broadcast_to(res.transpose(0, 2, 1, 3)[:, None], (nb, 16, 2, 16, 128)).reshape(nb, steps, 16, 128)
    cases.append(("c_config4_rows", xs, ys, np.repeat(z, nb, 0)))
    # lane map: A one-hot at (row 3, k 37), B with 16 distinct columns that shift with k
    x = np.zeros((1, 1, 16, 128), dtype=np.int64)
    x[0, 0, 3, 37] = 2
    vals = np.array([1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12])  # every grid value once
    y = vals[(np.arange(16)[:, None] + np.arange(128)[None, :]) % 15]
    y[15] = vals[(2 * np.arange(128)) % 15]  # (16 columns, 15 values: the last column walks them at its own pace)
    y = y[None, None]
    cases.append(("lane_map_one_hot", x, y, z))
    return cases


def run_exact(lib, a4):
    out = []
    for scale in (128, 127):
        word = scale * 0x01010101
        f = 4.0 ** (scale - 127) / 4.0  # the accumulator's unit: e2m1 values are half the grid's integers
        for name, x, y, c in exact_cases(a4):
            x, y = np.broadcast_to(x, np.broadcast_shapes(x.shape, y.shape)), np.broadcast_to(y, np.broadcast_shapes(
                x.shape, y.shape))
            ch, st = x.shape[:2]
            want = c + np.einsum("csik,csjk->cij", x, y)  # int64: [chain][first operand's row][second's row]
            # C / D: lane 16 q + j, register r = element [row 4 q + r][column j]
            cin = np.ascontiguousarray((c * f).astype(np.float32).reshape(ch, 4, 4, 16).transpose(0, 1, 3, 2))
            got = np.zeros((ch, 4, 16, 4), dtype=np.float32)
            fx, fy = frags(x), frags(y)
            rc = lib.mfma_fp4_exact(fx.ctypes.data, fy.ctypes.data, cin.ctypes.data, got.ctypes.data, ch, st, word)
            assert rc == 0, rc
            d = got.transpose(0, 1, 3, 2).reshape(ch, 16, 16).astype(np.float64) / f
            bad = int((d != want).sum())
            r = {"case": name, "scale_e8m0": scale, "chains": ch, "mfmas_per_chain": st, "elements": int(want.size),
                 "inexact": bad, "max_abs_expected": int(np.abs(want).max()),
                 "max_abs_difference": float(np.abs(d - want).max())}
            out.append(r)
            print(json.dumps(r), flush=True)
    return out


FORMS = ("f32_16x16x32_f16", "i32_16x16x64_i8", "scale_f32_16x16x128_f8f6f4_fp4")


def run(lib, form, ops, iters, warm_s, timed):
    out = (ctypes.c_double * 3)()
    stamps = np.zeros((1024, 4), dtype=np.uint64)
    rc = lib.mfma_rate(form, ops.ctypes.data, ops.shape[0], ops.strides[0], iters, warm_s, timed, out,
                       stamps.ctypes.data, 1024, 128 * 0x01010101)
    assert rc == 0, rc
    ms, per_wave, grid = out[0], out[1], int(out[2])
    st = stamps[:grid].astype(np.int64)
    cyc, real = st[:, 2] - st[:, 0], st[:, 3] - st[:, 1]
    clock = cyc / real * 0.1  # GHz (s_memrealtime ticks at 100 MHz)
    return {
        "form": FORMS[form],
        "grid": grid,
        "mfma_per_wave_per_launch": int(per_wave),
        "ms_per_launch": round(ms, 4),
        # The loop has no barrier, so the older wave of a SIMD (the stamped wave
        # 0 of waves 0 and 4) keeps the matrix pipe and its partner runs behind
        # it: the stamped span is one wave's MFMAs back to back.  The wall form
        # counts both waves over the whole launch at the stamped clock.
        "cycles_per_mfma_stamped_wave_median": round(float(np.median(cyc) / per_wave), 3),
        "cycles_per_mfma_simd_wall": round(float(ms * 1e-3 * np.median(clock) * 1e9 / (2 * per_wave)), 3),
        "clock_ghz_median": round(float(np.median(clock)), 4),
        "clock_ghz_p10_p90": [round(float(np.percentile(clock, q)), 4) for q in (10, 90)],
        "mfma_per_s_per_simd": round(2 * per_wave / (ms * 1e-3), 1),
    }


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    lib = ctypes.CDLL(os.path.join(HERE, "libmfma_rate_probe.so"))
    p = ctypes.c_void_p
    lib.mfma_rate.argtypes = [ctypes.c_int, p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                              p, p, ctypes.c_int, ctypes.c_int]
    lib.mfma_fp4_exact.argtypes = [p, p, p, p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    h, a, a4 = operands()
    c4 = codes_fp4(a4)  # [ROWS][128 B]: a 256-feature slice of a row is one staged row
    res = {"operand": f"first {ROWS} rows of the config-4 pool (U[0,1) {D}-d, default_rng(0))",
           "a_min_max": [int(a.min()), int(a.max())], "a4_min_max": [int(a4.min()), int(a4.max())], "runs": []}
    # exactness first: an inexact element stops the design whatever the rate
    res["fp4_exact"] = run_exact(lib, a4)
    res["fp4_inexact_elements"] = sum(r["inexact"] for r in res["fp4_exact"])
    print(json.dumps({"fp4_inexact_elements": res["fp4_inexact_elements"]}), flush=True)
    # the forms alternate, so a drift of the box shows in both
    for _ in range(rounds):
        for form, ops in ((0, h), (1, a), (2, c4)):
            r = run(lib, form, ops, 1000, 2.5, 20)
            res["runs"].append(r)
            print(json.dumps(r), flush=True)
    f16 = [r["mfma_per_s_per_simd"] for r in res["runs"] if r["form"].endswith("f16")]
    i8s = [r["mfma_per_s_per_simd"] for r in res["runs"] if r["form"].endswith("i8")]
    fp4 = [r["mfma_per_s_per_simd"] for r in res["runs"] if r["form"].endswith("fp4")]
    res["i8_mfma_per_s_over_f16_min_max"] = [round(min(i8s) / max(f16), 4), round(max(i8s) / min(f16), 4)]
    res["fp4_mfma_per_s_over_i8_min_max"] = [round(min(fp4) / max(i8s), 4), round(max(fp4) / min(i8s), 4)]
    res["fp4_stop_line"] = 0.6
    print(json.dumps({k: res[k] for k in ("i8_mfma_per_s_over_f16_min_max", "fp4_mfma_per_s_over_i8_min_max")}),
          flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
