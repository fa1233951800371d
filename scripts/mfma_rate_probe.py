"""What does the int8 matrix instruction buy the density Gram?  Bare loops of
v_mfma_f32_16x16x32_f16 and v_mfma_i32_16x16x64_i8 in the wide form's shape
(scripts/mfma_rate_probe.hip: two waves per SIMD, B fragments re-read from LDS
by ds_read_b128) on operands of the config-4 pool: H = fp16(2^12 u) of its
first rows for fp16, a(H) = clamp(rint(H / 32), -127, 127) for int8.

Per form: >= 2 s of back-to-back launches, then timed launches; cycles per
MFMA on one SIMD (stamped and from the wall time), the in-kernel clock of the last launch
(d s_memtime / d s_memrealtime x 100 MHz, median over blocks) and MFMAs per
second and SIMD.  The last line is the ratio the int8 form of the Gram rests
on: int8 MFMAs per second for each fp16 MFMA per second (an int8 MFMA covers
twice the features, so 1.0 would halve the kernel and 0.5 leave it as it is).

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
    return np.ascontiguousarray(h), np.ascontiguousarray(a)


def run(lib, i8, ops, iters, warm_s, timed):
    out = (ctypes.c_double * 3)()
    stamps = np.zeros((1024, 4), dtype=np.uint64)
    rc = lib.mfma_rate(int(i8), ops.ctypes.data, ops.shape[0], ops.strides[0], iters, warm_s, timed, out,
                       stamps.ctypes.data, 1024)
    assert rc == 0, rc
    ms, per_wave, grid = out[0], out[1], int(out[2])
    st = stamps[:grid].astype(np.int64)
    cyc, real = st[:, 2] - st[:, 0], st[:, 3] - st[:, 1]
    clock = cyc / real * 0.1  # GHz (s_memrealtime ticks at 100 MHz)
    return {
        "form": "i32_16x16x64_i8" if i8 else "f32_16x16x32_f16",
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
                              p, p, ctypes.c_int]
    h, a = operands()
    res = {"operand": f"first {ROWS} rows of the config-4 pool (U[0,1) {D}-d, default_rng(0))",
           "a_min_max": [int(a.min()), int(a.max())], "runs": []}
    # the forms alternate, so a drift of the box shows in both
    for _ in range(rounds):
        for i8, ops in ((False, h), (True, a)):
            r = run(lib, i8, ops, 1000, 2.5, 20)
            res["runs"].append(r)
            print(json.dumps(r), flush=True)
    f16 = [r["mfma_per_s_per_simd"] for r in res["runs"] if r["form"].endswith("f16")]
    i8s = [r["mfma_per_s_per_simd"] for r in res["runs"] if r["form"].endswith("i8")]
    res["i8_mfma_per_s_over_f16_min_max"] = [round(min(i8s) / max(f16), 4), round(max(i8s) / min(f16), 4)]
    print(json.dumps({"i8_mfma_per_s_over_f16_min_max": res["i8_mfma_per_s_over_f16_min_max"]}), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
