"""The int8 form of the symmetric density Gram (csrc/gram_i8.hpp), restated in
NumPy on exact integers (CPU only).

With a(h) = clamp(rint(h / 32), -127, 127) (ties to even) the MFMAs form
sum_j <a_r, a_j> over the super-block pairs taken by the orientation rule, in
int32, and nothing else; the closed form of tests/test_gram_hh_algebra.py,
fed h' = 32 a(h) and l' = (h - h') + l where it takes (h, l), completes every
row to sum_j <u~_r, u~_j> exactly -- whatever a is, a clamped a included:
    sum_j <u~_r, u~_j> = 1024 sum_{pairs B takes} <a_r, a_j> + <l'_r, S~> + <h'_r, S^{l'} + CH'_B>.
Operand values are held as integers in units of 1/8 (H of the config pools
has fractional bits), so 1024 <a, a> reads 2^16 <a, a> in units of 1/64.
The header's host functions are checked against the restatement through
tests/host/gram_i8_driver.cpp."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_gram_hh_algebra import SB, residual, takes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "distributed-active-learning_amd", "csrc")
SRC = os.path.join(REPO, "tests", "host", "gram_i8_driver.cpp")
UNIT = 8  # integer operand units per 1.0 of H


def quant(h):
    """a(h) of gram_i8.hpp (h in H units, any float array)."""
    return np.clip(np.rint(np.asarray(h, dtype=np.float64) / 32.0), -127, 127).astype(np.int64)


def requant(h8, l8):
    """(h, l) -> (a, h', l') on integers in units of 1 / UNIT."""
    a = quant(h8 / UNIT)
    hq = 32 * UNIT * a
    return a, hq, (h8 - hq) + l8


@pytest.mark.parametrize("nsb,D,seed", [(2, 8, 1), (3, 5, 4), (6, 7, 2), (9, 3, 3)])
def test_i8_sym_gram_completes_every_row(nsb, D, seed):
    rng = np.random.default_rng(seed)
    n = nsb * SB
    H = rng.integers(-4096 * UNIT, 4096 * UNIT + 1, (n, D)).astype(np.int64)
    L = rng.integers(-2 * UNIT, 2 * UNIT + 1, (n, D)).astype(np.int64)
    edge = rng.random((n, D))
    H[edge < 0.04] = 4096 * UNIT   # |h| = 4096: a clamps at 127 and l' carries 32
    H[edge > 0.96] = -4096 * UNIT
    tie = (edge > 0.45) & (edge < 0.55)  # h / 32 = k + 1/2 exactly
    H[tie] = (32 * rng.integers(-120, 120, (n, D)) + 16)[tie] * UNIT
    zero = rng.random(n) < 0.05  # excluded / padding rows are zero rows
    H[zero] = 0
    L[zero] = 0
    A, Hq, Lq = requant(H, L)
    assert np.array_equal(Hq + Lq, H + L)
    assert np.abs(A).max() == 127 and np.abs(Lq).max() >= 32 * UNIT
    U = H + L
    acc = np.zeros(n, dtype=np.int64)
    for P in range(nsb):
        for Q in range(nsb):
            if takes(P, Q):
                T = A[P * SB:(P + 1) * SB] @ A[Q * SB:(Q + 1) * SB].T
                assert np.abs(T).max() < 2 ** 31  # an int32 holds every entry, as the MFMA's accumulator
                acc[P * SB:(P + 1) * SB] += T.sum(axis=1)  # row sums only (the kernel)
    full = U @ U.sum(axis=0)
    assert np.array_equal((32 * UNIT) ** 2 * acc + residual(Hq, Lq, nsb), full)
    assert not np.array_equal((32 * UNIT) ** 2 * acc, full)
    # ... and the fp16 form's terms do not complete the int8 row sums: the two belong together
    assert not np.array_equal((32 * UNIT) ** 2 * acc + residual(H, L, nsb), full)


def test_quantiser_ties_and_clamp():
    h = np.array([0, 15.99, 16, 16.01, 48, 80, -16, -48, 47.99, 4048, 4064, 4080, 4096, -4080, -4096, 65504, -65504,
                  31.5])
    assert quant(h).tolist() == [0, 0, 0, 1, 2, 2, 0, -2, 1, 126, 127, 127, 127, -127, -127, 127, -127, 1]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gram_i8") / "driver")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I" + CSRC, SRC, "-o", exe], check=True)
    return exe


def test_header_agrees_with_the_restatement(driver):
    rng = np.random.default_rng(7)
    # every fp16 H a pool can hold is a multiple of 2^-24 up to 4096; take fp16 values, ties and the clamp range
    h = np.concatenate([
        (rng.uniform(-4200, 4200, 4000)).astype(np.float16).astype(np.float64),
        (rng.uniform(-40, 40, 2000)).astype(np.float16).astype(np.float64),
        32.0 * np.arange(-130, 131) + 16.0, 32.0 * np.arange(-130, 131), np.array([0.0, -0.0, 4096.0, -4096.0])])
    l = (rng.uniform(-2, 2, h.size)).astype(np.float16).astype(np.float64)
    text = "".join(f"{a!r} {b!r}\n" for a, b in zip(h.tolist(), l.tolist()))
    out = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout.split()
    got = np.array(out, dtype=np.float64).reshape(-1, 3)
    a = quant(h)
    assert np.array_equal(got[:, 0], a)
    assert np.array_equal(got[:, 1], 32.0 * a)
    assert np.array_equal(got[:, 2], (h - 32.0 * a) + l)
    assert np.array_equal(got[:, 1] + got[:, 2], h + l)  # exact: nothing of u~ is lost
