"""The fp4 form of the symmetric density Gram (csrc/gram_fp4.hpp), restated in
NumPy on exact integers (CPU only).

With a4(h) = the element of G = +-{0, 1, 2, 3, 4, 6, 8, 12} (twice the e2m1
magnitudes) nearest to h / 32, a tie to the smaller magnitude and anything
beyond +-12 to +-12, the MFMAs form sum_j <a4_r, a4_j> over the super-block
pairs taken by the orientation rule and nothing else; the closed form of
tests/test_gram_hh_algebra.py, fed h' = 32 a4(h) and l' = (h - h') + l where
it takes (h, l), completes every row to sum_j <u~_r, u~_j> exactly:
    sum_j <u~_r, u~_j> = 1024 sum_{pairs B takes} <a4_r, a4_j> + <l'_r, S~> + <h'_r, S^{l'} + CH'_B>.
Operand values are held as integers in units of 1/8 as in
test_gram_i8_algebra.py.  The header's host functions are checked against the
restatement through tests/host/gram_fp4_driver.cpp, over every finite fp16 h."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_gram_hh_algebra import SB, residual, takes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "distributed-active-learning_amd", "csrc")
SRC = os.path.join(REPO, "tests", "host", "gram_fp4_driver.cpp")
UNIT = 8  # integer operand units per 1.0 of H
GRID = np.array([0, 1, 2, 3, 4, 6, 8, 12], dtype=np.int64)  # index = the 3-bit value code
ACC_SHIFT, CHAIN_MAX, ROW_MAX = 18, 16 * 256 * 144, 256 * 256 * 144


def quant4(h):
    """a4(h) of gram_fp4.hpp (h in H units, any float array): nearest element of
    G to |h| / 32 -- argmin takes the first, i.e. the smaller, of a tie, and the
    last (12) beyond the grid -- with h's sign."""
    h = np.asarray(h, dtype=np.float64)
    m = np.abs(h) / 32.0
    idx = np.abs(m[..., None] - GRID).argmin(-1)
    return np.where(h < 0, -GRID[idx], GRID[idx])


def code4(g):
    """The 4-bit code of an element of G: sign in bit 3, value index in bits 0-2."""
    g = np.asarray(g, dtype=np.int64)
    idx = np.abs(np.abs(g)[..., None] - GRID).argmin(-1)
    assert np.array_equal(GRID[idx], np.abs(g))
    return idx | ((g < 0).astype(np.int64) << 3)


def decode4(code):
    code = np.asarray(code, dtype=np.int64)
    return np.where(code & 8, -GRID[code & 7], GRID[code & 7])


def requant4(h8, l8):
    """(h, l) -> (a4, h', l') on integers in units of 1 / UNIT."""
    a = quant4(h8 / UNIT)
    hq = 32 * UNIT * a
    return a, hq, (h8 - hq) + l8


@pytest.mark.parametrize("nsb,D,seed", [(2, 8, 1), (3, 5, 4), (6, 7, 2), (9, 3, 3)])
def test_fp4_sym_gram_completes_every_row(nsb, D, seed):
    rng = np.random.default_rng(seed)
    n = nsb * SB
    H = rng.integers(-4096 * UNIT, 4096 * UNIT + 1, (n, D)).astype(np.int64)
    small = rng.random((n, D)) < 0.6  # most of a pool's H lies inside the grid (|h| < 384)
    H[small] = rng.integers(-400 * UNIT, 400 * UNIT + 1, (n, D))[small]
    L = rng.integers(-2 * UNIT, 2 * UNIT + 1, (n, D)).astype(np.int64)
    edge = rng.random((n, D))
    H[edge < 0.04] = 4096 * UNIT   # |h| = 4096: a4 clamps at 12 and l' carries 3,712
    H[edge > 0.96] = -4096 * UNIT
    tie = (edge > 0.45) & (edge < 0.55)  # h / 32 at a midpoint of the grid exactly
    mid = np.array([0.5, 1.5, 2.5, 3.5, 5.0, 7.0, 10.0])
    H[tie] = (rng.choice([-1, 1], (n, D)) * (32 * UNIT * mid[rng.integers(0, 7, (n, D))]).astype(np.int64))[tie]
    zero = rng.random(n) < 0.05  # excluded / padding rows are zero rows
    H[zero] = 0
    L[zero] = 0
    A, Hq, Lq = requant4(H, L)
    assert np.array_equal(Hq + Lq, H + L)
    assert np.isin(np.abs(A), GRID).all() and np.abs(A).max() == 12
    # a clamped element's l' carries what h' left, and stays below 2^13 (the closed form's terms)
    assert np.abs(Lq).max() >= (4096 - 384) * UNIT and np.abs(Lq).max() < 8192 * UNIT
    U = H + L
    acc = np.zeros(n, dtype=np.int64)
    for P in range(nsb):
        for Q in range(nsb):
            if takes(P, Q):
                T = A[P * SB:(P + 1) * SB] @ A[Q * SB:(Q + 1) * SB].T
                assert np.abs(T).max() <= 144 * D
                acc[P * SB:(P + 1) * SB] += T.sum(axis=1)  # row sums only (the kernel)
    full = U @ U.sum(axis=0)
    assert np.array_equal((32 * UNIT) ** 2 * acc + residual(Hq, Lq, nsb), full)
    assert not np.array_equal((32 * UNIT) ** 2 * acc, full)
    # ... and neither the fp16 form's nor the int8 form's terms complete the fp4 row sums
    assert not np.array_equal((32 * UNIT) ** 2 * acc + residual(H, L, nsb), full)
    from test_gram_i8_algebra import requant
    _, H8, L8 = requant(H, L)
    assert not np.array_equal((32 * UNIT) ** 2 * acc + residual(H8, L8, nsb), full)


def test_quantiser_ties_and_clamp():
    h = np.array([0, 15.99, 16, 16.01, 48, 48.01, 80, 80.01, 112, 112.5, 160, 160.5, 224, 224.5, 320, 320.5, 384, 4096,
                  65504, -16, -16.01, -48, -112.5, -320, -320.5, -4096, -65504, 31.5])
    assert quant4(h).tolist() == [0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 6, 6, 8, 8, 12, 12, 12,
                                  12, 0, -1, -1, -4, -8, -12, -12, -12, 1]


def test_range_constants():
    """One fp32 chain element (16 column tiles x 256 features between two folds)
    and a lane's four of them stay exact integers; a row's pair sum fits an int32."""
    assert CHAIN_MAX == 589_824 and 4 * CHAIN_MAX < 2 ** 24
    assert ROW_MAX == 9_437_184 < 2 ** 31
    assert 32 * 32 * 2 ** 8 == 1 << ACC_SHIFT  # the unit of G is 32 H units; H units^2 are 2^8 of the accumulator's


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gram_fp4") / "driver")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I" + CSRC, SRC, "-o", exe], check=True)
    return exe


def test_header_constants(driver):
    out = subprocess.run([driver, "consts"], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [ACC_SHIFT, 12, CHAIN_MAX, ROW_MAX]


def test_header_agrees_with_the_restatement_on_every_fp16(driver):
    bits = np.arange(1 << 16, dtype=np.uint16)
    h = bits.view(np.float16).astype(np.float64)
    h = h[np.isfinite(h)]  # every finite fp16 value, -0 and the subnormals included
    assert h.size == 63_488
    rng = np.random.default_rng(7)
    l = (rng.uniform(-2, 2, h.size)).astype(np.float16).astype(np.float64)
    text = "".join(f"{a!r} {b!r}\n" for a, b in zip(h.tolist(), l.tolist())) + "nan 0.5\n"
    out = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout.split()
    got = np.array(out, dtype=np.float64).reshape(-1, 5)
    nan_row, got = got[-1], got[:-1]
    a = quant4(h)
    m = np.abs(h) / 32.0
    assert np.isin(np.abs(got[:, 0]), GRID).all()  # grid membership
    # nearest element: no element of G is closer, and of two equally close ones the smaller was taken
    dist = np.abs(m[:, None] - GRID[None, :])
    own = np.abs(m - np.abs(got[:, 0]))
    assert (own[:, None] <= dist).all()
    tied = (dist == own[:, None]).sum(axis=1) > 1
    assert tied.sum() == 2 * 7  # the seven midpoints, both signs (all are fp16 values)
    assert (np.abs(got[tied, 0])[:, None] <= np.where(dist[tied] == own[tied, None], GRID[None, :], 99)).all()
    assert np.array_equal(np.abs(got[m > 12, 0]), np.full((m > 12).sum(), 12.0))  # clamp
    assert np.array_equal(np.sign(got[:, 0]), np.sign(h) * (got[:, 0] != 0))
    assert np.array_equal(got[:, 0], a)
    # the code: sign in bit 3, value index in bits 0-2, never -0; decode inverts it
    assert np.array_equal(got[:, 1], code4(a))
    assert not (got[:, 1] == 8).any() and got[:, 1].max() <= 15
    assert np.array_equal(got[:, 2], a) and np.array_equal(decode4(code4(a)), a)
    assert np.array_equal(got[:, 3], 32.0 * a)
    assert np.array_equal(got[:, 4], (h - 32.0 * a) + l)
    assert np.array_equal(got[:, 3] + got[:, 4], h + l)  # exact in fp64: nothing of u~ is lost
    assert np.array_equal(got[:, 4] * 2.0 ** 24, np.rint(got[:, 4] * 2.0 ** 24))  # l' a multiple of 2^-24
    unit = np.abs(h) <= 4096  # H of a unit row
    assert np.abs(got[unit, 4]).max() < 2 ** 13
    assert nan_row[0] == 0 and nan_row[1] == 0 and nan_row[3] == 0  # a NaN: a4 = 0, a defined value
