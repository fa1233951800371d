"""Thresholded cosine pairs (column_similarities(threshold=)), the parts that
need no GPU: the filter's tile schedule walked on the CPU, its error bound
against a numpy emulation of the filter on adversarial rows, and the argument
checks of the C ABI and of the Python wrapper.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import pairs_reference as R
from dal import _lib
from oracle import dal_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "distributed-active-learning_amd", "csrc")
SRC = os.path.join(REPO, "tests", "host", "pairs_schedule_driver.cpp")
D_PADS = (32, 64, 128, 256, 512, 1024)


# ------------------------------------------------------------ schedule ----
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("pairs_schedule") / "driver")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I" + CSRC, SRC, "-o", exe], check=True)
    return exe


def test_schedule_sweep_every_pair_once(driver):
    """Block counts 1..40, every split of the rows and of the columns into two
    ranges: each call's linear index -> (P, Q) map visits exactly the pairs
    P <= Q of its rectangle, once, in row-major order, and the calls together
    tile the triangle with no pair twice or missing."""
    out = subprocess.run([driver, "sweep"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    # sum over nb = 1..40 of (nb + 1)^2 splits, plus one overhanging call each
    cases = sum((nb + 1) ** 2 for nb in range(1, 41)) + 40
    assert out.stdout.split() == ["cases", str(cases), "failures", "0"], out.stdout[-4000:]


def test_schedule_walk_matches_numpy(driver):
    """One call cutting inside the diagonal, against the rule stated in numpy."""
    r0, nr, j_lo, j_hi = 2, 7, 4, 11
    out = subprocess.run([driver, "walk", str(r0), str(nr), str(j_lo), str(j_hi)], capture_output=True, text=True,
                         check=True)
    got = [tuple(int(v) for v in line.split()) for line in out.stdout.splitlines()]
    want = [(P, Q, 3 if P == Q else 4) for P in range(r0, r0 + nr) for Q in range(j_lo, j_hi) if P <= Q]
    assert want and got == want


def test_schedule_index_map_at_pool_scale(driver):
    """2M rows are 7,814 blocks, 30.5M pairs: the fp64 square root of the
    index map lands on the right row for every one of them."""
    out = subprocess.run([driver, "large", "7814"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert out.stdout.split() == ["pairs", str(7814 * 7815 // 2), "failures", "0"]


# --------------------------------------------------------------- bound ----
def test_bound_range_and_monotone():
    lib = _lib.load()
    b = [lib.dal_cosine_pairs_error_bound(d) for d in D_PADS]
    assert all(np.isfinite(b))
    assert all(2.0 ** -11 < v < 2.0 ** -9 for v in b), b
    assert all(b[k] < b[k + 1] for k in range(len(b) - 1)), b


def _adversarial_rows(d, rng):
    """Rows that stress each term of the bound: components at the fp16
    subnormal edge of 2^12 u (|u| near 2^-26), one dominant component, mixed
    signs, rounding-boundary values, plus random rows."""
    rows = []
    e = np.zeros(d)
    e[0] = 1.0
    rows.append(e.copy())                                  # a single component
    for tiny in (2.0 ** -26, 2.0 ** -27, 1.5 * 2.0 ** -37, 2.0 ** -36 * 1.4999):
        r = np.full(d, tiny)
        r[d // 2] = 1.0                                    # one dominant, the rest subnormal in fp16
        rows.append(r)
        rows.append(r * np.where(np.arange(d) % 2, -1.0, 1.0))
    rows.append(np.ones(d))                                # equal components
    rows.append(np.where(np.arange(d) % 2, -1.0, 1.0))     # mixed signs
    rows.append(np.where(np.arange(d) % 3, 1.0, -1.0) * (1.0 + 2.0 ** -11))
    # components just above a half-ulp boundary of fp16 after the scaling
    rows.append((1.0 + (2.0 ** -11) * 1.0001) * np.ones(d) * np.where(np.arange(d) % 2, 1.0, 0.5))
    for _ in range(12):
        rows.append(rng.standard_normal(d))
        rows.append(rng.random(d))
        rows.append(rng.standard_normal(d) * 10.0 ** rng.uniform(-8, 0, d))  # wide dynamic range
    return np.asarray(rows, dtype=np.float32)


@pytest.mark.parametrize("d", [30, 64, 200, 1024])
def test_bound_holds_against_filter_emulation(d):
    """|filter value - canonical cosine| <= dal_cosine_pairs_error_bound(d_pad)
    for every pair of the adversarial rows.  The emulation: H = fp16(2^12
    fp32(u)), products exact (fp64 holds them), their exact sum (fp64, error
    below d 2^-52), plus the worst-case charge of the fp32 accumulation in any
    order, gamma_(d_pad) sum |h_i h_j| with unit roundoff 2^-24 (IEEE fp32
    round to nearest); a sequential fp32 accumulation is checked directly too."""
    lib = _lib.load()
    d_pad = int(lib.dal_pad_features(d))
    bound = lib.dal_cosine_pairs_error_bound(d_pad)
    X = _adversarial_rows(d, np.random.default_rng(3))
    U = O.l2_normalize(X)
    S = R.canonical_matrix(X)
    h = R.filter_emulation(U, d_pad)
    exact = h @ h.T
    u32 = 2.0 ** -24
    charge = (d_pad * u32 / (1 - d_pad * u32)) * (np.abs(h) @ np.abs(h).T)
    worst = np.abs(exact - S) + charge + d_pad * 2.0 ** -52
    print(f"d={d} d_pad={d_pad} bound={bound:.6e} worst={worst.max():.6e} exact-only={np.abs(exact - S).max():.6e}")
    assert worst.max() <= bound
    # sequential fp32 accumulation of the exact products (units of 2^-24, as the kernel holds them)
    H = (h * 4096.0).astype(np.float32)
    acc = np.zeros((H.shape[0], H.shape[0]), dtype=np.float32)
    for f in range(d_pad):
        acc = acc + H[:, f, None] * H[None, :, f]  # (products of two fp16 values: exact in fp32)
    assert np.abs(acc.astype(np.float64) * 2.0 ** -24 - S).max() <= bound


# ---------------------------------------------------------- validation ----
def test_host_argument_validation_without_gpu():
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    ok = dict(rows=p, rb0=0, nrb=2, cols=p, cb0=0, j_lo=0, j_hi=2, n=512, d_pad=64, flags=None, thr=0.5, cap=16,
              keys=p, approx=p, count=p, status=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.dal_cosine_pairs(a["rows"], a["rb0"], a["nrb"], a["cols"], a["cb0"], a["j_lo"], a["j_hi"], a["n"],
                                    a["d_pad"], a["flags"], a["thr"], a["cap"], a["keys"], a["approx"], a["count"],
                                    a["status"], None)

    # null pointers -> DAL_ERR_ARG before any HIP call
    for name in ("rows", "cols", "keys", "approx", "count", "status"):
        assert call(**{name: None}) == -1, name
    # shapes -> DAL_ERR_SHAPE
    assert call(d_pad=48) == -2                      # not a padded feature count
    assert call(d_pad=2048) == -2                    # beyond the supported widths
    assert call(rows=ctypes.c_void_p(264)) == -2     # operand not 16-byte aligned
    assert call(keys=ctypes.c_void_p(260)) == -2     # keys not 8-byte aligned
    assert call(j_hi=3) == -2                        # j_hi beyond the pool (512 rows = 2 blocks)
    assert call(n=513, j_hi=5) == -2
    assert call(j_lo=1, j_hi=0) == -2
    assert call(cb0=1, j_lo=0) == -2                 # columns before the operand's first block
    assert call(nrb=0) == -2
    assert call(rb0=-1) == -2
    assert call(n=0) == -2
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert call(thr=bad) == -2
    assert call(cap=-1) == -2
    # resolve
    assert lib.dal_cosine_pairs_resolve(None, 10, 4, 4, p, p, 1, p, None) == -1
    assert lib.dal_cosine_pairs_resolve(p, 10, 4, 4, None, p, 1, p, None) == -1
    assert lib.dal_cosine_pairs_resolve(p, 10, 4, 4, p, None, 1, p, None) == -1
    assert lib.dal_cosine_pairs_resolve(p, 10, 4, 4, p, p, 1, None, None) == -1
    assert lib.dal_cosine_pairs_resolve(p, 0, 4, 4, p, p, 1, p, None) == -2
    assert lib.dal_cosine_pairs_resolve(p, 10, 4, 3, p, p, 1, p, None) == -2    # ldx < d
    assert lib.dal_cosine_pairs_resolve(p, 10, 4, 4, p, p, -1, p, None) == -2
    assert lib.dal_cosine_pairs_resolve(p, 10, 4, 4, p, p, 0, p, None) == 0     # nothing to do, no launch


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf"), -1.0, -1.5, 1.0000001, 2.0, "x"])
def test_wrapper_rejects_threshold(bad):
    """The threshold is checked before the pool is touched (no GPU needed)."""
    from dal import similarity as sim

    with pytest.raises(ValueError, match="threshold"):
        sim.column_similarities(np.ones((4, 4), dtype=np.float32), threshold=bad)


def test_wrapper_rejects_max_pairs_without_threshold():
    from dal import similarity as sim

    with pytest.raises(ValueError, match="max_pairs"):
        sim.column_similarities(np.ones((4, 4), dtype=np.float32), max_pairs=10)
