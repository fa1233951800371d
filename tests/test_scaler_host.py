"""The exact StandardScaler and the LAL dataset classes without a GPU: the
restatement (tests/scaler_reference.py) against numpy's two-pass fp64 moments
and a closed form, the fp32 limb decomposition and the format rule of
csrc/scaler_exact.hpp (run on the host under AddressSanitizer + UBSan through
tests/host/scaler_exact_driver.cpp) against Python integers, the host finish
of dal.dataset, the start state, run_loop(initial_labeled=), the C ABI's
argument checks and dal.parallel.fit_scaler over gloo."""
import ctypes
import math
import os
import shutil
import socket
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import scaler_reference as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0:exitcode=86",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _pools():
    rng = np.random.default_rng(0)
    for n, d in ((2, 1), (65, 3), (4097, 30), (1000, 257)):
        yield f"u{n}x{d}", rng.random((n, d), dtype=np.float32)
    yield "n4097x8", (3.0 * rng.standard_normal((4097, 8)) + 10.0).astype(np.float32)


# ------------------------------------------------------------ restatement --
@pytest.mark.parametrize("name,X", list(_pools()), ids=[n for n, _ in _pools()])
def test_restatement_agrees_with_two_pass_fp64(name, X):
    # pairwise summation errs by about log2(n) 2^-53 relative; 1e-12 is a sanity bound some 500x above what
    # the two-pass formula shows on these pools, not a fit to the code under test
    mean, std = R.moments(X)
    x64 = X.astype(np.float64)
    want_mean, want_std = x64.mean(axis=0), x64.std(axis=0, ddof=1)
    rel_mean = np.abs(mean - want_mean) / np.abs(want_mean)
    rel_std = np.abs(std - want_std) / np.abs(want_std)
    print(name, "max rel mean", rel_mean.max(), "max rel std", rel_std.max())
    assert rel_mean.max() <= 1e-12 and rel_std.max() <= 1e-12


def _column_2p24(n=4097):
    return (16777216.0 + (np.arange(n) % 3)).astype(np.float32)[:, None]


def test_variance_of_2p24_column_is_the_closed_form():
    n = 4097
    X = _column_2p24(n)
    # 2^24 + 1 is not an fp32 value (it rounds to even): the fp32 column holds 2^24 + {0, 0, 2}
    assert X[:6, 0].astype(np.int64).tolist() == [2 ** 24, 2 ** 24, 2 ** 24 + 2] * 2
    # the variance does not see the offset 2^24: k = 0 on the 2,732 rows with i mod 3 in {0, 1}, k = 2 on 1,365
    n2 = 1365
    s1, s2 = 2 * n2, 4 * n2
    var = Fraction(n * s2 - s1 * s1, n * (n - 1))
    mean, std = R.moments(X)
    assert std[0] == math.sqrt(float(var))
    assert mean[0] == float(Fraction(n * 2 ** 24 + s1, n))
    # the one-pass fp64 formula the exact sums replace
    x64 = X[:, 0].astype(np.float64)
    one_pass = ((x64 * x64).sum() - x64.sum() ** 2 / n) / (n - 1)
    assert abs(one_pass - float(var)) > 1e-3


def test_restatement_edge_rows():
    X = np.float32([[1.5, -0.0, 3.0]])
    mean, std = R.moments(X)
    assert mean.tolist() == [1.5, 0.0, 3.0] and std.tolist() == [0.0, 0.0, 0.0]   # n == 1: zero variance
    assert not np.signbit(mean[1])
    z = R.transform(X, mean, std)
    assert z.dtype == np.float32 and not z.any() and not np.signbit(z).any()      # std == 0 -> +0.0
    X = np.float32([[1.0, 5.0], [3.0, 5.0]])
    mean, std = R.moments(X)
    assert mean.tolist() == [2.0, 5.0] and std.tolist() == [math.sqrt(2.0), 0.0]  # ddof = 1
    z = R.transform(X, mean, std, dtype=np.float64)
    assert z[:, 0].tolist() == [-1.0 * (1.0 / math.sqrt(2.0)), 1.0 * (1.0 / math.sqrt(2.0))]
    assert R.transform(X, mean, std, with_std=False, dtype=np.float64)[:, 0].tolist() == [-1.0, 1.0]
    assert R.transform(X, mean, std, with_mean=False, dtype=np.float64)[1].tolist() == [3.0 * (1.0 / math.sqrt(2.0)), 0.0]


# ------------------------------------------------------------ host finish --
def test_host_finish_equals_restatement():
    from dal.dataset import moments_from_cells, scale_factor, scaler_limbs

    rng = np.random.default_rng(3)
    X = np.concatenate([rng.random((301, 3), dtype=np.float32),
                        (3.0 * rng.standard_normal((301, 2)) + 10.0).astype(np.float32),
                        _column_2p24(301), np.zeros((301, 1), np.float32), np.full((301, 1), -2.5, np.float32),
                        (rng.choice([2.0 ** -40, 2.0 ** 20], 301) * rng.choice([-1, 1], 301)).astype(np.float32)[:, None]],
                       axis=1)
    low, top = R.column_format(X)
    k1, k2, q = scaler_limbs(low, top)
    assert (k1, k2) == (2, 4)                                   # the 2^-40 / 2^20 column: 61 and 122 bits
    assert q[6] == 0 and low[6] == R.NO_LOW and q[7] == -1 and q[8] == -40 and top[8] == 21
    mean, std = moments_from_cells(R.shard_cells(X, q, k1, k2), q, k1, k2, 301)
    want_mean, want_std = R.moments(X)
    assert np.array_equal(_bits(mean), _bits(want_mean)) and np.array_equal(_bits(std), _bits(want_std))
    assert std[6] == 0.0 and std[7] == 0.0 and scale_factor(std)[6] == 0.0 and scale_factor(std)[0] == 1.0 / std[0]
    # cells of two halves add word by word to cells of the same value
    a, b = R.shard_cells(X[:100], q, k1, k2), R.shard_cells(X[100:], q, k1, k2)
    m2, s2 = moments_from_cells(a + b, q, k1, k2, 301)
    assert np.array_equal(_bits(m2), _bits(mean)) and np.array_equal(_bits(s2), _bits(std))
    m1, s1 = moments_from_cells(R.shard_cells(X[:1], q, k1, k2), q, k1, k2, 1)
    assert np.array_equal(m1, X[0].astype(np.float64)) and not s1.any()


def test_span_refusal_names_the_column():
    from dal._lib import DalError
    from dal.dataset import scaler_limbs

    X = np.float32([[0.5, 1.0], [0.25, 1e-45]])                  # a subnormal beside 1.0: 150 bits
    low, top = R.column_format(X)
    assert (low[1], top[1]) == (-149, 1)
    with pytest.raises(DalError, match=r"status -3\): column 1 spans 150 bits"):
        scaler_limbs(low, top)
    k1, k2, _ = scaler_limbs([-124, 5], [0, 6])                  # the boundary itself: 124 bits -> 4 and 8 limbs
    assert (k1, k2) == (4, 8)
    with pytest.raises(DalError, match="column 0 spans 125 bits"):
        scaler_limbs([-125], [0])


# -------------------------------------------------- sanitizer: plain C++ --
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("scaler") / "scaler_exact_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "distributed-active-learning_amd", "csrc"),
                    os.path.join(REPO, "tests", "host", "scaler_exact_driver.cpp"), "-o", out],
                   check=True, capture_output=True, timeout=300)
    return out


def _run(driver, text):
    p = subprocess.run([driver], input=text, env=ENV, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-4000:]
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    return [ln.split() for ln in p.stdout.splitlines()]


def _check_values(driver, vals):
    """Every value's (low, top) and limbs of x and x^2 against Python integers."""
    vals = np.asarray(vals, dtype=np.float32)
    fin = np.isfinite(vals)
    low, top = R.column_format(vals[fin][:, None])
    q = 0 if low[0] == R.NO_LOW else int(low[0])
    span = 0 if low[0] == R.NO_LOW else int(top[0]) - q
    k1, k2 = max(1, -(-span // 31)), max(1, -(-2 * span // 31))
    assert k2 <= 8
    text = f"V {q} {k1} {k2} {len(vals)}\n" + "".join(f"{int(b):x}\n" for b in vals.view(np.uint32))
    out = iter(_run(driver, text))
    cell = [0] * (k1 + k2)
    for v in vals:
        f = next(out)
        if not np.isfinite(v):
            assert f == ["F", "0", "0", "0"]
            continue
        lo1, hi1 = R.column_format(np.float32([[v]]))
        assert f == ["F", "1"] + ([str(lo1[0]), str(hi1[0])] if v != 0 else ["0", "0"])
        xi = Fraction(float(v)) / Fraction(2) ** q
        assert xi.denominator == 1
        for tag, value, k, at in (("L", int(xi), k1, 0), ("S", int(xi) ** 2, k2, k1)):
            ln = next(out)
            want = R.digits(value, k)
            assert ln[0] == tag and [int(t) for t in ln[1:]] == want, (v, tag)
            for j, w in enumerate(want):
                cell[at + j] += w
    c = next(out)
    assert c[0] == "C" and [int(t) for t in c[1:]] == cell
    return q, k1, k2


def test_driver_limbs_of_x_and_x_squared(driver):
    rng = np.random.default_rng(1)
    assert _check_values(driver, rng.random(200, dtype=np.float32))[1:] == (1, 2)
    _check_values(driver, (3.0 * rng.standard_normal(200) + 10.0).astype(np.float32))
    assert _check_values(driver, [2.0 ** 24, 2.0 ** 24 + 2, 2.0 ** 24 + 6]) == (1, 1, 2)
    assert _check_values(driver, [0.0, -0.0]) == (0, 1, 1)
    _check_values(driver, [-1.5, 0.0, -0.0, 3.25, -1024.0])
    assert _check_values(driver, [2.0 ** -40, -(2.0 ** 20), 1.5 * 2.0 ** -40]) == (-41, 2, 4)
    # the widest legal span, 124 bits: subnormals beside 2^-26, and the top of the fp32 range beside 2^4
    assert _check_values(driver, [1e-45, 3e-45, -(2.0 ** -26), 1.1754942e-38]) == (-149, 4, 8)
    big = np.float32(3.4028235e38)
    assert _check_values(driver, [big, -big, 16.0, 2.0 ** 100]) == (4, 4, 8)
    # non-finite values are flagged and add nothing
    _check_values(driver, [1.0, np.nan, -np.inf, 0.5, np.inf])


def test_driver_format_rule(driver):
    from dal.dataset import scaler_limbs

    rng = np.random.default_rng(2)
    for _ in range(20):
        d = int(rng.integers(1, 9))
        low = rng.integers(-149, 100, d)
        top = low + rng.integers(1, 125, d)
        zeros = rng.random(d) < 0.2
        low[zeros], top[zeros] = R.NO_LOW, R.NO_TOP
        out = _run(driver, f"R {d}\n" + "".join(f"{a} {b}\n" for a, b in zip(low, top)))
        span = np.where(zeros, 0, top - low)
        k1, k2 = max(1, int(-(-span.max() // 31))), max(1, int(-(-2 * span.max() // 31)))
        assert out[0] == ["K", "-1", str(k1), str(k2)]
        assert [int(t) for t in out[1][1:]] == [0 if z else int(a) for a, z in zip(low, zeros)]
        got = scaler_limbs(low, top)                              # the library runs the same header
        assert got[:2] == (k1, k2) and got[2].tolist() == [int(t) for t in out[1][1:]]
    assert _run(driver, "R 3\n0 124\n-100 -25\n-149 -25\n")[0] == ["K", "-1", "4", "8"]
    assert _run(driver, "R 3\n0 10\n-149 1\n0 300\n")[0][:2] == ["K", "1"]
    assert _run(driver, f"R 2\n{R.NO_LOW} {R.NO_TOP}\n-100 25\n")[0][:2] == ["K", "1"]
    assert _run(driver, f"R 1\n{R.NO_LOW} {R.NO_TOP}\n") == [["K", "-1", "1", "1"], ["Q", "0"]]


# ------------------------------------------------------------ start state --
def test_start_state_properties():
    from dal.dataset import Dataset, start_state

    rng = np.random.default_rng(4)
    y = (rng.random(57) < 0.3).astype(np.int64)
    for n_start in (2, 3, 10, 57):
        known, unknown = start_state(y, n_start, seed=5)
        assert known.dtype == unknown.dtype == np.int64
        assert y[known[0]] == 1 and y[known[1]] == 0
        assert known.size == n_start and unknown.size == 57 - n_start
        assert np.array_equal(np.sort(np.concatenate([known, unknown])), np.arange(57))
        k2, u2 = start_state(y, n_start, seed=5)
        assert np.array_equal(k2, known) and np.array_equal(u2, unknown)
        rk, ru = R.start_state(y, n_start, seed=5)
        assert np.array_equal(rk, known) and np.array_equal(ru, unknown)
    assert not np.array_equal(start_state(y, 10, seed=6)[0], start_state(y, 10, seed=5)[0])
    ds = Dataset(np.zeros((57, 2), np.float32), y)
    known, unknown = ds.set_start_state(4, seed=9)
    assert ds.n_start == 4 and ds.indices_known is known and ds.indices_unknown is unknown
    assert np.array_equal(known, R.start_state(y, 4, seed=9)[0])
    for bad in (1, 0, -3):
        with pytest.raises(ValueError, match="at least 2"):
            start_state(y, bad)
    with pytest.raises(ValueError, match="each class"):
        start_state(np.ones(5, dtype=int), 2)
    with pytest.raises(ValueError, match="each class"):
        start_state(np.zeros(5, dtype=int), 2)
    with pytest.raises(ValueError, match="exceeds"):
        start_state(y, 58)


# --------------------------------------------------------------- run_loop --
def test_run_loop_initial_labeled_with_select_fn():
    from dal.loop import run_loop

    rng = np.random.default_rng(7)
    X = rng.standard_normal((40, 3)).astype(np.float32)
    y = (X[:, 0] > 0).astype(np.int64)
    start, _ = R.start_state(y, 4, seed=1)
    seen = []

    def select_fn(strategy, pool, unlabeled, model, k):
        seen.append(unlabeled.copy())
        return unlabeled[-k:]

    res = run_loop(X, y, strategy="lal", window_size=2, max_iterations=3, trainer="sklearn", select_fn=select_fn,
                   initial_labeled=start)
    rest = np.setdiff1d(np.arange(40), start)
    assert np.array_equal(seen[0], rest)                          # the ascending remainder
    assert res.log[0] == "labeled =  4  unlabeled =  36"
    assert np.array_equal(seen[1], rest[:-2]) and np.array_equal(seen[2], rest[:-4])
    assert [h.tolist() for h in res.labeled_history] == [rest[-2:].tolist(), rest[-4:-2].tolist(),
                                                         rest[-6:-4].tolist()]
    # None: the thesis scripts' start, unchanged
    seen.clear()
    run_loop(X, y, strategy="uncertainty", window_size=5, max_iterations=1, trainer="sklearn", select_fn=select_fn)
    assert np.array_equal(seen[0], np.arange(5, 40))
    for bad in ([], [3, 3], [-1, 2], [40]):
        with pytest.raises(ValueError, match="initial_labeled"):
            run_loop(X, y, trainer="sklearn", select_fn=select_fn, initial_labeled=bad)


def test_run_loop_initial_labeled_is_the_excluded_set(monkeypatch):
    """The density strategies' E is the given start (the GPU step replaced by recorders)."""
    import dal.density_weighting as dw
    import dal.engine as engine
    from dal.loop import run_loop

    rng = np.random.default_rng(8)
    X = rng.standard_normal((30, 3)).astype(np.float32)
    y = (X[:, 1] > 0).astype(np.int64)
    start = np.array([int(np.flatnonzero(y == 1)[-1]), int(np.flatnonzero(y == 0)[-1]), 11])
    rec = {}

    class FakeState:
        def __init__(self, pool, excluded=None, device=None):
            rec["excluded"] = None if excluded is None else np.asarray(excluded).copy()

    class FakeSel:
        def __init__(self, idx):
            self.indices = self
            self._idx = idx

        def cpu(self):
            return self

        def numpy(self):
            return self._idx

    def fake_select(state, unlabeled, forest, k, beta=1.0):
        rec.setdefault("unlabeled", []).append(np.asarray(unlabeled).copy())
        return FakeSel(np.asarray(unlabeled)[:k])

    monkeypatch.setattr(engine, "PoolState", FakeState)
    monkeypatch.setattr(dw, "select", fake_select)
    res = run_loop(X, y, strategy="density", window_size=3, max_iterations=2, trainer="sklearn",
                   initial_labeled=start)
    assert np.array_equal(rec["excluded"], start)
    rest = np.setdiff1d(np.arange(30), start)
    assert np.array_equal(rec["unlabeled"][0], rest) and np.array_equal(rec["unlabeled"][1], rest[3:])
    assert res.labeled_history[0].tolist() == rest[:3].tolist()
    rec.clear()
    run_loop(X, y, strategy="density", window_size=3, max_iterations=1, trainer="sklearn")
    assert np.array_equal(rec["excluded"], np.arange(3)) and np.array_equal(rec["unlabeled"][0], np.arange(3, 30))


# ------------------------------------------------------------------ C ABI --
def test_abi_exports_and_rejects_before_any_hip_call():
    import dal
    from dal import _lib

    lib = _lib.load()
    assert lib.dal_abi_version() == 10
    for name in ("dal_scaler_format", "dal_scaler_accumulate", "dal_scaler_transform", "dal_scaler_limbs",
                 "dal_scaler_rows_per_block"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert dal.StandardScaler is dal.dataset.StandardScaler and dal.Dataset is dal.dataset.Dataset
    assert _lib.DAL_FLAG_NONFINITE == 16
    p = ctypes.c_void_p(256)
    big = (1 << 31)
    fmt, acc, tr = lib.dal_scaler_format, lib.dal_scaler_accumulate, lib.dal_scaler_transform
    for i in range(4):                                            # x low top status
        a = [p, p, p, p]
        a[i] = None
        assert fmt(a[0], 10, 2, 2, a[1], a[2], a[3], None) == -1
    assert fmt(p, -1, 2, 2, p, p, p, None) == -2 and fmt(p, big, 2, 2, p, p, p, None) == -2
    assert fmt(p, 10, 0, 2, p, p, p, None) == -2 and fmt(p, 10, 3, 2, p, p, p, None) == -2
    assert fmt(p, 0, 2, 2, p, p, p, None) == 0                    # n == 0: nothing is launched
    for i in range(3):                                            # x q cells
        a = [p, p, p]
        a[i] = None
        assert acc(a[0], 10, 2, 2, a[1], 1, 2, a[2], None) == -1
    assert acc(p, big, 2, 2, p, 1, 2, p, None) == -2 and acc(p, 10, 2, 1, p, 1, 2, p, None) == -2
    for k1, k2 in ((0, 2), (9, 2), (1, 0), (1, 9)):
        assert acc(p, 10, 2, 2, p, k1, k2, p, None) == -3         # DAL_ERR_UNSUPPORTED
    assert acc(p, 0, 2, 2, p, 8, 8, p, None) == 0
    assert tr(None, 10, 2, 2, p, p, p, 0, 2, None) == -1 and tr(p, 10, 2, 2, p, p, None, 0, 2, None) == -1
    assert tr(p, 10, 2, 2, p, p, p, 2, 2, None) == -1             # a bad out_dtype
    assert tr(p, 10, 2, 2, p, p, p, 0, 1, None) == -2 and tr(p, 10, 2, 1, p, p, p, 1, 2, None) == -2
    assert tr(p, 0, 2, 2, None, None, p, 1, 2, None) == 0         # mean and factor are nullable
    assert lib.dal_scaler_limbs(None, p, 1, p, p, None, None) == -1
    rpb = lib.dal_scaler_rows_per_block
    assert rpb(0, 2) == 0 and rpb(10, 0) == 0
    assert rpb(1, 1) == 256 and rpb(4097, 30) == 8 and rpb(65, 257) == 4 and rpb(1 << 22, 2) == 2048


def test_fit_rejects_bad_input_before_the_gpu():
    from dal.dataset import Dataset, StandardScaler, StandardScalerModel

    with pytest.raises(ValueError, match="test_scaler"):
        Dataset(np.zeros((2, 2), np.float32), [0, 1]).standardize(test_scaler="both")
    m = StandardScalerModel([0.0, 1.0], [1.0, 0.0], 5)
    assert m.n == 5 and m.mean.dtype == np.float64 and m.with_mean and m.with_std
    s = StandardScaler(with_mean=False)
    assert (s.with_mean, s.with_std) == (False, True)


# ------------------------------------------------------------------- gloo --
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_pool():
    rng = np.random.default_rng(11)
    return np.concatenate([rng.random((700, 3), dtype=np.float32), _column_2p24(700),
                           (3.0 * rng.standard_normal((700, 2)) + 10.0).astype(np.float32)], axis=1)


def _restated_steps(x_local, fmt=None):
    """The local steps of fit_scaler from the restatement (CPU tensors)."""
    import torch

    x = x_local.numpy()
    if fmt is None:
        low, top = R.column_format(x)
        return torch.from_numpy(low), torch.from_numpy(top), 0
    q, k1, k2 = fmt
    return torch.from_numpy(R.shard_cells(x, q, k1, k2))


def _gloo_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist

    from dal import parallel

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        X = _gloo_pool()
        # world 3: rank 1's shard is empty
        cuts = {2: [0, 301, 700], 3: [0, 450, 450, 700]}[world]
        shard = torch.from_numpy(X[cuts[rank]:cuts[rank + 1]])
        m = parallel.fit_scaler(shard, parallel.TorchComm(), accumulate_fn=_restated_steps)
        q.put((rank, int(shard.shape[0]), m.n, m.mean.tobytes(), m.std.tobytes()))
    except Exception as e:
        q.put((rank, repr(e), None, None, None))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_fit_scaler_gives_the_single_process_bytes(world):
    import torch
    import torch.multiprocessing as mp

    from dal import parallel

    X = _gloo_pool()
    mean, std = R.moments(X)
    one = parallel.emulate_fit_scaler([torch.from_numpy(X)], accumulate_fn=_restated_steps)
    assert one.n == 700 and one.mean.tobytes() == mean.tobytes() and one.std.tobytes() == std.tobytes()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r[0] for r in res) == list(range(world))
    if world == 3:
        assert dict((r[0], r[1]) for r in res)[1] == 0
    for rank, rows, n, mb, sb in res:
        assert n == 700, (rank, rows)
        assert mb == mean.tobytes() and sb == std.tobytes()
