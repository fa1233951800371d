"""Incremental density exclusion, the parts that need no GPU: the exported
symbols and the downdate bound, the argument checks of the entry points and
of run_loop(density_over=), and the NumPy restatement of PoolState.exclude's
bookkeeping (tests/exclude_reference.py) against the oracle's canonical
column sum and density."""
import ctypes

import numpy as np
import pytest

import exclude_reference as XR
from conftest import load_golden
from dal import _lib, loop
from oracle import dal_oracle as O


def test_symbols_and_abi():
    lib = _lib.load()
    for name in ("dal_density_downdate", "dal_density_downdate_error_bound", "dal_canon_colsum_partials_chunks"):
        assert hasattr(lib, name), name
    assert lib.dal_abi_version() == 10
    assert _lib.DAL_DOWNDATE_MAX_ROWS == 1024 and _lib.DAL_DOWNDATE_TILE == 64
    assert _lib.DAL_DOWNDATE_MAX_ROWS % _lib.DAL_DOWNDATE_TILE == 0


@pytest.mark.parametrize("d_pad", [32, 64, 128, 256])
def test_downdate_bound_positive_and_monotone(d_pad):
    lib = _lib.load()
    b = [lib.dal_density_downdate_error_bound(m, d_pad) for m in range(1, _lib.DAL_DOWNDATE_MAX_ROWS + 1)]
    assert b[0] > 0.0
    assert all(y >= x for x, y in zip(b, b[1:]))
    # per column it stays below the cold Gram's bound: a downdate never costs
    # more interval width than the columns it removes were charged
    cold = lib.dal_density_error_bound_sym_d(1000, d_pad) / 1000
    assert b[-1] / _lib.DAL_DOWNDATE_MAX_ROWS < cold
    # and it covers the terms that do not depend on the kernel: the split's
    # 5 * 2^-22 and the dropped L.L's 2^-22 per column
    assert b[99] > 100 * 6 * 2.0 ** -22


def test_downdate_argument_checks_without_gpu():
    """Every check runs before any HIP call."""
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    ok = (p, 512, 64, p, 10, p, 0, None)
    assert lib.dal_density_downdate(None, *ok[1:]) == -1
    assert lib.dal_density_downdate(p, 512, 64, None, 10, p, 0, None) == -1
    assert lib.dal_density_downdate(p, 512, 64, p, 10, None, 0, None) == -1
    assert lib.dal_density_downdate(ctypes.c_void_p(4098), *ok[1:]) == -1  # operand not 16-byte aligned
    assert lib.dal_density_downdate(p, 384, 64, p, 10, p, 0, None) == -2   # n_pad not a multiple of 256
    assert lib.dal_density_downdate(p, 0, 64, p, 10, p, 0, None) == -2
    assert lib.dal_density_downdate(p, 512, 48, p, 10, p, 0, None) == -2   # d_pad not from dal_pad_features
    assert lib.dal_density_downdate(p, 512, 384, p, 10, p, 0, None) == -2
    assert lib.dal_density_downdate(p, 512, 64, p, 0, p, 0, None) == -2    # m < 1
    assert lib.dal_density_downdate(p, 512, 64, p, _lib.DAL_DOWNDATE_MAX_ROWS + 1, p, 0, None) == -5
    chunks = (p, 1000, 8, 8, p, p, p, 2, p, None)
    assert lib.dal_canon_colsum_partials_chunks(None, *chunks[1:]) == -1
    assert lib.dal_canon_colsum_partials_chunks(p, 1000, 8, 8, p, p, None, 2, p, None) == -1
    assert lib.dal_canon_colsum_partials_chunks(p, 1000, 8, 4, p, p, p, 2, p, None) == -2   # ldx < d
    assert lib.dal_canon_colsum_partials_chunks(p, 1000, 8, 8, p, p, p, 5, p, None) == -2   # more ids than chunks
    assert lib.dal_canon_colsum_partials_chunks(p, 1000, 8, 8, p, p, p, -1, p, None) == -2
    assert lib.dal_canon_colsum_partials_chunks(p, 1000, 8, 8, p, p, None, 0, p, None) == 0  # nothing listed


def test_run_loop_density_over_validation():
    g = load_golden("checkerboard2x2.npz")
    X, y = g["X"][:60], g["y"][:60]
    calls = []

    def pick(strategy, pool, unlabeled, model, k):
        calls.append(len(unlabeled))
        return unlabeled[:k]

    kw = dict(window_size=10, max_iterations=2, trainer="sklearn", select_fn=pick)
    with pytest.raises(ValueError, match="density_over"):
        loop.run_loop(X, y, strategy="density", density_over="labeled", **kw)
    for strategy in ("uncertainty", "random", "lal"):
        with pytest.raises(ValueError, match="has no density"):
            loop.run_loop(X, y, strategy=strategy, density_over="unlabeled", **kw)
    assert calls == []  # refused before any iteration
    for strategy in ("density", "information_density"):
        a = loop.run_loop(X, y, strategy=strategy, density_over="unlabeled", **kw)
        b = loop.run_loop(X, y, strategy=strategy, **kw)  # the default is "initial"
        c = loop.run_loop(X, y, strategy=strategy, density_over="initial", **kw)
        assert a.log == b.log == c.log  # with select_fn the value changes nothing


def test_labeled_sentinel_is_exported():
    from dal import density_weighting as dw

    assert dw.LABELED != dw.L0 and isinstance(dw.LABELED, str)
    with pytest.raises(ValueError, match="excluded_idx"):
        dw._pool_state(np.zeros((4, 2), np.float32), [1, 2], 1, "neither", None, None)


def _unit_rows(name):
    return O.l2_normalize(load_golden(name)["X"])


DELTAS = {
    "one": [700],
    "ten": list(range(300, 310)),
    "spread": list(range(5, 1500, 6))[:257],
    "tail": [1499, 1290, 1400, 1280],
    "dups": [3, 3, 9, 40, 40, 41],
}


@pytest.mark.parametrize("case", sorted(DELTAS))
def test_restated_bookkeeping_matches_canonical_colsum(case):
    U = _unit_rows("synthetic_1500x30_T100.npz")
    E = np.arange(10)
    delta = np.asarray(DELTAS[case])
    pool = XR.Pool(U, E)
    new = XR.new_rows(E, delta, U.shape[0])
    assert pool.exclude(delta) == new.size == np.setdiff1d(delta, E).size
    union = np.union1d(E, delta)
    assert np.array_equal(pool.excluded, union)
    assert pool.rewritten == sorted(set((new // 256).tolist()))  # only the touched chunks, each once
    s = pool.colsum()
    ref = O.column_sum_canonical(U, O.exclusion_mask(U.shape[0], union))
    assert np.array_equal(s.view(np.uint64), ref.view(np.uint64))
    # a second batch, and a batch that adds nothing
    assert pool.exclude(delta) == 0
    more = np.array([11, 1023, 1024])
    assert pool.exclude(more) == np.setdiff1d(more, union).size
    ref = O.column_sum_canonical(U, O.exclusion_mask(U.shape[0], np.union1d(union, more)))
    assert np.array_equal(pool.colsum().view(np.uint64), ref.view(np.uint64))


def test_restated_shard_chunks_and_range_check():
    # shard [1024, 1500): local chunks of the rows it owns only
    assert XR.touched_chunks(np.array([3, 1024, 1279, 1280, 1499]), 1024, 476).tolist() == [0, 1]
    assert XR.touched_chunks(np.array([3, 600]), 1024, 476).size == 0
    with pytest.raises(ValueError):
        XR.new_rows([], [1500], 1500)
    with pytest.raises(ValueError):
        XR.new_rows([], [-1], 1500)


def test_density_is_lowered_by_the_cosine_sums():
    """d(E u Delta) = d(E) - sum_{j in Delta} <u_i, u_j> on every row outside
    both: the identity the downdate kernel applies (fp64 here, 1e-12 relative
    to the densities' magnitude of ~n)."""
    X = load_golden("synthetic_512x64_T10.npz")["X"]
    U = O.l2_normalize(X)
    E = np.arange(10)
    delta = np.array([10, 11, 300, 511])
    before = O.density_canonical(X, E)
    after = O.density_canonical(X, np.union1d(E, delta))
    keep = ~O.exclusion_mask(X.shape[0], np.union1d(E, delta))
    dec = XR.density_decrement(U, delta)
    assert np.abs(before[keep] - dec[keep] - after[keep]).max() < 1e-12 * X.shape[0]
