"""column_similarities(threshold=): exact thresholded cosine pairs on the GPU
against the canonical fp64 definition (tests/pairs_reference.py).

Unless a test says otherwise it requires (i, j) equal to the reference as
arrays, order included, and ``value`` bit-equal.
"""
import numpy as np
import pytest

import pairs_reference as R
from conftest import load_golden
from oracle import dal_oracle as O

pytestmark = pytest.mark.gpu

BAND = 2.0 ** -10  # about the filter's error bound: the fp64 resolve decides pairs this close to tau


def _np(t):
    return t.detach().cpu().numpy()


def _call(pool, tau, cuda, **kw):
    from dal import similarity as sim

    i, j, v = sim.column_similarities(pool, threshold=tau, device=cuda, **kw)
    assert i.dtype.is_floating_point is False and str(v.dtype) == "torch.float64"
    return _np(i), _np(j), _np(v)


def _assert_equal(got, want):
    gi, gj, gv = got
    wi, wj, wv = want
    assert gi.shape == wi.shape, (gi.shape, wi.shape)
    assert np.array_equal(gi, wi) and np.array_equal(gj, wj)
    assert np.array_equal(gv.view(np.int64), wv.view(np.int64))  # bit-equal


# 1 -------------------------------------------------------------------------
SHAPES = [(1237, 64, "uniform"), (1237, 30, "normal"), (777, 256, "uniform"), (1237, 200, "uniform"),
          (600, 784, "uniform")]


@pytest.mark.parametrize("n,d,dist", SHAPES)
def test_parity_smallest_shapes_covering_every_path(cuda, n, d, dist):
    """Several row blocks (diagonal and off-diagonal tiles, padding rows in
    the last block), padding features (d = 30, 200, 784), a single K stage
    (d_pad 32) and many (d_pad 1024).  tau = the 2,000th largest reference
    value, so reference pairs lie within the filter's bound of tau on both
    sides and the fp64 resolve decides them."""
    X, S, tau = R.pool_reference(n, d, dist)
    _, _, v = R.upper_pairs(S)
    near = np.abs(v - tau) <= BAND
    print(f"{n}x{d} {dist}: tau={tau:.5f}, reference pairs within 2^-10 of tau: {int(near.sum())} "
          f"({int((near & (v >= tau)).sum())} at or above, {int((near & (v < tau)).sum())} below)")
    assert (near & (v >= tau)).sum() >= 10 and (near & (v < tau)).sum() >= 10
    want = R.threshold_pairs(S, tau)
    assert want[0].shape[0] == 2000
    _assert_equal(_call(X, tau, cuda), want)


# 2 -------------------------------------------------------------------------
def test_one_ulp_threshold(cuda):
    X, S, tau = R.pool_reference(1237, 64, "uniform")
    _, _, v = R.upper_pairs(S)
    assert (v >= tau).sum() == 2000 and (v == tau).sum() == 1  # no tie at that rank
    assert _call(X, tau, cuda)[0].shape[0] == 2000
    up = float(np.nextafter(tau, 2.0))
    got = _call(X, up, cuda)
    assert got[0].shape[0] == 1999
    _assert_equal(got, R.threshold_pairs(S, up))


# 3 -------------------------------------------------------------------------
def test_dense_hits(cuda):
    """Most of the 44,850 pairs pass: every wave reserves slots under load."""
    X = O.synthetic_pool(300, 30, seed=0, dist="normal")
    S = R.canonical_matrix(X)
    want = R.threshold_pairs(S, -0.2)
    assert want[0].shape[0] > 0.8 * 44850
    _assert_equal(_call(X, -0.2, cuda), want)


# 4 -------------------------------------------------------------------------
def test_duplicates_and_scaled_copies(cuda):
    """x_j = x_i and x_j = 2 x_i planted; the pairs and values are the
    reference's, whatever they come to (a canonical self-cosine need not be 1)."""
    X = O.synthetic_pool(700, 64, seed=0).copy()
    rng = np.random.default_rng(5)
    src = rng.choice(350, 40, replace=False)
    dst = 350 + rng.choice(350, 40, replace=False)
    X[dst[:20]] = X[src[:20]]
    X[dst[20:]] = 2.0 * X[src[20:]]
    S = R.canonical_matrix(X)
    want = R.threshold_pairs(S, 0.9999)
    planted = set(zip(np.minimum(src, dst).tolist(), np.maximum(src, dst).tolist()))
    assert planted <= set(zip(want[0].tolist(), want[1].tolist()))
    _assert_equal(_call(X, 0.9999, cuda), want)


# 5 -------------------------------------------------------------------------
def test_capacity_abi(cuda):
    """cap = 64 on the first shape: the flag is set, count is the candidate
    count of an unconstrained call, nothing is written past cap."""
    import torch

    from dal import _lib
    from dal import similarity as sim
    from dal.engine import PoolState, _ptr, _stream

    X, S, tau = R.pool_reference(1237, 64, "uniform")
    state = PoolState(X, device=cuda)
    keys, approx, count, status = sim.cosine_pair_candidates(state, tau, 1 << 16)
    n_all = int(count.item())
    assert 2000 <= n_all <= 1 << 16 and int(status.item()) == 0
    # every reference pair is a candidate, and every candidate's filter value is within the bound
    lib = _lib.load()
    bound = lib.dal_cosine_pairs_error_bound(64)
    k = _np(keys[:n_all])
    ci, cj = k >> 32, k & 0xFFFFFFFF
    assert np.all(ci < cj) and np.all(cj < 1237)
    assert np.abs(_np(approx[:n_all]).astype(np.float64) - S[ci, cj]).max() <= bound
    wi, wj, _ = R.threshold_pairs(S, tau)
    assert set(zip(wi.tolist(), wj.tolist())) <= set(zip(ci.tolist(), cj.tolist()))
    assert len(set(k.tolist())) == n_all  # no pair twice

    cap, guard = 64, 32
    SK, SA = 0x5A5A5A5A5A5A5A5A, -7.25
    keys = torch.full((cap + guard,), SK, dtype=torch.int64, device=cuda)
    approx = torch.full((cap + guard,), SA, dtype=torch.float32, device=cuda)
    count = torch.zeros(1, dtype=torch.int64, device=cuda)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    op = state.gram_operand()
    nb = state.n_pad // 256
    _lib.call("dal_cosine_pairs", _ptr(op), 0, nb, _ptr(op), 0, 0, nb, state.n, state.d_pad, 0, tau, cap,
              _ptr(keys), _ptr(approx), _ptr(count), _ptr(status), _stream(cuda))
    assert int(status.item()) & _lib.DAL_FLAG_CAND_OVERFLOW
    assert int(count.item()) == n_all
    assert np.all(_np(keys[cap:]) == SK) and np.all(_np(approx[cap:]) == SA)
    got = _np(keys[:cap])
    assert np.all(got != SK) and set(got.tolist()) <= set(k.tolist())


def test_capacity_python(cuda, monkeypatch):
    from dal import similarity as sim

    X, S, tau = R.pool_reference(1237, 64, "uniform")
    with pytest.raises(RuntimeError, match=r"max_pairs >= \d+"):
        sim.column_similarities(X, threshold=tau, device=cuda, max_pairs=64)
    # the default path with the initial capacity forced small: one retry, the full result
    calls = []
    real = sim.cosine_pair_candidates

    def counting(*a, **kw):
        calls.append(a[2])
        return real(*a, **kw)

    monkeypatch.setattr(sim, "PAIRS_INITIAL_CAP", 64)
    monkeypatch.setattr(sim, "cosine_pair_candidates", counting)
    got = _call(X, tau, cuda)
    assert len(calls) == 2 and calls[0] == 64 and calls[1] > 2000
    _assert_equal(got, R.threshold_pairs(S, tau))
    # a max_pairs that suffices
    monkeypatch.setattr(sim, "PAIRS_INITIAL_CAP", None)
    _assert_equal(_call(X, tau, cuda, max_pairs=calls[1]), R.threshold_pairs(S, tau))


# 6 -------------------------------------------------------------------------
SPLITS = {
    "rows-2": [((0, 2), (0, 6)), ((2, 6), (0, 6))],
    "cols-2": [((0, 6), (0, 3)), ((0, 6), (3, 6))],
    "rows-3": [((0, 1), (0, 6)), ((1, 4), (0, 6)), ((4, 6), (0, 6))],
    # cuts inside the diagonal: the column cut at block 3 crosses the rows of both row ranges
    "diag-3": [((0, 4), (0, 3)), ((0, 4), (3, 6)), ((4, 6), (0, 6))],
}


@pytest.mark.parametrize("name", sorted(SPLITS))
def test_range_split(cuda, name):
    import torch

    from dal import similarity as sim
    from dal.engine import PoolState

    X, S, tau = R.pool_reference(1237, 64, "uniform")
    state = PoolState(X, device=cuda)
    assert state.n_pad // 256 == 6
    keys, _, count, _ = sim.cosine_pair_candidates(state, tau, 1 << 16)
    whole = np.sort(_np(keys[: int(count.item())]))
    parts = []
    for rows, cols in SPLITS[name]:
        k, _, c, st = sim.cosine_pair_candidates(state, tau, 1 << 16, row_blocks=rows, col_blocks=cols)
        assert int(st.item()) == 0
        parts.append(k[: int(c.item())])
    cat = torch.cat(parts)
    assert np.array_equal(np.sort(_np(cat)), whole)  # the same candidates, none twice
    vals = sim.cosine_pair_values(state, cat, int(cat.shape[0]))
    keep = vals >= tau
    kk, order = torch.sort(cat[keep])
    _assert_equal((_np(kk >> 32), _np(kk & 0xFFFFFFFF), _np(vals[keep][order])), R.threshold_pairs(S, tau))


# 7 -------------------------------------------------------------------------
def test_excluded_rows(cuda):
    from dal.engine import PoolState

    X, S, tau = R.pool_reference(1237, 64, "uniform")
    tau = 0.80  # enough pairs that rows 0..9 would appear
    assert (R.threshold_pairs(S, tau)[0] < 10).any()
    state = PoolState(X, excluded=range(10), device=cuda)
    got = _call(state, tau, cuda)
    assert got[0].min() >= 10 and got[1].min() >= 10
    _assert_equal(got, R.threshold_pairs(S, tau, excluded=np.arange(10)))


def test_zero_row_and_tiny_pools(cuda):
    from dal import similarity as sim

    X = O.synthetic_pool(300, 30, seed=1).copy()
    X[17] = 0.0
    with pytest.raises(ValueError, match="zero-norm"):
        sim.column_similarities(X, threshold=0.5, device=cuda)
    one = _call(O.synthetic_pool(1, 30, seed=2), 0.1, cuda)
    assert one[0].shape == (0,) and one[2].shape == (0,)
    X2 = O.synthetic_pool(2, 30, seed=2)
    S2 = R.canonical_matrix(X2)
    _assert_equal(_call(X2, float(S2[0, 1]), cuda), R.threshold_pairs(S2, float(S2[0, 1])))
    assert _call(X2, float(np.nextafter(S2[0, 1], 2.0)), cuda)[0].shape == (0,)


# 8 -------------------------------------------------------------------------
def test_old_path_intact(cuda):
    """96 x 500 golden pool: the thresholded call at 0.5 returns the pair set
    of the dense column_similarities(pool) filtered at 0.5.  The dense values
    are fp32 MFMA sums, compared within the golden test's tolerance (2e-6);
    pairs whose dense value lies that close to 0.5 are left out of the set
    comparison (at most 1 % of the pairs)."""
    from dal import similarity as sim

    g = load_golden("similarity_96x500.npz")
    tol = 2e-6
    di, dj, dv = (_np(t) for t in sim.column_similarities(g["X"], device=cuda))
    assert np.array_equal(di, g["ci"]) and np.array_equal(dj, g["cj"])
    ref_v = R.upper_pairs(R.canonical_matrix(g["X"]))[2]
    assert (np.abs(ref_v - 0.5) <= 2 * tol).mean() <= 0.01
    ti, tj, tv = _call(g["X"], 0.5, cuda)
    assert ti.shape[0] > 0
    n = g["X"].shape[0]
    sure = np.abs(dv.astype(np.float64) - 0.5) > tol
    dense_set = set((di[sure & (dv >= 0.5)] * n + dj[sure & (dv >= 0.5)]).tolist())
    unsure = set((di[~sure] * n + dj[~sure]).tolist())
    thr_set = set((ti * n + tj).tolist())
    assert thr_set - unsure == dense_set
    dense = np.zeros((n, n))
    dense[di, dj] = dv
    assert np.abs(dense[ti, tj] - tv).max() <= tol


# 9 -------------------------------------------------------------------------
def test_size_the_dense_path_cannot_reach(cuda):
    """n = 65,573 (the dense matrix alone would be 17 GB), d = 64, uniform,
    seed 0.  Construction: with rng = default_rng(7), dst = 500 distinct rows
    of the upper half (rng.choice), src = 500 rows of the lower half
    (rng.integers), s ~ U(0.05, 0.30), then X[dst] = X[src] + s * N(0, 1) in
    fp32.  tau = 0.95: planted pairs fall on both sides, natural pairs at that
    level are absent or very rare."""
    n, d, tau = 65573, 64, 0.95
    X = O.synthetic_pool(n, d, seed=0).copy()
    rng = np.random.default_rng(7)
    dst = n // 2 + rng.choice(n - n // 2, 500, replace=False)
    src = rng.integers(0, n // 2, 500)
    s = rng.uniform(0.05, 0.30, 500)
    X[dst] = (X[src] + s[:, None] * rng.standard_normal((500, d))).astype(np.float32)
    U = O.l2_normalize(X)
    pv = R.canonical_values(U, src, dst)
    print(f"planted: {int((pv >= tau).sum())} at or above tau, {int((pv < tau).sum())} below, "
          f"{int((np.abs(pv - tau) <= BAND).sum())} within 2^-10")
    assert (pv >= tau).sum() >= 50 and (pv < tau).sum() >= 50

    gi, gj, gv = _call(X, tau, cuda)
    assert np.all(gi < gj) and np.all(gv >= tau)
    key = gi * n + gj
    assert np.all(np.diff(key) > 0)  # sorted by (i, j), no pair twice
    assert np.array_equal(gv.view(np.int64), R.canonical_values(U, gi, gj).view(np.int64))
    got = set(key.tolist())
    assert set((src[pv >= tau] * n + dst[pv >= tau]).tolist()) <= got

    # completeness on 2,048 sampled rows against all columns
    rows = np.sort(np.random.default_rng(11).choice(n, 2048, replace=False))
    want = _pairs_of_rows(U, rows, tau, 256)
    assert want <= got
    in_rows = np.isin(gi, rows) | np.isin(gj, rows)
    assert set(key[in_rows].tolist()) == want


def _pairs_of_rows(U, rows, tau, chunk):
    """Keys i * n + j (i < j) of every pair with one row in ``rows`` whose
    canonical cosine is >= tau: an fp64 BLAS product against all columns,
    entries within 1e-9 of tau re-decided by the sequential sum."""
    n = U.shape[0]
    want = set()
    for b0 in range(0, rows.shape[0], chunk):
        r = rows[b0:b0 + chunk]
        P = U[r] @ U.T
        P[np.arange(r.shape[0]), r] = -2.0  # no self pairs
        a, c = np.nonzero(P >= tau - 1e-9)
        near = np.abs(P[a, c] - tau) <= 1e-9
        ok = P[a, c] >= tau
        if near.any():
            ok[near] = R.canonical_values(U, r[a[near]], c[near]) >= tau
        ri, cj = r[a[ok]], c[ok]
        want |= set((np.minimum(ri, cj) * n + np.maximum(ri, cj)).tolist())
    return want


# 10 ------------------------------------------------------------------------
def test_more_tiles_than_one_grid_dimension_holds(cuda):
    """n = 741,889 rows are 2,898 blocks, 4.2M block pairs, 16.8M tiles of 256
    threads: past the 2^32 threads one grid dimension holds, so a launch that
    is not split over two dimensions loses the tiles of the last rows.  d = 30,
    N(0, 1), seed 0; with rng = default_rng(9): 200 rows dst of the last 20,000
    are overwritten by X[src] + s * N(0, 1), s ~ U(0.05, 0.30), src = 100 rows
    of the last 40,000..20,000 and 100 of the first 20,000.  tau = 0.97 (5.3 sd
    of a natural pair's cosine: none expected)."""
    n, d, tau = 741_889, 30, 0.97
    X = O.synthetic_pool(n, d, seed=0, dist="normal").copy()
    rng = np.random.default_rng(9)
    dst = n - 20_000 + rng.choice(20_000, 200, replace=False)
    src = np.concatenate([n - 40_000 + rng.integers(0, 20_000, 100), rng.integers(0, 20_000, 100)])
    s = rng.uniform(0.05, 0.30, 200)
    X[dst] = (X[src] + s[:, None] * rng.standard_normal((200, d))).astype(np.float32)
    U = O.l2_normalize(X)
    pv = R.canonical_values(U, src, dst)
    print(f"planted: {int((pv >= tau).sum())} at or above tau, {int((pv < tau).sum())} below")
    assert (pv >= tau).sum() >= 20 and (pv < tau).sum() >= 20

    gi, gj, gv = _call(X, tau, cuda)
    assert np.all(gi < gj) and np.all(gv >= tau)
    key = gi * n + gj
    assert np.all(np.diff(key) > 0)
    assert np.array_equal(gv.view(np.int64), R.canonical_values(U, gi, gj).view(np.int64))
    got = set(key.tolist())
    assert set((src[pv >= tau] * n + dst[pv >= tau]).tolist()) <= got
    # completeness on 192 rows: the very last ones, and sampled rows of the last 20,000
    rows = np.unique(np.concatenate([np.arange(n - 64, n), n - 20_000 + rng.choice(20_000, 128, replace=False)]))
    want = _pairs_of_rows(U, rows, tau, 32)
    assert want <= got
    in_rows = np.isin(gi, rows) | np.isin(gj, rows)
    assert set(key[in_rows].tolist()) == want
