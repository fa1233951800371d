"""LAL query selection on the GPU: the regression-forest kernel, the vote
histogram, the feature rows, the rescore, select_lal end to end, its sharded
form and the loop -- each against tests/lal_reference.py, bit for bit (every
value is an integer or an IEEE fp64 add / multiply / divide in a fixed order,
so there is no tolerance)."""
import functools

import numpy as np
import pytest

import lal_reference as L
from conftest import load_golden
from dal import _lib
from dal.forest import Forest, RegressionForest

pytestmark = pytest.mark.gpu


def _dev(a, cuda):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _stream(cuda):
    import torch

    return torch.cuda.current_stream(cuda).cuda_stream


def _regress(model, x, n, d, ldx, cuda):
    """dal_forest_regress over the first n rows of the device tensor x."""
    import torch

    feat, thr, leaf = model.device(cuda)
    out = torch.full((max(n, 1),), -7.0, dtype=torch.float64, device=cuda)
    _lib.call("dal_forest_regress", x.data_ptr(), _lib.DAL_X_F64 if x.dtype == torch.float64 else _lib.DAL_X_F32,
              n, d, ldx, feat.data_ptr(), thr.data_ptr(), leaf.data_ptr(), model.n_trees, model.depth,
              out.data_ptr(), _stream(cuda))
    return out.cpu().numpy()[:n]


def _wide_forest(TR, depth, d, seed):
    """RegressionForest.synthetic (+-10^e leaves) with a tenth of the leaves
    forced to 0.0 and -0.0."""
    F = RegressionForest.synthetic(TR, depth, d, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    u = rng.random(F.leaf.shape)
    F.leaf[u < 0.05] = 0.0
    F.leaf[(u >= 0.05) & (u < 0.10)] = -0.0
    return F


def _rows(n, d, ldx, f64, model, seed):
    """[n, ldx] rows; fp64: some entries exactly on a root threshold and some
    one ulp above it (the <=, and no fp32 rounding of the threshold)."""
    rng = np.random.default_rng(seed)
    X = rng.random((n, ldx))
    if not f64:
        return X.astype(np.float32)
    for t in range(min(model.n_trees, 8)):
        f, thr = int(model.inner_feature[t, 0]), float(model.inner_threshold[t, 0])
        for r in range(4 * t, min(4 * t + 2, n)):
            X[r, f] = thr
        for r in range(4 * t + 2, min(4 * t + 4, n)):
            X[r, f] = np.nextafter(thr, np.inf)
    return X


def _chunk(depth):
    return int(_lib.load().dal_forest_regress_chunk_trees(depth))


N_ROWS = (1, 63, 65, 1000)


def _check_regress(model, d, ldx, f64, cuda, seed, ns=N_ROWS):
    X = _rows(max(ns), d, ldx, f64, model, seed)
    ref = L.regress(model, X[:, :d])  # once, shared by every n (a row's value does not depend on n)
    xd = _dev(X, cuda)
    for n in ns:
        got = _regress(model, xd, n, d, ldx, cuda)
        assert L.bits_equal(got, ref[:n]), (n, np.flatnonzero(got != ref[:n])[:5])


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("d,ldx", [(5, 5), (37, 40)])
@pytest.mark.parametrize("tr", ["1", "7", "c-1", "c", "c+1", "2c+3"])
def test_regress_parity_depth4(cuda, tr, d, ldx, f64):
    c = _chunk(4)
    TR = {"1": 1, "7": 7, "c-1": c - 1, "c": c, "c+1": c + 1, "2c+3": 2 * c + 3}[tr]
    _check_regress(_wide_forest(TR, 4, d, seed=TR), d, ldx, f64, cuda, seed=TR + d)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("depth,TR", [(1, 9), (6, None), (10, 3)])
def test_regress_parity_other_depths(cuda, depth, TR, f64):
    TR = _chunk(depth) + 1 if TR is None else TR
    _check_regress(_wide_forest(TR, depth, 5, seed=depth), 5, 5, f64, cuda, seed=depth)
    _check_regress(_wide_forest(TR, depth, 37, seed=depth + 50), 37, 40, f64, cuda, seed=depth + 1, ns=(65,))


def test_regress_parity_sklearn_ragged(cuda):
    from sklearn.ensemble import RandomForestRegressor

    rng = np.random.default_rng(5)
    X = rng.random((400, 6)).astype(np.float32)
    y = np.sin(6 * X[:, 0]) + X[:, 1] * X[:, 2] + 0.1 * rng.standard_normal(400)
    rf = RandomForestRegressor(n_estimators=9, max_depth=5, min_samples_leaf=8, random_state=0).fit(X, y)
    F = RegressionForest.from_sklearn(rf)
    assert np.isposinf(F.inner_threshold).any()  # ragged: some shallow leaves were padded
    ref = L.regress(F, X)
    assert L.bits_equal(_regress(F, _dev(X, cuda), 400, 6, 6, cuda), ref)
    assert L.bits_equal(_regress(F, _dev(X.astype(np.float64), cuda), 400, 6, 6, cuda), ref)


def test_regress_nan_feature_goes_right(cuda):
    F = _wide_forest(5, 3, 5, seed=2)
    X = np.random.default_rng(2).random((70, 5))
    X[::3, 1] = np.nan
    X[5, :] = np.nan
    assert L.bits_equal(_regress(F, _dev(X, cuda), 70, 5, 5, cuda), L.regress(F, X))


# ------------------------------------------------------ histogram and rows
def _hist_and_rows(cuda, v, flags, T, n_labeled, n_positive, halves=False):
    import torch

    from dal.active_learner import lal_tables

    n = v.shape[0]
    vd = _dev(v.astype(np.int32), cuda)
    fd = None if flags is None else _dev(flags, cuda)
    hist = torch.zeros(T + 1, dtype=torch.int64, device=cuda)
    parts = [(0, n // 2), (n // 2, n)] if halves else [(0, n)]
    for a, b in parts:
        _lib.call("dal_vote_histogram", vd.data_ptr() + 4 * a, 0 if fd is None else fd.data_ptr() + a, b - a, T,
                  hist.data_ptr(), _stream(cuda))
    f1, f2 = (_dev(t, cuda) for t in lal_tables(T))
    rows = torch.empty((T + 1, 5), dtype=torch.float64, device=cuda)
    _lib.call("dal_lal_rows", hist.data_ptr(), f1.data_ptr(), f2.data_ptr(), T, float(n_positive) / n_labeled,
              float(n_labeled), rows.data_ptr(), _stream(cuda))
    return hist.cpu().numpy(), rows.cpu().numpy()


@pytest.mark.parametrize("with_flags", [True, False], ids=["flags", "null"])
@pytest.mark.parametrize("n", [1, 64, 4097])
@pytest.mark.parametrize("T", [2, 10, 50])
def test_histogram_and_rows(cuda, T, n, with_flags):
    rng = np.random.default_rng(T * 10000 + n)
    v = rng.binomial(T, 0.3, size=n)
    flags = None
    if with_flags:  # a third of the rows are not candidates (some EXCLUDED instead)
        flags = np.where(rng.random(n) < 1 / 3, rng.choice([0, _lib.DAL_ROW_EXCLUDED], size=n),
                         _lib.DAL_ROW_CANDIDATE).astype(np.uint8)
        if n == 1:
            flags[:] = _lib.DAL_ROW_CANDIDATE
    mask = None if flags is None else (flags & _lib.DAL_ROW_CANDIDATE) != 0
    ref_h = L.histogram(v, T, mask)
    hist, rows = _hist_and_rows(cuda, v, flags, T, 37, 11)
    assert np.array_equal(hist, ref_h) and hist.sum() == (n if mask is None else mask.sum())
    assert L.bits_equal(rows, L.lal_rows(ref_h, T, 37, 11))


def test_histogram_uniform_votes_and_accumulation(cuda):
    T = 10
    v = np.full(5000, 7)
    hist, rows = _hist_and_rows(cuda, v, None, T, 20, 20)
    assert np.array_equal(hist, L.histogram(v, T))
    assert L.bits_equal(rows, L.lal_rows(hist, T, 20, 20))
    rng = np.random.default_rng(8)
    v = rng.binomial(T, 0.6, size=4097)
    flags = np.where(rng.random(4097) < 1 / 3, 0, _lib.DAL_ROW_CANDIDATE).astype(np.uint8)
    hist, rows = _hist_and_rows(cuda, v, flags, T, 50, 3, halves=True)  # two accumulating calls
    ref_h = L.histogram(v, T, flags != 0)
    assert np.array_equal(hist, ref_h)
    assert L.bits_equal(rows, L.lal_rows(ref_h, T, 50, 3))


# ------------------------------------------------------------------ rescore
@pytest.mark.parametrize("order", [_lib.DAL_ASCENDING, _lib.DAL_DESCENDING], ids=["asc", "desc"])
def test_rescore_matches_forest_score(cuda, order):
    import torch

    from dal import engine

    rng = np.random.default_rng(12)
    T, n = 10, 1500
    X = rng.random((n, 16)).astype(np.float32)
    F = Forest.synthetic(T, 4, 16, seed=3)
    lut = rng.standard_normal(T + 1)
    lut[2], lut[4], lut[5] = np.nan, -0.0, 0.0
    lut_d = _dev(lut, cuda)
    state = engine.PoolState(X, device=cuda)
    flags_h = np.where(rng.random(n) < 1 / 3, 0, _lib.DAL_ROW_CANDIDATE).astype(np.uint8)
    flags = _dev(flags_h, cuda)
    votes, sc_ref, keys_ref, _ = engine.forest_score(state, F, lut_d, flags, order)
    assert len(np.unique(votes.cpu().numpy())) >= 5
    for fl in (flags, None):
        if fl is None:
            votes, sc_ref, keys_ref, _ = engine.forest_score(
                state, F, lut_d, torch.full((n,), _lib.DAL_ROW_CANDIDATE, dtype=torch.uint8, device=cuda), order)
        sc = torch.empty(n, dtype=torch.float64, device=cuda)
        keys = torch.empty(n, dtype=torch.int64, device=cuda)
        _lib.call("dal_votes_rescore", votes.data_ptr(), 0 if fl is None else fl.data_ptr(), n, lut_d.data_ptr(), T,
                  order, sc.data_ptr(), keys.data_ptr(), _stream(cuda))
        assert np.array_equal(sc.cpu().numpy().view(np.int64), sc_ref.cpu().numpy().view(np.int64))
        assert np.array_equal(keys.cpu().numpy(), keys_ref.cpu().numpy())


# --------------------------------------------------------------- select_lal
N_POOL, D_POOL, N_LABELED, N_POSITIVE = 3000, 16, 37, 11
FOREST_T = (2, 10, 50)


@functools.lru_cache(maxsize=None)
def _pool():
    X = np.random.default_rng(21).random((N_POOL, D_POOL)).astype(np.float32)
    unl = np.setdiff1d(np.arange(N_POOL), np.arange(0, N_POOL, 7))  # a strict subset
    unl = unl[np.random.default_rng(22).permutation(unl.size)]
    return X, unl


@functools.lru_cache(maxsize=None)
def _classifier(T):
    return Forest.synthetic(T, 4, D_POOL, seed=30 + T)


@functools.lru_cache(maxsize=None)
def _f6_range():
    """The values f6 takes over the tests' forests, from the reference."""
    X, unl = _pool()
    vals = []
    for T in FOREST_T:
        h = L.histogram(L.votes(_classifier(T), X[unl]), T)
        vals.append(L.lal_rows(h, T, N_LABELED, N_POSITIVE)[0, 3])
    return min(vals), max(vals)


@functools.lru_cache(maxsize=None)
def _lal_model(TR, f8=float(N_LABELED)):
    """A regressor over the five LAL features whose thresholds lie where the
    features do: f2 in [0, 0.75], f6 (feature 3) inside the range it actually
    takes here, f8 around the labeled count -- so every feature decides
    branches."""
    F = _wide_forest(TR, 4, 5, seed=40 + TR)
    lo, hi = _f6_range()
    u = F.inner_threshold
    F.inner_threshold = np.where(F.inner_feature == 1, 0.75 * u, u)
    F.inner_threshold = np.where(F.inner_feature == 3, lo - 0.05 * (hi - lo) + 1.1 * (hi - lo) * u,
                                 F.inner_threshold)
    F.inner_threshold = np.where(F.inner_feature == 4, 2.0 * f8 * u, F.inner_threshold)
    return F


def _regressor_sizes():
    return (7, 2 * _chunk(4) + 3)


@functools.lru_cache(maxsize=None)
def _reference(T, TR, k):
    X, unl = _pool()
    return L.select_lal(X, unl, _classifier(T), _lal_model(TR), k, N_LABELED, N_POSITIVE)


def _k_values():
    return (1, 10, _pool()[1].size)


def _assert_reference_is_a_test(T, TR):
    """The reference LUT takes at least 3 values over occupied vote counts and
    f6 decides a branch (another f6 gives another LUT)."""
    scores, _, _, v, lut = _reference(T, TR, 1)
    assert len(set(lut[np.unique(v)].view(np.int64).tolist())) >= 3
    rows = L.lal_rows(L.histogram(v, T), T, N_LABELED, N_POSITIVE)
    lo, hi = _f6_range()
    assert lo <= rows[0, 3] <= hi
    rows[:, 3] = hi + 1.0
    assert not L.bits_equal(L.regress(_lal_model(TR), rows), lut)


@pytest.mark.parametrize("big", [False, True], ids=["TR7", "TR2c+3"])
@pytest.mark.parametrize("T", FOREST_T)
def test_select_lal_end_to_end(cuda, T, big):
    from dal import engine
    from dal.active_learner import select_lal

    TR = _regressor_sizes()[big]
    X, unl = _pool()
    _assert_reference_is_a_test(T, TR)
    state = engine.PoolState(X, device=cuda)
    for call_no, k in enumerate(_k_values() + (10,)):  # the last call: the same PoolState again
        scores, idx, sel_sc, v, lut = _reference(T, TR, k)
        sel = select_lal(state, unl, _classifier(T), _lal_model(TR), k, N_LABELED, N_POSITIVE)
        assert np.array_equal(sel.votes.cpu().numpy(), v.astype(np.int32))
        assert L.bits_equal(sel.lut.cpu().numpy(), lut)
        assert L.bits_equal(sel.scores.cpu().numpy(), scores)
        assert np.array_equal(sel.indices.cpu().numpy(), idx)
        assert L.bits_equal(sel.selected_scores.cpu().numpy(), sel_sc)
        if call_no == 0:
            assert state._xb is None  # the first step on a pool: the row-major vote kernel
    # from the second step on the votes came from the blocked copy
    assert (state._xb is not None) == bool(_lib.load().dal_forest_blocked_rows(D_POOL, T, 4))
    if T == 10:
        assert state._xb is not None


def test_select_lal_reference_exercises_ties():
    """For at least one parametrisation the k-th and (k+1)-th reference scores
    tie, so the lower-index rule decides the selection."""
    X, unl = _pool()
    tied = 0
    for T in FOREST_T:
        for TR in _regressor_sizes():
            scores, _, _, _, _ = _reference(T, TR, 1)
            o = L.order_desc(scores, unl)
            for k in _k_values():
                if k < unl.size and scores[o[k - 1]] == scores[o[k]]:
                    tied += 1
    assert tied >= 1


def test_select_lal_argument_errors(cuda):
    from dal.active_learner import select_lal

    X, unl = _pool()
    with pytest.raises(ValueError):
        select_lal(X, unl, Forest.synthetic(5, 4, D_POOL, n_classes=3), _lal_model(7), 5, 10, 3, device=cuda)
    with pytest.raises(ValueError):
        select_lal(X, unl, Forest.synthetic(1, 4, D_POOL), _lal_model(7), 5, 10, 3, device=cuda)
    with pytest.raises(ValueError):
        bad = RegressionForest.synthetic(3, 2, 5)
        bad.inner_feature[0, 0] = 5  # a sixth feature: the LAL rows have five
        select_lal(X, unl, _classifier(10), bad, 5, 10, 3, device=cuda)
    with pytest.raises(ValueError):
        select_lal(X, np.zeros(0, dtype=np.int64), _classifier(10), _lal_model(7), 5, 10, 3, device=cuda)


# ------------------------------------------------------------------ sharded
@pytest.mark.parametrize("P", [1, 2, 3])
def test_emulate_lal_matches_single_gpu(cuda, P):
    from dal import parallel

    T, TR, k = 10, _regressor_sizes()[1], 10
    X, unl = _pool()
    _, idx, sel_sc, _, _ = _reference(T, TR, k)
    sels = []
    for r in range(P):
        lo, hi, _ = parallel.shard_range(N_POOL, P, r)
        sels.append(parallel.ShardedSelector(X[lo:hi], N_POOL, r, P, device=cuda))
    if P > 1:
        assert len({s.state.n for s in sels}) > 1  # uneven shards
    got_idx, got_sc = parallel.emulate_lal(sels, unl, _classifier(T), _lal_model(TR), k, N_LABELED, N_POSITIVE)
    assert np.array_equal(got_idx.cpu().numpy(), idx)
    assert L.bits_equal(got_sc.cpu().numpy(), sel_sc)


def _lal_rank(rank, world):
    """parallel.select_lal on one of two ranks sharing cuda:0 (collectives
    over gloo), its collectives counted; rank 0 also runs the single-device
    step and emulate_lal over the same two shards."""
    import torch

    from dal import parallel
    from dal.active_learner import select_lal
    from sharded_comm import CountingComm

    T, TR, k = 10, _regressor_sizes()[1], 10
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    X, unl = _pool()
    args = (unl, _classifier(T), _lal_model(TR), k, N_LABELED, N_POSITIVE)
    shards = [parallel.shard_range(N_POOL, world, r)[:2] for r in range(world)]
    lo, hi = shards[rank]
    comm = CountingComm()
    idx, sc = parallel.select_lal(parallel.ShardedSelector(X[lo:hi], N_POOL, rank, world, device=dev), comm, *args)
    out = {"counts": comm.take(), "ranks": (idx.cpu().numpy(), sc.cpu().numpy())}
    if rank == 0:
        one = select_lal(X, *args, device=dev)
        out["one"] = (one.indices.cpu().numpy(), one.selected_scores.cpu().numpy())
        sels = [parallel.ShardedSelector(X[a:b], N_POOL, r, world, device=dev) for r, (a, b) in enumerate(shards)]
        idx, sc = parallel.emulate_lal(sels, *args)
        out["emulated"] = (idx.cpu().numpy(), sc.cpu().numpy())
    return out


def test_select_lal_on_two_ranks(cuda):
    """parallel.select_lal over a real group: the single-device selection and
    emulate_lal's, byte for byte, with one all-reduce and one all-gather."""
    from sharded_comm import run_ranks

    res = run_ranks(_lal_rank, 2)
    for name in ("one", "emulated"):
        for out in res:
            assert np.array_equal(out["ranks"][0], res[0][name][0]), name
            assert L.bits_equal(out["ranks"][1], res[0][name][1]), name
    assert [out["counts"] for out in res] == [(1, 1), (1, 1)]


# ------------------------------------------------------- predict_regression
def test_predict_regression(cuda):
    from dal import engine
    from dal.random_forest import predict_regression

    X, _ = _pool()
    F = _wide_forest(2 * _chunk(4) + 3, 4, D_POOL, seed=77)
    ref32 = L.regress(F, X)
    assert L.bits_equal(predict_regression(F, engine.PoolState(X, device=cuda)).cpu().numpy(), ref32)
    X64 = np.random.default_rng(78).random((777, D_POOL))
    assert L.bits_equal(predict_regression(F, X64, device=cuda).cpu().numpy(), L.regress(F, X64))


# --------------------------------------------------------------------- loop
def test_lal_loop_matches_reference_loop(cuda):
    from dal import loop

    g = load_golden("checkerboard2x2.npz")
    X, y = g["X"], g["y"]
    model = _lal_model(7, f8=20.0)
    n = X.shape[0]

    def ref_select(strategy, pool, unlabeled, rf, k):
        assert strategy == "lal"
        lab = np.setdiff1d(np.arange(n), unlabeled)
        return L.select_lal(pool, unlabeled, rf.forest, model, k, lab.size, int(y[lab].sum()))[1]

    kw = dict(strategy="lal", lal_model=model, trainer="gpu", max_iterations=3, window_size=10, device=cuda)
    ref = loop.run_loop(X, y, X, y, select_fn=ref_select, **kw)
    got = loop.run_loop(X, y, X, y, **kw)
    assert got.log == ref.log
    assert len(got.labeled_history) == 3
    for a, b in zip(got.labeled_history, ref.labeled_history):
        assert np.array_equal(a, b)
