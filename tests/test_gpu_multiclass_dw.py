"""Multiclass information density on the GPU: dal_forest_score_multiclass_dw
(class entropy x density^beta, interval keys, the per-row entropy and identity
index) and everything above it, against the NumPy restatement of the
canonical semantics (tests/multiclass_dw_reference.py).  E = range(10) and
unlabeled = range(10, n) unless a test says otherwise."""
import functools

import numpy as np
import pytest

import multiclass_dw_reference as DW
import multiclass_reference as R
from dal import _lib
from dal.forest import Forest
from oracle import dal_oracle as O

pytestmark = pytest.mark.gpu

KEY_NONE = DW.KEY_NONE
E = np.arange(10)

# (n, d, T, depth, C): the smallest shape of each launcher path
#   1,037 x 30   scalar staging, ragged last block, byte count stores
#   1,037 x 13   256-row tiles, tpr 1
#   3,001 x 64   16-byte staging, tpr 4, CW 4
#   2,500 x 256  LDS-DMA, persistent grid
#   700 x 1,100  rows from global memory
#   600 x 40     forest from global memory, CW 8
SHAPES = [
    (1037, 30, 10, 4, 3),
    (1037, 13, 10, 4, 3),
    (3001, 64, 100, 4, 10),
    (2500, 256, 10, 4, 10),
    (700, 1100, 10, 3, 4),
    (600, 40, 255, 8, 32),
]


class Case:
    """A pool, a forest and their reference quantities (computed once, never written)."""

    def __init__(self, X, F):
        self.X, self.F, self.n, self.T = X, F, X.shape[0], F.n_trees
        self.cnt = R.counts(F, X)
        self.H = DW.entropy(self.cnt, self.T)
        self.d = O.density_canonical(X, E)
        self.s = DW.scores(self.H, self.d)
        self.unl = np.arange(10, self.n)
        for a in (self.cnt, self.H, self.d, self.s):
            a.setflags(write=False)

    def select(self, unl, k, beta=1.0):
        return DW.select(self.X, unl, self.F, k, beta=beta, density=self.d, cnt=self.cnt)


@functools.lru_cache(maxsize=None)
def _case(n, d, T, depth, C):
    return Case(O.synthetic_pool(n, d, seed=n % 97), Forest.synthetic(T, depth, d, seed=5, n_classes=C))


def _flags(state, seed):
    """The pool's EXCLUDED bits | DAL_ROW_CANDIDATE on ~70 % of the rows (seeded)."""
    cand = (np.random.default_rng(seed).random(state.n) < 0.7).astype(np.uint8)
    return state.flags.cpu().numpy() | cand * np.uint8(_lib.DAL_ROW_CANDIDATE)


def _launch(cuda, state, F, flags, density, kind, derr=0.0, beta=1.0):
    """One launch through the engine; numpy outputs, keys as uint64."""
    import torch

    from dal import engine

    out = engine.forest_score_multiclass_dw(state, F, torch.from_numpy(flags).to(cuda), density, kind, derr, beta,
                                            True)
    c, p, e, ix, s, klo, khi = (t.cpu().numpy() for t in out)
    return c, p, e, ix, s, klo.view(np.uint64), khi.view(np.uint64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_exact(cuda, case, state):
    """DAL_DENSITY_EXACT, beta = 1: every output equals the reference bit for bit."""
    n = case.n
    assert not np.isnan(case.H).any() and (case.cnt.sum(axis=1) == case.T).all()
    assert np.array_equal(np.isnan(case.d), np.isin(np.arange(n), E))
    flags = _flags(state, 11)
    c, p, e, ix, s, klo, khi = _launch(cuda, state, case.F, flags, state.density_exact(), _lib.DAL_DENSITY_EXACT)
    assert c.dtype == np.uint8 and np.array_equal(c, case.cnt)
    assert np.array_equal(p, R.pred(case.cnt))
    assert np.array_equal(_bits(e), _bits(case.H))
    assert ix.dtype == np.int32 and np.array_equal(ix, np.arange(n))
    ex = np.isin(np.arange(n), E)
    assert np.array_equal(np.isnan(s), ex)
    assert np.array_equal(_bits(s[~ex]), _bits(case.s[~ex]))
    assert np.array_equal(khi, klo)
    cand = (flags & _lib.DAL_ROW_CANDIDATE) != 0
    assert np.array_equal(klo == KEY_NONE, ~cand)
    assert np.array_equal(klo[cand], DW.score_key(case.s)[cand])


def _check_enclosure(cuda, case, state):
    """DAL_DENSITY_FIXED (the Gram density): the interval keys enclose the
    canonical score's key -- what makes the exact selection valid."""
    from dal import engine

    n = case.n
    flags = _flags(state, 12)
    derr = engine.density_error(state)
    assert derr > 0.0
    c, p, e, ix, s, klo, khi = _launch(cuda, state, case.F, flags, state.density_fixed(), _lib.DAL_DENSITY_FIXED,
                                       derr)
    assert np.array_equal(c, case.cnt) and np.array_equal(_bits(e), _bits(case.H))
    assert np.array_equal(ix, np.arange(n))
    cand = (flags & _lib.DAL_ROW_CANDIDATE) != 0
    assert np.array_equal(klo == KEY_NONE, ~cand) and np.array_equal(khi == KEY_NONE, ~cand)
    m = cand & ~np.isin(np.arange(n), E)
    assert m.sum() > n // 2
    ref, H = case.s[m], case.H[m]
    assert (np.abs(s[m] - ref) <= H * derr + 1e-15 * np.abs(ref)).all()
    key = DW.score_key(ref)
    assert (khi[m] <= key).all() and (key <= klo[m]).all()
    assert np.array_equal(khi[m] == klo[m], H == 0.0)
    ex = cand & np.isin(np.arange(n), E)  # an excluded candidate: NaN, a point interval
    assert (klo[ex] == DW.KEY_NAN).all() and (khi[ex] == DW.KEY_NAN).all()


def _state(cuda, X):
    from dal.engine import PoolState

    return PoolState(X, excluded=E, device=cuda)


@pytest.mark.parametrize("n,d,T,depth,C", SHAPES)
def test_kernel_outputs_exact_density(cuda, n, d, T, depth, C):
    case = _case(n, d, T, depth, C)
    _check_exact(cuda, case, _state(cuda, case.X))


@pytest.mark.parametrize("n,d,T,depth,C", SHAPES)
def test_interval_enclosure_fixed_density(cuda, n, d, T, depth, C):
    case = _case(n, d, T, depth, C)
    _check_enclosure(cuda, case, _state(cuda, case.X))


def test_dma_block_walks_two_tiles(cuda):
    """LDS-DMA at d = 128 (64-row tiles) with more tiles than twice the
    resident grid (n derived as tests/test_gpu_multiclass.py does): every
    block of the persistent grid loads a second tile's flags and density
    words.  DAL_DENSITY_EXACT: no Gram at this size."""
    import torch

    d, T, depth, C, rows = 128, 10, 4, 10, 64
    lds = rows * (d + 4) * 4 + (T + 2) * 8 + T * (((1 << depth) - 1) * 8 + (1 << depth))
    per_cu = (160 * 1024) // lds
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    n = min(2 * cus * per_cu * rows + 37, 400_000)
    assert n > cus * per_cu * rows  # the second tile of at least one block, whatever the cap
    case = Case(O.synthetic_pool(n, d, seed=3), Forest.synthetic(T, depth, d, seed=6, n_classes=C))
    _check_exact(cuda, case, _state(cuda, case.X))


def _check_selection(cuda, case, state, calls, mode, beta=1.0, rtol=0.0):
    from dal import density_weighting as dw

    for unl, k in calls:
        sel = dw.select_multiclass(state, unl, case.F, k, beta=beta, mode=mode)
        _, ref_idx, ref_sc, ref_cnt = case.select(unl, k, beta)
        assert ref_idx.shape[0] == min(k, unl.shape[0])
        assert np.array_equal(sel.indices.cpu().numpy(), ref_idx), (mode, k)
        got = sel.selected_scores.cpu().numpy()
        if rtol:
            assert np.allclose(got, ref_sc, rtol=rtol, atol=0.0), (mode, k)
        else:
            assert np.array_equal(_bits(got), _bits(ref_sc)), (mode, k)
        assert sel.votes is None
        assert np.array_equal(sel.counts.cpu().numpy(), ref_cnt)
        assert sel.scores.shape[0] == unl.shape[0]


@pytest.mark.parametrize("n,d,T,depth,C", SHAPES)
def test_selection(cuda, n, d, T, depth, C):
    """select_multiclass, gram (cold, then two warm calls on one PoolState)
    and separable: k = 1 and 100 over a two-thirds subset, k = 100 over 40
    rows (clamped)."""
    case = _case(n, d, T, depth, C)
    rng = np.random.default_rng(n)
    subset = np.sort(rng.choice(case.unl, size=(2 * case.unl.size) // 3, replace=False))
    few = np.sort(rng.choice(case.unl, size=40, replace=False))
    # preconditions, on the CPU: no zero-entropy tie, a strict positive top 100
    assert (case.H[case.unl] > 0.0).all()
    top = case.select(subset, 100)[2]
    assert np.unique(top).size == 100 and (top > 0.0).all()
    calls = ((subset, 1), (subset, 100), (few, 100))
    state = _state(cuda, case.X)
    _check_selection(cuda, case, state, calls, "gram")
    assert state._density is not None  # the second and third calls were warm
    _check_selection(cuda, case, _state(cuda, case.X), calls, "separable")


def test_zero_entropy_ties(cuda):
    """A skewed forest: most rows have H == 0.  k = 100 stays among positive
    scores; k = 300 crosses into the +0.0 point intervals, where the lowest
    indices win."""
    n, d, T, depth, C = 3000, 40, 10, 4, 4
    case = Case(O.synthetic_pool(n, d, seed=4), Forest.synthetic(T, depth, d, seed=8, n_classes=C, skew=0.97))
    pos = int((case.H[case.unl] > 0.0).sum())
    assert 200 < pos < 300 and (case.d[case.unl] > 0.0).all()
    _, idx300, sc300, _ = case.select(case.unl, 300)
    assert (sc300[:pos] > 0.0).all() and (sc300[pos:] == 0.0).all()
    zero_rows = case.unl[case.H[case.unl] == 0.0]
    assert np.array_equal(idx300[pos:], zero_rows[:300 - pos])
    calls = ((case.unl, 100), (case.unl, 300))
    _check_selection(cuda, case, _state(cuda, case.X), calls, "gram")
    _check_selection(cuda, case, _state(cuda, case.X), calls, "separable")


def test_one_tree_every_entropy_zero(cuda):
    n, d = 1300, 13
    case = Case(O.synthetic_pool(n, d, seed=n % 97), Forest.synthetic(1, 1, d, seed=5, n_classes=2))
    assert (case.H == 0.0).all()
    _, idx, sc, _ = case.select(case.unl, 50)
    assert np.array_equal(idx, case.unl[:50]) and (sc == 0.0).all()
    for mode in ("gram", "separable"):
        _check_selection(cuda, case, _state(cuda, case.X), ((case.unl, 50),), mode)


def test_signed_pool(cuda):
    """Normal features: densities of both signs, so scores of both signs and
    intervals around negative values."""
    case = Case(O.synthetic_pool(3000, 30, seed=7, dist="normal"), Forest.synthetic(100, 4, 30, seed=5, n_classes=10))
    du = case.d[case.unl]
    assert (du < 0.0).sum() > 100 and (du > 0.0).sum() > 100
    state = _state(cuda, case.X)
    _check_selection(cuda, case, state, ((case.unl, 100),), "gram")
    _check_enclosure(cuda, case, state)
    _check_selection(cuda, case, _state(cuda, case.X), ((case.unl, 100),), "separable")


@pytest.mark.parametrize("beta", [0.5, 2.0])
def test_beta(cuda, beta):
    """beta != 1: the indices equal the reference; the scores agree to the
    two libms' pow (tests/test_gpu_beta.py's tolerance)."""
    case = _case(3001, 64, 100, 4, 10)
    calls = ((case.unl, 25),)
    _check_selection(cuda, case, _state(cuda, case.X), calls, "gram", beta=beta, rtol=1e-14)
    _check_selection(cuda, case, _state(cuda, case.X), calls, "separable", beta=beta, rtol=1e-14)


def test_two_classes_is_the_two_term_entropy(cuda):
    """A binary forest through select_multiclass: counts[:, 1] are the binary
    kernel's votes, the selection is the two-term entropy's and differs from
    density_weighting.select's on the same state."""
    from dal import density_weighting as dw

    n, d, T, k = 3001, 64, 100, 25
    case = Case(O.synthetic_pool(n, d, seed=n % 97), Forest.synthetic(T, 4, d, seed=3))
    assert case.F.n_classes == 2
    of = O.synthetic_forest(T, 4, d, seed=3)
    _, bin_idx, bin_sc = O.density_select(case.X, case.unl, of, k, 1.0, E, density=case.d)
    _, ref_idx, ref_sc, _ = case.select(case.unl, k)
    assert not np.array_equal(bin_idx, ref_idx)  # (on the CPU first: the two definitions differ here)
    state = _state(cuda, case.X)
    one = dw.select(state, case.unl, case.F, k)
    assert np.array_equal(one.indices.cpu().numpy(), bin_idx)
    two = dw.select_multiclass(state, case.unl, case.F, k)
    assert np.array_equal(two.counts.cpu().numpy()[:, 1].astype(np.int32), one.votes.cpu().numpy())
    assert np.array_equal(two.indices.cpu().numpy(), ref_idx)
    assert np.array_equal(_bits(two.selected_scores.cpu().numpy()), _bits(ref_sc))
    assert not np.array_equal(two.indices.cpu().numpy(), one.indices.cpu().numpy())


def test_sharded_selection_equals_single_gpu(cuda):
    from dal import density_weighting as dw
    from dal import parallel

    n, d, world, k = 10_007, 24, 3, 50
    case = Case(O.synthetic_pool(n, d, seed=n % 97), Forest.synthetic(10, 4, d, seed=5, n_classes=10))
    unl = np.arange(17, n)
    _, ref_idx, ref_sc, _ = case.select(unl, k)
    for density_mode in ("gram", "separable"):
        sels = []
        for r in range(world):
            lo, hi, _ = parallel.shard_range(n, world, r)
            sels.append(parallel.ShardedSelector(case.X[lo:hi], n, r, world, excluded=E, device=cuda))
        assert len({s.hi - s.lo for s in sels}) > 1  # uneven shards
        idx, sc = parallel.emulate(sels, unl, case.F, k, mode="dw_multiclass", density_mode=density_mode)
        one = dw.select_multiclass(case.X, unl, case.F, k, excluded_idx=E, device=cuda, mode=density_mode)
        assert np.array_equal(idx.cpu().numpy(), one.indices.cpu().numpy())
        assert np.array_equal(_bits(sc.cpu().numpy()), _bits(one.selected_scores.cpu().numpy()))
        assert np.array_equal(idx.cpu().numpy(), ref_idx)
        assert np.array_equal(_bits(sc.cpu().numpy()), _bits(ref_sc))


def test_run_loop_three_classes(cuda):
    """run_loop(strategy="information_density") over the 3-class pool of
    tests/test_gpu_multiclass.py, scikit-learn trainer, 3 iterations: the
    history equals the same loop with the reference as select_fn."""
    from dal.loop import run_loop

    rng = np.random.default_rng(17)
    X = rng.random((600, 8)).astype(np.float32)
    y = (X[:, 0] * 3).astype(int).clip(0, 2) * 2 + 5  # labels 5, 7, 9
    assert len(set(y[:20].tolist())) == 3  # every class in the initial window: each forest has 3 classes
    dens = O.density_canonical(X, np.arange(20))

    def ref_select(strategy, pool, unlabeled, model, k):
        F = Forest.from_sklearn(model, multiclass=True)
        assert F.n_classes == 3
        return DW.select(pool, unlabeled, F, k, density=dens)[1]

    kw = dict(strategy="information_density", window_size=20, n_estimators=10, max_iterations=3, seed=4,
              trainer="sklearn")
    got = run_loop(X, y, device=cuda, **kw)
    ref = run_loop(X, y, select_fn=ref_select, **kw)
    assert len(got.labeled_history) == 3
    for a, b in zip(got.labeled_history, ref.labeled_history):
        assert np.array_equal(np.asarray(a), np.asarray(b))
