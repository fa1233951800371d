"""Soft-vote information density on the GPU: dal_forest_score_soft_dw (the
soft-vote class entropy x density^beta, interval keys, the per-row entropy and
identity index), dal_dw_step_soft and everything above them, against the
restatement (tests/soft_dw_reference.py).

The device entropy e_dev carries the device log2: it is byte-identical to
dal_forest_score_soft's entropy score on the same pool and within C 2^-49 of
the restatement's H (tests/test_gpu_soft.py's bound).  Every exactness claim
below is therefore stated on e_dev: scores, keys and selections are compared
bit for bit with e_dev * (canonical density), the restatement applied to the
entropy the call returned.  E = range(10) unless a test says otherwise."""
import functools
import os
import socket

import numpy as np
import pytest

import soft_dw_reference as DW
import soft_reference as R
import strided_pool as SP
from dal import _lib
from dal.forest import ProbabilityForest
from oracle import dal_oracle as O

pytestmark = pytest.mark.gpu

KEY_NONE, KEY_NAN = DW.KEY_NONE, DW.KEY_NAN
FIXED, EXACT = _lib.DAL_DENSITY_FIXED, _lib.DAL_DENSITY_EXACT

# name -> (n, d, T, depth, C): tests/test_gpu_soft.py's table, restated -- the
# smallest shape that reaches each path of the launcher
CASES = {
    "scalar_ragged": (1037, 30, 10, 4, 3),     # scalar staging, 128-row tiles, ragged last tile
    "vec4_binary": (1037, 64, 10, 4, 2),       # 16-byte staging, the binary case (class width 2)
    "dma_persistent": (517, 256, 10, 4, 10),   # LDS-DMA staging on the persistent grid, class width 16
    "rows_global": (131, 1100, 3, 2, 3),       # rows read from global memory (16 rows exceed 64 KiB)
    "lanes_per_row": (1037, 30, 100, 4, 5),    # T >= 64: several lanes per row, the cross-lane integer sum
    "widest_largest": (259, 8, 255, 3, 32),    # class width 32; one-hot leaves: some S_c = 255 2^31
    "forest_global": (523, 16, 40, 12, 4),     # synthetic, depth 12: the forest does not fit LDS
    "single_row": (1, 30, 10, 4, 3),
    "wide_resident": (300, 12, 9, 3, 21),      # class width 32 with the forest in LDS, an odd class count
    "sixteen_lanes": (67, 300, 5, 3, 6),       # 16-row tiles: 16 lanes per row, more lanes than trees or classes
}
ONE_HOT_CLASS = 7


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _fitted(n, d, T, depth, C, seed):
    """A seeded pool and a scikit-learn forest fitted on its first rows (every
    class among them): ragged trees, shallow leaves, real distributions."""
    from sklearn.ensemble import RandomForestClassifier

    rng = np.random.default_rng(seed)
    X = rng.random((max(n, 200), d)).astype(np.float32)
    y = (np.floor(X[:, 0] * C).astype(int) + (X[:, 1] > 0.6)) % C
    y[:C] = np.arange(C)
    rf = RandomForestClassifier(n_estimators=T, max_depth=depth, random_state=0, n_jobs=1).fit(X[:200], y[:200])
    return X[:n], ProbabilityForest.from_sklearn(rf)


def np_sums(F, X):
    """soft_reference.sums as an int64 array (the sums stay below 2^39: exact)."""
    lr = R.leaf_rows(F, X)
    q = F.leaf_q.astype(np.int64)
    S = np.zeros((lr.shape[1], int(F.n_classes)), dtype=np.int64)
    for t in range(lr.shape[0]):
        S += q[lr[t]]
    return S


class Ref:
    """A pool, a forest and their reference quantities (computed once, never
    written): the exact sums S, the restatement's entropy H, the canonical
    density d over the pool without E."""

    def __init__(self, X, F, excluded=None, python_sums=False):
        self.X, self.F, self.n, self.T, self.C = X, F, X.shape[0], F.n_trees, int(F.n_classes)
        self.E = (np.arange(10) if self.n > 10 else np.arange(0)) if excluded is None else np.asarray(excluded)
        self.S = np_sums(F, X)
        if python_sums:
            assert self.S.tolist() == R.sums(F, X)
        self.H = DW.entropy(self.S.tolist(), self.T)
        self.d = O.density_canonical(X, self.E)
        self.ex = np.isin(np.arange(self.n), self.E)
        self.unl = np.setdiff1d(np.arange(self.n), self.E)
        for a in (self.S, self.H, self.d):
            a.setflags(write=False)

    def state(self, cuda, excluded=None):
        from dal.engine import PoolState

        return PoolState(self.X, excluded=self.E if excluded is None else excluded, device=cuda)

    def e_dev(self, cuda):
        """The entropy dal_forest_score_soft returns for every row (cached): the
        yardstick of the exactness claims, itself within C 2^-49 of H."""
        if getattr(self, "_e_dev", None) is None:
            from dal import engine

            _, _, sc, _ = engine.forest_score_soft(self.state(cuda), self.F, None, _lib.DAL_DESCENDING,
                                                   _lib.DAL_SOFT_ENTROPY)
            e = _np(sc)
            err = np.abs(e - self.H).max()
            print(f"max |e_dev - H| = {err * 2.0 ** 49:.3f} x 2^-49 (bound {self.C} x 2^-49)")
            assert err <= self.C * 2.0 ** -49
            assert not np.isnan(e).any() and not np.signbit(e).any()
            e.setflags(write=False)
            self._e_dev = e
        return self._e_dev

    def select(self, e, unl, k, beta=1.0, density=None):
        return DW.select(self.X, unl, self.F, k, beta=beta, density=self.d if density is None else density, H=e)


@functools.lru_cache(maxsize=None)
def case(name):
    n, d, T, depth, C = CASES[name]
    if name == "widest_largest":
        X = np.random.default_rng(5).random((n, d)).astype(np.float32)
        F = ProbabilityForest.synthetic(T, depth, d, C, seed=3)
        # the leaf row 0 reaches in every tree becomes one-hot in one class: S_c(0) = T 2^31
        hot = [(t, int(l) - t * (1 << depth), ONE_HOT_CLASS) for t, l in enumerate(R.leaf_rows(F, X[:1])[:, 0])]
        F = ProbabilityForest.synthetic(T, depth, d, C, seed=3, one_hot=hot)
    elif name == "forest_global":
        X = np.random.default_rng(6).random((n, d)).astype(np.float32)
        F = ProbabilityForest.synthetic(T, depth, d, C, seed=4)
    else:
        X, F = _fitted(n, d, T, depth, C, seed=100 + d + C)
    assert F.n_trees == T and F.n_classes == C and F.depth <= depth
    return Ref(X, F, python_sums=name in ("scalar_ragged", "widest_largest", "sixteen_lanes"))


def _flags(state, seed):
    """The pool's EXCLUDED bits | DAL_ROW_CANDIDATE on ~70 % of the rows (seeded; row 0 always)."""
    cand = (np.random.default_rng(seed).random(state.n) < 0.7).astype(np.uint8)
    cand[0] = 1
    return _np(state.flags) | cand * np.uint8(_lib.DAL_ROW_CANDIDATE)


def _launch(cuda, state, F, flags, density, kind, derr=0.0, beta=1.0):
    """One launch through the engine; numpy outputs, keys as uint64."""
    import torch

    from dal import engine

    out = engine.forest_score_soft_dw(state, F, torch.from_numpy(flags).to(cuda), density, kind, derr, beta, True)
    s, p, e, ix, sc, klo, khi = (_np(t) for t in out)
    return s, p, e, ix, sc, klo.view(np.uint64), khi.view(np.uint64)


def _check_rows(ref, cuda, sums, pred, e, ix):
    """What does not depend on the density: equal to the restatement bit for
    bit, the entropy byte-identical to dal_forest_score_soft's."""
    assert sums.dtype == np.int64 and np.array_equal(sums, ref.S)
    assert pred.dtype == np.uint8 and np.array_equal(pred, R.pred(ref.S.tolist()))
    assert ix.dtype == np.int32 and np.array_equal(ix, np.arange(ref.n))
    assert e.tobytes() == ref.e_dev(cuda).tobytes()


def _check_exact(cuda, ref, state):
    """DAL_DENSITY_EXACT, beta = 1: scores and keys are those of e_dev * d bit for bit."""
    n = ref.n
    assert np.array_equal(np.isnan(ref.d), ref.ex)
    flags = _flags(state, 11)
    sums, pred, e, ix, s, klo, khi = _launch(cuda, state, ref.F, flags, state.density_exact(), EXACT)
    _check_rows(ref, cuda, sums, pred, e, ix)
    want = e * ref.d  # one fp64 multiply
    assert np.array_equal(np.isnan(s), ref.ex)
    assert np.array_equal(_bits(s[~ref.ex]), _bits(want[~ref.ex]))
    assert np.array_equal(khi, klo)
    cand = (flags & _lib.DAL_ROW_CANDIDATE) != 0
    assert cand.sum() >= 1 and np.array_equal(klo == KEY_NONE, ~cand)
    assert np.array_equal(klo[cand], DW.score_key(want)[cand])
    assert (klo[cand & ref.ex] == KEY_NAN).all()  # an excluded candidate: the NaN key


def _check_enclosure(cuda, ref, state):
    """DAL_DENSITY_FIXED (the Gram density): the interval keys enclose the key
    of e_dev * d_canonical -- what makes the exact selection valid
    (tests/test_gpu_multiclass_dw.py's inequality)."""
    from dal import engine

    n = ref.n
    flags = _flags(state, 12)
    derr = engine.density_error(state)
    assert derr > 0.0
    sums, pred, e, ix, s, klo, khi = _launch(cuda, state, ref.F, flags, state.density_fixed(), FIXED, derr)
    _check_rows(ref, cuda, sums, pred, e, ix)
    cand = (flags & _lib.DAL_ROW_CANDIDATE) != 0
    assert np.array_equal(klo == KEY_NONE, ~cand) and np.array_equal(khi == KEY_NONE, ~cand)
    m = cand & ~ref.ex
    assert m.sum() > n // 2
    want, em = (e * ref.d)[m], e[m]
    assert (np.abs(s[m] - want) <= em * derr + 1e-15 * np.abs(want)).all()
    key = DW.score_key(want)
    assert (khi[m] <= key).all() and (key <= klo[m]).all()
    assert np.array_equal(khi[m] == klo[m], em == 0.0)
    ex = cand & ref.ex  # an excluded candidate: NaN, a point interval
    assert (klo[ex] == KEY_NAN).all() and (khi[ex] == KEY_NAN).all()


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_outputs_exact_density(cuda, name):
    ref = case(name)
    _check_exact(cuda, ref, ref.state(cuda))


@pytest.mark.parametrize("name", [c for c in CASES if c != "single_row"])
def test_interval_enclosure_fixed_density(cuda, name):
    ref = case(name)
    _check_enclosure(cuda, ref, ref.state(cuda))


def test_paths_reached():
    """The staging form each case is listed for (tests/strided_pool.py restates the tiling rule)."""
    for name, staging in (("scalar_ragged", "scalar"), ("vec4_binary", "vec4"), ("dma_persistent", "dma"),
                          ("rows_global", "none"), ("lanes_per_row", "scalar"), ("sixteen_lanes", "dma")):
        n, d, T, depth, C = CASES[name]
        t = SP.forest_tiling(d, d, 4096, T)
        assert t.staging == staging, (name, t)
    F = case("forest_global").F
    assert F.n_trees * (((1 << F.depth) - 1) * 8 + (1 << F.depth) * 4) > 65536


def test_dma_block_walks_two_tiles(cuda):
    """LDS-DMA at d = 128 (64-row tiles) with more tiles than twice the grid
    the soft kernel's LDS use lets be resident: every block of the persistent
    grid loads a second tile's flags and density words.  DAL_DENSITY_EXACT: no
    Gram at this size."""
    import torch

    d, T, depth, C, rows = 128, 10, 4, 10, 64
    assert SP.forest_tiling(d, d, 4096, T)[:2] == ("dma", rows)
    F = ProbabilityForest.synthetic(T, depth, d, C, seed=6)
    # forest_soft.hip's LDS: the tile, then nodes and leaf ids (rounded to 16 B), then round2(C) words per leaf
    nodes = T * (((1 << depth) - 1) * 8 + (1 << depth) * 4)
    lds = rows * (d + 4) * 4 + (nodes + 15) // 16 * 16 + F.n_leaves * ((C + 1) // 2 * 2) * 4
    per_cu = (160 * 1024) // lds
    assert per_cu >= 1
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    n = min(2 * cus * per_cu * rows + 37, 400_000)
    assert n > cus * per_cu * rows  # the second tile of at least one block, whatever the cap
    ref = Ref(O.synthetic_pool(n, d, seed=3), F)
    _check_exact(cuda, ref, ref.state(cuda))


# ------------------------------------------------------- through the C entry --
def _call_c(cuda, ref, x, x_stride, density, kind, flags, derr=0.0, beta=1.0, want_sums=True, want_pred=True,
            want_hi=True):
    import torch

    n, C, F = ref.n, ref.C, ref.F
    inner, leaf_id, leaf_q = F.device(cuda)
    fl = torch.from_numpy(flags).to(cuda)
    out = {"sums": torch.empty((n, C), dtype=torch.int64, device=cuda) if want_sums else None,
           "pred": torch.empty(n, dtype=torch.uint8, device=cuda) if want_pred else None,
           "entropy": torch.empty(n, dtype=torch.float64, device=cuda),
           "row_index": torch.empty(n, dtype=torch.int32, device=cuda),
           "scores": torch.empty(n, dtype=torch.float64, device=cuda),
           "keys": torch.empty(n, dtype=torch.int64, device=cuda),
           "keys_hi": torch.empty(n, dtype=torch.int64, device=cuda) if want_hi else None}
    ptr = {k: 0 if v is None else v.data_ptr() for k, v in out.items()}
    _lib.call("dal_forest_score_soft_dw", x.data_ptr(), n, ref.X.shape[1], x_stride, inner.data_ptr(),
              leaf_id.data_ptr(), leaf_q.data_ptr(), F.n_leaves, F.n_trees, int(F.depth), C, density.data_ptr(),
              kind, float(derr), fl.data_ptr(), float(beta), ptr["sums"], ptr["pred"], ptr["entropy"],
              ptr["row_index"], ptr["scores"], ptr["keys"], ptr["keys_hi"],
              torch.cuda.current_stream(cuda).cuda_stream)
    return {k: None if v is None else _np(v).tobytes() for k, v in out.items()}


@pytest.mark.parametrize("name", ["scalar_ragged", "dma_persistent"])
def test_optional_outputs(cuda, name):
    """keys_hi = NULL, and sums = pred = NULL: the remaining outputs unchanged."""
    from dal import engine

    ref = case(name)
    state = ref.state(cuda)
    flags = _flags(state, 13)
    dens, derr = state.density_fixed(), engine.density_error(state)
    full = _call_c(cuda, ref, state.x, ref.X.shape[1], dens, FIXED, flags, derr)
    assert full["sums"] == ref.S.tobytes() and full["keys_hi"] != full["keys"]
    no_hi = _call_c(cuda, ref, state.x, ref.X.shape[1], dens, FIXED, flags, derr, want_hi=False)
    assert no_hi["keys_hi"] is None
    assert all(no_hi[k] == full[k] for k in full if k != "keys_hi")
    bare = _call_c(cuda, ref, state.x, ref.X.shape[1], dens, FIXED, flags, derr, want_sums=False, want_pred=False)
    assert bare["sums"] is None and bare["pred"] is None
    assert all(bare[k] == full[k] for k in full if k not in ("sums", "pred"))


def test_strided_unaligned_pool(cuda):
    """One pool with x_stride = d + 3 and a base 4 bytes off the allocation
    (NaN in every padding element), through the C entry: the outputs of the
    contiguous pool, and the buffer unchanged."""
    from dal import engine

    ref = case("scalar_ragged")
    d = ref.X.shape[1]
    state = ref.state(cuda)
    flags = _flags(state, 14)
    view = SP.strided(ref.X, d + 3, 1, cuda)
    assert view.data_ptr() % 16 == 4
    for dens, kind, derr in ((state.density_exact(), EXACT, 0.0),
                             (state.density_fixed(), FIXED, engine.density_error(state))):
        want = _call_c(cuda, ref, state.x, d, dens, kind, flags, derr)
        got = _call_c(cuda, ref, view, d + 3, dens, kind, flags, derr)
        assert want["sums"] == ref.S.tobytes() and want["entropy"] == ref.e_dev(cuda).tobytes()
        for k in want:
            assert got[k] == want[k], (kind, k)
    SP.assert_unchanged(view)


# ----------------------------------------------------------------- selection --
def _check_selection(cuda, ref, state, calls, mode, beta=1.0, rtol=0.0, density=None, unfused=False):
    """select_soft against the restatement on e_dev; returns the selections."""
    from dal import density_weighting as dw

    e = ref.e_dev(cuda)
    out = []
    for unl, k in calls:
        if unfused:
            state.select_events = []  # the per-kernel path: dal_forest_score_soft_dw, then dal_dw_select
        sel = dw.select_soft(state, unl, ref.F, k, beta=beta, mode=mode)
        state.select_events = None
        _, ref_idx, ref_sc = ref.select(e, unl, k, beta, density)
        assert ref_idx.shape[0] == min(k, unl.shape[0])
        assert np.array_equal(_np(sel.indices), ref_idx), (mode, k)
        got = _np(sel.selected_scores)
        if rtol:
            assert np.allclose(got, ref_sc, rtol=rtol, atol=0.0), (mode, k)
        else:
            assert np.array_equal(_bits(got), _bits(ref_sc)), (mode, k)
        assert sel.votes is None and sel.counts is None and sel.denominator == ref.T * R.ONE
        assert np.array_equal(_np(sel.sums), ref.S[unl])
        assert _np(sel.proba()).tobytes() == R.proba(ref.S[unl].tolist(), ref.T).tobytes()
        assert sel.scores.shape[0] == unl.shape[0]
        out.append((_np(sel.indices), got))
    return out


@functools.lru_cache(maxsize=None)
def sklearn_case(n, d, T, depth, C):
    """tests/test_soft_host.py's sklearn_case, restated: a seeded pool and a
    scikit-learn forest fitted on 300 of its rows with every class present."""
    from sklearn.ensemble import RandomForestClassifier

    rng = np.random.default_rng(1000 * C + d)
    X = rng.random((n, d)).astype(np.float32)
    y = (np.floor(X[:, 0] * C).astype(int) + (X[:, 1] > 0.6)) % C
    y[:C] = np.arange(C)  # every class among the fitted rows
    rf = RandomForestClassifier(n_estimators=T, max_depth=depth, random_state=0, n_jobs=1).fit(X[:300], y[:300])
    assert len(rf.classes_) == C
    return Ref(X, ProbabilityForest.from_sklearn(rf))


@pytest.mark.parametrize("shape", [(1037, 30, 10, 4, 3), (2051, 64, 100, 6, 10)])
def test_selection(cuda, shape):
    """select_soft, gram (cold, then two warm calls on one PoolState) and
    separable: k = 1 and 100 over a two-thirds subset, k = 100 over 40 rows
    (clamped); the one-call step equals the unfused pair of calls."""
    ref = sklearn_case(*shape)
    rng = np.random.default_rng(ref.n)
    subset = np.sort(rng.choice(ref.unl, size=(2 * ref.unl.size) // 3, replace=False))
    few = np.sort(rng.choice(ref.unl, size=40, replace=False))
    # preconditions, on the CPU and on the restatement's H: a strictly positive top 100 of 100 distinct values
    top = ref.select(ref.H, subset, 100)[2]
    assert np.unique(top).size == 100 and (top > 0.0).all()
    calls = ((subset, 1), (subset, 100), (few, 100))
    state = ref.state(cuda)
    step = _check_selection(cuda, ref, state, calls, "gram")
    assert state._density is not None  # the second and third calls were warm
    _check_selection(cuda, ref, ref.state(cuda), calls, "separable")
    pair = _check_selection(cuda, ref, ref.state(cuda), calls, "gram", unfused=True)
    for (i, s), (j, t) in zip(step, pair):
        assert np.array_equal(i, j) and s.tobytes() == t.tobytes()


def test_zero_entropy_ties(cuda):
    """Every leaf one-hot in class 0 but three: most rows have e == +0.0.
    k = 100 stays among the positive scores; k = pos + 50 crosses into the
    +0.0 point intervals, where the lowest indices win."""
    n, d, T, depth, C = 3000, 40, 10, 4, 4
    keep = {(0, 3), (4, 9), (7, 12)}
    hot = [(t, l, 0) for t in range(T) for l in range(1 << depth) if (t, l) not in keep]
    ref = Ref(O.synthetic_pool(n, d, seed=4), ProbabilityForest.synthetic(T, depth, d, C, seed=8, one_hot=hot))
    pos = int((ref.H[ref.unl] > 0.0).sum())
    assert 150 < pos < 1500 and (ref.d[ref.unl] > 0.0).all()
    _, idx, sc = ref.select(ref.H, ref.unl, pos + 50)
    assert (sc[:pos] > 0.0).all() and (sc[pos:] == 0.0).all()
    zero_rows = ref.unl[ref.H[ref.unl] == 0.0]
    assert np.array_equal(idx[pos:], zero_rows[:50])
    calls = ((ref.unl, 100), (ref.unl, pos + 50))
    for unfused in (False, True):
        _check_selection(cuda, ref, ref.state(cuda), calls, "gram", unfused=unfused)
    _check_selection(cuda, ref, ref.state(cuda), calls, "separable")
    assert np.array_equal(ref.e_dev(cuda) == 0.0, ref.H == 0.0)


def test_one_tree_every_entropy_zero(cuda):
    n, d = 1300, 13
    F = ProbabilityForest.synthetic(1, 1, d, 2, seed=5, one_hot=[(0, 0, 0), (0, 1, 1)])
    ref = Ref(O.synthetic_pool(n, d, seed=n % 97), F)
    assert (ref.H == 0.0).all()
    _, idx, sc = ref.select(ref.H, ref.unl, 50)
    assert np.array_equal(idx, ref.unl[:50]) and (sc == 0.0).all()
    for mode in ("gram", "separable"):
        _check_selection(cuda, ref, ref.state(cuda), ((ref.unl, 50),), mode)


def test_signed_pool(cuda):
    """Normal features: densities of both signs, so scores of both signs and
    intervals around negative values."""
    ref = Ref(O.synthetic_pool(3000, 30, seed=7, dist="normal"),
              ProbabilityForest.synthetic(100, 4, 30, 10, seed=5, dist="normal"))
    du = ref.d[ref.unl]
    assert (du < 0.0).sum() > 100 and (du > 0.0).sum() > 100
    state = ref.state(cuda)
    _check_selection(cuda, ref, state, ((ref.unl, 100),), "gram")
    _check_enclosure(cuda, ref, state)
    _check_selection(cuda, ref, ref.state(cuda), ((ref.unl, 100),), "separable")


@pytest.mark.parametrize("beta", [0.5, 2.0])
def test_beta(cuda, beta):
    """beta != 1: the indices equal the restatement's on e_dev; the scores agree
    to the two libms' pow (tests/test_gpu_beta.py's tolerance)."""
    ref = case("lanes_per_row")
    calls = ((ref.unl, 25),)
    _check_selection(cuda, ref, ref.state(cuda), calls, "gram", beta=beta, rtol=1e-14)
    _check_selection(cuda, ref, ref.state(cuda), calls, "gram", beta=beta, rtol=1e-14, unfused=True)
    _check_selection(cuda, ref, ref.state(cuda), calls, "separable", beta=beta, rtol=1e-14)


def test_excluded_labeled(cuda):
    """excluded_idx=LABELED on a warm PoolState grows E by 50 rows through
    PoolState.exclude; the step then equals a fresh state with the larger E,
    and the restatement with that E's density."""
    from dal import density_weighting as dw

    ref = case("scalar_ragged")
    k = 30
    state = ref.state(cuda)
    _check_selection(cuda, ref, state, ((ref.unl, k),), "gram")  # warm: the density is cached
    delta = np.random.default_rng(2).choice(ref.unl, size=50, replace=False)
    union = np.union1d(ref.E, delta)
    unl = np.setdiff1d(np.arange(ref.n), union)
    d_union = O.density_canonical(ref.X, union)
    addr = state._density.data_ptr()
    got = dw.select_soft(state, unl, ref.F, k, excluded_idx=dw.LABELED)
    assert np.array_equal(state.excluded, union) and state._density.data_ptr() == addr  # downdated, not recomputed
    fresh = dw.select_soft(ref.state(cuda, excluded=union), unl, ref.F, k)
    _, ref_idx, ref_sc = ref.select(ref.e_dev(cuda), unl, k, density=d_union)
    for sel in (got, fresh):
        assert np.array_equal(_np(sel.indices), ref_idx)
        assert np.array_equal(_bits(_np(sel.selected_scores)), _bits(ref_sc))


def test_sharded_selection_equals_single_gpu(cuda):
    """Three uneven emulated shards of 10,007 x 24 on one device, both density
    modes; parallel.exclude's emulation then grows E on every shard."""
    from dal import density_weighting as dw
    from dal import parallel

    n, d, world, k = 10_007, 24, 3, 50
    ref = Ref(O.synthetic_pool(n, d, seed=n % 97), ProbabilityForest.synthetic(10, 4, d, 10, seed=5))
    unl = np.arange(17, n)
    e = ref.e_dev(cuda)
    _, ref_idx, ref_sc = ref.select(e, unl, k)
    for density_mode in ("gram", "separable"):
        sels = []
        for r in range(world):
            lo, hi, _ = parallel.shard_range(n, world, r)
            sels.append(parallel.ShardedSelector(ref.X[lo:hi], n, r, world, excluded=ref.E, device=cuda))
        assert len({s.hi - s.lo for s in sels}) > 1  # uneven shards
        idx, sc = parallel.emulate(sels, unl, ref.F, k, mode="dw_soft", density_mode=density_mode)
        one = dw.select_soft(ref.X, unl, ref.F, k, excluded_idx=ref.E, device=cuda, mode=density_mode)
        assert np.array_equal(_np(idx), _np(one.indices))
        assert np.array_equal(_bits(_np(sc)), _bits(_np(one.selected_scores)))
        assert np.array_equal(_np(idx), ref_idx)
        assert np.array_equal(_bits(_np(sc)), _bits(ref_sc))
    # warm gram shards: E grows by the selection (the sharded exclude), the next step is the larger E's
    sels = []
    for r in range(world):
        lo, hi, _ = parallel.shard_range(n, world, r)
        sels.append(parallel.ShardedSelector(ref.X[lo:hi], n, r, world, excluded=ref.E, device=cuda))
    parallel.emulate(sels, unl, ref.F, k, mode="dw_soft")
    assert all(s._density is not None for s in sels)
    assert parallel.emulate_exclude(sels, ref_idx) == k
    unl2 = np.setdiff1d(unl, ref_idx)
    idx, sc = parallel.emulate(sels, unl2, ref.F, k, mode="dw_soft")
    _, ref_idx2, ref_sc2 = ref.select(e, unl2, k, density=O.density_canonical(ref.X, np.union1d(ref.E, ref_idx)))
    assert np.array_equal(_np(idx), ref_idx2) and np.array_equal(_bits(_np(sc)), _bits(ref_sc2))


# ------------------------------------------------- a one-rank RCCL group --
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(port, q):
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    for p in (repo, os.path.join(repo, "distributed-active-learning_amd"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        from dal import density_weighting as dw
        from dal import parallel

        ref = case("scalar_ragged")
        k = 20
        comm = parallel.TorchComm()
        out = {"backend": comm.backend}
        for density_mode in ("gram", "separable"):
            shard = parallel.ShardedSelector(torch.from_numpy(np.array(ref.X)).to(dev), ref.n, 0, 1, excluded=ref.E,
                                             device=dev)
            idx, sc = parallel.select(shard, comm, ref.unl, ref.F, k, mode="dw_soft", density_mode=density_mode)
            one = dw.select_soft(np.array(ref.X), ref.unl, ref.F, k, excluded_idx=ref.E, device=dev, mode=density_mode)
            torch.cuda.synchronize()
            out[density_mode] = (_np(idx), _np(sc), _np(one.indices), _np(one.selected_scores))
        q.put(out)
    except Exception:  # surface worker failures instead of a queue timeout
        import traceback

        q.put(traceback.format_exc())
        raise
    finally:
        dist.destroy_process_group()


def test_sharded_dw_soft_on_a_one_rank_nccl_group(cuda):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(_free_port(), q))
    p.start()
    out = q.get(timeout=240)
    p.join(timeout=60)
    assert isinstance(out, dict), out
    assert p.exitcode == 0 and out["backend"] == "nccl"
    ref = case("scalar_ragged")
    _, ref_idx, ref_sc = ref.select(ref.e_dev(cuda), ref.unl, 20)
    for density_mode in ("gram", "separable"):
        idx, sc, one_idx, one_sc = out[density_mode]
        assert idx.shape[0] == 20 and np.array_equal(idx, one_idx), density_mode
        assert sc.tobytes() == one_sc.tobytes(), density_mode
        assert np.array_equal(idx, ref_idx) and np.array_equal(_bits(sc), _bits(ref_sc)), density_mode


@pytest.mark.parametrize("density_over", ["initial", "unlabeled"])
def test_run_loop_soft_information_density(cuda, density_over):
    """run_loop(strategy="soft_information_density") over a 3-class pool,
    scikit-learn trainer, 3 iterations: the history of the same loop with the
    restatement as select_fn (E the initial window, or the current labeled set)."""
    from dal.loop import run_loop

    rng = np.random.default_rng(17)
    X = rng.random((600, 8)).astype(np.float32)
    y = (X[:, 0] * 3).astype(int).clip(0, 2) * 2 + 5  # labels 5, 7, 9
    assert len(set(y[:20].tolist())) == 3  # every class in the initial window: each forest has 3 classes
    dens0 = O.density_canonical(X, np.arange(20))

    def ref_select(strategy, pool, unlabeled, model, k):
        F = ProbabilityForest.from_sklearn(model)
        assert F.n_classes == 3
        dens = dens0 if density_over == "initial" else \
            O.density_canonical(pool, np.setdiff1d(np.arange(pool.shape[0]), unlabeled))
        return DW.select(pool, unlabeled, F, k, density=dens)[1]

    kw = dict(strategy="soft_information_density", window_size=20, n_estimators=10, max_iterations=3, seed=4,
              trainer="sklearn", density_over=density_over)
    got = run_loop(X, y, device=cuda, **kw)
    ref = run_loop(X, y, select_fn=ref_select, **kw)
    assert len(got.labeled_history) == 3
    for a, b in zip(got.labeled_history, ref.labeled_history):
        assert np.array_equal(np.asarray(a), np.asarray(b))
