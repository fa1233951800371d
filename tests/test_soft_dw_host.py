"""Soft-vote information density, host side: the two new symbols and every
host-side status of dal_forest_score_soft_dw and dal_dw_step_soft, the
restatement (tests/soft_dw_reference.py) on a hand-computed case, the refusals
of select_soft and of the sharded mode "dw_soft", and the merge and the loop
with the restatement injected.  CPU only (no kernel launches)."""
import math
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import soft_dw_reference as DW
import soft_reference as R
from dal import _lib, parallel
from dal.forest import Forest, ProbabilityForest
from oracle import dal_oracle as O

ARG, SHAPE, UNSUPPORTED = -1, -2, -3
P = c_void_p(256)        # a 16-B aligned address that is never dereferenced
WS = c_void_p(1 << 20)   # 256-B aligned


def test_symbols_and_argument_lists():
    lib = _lib.load()
    S = _lib.SIGNATURES
    assert lib.dal_abi_version() == 10  # new symbols only
    for name in ("dal_forest_score_soft_dw", "dal_dw_step_soft"):
        assert callable(getattr(lib, name)), name
    # dal_forest_score_soft's forest (up to n_classes), then dal_forest_score_multiclass_dw's arguments from the
    # density on, with the class sums in the place of the counts
    res, soft = S["dal_forest_score_soft"]
    _, mcdw = S["dal_forest_score_multiclass_dw"]
    assert S["dal_forest_score_soft_dw"] == (res, soft[:11] + mcdw[10:])
    assert len(S["dal_forest_score_soft_dw"][1]) == 24
    # ... and dal_dw_step_multiclass's arguments from the density on
    _, mcstep = S["dal_dw_step_multiclass"]
    assert S["dal_dw_step_soft"] == (res, soft[:11] + mcstep[12:])
    assert len(S["dal_dw_step_soft"][1]) == 37


FIXED, EXACT = _lib.DAL_DENSITY_FIXED, _lib.DAL_DENSITY_EXACT


def _score(x=P, n=10, d=4, x_stride=4, inner=P, leaf_id=P, leaf_q=P, L=20, T=10, depth=4, C=3, density=P, dkind=FIXED,
           derr=0.0, flags=None, beta=1.0, sums=P, pred=P, entropy=P, row_index=P, scores=P, keys=P, keys_hi=P):
    return _lib.load().dal_forest_score_soft_dw(x, n, d, x_stride, inner, leaf_id, leaf_q, L, T, depth, C, density,
                                                dkind, derr, flags, beta, sums, pred, entropy, row_index, scores,
                                                keys, keys_hi, None)


def test_score_statuses_without_gpu():
    limit = _lib.load().dal_forest_soft_max_depth()
    assert {FIXED, EXACT} == {1, 2}
    for name in ("x", "inner", "leaf_id", "leaf_q", "density", "entropy", "row_index", "scores", "keys"):
        assert _score(**{name: None}) == ARG, name
    assert _score(dkind=0) == ARG and _score(dkind=3) == ARG and _score(dkind=EXACT, x_stride=3) == SHAPE
    assert _score(x_stride=3) == SHAPE and _score(d=30, x_stride=29) == SHAPE and _score(d=30, x_stride=0) == SHAPE
    assert _score(n=-1) == SHAPE and _score(d=0, x_stride=0) == SHAPE and _score(L=0) == SHAPE
    assert _score(L=(1 << 26) + 1) == SHAPE
    assert _score(n=1 << 31) == SHAPE and _score(n=(1 << 31) + 5, dkind=EXACT) == SHAPE  # row_index is int32
    assert _score(T=256) == UNSUPPORTED and _score(T=0) == UNSUPPORTED
    assert _score(C=33) == UNSUPPORTED and _score(C=1) == UNSUPPORTED
    assert _score(depth=limit + 1) == UNSUPPORTED and _score(depth=0) == UNSUPPORTED
    # the documented order: ARG before SHAPE before UNSUPPORTED
    assert _score(x=None, x_stride=3) == ARG and _score(density=None, n=1 << 31, T=256) == ARG
    assert _score(dkind=0, x_stride=3, T=256) == ARG
    assert _score(x_stride=3, T=256) == SHAPE and _score(n=1 << 31, C=33, depth=limit + 1) == SHAPE
    # nothing to score: no launch; sums, pred and keys_hi are optional; the limits themselves pass
    assert _score(n=0) == 0 and _score(n=0, sums=None, pred=None, keys_hi=None) == 0
    assert _score(n=0, dkind=EXACT, beta=0.5) == 0
    assert _score(n=0, T=255, C=32, depth=limit) == 0 and _score(n=0, T=1, C=2, depth=1, d=1, x_stride=1) == 0
    assert _score(n=0, x_stride=7) == 0  # any stride >= d


def _step(x=P, n=2500, d=256, x_stride=256, inner=P, leaf_id=P, leaf_q=P, L=160, T=10, depth=4, C=10, density=P,
          derr=0.0, flags=P, beta=1.0, idx_base=0, norm64=P, colsum=P, k=16, cap=2500, passes=1, step_flags=0, ws=WS,
          ws_bytes=0, sums=P, pred=P, entropy=P, row_index=P, scores=P, keys_lo=P, keys_hi=P, out_idx=P, out_scores=P,
          out_keys=P, status=P):
    return _lib.load().dal_dw_step_soft(x, n, d, x_stride, inner, leaf_id, leaf_q, L, T, depth, C, density, derr, flags,
                                        beta, idx_base, norm64, colsum, k, cap, passes, step_flags, ws, ws_bytes, sums,
                                        pred, entropy, row_index, scores, keys_lo, keys_hi, out_idx, out_scores,
                                        out_keys, status, None, None)


def test_step_statuses_without_gpu():
    """Every argument error comes back before device work.  A call whose
    arguments are all valid is stopped here by its workspace size (0 bytes:
    DAL_ERR_SHAPE, the last host check)."""
    limit = _lib.load().dal_forest_soft_max_depth()
    assert _step() == SHAPE and _step(sums=None, pred=None) == SHAPE  # valid but for the workspace
    assert _step(out_keys=None) == SHAPE and _step(passes=0) == SHAPE
    for name in ("x", "inner", "leaf_id", "leaf_q", "density", "norm64", "colsum", "ws", "entropy", "row_index",
                 "scores", "keys_lo", "keys_hi", "out_idx", "out_scores", "status"):
        assert _step(**{name: None}) == ARG, name
    # the two measurement flags are not this entry's
    assert _step(step_flags=_lib.DAL_STEP_KEEP_GROUPS) == ARG
    assert _step(step_flags=_lib.DAL_STEP_SELECT_ONLY | _lib.DAL_STEP_WS_CLEAN) == ARG and _step(step_flags=16) == ARG
    assert _step(step_flags=_lib.DAL_STEP_RESET_STATUS | _lib.DAL_STEP_WS_CLEAN) == SHAPE
    assert _step(n=-1) == SHAPE and _step(x_stride=255) == SHAPE and _step(d=0, x_stride=0) == SHAPE
    assert _step(L=0) == SHAPE and _step(n=1 << 31) == SHAPE
    assert _step(C=1) == UNSUPPORTED and _step(C=33) == UNSUPPORTED
    assert _step(T=256) == UNSUPPORTED and _step(T=0) == UNSUPPORTED
    assert _step(depth=limit + 1) == UNSUPPORTED and _step(depth=0) == UNSUPPORTED
    # the documented order: ARG before SHAPE before UNSUPPORTED
    assert _step(x=None, x_stride=255, T=256) == ARG and _step(step_flags=16, n=-1) == ARG
    assert _step(x_stride=255, T=256) == SHAPE
    assert _step(n=0) == 0 and _step(n=0, k=0) == 0  # nothing to score or select: before the selection's checks
    # the selection's checks
    assert _step(k=0) == SHAPE and _step(k=2501) == SHAPE and _step(cap=8) == SHAPE
    assert _step(passes=6) == ARG and _step(passes=-1) == ARG
    need = _lib.load().dal_dw_step_workspace_bytes(2500, 16, 2500)
    assert _step(ws=c_void_p((1 << 20) + 8), ws_bytes=need) == SHAPE  # a misaligned workspace of the right size


# ------------------------------------------------------ the restatement --
def _two_leaf_forest():
    """One tree, one node: x[0] <= 0.5 reaches leaf 0 (p = 1/4, 3/4), else leaf 1 (p = 1, 0)."""
    return ProbabilityForest.from_nodes([0, -1, -1], [0.5, 0.0, 0.0], [1, -1, -1], [2, -1, -1],
                                        [[0, 0], [1, 3], [2, 0]], [0], n_classes=2)


def test_restatement_on_a_hand_computed_two_leaf_case():
    F = _two_leaf_forest()
    assert F.n_trees == 1 and F.depth == 1 and F.n_classes == 2
    X = np.array([[0.1, 1.0], [0.9, 0.1], [0.2, 0.3], [0.8, 0.9], [0.3, 0.1]], dtype=np.float32)
    S = R.sums(F, X)
    assert S == [[1 << 29, 3 << 29], [1 << 31, 0], [1 << 29, 3 << 29], [1 << 31, 0], [1 << 29, 3 << 29]]
    h = (0.0 + 0.25 * 2.0) + (-0.75) * math.log2(0.75)  # -(1/4) log2(1/4) = 1/2, exactly
    H = DW.entropy(S, 1)
    assert H.tolist() == [h, 0.0, h, 0.0, h] and not np.signbit(H).any()
    # E = {0}: the densities sum the cosines to rows 1..4 (row 0 is NaN)
    d = O.density_canonical(X, [0])
    assert np.isnan(d[0]) and not np.isnan(d[1:]).any()
    U = X.astype(np.float64) / np.sqrt((X.astype(np.float64) ** 2).sum(axis=1, keepdims=True))
    assert np.allclose(d[1:], (U[1:] @ U[1:].T).sum(axis=1), rtol=1e-12)
    sc = DW.scores(H, d)
    assert np.isnan(sc[0]) and sc[1] == 0.0 and sc[3] == 0.0 and sc[2] == h * d[2] and sc[4] == h * d[4]
    assert np.array_equal(DW.scores(H, d, 2.0)[1:], H[1:] * np.power(d[1:], 2.0))
    # descending, NaN last, the zeros by index
    unl = np.arange(5)
    order = [2, 4] if sc[2] >= sc[4] else [4, 2]
    _, idx, sel = DW.select(X, unl, F, 5, excluded=[0])
    assert idx.tolist() == order + [1, 3, 0] and np.isnan(sel[4]) and sel[2] == 0.0 and sel[0] == sc[order[0]]
    _, idx, _ = DW.select(X, unl[1:], F, 3, density=d, H=H)
    assert idx.tolist() == order + [1]
    # the keys: descending, so a larger score has the smaller key; NaN after every number
    key = DW.score_key(sc)
    assert key[0] == DW.KEY_NAN and key[1] == key[3] and key[order[0]] <= key[order[1]] < key[1] < key[0]
    assert [int(v) for v in key] == [R.score_key(float(v), False) for v in sc]


# ------------------------------------------------------------- refusals --
def test_select_soft_refuses_a_hard_voting_forest():
    from dal import density_weighting as dw

    assert "select_soft" in dw.__all__
    X = O.synthetic_pool(64, 8, seed=1)
    for F in (Forest.synthetic(10, 3, 8, seed=1), Forest.synthetic(10, 3, 8, seed=1, n_classes=4),
              ProbabilityForest.synthetic(10, 3, 8, 4, seed=1).hard()):
        with pytest.raises(ValueError, match="select_multiclass"):
            dw.select_soft(X, np.arange(10, 64), F, 5, device="cuda:0")  # (raised before the device is touched)


# ------------------------------------------------- the merge and the loop --
class _HostState:
    """What ShardedSelector.status_word reads of a shard's PoolState."""

    status = torch.zeros(1, dtype=torch.int32)


class RestatementShard(parallel.ShardedSelector):
    """ShardedSelector whose local step is the restatement (CPU); the density
    is the canonical one of the whole pool, handed in (a warm shard: no
    operand exchange)."""

    def __init__(self, X, density, n_total, rank, world):
        self.n_total, self.rank, self.world = n_total, rank, world
        self.lo, self.hi, self.shard = parallel.shard_range(n_total, world, rank)
        self.x = X[self.lo:self.hi]
        self.dens = density
        self.state = _HostState()
        self._density = density  # (cached: the step is warm)
        self._parts_full = torch.zeros(1)

    def index_tensor(self, unl):
        return torch.as_tensor(np.asarray(unl), dtype=torch.int64)

    def local_select(self, u_full, parts_full, unl, forest, k, mode="dw", strategy="least_confidence", beta=1.0,
                     density_mode="gram", warm=None):
        assert parallel._soft_forest(forest, mode) and mode == "dw_soft"
        keys = torch.full((k,), parallel._as_i64(R.KEY_NONE), dtype=torch.int64)
        idx = torch.full((k,), -1, dtype=torch.int64)
        sc = torch.full((k,), float("nan"), dtype=torch.float64)
        unl = np.asarray(unl)
        mine = unl[(unl >= self.lo) & (unl < self.hi)]
        if mine.size:
            H = DW.entropy(R.sums(forest, self.x[mine - self.lo]), forest.n_trees)
            si, ss = DW.select_scores(DW.scores(H, self.dens[mine], beta), mine, k)
            kk = si.size
            keys[:kk] = torch.from_numpy(DW.score_key(ss).view(np.int64))
            idx[:kk] = torch.from_numpy(si)
            sc[:kk] = torch.from_numpy(ss)
        return parallel.LocalTopk(keys, idx, sc)


def _cpu_sort_positions(keys, pos, k):
    order = np.lexsort((pos.numpy(), keys.numpy().view(np.uint64)))[:k]
    return torch.from_numpy(order.astype(np.int64))


def _pool_1037():
    """The 1,037 x 30 three-class scikit-learn case of tests/test_soft_host.py (restated)."""
    from sklearn.ensemble import RandomForestClassifier

    n, d, T, depth, C = 1037, 30, 10, 4, 3
    rng = np.random.default_rng(1000 * C + d)
    X = rng.random((n, d)).astype(np.float32)
    y = (np.floor(X[:, 0] * C).astype(int) + (X[:, 1] > 0.6)) % C
    y[:C] = np.arange(C)
    rf = RandomForestClassifier(n_estimators=T, max_depth=depth, random_state=0, n_jobs=1).fit(X[:300], y[:300])
    return X, ProbabilityForest.from_sklearn(rf)


def test_dw_soft_refuses_a_hard_voting_forest():
    assert parallel.SOFT_DENSITY_MODES == ("dw_soft",) and "dw_soft" in parallel.ALL_DENSITY_MODES
    X, F = _pool_1037()
    dens = np.ones(1037)
    sels = [RestatementShard(X, dens, 1037, r, 2) for r in range(2)]
    unl = np.arange(10, 1037)
    for hard in (F.hard(), Forest.synthetic(10, 4, 30, seed=1)):
        with pytest.raises(ValueError, match="ProbabilityForest"):
            parallel.emulate(sels, unl, hard, 5, mode="dw_soft", sort_fn=_cpu_sort_positions)
        with pytest.raises(ValueError, match="ProbabilityForest"):
            parallel.select(sels[0], None, unl, hard, 5, mode="dw_soft")
        with pytest.raises(ValueError, match="ProbabilityForest"):
            parallel.ShardedSelector.local_select(sels[0], None, None, unl, hard, 5, mode="dw_soft")
    # the hard-vote modes keep refusing the soft forest
    for mode in ("dw", "dw_multiclass", "lal"):
        with pytest.raises(ValueError, match="soft votes"):
            parallel._soft_forest(F, mode)
    assert parallel._soft_forest(F, "us") and parallel._soft_forest(F, "dw_soft")


def test_emulate_merge_equals_the_single_selection():
    """1, 2, 3 and 5 shards of 1,037 rows (512-row granule: at 5 shards the
    last two hold no row at all), a rank whose rows are all labeled, and fewer
    candidates than k."""
    n, k = 1037, 25
    X, F = _pool_1037()
    E = np.arange(7)
    dens = O.density_canonical(X, E)
    H = DW.entropy(R.sums(F, X), F.n_trees)
    unl = np.arange(7, n)
    unl = unl[(unl < 512) | (unl >= 1024)]  # (at 3 shards rank 1 holds rows and no candidate)
    for beta in (1.0, 2.0):
        _, ref_idx, ref_sc = DW.select(X, unl, F, k, beta=beta, density=dens, H=H)
        assert np.unique(ref_sc).size == k and (ref_sc > 0.0).all()
        for world in (1, 2, 3, 5):
            sels = [RestatementShard(X, dens, n, r, world) for r in range(world)]
            if world == 5:
                assert sum(s.hi == s.lo for s in sels) >= 1
            idx, sc = parallel.emulate(sels, unl, F, k, mode="dw_soft", beta=beta, sort_fn=_cpu_sort_positions)
            assert np.array_equal(idx.numpy(), ref_idx), (beta, world)
            assert np.array_equal(sc.numpy(), ref_sc), (beta, world)
    # fewer candidates than k: the padding keys never reach the result
    few = unl[:9]
    idx, sc = parallel.emulate([RestatementShard(X, dens, n, r, 3) for r in range(3)], few, F, k, mode="dw_soft",
                               sort_fn=_cpu_sort_positions)
    _, ref_idx, ref_sc = DW.select(X, few, F, k, density=dens, H=H)
    assert idx.shape[0] == 9 and np.array_equal(idx.numpy(), ref_idx) and np.array_equal(sc.numpy(), ref_sc)


def test_run_loop_soft_information_density_arguments_and_restatement():
    from dal.loop import run_loop

    rng = np.random.default_rng(3)
    X = rng.random((240, 6)).astype(np.float32)
    y = (X[:, 0] * 3).astype(int).clip(0, 2)
    dens = O.density_canonical(X, np.arange(20))
    seen = []

    def select_fn(strategy, pool, unlabeled, model, k):
        assert strategy == "soft_information_density"
        F = ProbabilityForest.from_sklearn(model)
        seen.append(F.n_classes)
        return DW.select(pool, unlabeled, F, k, density=dens)[1]

    with pytest.raises(ValueError, match="trainer='gpu'"):  # the soft-vote uncertainty loop's message
        run_loop(X, y, strategy="soft_information_density", num_classes=3, max_iterations=1)
    with pytest.raises(ValueError, match="trainer='gpu'"):
        run_loop(X, y, strategy="soft_information_density", soft_votes=True, num_classes=3, max_iterations=1)
    with pytest.raises(ValueError, match="soft_votes"):  # the hard-vote strategy keeps refusing the flag
        run_loop(X, y, strategy="information_density", trainer="sklearn", soft_votes=True, max_iterations=1)
    with pytest.raises(ValueError, match="density_over"):
        run_loop(X, y, strategy="soft_information_density", trainer="sklearn", density_over="all", max_iterations=1)
    with pytest.raises(ValueError, match="alpha"):
        run_loop(X, y, strategy="soft_information_density", trainer="sklearn", alpha=0.5, max_iterations=1)
    kw = dict(strategy="soft_information_density", window_size=20, n_estimators=10, max_iterations=3, seed=4,
              trainer="sklearn", select_fn=select_fn)
    a = run_loop(X, y, **kw)
    b = run_loop(X, y, soft_votes=True, **kw)  # redundant, accepted
    c = run_loop(X, y, density_over="unlabeled", **kw)  # allowed (with select_fn only validated)
    assert len(a.labeled_history) == 3 and seen and set(seen) == {3}
    for u, v, w in zip(a.labeled_history, b.labeled_history, c.labeled_history):
        assert np.array_equal(u, v) and np.array_equal(u, w)
    picked = np.concatenate(a.labeled_history)
    assert np.unique(picked).size == 60 and picked.min() >= 20
