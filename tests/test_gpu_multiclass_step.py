"""The fused multiclass density step (dal_dw_step_multiclass) and its plan
(dal_dw_plan_create_multiclass) on the GPU.

Every case compares the selection (indices and canonical scores, bit for bit)
with tests/multiclass_dw_reference.select, and counts, pred, entropy,
row_index, scores, keys_lo, keys_hi bit for bit with what the unfused pair
(dal_forest_score_multiclass_dw_blocked, then dal_dw_select with lut = entropy,
votes = row_index) writes on the same inputs.  The shapes are chosen, and
asserted, with dal_dw_step_multiclass_form: one per branch of the step.
E = range(10) and unlabeled = range(10, n) unless a test says otherwise."""
import functools

import numpy as np
import pytest

import multiclass_dw_reference as DW
import multiclass_reference as R
from dal import _lib
from dal.forest import Forest
from oracle import dal_oracle as O

pytestmark = pytest.mark.gpu

E = np.arange(10)
EXACT, GROUP_MIN, FOLD_STORES, FOLD_ATOMICS = 0, 1, 2, 3
RESET, CLEAN = _lib.DAL_STEP_RESET_STATUS, _lib.DAL_STEP_WS_CLEAN

# (n, d, T, depth, C, k, form)
#   2,500 x 256          ragged last tile, one tile per group: plain-store fold
#   300,037 x 16         two tiles per group, a last group of one tile: atomics from different persistent blocks
#   1,037 x 30           17 tiles < 2k: the group-minimum pass after the blocked kernel
#   600 x 40             the blocked rule gives 0: the row-major kernel with the status and flag hooks
#   2,500 x 256, T 100   the eight-wave block
SHAPES = [
    (2500, 256, 10, 4, 10, 16, FOLD_STORES),
    (300_037, 16, 10, 4, 3, 20, FOLD_ATOMICS),
    (1037, 30, 10, 4, 3, 20, GROUP_MIN),
    (600, 40, 255, 8, 32, 10, GROUP_MIN),
    (2500, 256, 100, 4, 10, 16, FOLD_STORES),
]
BASE = SHAPES[0]


class Case:
    """A pool, a forest and their reference quantities (computed once, never written)."""

    def __init__(self, X, F, cnt=None, d=None):
        self.X, self.F, self.n, self.T = X, F, X.shape[0], F.n_trees
        self.cnt = R.counts(F, X) if cnt is None else cnt
        self.d = O.density_canonical(X, E) if d is None else d
        self.unl = np.arange(10, self.n)
        for a in (self.cnt, self.d):
            a.setflags(write=False)

    def other_forest(self, seed):
        """The same pool (and density) under another forest."""
        return Case(self.X, Forest.synthetic(self.T, self.F.depth, self.X.shape[1], seed=seed,
                                             n_classes=self.F.n_classes), d=self.d)

    def select(self, unl, k, beta=1.0):
        _, idx, sc, cnt = DW.select(self.X, unl, self.F, k, beta=beta, density=self.d, cnt=self.cnt)
        return idx, sc, cnt


@functools.lru_cache(maxsize=None)
def _case(n, d, T, depth, C):
    return Case(O.synthetic_pool(n, d, seed=n % 97), Forest.synthetic(T, depth, d, seed=5, n_classes=C))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Inputs:
    """What both routes read: the pool's caches (Gram density, norms, column
    sum), the row flags of ``cand`` and the blocked copy -- the engine's when
    the C-class rule allows one, else built here, so that the entry is handed
    an xb where the row-major kernel runs."""

    def __init__(self, cuda, case, cand):
        import torch

        from dal import engine
        from dal.engine import PoolState, _ptr, _stream

        self.state = st = PoolState(case.X, excluded=E, device=cuda)
        self.dens, self.norm64, self.colsum = st.density_fixed(), st.norms(), st.colsum()
        self.derr = float(engine.density_error(st))
        self.flags = st.row_flags(cand)[0]
        self.xb = st.blocked_pool(case.F, multiclass=True)
        if self.xb is None:
            lib = _lib.load()
            self.xb = torch.empty(int(lib.dal_pool_blocked_floats(st.n, st.d)), dtype=torch.float32, device=cuda)
            _lib.call("dal_pool_blocked", _ptr(st.x), st.n, st.d, st.d, _ptr(self.xb), _stream(cuda))
        self.fprep = engine._fprep(case.F, st, self.xb)
        self.inner, self.leaf = case.F.device(cuda)
        self.lut = engine.device_multiclass_lut("entropy", case.T, cuda)


NAMES = ("counts", "pred", "entropy", "row_index", "scores", "keys_lo", "keys_hi", "out_idx", "out_scores", "out_keys")


def _buffers(cuda, n, C, k):
    """Output buffers, filled: a row the step failed to write cannot pass by accident."""
    import torch

    def ints(shape, dt):
        return torch.full(shape, 0x5A, dtype=dt, device=cuda)

    def reals(m):
        return torch.full((m,), -7.0, dtype=torch.float64, device=cuda)

    return dict(counts=ints((n, C), torch.uint8), pred=ints((n,), torch.uint8), entropy=reals(n),
                row_index=ints((n,), torch.int32), scores=reals(n), keys_lo=ints((n,), torch.int64),
                keys_hi=ints((n,), torch.int64), out_idx=ints((k,), torch.int64), out_scores=reals(k),
                out_keys=ints((k,), torch.int64))


def _numpy(bufs, status):
    out = {name: t.cpu().numpy() for name, t in bufs.items() if t is not None}
    for name in ("entropy", "scores", "out_scores"):
        out[name] = _bits(out[name])
    out["status"] = int(status.item())
    return out


def _pair(cuda, case, I, k, cap, passes, beta):
    """The unfused pair, as C calls on the inputs the fused call gets."""
    import torch

    from dal.engine import _ptr, _stream, workspace

    lib = _lib.load()
    st, F = I.state, case.F
    n, C = st.n, int(F.n_classes)
    b = _buffers(cuda, n, C, k)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    _lib.call("dal_forest_score_multiclass_dw_blocked", _ptr(st.x), _ptr(I.xb), I.fprep, n, st.d, st.d,
              _ptr(I.inner), _ptr(I.leaf), F.n_trees, F.depth, C, _ptr(I.lut), _ptr(I.dens), _lib.DAL_DENSITY_FIXED,
              I.derr, _ptr(I.flags), float(beta), _ptr(b["counts"]), _ptr(b["pred"]), _ptr(b["entropy"]),
              _ptr(b["row_index"]), _ptr(b["scores"]), _ptr(b["keys_lo"]), _ptr(b["keys_hi"]), _stream(cuda))
    wsb = int(lib.dal_dw_select_workspace_bytes(n, k, cap))
    ws, wsp = workspace(wsb, cuda)
    _lib.call("dal_dw_select", _ptr(b["keys_lo"]), _ptr(b["keys_hi"]), _ptr(b["row_index"]), _ptr(I.flags), n, k, 0,
              _ptr(b["entropy"]), float(beta), _ptr(st.x), st.d, st.d, _ptr(I.norm64), _ptr(I.colsum), cap, passes,
              wsp, wsb, _ptr(b["out_idx"]), _ptr(b["out_scores"]), _ptr(b["out_keys"]), _ptr(status), 0,
              _stream(cuda))
    return _numpy(b, status)


def _fused(cuda, case, I, k, cap, passes, beta, step_flags=0, calls=1, with_counts=True):
    """dal_dw_step_multiclass, ``calls`` times on one workspace zeroed once;
    the outputs of every call (fresh buffers each)."""
    import torch

    from dal.engine import _ptr, _stream, workspace

    lib = _lib.load()
    st, F = I.state, case.F
    n, C = st.n, int(F.n_classes)
    wsb = int(lib.dal_dw_step_workspace_bytes(n, k, cap))
    ws, wsp = workspace(wsb, cuda)
    ws.zero_()
    outs = []
    for _ in range(calls):
        b = _buffers(cuda, n, C, k)
        if not with_counts:
            b["counts"] = b["pred"] = None
        # a set word: DAL_STEP_RESET_STATUS must clear it on the device
        status = torch.full((1,), _lib.DAL_FLAG_CAND_OVERFLOW if step_flags & RESET else 0, dtype=torch.int32,
                            device=cuda)
        _lib.call("dal_dw_step_multiclass", _ptr(st.x), _ptr(I.xb), I.fprep, n, st.d, st.d, _ptr(I.inner),
                  _ptr(I.leaf), F.n_trees, F.depth, C, _ptr(I.lut), _ptr(I.dens), I.derr, _ptr(I.flags), float(beta),
                  0, _ptr(I.norm64), _ptr(I.colsum), k, cap, passes, step_flags, wsp, wsb,
                  0 if b["counts"] is None else _ptr(b["counts"]), 0 if b["pred"] is None else _ptr(b["pred"]),
                  _ptr(b["entropy"]), _ptr(b["row_index"]), _ptr(b["scores"]), _ptr(b["keys_lo"]),
                  _ptr(b["keys_hi"]), _ptr(b["out_idx"]), _ptr(b["out_scores"]), _ptr(b["out_keys"]), _ptr(status),
                  0, _stream(cuda))
        outs.append(_numpy(b, status))
    return outs


def _check(cuda, case, k, form, cand=None, passes=1, beta=1.0, cap=None, with_counts=True):
    """One case: the form, the fused call against the pair, both against the reference."""
    from dal.engine import candidate_cap

    lib = _lib.load()
    n, d, F = case.n, case.X.shape[1], case.F
    cand = case.unl if cand is None else cand
    cap = candidate_cap(n, k) if cap is None else cap
    assert lib.dal_dw_step_multiclass_form(n, d, F.n_trees, F.depth, int(F.n_classes), k, cap, passes, 1) == form
    I = Inputs(cuda, case, cand)
    pair = _pair(cuda, case, I, k, cap, passes, beta)
    # plain, then twice with DAL_STEP_WS_CLEAN on one workspace: the second call
    # finds the header and the folded group minima as the first left them (zero)
    runs = _fused(cuda, case, I, k, cap, passes, beta, with_counts=with_counts)
    runs += _fused(cuda, case, I, k, cap, passes, beta, step_flags=RESET | CLEAN, calls=2, with_counts=with_counts)
    ref_idx, ref_sc, _ = case.select(cand, k, beta)
    assert pair["status"] == 0
    for got in runs:
        assert got["status"] == 0
        for name in NAMES:
            if name in got:
                assert np.array_equal(got[name], pair[name]), name
        assert np.array_equal(got["out_idx"], ref_idx)
    # the pair's per-row outputs are the reference's (so the comparison above is not of two wrong answers)
    assert np.array_equal(pair["counts"], case.cnt) and np.array_equal(pair["pred"], R.pred(case.cnt))
    assert np.array_equal(pair["entropy"], _bits(DW.entropy(case.cnt, case.T)))
    assert np.array_equal(pair["row_index"], np.arange(n))
    # the canonical scores against the reference, last (every run's equal the pair's, checked above)
    ulps = pair["out_scores"].astype(np.int64) - _bits(ref_sc).astype(np.int64)
    print(f"selected scores, fused - reference, in ulps: {ulps.tolist()}")
    assert np.array_equal(pair["out_scores"], _bits(ref_sc))


@pytest.mark.parametrize("n,d,T,depth,C,k,form", SHAPES)
def test_fused_step_equals_pair_and_reference(cuda, n, d, T, depth, C, k, form):
    _check(cuda, _case(n, d, T, depth, C), k, form)


def test_exact_level_one(cuda):
    n, d, T, depth, C, k, _ = BASE
    _check(cuda, _case(n, d, T, depth, C), k, EXACT, passes=0)


def test_beta_two(cuda):
    """The POW kernels.  The re-rank forms d^2 as d * d, the correctly rounded
    square that the reference's np.power(d, 2.0) gives too, so the selected
    scores are the reference's bits here as well."""
    n, d, T, depth, C, k, form = BASE
    _check(cuda, _case(n, d, T, depth, C), k, form, beta=2.0)


def test_counts_and_pred_null(cuda):
    n, d, T, depth, C, k, form = BASE
    _check(cuda, _case(n, d, T, depth, C), k, form, with_counts=False)


def test_non_candidates(cuda):
    """About 30 % of the rows are no candidates (seeded): DAL_KEY_NONE lanes in
    every tile's fold."""
    n, d, T, depth, C, k, form = BASE
    case = _case(n, d, T, depth, C)
    cand = case.unl[np.random.default_rng(5).random(case.unl.size) < 0.7]
    assert 0.6 * n < cand.size < 0.8 * n
    _check(cuda, case, k, form, cand=cand)


def _state(cuda, X):
    from dal.engine import PoolState

    return PoolState(X, excluded=E, device=cuda)


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "plan"])
def test_forced_retry(cuda, graphs):
    """cap_base = k: the first capacity overflows, the engine re-runs with a
    larger one (or the exact level 1) and the same selection comes out."""
    from dal import density_weighting as dw

    n, d, T, depth, C, k, _ = BASE
    case = _case(n, d, T, depth, C)
    ref_idx, ref_sc, ref_cnt = case.select(case.unl, k)
    st = _state(cuda, case.X)
    st.use_graphs = graphs
    dw.select_multiclass(st, case.unl, case.F, k)  # cold
    st.cap_base = k
    for _ in range(2):
        sel = dw.select_multiclass(st, case.unl, case.F, k)
        assert np.array_equal(sel.indices.cpu().numpy(), ref_idx)
        assert np.array_equal(_bits(sel.selected_scores.cpu().numpy()), _bits(ref_sc))
        assert np.array_equal(sel.counts.cpu().numpy(), ref_cnt)
    assert st.cap_scale > 1 or not st.level1_fast  # the first capacity did overflow
    assert (len(st._graphs) >= 1) == graphs


# ------------------------------------------------------------------ plan --
PLAN = (6000, 32, 10, 4, 4, 20)  # n, d, T, depth, C, k


def test_plan_stamps_wrap(cuda):
    """The C-class twin of tests/test_gpu_plan_stamps.py: 300 replays of one
    plan, the unlabeled list halved after replay 1; a row listed at replay 1
    only must not come back at replay 256, when the 8-bit step id is 1 again."""
    import torch

    from dal import density_weighting as dw

    n, d, T, depth, C, k = PLAN
    assert _lib.load().dal_dw_step_multiclass_form(n, d, T, depth, C, k, 4096, 1, 1) == FOLD_STORES
    case = _case(n, d, T, depth, C)
    full, half = np.arange(10, n), np.arange(10, n // 2)
    ref_full, ref_full_ss, _ = case.select(full, k)
    ref_half, ref_half_ss, _ = case.select(half, k)
    assert not np.isin(ref_full, half).all()  # the full list's top rows are not all in the half
    st = _state(cuda, case.X)
    half_dev, full_dev = torch.from_numpy(half).to(cuda), torch.from_numpy(full).to(cuda)
    dw.select_multiclass(st, full_dev, case.F, k)  # cold
    assert len(st._graphs) == 0
    for step in range(1, 301):
        sel = dw.select_multiclass(st, full_dev if step == 1 else half_dev, case.F, k)
        got = sel.indices.cpu().numpy()
        if step == 1:
            assert np.array_equal(got, ref_full)
            assert np.array_equal(_bits(sel.selected_scores.cpu().numpy()), _bits(ref_full_ss))
        elif step in (2, 254, 255, 256, 257, 300):
            assert np.array_equal(got, ref_half), step
            assert np.array_equal(_bits(sel.selected_scores.cpu().numpy()), _bits(ref_half_ss)), step
        else:
            assert got.max() < n // 2, step
    assert len(st._graphs) == 1  # one plan replayed throughout
    (key,) = st._graphs
    assert key[-1] == C


def test_plan_forests_and_kept_selection(cuda):
    """One plan serves a second forest of the same shape; a forest with another
    C builds a second plan; a Selection kept across replays still reads its own
    step's counts and scores."""
    from dal import density_weighting as dw
    from dal import engine

    n, d, T, depth, C, k = PLAN
    a = _case(n, d, T, depth, C)
    b = a.other_forest(seed=9)
    c = Case(a.X, Forest.synthetic(T, depth, d, seed=5, n_classes=C + 1), d=a.d)
    assert not np.array_equal(a.cnt, b.cnt)
    st = _state(cuda, a.X)
    derr = engine.density_error(st)
    dw.select_multiclass(st, a.unl, a.F, k)  # cold
    kept = {}
    for name, case in (("a", a), ("b", b), ("a2", a), ("c", c), ("b2", b)):
        sel = dw.select_multiclass(st, case.unl, case.F, k)
        idx, sc, _ = case.select(case.unl, k)
        assert np.array_equal(sel.indices.cpu().numpy(), idx), name
        assert np.array_equal(_bits(sel.selected_scores.cpu().numpy()), _bits(sc)), name
        kept[name] = (sel, case)
        assert len(st._graphs) == (1 if name in ("a", "b", "a2") else 2), name
    assert sorted(key[-1] for key in st._graphs) == [C, C + 1]
    # read only now, after later replays reused the plans' buffers
    for name, (sel, case) in kept.items():
        assert sel.votes is None
        assert np.array_equal(sel.counts.cpu().numpy(), case.cnt[case.unl]), name
        H = DW.entropy(case.cnt[case.unl], T)
        ref = DW.scores(H, case.d[case.unl])
        got = sel.scores.cpu().numpy()
        # (the per-row scores come from the Gram density: within its bound of the canonical ones)
        assert got.shape == ref.shape and (np.abs(got - ref) <= H * derr + 1e-15 * np.abs(ref)).all(), name
    sa, sa2 = kept["a"][0].scores.cpu().numpy(), kept["a2"][0].scores.cpu().numpy()
    sb = kept["b"][0].scores.cpu().numpy()
    assert np.array_equal(_bits(sa), _bits(sa2)) and not np.array_equal(_bits(sa), _bits(sb))


def test_run_loop_equals_eager(cuda, monkeypatch):
    """run_loop(strategy="information_density", trainer="gpu", num_classes=3),
    5 iterations: the plan's history equals the eager steps'."""
    from dal import engine
    from dal.loop import run_loop

    rng = np.random.default_rng(17)
    X = rng.random((600, 8)).astype(np.float32)
    y = (X[:, 0] * 3).astype(int).clip(0, 2) * 2 + 5  # labels 5, 7, 9
    kw = dict(strategy="information_density", window_size=20, n_estimators=10, max_iterations=5, seed=4,
              trainer="gpu", num_classes=3, device=cuda)
    states = []

    class Recorded(engine.PoolState):
        use_graphs_default = True

        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            self.use_graphs = self.use_graphs_default
            states.append(self)

    monkeypatch.setattr(engine, "PoolState", Recorded)
    got = run_loop(X, y, **kw)
    Recorded.use_graphs_default = False
    ref = run_loop(X, y, **kw)
    plan_state, eager_state = states
    assert len(plan_state._graphs) >= 1 and len(eager_state._graphs) == 0  # the warm iterations replayed a plan
    assert len(got.labeled_history) == 5
    for a, b in zip(got.labeled_history, ref.labeled_history):
        assert np.array_equal(np.asarray(a), np.asarray(b))
