"""Strided and unaligned fp32 pools through the C ABI (include/dal.h: "Pool
rows are fp32, row-major with leading dimension ldx").

Every entry that takes an ``ldx`` is called directly (dal._lib.call) on a view
of row stride ldx > d, or with its first row off the allocation's 16-byte
alignment, whose every non-logical element is NaN (tests/strided_pool.py).
Each case asserts, bit for bit,
  (a) the outputs equal the plain high-precision reference of the LOGICAL
      matrix -- the reference the entry's contiguous test uses;
  (b) the outputs equal the same entry on the contiguous copy with ldx = d;
and that the input buffer, padding included, is byte-identical afterwards.
No tolerance appears anywhere.

The forest cases also assert, through the restated predicates
(strided_pool.forest_tiling), which staging branch and rows-per-block they
reach: the row-major kernels choose between LDS-DMA, 16-byte and 4-byte
staging from d, ldx and the pool's address.

Negative check (done once by hand on a scratch build, not committed): with
forest_score_kernel's scalar staging indexing rows by A.d in place of A.ldx,
the (ldx, offset) = (65, 0) and (129, 0) cases of test_forest_score fail
assertion (a) on the votes.
"""
import ctypes
import functools

import numpy as np
import pytest

import metrics_reference as MET
import multiclass_dw_reference as DW
import multiclass_reference as MR
import pairs_reference as PR
import rf_multiclass_reference as M
import strided_pool as SP
from conftest import load_golden
from dal import _lib
from dal.forest import Forest
from oracle import dal_oracle as O

pytestmark = pytest.mark.gpu

CAND, EXCL = _lib.DAL_ROW_CANDIDATE, _lib.DAL_ROW_EXCLUDED
KEY_NONE, KEY_NAN = np.uint64(_lib.DAL_KEY_NONE), np.uint64(_lib.DAL_KEY_NAN)


# ---------------------------------------------------------------- plumbing --
def _stream(cuda):
    import torch

    return torch.cuda.current_stream(cuda).cuda_stream


def _dev(cuda, a, dtype=None):
    import torch

    return torch.from_numpy(np.array(a, dtype=dtype)).to(cuda)  # (a copy: the cases are read-only)


def _filled(cuda, shape, dtype, value):
    """An output buffer holding a sentinel no entry writes."""
    import torch

    return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=dtype, device=cuda)


def _np(t):
    return t.cpu().numpy()


def _u64(t):
    return _np(t).view(np.uint64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    """Equal dtype, shape and bytes (NaN payloads and signed zeros included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _layouts(cuda, X, ldx, off):
    """((strided view, ldx), (contiguous copy, d)) of the logical matrix."""
    return (SP.strided(X, ldx, off, cuda), ldx), (SP.contiguous(X, cuda), X.shape[1])


def _workspace(cuda, nbytes):
    import torch

    ws = torch.zeros(int(nbytes) + 256, dtype=torch.uint8, device=cuda)
    return ws, (ws.data_ptr() + 255) // 256 * 256


def score_key(s, descending):
    """dal_score_key (csrc/common.hpp score_key): -0.0 -> +0.0, NaN ->
    DAL_KEY_NAN, smaller = better."""
    s = np.asarray(s, dtype=np.float64) + 0.0
    b = s.view(np.uint64)
    u = np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))
    return np.where(np.isnan(s), KEY_NAN, ~u if descending else u)


def interval_keys(e, acc, derr, flags):
    """The density mode's scores and interval keys at beta == 1, descending
    (include/dal.h, dal_forest_score / dal_forest_score_multiclass_dw):
    d = acc 2^-32 (NaN for EXCLUDED rows), score = e d, half-width
    max(|e| density_err, |score| 4.5e-16) unless the score is exact (e zero or
    NaN, d NaN); keys = the pessimistic end's, keys_hi = the optimistic end's,
    DAL_KEY_NONE when the row is no candidate.  One fp64 operation each."""
    d = acc.astype(np.float64) * 2.0 ** -32
    d = np.where(flags & EXCL, np.nan, d)
    with np.errstate(invalid="ignore"):
        s = e * d
        exact = np.isnan(e) | (e == 0.0) | np.isnan(d)
        err = np.where(exact, 0.0, np.maximum(np.abs(e) * derr, np.abs(s) * 4.5e-16))
        lo, hi = s + -err, s + err
    cand = (flags & CAND) != 0
    return s, np.where(cand, score_key(lo, True), KEY_NONE), np.where(cand, score_key(hi, True), KEY_NONE)


def _assert_scores(got, ref):
    """Bit for bit, signed zeros included; a NaN is a NaN (its payload is not part of the contract)."""
    ok = ~np.isnan(ref)
    assert np.array_equal(np.isnan(got), ~ok)
    assert np.array_equal(_bits(got[ok]), _bits(ref[ok]))


# ============================================================ forest cases ==
N, DEPTH = 700, 4  # the last tile is ragged for every R below
EDGE_THRESHOLD = 0.5  # of the two roots that test the first and the last feature
E_ROWS = np.array([0, 255, 256, N - 1])

# (d, ldx, offset_elems, T, staging, R): the branch the case must reach
FOREST_CASES = [
    (30, 33, 0, 10, "scalar", 128),    # scalar staging, strided
    (64, 68, 0, 10, "vec4", 64),       # 16-byte staging with a row stride
    (64, 65, 0, 10, "scalar", 64),     # scalar staging at d % 4 == 0: odd stride
    (64, 64, 1, 10, "scalar", 64),     # ... and a pool 4 bytes off 16-byte alignment
    (128, 132, 0, 10, "dma", 64),      # LDS-DMA, persistent grid, with a row stride
    (128, 129, 0, 10, "scalar", 32),   # scalar staging at d >= 128: non-persistent grid, R = 32
    (128, 128, 1, 10, "scalar", 32),
    (260, 260, 0, 10, "dma", 16),      # rows over 1 KiB: a second DMA piece with one live lane
    (260, 264, 0, 10, "dma", 16),
    (1028, 1028, 0, 10, "none", 256),  # no LDS staging (x_lds false)
    (1028, 1029, 0, 10, "none", 256),
    (64, 68, 0, 100, "vec4", 64),      # T >= 64 (tpr_min = 2; R already leaves 4 lanes per row here)
    (128, 132, 0, 100, "dma", 64),
    (12, 16, 0, 100, "vec4", 128),     # ... and where tpr_min does shrink R: a 256-row tile (d <= 15) halved
    (13, 14, 0, 100, "scalar", 128),
]
_IDS = [f"d{d}-ldx{l}-off{o}-T{t}" for d, l, o, t, _, _ in FOREST_CASES]
forest_cases = pytest.mark.parametrize("d,ldx,off,T,staging,R", FOREST_CASES, ids=_IDS)


def _assert_branch(view, d, ldx, T, staging, R):
    """The case reaches the staging branch and the rows per block the table
    names (both row-major launchers use 256-thread blocks), the last tile is
    ragged, and d = 260's second DMA piece has one live lane.  (The table
    itself is checked without a GPU by tests/test_strided_host.py.)"""
    t = SP.forest_tiling(d, ldx, view.data_ptr(), T)
    assert (t.staging, t.R) == (staging, R), t
    assert N % R != 0
    assert d != 260 or (staging == "dma" and SP.dma_pieces(d) == (2, 1))


@functools.lru_cache(maxsize=None)
def _edge_forest(d, T):
    """O.synthetic_forest with tree 0's root testing feature d - 1 and tree
    1's root feature 0, both at 0.5 (half the rows each way): a read one
    column into the padding, or one column short, changes votes."""
    of = O.synthetic_forest(T, DEPTH, d, seed=7)
    for t, f in ((0, d - 1), (1, 0)):
        of.feature[of.roots[t]], of.threshold[of.roots[t]] = f, EDGE_THRESHOLD
    return of


@functools.lru_cache(maxsize=None)
def _pool(d):
    """The logical pool of every forest case at d (read-only): rows 0..3 sit
    exactly on the two edge roots' threshold (they go left) and one fp32 ulp
    above it (they go right)."""
    X = O.synthetic_pool(N, d, seed=100 + d)
    thr = np.float32(EDGE_THRESHOLD)
    X[0, d - 1], X[1, d - 1] = thr, np.nextafter(thr, np.float32(np.inf))
    X[2, 0], X[3, 0] = thr, np.nextafter(thr, np.float32(np.inf))
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _flags():
    """EXCLUDED on E_ROWS, DAL_ROW_CANDIDATE on ~70 % of the rows (the last
    row is an excluded candidate, row 1 a plain one)."""
    f = (np.random.default_rng(5).random(N) < 0.7).astype(np.uint8) * np.uint8(CAND)
    f[[1, N - 1]] |= np.uint8(CAND)
    f[E_ROWS] |= np.uint8(EXCL)
    f.setflags(write=False)
    return f


class BinaryCase:
    def __init__(self, d, T):
        self.X, self.of = _pool(d), _edge_forest(d, T)
        of = self.of
        self.F = Forest.from_nodes(of.feature, of.threshold, of.left, of.right, of.value, of.roots)
        assert self.F.depth == DEPTH and self.F.inner[0, 0, 0] == d - 1 and self.F.inner[1, 0, 0] == 0
        self.votes = O.votes(of, self.X)
        # the edge features decide votes: a kernel reading padding (NaN goes right) there is seen
        for col in (0, d - 1):
            Xs = self.X.copy()
            Xs[:, col] = np.nan
            assert (O.votes(of, Xs) != self.votes).sum() > N // 20
        self.votes.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _binary_case(d, T):
    return BinaryCase(d, T)


def _edge_multiclass_forest(T, d, C):
    """Forest.synthetic with the two edge roots of _edge_forest."""
    F = Forest.synthetic(T, DEPTH, d, seed=5, n_classes=C)
    half = np.array([EDGE_THRESHOLD], dtype=np.float32).view(np.int32)[0]
    F.inner[0, 0], F.inner[1, 0] = (d - 1, half), (0, half)
    return F


class MultiCase:
    def __init__(self, d, T, C):
        self.X = _pool(d)
        F = _edge_multiclass_forest(T, d, C)
        self.F, self.T, self.C = F, T, C
        self.cnt = MR.counts(F, self.X)
        assert (self.cnt.sum(axis=1) == T).all()
        for col in (0, d - 1):
            Xs = self.X.copy()
            Xs[:, col] = np.inf  # (an fp32 compare: +inf goes right, as a NaN does)
            assert (MR.counts(F, Xs) != self.cnt).any(axis=1).sum() > N // 20
        self.H = DW.entropy(self.cnt, T)
        self.cnt.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _multi_case(d, T, C):
    return MultiCase(d, T, C)


_DENSITY = {}


def _density(cuda, d):
    """(Gram density int64 [N], its error bound, canonical density fp64 [N])
    of the logical pool at d with E = E_ROWS: inputs without an ldx, from a
    contiguous PoolState."""
    if d not in _DENSITY:
        from dal import engine

        st = engine.PoolState(np.array(_pool(d)), excluded=E_ROWS, device=cuda)  # (a copy: the pool is read-only)
        acc = _np(st.density_fixed())[:N].copy()
        derr = float(engine.density_error(st))
        canon = O.density_canonical(_pool(d), E_ROWS)
        assert derr > 0.0 and np.array_equal(np.isnan(canon), np.isin(np.arange(N), E_ROWS))
        assert np.abs(acc * 2.0 ** -32 - canon)[~np.isnan(canon)].max() <= derr
        _DENSITY[d] = (acc, derr, canon)
    return _DENSITY[d]


# --------------------------------------------------------- dal_forest_score --
def _forest_score(cuda, x, ldx, F, lut, flags, order, density=None, kind=_lib.DAL_DENSITY_NONE, derr=0.0):
    import torch

    n, d = x.shape
    inner, leaf = F.device(cuda)
    votes = _filled(cuda, n, torch.int32, -7)
    scores = _filled(cuda, n, torch.float64, -7.0)
    keys = _filled(cuda, n, torch.int64, 0x5555)
    keys_hi = _filled(cuda, n, torch.int64, 0x5555)
    lut_d, fl_d = _dev(cuda, lut), _dev(cuda, flags)
    dens = None if density is None else _dev(cuda, density)
    _lib.call("dal_forest_score", x.data_ptr(), n, d, ldx, inner.data_ptr(), leaf.data_ptr(), F.n_trees, F.depth,
              lut_d.data_ptr(), 0 if dens is None else dens.data_ptr(), kind, derr, fl_d.data_ptr(), 1.0, order,
              votes.data_ptr(), scores.data_ptr(), keys.data_ptr(), keys_hi.data_ptr(), _stream(cuda))
    return _np(votes), _np(scores), _u64(keys), _u64(keys_hi)


@forest_cases
def test_forest_score(cuda, d, ldx, off, T, staging, R):
    """dal_forest_score: uncertainty mode (ascending and descending tables)
    and DAL_DENSITY_FIXED with keys_hi."""
    case, flags = _binary_case(d, T), _flags()
    (xs, ls), (xc, lc) = _layouts(cuda, case.X, ldx, off)
    _assert_branch(xs, d, ldx, T, staging, R)
    cand = (flags & CAND) != 0
    for strategy in ("least_confidence", "entropy"):
        lut, desc = O.lut(strategy, T), not O.ASCENDING[strategy]
        order = _lib.DAL_DESCENDING if desc else _lib.DAL_ASCENDING
        v, s, k, kh = _forest_score(cuda, xs, ls, case.F, lut, flags, order)
        assert np.array_equal(v, case.votes), strategy                                   # (a)
        _assert_scores(s, lut[case.votes])
        ref_keys = np.where(cand, score_key(lut[case.votes], desc), KEY_NONE)
        assert np.array_equal(k, ref_keys) and np.array_equal(kh, ref_keys)
        for a, b in zip((v, s, k, kh), _forest_score(cuda, xc, lc, case.F, lut, flags, order)):  # (b)
            assert _same(a, b), strategy
    acc, derr, _ = _density(cuda, d)
    lut = O.lut("entropy", T)
    v, s, k, kh = _forest_score(cuda, xs, ls, case.F, lut, flags, _lib.DAL_DESCENDING, acc, _lib.DAL_DENSITY_FIXED,
                                derr)
    ref_s, ref_lo, ref_hi = interval_keys(lut[case.votes], acc, derr, flags)
    assert np.array_equal(v, case.votes)                                                 # (a)
    _assert_scores(s, ref_s)
    assert np.array_equal(k, ref_lo) and np.array_equal(kh, ref_hi)
    assert (k[cand] >= kh[cand]).all() and (k[cand] > kh[cand]).sum() > N // 4  # real intervals
    for a, b in zip((v, s, k, kh), _forest_score(cuda, xc, lc, case.F, lut, flags, _lib.DAL_DESCENDING, acc,
                                                 _lib.DAL_DENSITY_FIXED, derr)):        # (b)
        assert _same(a, b)
    SP.assert_unchanged(xs)


# ------------------------------------- dal_forest_score_multiclass (and _dw) --
def _mc_outputs(cuda, n, C):
    import torch

    return dict(counts=_filled(cuda, (n, C), torch.uint8, 0xEE), pred=_filled(cuda, n, torch.uint8, 0xEE),
                scores=_filled(cuda, n, torch.float64, -7.0), keys=_filled(cuda, n, torch.int64, 0x5555))


def _score_multiclass(cuda, x, ldx, F, strategy, flags, xb=None, fprep=None):
    """dal_forest_score_multiclass, or with ``xb`` its _blocked form."""
    from dal import luts

    n, d = x.shape
    inner, leaf = F.device(cuda)
    o = _mc_outputs(cuda, n, int(F.n_classes))
    lut_d, fl_d = _dev(cuda, luts.multiclass_lut(strategy, F.n_trees)), _dev(cuda, flags)
    order = _lib.DAL_ASCENDING if MR.ASCENDING[strategy] else _lib.DAL_DESCENDING
    kind = {"least_confidence": _lib.DAL_MC_LEAST_CONFIDENCE, "margin": _lib.DAL_MC_MARGIN,
            "entropy": _lib.DAL_MC_ENTROPY}[strategy]
    args = (n, d, ldx, inner.data_ptr(), leaf.data_ptr(), F.n_trees, F.depth, int(F.n_classes), lut_d.data_ptr(), kind,
            fl_d.data_ptr(), order, o["counts"].data_ptr(), o["pred"].data_ptr(), o["scores"].data_ptr(),
            o["keys"].data_ptr(), _stream(cuda))
    if xb is None:
        _lib.call("dal_forest_score_multiclass", x.data_ptr(), *args)
    else:
        _lib.call("dal_forest_score_multiclass_blocked", x.data_ptr(), xb.data_ptr(),
                  0 if fprep is None else fprep.data_ptr(), *args)
    return _np(o["counts"]), _np(o["pred"]), _np(o["scores"]), _u64(o["keys"])


def _check_multiclass(case, strategy, flags, got):
    c, p, s, k = got
    assert c.dtype == np.uint8 and np.array_equal(c, case.cnt), strategy
    assert np.array_equal(p, MR.pred(case.cnt))
    ref = MR.scores(case.cnt, case.T, strategy)
    assert np.array_equal(_bits(s), _bits(ref)), strategy
    cand = (flags & CAND) != 0
    assert np.array_equal(k, np.where(cand, score_key(ref, not MR.ASCENDING[strategy]), KEY_NONE))


@pytest.mark.parametrize("C", [3, 32])
@forest_cases
def test_forest_score_multiclass(cuda, d, ldx, off, T, staging, R, C):
    case, flags = _multi_case(d, T, C), _flags()
    (xs, ls), (xc, lc) = _layouts(cuda, case.X, ldx, off)
    _assert_branch(xs, d, ldx, T, staging, R)
    for strategy in MR.STRATEGIES:
        got = _score_multiclass(cuda, xs, ls, case.F, strategy, flags)
        _check_multiclass(case, strategy, flags, got)                                    # (a)
        for a, b in zip(got, _score_multiclass(cuda, xc, lc, case.F, strategy, flags)):  # (b)
            assert _same(a, b), strategy
    SP.assert_unchanged(xs)


def _score_multiclass_dw(cuda, x, ldx, F, flags, density, kind, derr):
    import torch

    from dal import luts

    n, d = x.shape
    inner, leaf = F.device(cuda)
    o = _mc_outputs(cuda, n, int(F.n_classes))
    o.update(entropy=_filled(cuda, n, torch.float64, -7.0), row_index=_filled(cuda, n, torch.int32, -7),
             keys_hi=_filled(cuda, n, torch.int64, 0x5555))
    lut_d, fl_d, dens = _dev(cuda, luts.multiclass_lut("entropy", F.n_trees)), _dev(cuda, flags), _dev(cuda, density)
    _lib.call("dal_forest_score_multiclass_dw", x.data_ptr(), n, d, ldx, inner.data_ptr(), leaf.data_ptr(),
              F.n_trees, F.depth, int(F.n_classes), lut_d.data_ptr(), dens.data_ptr(), kind, derr, fl_d.data_ptr(), 1.0,
              o["counts"].data_ptr(), o["pred"].data_ptr(), o["entropy"].data_ptr(), o["row_index"].data_ptr(),
              o["scores"].data_ptr(), o["keys"].data_ptr(), o["keys_hi"].data_ptr(), _stream(cuda))
    return (_np(o["counts"]), _np(o["pred"]), _np(o["entropy"]), _np(o["row_index"]), _np(o["scores"]),
            _u64(o["keys"]), _u64(o["keys_hi"]))


@pytest.mark.parametrize("C", [3, 32])
@forest_cases
def test_forest_score_multiclass_dw(cuda, d, ldx, off, T, staging, R, C):
    """Class entropy x density: DAL_DENSITY_EXACT (canonical scores, point
    intervals) and DAL_DENSITY_FIXED (interval keys)."""
    case, flags = _multi_case(d, T, C), _flags()
    (xs, ls), (xc, lc) = _layouts(cuda, case.X, ldx, off)
    _assert_branch(xs, d, ldx, T, staging, R)
    acc, derr, canon = _density(cuda, d)
    cand = (flags & CAND) != 0
    for kind, dens, err in ((_lib.DAL_DENSITY_EXACT, canon, 0.0), (_lib.DAL_DENSITY_FIXED, acc, derr)):
        got = _score_multiclass_dw(cuda, xs, ls, case.F, flags, dens, kind, err)
        c, p, h, ix, s, k, kh = got
        assert np.array_equal(c, case.cnt) and np.array_equal(p, MR.pred(case.cnt))      # (a)
        assert np.array_equal(_bits(h), _bits(case.H))
        assert ix.dtype == np.int32 and np.array_equal(ix, np.arange(N))
        if kind == _lib.DAL_DENSITY_EXACT:
            ref_s = DW.scores(case.H, canon)
            ref_lo = ref_hi = np.where(cand, DW.score_key(ref_s), KEY_NONE)
        else:
            ref_s, ref_lo, ref_hi = interval_keys(case.H, acc, derr, flags)
        _assert_scores(s, ref_s)
        assert np.array_equal(k, ref_lo) and np.array_equal(kh, ref_hi)
        for a, b in zip(got, _score_multiclass_dw(cuda, xc, lc, case.F, flags, dens, kind, err)):  # (b)
            assert _same(a, b)
    SP.assert_unchanged(xs)


# ------------------------------------------------------ dal_forest_evaluate --
def _evaluate(cuda, x, ldx, F, y, flags):
    import torch

    n, d = x.shape
    inner, leaf = F.device(cuda)
    C = int(F.n_classes)
    cells = int(_lib.load().dal_forest_evaluate_cells(F.n_trees, C))
    hist = torch.zeros(cells, dtype=torch.int64, device=cuda)
    y_d, fl_d = _dev(cuda, y, np.uint8), _dev(cuda, flags)
    _lib.call("dal_forest_evaluate", x.data_ptr(), 0, 0, n, d, ldx, inner.data_ptr(), leaf.data_ptr(), F.n_trees,
              F.depth, C, y_d.data_ptr(), fl_d.data_ptr(), hist.data_ptr(), _stream(cuda))
    return _np(hist).reshape((F.n_trees + 1, 2) if C == 2 else (C, C))


@pytest.mark.parametrize("C", [2, 3])
@forest_cases
def test_forest_evaluate_rows(cuda, d, ldx, off, T, staging, R, C):
    """xb = fprep = NULL: the row kernel on the strided x (one thread per
    row, no staging: the table's branch columns do not apply)."""
    F = _binary_case(d, T).F if C == 2 else _multi_case(d, T, C).F
    X, flags = _pool(d), _flags()
    y = np.random.default_rng(d + C).integers(0, C, N).astype(np.uint8)
    (xs, ls), (xc, lc) = _layouts(cuda, X, ldx, off)
    got = _evaluate(cuda, xs, ls, F, y, flags)
    want = np.array(MET.joint_table(F, X, y, flags=flags), dtype=np.int64)
    assert int(want.sum()) == int(((flags & CAND) != 0).sum())
    assert np.array_equal(got, want)                                                     # (a)
    assert _same(got, _evaluate(cuda, xc, lc, F, y, flags))                              # (b)
    SP.assert_unchanged(xs)


# ---------------------------------------------- blocked copy and its kernels --
def _pool_blocked(cuda, x, ldx):
    import torch

    n, d = x.shape
    floats = int(_lib.load().dal_pool_blocked_floats(n, d))
    xb = _filled(cuda, floats, torch.float32, float("nan"))
    _lib.call("dal_pool_blocked", x.data_ptr(), n, d, ldx, xb.data_ptr(), _stream(cuda))
    assert xb.data_ptr() % 16 == 0
    return xb


@pytest.mark.parametrize("d", [30, 64, 260])
@pytest.mark.parametrize("pad,off", [(1, 0), (4, 0), (0, 1)])
def test_pool_blocked(cuda, d, pad, off):
    """xb[(t * d + f) * 64 + r] = x[t * 64 + r][f], zeros past n."""
    X = _pool(d)
    (xs, ls), (xc, lc) = _layouts(cuda, X, d + pad, off)
    tiles = (N + 63) // 64
    ref = np.zeros((tiles * 64, d), dtype=np.float32)
    ref[:N] = X
    ref = ref.reshape(tiles, 64, d).transpose(0, 2, 1).reshape(-1)
    got = _np(_pool_blocked(cuda, xs, ls))
    assert _same(got, ref)                                                               # (a)
    assert _same(got, _np(_pool_blocked(cuda, xc, lc)))                                  # (b)
    SP.assert_unchanged(xs)


def _fprep(cuda, F, d):
    import torch

    nb = int(_lib.load().dal_forest_prep_bytes(d, F.n_trees, F.depth))
    if nb == 0:
        return None
    inner, leaf = F.device(cuda)
    buf = torch.empty(nb, dtype=torch.uint8, device=cuda)
    _lib.call("dal_forest_prepare", inner.data_ptr(), leaf.data_ptr(), F.n_trees, F.depth, d, buf.data_ptr(), nb,
              _stream(cuda))
    return buf


# (d, ldx, off, T, blocked): T = 100 at d = 260 tests 260 > 256 distinct
# features at most: dal_forest_blocked_rows is 0 and the entries fall back to
# the row-major kernel on the strided x; elsewhere xb, built by
# dal_pool_blocked from the strided x, is what the kernel reads.
BLOCKED_CASES = [(260, 264, 0, 100, False), (260, 261, 0, 100, False), (64, 65, 0, 10, True), (64, 68, 0, 10, True),
                 (128, 129, 0, 10, True), (30, 30, 1, 10, True)]
blocked_cases = pytest.mark.parametrize("d,ldx,off,T,blocked", BLOCKED_CASES)


@blocked_cases
def test_forest_score_blocked(cuda, d, ldx, off, T, blocked):
    import torch

    case, flags = _binary_case(d, T), _flags()
    assert bool(_lib.load().dal_forest_blocked_rows(d, T, DEPTH)) == blocked
    (xs, ls), _ = _layouts(cuda, case.X, ldx, off)
    xb, F = _pool_blocked(cuda, xs, ls), case.F
    inner, leaf = F.device(cuda)
    acc, derr, _ = _density(cuda, d)
    lut = O.lut("entropy", T)
    lut_d, fl_d, dens = _dev(cuda, lut), _dev(cuda, flags), _dev(cuda, acc)
    ref_s, ref_lo, ref_hi = interval_keys(lut[case.votes], acc, derr, flags)
    rowmajor = _forest_score(cuda, xs, ls, F, lut, flags, _lib.DAL_DESCENDING, acc, _lib.DAL_DENSITY_FIXED, derr)
    for prep in ((None, _fprep(cuda, F, d)) if blocked else (None,)):
        assert blocked or prep is None
        votes = _filled(cuda, N, torch.int32, -7)
        scores = _filled(cuda, N, torch.float64, -7.0)
        keys, keys_hi = _filled(cuda, N, torch.int64, 0x5555), _filled(cuda, N, torch.int64, 0x5555)
        _lib.call("dal_forest_score_blocked", xs.data_ptr(), xb.data_ptr(), 0 if prep is None else prep.data_ptr(), N,
                  d, ls, inner.data_ptr(), leaf.data_ptr(), T, DEPTH, lut_d.data_ptr(), dens.data_ptr(),
                  _lib.DAL_DENSITY_FIXED, derr, fl_d.data_ptr(), 1.0, _lib.DAL_DESCENDING, votes.data_ptr(),
                  scores.data_ptr(), keys.data_ptr(), keys_hi.data_ptr(), _stream(cuda))
        got = (_np(votes), _np(scores), _u64(keys), _u64(keys_hi))
        assert np.array_equal(got[0], case.votes)                                        # (a)
        _assert_scores(got[1], ref_s)
        assert np.array_equal(got[2], ref_lo) and np.array_equal(got[3], ref_hi)
        for a, b in zip(got, rowmajor):                                                  # (b) dal_forest_score's bits
            assert _same(a, b)
    SP.assert_unchanged(xs)


@pytest.mark.parametrize("C", [3, 32])
@blocked_cases
def test_forest_score_multiclass_blocked(cuda, d, ldx, off, T, blocked, C):
    case, flags = _multi_case(d, T, C), _flags()
    assert bool(_lib.load().dal_forest_multiclass_blocked_rows(d, T, DEPTH, C)) == blocked
    (xs, ls), (xc, lc) = _layouts(cuda, case.X, ldx, off)
    xb, prep = _pool_blocked(cuda, xs, ls), _fprep(cuda, case.F, d)
    for strategy in MR.STRATEGIES:
        got = _score_multiclass(cuda, xs, ls, case.F, strategy, flags, xb=xb, fprep=prep if blocked else None)
        _check_multiclass(case, strategy, flags, got)                                    # (a)
        for a, b in zip(got, _score_multiclass(cuda, xc, lc, case.F, strategy, flags)):  # (b) the row-major entry
            assert _same(a, b), strategy
    SP.assert_unchanged(xs)


# ================================================ preparation and density ==
PREP_SHAPES = [(n, d) for n in (700, 1300) for d in (30, 64, 200)]
prep_cases = pytest.mark.parametrize("n,d", PREP_SHAPES)
strides = pytest.mark.parametrize("pad,off", [(1, 0), (4, 0), (0, 1)])


class PrepCase:
    """A signed pool, E at the chunk edges, and the fp64 restatements of its
    preparation (computed once, read-only)."""

    def __init__(self, n, d):
        self.n, self.d = n, d
        self.X = O.synthetic_pool(n, d, seed=n + d, dist="normal")
        self.E = np.array([0, 255, 256, n - 1])
        self.mask = O.exclusion_mask(n, self.E)
        X64 = self.X.astype(np.float64)
        n2 = np.zeros(n)
        for f in range(d):
            n2 = n2 + X64[:, f] * X64[:, f]
        self.norm = np.sqrt(n2)                       # test_normalize_bit_exact's restatement
        self.U = O.l2_normalize(self.X)
        assert np.array_equal(self.U, X64 / self.norm[:, None])
        self.u32 = self.U.astype(np.float32)
        self.u32[self.E] = 0
        # O.column_sum_canonical's chunk partials (its inner loop), then its own total
        chunks = (n + 255) // 256
        self.partials = np.zeros((chunks, d))
        for c in range(chunks):
            acc = np.zeros(d)
            for r in range(c * 256, min(n, (c + 1) * 256)):
                if not self.mask[r]:
                    acc = acc + self.U[r]
            self.partials[c] = acc
        self.colsum = O.column_sum_canonical(self.U, self.mask)
        s = np.zeros(d)
        for c in range(chunks):
            s = s + self.partials[c]
        assert np.array_equal(s, self.colsum)
        self.density = O.density_canonical(self.X, self.E)
        for a in (self.X, self.norm, self.U, self.u32, self.partials, self.colsum, self.density):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _prep_case(n, d):
    return PrepCase(n, d)


def _prep_flags(case):
    f = np.zeros(case.n, dtype=np.uint8)
    f[case.E] = EXCL
    return f


def _pads(n, d):
    lib = _lib.load()
    return int(lib.dal_pad_rows(n)), int(lib.dal_pad_features(d))


def _normalize(cuda, x, ldx, flags):
    import torch

    n, d = x.shape
    n_pad, d_pad = _pads(n, d)
    u = _filled(cuda, (n_pad, d_pad), torch.float32, float("nan"))
    norm = _filled(cuda, n, torch.float64, -7.0)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    fl = _dev(cuda, flags)
    _lib.call("dal_normalize_rows", x.data_ptr(), n, d, ldx, fl.data_ptr(), n_pad, d_pad, u.data_ptr(), norm.data_ptr(),
              status.data_ptr(), _stream(cuda))
    assert int(status.item()) == 0
    return _np(u), _np(norm)


@strides
@prep_cases
def test_normalize_rows(cuda, n, d, pad, off):
    case = _prep_case(n, d)
    (xs, ls), (xc, lc) = _layouts(cuda, case.X, d + pad, off)
    u, norm = _normalize(cuda, xs, ls, _prep_flags(case))
    assert np.array_equal(_bits(norm), _bits(case.norm))                                 # (a)
    assert np.array_equal(u[:n, :d].view(np.uint32), case.u32.view(np.uint32))
    assert not u[:, d:].any() and not u[n:].any() and not np.isnan(u).any()  # the zero padding, all written
    for a, b in zip((u, norm), _normalize(cuda, xc, lc, _prep_flags(case))):            # (b)
        assert _same(a, b)
    SP.assert_unchanged(xs)


def _colsum(cuda, x, ldx, case):
    """dal_canon_colsum_partials + _reduce, and _partials_chunks over a copy
    whose listed chunks were poisoned: (partials, colsum, repaired partials)."""
    import torch

    n, d = x.shape
    chunks = (n + 255) // 256
    norm, fl = _dev(cuda, case.norm), _dev(cuda, _prep_flags(case))
    parts = _filled(cuda, (chunks, d), torch.float64, float("nan"))
    _lib.call("dal_canon_colsum_partials", x.data_ptr(), n, d, ldx, norm.data_ptr(), fl.data_ptr(), parts.data_ptr(),
              _stream(cuda))
    s = _filled(cuda, d, torch.float64, float("nan"))
    _lib.call("dal_canon_colsum_reduce", parts.data_ptr(), chunks, d, s.data_ptr(), _stream(cuda))
    ids = np.array([chunks - 1, 0], dtype=np.int64)  # the first chunk and the ragged last one
    redo = parts.clone()
    redo[torch.from_numpy(ids).to(cuda)] = float("nan")
    ids_d = _dev(cuda, ids)
    _lib.call("dal_canon_colsum_partials_chunks", x.data_ptr(), n, d, ldx, norm.data_ptr(), fl.data_ptr(),
              ids_d.data_ptr(), int(ids.size), redo.data_ptr(), _stream(cuda))
    return _np(parts), _np(s), _np(redo)


@strides
@prep_cases
def test_canon_colsum(cuda, n, d, pad, off):
    case = _prep_case(n, d)
    (xs, ls), (xc, lc) = _layouts(cuda, case.X, d + pad, off)
    parts, s, redo = _colsum(cuda, xs, ls, case)
    assert np.array_equal(_bits(s), _bits(case.colsum))                                  # (a) O.column_sum_canonical
    assert np.array_equal(_bits(parts), _bits(case.partials))
    assert np.array_equal(_bits(redo), _bits(case.partials))
    for a, b in zip((parts, s, redo), _colsum(cuda, xc, lc, case)):                      # (b)
        assert _same(a, b)
    SP.assert_unchanged(xs)


def _separable(cuda, x, ldx, case):
    import torch

    n, d = x.shape
    norm, cs, fl = _dev(cuda, case.norm), _dev(cuda, case.colsum), _dev(cuda, _prep_flags(case))
    out = _filled(cuda, n, torch.float64, -7.0)
    _lib.call("dal_density_separable", x.data_ptr(), n, d, ldx, norm.data_ptr(), cs.data_ptr(), fl.data_ptr(),
              out.data_ptr(), _stream(cuda))
    return _np(out)


@strides
@prep_cases
def test_density_separable(cuda, n, d, pad, off):
    case = _prep_case(n, d)
    (xs, ls), (xc, lc) = _layouts(cuda, case.X, d + pad, off)
    got = _separable(cuda, xs, ls, case)
    assert np.array_equal(np.isnan(got), case.mask)                                      # (a) O.density_canonical
    assert np.array_equal(_bits(got[~case.mask]), _bits(case.density[~case.mask]))
    assert _same(got, _separable(cuda, xc, lc, case))                                    # (b)
    SP.assert_unchanged(xs)


def _prep_split(cuda, x, ldx, case, with_partials):
    import torch

    n, d = x.shape
    n_pad, d_pad = _pads(n, d)
    out = _filled(cuda, (n_pad, 2 * d_pad), torch.int16, 0x7E7E)
    norm = _filled(cuda, n, torch.float64, -7.0)
    parts = _filled(cuda, ((n + 255) // 256, d), torch.float64, float("nan"))
    acc = _filled(cuda, n_pad, torch.int64, 1)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    fl = _dev(cuda, _prep_flags(case))
    _lib.call("dal_prep_split", x.data_ptr(), n, d, ldx, fl.data_ptr(), n_pad, d_pad, out.data_ptr(), norm.data_ptr(),
              parts.data_ptr() if with_partials else 0, acc.data_ptr(), status.data_ptr(), _stream(cuda))
    assert int(status.item()) == 0
    return _np(out), _np(norm), _np(parts), _np(acc)


@pytest.mark.parametrize("with_partials", [False, True], ids=["split", "split+partials"])
@strides
@prep_cases
def test_prep_split(cuda, n, d, pad, off, with_partials):
    """The split operand H = fp16(2^12 u), L = fp16(2^12 u - H) in the layout
    [n_pad][d_pad / KS][KS H | KS L] (test_split_operand_bit_exact's
    restatement on the fp64 unit rows), the canonical norms, the fused
    partials and the zeroed accumulator."""
    case = _prep_case(n, d)
    (xs, ls), (xc, lc) = _layouts(cuda, case.X, d + pad, off)
    op, norm, parts, acc = _prep_split(cuda, xs, ls, case, with_partials)
    n_pad, d_pad = _pads(n, d)
    ks = 32 if d_pad == 32 else (128 if d_pad % 128 == 0 else 64)
    u = np.zeros((n_pad, d_pad), dtype=np.float32)
    u[:n, :d] = case.u32
    v = u * np.float32(4096)  # exact
    h = v.astype(np.float16)
    lo = (v - h.astype(np.float32)).astype(np.float16)
    ref = np.empty((n_pad, 2 * d_pad), dtype=np.float16)
    for s0 in range(0, d_pad, ks):
        ref[:, 2 * s0:2 * s0 + ks] = h[:, s0:s0 + ks]
        ref[:, 2 * s0 + ks:2 * s0 + 2 * ks] = lo[:, s0:s0 + ks]
    assert np.array_equal(op.view(np.uint16), ref.view(np.uint16))                       # (a)
    assert np.array_equal(_bits(norm), _bits(case.norm))
    assert not acc.any()
    if with_partials:
        assert np.array_equal(_bits(parts), _bits(case.partials))
    else:
        assert np.isnan(parts).all()  # untouched
    for a, b in zip((op, norm, parts, acc), _prep_split(cuda, xc, lc, case, with_partials)):  # (b)
        assert _same(a, b)
    SP.assert_unchanged(xs)


def _resolve(cuda, x, ldx, case, keys):
    import torch

    n, d = x.shape
    norm, k = _dev(cuda, case.norm), _dev(cuda, keys.view(np.int64))
    out = _filled(cuda, keys.size, torch.float64, -7.0)
    _lib.call("dal_cosine_pairs_resolve", x.data_ptr(), n, d, ldx, norm.data_ptr(), k.data_ptr(), int(keys.size),
              out.data_ptr(), _stream(cuda))
    return _np(out)


@strides
@prep_cases
def test_cosine_pairs_resolve(cuda, n, d, pad, off):
    """300 candidate pairs i < j, the last row's among them."""
    case = _prep_case(n, d)
    rng = np.random.default_rng(n * d)
    i = rng.integers(0, n - 1, 300)
    j = i + 1 + rng.integers(0, n - 1 - i)
    i[:4], j[:4] = (0, n - 2, 255, n - 300), (n - 1, n - 1, n - 1, n - 1)
    assert (i < j).all() and (j < n).all() and (j == n - 1).sum() >= 4
    keys = (i.astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64)
    (xs, ls), (xc, lc) = _layouts(cuda, case.X, d + pad, off)
    got = _resolve(cuda, xs, ls, case, keys)
    assert np.array_equal(_bits(got), _bits(PR.canonical_values(case.U, i, j)))           # (a)
    assert _same(got, _resolve(cuda, xc, lc, case, keys))                                # (b)
    SP.assert_unchanged(xs)


# ================================== selection with the fp64 re-rank (n 20,000) ==
SEL_D, SEL_T, SEL_K = 128, 10, 10
SEL_STRIDES = [(132, 0, "dma", 64), (129, 0, "scalar", 32), (128, 1, "scalar", 32)]
sel_strides = pytest.mark.parametrize("ldx,off,staging,R", SEL_STRIDES, ids=["ldx132", "ldx129", "off1"])
SEL_E = np.arange(10)
MAX_GROUPS = 4096  # csrc/topk.hip kMaxGroups


class SelCase:
    def __init__(self, n):
        self.n = n
        self.X = O.synthetic_pool(n, SEL_D, seed=n % 89)
        self.of = _edge_forest(SEL_D, SEL_T)
        of = self.of
        self.F = Forest.from_nodes(of.feature, of.threshold, of.left, of.right, of.value, of.roots)
        self.unl = np.arange(10, n)
        self.density = O.density_canonical(self.X, SEL_E)
        self.votes = O.votes(of, self.X)
        for a in (self.X, self.density, self.votes):
            a.setflags(write=False)

    @functools.lru_cache(maxsize=None)
    def select(self, beta):
        """O.density_select: (selected indices, their canonical scores)."""
        _, idx, sc = O.density_select(self.X, self.unl, self.of, SEL_K, beta, SEL_E, density=self.density)
        assert np.unique(sc).size == SEL_K and (sc > 0).all()  # a strict top k: no tie decides
        return idx, sc


@functools.lru_cache(maxsize=None)
def _sel_case(n):
    return SelCase(n)


_SEL_STATE = {}


def _sel_inputs(cuda, case):
    """The step's inputs that carry no ldx, from a contiguous PoolState of the
    logical matrix: flags, Gram density and its bound, norm64, colsum."""
    if case.n not in _SEL_STATE:
        from dal import engine

        st = engine.PoolState(np.array(case.X), excluded=SEL_E, device=cuda)  # (a copy: the pool is read-only)
        flags, _, _ = st.row_flags(case.unl)
        _SEL_STATE[case.n] = dict(flags=flags, dens=st.density_fixed(), derr=float(engine.density_error(st)),
                                  norm=st.norms(), colsum=st.colsum(), state=st)
    return _SEL_STATE[case.n]


def _sel_cap(n):
    from dal import engine

    return engine.candidate_cap(n, SEL_K)


def _groups(n, R):
    """csrc/topk.hip make_groups: (groups, rows per group) of R-row blocks."""
    units = -(-n // R)
    per = -(-units // MAX_GROUPS)
    return -(-units // per), per * R


def _select_pair(cuda, case, x, ldx, beta, passes):
    """dal_forest_score (density mode) then dal_dw_select, both on x."""
    import torch

    I, n, F = _sel_inputs(cuda, case), case.n, case.F
    inner, leaf = F.device(cuda)
    lut = _dev(cuda, O.lut("entropy", SEL_T))
    votes = _filled(cuda, n, torch.int32, -7)
    scores = _filled(cuda, n, torch.float64, -7.0)
    klo, khi = _filled(cuda, n, torch.int64, 0x5555), _filled(cuda, n, torch.int64, 0x5555)
    _lib.call("dal_forest_score", x.data_ptr(), n, SEL_D, ldx, inner.data_ptr(), leaf.data_ptr(), SEL_T, DEPTH,
              lut.data_ptr(), I["dens"].data_ptr(), _lib.DAL_DENSITY_FIXED, I["derr"], I["flags"].data_ptr(), beta,
              _lib.DAL_DESCENDING, votes.data_ptr(), scores.data_ptr(), klo.data_ptr(), khi.data_ptr(), _stream(cuda))
    cap = _sel_cap(n)
    wsb = int(_lib.load().dal_dw_select_workspace_bytes(n, SEL_K, cap))
    ws, wsp = _workspace(cuda, wsb)
    out_idx = _filled(cuda, SEL_K, torch.int64, -7)
    out_sc = _filled(cuda, SEL_K, torch.float64, -7.0)
    out_keys = _filled(cuda, SEL_K, torch.int64, 0x5555)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    _lib.call("dal_dw_select", klo.data_ptr(), khi.data_ptr(), votes.data_ptr(), I["flags"].data_ptr(), n, SEL_K, 0,
              lut.data_ptr(), beta, x.data_ptr(), SEL_D, ldx, I["norm"].data_ptr(), I["colsum"].data_ptr(), cap, passes,
              wsp, wsb, out_idx.data_ptr(), out_sc.data_ptr(), out_keys.data_ptr(), status.data_ptr(), 0,
              _stream(cuda))
    assert int(status.item()) == 0
    del ws
    return _np(votes), _np(out_idx), _np(out_sc), _u64(out_keys)


def _dw_step(cuda, case, x, ldx, beta, passes):
    import torch

    I, n, F = _sel_inputs(cuda, case), case.n, case.F
    inner, leaf = F.device(cuda)
    lut = _dev(cuda, O.lut("entropy", SEL_T))
    votes = _filled(cuda, n, torch.int32, -7)
    scores = _filled(cuda, n, torch.float64, -7.0)
    klo, khi = _filled(cuda, n, torch.int64, 0x5555), _filled(cuda, n, torch.int64, 0x5555)
    cap = _sel_cap(n)
    wsb = int(_lib.load().dal_dw_step_workspace_bytes(n, SEL_K, cap))
    ws, wsp = _workspace(cuda, wsb)
    out_idx = _filled(cuda, SEL_K, torch.int64, -7)
    out_sc = _filled(cuda, SEL_K, torch.float64, -7.0)
    out_keys = _filled(cuda, SEL_K, torch.int64, 0x5555)
    status = _filled(cuda, 1, torch.int32, 0x7F)  # DAL_STEP_RESET_STATUS zeroes it on the device
    _lib.call("dal_dw_step", x.data_ptr(), 0, 0, n, SEL_D, ldx, inner.data_ptr(), leaf.data_ptr(), SEL_T, DEPTH,
              lut.data_ptr(), I["dens"].data_ptr(), I["derr"], I["flags"].data_ptr(), beta, 0, I["norm"].data_ptr(),
              I["colsum"].data_ptr(), SEL_K, cap, passes, _lib.DAL_STEP_RESET_STATUS, wsp, wsb, votes.data_ptr(),
              scores.data_ptr(), klo.data_ptr(), khi.data_ptr(), out_idx.data_ptr(), out_sc.data_ptr(),
              out_keys.data_ptr(), status.data_ptr(), 0, _stream(cuda))
    assert int(status.item()) == 0
    del ws
    return _np(votes), _np(out_idx), _np(out_sc), _u64(out_keys)


def _check_selection(case, beta, got):
    votes, idx, sc, keys = got
    ref_idx, ref_sc = case.select(beta)
    assert np.array_equal(votes, case.votes)
    assert np.array_equal(idx, ref_idx)
    assert np.array_equal(_bits(sc), _bits(ref_sc))
    assert np.array_equal(keys, score_key(ref_sc, True))


@pytest.mark.parametrize("beta", [1.0, 2.0])
@pytest.mark.parametrize("passes", [0, 1], ids=["exact-l1", "fast-l1"])
@sel_strides
def test_dw_select(cuda, ldx, off, staging, R, passes, beta):
    case = _sel_case(20_000)
    (xs, ls), (xc, lc) = _layouts(cuda, case.X, ldx, off)
    _tiling = SP.forest_tiling(SEL_D, ldx, xs.data_ptr(), SEL_T)
    assert (_tiling.staging, _tiling.R) == (staging, R)
    got = _select_pair(cuda, case, xs, ls, beta, passes)
    _check_selection(case, beta, got)                                                    # (a) O.density_select
    for a, b in zip(got, _select_pair(cuda, case, xc, lc, beta, passes)):                # (b)
        assert _same(a, b)
    SP.assert_unchanged(xs)


@pytest.mark.parametrize("beta", [1.0, 2.0])
@pytest.mark.parametrize("passes", [0, 1], ids=["exact-l1", "fast-l1-folded"])
@sel_strides
def test_dw_step(cuda, ldx, off, staging, R, passes, beta):
    """The fused step: level1_passes = 0 is the exact form; with the fast
    level 1 the score kernel's blocks are the row groups (>= 2k of them), so
    the pool's alignment decides the groups: 64 rows with LDS-DMA staging, 32
    with scalar staging."""
    case = _sel_case(20_000)
    (xs, ls), (xc, lc) = _layouts(cuda, case.X, ldx, off)
    t = SP.forest_tiling(SEL_D, ldx, xs.data_ptr(), SEL_T)
    assert (t.staging, t.R) == (staging, R)
    ng, group_rows = _groups(case.n, R)
    assert ng >= 2 * SEL_K and group_rows == R  # folded by the score kernel with plain stores
    got = _dw_step(cuda, case, xs, ls, beta, passes)
    _check_selection(case, beta, got)                                                    # (a)
    for a, b in zip(got, _select_pair(cuda, case, xs, ls, beta, passes)):                # the two separate calls
        assert _same(a, b)
    for a, b in zip(got, _dw_step(cuda, case, xc, lc, beta, passes)):                    # (b)
        assert _same(a, b)
    SP.assert_unchanged(xs)


@sel_strides
def test_dw_step_prefetch_rows(cuda, ldx, off, staging, R):
    """prefetch_row (csrc/topk.hip) issues its loads from x + i * ldx for each
    group's hinted row before the re-rank: a smaller pool (n = 5,003, a
    ragged last group) where ng >= 2k holds for R = 64 and R = 32, so the
    hints come from the score kernel's fold in every layout, and the last
    rows are candidates."""
    case = _sel_case(5_003)
    for rows in (64, 32):
        assert _groups(case.n, rows)[0] >= 2 * SEL_K and _groups(case.n, rows)[1] == rows
    (xs, ls), (xc, lc) = _layouts(cuda, case.X, ldx, off)
    t = SP.forest_tiling(SEL_D, ldx, xs.data_ptr(), SEL_T)
    assert (t.staging, t.R) == (staging, R)
    got = _dw_step(cuda, case, xs, ls, 1.0, 1)
    _check_selection(case, 1.0, got)                                                     # (a)
    for a, b in zip(got, _select_pair(cuda, case, xs, ls, 1.0, 1)):
        assert _same(a, b)
    for a, b in zip(got, _dw_step(cuda, case, xc, lc, 1.0, 1)):                          # (b)
        assert _same(a, b)
    SP.assert_unchanged(xs)


def _dw_step_multiclass(cuda, case, F, x, ldx, passes):
    import torch

    from dal import luts

    I, n, C = _sel_inputs(cuda, case), case.n, int(F.n_classes)
    inner, leaf = F.device(cuda)
    lut = _dev(cuda, luts.multiclass_lut("entropy", F.n_trees))
    o = _mc_outputs(cuda, n, C)
    entropy, row_index = _filled(cuda, n, torch.float64, -7.0), _filled(cuda, n, torch.int32, -7)
    klo, khi = _filled(cuda, n, torch.int64, 0x5555), _filled(cuda, n, torch.int64, 0x5555)
    cap = _sel_cap(n)
    wsb = int(_lib.load().dal_dw_step_workspace_bytes(n, SEL_K, cap))
    ws, wsp = _workspace(cuda, wsb)
    out_idx = _filled(cuda, SEL_K, torch.int64, -7)
    out_sc = _filled(cuda, SEL_K, torch.float64, -7.0)
    status = _filled(cuda, 1, torch.int32, 0x7F)
    _lib.call("dal_dw_step_multiclass", x.data_ptr(), 0, 0, n, SEL_D, ldx, inner.data_ptr(), leaf.data_ptr(),
              F.n_trees, F.depth, C, lut.data_ptr(), I["dens"].data_ptr(), I["derr"], I["flags"].data_ptr(), 1.0, 0,
              I["norm"].data_ptr(), I["colsum"].data_ptr(), SEL_K, cap, passes, _lib.DAL_STEP_RESET_STATUS, wsp, wsb,
              o["counts"].data_ptr(), o["pred"].data_ptr(), entropy.data_ptr(), row_index.data_ptr(),
              o["scores"].data_ptr(), klo.data_ptr(), khi.data_ptr(), out_idx.data_ptr(), out_sc.data_ptr(), 0,
              status.data_ptr(), 0, _stream(cuda))
    assert int(status.item()) == 0
    del ws
    return _np(o["counts"]), _np(o["pred"]), _np(entropy), _np(out_idx), _np(out_sc)


@pytest.mark.parametrize("passes", [0, 1])
def test_dw_step_multiclass(cuda, passes):
    """One strided case (ldx = 129: scalar staging, R = 32) against
    multiclass_dw_reference.select."""
    case = _sel_case(5_003)
    F = _edge_multiclass_forest(SEL_T, SEL_D, 3)
    _, ref_idx, ref_sc, _ = DW.select(case.X, case.unl, F, SEL_K, excluded=SEL_E, density=case.density)
    assert np.unique(ref_sc).size == SEL_K and (ref_sc > 0).all()
    cnt = MR.counts(F, case.X)
    (xs, ls), (xc, lc) = _layouts(cuda, case.X, 129, 0)
    assert SP.forest_tiling(SEL_D, 129, xs.data_ptr(), SEL_T)[:2] == ("scalar", 32)
    got = _dw_step_multiclass(cuda, case, F, xs, ls, passes)
    c, p, h, idx, sc = got
    assert np.array_equal(c, cnt) and np.array_equal(p, MR.pred(cnt))                    # (a)
    assert np.array_equal(_bits(h), _bits(DW.entropy(cnt, SEL_T)))
    assert np.array_equal(idx, ref_idx) and np.array_equal(_bits(sc), _bits(ref_sc))
    for a, b in zip(got, _dw_step_multiclass(cuda, case, F, xc, lc, passes)):            # (b)
        assert _same(a, b)
    SP.assert_unchanged(xs)


# ================================================================ training ==
# The smallest shapes of the trainers' own GPU tests, rows of stride d + 3.
def _find_splits(cuda, x, ldx, ns, f64):
    """dal_rf_find_splits (fp32 thresholds) or dal_rf_find_splits_f64."""
    import torch

    n, d = x.shape
    thr = _filled(cuda, (d, _lib.DAL_RF_MAX_SPLITS), torch.float64 if f64 else torch.float32, float("nan"))
    cnt = _filled(cuda, d, torch.int32, -7)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    if f64:
        x_dtype = _lib.DAL_X_F64 if x.dtype == torch.float64 else _lib.DAL_X_F32
        _lib.call("dal_rf_find_splits_f64", x.data_ptr(), x_dtype, n, d, ldx, 0, n, ns, thr.data_ptr(), cnt.data_ptr(),
                  status.data_ptr(), _stream(cuda))
    else:
        _lib.call("dal_rf_find_splits", x.data_ptr(), n, d, ldx, 0, n, ns, thr.data_ptr(), cnt.data_ptr(),
                  status.data_ptr(), _stream(cuda))
    assert int(status.item()) == 0
    return thr, cnt


def _check_thresholds(thr, cnt, X, ns, f64):
    from oracle import rf_oracle

    t, c = _np(thr), _np(cnt)
    for f in range(X.shape[1]):
        ref = rf_oracle.find_splits(X[:, f], ns)
        assert c[f] == ref.size, f
        assert _same(t[f, :ref.size], ref if f64 else ref.astype(np.float32)), f


@pytest.mark.parametrize("f64_rows", [False, True], ids=["f32rows", "f64rows"])
def test_rf_find_splits_and_bins(cuda, f64_rows):
    """dal_rf_find_splits, dal_rf_find_splits_f64 and dal_rf_bin_rows over
    strided rows (fp32, and fp64 values no fp32 holds): the thresholds of
    oracle.rf_oracle.find_splits and the bins of bin_values, as
    tests/test_gpu_rf_regress.py's fit checks them."""
    import torch

    from dal.random_forest import num_splits
    from oracle import rf_oracle

    n, d = 48, 3  # test_gpu_rf_regress "tiny": fewer rows than bins
    rng = np.random.default_rng(304)
    X = rng.random((n, d)) if f64_rows else rng.random((n, d), dtype=np.float32)
    if f64_rows:
        assert not np.array_equal(X, X.astype(np.float32).astype(np.float64))
    X[5:9, 1] = X[4, 1]  # repeated values: a threshold with a count
    ns = num_splits(n)
    outs = []
    for x, ldx in _layouts(cuda, X, d + 3, 0):
        thr, cnt = _find_splits(cuda, x, ldx, ns, True)
        _check_thresholds(thr, cnt, X, ns, True)                                         # (a)
        res = [_np(thr), _np(cnt)]
        if not f64_rows:
            thr32, cnt32 = _find_splits(cuda, x, ldx, ns, False)
            _check_thresholds(thr32, cnt32, X, ns, False)
            res += [_np(thr32), _np(cnt32)]
        bins = _filled(cuda, (n, d), torch.uint8, 0xEE)
        _lib.call("dal_rf_bin_rows", x.data_ptr(), _lib.DAL_X_F64 if f64_rows else _lib.DAL_X_F32, n, d, ldx,
                  thr.data_ptr(), cnt.data_ptr(), bins.data_ptr(), _stream(cuda))
        ref_bins = np.stack([rf_oracle.bin_values(X[:, f], rf_oracle.find_splits(X[:, f], ns)) for f in range(d)],
                            axis=1)
        assert np.array_equal(_np(bins), ref_bins.astype(np.uint8))                      # (a)
        res.append(_np(bins))
        outs.append(res)
        if hasattr(x, "pool_buffer"):
            SP.assert_unchanged(x)
    for a, b in zip(*outs):                                                              # (b)
        assert _same(a, b)


def _raw_train(cuda, x, ldx, y, w, s, depth, n_classes, steps):
    """dal_rf_find_splits + dal_rf_train (n_classes None) or
    dal_rf_train_multiclass over x -- in one call, or (``steps``) as the
    header spells it out: *_begin, then *_level_stats and *_level_split for
    l = 0..max_depth, then *_finish.  (inner, leaf) bytes."""
    import torch

    from dal.random_forest import num_splits

    lib = _lib.load()
    n, d = x.shape
    T, n_inner, m = w.shape[0], (1 << depth) - 1, s.shape[2]
    ns = num_splits(n)
    lab, wt, sub = _dev(cuda, y, np.uint8), _dev(cuda, w, np.int32), _dev(cuda, s, np.int32)
    thr, cnt = _find_splits(cuda, x, ldx, ns, False)
    wsb = int(lib.dal_rf_train_workspace_bytes(n, d, T, depth, m, ns) if n_classes is None else
              lib.dal_rf_train_multiclass_workspace_bytes(n, d, T, depth, m, ns, n_classes))
    assert wsb > 0
    ws, wsp = _workspace(cuda, wsb)
    inner = _filled(cuda, (T, n_inner, 2), torch.int32, -7)
    leaf = _filled(cuda, (T, n_inner + 1), torch.uint8, 99)
    st = _stream(cuda)
    head = (x.data_ptr(), n, d, ldx, lab.data_ptr(), thr.data_ptr(), cnt.data_ptr(), ns, wt.data_ptr(),
            sub.data_ptr(), m, T, depth, 1, 0.0)
    classes = () if n_classes is None else (n_classes,)
    tail = (inner.data_ptr(), leaf.data_ptr(), wsp, wsb, st)
    name = "dal_rf_train" if n_classes is None else "dal_rf_train_multiclass"
    if not steps:
        _lib.call(name, *head, *classes, *tail)
    else:
        job = ctypes.create_string_buffer(_lib.DAL_RF_JOB_BYTES)
        _lib.call(name + "_begin", job, *head, *classes, *tail)
        for level in range(depth + 1):
            _lib.call(name + "_level_stats", job, level, st)
            _lib.call(name + "_level_split", job, level, st)
        _lib.call(name + "_finish", job, st)
    torch.cuda.synchronize(cuda)
    del ws
    return inner.cpu().numpy().tobytes(), leaf.cpu().numpy().tobytes()


@pytest.mark.parametrize("steps", [False, True], ids=["fit", "level-steps"])
def test_rf_train_binary(cuda, steps):
    """dal_rf_train (and dal_rf_train_begin's level steps) over rows of
    stride d + 3: the bytes of the binary CPU restatement
    (oracle/rf_oracle.py), as test_two_classes_equal_the_binary_oracle."""
    from dal.random_forest import bagging_inputs
    from oracle import rf_oracle

    g = load_golden("checkerboard4x4.npz")
    X, y = np.ascontiguousarray(g["X"], dtype=np.float32), g["y"].astype(np.int64)
    w, s = bagging_inputs(X.shape[0], X.shape[1], 10, 4, seed=14)
    _, sf, st, lc = rf_oracle.train_classifier(X, y, w, s, max_depth=4)
    assert ((sf >= 0).sum(axis=1) >= 9).all()  # real trees
    inner = np.zeros(sf.shape + (2,), dtype=np.int32)
    inner[..., 1] = np.array([np.inf], dtype=np.float32).view(np.int32)[0]
    inner[..., 0][sf >= 0] = sf[sf >= 0]
    inner[..., 1][sf >= 0] = st[sf >= 0].astype(np.float32).view(np.int32)
    ref = (inner.tobytes(), lc.astype(np.uint8).tobytes())
    (xs, ls), (xc, lc_) = _layouts(cuda, X, X.shape[1] + 3, 0)
    got = _raw_train(cuda, xs, ls, y, w, s, 4, None, steps)
    assert got == ref                                                                    # (a)
    assert got == _raw_train(cuda, xc, lc_, y, w, s, 4, None, steps)                     # (b)
    SP.assert_unchanged(xs)


@pytest.mark.parametrize("steps", [False, True], ids=["fit", "level-steps"])
def test_rf_train_multiclass(cuda, steps):
    """dal_rf_train_multiclass (and its level steps) at
    tests/test_gpu_rf_multiclass.py's smallest shape, "c5_tiny"."""
    from dal.random_forest import bagging_inputs

    n, d, C, T, depth = 64, 4, 5, 3, 2
    rng = np.random.default_rng(103)
    X = rng.random((n, d), dtype=np.float32)
    y = np.minimum(np.floor(X[:, 0] * C).astype(np.int64) + (X[:, 1] > 0.8), C - 1)
    noisy = rng.random(n) < 0.1
    y[noisy] = rng.integers(0, C, int(noisy.sum()))
    w, s = bagging_inputs(n, d, T, depth, seed=T + depth)
    _, sf, st, lc = M.train_classifier(X, y, w, s, C, max_depth=depth)
    assert ((sf >= 0).sum(axis=1) >= 2).all()
    inner, leaf = M.heap_arrays(sf, st, lc)
    ref = (inner.tobytes(), leaf.tobytes())
    (xs, ls), (xc, lc_) = _layouts(cuda, X, d + 3, 0)
    got = _raw_train(cuda, xs, ls, y, w, s, depth, C, steps)
    assert got == ref                                                                    # (a)
    assert got == _raw_train(cuda, xc, lc_, y, w, s, depth, C, steps)                    # (b)
    SP.assert_unchanged(xs)
