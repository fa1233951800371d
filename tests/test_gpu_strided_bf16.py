"""Strided and unaligned bf16 pools through the C ABI: every entry that takes
an ``ld`` beside a bf16 pool -- the max-cosine helpers and the greedy k-center
selection -- on a view of row stride ld > d whose padding, lead-in and tail
hold the bf16 NaN 0x7FC0 (tests/strided_pool.py).

At ld = d + 4 the rows are alternately 16-byte aligned and 8 bytes off, so
row_sq_norm_bf16 (csrc/common.hpp) takes its 16-byte and its scalar branch
within one call; at ld = d + 8 every row is aligned; with the first row 8 or 2
bytes into the allocation none is.  Each case asserts, bit for bit, (a) the
plain fp64 reference of the logical matrix (O.max_cosine_canonical,
O.diversity_select_canonical, kcenter_reference on O.bf16_round(X), as
tests/test_gpu_maxcos.py and tests/test_gpu_kcenter.py do) and (b) the same
entry on the contiguous copy with ld = d; and that the input buffer is
byte-identical afterwards."""
import ctypes
import functools

import numpy as np
import pytest

import kcenter_reference as KC
import strided_pool as SP
from dal import _lib
from oracle import dal_oracle as O

pytestmark = pytest.mark.gpu

N, M, K = 700, 40, 10
# (ld - d, offset_elems): alternating rows; all rows aligned; no row aligned (8 bytes off, 2 bytes off)
STRIDES = [(4, 0), (8, 0), (8, 4), (4, 1)]
strides = pytest.mark.parametrize("pad,off", STRIDES)
widths = pytest.mark.parametrize("d", [64, 128])


def _stream(cuda):
    import torch

    return torch.cuda.current_stream(cuda).cuda_stream


def _dev(cuda, a, dtype=None):
    import torch

    return torch.from_numpy(np.array(a, dtype=dtype)).to(cuda)  # (a copy: the cases are read-only)


def _filled(cuda, shape, dtype, value):
    import torch

    return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=dtype, device=cuda)


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Case:
    """A bf16 pool (fp32 values, bf16-representable), its labeled rows 0..M-1
    and the canonical quantities, computed once and read-only."""

    def __init__(self, d, clustered=False):
        self.d = d
        X = KC.clustered_pool(N, d, 7, seed=d) if clustered else O.bf16_round(O.synthetic_pool(N, d, seed=3 * d,
                                                                                                dist="normal"))
        X[500:503] = X[600]  # duplicate rows: exact ties, resolved by index
        self.X, self.bits = X, KC.bf16_bits(X)
        assert np.array_equal((self.bits.astype(np.uint32) << 16).view(np.float32), X)
        self.L = np.arange(M)
        self.cand = np.arange(M, N)
        X64 = X.astype(np.float64)
        n2 = np.zeros(N)
        for f in range(d):
            n2 = n2 + X64[:, f] * X64[:, f]
        self.norm = np.sqrt(n2)
        self.U = O.l2_normalize(X)
        assert np.array_equal(self.U, X64 / self.norm[:, None])
        self.ulab_t = np.ascontiguousarray(self.U[self.L].T)  # canonical unit labeled rows, feature-major [d][M]
        self.m, self.arg = O.max_cosine_canonical(X, self.L)
        for a in (self.X, self.bits, self.norm, self.U, self.ulab_t, self.m, self.arg):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _case(d, clustered=False):
    return Case(d, clustered)


def _layouts(cuda, case, pad, off):
    return (SP.strided(case.bits, case.d + pad, off, cuda), case.d + pad), (SP.contiguous(case.bits, cuda), case.d)


def _assert_alignment_mix(view, pad, off):
    """The branches of row_sq_norm_bf16 the layout reaches: which rows start
    on a 16-byte boundary."""
    ld = view.ldx
    aligned = {(view.data_ptr() + 2 * i * ld) % 16 == 0 for i in range(N)}
    assert aligned == {(4, 0): {True, False}, (8, 0): {True}, (8, 4): {False}, (4, 1): {False}}[(pad, off)]


# --------------------------------------------------------------- helpers --
def _inv_norms(cuda, x, ld, d):
    import torch

    n_pad = N + 68
    inv = _filled(cuda, n_pad, torch.float32, -7.0)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    _lib.call("dal_inv_norms_bf16", x.data_ptr(), N, n_pad, d, ld, inv.data_ptr(), status.data_ptr(), _stream(cuda))
    assert int(status.item()) == 0
    return _np(inv)


@strides
@widths
def test_inv_norms_bf16(cuda, d, pad, off):
    """inv[i] = fp32(1 / sqrt(sum_f x_if^2)), the sum sequential in fp64;
    rows n .. n_pad - 1 are NaN."""
    case = _case(d)
    (xs, ls), (xc, lc) = _layouts(cuda, case, pad, off)
    _assert_alignment_mix(xs, pad, off)
    got = _inv_norms(cuda, xs, ls, d)
    assert np.array_equal(got[:N].view(np.uint32), (1.0 / case.norm).astype(np.float32).view(np.uint32))  # (a)
    assert np.isnan(got[N:]).all()
    assert _same(got, _inv_norms(cuda, xc, lc, d))                                       # (b)
    SP.assert_unchanged(xs)


def _canon_unit_rows(cuda, x, ld, d, feature_major):
    import torch

    u = _filled(cuda, N * d, torch.float64, -7.0)
    _lib.call("dal_canon_unit_rows_bf16", x.data_ptr(), N, d, ld, feature_major, u.data_ptr(), _stream(cuda))
    return _np(u)


@pytest.mark.parametrize("feature_major", [0, 1])
@strides
@widths
def test_canon_unit_rows_bf16(cuda, d, pad, off, feature_major):
    case = _case(d)
    (xs, ls), (xc, lc) = _layouts(cuda, case, pad, off)
    got = _canon_unit_rows(cuda, xs, ls, d, feature_major)
    ref = case.U.T if feature_major else case.U
    assert np.array_equal(_bits(got), _bits(np.ascontiguousarray(ref).reshape(-1)))      # (a) O.l2_normalize
    assert _same(got, _canon_unit_rows(cuda, xc, lc, d, feature_major))                  # (b)
    SP.assert_unchanged(xs)


def _unit_rows_f16(cuda, x, ld, d, m, m_pad):
    import torch

    out = _filled(cuda, (m_pad, d), torch.int16, 0x7E7E)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    _lib.call("dal_unit_rows_f16", x.data_ptr(), m, m_pad, d, ld, out.data_ptr(), status.data_ptr(), _stream(cuda))
    assert int(status.item()) == 0
    return _np(out).view(np.float16)


@strides
@widths
def test_unit_rows_f16(cuda, d, pad, off):
    """The folded labeled operand of the first M rows: fp16(2^15 x / ||x||),
    one rounding from fp64; the padding rows repeat row 0."""
    case = _case(d)
    m_pad = int(_lib.load().dal_maxcos_label_rows_granule(d))
    assert m_pad >= M
    (xs, ls), (xc, lc) = _layouts(cuda, case, pad, off)
    got = _unit_rows_f16(cuda, xs, ls, d, M, m_pad)
    ref = np.empty((m_pad, d), dtype=np.float16)
    ref[:M] = (case.U[:M] * 32768.0).astype(np.float16)
    ref[M:] = ref[0]
    assert np.array_equal(got.view(np.uint16), ref.view(np.uint16))                      # (a)
    assert _same(got, _unit_rows_f16(cuda, xc, lc, d, M, m_pad))                         # (b)
    SP.assert_unchanged(xs)


def _argmax_resolve(cuda, x, ld, case, arg_in):
    arg = _dev(cuda, arg_in)
    ulab = _dev(cuda, case.ulab_t)
    _lib.call("dal_maxcos_argmax_resolve", x.data_ptr(), N, case.d, ld, ulab.data_ptr(), M, arg.data_ptr(),
              _stream(cuda))
    return _np(arg)


@strides
@widths
def test_maxcos_argmax_resolve(cuda, d, pad, off):
    """Every entry < 0 becomes the canonical fp64 arg-max (first l on ties);
    every other entry is left alone."""
    case = _case(d)
    arg_in = (-1 - np.arange(N) % M).astype(np.int32)  # "ambiguous", with some l
    keep = np.arange(N) % 3 == 1
    arg_in[keep] = 12345
    assert (~keep)[[N - 1, 501, 600]].all()
    (xs, ls), (xc, lc) = _layouts(cuda, case, pad, off)
    got = _argmax_resolve(cuda, xs, ls, case, arg_in)
    assert np.array_equal(got, np.where(keep, 12345, case.arg).astype(np.int32))          # (a) O.max_cosine_canonical
    assert _same(got, _argmax_resolve(cuda, xc, lc, case, arg_in))                       # (b)
    SP.assert_unchanged(xs)


def _maxcos_select(cuda, x, ld, case, passes):
    """dal_maxcos_select over interval keys of fp32 max-cosines within the
    folded kernel's bound of the canonical values (here their fp32 rounding:
    the keys are a function of the logical matrix, not of the layout)."""
    import torch

    from dal.engine import candidate_cap

    lib, d = _lib.load(), case.d
    flags = np.zeros(N, dtype=np.uint8)
    flags[case.cand] = _lib.DAL_ROW_CANDIDATE
    mx, fl = _dev(cuda, case.m.astype(np.float32)), _dev(cuda, flags)
    lo, hi = _filled(cuda, N, torch.int64, 0x5555), _filled(cuda, N, torch.int64, 0x5555)
    _lib.call("dal_interval_keys_f32", mx.data_ptr(), N, float(lib.dal_maxcos_unit_error_bound(d)), fl.data_ptr(),
              _lib.DAL_ASCENDING, lo.data_ptr(), hi.data_ptr(), _stream(cuda))
    cap = candidate_cap(N, K)
    wsb = int(lib.dal_maxcos_select_workspace_bytes(N, K, cap))
    ws = torch.zeros(wsb + 256, dtype=torch.uint8, device=cuda)
    wsp = (ws.data_ptr() + 255) // 256 * 256
    ulab = _dev(cuda, case.ulab_t)
    out_idx = _filled(cuda, K, torch.int64, -7)
    out_sc = _filled(cuda, K, torch.float64, -7.0)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    _lib.call("dal_maxcos_select", lo.data_ptr(), hi.data_ptr(), N, K, 0, x.data_ptr(), d, ld, ulab.data_ptr(), M, cap,
              passes, wsp, wsb, out_idx.data_ptr(), out_sc.data_ptr(), 0, status.data_ptr(), _stream(cuda))
    assert int(status.item()) == 0
    del ws
    return _np(out_idx), _np(out_sc)


@pytest.mark.parametrize("passes", [0, 1], ids=["exact-l1", "fast-l1"])
@strides
@widths
def test_maxcos_select(cuda, d, pad, off, passes):
    case = _case(d)
    ref_idx, ref_sc = O.diversity_select_canonical(case.X, case.L, K, candidates=case.cand)
    (xs, ls), (xc, lc) = _layouts(cuda, case, pad, off)
    idx, sc = _maxcos_select(cuda, xs, ls, case, passes)
    assert np.array_equal(idx, ref_idx) and np.array_equal(_bits(sc), _bits(ref_sc))     # (a)
    for a, b in zip((idx, sc), _maxcos_select(cuda, xc, lc, case, passes)):              # (b)
        assert _same(a, b)
    SP.assert_unchanged(xs)


# --------------------------------------------------------------- k-center --
def _kcenter_select(cuda, x, ld, case, k):
    """dal_kcenter_select with the caller's state built from the logical
    matrix: m32 = the fp32 rounding of the canonical m_i(0) (within
    dal_kcenter_error_bound), inv_norm, the labeled rows' canonical unit
    rows in the first M columns of the centers table."""
    import torch

    lib, d = _lib.load(), case.d
    assert float(lib.dal_kcenter_error_bound(d)) > 2.0 ** -24
    flags = np.zeros(N, dtype=np.uint8)
    flags[case.cand] = _lib.DAL_ROW_CANDIDATE
    fl, m32 = _dev(cuda, flags), _dev(cuda, case.m.astype(np.float32))
    inv = _dev(cuda, (1.0 / case.norm).astype(np.float32))
    centers = np.full((d, M + k), np.nan)
    centers[:, :M] = case.ulab_t
    cen = _dev(cuda, centers)
    wsb = int(lib.dal_kcenter_workspace_bytes(N, d, M, k))
    ws = torch.zeros(wsb + 256, dtype=torch.uint8, device=cuda)
    wsp = (ws.data_ptr() + 255) // 256 * 256
    job = ctypes.create_string_buffer(_lib.DAL_KCENTER_JOB_BYTES)
    out_idx = _filled(cuda, k, torch.int64, -7)
    out_sc = _filled(cuda, k, torch.float64, -7.0)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    assert x.data_ptr() % 16 == 0 and ld % 8 == 0 and m32.data_ptr() % 16 == 0 and inv.data_ptr() % 16 == 0
    _lib.call("dal_kcenter_select", job, x.data_ptr(), N, d, ld, 0, fl.data_ptr(), m32.data_ptr(), inv.data_ptr(),
              cen.data_ptr(), M, k, wsp, wsb, out_idx.data_ptr(), out_sc.data_ptr(), status.data_ptr(), _stream(cuda))
    assert int(status.item()) == 0
    del ws
    return _np(out_idx), _np(out_sc), _np(fl), _np(cen)[:, M:]


@pytest.mark.parametrize("clustered", [False, True], ids=["normal", "clustered"])
@widths
def test_kcenter_select(cuda, d, clustered):
    """ld = d + 8 on a 16-byte aligned pool (the entry requires both): the
    picks, the pick-time values, the picks' flags and their appended unit
    rows."""
    k = 5
    case = _case(d, clustered)
    picks, values, _ = KC.kcenter_reference(case.X, case.L, k, candidates=case.cand)
    assert picks.size == k and np.unique(picks).size == k
    (xs, ls), (xc, lc) = _layouts(cuda, case, 8, 0)
    got = _kcenter_select(cuda, xs, ls, case, k)
    idx, sc, fl, cols = got
    assert np.array_equal(idx, picks) and np.array_equal(_bits(sc), _bits(values))       # (a) kcenter_reference
    picked = (fl & _lib.DAL_ROW_PICKED) != 0
    assert np.array_equal(np.flatnonzero(picked), np.sort(picks))
    assert np.array_equal(_bits(cols), _bits(case.U[picks].T))
    for a, b in zip(got, _kcenter_select(cuda, xc, lc, case, k)):                        # (b)
        assert _same(a, b)
    SP.assert_unchanged(xs)
