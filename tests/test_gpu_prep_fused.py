"""The fp4 form's one-pass preparation (dal_prep_split_fp4, csrc/prep_fp4.hip)
writes the bytes of the separate entries:

 1. per shape, against dal_prep_split + dal_quant_fp4 + dal_gram_sym_residual_fp4:
    norm64, the status word, the zeroed accumulator, the split operand, the
    canonical column-sum partials, the e2m1 codes, sigma^H' (read from the
    residual's workspace) and S^L' (S~ minus the sigma^H' total: both exact
    integers below 2^53 here); and dal_gram_sym_residual_fp4_pre fed with the
    fused sums leaves the same S~, D_B and accumulator as the three-launch
    entry.  Shapes: a partial last chunk with a half-empty last super block and
    rows of E in the first and last chunk; one row in the second super block;
    zero-padded features on a strided pool; two 256-feature slices; an
    all-zero row; a row that clamps a4 at 12; U[0,1) and N(0,1) data.
 2. end to end on 36,000 x 256 (the smallest kind of pool that takes the fp4
    form by the default rule): PoolState(prep_fused=True) and (prep_fused=False)
    give the same int64 density and the same density_step selection, before and
    after exclude().
Needs an MI355X: ``pytest -m gpu``."""
import numpy as np
import pytest

from oracle import dal_oracle as O

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _case(name):
    """(x [n, ldx] fp32, d, excluded rows) of a named shape."""
    if name == "partial_last_chunk":  # n_pad 1,024: the last chunk partial, the last super block half empty
        return O.synthetic_pool(1000, 256, seed=11), 256, list(range(10)) + [999]
    if name == "one_row_second_super_block":
        return O.synthetic_pool(513, 256, seed=12, dist="normal"), 256, []
    if name == "strided_padded_features":  # d_pad 256 > d, ldx 208 > d
        x = O.synthetic_pool(700, 208, seed=13, dist="normal")
        return x, 200, [3, 699]
    if name == "two_slices":  # d_pad 512
        return O.synthetic_pool(600, 300, seed=14), 300, [0, 255, 256, 599]
    if name == "zero_row":
        x = O.synthetic_pool(777, 256, seed=15, dist="normal")
        x[300] = 0.0
        return x, 256, [5]
    if name == "clamped":  # one dominant feature: H = +-4096, a4 clamps at +-12
        x = O.synthetic_pool(520, 256, seed=16, dist="normal")
        x[7] *= np.float32(1e-3)
        x[7, 5] = -1.0
        x[515] *= np.float32(1e-3)
        x[515, 255] = 1.0
        return x, 256, []
    raise ValueError(name)


CASES = ["partial_last_chunk", "one_row_second_super_block", "strided_padded_features", "two_slices", "zero_row",
         "clamped"]


def _run_both(cuda, x_np, d, excluded):
    import torch

    from dal import _lib
    from dal.engine import workspace

    lib = _lib.load()
    n, ldx = x_np.shape
    x = torch.from_numpy(np.ascontiguousarray(x_np)).to(cuda)
    n_pad, d_pad = int(lib.dal_pad_rows(n)), int(lib.dal_pad_features(d))
    assert d_pad % 256 == 0 and n_pad % 512 == 0
    flags = torch.zeros(n, dtype=torch.uint8, device=cuda)
    if excluded:
        flags[torch.tensor(excluded, device=cuda)] = _lib.DAL_ROW_EXCLUDED
    chunks = (n + 255) // 256
    nb = n_pad // 256
    stream = torch.cuda.current_stream(cuda).cuda_stream
    res_bytes = int(lib.dal_gram_sym_residual_workspace_bytes(nb, nb, d_pad))
    sig_words = n_pad // 512 * d_pad

    def buffers():
        # filled with a pattern: every word the entries own must be written
        return dict(ops=torch.full((n_pad, 2 * d_pad), 0x5A5A, dtype=torch.int16, device=cuda),
                    norm=torch.full((n,), -7.0, dtype=torch.float64, device=cuda),
                    parts=torch.full((chunks, d), -7.0, dtype=torch.float64, device=cuda),
                    acc0=torch.full((n_pad,), 12345, dtype=torch.int64, device=cuda),
                    codes=torch.full((n_pad, d_pad // 2), 0xEE, dtype=torch.uint8, device=cuda),
                    status=torch.zeros(1, dtype=torch.int32, device=cuda),
                    acc=torch.zeros(n_pad, dtype=torch.int64, device=cuda))

    def residual_words(ws, wsp):
        w = _np(ws)[wsp - ws.data_ptr():][:res_bytes].view(np.int64)
        return w[:sig_words].copy(), w[sig_words:sig_words + d_pad].copy(), w[2 * sig_words:3 * sig_words].copy()

    a = buffers()
    _lib.call("dal_prep_split", x.data_ptr(), n, d, ldx, flags.data_ptr(), n_pad, d_pad, a["ops"].data_ptr(),
              a["norm"].data_ptr(), a["parts"].data_ptr(), a["acc0"].data_ptr(), a["status"].data_ptr(), stream)
    _lib.call("dal_quant_fp4", a["ops"].data_ptr(), n_pad, d_pad, a["codes"].data_ptr(), stream)
    ws, wsp = workspace(res_bytes, cuda)
    _lib.call("dal_gram_sym_residual_fp4", a["ops"].data_ptr(), nb, 0, nb, d_pad, a["acc"].data_ptr(), wsp, res_bytes,
              stream)
    torch.cuda.synchronize(cuda)
    a["sig"], a["stilde"], a["cb"] = residual_words(ws, wsp)

    b = buffers()
    b["sig_t"] = torch.full((n_pad // 512, d_pad), -1, dtype=torch.int64, device=cuda)
    b["sl_t"] = torch.full((d_pad,), -1, dtype=torch.int64, device=cuda)
    pb = int(lib.dal_prep_split_fp4_workspace_bytes(n_pad, d_pad))
    pws, pwsp = workspace(pb, cuda)
    _lib.call("dal_prep_split_fp4", x.data_ptr(), n, d, ldx, flags.data_ptr(), n_pad, d_pad, b["ops"].data_ptr(),
              b["norm"].data_ptr(), b["parts"].data_ptr(), b["acc0"].data_ptr(), b["codes"].data_ptr(),
              b["sig_t"].data_ptr(), b["sl_t"].data_ptr(), pwsp, pb, b["status"].data_ptr(), stream)
    ws2, wsp2 = workspace(res_bytes, cuda)
    _lib.call("dal_gram_sym_residual_fp4_pre", b["ops"].data_ptr(), nb, 0, nb, d_pad, b["acc"].data_ptr(),
              b["sig_t"].data_ptr(), b["sl_t"].data_ptr(), wsp2, res_bytes, stream)
    torch.cuda.synchronize(cuda)
    _, b["stilde"], b["cb"] = residual_words(ws2, wsp2)
    b["sig"] = _np(b["sig_t"]).reshape(-1)
    return a, b, (n, n_pad, d_pad)


@pytest.fixture(scope="module")
def both(cuda):
    cache = {}

    def get(name):
        if name not in cache:
            x, d, ex = _case(name)
            cache[name] = _run_both(cuda, x, d, ex) + (x, d, ex)
        return cache[name]

    return get


@pytest.mark.parametrize("name", CASES)
def test_fused_prep_writes_the_separate_entries_bytes(both, name):
    a, b, (n, n_pad, d_pad), x, d, ex = both(name)
    for key in ("norm", "ops", "parts", "acc0", "codes", "status"):
        ga, gb = _np(a[key]), _np(b[key])
        assert ga.tobytes() == gb.tobytes(), (name, key, np.flatnonzero(ga.reshape(-1).view(np.uint8) !=
                                                                       gb.reshape(-1).view(np.uint8))[:8])
    assert not _np(b["acc0"]).any()
    # sigma^H' per super block, and S^L' = S~ - the sigma^H' total (exact integers)
    assert np.array_equal(a["sig"], b["sig"]), np.flatnonzero(a["sig"] != b["sig"])[:8]
    assert a["sig"].any()
    stilde = a["stilde"].view(np.float64)
    assert np.all(np.abs(stilde) < 2.0 ** 52) and np.array_equal(stilde, np.rint(stilde))
    s_l = stilde.astype(np.int64) - a["sig"].reshape(-1, d_pad).sum(axis=0)
    assert np.array_equal(s_l, _np(b["sl_t"])), np.flatnonzero(s_l != _np(b["sl_t"]))[:8]
    assert s_l.any()
    # the residual fed with the fused sums: the same S~, D_B and accumulator
    assert a["stilde"].tobytes() == b["stilde"].tobytes()
    assert a["cb"].tobytes() == b["cb"].tobytes()
    assert np.array_equal(_np(a["acc"]), _np(b["acc"])) and _np(a["acc"]).any()


def test_zero_row_sets_the_flag_and_writes_zeros(both):
    from dal import _lib

    a, b, (n, n_pad, d_pad), x, d, ex = both("zero_row")
    assert int(_np(b["status"])[0]) & _lib.DAL_FLAG_ZERO_NORM
    assert _np(b["norm"])[300] == 0.0
    assert not _np(b["ops"])[300].any() and not _np(b["codes"])[300].any()
    assert not _np(b["ops"])[5].any() and not _np(b["codes"])[5].any()  # (a row of E)
    assert not _np(b["ops"])[n:].any() and not _np(b["codes"])[n:].any()  # (padding rows)


def test_sign_nibbles_and_the_clamp_occur(both):
    _, b, _, _, _, _ = both("one_row_second_super_block")  # N(0, 1): negative a4
    q = _np(b["codes"])
    assert np.any((q & 8) != 0) and np.any((q >> 4) & 8)
    _, b, _, _, _, _ = both("clamped")
    q = _np(b["codes"])
    assert q[7, 5 // 2] >> 4 == 15       # feature 5 (odd: high nibble): -12, code 7 | 8
    assert q[515, 255 // 2] >> 4 == 7    # feature 255: +12
    _, b, _, _, _, _ = both("partial_last_chunk")  # U[0, 1): no sign bit anywhere
    q = _np(b["codes"])
    assert not np.any(q & 0x88)


def test_rule_and_constructor(cuda):
    from dal.engine import PREP_FUSED_MIN_CHUNKS, PoolState

    X = O.synthetic_pool(700, 256, seed=1)
    st = PoolState(X, device=cuda, gram="sym", gram_fp4=True)
    assert st.gram_fp4 and not st.prep_fused and (700 + 255) // 256 < PREP_FUSED_MIN_CHUNKS
    assert PoolState(X, device=cuda, gram="sym", gram_fp4=True, prep_fused=True).prep_fused
    with pytest.raises(ValueError):
        PoolState(X, device=cuda, gram="sym", gram_i8=False, prep_fused=True)  # the fp16 form
    with pytest.raises(ValueError):
        PoolState(X, device=cuda, gram="sym", gram_fp4=True, prep_fused=True, row_base=512, n_total=2048)


@pytest.fixture(scope="module")
def end_to_end(cuda):
    from dal.engine import PoolState, density_step
    from dal.forest import Forest

    n, d, k = 36000, 256, 25
    X = O.synthetic_pool(n, d, seed=5)
    F = Forest.synthetic(10, 4, d, seed=1)
    ex = list(range(10))
    unl = np.arange(10, n)
    out = {}
    for fused in (True, False):
        st = PoolState(X, excluded=ex, device=cuda, prep_fused=fused)
        assert st.gram_fp4 and st.prep_fused == fused  # the default rule's form
        s1 = density_step(st, unl, F, k)
        dens1 = _np(st.density_fixed()).copy()
        more = [11, 300, 511, 512, 20000, n - 1]
        assert st.exclude(more) == len(more)
        unl2 = np.setdiff1d(unl, more)
        s2 = density_step(st, unl2, F, k)
        # a cold density of the grown E on a fresh pool of the same path
        st2 = PoolState(X, excluded=ex + more, device=cuda, prep_fused=fused)
        out[fused] = dict(dens1=dens1, i1=_np(s1.indices), v1=_np(s1.selected_scores), i2=_np(s2.indices),
                          v2=_np(s2.selected_scores), dens2=_np(st.density_fixed()).copy(),
                          cold2=_np(st2.density_fixed()).copy(), codes=_np(st.gram_operand_fp4()).copy(),
                          ops=_np(st.gram_operand()).copy())
    return out


def test_end_to_end_density_is_identical(end_to_end):
    t, f = end_to_end[True], end_to_end[False]
    assert t["dens1"].dtype == np.int64 and t["dens1"].any()
    assert np.array_equal(t["dens1"], f["dens1"])
    assert np.array_equal(t["cold2"], f["cold2"])  # density_fixed() without a step before it


def test_end_to_end_selection_is_identical(end_to_end):
    t, f = end_to_end[True], end_to_end[False]
    assert np.array_equal(t["i1"], f["i1"]) and t["v1"].tobytes() == f["v1"].tobytes()


def test_end_to_end_after_exclude(end_to_end):
    t, f = end_to_end[True], end_to_end[False]
    assert np.array_equal(t["i2"], f["i2"]) and t["v2"].tobytes() == f["v2"].tobytes()
    assert np.array_equal(t["dens2"], f["dens2"])
    assert t["codes"].tobytes() == f["codes"].tobytes() and t["ops"].tobytes() == f["ops"].tobytes()
