"""Every exported entry that takes a leading dimension (``ldx`` of an fp32 or
fp64 pool, ``ld`` of a bf16 pool or of the normalised rows) refuses a stride
shorter than the row with DAL_ERR_SHAPE -- on the host, before any device
call.  CPU only: the pointers are fake (non-null, 256-byte aligned), so a call
that got past its checks would fault; every call here is a refusal.

The entries are read from include/dal.h; the table below must name exactly
those.  Also here, because it needs no GPU: the case table of
tests/test_gpu_strided_pool.py against the restated staging predicates."""
import ctypes
import os
import re

import pytest

import strided_pool as SP
import test_gpu_strided_pool as G
from conftest import REPO
from dal import _lib

ERR_ARG, ERR_SHAPE = -1, -2
P = ctypes.c_void_p(256)


def leading_dimension_entries():
    """{name: [(type, parameter name), ...]} of every declaration of
    include/dal.h with an ``int64_t ldx`` or ``int64_t ld`` parameter."""
    src = open(os.path.join(REPO, "include", "dal.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, params in re.findall(r"\bint\s+(dal_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        plist = []
        for prm in params.split(","):
            m = re.fullmatch(r"\s*(.*?)(\w+)\s*", prm, flags=re.S)
            plist.append((" ".join(m.group(1).split()), m.group(2)))
        if any(t == "int64_t" and p in ("ldx", "ld") for t, p in plist):
            out[name] = plist
    return out


# Arguments by parameter name: a small valid shape in which the leading
# dimension alone is wrong (d - 1, or d_pad - 4 where the entry also wants a
# multiple of 4, d - 8 where it wants a multiple of 8).
DEFAULTS = dict(n=10, n_local=10, d=4, ldx=3, n_pad=512, d_pad=32, n_trees=3, depth=2, max_depth=2, n_classes=3,
                density_kind=0, density_err=0.0, beta=1.0, order=0, score_kind=0, k=2, idx_base=0, cap=10,
                level1_passes=0, ws_bytes=1 << 20, step_flags=0, n_chunks=1, n_sample=10, num_splits=9, m=2,
                min_instances=1, min_info_gain=0.0, x_dtype=0, out_dtype=0, ldo=4, k1=1, k2=1, feature_major=0,
                grid_blocks=0)
BF16 = dict(d=64, ld=63, m=4, m_pad=4)

# name -> overrides of DEFAULTS
TABLE = {
    "dal_normalize_rows": {}, "dal_canon_colsum_partials": {}, "dal_canon_colsum_partials_chunks": {},
    "dal_density_separable": {}, "dal_prep_split": {}, "dal_cosine_pairs_resolve": dict(n_cand=5),
    "dal_forest_score": {}, "dal_pool_blocked": {}, "dal_forest_score_blocked": {}, "dal_forest_evaluate": {},
    "dal_forest_score_multiclass": {}, "dal_forest_score_multiclass_dw": dict(density_kind=1),
    "dal_forest_score_multiclass_blocked": {}, "dal_forest_score_multiclass_dw_blocked": dict(density_kind=1),
    "dal_dw_select": {}, "dal_dw_step": {}, "dal_dw_step_multiclass": {},
    "dal_dw_plan_create": {}, "dal_dw_plan_create_multiclass": {},
    "dal_forest_regress": {}, "dal_rf_find_splits": {}, "dal_rf_find_splits_f64": {}, "dal_rf_bin_rows": {},
    "dal_rf_train": {}, "dal_rf_train_multiclass": {}, "dal_rf_train_begin": {}, "dal_rf_train_multiclass_begin": {},
    "dal_scaler_format": {}, "dal_scaler_accumulate": {}, "dal_scaler_transform": {},
    # the normalised rows u [n_pad][ld]: ld >= d_pad (and a multiple of 4 for the two 16-byte readers)
    "dal_gram_rowsum": dict(n_rows_pad=256, n_cols_pad=512, d_pad=64, ld=60),
    "dal_split_f16": dict(d_pad=64, ld=60), "dal_gram_entries": dict(n_pad=32, d_pad=64, ld=63),
    # bf16 pools
    "dal_inv_norms_bf16": BF16, "dal_canon_unit_rows_bf16": BF16, "dal_unit_rows_f16": BF16,
    "dal_maxcos_argmax_resolve": BF16, "dal_maxcos_select": BF16,
    "dal_kcenter_begin": dict(BF16, ld=56), "dal_kcenter_select": dict(BF16, ld=56),
}


def _call(name, params, **over):
    """Call ``name`` with fake pointers and the table's values; ``over`` last."""
    values = dict(DEFAULTS, **TABLE[name])
    values.update(over)
    keep = []  # real memory for what a refusing entry may still write
    args = []
    for typ, prm in params:
        if prm in over and not isinstance(over[prm], (int, float)):
            args.append(over[prm])
        elif typ in ("dal_stream_t", "dal_event_t"):
            args.append(None)
        elif prm == "job" and "*" in typ:  # a refused dal_kcenter_begin clears the descriptor
            keep.append(ctypes.create_string_buffer(max(_lib.DAL_RF_JOB_BYTES, _lib.DAL_KCENTER_JOB_BYTES)))
            args.append(keep[-1])
        elif typ.endswith("**"):  # the plan's out pointer is nulled by a refusal
            keep.append(ctypes.c_void_p(0x55))
            args.append(ctypes.byref(keep[-1]))
        elif "*" in typ:
            args.append(P)
        else:
            args.append(values[prm])
    rc = getattr(_lib.load(), name)(*args)
    if keep and isinstance(keep[-1], ctypes.c_void_p):
        assert keep[-1].value is None  # no plan behind a refusal
    return rc


def test_table_names_every_leading_dimension_entry():
    entries = leading_dimension_entries()
    assert len(entries) >= 40
    assert set(TABLE) == set(entries), set(TABLE) ^ set(entries)
    assert set(entries) <= set(_lib.SIGNATURES)
    for name, params in entries.items():
        assert len(params) == len(_lib.SIGNATURES[name][1]), name


@pytest.mark.parametrize("name", sorted(TABLE))
def test_short_leading_dimension_is_refused(name):
    params = leading_dimension_entries()[name]
    names = [p for _, p in params]
    ld = "ldx" if "ldx" in names else "ld"
    values = dict(DEFAULTS, **TABLE[name])
    width = values["d"] if "d" in names else values["d_pad"]
    assert values[ld] < width  # the row is wider than the stride ...
    assert _call(name, params) == ERR_SHAPE
    # ... by as little as one element (where no other rule of the entry speaks first)
    if name not in ("dal_gram_rowsum", "dal_split_f16", "dal_kcenter_begin", "dal_kcenter_select"):
        assert _call(name, params, **{ld: width - 1}) == ERR_SHAPE
    # a null pool is DAL_ERR_ARG whatever the stride says: the documented order
    pool = params[1][1] if names[0] == "job" else "pool" if "pool" in names else names[0] if ld == "ld" else "x"
    assert pool in names
    assert _call(name, params, **{pool: None}) == ERR_ARG


def test_kcenter_stride_and_alignment_rules():
    """dal_kcenter_begin reads every pool row with 16-byte loads: ld % 8 != 0
    and a pool that is not 16-byte aligned are DAL_ERR_SHAPE (include/dal.h),
    each with every other argument in order."""
    entries = leading_dimension_entries()
    for name in ("dal_kcenter_begin", "dal_kcenter_select"):
        params = entries[name]
        assert _call(name, params, ld=68) == ERR_SHAPE           # ld >= d, not a multiple of 8
        assert _call(name, params, ld=60) == ERR_SHAPE
        for addr in (256 + 2, 256 + 4, 256 + 8):
            assert _call(name, params, ld=72, pool=ctypes.c_void_p(addr)) == ERR_SHAPE, addr
        assert _call(name, params, ld=72, m32=ctypes.c_void_p(256 + 4)) == ERR_SHAPE
        assert _call(name, params, ld=72, inv_norm=ctypes.c_void_p(256 + 8)) == ERR_SHAPE


def test_forest_case_table_reaches_every_staging_branch():
    """tests/test_gpu_strided_pool.py's forest cases through the restated
    predicates (any 256-byte aligned buffer, the first row offset_elems floats
    in): each case names the branch and the rows per block it reaches, every
    branch of the row-major kernels occurs, both R of d = 128 occur, and the
    second LDS-DMA piece of a d = 260 row has one live lane."""
    seen = set()
    for d, ldx, off, T, staging, R in G.FOREST_CASES:
        t = SP.forest_tiling(d, ldx, 4096 + 4 * off, T)
        assert (t.staging, t.R) == (staging, R), (d, ldx, off, T, t)
        assert G.N % R != 0  # a ragged last tile
        seen.add((staging, d % 4 == 0, ldx > d, d >= 128))
    # (staging, d % 4 == 0, strided, d >= 128)
    assert {("scalar", False, True, False), ("scalar", True, True, False), ("scalar", True, False, False),
            ("scalar", True, True, True), ("scalar", True, False, True), ("vec4", True, True, False),
            ("dma", True, True, True), ("dma", True, False, True), ("none", True, True, True)} <= seen
    assert {R for d, _, _, _, _, R in G.FOREST_CASES if d == 128} == {32, 64}
    # n_trees >= 64 shrinks R through tpr_min in at least one case of each staging it can meet
    shrunk = {s for d, ldx, off, T, s, R in G.FOREST_CASES if SP.forest_tiling(d, ldx, 4096 + 4 * off, 10).R > R}
    assert shrunk == {"vec4", "scalar"}
    assert SP.dma_pieces(260) == (2, 1) and SP.dma_pieces(128) == (1, 32) and SP.dma_pieces(256) == (1, 64)
    for ldx, off, staging, R in G.SEL_STRIDES:
        t = SP.forest_tiling(G.SEL_D, ldx, 4096 + 4 * off, G.SEL_T)
        assert (t.staging, t.R) == (staging, R)
    # the contiguous layout every other test passes: the branches the engine runs
    assert SP.forest_tiling(64, 64, 4096, 10).staging == "vec4" and SP.forest_tiling(30, 30, 4096, 10).staging == "scalar"
    assert SP.forest_tiling(256, 256, 4096, 10)[:2] == ("dma", 32)
    # n_trees >= 64 halves a 256-row tile (d <= 15); at d = 64 and 128 R already leaves two lanes per row
    assert SP.forest_tiling(13, 13, 4096, 10).R == 256 and SP.forest_tiling(13, 13, 4096, 100).R == 128


def test_strided_helper_layout():
    """strided_pool's layout arithmetic, on the host: where the logical
    entries sit and what the poison is."""
    import numpy as np

    for dtype in (np.float32, np.float64, np.uint16):
        X = (np.arange(12).reshape(3, 4) + 1).astype(dtype)
        for ldx, off in ((4, 0), (7, 3), (5, 1)):
            host = SP.layout(X, ldx, off)
            assert host.dtype == dtype and host.size == off + 2 * ldx + 4 + SP.TAIL and SP.TAIL >= 64
            logical = np.zeros(host.size, dtype=bool)
            for i in range(3):
                assert np.array_equal(host[off + i * ldx: off + i * ldx + 4], X[i])
                logical[off + i * ldx: off + i * ldx + 4] = True
            rest = host[~logical]
            assert rest.size == off + 2 * (ldx - 4) + SP.TAIL
            assert (rest == SP.BF16_NAN).all() if dtype == np.uint16 else np.isnan(rest).all()
    with pytest.raises(ValueError):
        SP.layout(np.zeros((2, 4), np.float32), 3, 0)
