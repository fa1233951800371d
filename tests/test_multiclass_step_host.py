"""The fused multiclass density step and its plan, host side: the three new
symbols' argument lists, the branch rule (dal_dw_step_multiclass_form) at the
shapes the GPU tests use, and the entry's argument validation.  CPU only: every
call here returns before any device work."""
import ctypes
from ctypes import c_int, c_int32, c_int64, c_void_p

from dal import _lib

ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED, ERR_CAPACITY = -1, -2, -3, -5
EXACT, GROUP_MIN, FOLD_STORES, FOLD_ATOMICS = 0, 1, 2, 3
PAYLOAD = _lib.DAL_SORT_CAP_PAYLOAD


def test_symbols_and_argument_lists():
    lib = _lib.load()
    S = _lib.SIGNATURES
    assert lib.dal_abi_version() == 10  # new symbols only
    for name in ("dal_dw_step_multiclass", "dal_dw_step_multiclass_form", "dal_dw_plan_create_multiclass"):
        assert callable(getattr(lib, name)), name
    # dal_dw_step's arguments with n_classes after depth and counts, pred, entropy, row_index for votes
    res, step = S["dal_dw_step"]
    assert S["dal_dw_step_multiclass"] == (res, step[:10] + [c_int32] + step[10:24] + [c_void_p] * 4 + step[25:])
    assert len(S["dal_dw_step_multiclass"][1]) == 38
    # ... and the same two changes to dal_dw_plan_create's
    res, plan = S["dal_dw_plan_create"]
    assert S["dal_dw_plan_create_multiclass"] == (res, plan[:10] + [c_int32] + plan[10:24] + [c_void_p] * 4 + plan[25:])
    assert len(S["dal_dw_plan_create_multiclass"][1]) == 37
    assert S["dal_dw_step_multiclass_form"] == (c_int, [c_int64, c_int64, c_int32, c_int32, c_int32, c_int64, c_int64,
                                                        c_int32, c_int])


def _form(n, d, T, depth, C, k, cap=None, passes=1, blocked=1):
    cap = min(n, max(4 * k, PAYLOAD)) if cap is None else cap  # engine.candidate_cap
    return _lib.load().dal_dw_step_multiclass_form(n, d, T, depth, C, k, cap, passes, blocked)


def test_form_at_the_gpu_tests_shapes():
    rows = _lib.load().dal_forest_multiclass_blocked_rows
    for d, T, depth, C in ((256, 10, 4, 10), (16, 10, 4, 3), (30, 10, 4, 3), (32, 10, 4, 4), (256, 100, 4, 10)):
        assert rows(d, T, depth, C) == 64
    assert _form(2500, 256, 10, 4, 10, 16) == FOLD_STORES      # 40 tiles >= 2k groups of one tile
    assert _form(2500, 256, 100, 4, 10, 16) == FOLD_STORES     # (the eight-wave block)
    assert _form(300_037, 16, 10, 4, 3, 20) == FOLD_ATOMICS    # 4,689 tiles, two per group
    assert _form(1037, 30, 10, 4, 3, 20) == GROUP_MIN          # 17 tiles < 2k
    assert _form(6000, 32, 10, 4, 4, 20) == FOLD_STORES        # the plan test's shape
    # the row-major kernel runs: no fold, with or without a blocked copy
    assert rows(40, 255, 8, 32) == 0
    assert _form(600, 40, 255, 8, 32, 10) == GROUP_MIN
    assert _form(2500, 256, 10, 4, 10, 16, blocked=0) == GROUP_MIN
    assert _form(300_037, 16, 10, 4, 3, 20, blocked=0) == GROUP_MIN


def test_form_exact_level_one():
    assert _form(2500, 256, 10, 4, 10, 16, passes=0) == EXACT
    assert _form(300_037, 16, 10, 4, 3, 20, passes=0) == EXACT
    # a capacity past the one-block sort has no fast level 1
    assert _form(300_037, 16, 10, 4, 3, 20, cap=PAYLOAD + 1, passes=0) == EXACT
    assert _form(300_037, 16, 10, 4, 3, 20, cap=PAYLOAD + 1, passes=1) == EXACT
    assert _form(300_037, 16, 10, 4, 3, 20, cap=PAYLOAD, passes=1) == FOLD_ATOMICS


def test_form_statuses():
    assert _form(0, 256, 10, 4, 10, 16) == 0                                    # n == 0: DAL_OK, first
    assert _form(2500, 256, 10, 4, 1, 16) == ERR_UNSUPPORTED
    assert _form(2500, 256, 10, 4, 33, 16) == ERR_UNSUPPORTED
    assert _form(2500, 256, 256, 4, 10, 16) == ERR_UNSUPPORTED
    assert _form(2500, 256, 10, 17, 10, 16) == ERR_UNSUPPORTED
    assert _form(1 << 31, 256, 10, 4, 10, 16) == ERR_SHAPE                      # row_index is int32
    assert _form(2500, 0, 10, 4, 10, 16) == ERR_SHAPE
    assert _form(2500, 256, 10, 4, 10, 0) == ERR_SHAPE
    assert _form(2500, 256, 10, 4, 10, 16, cap=8) == ERR_SHAPE                  # cap < k
    assert _form(2500, 256, 10, 4, 10, 16, passes=6) == ERR_ARG
    assert _form(2500, 256, 10, 4, 10, 16, passes=-1) == ERR_ARG
    assert _form(20_000, 256, 10, 4, 10, 9000, cap=9000, passes=0) == ERR_CAPACITY


P = c_void_p(256)  # a 16-B aligned address that is never dereferenced
WS = c_void_p(1 << 20)  # 256-B aligned


def _step(x=P, xb=P, fprep=P, n=2500, d=256, ldx=256, inner=P, leaf=P, T=10, depth=4, C=10, lut=P, density=P, derr=0.0,
          flags=P, beta=1.0, idx_base=0, norm64=P, colsum=P, k=16, cap=2500, passes=1, step_flags=0, ws=WS,
          ws_bytes=None, counts=P, pred=P, entropy=P, row_index=P, scores=P, keys_lo=P, keys_hi=P, out_idx=P,
          out_scores=P, out_keys=P, status=P):
    lib = _lib.load()
    if ws_bytes is None:
        ws_bytes = 0  # (too small: the last check before any device work)
    return lib.dal_dw_step_multiclass(x, xb, fprep, n, d, ldx, inner, leaf, T, depth, C, lut, density, derr, flags,
                                      beta, idx_base, norm64, colsum, k, cap, passes, step_flags, ws, ws_bytes,
                                      counts, pred, entropy, row_index, scores, keys_lo, keys_hi, out_idx,
                                      out_scores, out_keys, status, None, None)


def test_entry_validation_without_gpu():
    """Every argument error comes back before device work.  A call whose
    arguments are all valid is stopped here by its workspace size (0 bytes:
    DAL_ERR_SHAPE, the last host check)."""
    assert _step() == ERR_SHAPE and _step(counts=None, pred=None) == ERR_SHAPE  # valid but for the workspace
    for name in ("x", "inner", "leaf", "lut", "density", "norm64", "colsum", "ws", "entropy", "row_index", "scores",
                 "keys_lo", "keys_hi", "out_idx", "out_scores", "status"):
        assert _step(**{name: None}) == ERR_ARG, name
        assert _step(xb=None, **{name: None}) == ERR_ARG, name
    for xb in (P, None):
        assert _step(xb=xb, C=1) == ERR_UNSUPPORTED and _step(xb=xb, C=33) == ERR_UNSUPPORTED
        assert _step(xb=xb, T=256) == ERR_UNSUPPORTED and _step(xb=xb, T=0) == ERR_UNSUPPORTED
        assert _step(xb=xb, depth=17) == ERR_UNSUPPORTED
        assert _step(xb=xb, n=1 << 31) == ERR_SHAPE
        assert _step(xb=xb, n=-1) == ERR_SHAPE and _step(xb=xb, ldx=255) == ERR_SHAPE
        # the two measurement flags are not this entry's
        assert _step(xb=xb, step_flags=_lib.DAL_STEP_KEEP_GROUPS) == ERR_ARG
        assert _step(xb=xb, step_flags=_lib.DAL_STEP_SELECT_ONLY | _lib.DAL_STEP_WS_CLEAN) == ERR_ARG
        assert _step(xb=xb, step_flags=16) == ERR_ARG
        assert _step(xb=xb, step_flags=_lib.DAL_STEP_RESET_STATUS | _lib.DAL_STEP_WS_CLEAN) == ERR_SHAPE
        assert _step(xb=xb, n=0) == 0                      # nothing to score or select
        assert _step(xb=xb, k=0) == ERR_SHAPE and _step(xb=xb, k=2501) == ERR_SHAPE and _step(xb=xb, cap=8) == ERR_SHAPE
        assert _step(xb=xb, passes=6) == ERR_ARG
    # the blocked operands
    assert _step(xb=c_void_p(260)) == ERR_ARG              # misaligned xb
    assert _step(fprep=None) == ERR_ARG                    # the rule gives 64: no unprepared form
    assert _step(fprep=c_void_p(264)) == ERR_ARG
    assert _step(fprep=None, n=0) == ERR_ARG
    kw = dict(n=600, d=40, ldx=40, T=255, depth=8, C=32, k=10, cap=600)
    assert _lib.load().dal_forest_multiclass_blocked_rows(40, 255, 8, 32) == 0
    assert _step(fprep=None, **kw) == ERR_SHAPE            # the rule gives 0: fprep ignored (workspace next)
    assert _step(xb=None, fprep=None) == ERR_SHAPE         # xb NULL: the row-major kernel, fprep ignored
    # a misaligned workspace of the right size
    need = _lib.load().dal_dw_step_workspace_bytes(2500, 16, 2500)
    assert _step(ws=c_void_p((1 << 20) + 8), ws_bytes=need) == ERR_SHAPE


def test_plan_create_validation_without_gpu():
    lib = _lib.load()
    plan = c_void_p()
    args = [P, P, P, 2500, 256, 256, P, P, 10, 4, 10, P, P, 0.0, P, P, 1.0, 0, P, P, 16, 2500, 1, WS, 0, P, P, P, P, P,
            P, P, P, P, P, None]
    assert lib.dal_dw_plan_create_multiclass(*args, None) == ERR_ARG            # no plan out
    for i in (14, 15, 32, 23):  # base_flags, flags, out_pair, ws
        bad = list(args)
        bad[i] = None
        assert lib.dal_dw_plan_create_multiclass(*bad, ctypes.byref(plan)) == ERR_ARG, i
        assert plan.value is None
    bad = list(args)
    bad[3] = 0
    assert lib.dal_dw_plan_create_multiclass(*bad, ctypes.byref(plan)) == ERR_SHAPE
