"""Multiclass votes over the blocked pool copy, host side: the three new
symbols' argument lists, the applicability rule
(dal_forest_multiclass_blocked_rows) and the entries' argument validation.
CPU only: every call here returns before any device work."""
import ctypes
import itertools
from ctypes import c_double, c_int, c_int32, c_int64, c_void_p

import pytest

from dal import _lib

ERR_ARG, ERR_SHAPE, ERR_UNSUPPORTED = -1, -2, -3


def test_symbols_and_argument_lists():
    lib = _lib.load()
    S = _lib.SIGNATURES
    assert lib.dal_abi_version() == 10  # new symbols only
    assert S["dal_forest_multiclass_blocked_rows"] == (c_int, [c_int64, c_int32, c_int32, c_int32])
    # x, xb, fprep, then the row-major entry's arguments from n on
    for name in ("dal_forest_score_multiclass", "dal_forest_score_multiclass_dw"):
        res, args = S[name]
        assert S[name + "_blocked"] == (res, [c_void_p] * 3 + args[1:])
        assert callable(getattr(lib, name + "_blocked"))
    assert S["dal_forest_score_multiclass_dw_blocked"][1][12:17] == [c_void_p, c_int, c_double, c_void_p, c_double]
    assert len(S["dal_forest_score_multiclass_blocked"][1]) == 20
    assert len(S["dal_forest_score_multiclass_dw_blocked"][1]) == 25


def test_rule_values():
    rows = _lib.load().dal_forest_multiclass_blocked_rows
    assert rows(256, 10, 4, 10) == 64
    assert rows(64, 100, 4, 10) == 64
    assert rows(64, 255, 4, 32) == 64
    assert rows(40, 255, 8, 32) == 0      # a 585 KB forest
    assert rows(70_000, 10, 4, 3) == 0    # a 16-bit feature list
    assert rows(256, 10, 4, 1) == 0 and rows(256, 10, 4, 33) == 0
    assert rows(256, 256, 4, 10) == 0 and rows(64, 256, 1, 3) == 0
    assert rows(256, 0, 4, 10) == 0 and rows(0, 10, 4, 10) == 0 and rows(256, 10, 0, 10) == 0
    assert rows(256, 10, 17, 10) == 0


def test_rule_implies_a_prepared_forest():
    lib = _lib.load()
    hits = 0
    for d, T, depth, C in itertools.product((1, 30, 64, 256, 1100), (1, 10, 100, 255), (1, 4, 8), (2, 3, 8, 32)):
        r = lib.dal_forest_multiclass_blocked_rows(d, T, depth, C)
        assert r in (0, 64)
        if r:
            hits += 1
            assert lib.dal_forest_blocked_rows(d, T, depth) == 64, (d, T, depth, C)
            assert lib.dal_forest_prep_bytes(d, T, depth) > 0, (d, T, depth, C)
    assert hits > 50  # the rule is not vacuous over the grid


def test_rule_counts_the_exchange_region():
    """A forest the binary rule takes with less than one exchange region to
    spare: more classes (more packed words per row) turn the C-class rule off."""
    lib = _lib.load()
    d, depth = 256, 4
    found = False
    for T in range(100, 256):
        if lib.dal_forest_blocked_rows(d, T, depth) and not lib.dal_forest_multiclass_blocked_rows(d, T, depth, 32):
            assert lib.dal_forest_multiclass_blocked_rows(d, T, depth, 2) in (0, 64)
            found = True
            break
    assert found


P = ctypes.c_void_p(256)  # a 16-B aligned address that is never dereferenced


def _us(x=P, xb=P, fprep=P, n=10, d=256, ldx=256, inner=P, leaf=P, T=10, depth=4, C=10, lut=P, kind=2, flags=None,
        order=1, counts=P, pred=P, scores=P, keys=P):
    return _lib.load().dal_forest_score_multiclass_blocked(x, xb, fprep, n, d, ldx, inner, leaf, T, depth, C, lut,
                                                           kind, flags, order, counts, pred, scores, keys, None)


def _dw(x=P, xb=P, fprep=P, n=10, d=256, ldx=256, inner=P, leaf=P, T=10, depth=4, C=10, lut=P, density=P, dkind=1,
        derr=0.0, flags=None, beta=1.0, counts=P, pred=P, entropy=P, row_index=P, scores=P, keys=P, keys_hi=P):
    return _lib.load().dal_forest_score_multiclass_dw_blocked(x, xb, fprep, n, d, ldx, inner, leaf, T, depth, C, lut,
                                                              density, dkind, derr, flags, beta, counts, pred, entropy,
                                                              row_index, scores, keys, keys_hi, None)


@pytest.mark.parametrize("xb", [P, None], ids=["blocked", "xb-null"])
def test_validation_without_gpu(xb):
    """The row-major entries' checks and statuses, with and without xb."""
    for name in ("x", "inner", "leaf", "lut", "scores", "keys"):
        assert _us(xb=xb, **{name: None}) == ERR_ARG, name
    for name in ("x", "inner", "leaf", "lut", "density", "entropy", "row_index", "scores", "keys"):
        assert _dw(xb=xb, **{name: None}) == ERR_ARG, name
    assert _us(xb=xb, order=2) == ERR_ARG and _us(xb=xb, kind=3) == ERR_ARG
    assert _dw(xb=xb, dkind=0) == ERR_ARG and _dw(xb=xb, dkind=3) == ERR_ARG
    for f in (_us, _dw):
        assert f(xb=xb, n=-1) == ERR_SHAPE and f(xb=xb, d=0) == ERR_SHAPE and f(xb=xb, ldx=255) == ERR_SHAPE
        assert f(xb=xb, C=1) == ERR_UNSUPPORTED and f(xb=xb, C=33) == ERR_UNSUPPORTED
        assert f(xb=xb, T=0) == ERR_UNSUPPORTED and f(xb=xb, T=256) == ERR_UNSUPPORTED
        assert f(xb=xb, depth=0) == ERR_UNSUPPORTED and f(xb=xb, depth=17) == ERR_UNSUPPORTED
        assert f(xb=xb, n=0) == 0                                     # nothing to score: no launch
        assert f(xb=xb, n=0, counts=None, pred=None) == 0             # the optional outputs
    assert _dw(xb=xb, n=1 << 31) == ERR_SHAPE                         # row_index is int32
    assert _dw(xb=xb, n=0, keys_hi=None, dkind=2) == 0


def test_blocked_operands_validation_without_gpu():
    rows = _lib.load().dal_forest_multiclass_blocked_rows
    assert rows(256, 10, 4, 10) == 64
    for f in (_us, _dw):
        assert f(fprep=None) == ERR_ARG                               # no unprepared form
        assert f(fprep=None, n=0) == ERR_ARG                          # ... an argument error at any n
        assert f(fprep=ctypes.c_void_p(264)) == ERR_ARG               # fprep 8-B aligned only
        assert f(xb=ctypes.c_void_p(260)) == ERR_ARG                  # misaligned xb
        assert f(xb=ctypes.c_void_p(264), n=0) == ERR_ARG
        # the rule is 0 (a 585 KB forest): fprep is ignored, xb still 16-B aligned
        assert rows(40, 255, 8, 32) == 0
        kw = dict(d=40, ldx=40, T=255, depth=8, C=32, n=0)
        assert f(fprep=None, **kw) == 0
        assert f(xb=ctypes.c_void_p(260), **kw) == ERR_ARG
        # xb NULL: the row-major entry, whatever fprep is
        assert f(xb=None, fprep=None, n=0) == 0 and f(xb=None, fprep=ctypes.c_void_p(264), n=0) == 0
