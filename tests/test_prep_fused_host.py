"""dal_prep_split_fp4 / dal_gram_sym_residual_fp4_pre on the host: the symbols,
the workspace size and the refusals (before any device call; the pointers are
fake, so every call here is a refusal).  The stride parameter is dal_prep_split's
``ldx`` under the name ``x_stride``; its rules are checked here."""
import ctypes

from dal import _lib

ERR_ARG, ERR_SHAPE = -1, -2
P = ctypes.c_void_p(256)


def _prep(**over):
    v = dict(x=P, n=1000, d=256, x_stride=256, flags=P, n_pad=1024, d_pad=256, out=P, norm64=P, partials=P, acc_zero=P,
             out_fp4=P, sigma_h=P, s_l=P, ws=P, ws_bytes=1 << 20, status=P, stream=None)
    v.update(over)
    return _lib.load().dal_prep_split_fp4(*v.values())


def test_symbols_and_abi_version():
    lib = _lib.load()
    assert lib.dal_abi_version() == 10  # new symbols only
    for name in ("dal_prep_split_fp4", "dal_prep_split_fp4_workspace_bytes", "dal_gram_sym_residual_fp4_pre"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES


def test_workspace_bytes():
    lib = _lib.load()
    assert lib.dal_prep_split_fp4_workspace_bytes(1024, 256) == 2 * 256 * 8  # one partial row per super block ...
    assert lib.dal_prep_split_fp4_workspace_bytes(4096 * 512 * 3, 512) == 4096 * 512 * 8  # ... 4,096 at most
    assert lib.dal_prep_split_fp4_workspace_bytes(0, 256) == 0


def test_prep_refusals():
    assert _prep(x_stride=255) == ERR_SHAPE  # a stride shorter than the row
    assert _prep(d=200, x_stride=199) == ERR_SHAPE
    assert _prep(x=None, x_stride=255) == ERR_ARG  # a null pool first, whatever the stride says
    for name in ("out", "norm64", "out_fp4", "sigma_h", "s_l", "ws", "status"):
        assert _prep(**{name: None}) == ERR_ARG, name
    assert _prep(d=64, x_stride=64, d_pad=64) == ERR_SHAPE    # not a 256-feature slice
    assert _prep(d=128, x_stride=128, d_pad=128) == ERR_SHAPE
    assert _prep(n=0) == ERR_SHAPE
    assert _prep(n_pad=768) == ERR_SHAPE and _prep(n=1025) == ERR_SHAPE
    assert _prep(out=ctypes.c_void_p(264)) == ERR_SHAPE       # 16-byte stores
    assert _prep(ws_bytes=2 * 256 * 8 - 1) == ERR_SHAPE


def test_residual_pre_refusals():
    f = _lib.load().dal_gram_sym_residual_fp4_pre
    ok = [P, 4, 0, 4, 256, P, P, P, P, 1 << 20, None]

    def call(i, v):
        a = list(ok)
        a[i] = v
        return f(*a)

    assert call(6, None) == ERR_ARG and call(7, None) == ERR_ARG  # the caller's sums
    assert call(0, None) == ERR_ARG and call(5, None) == ERR_ARG and call(8, None) == ERR_ARG
    assert call(4, 128) == ERR_SHAPE
    assert call(1, 3) == ERR_SHAPE
    assert call(9, 16) == ERR_SHAPE  # a short workspace
