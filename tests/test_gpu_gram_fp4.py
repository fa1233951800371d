"""The fp4 form of the symmetric density Gram (gram_fp4sym_kernel: exact row
sums of <a4_i, a4_j>, a4 = the element of +-{0, 1, 2, 3, 4, 6, 8, 12} nearest to
H / 32, by v_mfma_scale_f32_16x16x128_f8f6f4 over 256-feature slices;
dal_gram_sym_residual_fp4 adds the rest in closed form), forced on small pools
with ``gram_fp4=True``:

 1. the operand read back (dal_quant_fp4) is the e2m1 code of a4 of the split
    operand's H, even feature in the low nibble, and gram_accumulate alone
    adds, bit for bit, 2^18 sum_{taken pairs} <a4_r, a4_j> (NumPy int64;
    padding and excluded rows 0) -- d = 200 (a zero-padded tail), 256 (one
    slice), 512 (two): the check that catches a wrong lane map, nibble order,
    slice offset or fold, an idle half, a last row unit with one live super
    block;
 2. the density meets the two assertions of test_gpu_gram_hh._check_density,
    and its error against the split operand's fp64 row sums is no larger than
    the fp16 form's on the same pool;
 3. the bits do not depend on the grid, the column split or a skip range with
    a column offset;
 4. the same on a pool whose a4 clamps (rows near +-e_1 among dense rows);
 5. the default rule (constructor checks), and the int8 wide form at d = 256,
    which the rule no longer reaches.
Needs an MI355X: ``pytest -m gpu``."""
import numpy as np
import pytest

from oracle import dal_oracle as O
from test_gpu_gram_hh import E, _np
from test_gpu_gram_i8 import _a_of, _accumulate, _density_errors, _mfma_part
from test_gram_fp4_algebra import code4, decode4, quant4

pytestmark = pytest.mark.gpu


def _pool(cuda, X, **kw):
    from dal.engine import PoolState

    return PoolState(X, excluded=E, device=cuda, gram="sym", **kw)


def _a4_of(st):
    """a4(H) [n_pad, d_pad] int64: decoded from the fp4 operand read back, and
    checked against the quantiser on the split operand (KS 128: [slice][128 H | 128 L])."""
    sp = _np(st.gram_operand()).view(np.float16).astype(np.float64)
    want = np.zeros((st.n_pad, st.d_pad), dtype=np.int64)
    for s0 in range(0, st.d_pad, 128):
        want[:, s0:s0 + 128] = quant4(sp[:, 2 * s0:2 * s0 + 128])
    q = _np(st.gram_operand_fp4())
    assert q.dtype == np.uint8 and q.shape == (st.n_pad, st.d_pad // 2)
    codes = np.stack([q & 15, q >> 4], axis=-1).reshape(st.n_pad, st.d_pad)  # feature f: byte f / 2, even f low
    assert np.array_equal(codes, code4(want))  # (so no -0 code either)
    return decode4(codes)


def _check_pool(cuda, X):
    n = X.shape[0]
    st = _pool(cuda, X, gram_fp4=True)
    assert st.gram_fp4 and not st.gram_i8 and st.d_pad % 256 == 0
    a = _a4_of(st)
    assert not a[n:].any() and not a[E].any()
    got = _accumulate(st, cuda)
    ref = _mfma_part(st, a)
    assert np.any(ref != 0)
    assert np.array_equal(got, ref), np.flatnonzero(got != ref)[:8]
    e_fp4 = _density_errors(st, X, n)
    f16 = _pool(cuda, X, gram_i8=False)
    assert not f16.gram_fp4 and not f16.gram_i8
    e_f16 = _density_errors(f16, X, n)
    assert e_fp4 <= e_f16, (e_fp4, e_f16)
    return st, a


@pytest.mark.parametrize("dist", ["uniform", "normal"])
@pytest.mark.parametrize("d", [200, 256, 512])
@pytest.mark.parametrize("n", [700, 1300, 2700, 4300])
def test_fp4_row_sums_exact_and_density_within_bound(cuda, n, d, dist):
    _check_pool(cuda, O.synthetic_pool(n, d, seed=7, dist=dist))


def test_fp4_clamped_rows(cuda):
    """2,700 x 256: every third row within 1e-3 of +-e_1 (H = +-4096 there, so
    a4 clamps at +-12 and l' carries the 3,712 left over) among dense rows."""
    rng = np.random.default_rng(21)
    X = rng.standard_normal((2700, 256), dtype=np.float32)
    spike = np.arange(11, 2700, 3)
    X[spike] *= np.float32(1e-3)
    X[spike, 0] = np.where(rng.random(spike.size) < 0.5, -1.0, 1.0).astype(np.float32)
    st, a = _check_pool(cuda, X)
    assert np.abs(a[spike, 0]).min() == 12


@pytest.mark.parametrize("n,d", [(4300, 256), (2700, 512)])
def test_fp4_bits_do_not_depend_on_the_launch(cuda, n, d):
    import torch

    st = _pool(cuda, O.synthetic_pool(n, d, seed=3), gram_fp4=True)
    op = st.gram_operand()
    a = _a4_of(st)
    ref = _mfma_part(st, a)
    for grid in (0, 1, 7, 333):
        assert np.array_equal(_accumulate(st, cuda, grid_blocks=grid), ref), grid
    q = max(512, st.n_pad // 512 // 4 * 512)  # a quarter of the columns, in whole super blocks
    part = torch.zeros(st.n_pad, dtype=torch.int64, device=cuda)
    for c0, c1 in ((2 * q, 3 * q), (0, q), (3 * q, st.n_pad), (q, 2 * q)):
        if c1 > c0:
            st.gram_accumulate(part, op[c0:], c1 - c0, col_row0=c0)
    assert np.array_equal(_np(part), ref)
    # a column offset and a skip range inside the columns; then the two ranges left out
    c0, s0, s1 = 512, 1024, min(2048, st.n_pad)
    part = torch.zeros(st.n_pad, dtype=torch.int64, device=cuda)
    st.gram_accumulate(part, op[c0:], st.n_pad - c0, col_row0=c0, skip=(s0, s1))
    assert np.array_equal(_np(part), _mfma_part(st, a, c0 // 256, None, (s0 // 256, s1 // 256)))
    st.gram_accumulate(part, op, c0, col_row0=0)
    st.gram_accumulate(part, op[s0:], s1 - s0, col_row0=s0)
    assert np.array_equal(_np(part), ref)
    # ... and the whole density: one call against the pool's own
    whole = torch.zeros(st.n_pad, dtype=torch.int64, device=cuda)
    st.gram_accumulate(whole, op, st.n_pad)
    st.gram_residual(whole, op)
    assert np.array_equal(_np(whole), _np(st.density_fixed()))


def test_default_rule(cuda):
    """The form is the pool's: fp4 where the int8 rule picks int8, gram_i8 was
    not given and d_pad is a multiple of 256 (constructors only, no Gram launch)."""
    rng = np.random.default_rng(5)

    def pool(n, d, **kw):
        return _pool(cuda, rng.random((n, d), dtype=np.float32), **kw)

    st = pool(33_000, 256)  # 33.8 MB of split operand
    assert st.gram_fp4 and not st.gram_i8
    st = pool(70_000, 128)
    assert st.gram_i8 and not st.gram_fp4
    # 384 features pad to d_pad = 512 (dal_pad_features rounds to 256 above 128;
    # 128 is the only d_pad that is a multiple of 128 and not of 256), so by
    # the rule -- d_pad % 256 == 0 -- this pool takes the fp4 form too
    st = pool(30_000, 384)
    assert st.d_pad == 512 and st.gram_fp4 and not st.gram_i8
    st = pool(4_300, 256)  # below the contiguous schedule's limit: the fp16 form
    assert not st.gram_i8 and not st.gram_fp4
    for given in (True, False):  # an explicit gram_i8 means no fp4
        st = pool(4_300, 256, gram_i8=given)
        assert st.gram_i8 == given and not st.gram_fp4
    assert pool(33_000, 256, gram_i8=True).gram_i8
    assert not pool(33_000, 256, gram_fp4=False).gram_fp4 and pool(33_000, 256, gram_fp4=False).gram_i8
    with pytest.raises(ValueError):
        pool(4_300, 128, gram_fp4=True)
    with pytest.raises(ValueError):
        pool(4_300, 256, gram_i8=True, gram_fp4=True)
    from dal.engine import PoolState

    with pytest.raises(ValueError):
        PoolState(rng.random((1_000, 256), dtype=np.float32), device=cuda, gram="f32", gram_fp4=True)


def test_i8_wide_form_stays_covered_at_256(cuda):
    """4,300 x 256 with gram_i8=True: gram_i8sym_kernel over two 128-feature
    slices, the form such pools took before the fp4 one."""
    st = _pool(cuda, O.synthetic_pool(4300, 256, seed=7), gram_i8=True)
    assert st.gram_i8 and not st.gram_fp4
    a = _a_of(st)
    ref = _mfma_part(st, a)
    assert np.any(ref != 0)
    assert np.array_equal(_accumulate(st, cuda), ref)
