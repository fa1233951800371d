"""The int8 form of the symmetric density Gram (gram_i8sym_kernel: exact int32
row sums of <a_i, a_j>, a = clamp(rint(H / 32), -127, 127), by
v_mfma_i32_16x16x64_i8; dal_gram_sym_residual_i8 adds the rest in closed
form), forced on small pools with ``gram_i8=True``:

 1. gram_accumulate alone adds, bit for bit, 2^18 sum_{taken pairs} <a_r, a_j>
    (NumPy int64 from the operand read back; padding and excluded rows 0) --
    the check that catches a wrong tile / lane map, swizzle, slice offset or
    fold, an idle half, a last row unit with one live super block;
 2. the density meets the two assertions of test_gpu_gram_hh._check_density,
    and its error against the split operand's fp64 row sums is no larger than
    the fp16 form's on the same pool;
 3. the bits do not depend on the grid, the column split, a skip range with a
    column offset, or a second stream running beside;
 4. the same on a pool whose a clamps (rows near +-e_1 among dense rows);
 5. at 70,000 x 128 the default rule picks the form.
Needs an MI355X: ``pytest -m gpu``."""
import numpy as np
import pytest

from oracle import dal_oracle as O
from test_gpu_gram_hh import E, _np, _split_rows
from test_gram_hh_algebra import takes
from test_gram_i8_algebra import quant

pytestmark = pytest.mark.gpu


def _pool(cuda, X, gram_i8):
    from dal.engine import PoolState

    return PoolState(X, excluded=E, device=cuda, gram="sym", gram_i8=gram_i8)


def _a_of(st):
    """a(H) [n_pad, d_pad] int64 of the split operand read back (KS 128: [slice][128 H | 128 L])."""
    sp = _np(st.gram_operand()).view(np.float16).astype(np.float64)
    a = np.zeros((st.n_pad, st.d_pad), dtype=np.int64)
    for s0 in range(0, st.d_pad, 128):
        a[:, s0:s0 + 128] = quant(sp[:, 2 * s0:2 * s0 + 128])
    return a


def _mfma_part(st, a, j_lo=0, j_hi=None, skip=(0, 0)):
    """2^18 sum <a_r, a_j> over the 256-column blocks [j_lo, j_hi) less ``skip``
    that each row's super block takes (sum_j <a_r, a_j> = <a_r, sum_j a_j>)."""
    nb = st.nb_active()
    j_hi = nb if j_hi is None else j_hi
    cb = a.reshape(-1, 256, st.d_pad).sum(axis=1)
    ref = np.zeros(st.n_pad, dtype=np.int64)
    for P in range(nb // 2):
        s = np.zeros(st.d_pad, dtype=np.int64)
        for J in range(j_lo, j_hi):
            if takes(P, J // 2) and not skip[0] <= J < skip[1]:
                s += cb[J]
        ref[P * 512:(P + 1) * 512] = a[P * 512:(P + 1) * 512] @ s
    return ref << 18


def _accumulate(st, cuda, **kw):
    import torch

    acc = torch.zeros(st.n_pad, dtype=torch.int64, device=cuda)
    st.gram_accumulate(acc, st.gram_operand(), st.n_pad, **kw)
    return _np(acc)


def _density_errors(st, X, n):
    """test_gpu_gram_hh._check_density's two assertions on ``st``; returns the
    error against the split operand's own fp64 row sums."""
    from dal import _lib

    got = _np(st.density())
    keep = np.ones(n, bool)
    keep[E] = False
    assert np.array_equal(np.isnan(got), ~keep)
    ut = _split_rows(st, n)
    d_split = ut @ ut[keep].sum(axis=0)
    e2 = np.abs(got[keep] - d_split[keep]).max()
    err = np.abs(got[keep] - O.density_canonical(X, E)[keep]).max()
    bound = _lib.load().dal_density_error_bound_sym_d(n - len(E), st.d_pad)
    print(f"{n} x {X.shape[1]} i8={st.gram_i8}: vs split operand {e2:.3g} (<= {1e-6 * (n - len(E)):.3g}), "
          f"vs canonical {err:.3g} (<= {bound:.3g})")
    assert e2 <= 1e-6 * (n - len(E)), e2
    assert err <= bound
    return e2


def _check_pool(cuda, X):
    n = X.shape[0]
    st = _pool(cuda, X, True)
    assert st.gram_i8 and st.d_pad % 128 == 0
    a = _a_of(st)
    assert not a[n:].any() and not a[E].any()
    got = _accumulate(st, cuda)
    ref = _mfma_part(st, a)
    assert np.any(ref != 0)
    assert np.array_equal(got, ref), np.flatnonzero(got != ref)[:8]
    e_i8 = _density_errors(st, X, n)
    e_f16 = _density_errors(_pool(cuda, X, False), X, n)
    assert e_i8 <= e_f16, (e_i8, e_f16)
    return st, a


@pytest.mark.parametrize("dist", ["uniform", "normal"])
@pytest.mark.parametrize("d", [100, 128, 256, 384])
@pytest.mark.parametrize("n", [700, 1300, 2700, 4300])
def test_i8_row_sums_exact_and_density_within_bound(cuda, n, d, dist):
    _check_pool(cuda, O.synthetic_pool(n, d, seed=7, dist=dist))


def test_i8_clamped_rows(cuda):
    """2,700 x 128: every third row within 1e-3 of +-e_1 (H = +-4096 there, so a
    clamps at +-127 and l' carries the 32 left over) among dense rows."""
    rng = np.random.default_rng(21)
    X = rng.standard_normal((2700, 128), dtype=np.float32)
    spike = np.arange(11, 2700, 3)
    X[spike] *= np.float32(1e-3)
    X[spike, 0] = np.where(rng.random(spike.size) < 0.5, -1.0, 1.0).astype(np.float32)
    st, a = _check_pool(cuda, X)
    assert np.abs(a[spike, 0]).min() == 127


@pytest.mark.parametrize("n,d", [(4300, 256), (2700, 128)])
def test_i8_bits_do_not_depend_on_the_launch(cuda, n, d):
    import torch

    st = _pool(cuda, O.synthetic_pool(n, d, seed=3), True)
    op = st.gram_operand()
    a = _a_of(st)
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
    # two streams at once, each with a counter slot of its own
    torch.cuda.synchronize()
    accs = [torch.zeros(st.n_pad, dtype=torch.int64, device=cuda) for _ in range(2)]
    for acc in accs:
        with torch.cuda.stream(torch.cuda.Stream(device=cuda)):
            for _ in range(3):
                st.gram_accumulate(acc, op, st.n_pad, grid_blocks=7)
    torch.cuda.synchronize()
    for acc in accs:
        assert np.array_equal(_np(acc), 3 * ref)
    # ... and the whole density: one call against the quarters
    whole = torch.zeros(st.n_pad, dtype=torch.int64, device=cuda)
    st.gram_accumulate(whole, op, st.n_pad)
    st.gram_residual(whole, op)
    assert np.array_equal(_np(whole), _np(st.density_fixed()))


@pytest.fixture(scope="module")
def pool70k():
    return O.synthetic_pool(70_000, 128, seed=14)


def test_default_rule_picks_i8_above_32_mb(cuda, pool70k):
    """70,000 x 128: the split operand (35.9 MB) is above the contiguous
    schedule's limit, so the pool takes the int8 form by itself; its density
    equals the forced form's summed over shuffled column quarters."""
    import torch

    st = _pool(cuda, pool70k, None)
    assert st.gram_i8 and st.n_pad * 2 * st.d_pad * 2 > 32 << 20
    assert not _pool(cuda, pool70k[:60_000], None).gram_i8  # 30.7 MB: the contiguous fp16 form
    forced = _pool(cuda, pool70k, True)
    op = forced.gram_operand()
    q = forced.n_pad // 512 // 4 * 512
    part = torch.zeros(forced.n_pad, dtype=torch.int64, device=cuda)
    for c0, c1 in ((2 * q, 3 * q), (0, q), (3 * q, forced.n_pad), (q, 2 * q)):
        forced.gram_accumulate(part, op[c0:], c1 - c0, col_row0=c0)
    forced.gram_residual(part, op)
    assert np.array_equal(_np(st.density_fixed()), _np(part))
    _density_errors(st, pool70k, 70_000)


def test_fp16_wide_form_stays_covered(cuda, pool70k):
    """70,000 x 128 with gram_i8=False: gram_csym_kernel<128, 8, 4>, the form
    every large KS-128 pool ran before the int8 one."""
    import torch

    st = _pool(cuda, pool70k, False)
    assert not st.gram_i8
    _density_errors(st, pool70k, 70_000)
    # its chains are the contiguous 4-wave form's: column quarters (each <= 32 MB) give the same bits
    op = st.gram_operand()
    q = st.n_pad // 512 // 4 * 512
    part = torch.zeros(st.n_pad, dtype=torch.int64, device=cuda)
    for c0, c1 in ((2 * q, 3 * q), (0, q), (3 * q, st.n_pad), (q, 2 * q)):
        st.gram_accumulate(part, op[c0:], c1 - c0, col_row0=c0)
    st.gram_residual(part, op)
    assert np.array_equal(_np(part), _np(st.density_fixed()))
