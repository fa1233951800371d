"""The H.H symmetric Gram (gram_csym_kernel: one fp16 MFMA product per feature
pair) with the closed-form remainder <L_r, S~> + <H_r, S^L + CH_B> of
dal_gram_sym_residual, at the smallest shapes where either can go wrong: both
orientation parities and the diagonal (2, 3 and 6 super blocks), padding rows,
KS 32 / 64 / 128 in one, two and three slices, d_pad != d, signed data, the
fused, staged and global residual forms and the 8-wave round-robin form.  The
assertions and tolerances are those of test_gram_density_within_bound.
Needs an MI355X: ``pytest -m gpu``."""
import numpy as np
import pytest

from oracle import dal_oracle as O

pytestmark = pytest.mark.gpu

E = list(range(10))


def _np(t):
    return t.detach().cpu().numpy()


def _split_rows(st, n):
    """u~ = (H + L) 2^-12 of the operand read back from the device, fp64."""
    sp = _np(st.gram_operand()).view(np.float16).astype(np.float64)
    ks = 32 if st.d_pad == 32 else (128 if st.d_pad % 128 == 0 else 64)
    ut = np.zeros((st.n_pad, st.d_pad))
    for s0 in range(0, st.d_pad, ks):
        ut[:, s0:s0 + ks] = (sp[:, 2 * s0:2 * s0 + ks] + sp[:, 2 * s0 + ks:2 * s0 + 2 * ks]) * 2.0**-12
    return ut[:n]


def _check_density(cuda, n, d, dist, seed):
    from dal import _lib
    from dal.engine import PoolState

    X = O.synthetic_pool(n, d, seed=seed, dist=dist)
    st = PoolState(X, excluded=E, device=cuda, gram="sym")
    got = _np(st.density())
    keep = np.ones(n, bool)
    keep[E] = False
    assert np.array_equal(np.isnan(got), ~keep)
    # against the split operand's own fp64 row sums only the MFMA accumulation error remains
    ut = _split_rows(st, n)
    d_split = ut @ ut[keep].sum(axis=0)  # separable: no N x N matrix
    e2 = np.abs(got[keep] - d_split[keep]).max()
    ref = O.density_canonical(X, E)
    err = np.abs(got[keep] - ref[keep]).max()
    bound = _lib.load().dal_density_error_bound_sym_d(n - len(E), st.d_pad)
    print(f"{n} x {d} {dist}: vs split operand {e2:.3g} (<= {1e-6 * (n - len(E)):.3g}), "
          f"vs canonical {err:.3g} (<= {bound:.3g})")
    assert e2 <= 1e-6 * (n - len(E)), e2
    assert err <= bound
    return st


@pytest.mark.parametrize("dist", ["uniform", "normal"])
@pytest.mark.parametrize("d", [30, 64, 96, 256, 384])
@pytest.mark.parametrize("n", [700, 1300, 2700])
def test_hh_gram_density_within_bound(cuda, n, d, dist):
    _check_density(cuda, n, d, dist, seed=7)


def test_hh_gram_global_residual_form(cuda):
    """d = 1,100 (d_pad 1,152 > 1,024): S~ and D_B read in place."""
    st = _check_density(cuda, 1300, 1100, "normal", seed=12)
    assert st.d_pad > 1024


def test_hh_gram_scan_residual_form(cuda):
    """2,700 x 96 (d_pad 128 > 64): the scan launch and the LDS-staged residual
    (d_pad <= 64 with few super blocks takes the fused form instead)."""
    st = _check_density(cuda, 2700, 96, "normal", seed=13)
    assert 64 < st.d_pad <= 1024


def test_hh_gram_round_robin_8_wave_form(cuda):
    """70,000 x 128: the column operand (35.9 MB) is above the 32 MB limit of
    the contiguous schedule, so gram_csym_kernel<128, 8> runs with round-robin
    column chunks, as at the flagship shape."""
    st = _check_density(cuda, 70_000, 128, "uniform", seed=14)
    assert st.n_pad * 2 * st.d_pad * 2 > 32 << 20


@pytest.mark.parametrize("n,d", [(5000, 256), (70_000, 128)])
def test_hh_gram_deterministic_across_grids_and_column_splits(cuda, n, d):
    """gram_accumulate + gram_residual: identical int64 bits for any grid and
    for the columns split into four ranges in shuffled order."""
    import torch
    from dal.engine import PoolState

    X = O.synthetic_pool(n, d, seed=3)
    st = PoolState(X, excluded=E, device=cuda, gram="sym")
    op = st.gram_operand()
    outs = []
    for grid in (0, 1, 7, 333):
        acc = torch.zeros(st.n_pad, dtype=torch.int64, device=cuda)
        st.gram_accumulate(acc, op, st.n_pad, grid_blocks=grid)
        st.gram_residual(acc, op)
        outs.append(_np(acc))
    assert np.any(outs[0] != 0)
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])
    q = st.n_pad // 512 // 4 * 512  # a quarter of the columns, in whole super blocks
    part = torch.zeros(st.n_pad, dtype=torch.int64, device=cuda)
    for c0, c1 in ((2 * q, 3 * q), (0, q), (3 * q, st.n_pad), (q, 2 * q)):
        st.gram_accumulate(part, op[c0:], c1 - c0, col_row0=c0)
    st.gram_residual(part, op)
    assert np.array_equal(_np(part), outs[0])
