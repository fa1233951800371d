"""The chunk form of gram_csym_kernel with one launch for every feature slice
and units claimed from a device counter, at the smallest shapes that reach
each path: two and three slices in the 8-wave form (column operand just above
the 32 MB limit of the contiguous schedule), KS 64 and KS 32 chunked.  The
assertions and tolerances are test_gpu_gram_hh._check_density's.  At 34,000 x
256 the int64 accumulator bits must not depend on the grid, on a column split
(which mixes the contiguous 4-wave and the chunked 8-wave forms), on earlier
launches having used the counter, or on a second launch running beside it on
another stream.  Needs an MI355X: ``pytest -m gpu``."""
import numpy as np
import pytest

from oracle import dal_oracle as O
from test_gpu_gram_hh import E, _check_density, _np

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,d,dist", [
    (34_000, 256, "uniform"),   # two slices, <128, 8> chunked
    (22_500, 384, "normal"),    # three slices
    (2_700, 64, "uniform"),     # KS 64 chunked
    (263_000, 30, "normal"),    # KS 32 chunked
])
def test_claimed_units_density_within_bound(cuda, n, d, dist):
    st = _check_density(cuda, n, d, dist, seed=21)
    if d != 64:  # (KS 64 takes column chunks at any size)
        assert st.n_pad * 2 * st.d_pad * 2 > 32 << 20


@pytest.fixture(scope="module")
def pool(cuda):
    """34,000 x 256 and its accumulator bits at the default grid (computed once, read only)."""
    import torch
    from dal.engine import PoolState

    X = O.synthetic_pool(34_000, 256, seed=3)
    st = PoolState(X, excluded=E, device=cuda, gram="sym")
    op = st.gram_operand()
    assert st.n_pad * 2 * st.d_pad * 2 > 32 << 20
    acc = torch.zeros(st.n_pad, dtype=torch.int64, device=cuda)
    st.gram_accumulate(acc, op, st.n_pad)
    st.gram_residual(acc, op)
    want = _np(acc)
    assert np.any(want != 0)
    want.setflags(write=False)
    return st, op, want


def _full(st, op, cuda, **kw):
    import torch

    acc = torch.zeros(st.n_pad, dtype=torch.int64, device=cuda)
    st.gram_accumulate(acc, op, st.n_pad, **kw)
    st.gram_residual(acc, op)
    return _np(acc)


@pytest.mark.parametrize("grid", [0, 1, 7, 333])
def test_bits_across_grids(cuda, pool, grid):
    st, op, want = pool
    assert np.array_equal(_full(st, op, cuda, grid_blocks=grid), want)


def test_bits_across_column_split(cuda, pool):
    """Four quarter ranges in shuffled order: each is below the contiguous
    limit and runs the 4-wave kernel, one slice per launch."""
    import torch

    st, op, want = pool
    q = st.n_pad // 512 // 4 * 512
    part = torch.zeros(st.n_pad, dtype=torch.int64, device=cuda)
    for c0, c1 in ((2 * q, 3 * q), (0, q), (3 * q, st.n_pad), (q, 2 * q)):
        st.gram_accumulate(part, op[c0:], c1 - c0, col_row0=c0)
    st.gram_residual(part, op)
    assert np.array_equal(_np(part), want)


def test_bits_back_to_back_calls(cuda, pool):
    """Three calls in stream order with no synchronisation between them: each
    finds the counter as the launch before it left it."""
    import torch

    st, op, want = pool
    accs = [torch.zeros(st.n_pad, dtype=torch.int64, device=cuda) for _ in range(3)]
    for acc in accs:
        st.gram_accumulate(acc, op, st.n_pad)
    for acc in accs:
        st.gram_residual(acc, op)
        assert np.array_equal(_np(acc), want)


def test_bits_two_streams_at_once(cuda, pool):
    """Two calls on two streams, in flight together, each into its own acc."""
    import torch

    st, op, want = pool
    accs = [torch.zeros(st.n_pad, dtype=torch.int64, device=cuda) for _ in range(2)]
    streams = [torch.cuda.Stream(device=cuda) for _ in range(2)]
    here = torch.cuda.current_stream(cuda)
    for s, acc in zip(streams, accs):
        s.wait_stream(here)
        with torch.cuda.stream(s):
            st.gram_accumulate(acc, op, st.n_pad)
    for s in streams:
        here.wait_stream(s)
    for acc in accs:
        st.gram_residual(acc, op)
        assert np.array_equal(_np(acc), want)


@pytest.mark.parametrize("grid", [1, 7])
def test_ks64_bits_with_claimed_units(cuda, grid):
    """2,700 x 64 has fewer units than the default grid has blocks (no unit
    is left to claim); a small grid makes its blocks claim."""
    from dal.engine import PoolState

    X = O.synthetic_pool(2_700, 64, seed=5)
    st = PoolState(X, excluded=E, device=cuda, gram="sym")
    op = st.gram_operand()
    assert np.array_equal(_full(st, op, cuda, grid_blocks=grid), _full(st, op, cuda))
