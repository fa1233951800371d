"""The wide form's pair loop (gram_csym_kernel<128, 8, 4>, round 12: the
look-ahead of waves 4-7 runs behind their first column tiles instead of
behind the barrier) at the smallest wide-form shapes, 70,000 x 128 and 36,000
x 256, on uniform and normal data, rows 0-9 excluded.

Bits: the int64 accumulator of the wide form must equal the accumulator built
from shuffled column-quarter calls, which run the 4-wave contiguous form (one
chain per (row, pair, 64-feature half), each rounded on its own) -- for
grid_blocks in (1, 2, 5, 0), for a call with a nonzero col_row0 and a skip
range inside its columns, and for one whose skip range leaves a single column
block (every unit then holds one pair, most blocks a single pair: the
look-ahead finds no next pair, or a claim past the end, at its first call).
The launches are those tests/test_gram_pipe_schedule.py walks on the CPU.
Density: the assertions and tolerances of test_gpu_gram_hh._check_density.
Needs an MI355X: ``pytest -m gpu``."""
import numpy as np
import pytest

from oracle import dal_oracle as O
from test_gpu_gram_hh import E, _check_density, _np
from test_gram_pipe_schedule import COL_ROW0, GRIDS, SHAPES, SKIP_INSIDE

pytestmark = pytest.mark.gpu

LIMIT = 32 << 20  # column operands above it take the wide form, up to it the contiguous 4-wave form


@pytest.mark.parametrize("dist", ["uniform", "normal"])
@pytest.mark.parametrize("n,d", SHAPES)
def test_pipe_density_within_bound(cuda, n, d, dist):
    st = _check_density(cuda, n, d, dist, seed=41)
    assert st.d_pad % 128 == 0 and st.n_pad * 2 * st.d_pad * 2 > LIMIT


def _contig(st, op, cuda, ranges, skip=None):
    """The accumulator of the column ranges (rows, multiples of 512), each small
    enough for the contiguous 4-wave form, in the order given."""
    import torch

    q = LIMIT // (2 * st.d_pad * 2) // 512 * 512
    part = torch.zeros(st.n_pad, dtype=torch.int64, device=cuda)
    for c0, c1 in ranges:
        for a in range(c0, c1, q):
            b = min(a + q, c1)
            assert (b - a) * 2 * st.d_pad * 2 <= LIMIT
            st.gram_accumulate(part, op[a:], b - a, col_row0=a, skip=skip)
    return _np(part)


def _wide(st, op, cuda, c0=0, **kw):
    import torch

    assert (st.n_pad - c0) * 2 * st.d_pad * 2 > LIMIT
    acc = torch.zeros(st.n_pad, dtype=torch.int64, device=cuda)
    st.gram_accumulate(acc, op[c0:], st.n_pad - c0, col_row0=c0, **kw)
    return _np(acc)


@pytest.fixture(scope="module", params=[(s, dist) for s in SHAPES for dist in ("uniform", "normal")],
                ids=lambda p: f"{p[0][0]}x{p[0][1]}-{p[1]}")
def pool(request, cuda):
    """A pool and its accumulator from four shuffled column quarters (the
    4-wave contiguous form; computed once per pool, read only)."""
    from dal.engine import PoolState

    (n, d), dist = request.param
    X = O.synthetic_pool(n, d, seed=5, dist=dist)
    st = PoolState(X, excluded=E, device=cuda, gram="sym")
    op = st.gram_operand()
    q = st.n_pad // 512 // 4 * 512
    want = _contig(st, op, cuda, ((2 * q, 3 * q), (0, q), (3 * q, st.n_pad), (q, 2 * q)))
    assert np.any(want != 0)
    want.setflags(write=False)
    return st, op, want


def test_pipe_bits_against_contiguous_quarters_across_grids(cuda, pool):
    st, op, want = pool
    for grid in GRIDS:
        assert np.array_equal(_wide(st, op, cuda, grid_blocks=grid), want), grid


def test_pipe_bits_with_skip_range_and_column_offset(cuda, pool):
    st, op, _ = pool
    s0, s1 = SKIP_INSIDE
    want = _contig(st, op, cuda, ((s1, st.n_pad), (COL_ROW0, s0)))
    assert np.any(want != 0)
    assert np.array_equal(_wide(st, op, cuda, c0=COL_ROW0, skip=SKIP_INSIDE), want)


def test_pipe_bits_with_one_column_block_left(cuda, pool):
    st, op, _ = pool
    want = _contig(st, op, cuda, ((COL_ROW0, COL_ROW0 + 512),), skip=(COL_ROW0 + 256, COL_ROW0 + 512))
    assert np.any(want != 0)
    assert np.array_equal(_wide(st, op, cuda, c0=COL_ROW0, skip=(COL_ROW0 + 256, st.n_pad)), want)
