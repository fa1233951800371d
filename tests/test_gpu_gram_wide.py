"""The wide form of gram_csym_kernel (KS 128, round-robin chunk schedule: 8
waves hold four super blocks of one parity, 256 rows per wave, and walk the
64-feature sub-slices of every slice) at the smallest shapes whose column
operand exceeds the 32 MB limit of the contiguous 4-wave form:

  70,000 x 128   137 super blocks (137 % 8 == 1: the last row unit holds one
                 live super block), 2 sub-slices
  36,000 x 256    71 super blocks, 4 sub-slices
  24,000 x 384    47 super blocks; d_pad is 512 (four slices): 8 sub-slices

Density: the assertions and tolerances of test_gpu_gram_hh._check_density
(within 1e-6 N of the split operand's fp64 row sums, within
dal_density_error_bound_sym_d of the canonical density; rows 0-9 excluded), on
uniform and normal data.  Bits: the int64 accumulator must not depend on the
grid (0, 1, 7, 333), on the columns being split into four shuffled quarter
ranges (each <= 32 MB: they run the contiguous 4-wave form, so this compares
the two KS-128 forms' chains -- one per (row, pair, 64-feature half), each
rounded on its own), on calls back to back or on a second call in flight on
another stream.  A two- and a three-rank emulated exchange_density at 70,000 x
128 (the other ranks' columns in one launch with the own columns skipped: the
skip range at four super blocks per row unit) must give the single-GPU bits.
Needs an MI355X: ``pytest -m gpu``."""
import numpy as np
import pytest

from oracle import dal_oracle as O
from test_gpu_gram_hh import E, _check_density, _np

pytestmark = pytest.mark.gpu

SHAPES = [(70_000, 128), (36_000, 256), (24_000, 384)]


@pytest.mark.parametrize("dist", ["uniform", "normal"])
@pytest.mark.parametrize("n,d", SHAPES)
def test_wide_density_within_bound(cuda, n, d, dist):
    st = _check_density(cuda, n, d, dist, seed=31)
    assert st.d_pad % 128 == 0 and st.n_pad * 2 * st.d_pad * 2 > 32 << 20
    if n == 70_000:  # the last row units: one live super block, and none
        assert st.n_pad // 512 % 8 == 1


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def pool(request, cuda):
    """A pool and its accumulator bits at the default grid (computed once per shape, read only)."""
    import torch
    from dal.engine import PoolState

    n, d = request.param
    X = O.synthetic_pool(n, d, seed=3)
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


def test_wide_bits_across_grids(cuda, pool):
    st, op, want = pool
    for grid in (0, 1, 7, 333):
        assert np.array_equal(_full(st, op, cuda, grid_blocks=grid), want), grid


def test_wide_bits_against_contiguous_form_on_column_quarters(cuda, pool):
    """Four quarter ranges in shuffled order, each below the contiguous limit:
    the 4-wave form, one slice per launch, must define the wide form's chains."""
    import torch

    st, op, want = pool
    q = st.n_pad // 512 // 4 * 512
    assert (st.n_pad - 3 * q) * 2 * st.d_pad * 2 <= 32 << 20
    part = torch.zeros(st.n_pad, dtype=torch.int64, device=cuda)
    for c0, c1 in ((2 * q, 3 * q), (0, q), (3 * q, st.n_pad), (q, 2 * q)):
        st.gram_accumulate(part, op[c0:], c1 - c0, col_row0=c0)
    st.gram_residual(part, op)
    assert np.array_equal(_np(part), want)


def test_wide_bits_back_to_back_calls(cuda, pool):
    import torch

    st, op, want = pool
    accs = [torch.zeros(st.n_pad, dtype=torch.int64, device=cuda) for _ in range(2)]
    for acc in accs:
        st.gram_accumulate(acc, op, st.n_pad)
    for acc in accs:
        st.gram_residual(acc, op)
        assert np.array_equal(_np(acc), want)


def test_wide_bits_two_streams_at_once(cuda, pool):
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


class _GatheredComm:
    """Single-process stand-in for the communicator: the all-gather returns
    the precomputed gathered operand; the density exchange uses nothing else."""

    overlaps = True  # the RCCL code path: own-shard Gram queued before the collectives

    def __init__(self, u_full):
        self.u_full = u_full

    def all_gather_start(self, t):
        return self.u_full, "work"

    def wait(self, work):
        assert work in ("work", None)


@pytest.mark.parametrize("world", [2, 3])
def test_wide_sharded_exchange_density_bits(cuda, world):
    """Every rank's rows against its own columns, then against all columns with
    its own skipped (above 32 MB: the wide form with a skip range), give the
    single-GPU density bits."""
    import torch
    from dal import parallel
    from dal.engine import PoolState

    n, d = 70_000, 128
    X = O.synthetic_pool(n, d, seed=3)
    sels = []
    for r in range(world):
        lo, hi, _ = parallel.shard_range(n, world, r)
        sels.append(parallel.ShardedSelector(X[lo:hi], n, r, world, excluded=E, device=cuda, gram="sym"))
    u_full = torch.cat([s.prep()[0] for s in sels])
    assert u_full.shape[0] * u_full.shape[1] * u_full.element_size() > 32 << 20
    for s in sels:
        s.exchange_density(_GatheredComm(u_full), s.prep()[0])
    total = torch.cat([s._density for s in sels])
    st = PoolState(X, excluded=E, device=cuda, gram="sym")
    assert torch.equal(total[:n], st.density_fixed()[:n])
