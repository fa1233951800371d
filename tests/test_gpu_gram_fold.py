"""The deferred fold of the integer Gram forms (round 15: gram_fp4sym_kernel
and gram_i8sym_kernel fold their row chains once per Cfg::FOLD_PAIRS pairs of a
row unit and when the rows change, instead of at the end of every pair).
Integer adds are exact, so nothing may change:

 1. for fp4 (36,000 x 256 and x 512) and int8 (70,000 x 128, gram_i8=True), at
    grids 1, 2, 5 and the device's, gram_accumulate adds, bit for bit, the
    NumPy int64 reference 2^18 sum_{taken pairs} <a_r, a_j> of
    test_gpu_gram_fp4.py / test_gpu_gram_i8.py;
 2. the same bits from the call split into shuffled column quarters, and from a
    call with a column offset and a skip range plus the two ranges it left out;
 3. crafted operands handed to the C entry points drive the chains to their
    cap: every code +12 (fp4; rows of -12 against columns of +12 for the other
    sign) or every byte +127, -127 against +127, and -128 (int8), 16,384 rows,
    at a one-block grid -- where a unit holds 16 pairs, so every chain runs its
    FOLD_PAIRS pairs at the largest magnitude the bound allows: fp4 chain
    elements of 7 x 589,824 and a lane's fp32 sum of four of 16,515,072 < 2^24,
    int8 row sums of 3 x 2^29 < 2^31 -- and at the device's grid.  The row sums
    must equal the closed-form integers.
The launches here are walked on the CPU by tests/test_gram_fold_schedule.py,
which asserts that they meet every fold trigger.
Needs an MI355X: ``pytest -m gpu``."""
import numpy as np
import pytest

from oracle import dal_oracle as O
from test_gpu_gram_hh import E, _np
from test_gpu_gram_fp4 import _a4_of
from test_gpu_gram_i8 import _a_of, _accumulate, _mfma_part
from test_gram_fold_schedule import CRAFTED, GRIDS, POOLS, column_calls
from test_gram_hh_algebra import takes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=POOLS, ids=lambda p: f"{p[0]}-{p[1]}x{p[2]}")
def pool(request, cuda):
    """(pool state, a [n_pad, d_pad] int64, the reference bits): built once per form and shape."""
    from dal.engine import PoolState

    form, n, d = request.param
    kw = {"gram_fp4": True} if form == "fp4" else {"gram_i8": True}
    st = PoolState(O.synthetic_pool(n, d, seed=15), excluded=E, device=cuda, gram="sym", **kw)
    assert st.gram_fp4 == (form == "fp4") and st.gram_i8 == (form == "i8") and st.d_pad == d
    a = _a4_of(st) if form == "fp4" else _a_of(st)
    ref = _mfma_part(st, a)
    assert np.any(ref != 0)
    ref.setflags(write=False)
    return st, a, ref


def test_bits_at_every_grid(cuda, pool):
    st, _, ref = pool
    for grid in GRIDS:
        got = _accumulate(st, cuda, grid_blocks=grid)
        assert np.array_equal(got, ref), (grid, np.flatnonzero(got != ref)[:8])


def test_bits_of_column_quarters_and_a_skip_range(cuda, pool):
    import torch

    st, a, ref = pool
    op = st.gram_operand()
    quarters, skipped = column_calls(st.n_pad)
    part = torch.zeros(st.n_pad, dtype=torch.int64, device=cuda)
    for c0, c1, _ in quarters:
        st.gram_accumulate(part, op[c0:], c1 - c0, col_row0=c0)
    assert np.array_equal(_np(part), ref)
    part.zero_()
    (c0, c1, skip), rest = skipped[0], skipped[1:]
    st.gram_accumulate(part, op[c0:], c1 - c0, col_row0=c0, skip=skip)
    assert np.array_equal(_np(part), _mfma_part(st, a, c0 // 256, None, (skip[0] // 256, skip[1] // 256)))
    for c0, c1, _ in rest:
        st.gram_accumulate(part, op[c0:], c1 - c0, col_row0=c0)
    assert np.array_equal(_np(part), ref)


# (rows' value, columns' value): fp4 as e2m1 codes of +-12 in both nibbles, int8 as bytes
CRAFTED_VALUES = {"fp4": [(12, 12), (-12, 12)], "i8": [(127, 127), (-127, 127), (-128, -128)]}


@pytest.mark.parametrize("form,rows,d,grids", CRAFTED, ids=lambda v: str(v).replace(" ", ""))
def test_chains_at_their_cap(cuda, form, rows, d, grids):
    import torch

    from dal import _lib
    from dal.engine import _ptr, _stream

    nb = rows // 256
    # the column blocks every super block takes: a row of P sums taken * 256 columns x d features of one product
    taken = np.array([sum(takes(P, J // 2) for J in range(nb)) for P in range(nb // 2)], dtype=np.int64)
    assert taken.max() >= 16  # (a unit of the one-block grid's two column chunks holds its cap of pairs twice over)
    for rv, cv in CRAFTED_VALUES[form]:
        if form == "fp4":
            byte = {12: 0x77, -12: 0xFF}
            r_op = torch.full((rows, d // 2), byte[rv], dtype=torch.uint8, device=cuda)
            c_op = torch.full((rows, d // 2), byte[cv], dtype=torch.uint8, device=cuda)
            entry = "dal_gram_rowsum_sym_fp4_skip"
        else:
            r_op = torch.full((rows, d), rv, dtype=torch.int8, device=cuda)
            c_op = torch.full((rows, d), cv, dtype=torch.int8, device=cuda)
            entry = "dal_gram_rowsum_sym_i8_skip"
        want = np.repeat(taken * 256 * d * rv * cv, 512) << 18
        for grid in grids:
            acc = torch.zeros(rows, dtype=torch.int64, device=cuda)
            _lib.call(entry, _ptr(r_op), 0, nb, _ptr(c_op), 0, 0, nb, 0, 0, nb, d, _ptr(acc), grid, _stream(cuda))
            got = _np(acc)
            assert np.array_equal(got, want), (rv, cv, grid, np.flatnonzero(got != want)[:8])
