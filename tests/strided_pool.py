"""Test-side helper (not a test): a pool laid out the way a caller of the C ABI
may hand it over -- row stride ldx > d, first row off the allocation's 16-byte
alignment -- with poison in every element that is not a logical entry.

include/dal.h: "Pool rows are fp32, row-major with leading dimension ldx".
A kernel that indexes with d where it should use ldx, or that reads a padding
column as a feature, then computes on NaN (fp32, fp64) or on the bf16 NaN
0x7FC0 and misses the reference of the logical matrix; a kernel that writes
through its const input changes the buffer, which assert_unchanged compares
byte for byte with what was uploaded.

forest_tiling restates the staging rule of the row-major forest kernels
(csrc/forest_shared.hpp, forest_tiling; csrc/forest.hip and
csrc/forest_multi.hip, ``vec4``) so that a case can assert which staging
branch and which rows-per-block it reaches.  A drift between this restatement
and the code costs coverage (a case asserts a branch the code no longer takes
there), not correctness: the outputs are compared with the reference either
way.
"""
from collections import namedtuple

import numpy as np

TAIL = 64  # poisoned elements after the last row (at least 64)
BF16_NAN = 0x7FC0


def _poison(dtype, poison):
    if dtype == np.uint16:  # bf16 bits
        return np.uint16(BF16_NAN if poison is None or poison != poison else poison)
    return dtype.type(np.nan if poison is None else poison)


def layout(X, ldx, offset_elems, poison=float("nan")):
    """The flat host buffer of strided(): offset_elems + (n - 1) * ldx + d +
    TAIL elements of X's dtype, X[i][f] at offset_elems + i * ldx + f, poison
    everywhere else."""
    X = np.ascontiguousarray(X)
    if X.dtype not in (np.float32, np.float64, np.uint16):
        raise TypeError(f"strided: fp32, fp64 or bf16 bits (uint16), not {X.dtype}")
    n, d = X.shape
    if n < 1 or ldx < d or offset_elems < 0:
        raise ValueError("strided: n >= 1, ldx >= d and offset_elems >= 0")
    total = offset_elems + (n - 1) * ldx + d + TAIL
    host = np.full(total, _poison(X.dtype, poison), dtype=X.dtype)
    rows = np.lib.stride_tricks.as_strided(host[offset_elems:], shape=(n, d),
                                           strides=(ldx * X.itemsize, X.itemsize))
    rows[...] = X
    return host


def strided(X, ldx, offset_elems, device, poison=float("nan")):
    """The logical [n, d] matrix X (fp32, fp64, or bf16 bits as uint16) as a
    device tensor view of row stride ``ldx`` whose data_ptr() is element
    ``offset_elems`` of one flat buffer of offset_elems + (n - 1) * ldx + d +
    TAIL elements.  Every element that is no logical entry is ``poison`` (NaN;
    0x7FC0 for bf16): the lead-in, the ldx - d padding columns of every row
    and the tail.  bf16 bits travel as int16 (the engine's own choice for
    16-bit words).  The view carries the buffer and its uploaded bytes for
    assert_unchanged."""
    import torch

    X = np.ascontiguousarray(X)
    n, d = X.shape
    ldx, offset_elems = int(ldx), int(offset_elems)
    host = layout(X, ldx, offset_elems, poison)
    buf = torch.from_numpy(host.view(np.int16) if X.dtype == np.uint16 else host).to(device)
    # the allocator hands out 256-byte aligned blocks: offset_elems alone decides the view's alignment
    assert buf.data_ptr() % 256 == 0
    view = buf.as_strided((n, d), (ldx, 1), offset_elems)
    assert view.data_ptr() == buf.data_ptr() + offset_elems * X.itemsize and view.stride() == (ldx, 1)
    view.pool_buffer = buf
    view.pool_bytes = host.tobytes()
    view.ldx = ldx
    return view


def assert_unchanged(view):
    """The whole flat buffer behind a strided() view -- rows, padding, lead-in
    and tail -- holds the bytes that were uploaded (inputs are const)."""
    import torch

    torch.cuda.synchronize(view.device)
    now = view.pool_buffer.cpu().numpy().tobytes()
    assert now == view.pool_bytes, "a kernel wrote through its const pool (or its padding)"


def contiguous(X, device):
    """X on the device, contiguous (ldx = d), 256-byte aligned: the layout
    every other test of the suite passes."""
    import torch

    X = np.array(X)  # (a copy: torch does not take read-only arrays)
    t = torch.from_numpy(X.view(np.int16) if X.dtype == np.uint16 else X).to(device)
    assert t.data_ptr() % 256 == 0
    return t


# ---------------------------------------------------------------- staging --
Tiling = namedtuple("Tiling", "staging R dma vec4 x_lds")


def forest_tiling(d, ldx, ptr, n_trees, threads=256):
    """csrc/forest_shared.hpp forest_tiling() and the launchers' ``vec4``
    (csrc/forest.hip forest_score_launch, csrc/forest_multi.hip multi_launch),
    restated: which staging the row-major forest kernels take for a pool at
    address ``ptr`` and how many rows a block holds.

    staging  "dma"     LDS-DMA, persistent grid (d >= 128 and 16-byte rows)
             "vec4"    16-byte loads, d + 4 words per LDS row
             "scalar"  4-byte loads, d + 1 words per LDS row
             "none"    rows read from global memory (x_lds false)
    """
    aligned = d % 4 == 0 and ldx % 4 == 0 and ptr % 16 == 0
    dma = d >= 128 and aligned
    R, x_lds = 256, True
    tile_cap = 33280 if dma else 16640 * (threads // 256)
    while R > 16 and R * (d + 1) * 4 > tile_cap:
        R >>= 1
    if R * (d + 1) * 4 > 65536:
        x_lds, dma, R = False, False, 256
    tpr_min = 2 if n_trees >= 64 else 1  # DAL_FOREST_TPR
    if x_lds:
        while R > 1 and threads // R < tpr_min:
            R >>= 1
    staging = "none" if not x_lds else "dma" if dma else "vec4" if aligned else "scalar"
    return Tiling(staging, R, dma, aligned, x_lds)


def dma_pieces(d):
    """(pieces, live lanes of the last piece) of one row's LDS-DMA staging:
    one 64-lane x 16-byte instruction per 1 KiB of the row (csrc/forest.hip,
    forest_score_kernel)."""
    row_bytes = 4 * d
    pieces = (row_bytes + 1023) // 1024
    return pieces, (row_bytes - (pieces - 1) * 1024) // 16
