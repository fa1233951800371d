"""The symmetric Gram's pair schedule (csrc/gram_schedule.hpp) walked on the
CPU, no GPU needed.

gram_csym_kernel and its launcher share one integer-only header that decides
which block multiplies which (512-row super block P, 256-column block J) pair,
in what order, and when a row unit's sums are flushed.  tests/host/
gram_schedule_driver.cpp (host C++ compiler, no HIP) walks every block of a
launch with the header's cursor exactly as the kernel's pair loop does and
checks, over a sweep of the smallest shapes at which each branch can go wrong
(ns_active 1..9, every srow0 / n_srb including a padding super block, column
ranges, three skip ranges, G in {1, 3, 5, 7}; contiguous form, and the chunk
form with one and two super blocks per row unit at 1..4 requested chunks):
 (a) all blocks together visit every live, in-range, unskipped pair its row
     super block takes exactly once, and nothing else (a half acts only on
     pairs its own super block takes);
 (b) the pair the cursor announces is the pair it yields after the advance,
     and "rows change" is true exactly when the row unit differs;
 (c) pairs_skip equals the brute-force count;
 (d) the launch's (chunk_j, n_chunks) tile the column range exactly.
The driver's expected set restates the rule in its unordered-pair form; for a
few cases the visited pairs are also compared here with the numpy takes() of
tests/test_gram_balance.py.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_gram_balance import takes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "distributed-active-learning_amd", "csrc")
SRC = os.path.join(REPO, "tests", "host", "gram_schedule_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gram_schedule") / "driver")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall","-I" + CSRC, SRC, "-o", exe], check=True)
    return exe


def test_sweep_every_pair_once(driver):
    out = subprocess.run([driver, "sweep"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert out.stdout.split() == ["cases", "491508", "failures", "0"], out.stdout[-4000:]


# (ns, srow0, n_srb, j_lo, j_hi, skip_lo, skip_hi, G, contig, hv, requested chunks)
WALKS = [
    (9, 0, 9, 0, 18, 0, 0, 5, 1, 1, 1),      # whole pool, contiguous
    (9, 2, 5, 3, 16, 4, 14, 3, 1, 1, 1),     # a shard's rows, its own columns skipped
    (9, 0, 10, 0, 18, 0, 0, 7, 0, 1, 4),     # chunked, a padding super block
    (9, 0, 9, 0, 18, 0, 0, 3, 0, 2, 3),      # two super blocks per unit, odd unit count
    (7, 1, 7, 3, 14, 4, 6, 5, 0, 2, 2),      # ... rows past the pool, a skip range inside the columns
]


@pytest.mark.parametrize("case", WALKS)
def test_walk_matches_numpy_rule(driver, case):
    ns, srow0, n_srb, j_lo, j_hi, skip_lo, skip_hi = case[:7]
    out = subprocess.run([driver, "walk"] + [str(v) for v in case], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    got = np.zeros((ns + 2, 2 * ns), dtype=np.int32)
    for line in out.stdout.splitlines():
        P, J = (int(v) for v in line.split())
        got[P, J] += 1
    want = np.zeros_like(got)
    rows = np.arange(srow0, min(srow0 + n_srb, ns))
    cols = np.arange(j_lo, j_hi)
    want[rows[:, None], cols[None, :]] = takes(rows, cols, skip_lo, skip_hi)
    assert want.sum() > 0
    assert np.array_equal(got, want)


# DAL_GRAM_MIN_CHUNKS(_SMALL) and the grids of a 256-CU device: the chooser's
# values at the benchmark configurations, whole pool, no skip range
# (G0, hv, min_chunks, super blocks) -> (chunks, columns per chunk)
PINNED = {
    "config2 100k x 64": ((1024, 1, 2, 196), (5, 79)),
    "config3 284807 x 30": ((1280, 1, 16, 557), (16, 70)),
    "config4 2M x 256": ((256, 2, 16, 3907), (16, 489)),
    "500k x 256": ((256, 2, 16, 977), (16, 123)),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_chooser_pinned(driver, name):
    args, want = PINNED[name]
    out = subprocess.run([driver, "choose"] + [str(v) for v in args], capture_output=True, text=True, check=True)
    assert tuple(int(v) for v in out.stdout.split()) == want
