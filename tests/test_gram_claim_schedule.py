"""The symmetric Gram's dynamic unit walk (GramClaimCursor, csrc/
gram_schedule.hpp) on the CPU, no GPU needed.

gram_csym_kernel's blocks enter unit g and take every later unit (feature
slice x column chunk x row unit) from a counter the launch's blocks share.
tests/host/gram_claim_driver.cpp (host C++ compiler, no HIP) runs G simulated
blocks through the kernel's pair loop, one pair per step, under three orders
of the claims -- the blocks step in turn, one block runs to its end first and
so claims everything, a seeded random interleaving -- plus the fixed deal (no
counter; also the contiguous form, which walks through the same cursor) and a
counter that starts past the end.  Sweep: ns_active 1..9, shard rows with and
without a padding super block, whole and half column ranges, G in {1, 3, 5, 7},
1..4 requested chunks, 1..3 slices, one and two super blocks per row unit, no
skip range and one inside the columns.  Checked:
 (a) every (slice, live unskipped pair its row super block takes) is visited
     exactly once, nothing else -- against sb_takes restated over unordered
     pairs;
 (b) the announced next pair (row unit, slice, column block) is the one the
     advance yields, "rows change" exactly when row unit or slice differ;
 (c) a unit's rows are flushed before another unit's sums enter rowacc, and
     the last pair flushes;
 (d) no empty unit is handed over, and a claimed index at or beyond the total
     ends the walk whatever the counter holds (a poisoned counter leaves every
     block the one unit it entered by itself).
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "distributed-active-learning_amd", "csrc")
SRC = os.path.join(REPO, "tests", "host", "gram_claim_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gram_claim") / "driver")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I" + CSRC, SRC, "-o", exe], check=True)
    return exe


def test_sweep_every_slice_pair_once_under_every_claim_order(driver):
    out = subprocess.run([driver, "sweep"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert out.stdout.split() == ["cases", "282656", "failures", "0"], out.stdout[-4000:]
