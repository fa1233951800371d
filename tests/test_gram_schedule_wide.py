"""The symmetric Gram's pair schedule at four super blocks per row unit (the
wide form of gram_csym_kernel; GramSchedule<4> / GramCursor<4> /
GramClaimCursor<4> in csrc/gram_schedule.hpp) walked on the CPU, no GPU needed.

tests/host/gram_schedule_wide_driver.cpp (host C++ compiler, no HIP) checks
for HV = 4 what test_gram_schedule.py and test_gram_claim_schedule.py check
for HV <= 2.  Sweep: ns_active 1..17 (every n_srb % 8, with and without a
padding super block), shard rows from even and odd super blocks, whole and
half column ranges, no skip range / the shard's own columns / one inside the
columns, G in {1, 3, 5, 7}, 1..4 requested chunks, 1..3 slices (2, 4, 6
sub-slices: the wide form's units count sub-slices slowest).  Checked:
 (a) a row unit ru is the super blocks srow0 + 8 (ru >> 1) + (ru & 1) + 2 h,
     h = 0..3, n_ru = 2 ceil(n_srb / 8), every super block in exactly one;
 (b) every (sub-slice, live unskipped pair its row super block takes) is
     visited exactly once and nothing else, against sb_takes restated over
     unordered pairs -- for the fixed deal (GramCursor) and, through
     GramClaimCursor, under three orders of the claims (in turn, one block
     takes all, a seeded random interleaving), the fixed deal and a counter
     that starts past the end (every block then walks its own first unit only);
 (c) every visited pair has a part that acts on it; the announced next pair is
     the one the advance yields; "rows change" exactly when row unit or
     sub-slice differ; a unit's rows are flushed before another's enter;
 (d) the launch's chunks tile the columns, its units count every sub-slice, and
     the contiguous form is refused.
The fixed deal's pairs are also compared here with the numpy takes() of
tests/test_gram_balance.py, and the driver runs once more under ASan + UBSan
(host code with its own main, nothing preloaded).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_gram_balance import takes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "distributed-active-learning_amd", "csrc")
SRC = os.path.join(REPO, "tests", "host", "gram_schedule_wide_driver.cpp")


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gram_schedule_wide") / "driver")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-Wall", "-I" + CSRC, SRC, "-o", exe], check=True)
    return exe


def test_sweep_every_sub_slice_pair_once(driver):
    out = subprocess.run([driver, "sweep"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert out.stdout.split() == ["cases", "1566720", "failures", "0"], out.stdout[-4000:]


# (ns, srow0, n_srb, j_lo, j_hi, skip_lo, skip_hi, G, requested chunks)
WALKS = [
    (17, 0, 17, 0, 34, 0, 0, 5, 3),     # whole pool, the last row units hold one live super block
    (17, 0, 18, 0, 34, 0, 0, 7, 4),     # ... and a padding super block
    (13, 3, 9, 2, 26, 6, 24, 3, 2),     # a shard's rows from an odd super block, its own columns skipped
    (9, 1, 8, 3, 18, 4, 6, 1, 1),       # one block, a skip range inside the columns
    (5, 0, 5, 0, 10, 0, 0, 7, 2),       # fewer super blocks than one pair of row units holds
]


@pytest.mark.parametrize("case", WALKS)
def test_walk_matches_numpy_rule(driver, case):
    ns, srow0, n_srb, j_lo, j_hi, skip_lo, skip_hi = case[:7]
    out = subprocess.run([driver, "walk"] + [str(v) for v in case], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    got = np.zeros((ns + 10, 2 * ns), dtype=np.int32)
    for line in out.stdout.splitlines():
        P, J = (int(v) for v in line.split())
        got[P, J] += 1
    want = np.zeros_like(got)
    rows = np.arange(srow0, min(srow0 + n_srb, ns))
    cols = np.arange(j_lo, j_hi)
    want[rows[:, None], cols[None, :]] = takes(rows, cols, skip_lo, skip_hi)
    assert want.sum() > 0
    assert np.array_equal(got, want)


def test_sweep_under_asan_ubsan(tmp_path):
    """The same sweep with the driver (and the header it walks) built with
    -fsanitize=address,undefined: a stand-alone host program, no preload."""
    # ROCm's clang links the sanitizer runtimes statically (as scripts/asan/build.sh relies on)
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    cxx = clang if os.path.exists(clang) else _cxx()
    exe = str(tmp_path / "driver_san")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I" + CSRC, SRC, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr + build.stdout:
        pytest.skip("host compiler without the sanitizer runtimes")
    assert build.returncode == 0, build.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0:exitcode=86",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe, "sweep"], capture_output=True, text=True, env=env)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.split() == ["cases", "1566720", "failures", "0"], out.stdout[-4000:]
