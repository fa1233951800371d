"""The wide form's pair loop as of round 12, walked on the CPU (no GPU needed):
tests/host/gram_pipe_driver.cpp (host C++ compiler, no HIP) runs every wave of
every block through gram_csym_kernel<128, 8, 4>'s loop with GramClaimCursor<4>
and lookahead_tiles() of csrc/gram_schedule.hpp -- the first half of a block's
waves runs the look-ahead (claim, peek(), the next stage's DMA issue) behind the
pair's barrier, their SIMD partners behind their first column tiles -- and
models the two ring buffers, the two claim words, the row accumulator and the
barriers.  Events of different waves are ordered only by a barrier between
them, so every check compares barrier counts.

Sweep (a thinned version of test_gram_schedule_wide.py's, under the fixed
deal and two orders of the claims).  Asserted:
 (a) GramSchedule<4>::first_r (closed form away from the diagonal since round
     12) returns the first column block some live part of the unit owns, for
     every (row unit, start, end), against the orientation rule restated;
 (b) every live taken (sub-slice, pair, wave of the half, tile group) chain is
     folded exactly once, before its rows' flush and after no later rows'
     first fold;
 (c) no buffer gets a DMA in the barrier interval of a read of it, and no read
     lies in the interval of its DMA (the wait before the barrier between
     confirms it landed); no claim word is written in the interval of a read
     of it, or read in the interval of its write;
 (d) all eight waves execute the same number of barriers, idle halves and
     the barriers inside claim_take() included; the two waves of every SIMD run
     their look-ahead at different places of the pair.
For the exact launches of tests/test_gpu_gram_pipe.py (shape, grid, column and
skip ranges, planned with plan_launch<4> as the launcher does) every kind of
pair boundary must occur at least once over the launches: same rows, a change
of row unit, a new sub-slice of the same rows, a one-pair unit, a half going
from acting to idle and back, a block with a single pair, and a first
look-ahead that finds the claim past the end.
The driver runs once more under ASan + UBSan (host code with its own main,
nothing preloaded)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "distributed-active-learning_amd", "csrc")
SRC = os.path.join(REPO, "tests", "host", "gram_pipe_driver.cpp")

# the launches of tests/test_gpu_gram_pipe.py
SHAPES = [(70_000, 128), (36_000, 256)]
GRIDS = (1, 2, 5, 0)              # grid_blocks (4-wave blocks: an 8-wave grid of 1, 1, 2 blocks, and the device's)
COL_ROW0 = 1024                   # first column row of the calls with a skip range
SKIP_INSIDE = (5120, 7168)        # ... a range inside the columns
CUS = 256                         # MI355X
MIN_CHUNKS = 16                   # DAL_GRAM_MIN_CHUNKS: column operands above 32 MB
SWEEP_CASES = "35640"


def _launches():
    """(ns, srow0, n_srb, j_lo, j_hi, skip_lo, skip_hi, G0, min_chunks, sub-slices) of every wide launch."""
    out = []
    for n, d in SHAPES:
        ns = -(-n // 512)
        nb, sub = 2 * ns, 2 * (d // 128)
        for grid in GRIDS:
            g0 = max(grid * 4 // 8, 1) if grid > 0 else CUS
            out.append((ns, 0, ns, 0, nb, 0, 0, g0, MIN_CHUNKS, sub))
        j0 = COL_ROW0 // 256
        out.append((ns, 0, ns, j0, nb, SKIP_INSIDE[0] // 256, SKIP_INSIDE[1] // 256, CUS, MIN_CHUNKS, sub))
        out.append((ns, 0, ns, j0, nb, j0 + 1, nb, CUS, MIN_CHUNKS, sub))
    return out


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gram_pipe") / "driver")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-Wall", "-I" + CSRC, SRC, "-o", exe], check=True)
    return exe


def test_sweep_every_chain_once_and_protocols_hold(driver):
    out = subprocess.run([driver, "sweep"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert out.stdout.split() == ["cases", SWEEP_CASES, "failures", "0"], out.stdout[-4000:]


def test_gpu_test_launches_meet_every_boundary_kind(driver):
    total = {}
    for launch in _launches():
        out = subprocess.run([driver, "kinds"] + [str(v) for v in launch], capture_output=True, text=True)
        assert out.returncode == 0, (launch, out.stdout[-4000:])
        words = out.stdout.split()
        got = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
        assert got["failures"] == 0, (launch, out.stdout)
        for k, v in got.items():
            total[k] = total.get(k, 0) + v
    for kind in ("same_rows", "rows_change", "sub_slice", "one_pair_unit", "act_to_idle", "idle_to_act",
                 "single_pair_block", "claim_past_end"):
        assert total[kind] > 0, (kind, total)


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
    assert out.stdout.split() == ["cases", SWEEP_CASES, "failures", "0"], out.stdout[-4000:]
