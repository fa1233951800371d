"""The integer forms' pair loop as of round 15, walked on the CPU (no GPU
needed): tests/host/gram_fold_driver.cpp (host C++ compiler, no HIP) runs every
wave of every block through the loop of gram_i8sym_kernel / gram_fp4sym_kernel
with GramClaimCursor<4>, lookahead_tiles() and fold_due() of
csrc/gram_schedule.hpp.  A wave's row chains run over up to FOLD_PAIRS pairs of
a row unit: the wave folds at the end of a pair's body when its chain holds
FOLD_PAIRS pairs, or when the rows change behind the pair and the chain holds
anything -- also a wave that idles on that pair.

Sweep (a thinned version of test_gram_schedule_wide.py's, under the fixed deal
and two orders of the claims), for caps 1 (a fold per pair, the parent), 2, 3
(the int8 form's) and 7 (the fp4 form's).  Asserted:
 (a) every taken (slice, pair, wave of the half, tile group) contribution is
     folded exactly once, into the rows it was formed on;
 (b) no chain holds more than FOLD_PAIRS pairs;
 (c) a chain is folded before its rows' flush (no wave holds a chain when the
     row accumulator is flushed), after no later rows' first fold, and before
     load_a replaces its rows;
 (d) all eight waves execute the same number of barriers.
For the exact launches of tests/test_gpu_gram_fold.py (shapes, grids, column
quarters, skip ranges and the crafted operands, planned with plan_launch<4> as
the launcher does) every fold trigger must occur at least once per form: the cap
reached, a rows change with each of 1 .. FOLD_PAIRS - 1 pairs pending, a rows
change while the wave idles with a pending chain, a chain that spans an idle
pair, a one-pair unit, a new slice of the same rows (the forms with several
slices), and the walk's end.
The driver runs once more under ASan + UBSan (host code with its own main,
nothing preloaded)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "distributed-active-learning_amd", "csrc")
SRC = os.path.join(REPO, "tests", "host", "gram_fold_driver.cpp")

FOLD_PAIRS = {"fp4": 7, "i8": 3}    # Cfg::FOLD_PAIRS (DAL_GRAM_FOLD_PAIRS_FP4, _I8)
SLICE_FEATURES = {"fp4": 256, "i8": 128}
# the launches of tests/test_gpu_gram_fold.py: (form, pool rows, features) ...
POOLS = [("fp4", 36_000, 256), ("fp4", 36_000, 512), ("i8", 70_000, 128)]
GRIDS = (1, 2, 5, 0)              # grid_blocks (4-wave blocks: an 8-wave grid of 1, 1, 2 blocks, and the device's)
COL_ROW0 = 512                    # first column row of the call with a skip range
SKIP_INSIDE = (1024, 2048)        # ... a range inside the columns
# ... and the crafted operands: (form, operand rows, features, grids)
CRAFTED = [("fp4", 16_384, 256, (1, 0)), ("fp4", 16_384, 512, (1, 0)), ("i8", 16_384, 128, (1, 0)),
           ("i8", 16_384, 256, (1, 0))]
CUS = 256                         # MI355X
SMALL_BYTES = 32 << 20            # DAL_GRAM_SMALL_MB: column operands up to it take DAL_GRAM_MIN_CHUNKS_SMALL chunks
SWEEP_CASES = "55080"


def quarter_rows(n_pad):
    return n_pad // 512 // 4 * 512  # a quarter of the columns, in whole super blocks


def column_calls(n_pad):
    """(first column row, end, skip) of the calls that add up to the whole Gram: the shuffled
    quarters, then a call with a column offset and a skip range and the two ranges it left out."""
    q = quarter_rows(n_pad)
    quarters = [(2 * q, 3 * q, None), (0, q, None), (3 * q, n_pad, None), (q, 2 * q, None)]
    skipped = [(COL_ROW0, n_pad, SKIP_INSIDE), (0, COL_ROW0, None), (SKIP_INSIDE[0], SKIP_INSIDE[1], None)]
    return quarters, skipped


def _launch(ns, d_pad, form, j_lo, j_hi, skip, g0):
    min_chunks = 2 if (j_hi - j_lo) * 256 * d_pad * 4 <= SMALL_BYTES else 16
    return (ns, 0, ns, j_lo, j_hi, skip[0], skip[1], g0, min_chunks, d_pad // SLICE_FEATURES[form])


def _g0(grid):
    return max(grid // 2, 1) if grid > 0 else CUS


def _launches(form):
    out = []
    for f, n, d in POOLS:
        if f != form:
            continue
        ns = -(-n // 512)
        nb = 2 * ns
        for grid in GRIDS:
            out.append(_launch(ns, d, form, 0, nb, (0, 0), _g0(grid)))
        quarters, skipped = column_calls(ns * 512)
        for c0, c1, skip in quarters + skipped:
            sk = (0, 0) if skip is None else (skip[0] // 256, skip[1] // 256)
            out.append(_launch(ns, d, form, c0 // 256, c1 // 256, sk, CUS))
    for f, rows, d, grids in CRAFTED:
        if f != form:
            continue
        for grid in grids:
            out.append(_launch(rows // 512, d, form, 0, rows // 256, (0, 0), _g0(grid)))
    return out


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gram_fold") / "driver")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-Wall", "-I" + CSRC, SRC, "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("cap", [1, 2, 3, 7])
def test_sweep_every_contribution_folded_once(driver, cap):
    out = subprocess.run([driver, "sweep", str(cap)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:]
    assert out.stdout.split() == ["cases", SWEEP_CASES, "failures", "0"], out.stdout[-4000:]


def test_the_caps_are_the_kernels():
    """FOLD_PAIRS above restates the defaults of csrc/gram_sym.hip."""
    text = open(os.path.join(CSRC, "gram_sym.hip")).read()
    assert f"#define DAL_GRAM_FOLD_PAIRS_FP4 {FOLD_PAIRS['fp4']} " in text
    assert f"#define DAL_GRAM_FOLD_PAIRS_I8 {FOLD_PAIRS['i8']} " in text


@pytest.mark.parametrize("form", ["fp4", "i8"])
def test_gpu_test_launches_meet_every_fold_trigger(driver, form):
    cap = FOLD_PAIRS[form]
    total = {}
    for launch in _launches(form):
        out = subprocess.run([driver, "kinds", str(cap)] + [str(v) for v in launch], capture_output=True, text=True)
        assert out.returncode == 0, (launch, out.stdout[-4000:])
        words = out.stdout.split()
        got = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
        assert got["failures"] == 0, (launch, out.stdout)
        for k, v in got.items():
            total[k] = total.get(k, 0) + v
    kinds = ["cap", "idle_fold", "span_idle", "one_pair_unit", "walk_end"] + [f"partial_{p}" for p in range(1, cap)]
    if any(e[0] == form and e[2] > SLICE_FEATURES[form] for e in POOLS + CRAFTED):  # (launches over several slices)
        kinds.append("same_rows_slice")
    for kind in kinds:
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
    out = subprocess.run([exe, "sweep", "3"], capture_output=True, text=True, env=env)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.split() == ["cases", SWEEP_CASES, "failures", "0"], out.stdout[-4000:]
