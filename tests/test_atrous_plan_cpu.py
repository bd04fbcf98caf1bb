"""plan_atrous (caesar_yolo_amd/csrc/cy_measure_plan.cpp) on the CPU against the geometry restated here: column blocks of 256, the
residue classes y mod step that hold a row, chunks of 64 rows of a class, the grid cap, sizes in 64-bit, and the limit messages (shape,
step, null buffers, 2^31 pixels, overlapping buffers).  The planner is linked into tests/host/atrous_plan_main.cpp, built here with
AddressSanitizer and UBSan and run as a child process; a sanitizer report ends the child with a non-zero status and fails the test."""
import os
import shutil
import subprocess

import pytest

import atrous_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "caesar_yolo_amd", "csrc")
COLS, CHUNK, GRID_MAX, STEP_MAX = AC.COLS, AC.CHUNK, AC.GRID_MAX, 64
BAD_SHAPE, BAD_STEP, NULL, NO_OUT = "MH, MW > 0 required", "step outside 1 .. CY_ATROUS_STEP_MAX", "null argument", "d_smooth and d_detail are both null"
TOO_LARGE, WRAPS = "image of 2^31 pixels or more", "buffer beyond the address range"
OVER_IN, OVER_OUT = "an output overlaps the input", "d_smooth overlaps d_detail"
BASE = 1 << 40                                                # a plausible device address


def geometry(MH, MW, step, a_in, smooth, detail):
    """What plan_atrous returns, in Python integers; the checks in its order."""
    if MH <= 0 or MW <= 0:
        return "error " + BAD_SHAPE
    if not 1 <= step <= STEP_MAX:
        return "error " + BAD_STEP
    if not a_in:
        return "error " + NULL
    if not smooth and not detail:
        return "error " + NO_OUT
    if MH * MW >= 1 << 31:
        return "error " + TOO_LARGE
    nbytes = 4 * MH * MW
    if any(a + nbytes >= 1 << 64 for a in (a_in, smooth, detail)):
        return "error " + WRAPS
    over = lambda a, b: bool(a and b and a < b + nbytes and b < a + nbytes)
    if over(a_in, smooth) or over(a_in, detail):
        return "error " + OVER_IN
    if over(smooth, detail):
        return "error " + OVER_OUT
    ncb, nres, nchunk = -(-MW // COLS), min(step, MH), -(-(-(-MH // step)) // CHUNK)
    items = ncb * nres * nchunk
    return "ok %d %d %d %d %d %d" % (ncb, nres, nchunk, items, min(items, GRID_MAX), nbytes)


def buffers(MH, MW):
    """Three buffers that touch without overlapping."""
    n = 4 * MH * MW
    return BASE, BASE + n, BASE + 2 * n


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """The sanitized program, built once: the clang++ beside hipcc, else g++; no compiler is a failure."""
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    near = [os.path.join(os.path.dirname(hipcc), d, "clang++") for d in (".", "../llvm/bin", "../lib/llvm/bin")]
    cxx = next((c for c in near if os.path.exists(c)), None) or shutil.which("g++")
    assert cxx, "no clang++ beside hipcc and no g++: the planner cannot be checked"
    exe = str(tmp_path_factory.mktemp("atrous_plan") / "atrous_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "host", "atrous_plan_main.cpp"), os.path.join(CSRC, "cy_measure_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, "%s: exit %d\n%s" % (args, r.returncode, r.stderr[-4000:])
        return r.stdout.strip()
    return run


SHAPES = [(1, 1), (1, 7), (7, 1), (3, 5), (70, 75), (64, 96), (9, 256), (9, 257), (9, 513), (64, 31), (65, 31), (129, 31), (258, 31),
          (GRID_MAX * CHUNK + 1, 3), (16384, 16384), (46340, 46340),
          (1, (1 << 31) - 1), ((1 << 31) - 1, 1), (2, (1 << 30) - 1), (32768, 65535)]       # strips and shapes just below 2^31 pixels


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_geometry(planner, shape):
    MH, MW = shape
    a = buffers(MH, MW)
    for step in (1, 2, 3, 8, 63, 64):
        for args in ((a[0], a[1], a[2]), (a[0], a[1], 0), (a[0], 0, a[2]), (a[1], a[0], a[2])):
            want = geometry(MH, MW, step, *args)
            assert want.startswith("ok") and planner(MH, MW, step, *args) == want, (step, args)


def test_the_reference_geometry_is_the_one_the_cases_assume():
    a = buffers(64, 96)
    assert geometry(64, 96, 1, *a) == "ok 1 1 1 1 1 24576" and geometry(65, 257, 1, *buffers(65, 257)) == "ok 2 1 2 4 4 66820"
    assert geometry(129, 31, 2, *buffers(129, 31)).split()[1:5] == ["1", "2", "2", "4"]
    assert geometry(5, 31, 64, *buffers(5, 31)).split()[1:5] == ["1", "5", "1", "5"]          # classes without a row are no items
    for name in ("tall_s1", "tall_s3"):
        c = AC.case(name)
        MH, MW = c.map.shape
        got = geometry(MH, MW, c.step, *buffers(MH, MW)).split()
        assert int(got[4]) == AC.items(MH, MW, c.step) > GRID_MAX == int(got[5])
    assert geometry((1 << 31) - 1, 1, 1, *buffers((1 << 31) - 1, 1)).split()[3:6] == ["33554432", "33554432", "8192"]


def test_limit_messages(planner):
    def both(want, *args):
        assert geometry(*args) == "error " + want and planner(*args) == "error " + want, args
    a = buffers(64, 96)
    n = 4 * 64 * 96
    for MH, MW in ((0, 96), (64, 0), (-1, 96), (64, -5)):
        both(BAD_SHAPE, MH, MW, 1, *a)
    for step in (0, 65, -1, 1 << 20):
        both(BAD_STEP, 64, 96, step, *a)
    for step in (1, 64):
        assert planner(64, 96, step, *a).startswith("ok")
    both(NULL, 64, 96, 1, 0, a[1], a[2])
    both(NO_OUT, 64, 96, 1, a[0], 0, 0)
    for MH, MW in ((1 << 16, 1 << 15), (1 << 30, 2), ((1 << 31) - 1, (1 << 31) - 1), (46341, 46341), (2, 1 << 30)):
        both(TOO_LARGE, MH, MW, 1, BASE, BASE + (1 << 34), BASE + (1 << 35))
    both(WRAPS, 64, 96, 1, a[0], (1 << 64) - n, 0)
    both(WRAPS, 64, 96, 1, (1 << 64) - 4, a[1], 0)
    # overlapping by one float at either end, identical, and adjacent (which is allowed)
    for d in (0, 4, n - 4, -4, -(n - 4)):
        both(OVER_IN, 64, 96, 1, a[0], a[0] + d, 0)
        both(OVER_IN, 64, 96, 1, a[0], 0, a[0] + d)
        both(OVER_IN, 64, 96, 1, a[0], a[0] + 8 * n, a[0] + d)
        both(OVER_OUT, 64, 96, 1, a[0], a[0] + 8 * n, a[0] + 8 * n + d)
    for d in (n, -n):
        assert planner(64, 96, 1, a[0], a[0] + d, 0).startswith("ok") and planner(64, 96, 1, a[0], a[0] + 8 * n, a[0] + 8 * n + d).startswith("ok")
