"""plan_peaks (caesar_yolo_amd/csrc/cy_measure_plan.cpp) on the CPU against the segment geometry restated here: segments of 1024
consecutive pixels of one row, row-major, table sizes in 64-bit, and the limit messages (pixels, segments, and a row whose last
segment, plus the radius, leaves the 32-bit range the kernels hold columns in).  The planner is linked into
tests/host/peaks_plan_main.cpp, built here with AddressSanitizer and UBSan and run as a child process; a sanitizer report ends the
child with a non-zero status and fails the test."""
import os
import shutil
import subprocess

import pytest

import peaks_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "caesar_yolo_amd", "csrc")
SEG, WORDS, FIELDS, MAX_SEG = PC.SEG, PC.SEG // 64, 12, 1 << 24
TOO_LARGE = "image of 2^31 pixels or more (32-bit pixel indices and peak counts)"
TOO_MANY = "segment table above 2^24 entries"
TOO_WIDE = "row too wide (its last segment ends beyond column 2^31 - 1 - radius)"


def geometry(MH, MW, radius, cap):
    """What plan_peaks returns, in Python integers."""
    if MH * MW >= 1 << 31:
        return "error " + TOO_LARGE
    nsx = -(-MW // SEG)
    if nsx * SEG + radius > (1 << 31) - 1:
        return "error " + TOO_WIDE
    nseg = MH * nsx
    if nseg > MAX_SEG:
        return "error " + TOO_MANY
    return "ok %d %d %d %d" % (nsx, nseg, nseg * WORDS, cap * FIELDS)


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """The sanitized program, built once: the clang++ beside hipcc, else g++; no compiler is a failure."""
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    near = [os.path.join(os.path.dirname(hipcc), d, "clang++") for d in (".", "../llvm/bin", "../lib/llvm/bin")]
    cxx = next((c for c in near if os.path.exists(c)), None) or shutil.which("g++")
    assert cxx, "no clang++ beside hipcc and no g++: the planner cannot be checked"
    exe = str(tmp_path_factory.mktemp("peaks_plan") / "peaks_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "host", "peaks_plan_main.cpp"), os.path.join(CSRC, "cy_measure_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, "%s: exit %d\n%s" % (args, r.returncode, r.stderr[-4000:])
        return r.stdout.strip()
    return run


SHAPES = [(1, 1), (1, 37), (37, 1), (70, 75), (64, 96), (12, 1023), (12, 1024), (12, 1025), (12, 2048), (12, 2049), (16384, 16384),
          (46340, 46340),                    # 2147395600 pixels
          (1, (1 << 31) - SEG), (2, (1 << 30) - 1), (32768, 65535),      # just below 2^31 pixels; the widest row that fits
          (1 << 24, 1), (1 << 24, 127)]      # 2^24 segments exactly


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_geometry(planner, shape):
    for radius, cap in ((1, 0), (2, 65536), (8, 1 << 20)):
        want = geometry(shape[0], shape[1], radius, cap)
        assert want.startswith("ok") and planner(shape[0], shape[1], radius, cap) == want


def test_the_reference_geometry_is_the_one_the_cases_assume():
    assert geometry(12, 1025, 2, 4) == "ok 2 24 384 48" and geometry(12, 2049, 2, 4) == "ok 3 36 576 48"
    assert geometry(1, (1 << 31) - SEG, 8, 0) == "ok 2097151 2097151 33554416 0"


def test_limit_messages(planner):
    for MH, MW in ((1 << 16, 1 << 15), (1 << 30, 2),((1 << 31) - 1, (1 << 31) - 1), (46341, 46341), ((1 << 23) + 1, 1025)):
        assert geometry(MH, MW, 2, 16) == "error " + TOO_LARGE and planner(MH, MW, 2, 16) == "error " + TOO_LARGE
    for MW in ((1 << 31) - 1, (1 << 31) - SEG + 1):      # 2^21 segments: the last one would end at column 2^31
        for radius in (1, 8):
            assert geometry(1, MW, radius, 16) == "error " + TOO_WIDE and planner(1, MW, radius, 16) == "error " + TOO_WIDE
    assert geometry(1, (1 << 31) - SEG, 8, 16).startswith("ok") and planner(1, (1 << 31) - SEG, 8, 16).startswith("ok")
    for MH, MW in (((1 << 24) + 1, 1), ((1 << 24) + 1, 127), ((1 << 31) - 1, 1)):
        assert geometry(MH, MW, 2, 16) == "error " + TOO_MANY and planner(MH, MW, 2, 16) == "error " + TOO_MANY
