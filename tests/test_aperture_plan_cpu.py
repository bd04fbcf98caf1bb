"""plan_apertures (caesar_yolo_amd/csrc/cy_measure_plan.cpp) on the CPU against the rules restated in tests/aperture_ref.py with
Python integers (math.ceil / math.floor give exact integers, so no window edge is ever converted out of range): statuses, windows,
the clipped flag and the squared radii for the centres and radii of tests/aperture_cases.py, images of one row or column and just
below 2^31 pixels, and every argument error with its message, in the planner's order.  The planner is linked into
tests/host/aperture_plan_main.cpp, built here with AddressSanitizer and UBSan and run as a child process; a sanitizer report ends the
child with a non-zero status and fails the test."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import aperture_cases as PC
import aperture_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "caesar_yolo_amd", "csrc")
BAD_SHAPE, TOO_LARGE, BAD_N, BAD_K = "MH, MW > 0 required", "image of 2^31 pixels or more", "n outside 0 .. CY_APER_JOBS_MAX", "K outside 1 .. CY_APER_RINGS_MAX"
NULL, BAD_FACTORS = "null argument", "factors must be finite, positive and strictly increasing"
INF, NAN = float("inf"), float("nan")


def expected(MH, MW, jobs, K, factors, nulls="-", n=None):
    """What aperture_plan_main prints; the checks in the planner's order."""
    n = len(jobs) if n is None else n
    if MH <= 0 or MW <= 0:
        return "error " + BAD_SHAPE
    if MH * MW >= 1 << 31:
        return "error " + TOO_LARGE
    if not 0 <= n <= PR.JOBS_MAX:
        return "error " + BAD_N
    if not 1 <= K <= PR.RINGS_MAX:
        return "error " + BAD_K
    if n > 0 and set(nulls) & set("mjfo"):
        return "error " + NULL
    if "f" not in nulls and not all(math.isfinite(f) and f > 0 and (k == 0 or f > factors[k - 1]) for k, f in enumerate(factors[:K])):
        return "error " + BAD_FACTORS
    lines, measured = [], 0
    for cx, cy, unit in jobs:
        st, x0, x1, y0, y1, clipped, r2 = PR.window(cx, cy, unit, factors[:K], MH, MW)
        if st:
            x0, x1, y0, y1 = 0, -1, 0, -1                     # the planner's empty window; the row of the entry says -1
        measured += st == 0
        lines.append(" ".join(["%d %d %d %d %d %d" % (st, x0, x1, y0, y1, clipped)] + [float(v).hex() for v in r2 + [0.0] * (PR.RINGS_MAX - len(r2))]))
    return "\n".join(["ok %d" % measured] + lines)


def _canon(text):
    """The program's output with its %a numbers in Python's spelling."""
    out = []
    for line in text.strip().split("\n"):
        t = line.split()
        out.append(line if t[0] in ("ok", "error") else " ".join(t[:6] + [float.fromhex(v).hex() for v in t[6:]]))
    return "\n".join(out)


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """The sanitized program, built once: the clang++ beside hipcc, else g++; no compiler is a failure."""
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    near = [os.path.join(os.path.dirname(hipcc), d, "clang++") for d in (".", "../llvm/bin", "../lib/llvm/bin")]
    cxx = next((c for c in near if os.path.exists(c)), None) or shutil.which("g++")
    assert cxx, "no clang++ beside hipcc and no g++: the planner cannot be checked"
    exe = str(tmp_path_factory.mktemp("aperture_plan") / "aperture_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "host", "aperture_plan_main.cpp"), os.path.join(CSRC, "cy_measure_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(MH, MW, jobs, K, factors, nulls="-", n=None):
        n = len(jobs) if n is None else n
        text = " ".join(float(v).hex() if math.isfinite(v) else repr(float(v)) for v in list(factors) + [x for j in jobs for x in j])
        r = subprocess.run([exe, str(MH), str(MW), str(n), str(K), nulls], input=text, capture_output=True, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, "%s: exit %d\n%s" % ((MH, MW, n, K, nulls), r.returncode, r.stderr[-4000:])
        return _canon(r.stdout)
    return run


def both(planner, MH, MW, jobs, factors, nulls="-", n=None, K=None):
    K = len(factors) if K is None else K
    want = expected(MH, MW, jobs, K, list(factors), nulls, n)
    got = planner(MH, MW, jobs, K, factors, nulls, n)
    assert got == want, (MH, MW, K, nulls, n)
    return want


@pytest.mark.parametrize("name", [n for n in PC.NAMES if n != "many_jobs"])
def test_the_cases(planner, name):
    c = PC.case(name)
    MH, MW = c.map.shape
    want = both(planner, MH, MW, c.jobs.tolist(), c.factors)
    # the windows are those of the reference rows the GPU test compares with
    rows = PC.rows(name)
    for line, row in zip(want.split("\n")[1:], rows):
        t = [int(v) for v in line.split()[:6]]
        assert t[0] == row[0] and t[5] == row[5] and (t[1:5] == row[1:5].tolist() if t[0] == 0 else row[1:5].tolist() == [-1.0] * 4)


def test_centres_and_radii_on_other_shapes(planner):
    centres = PC.CENTRES + [(0.5, 0.5), (0.49999999999999994, 0.0), (-0.5, 0.0), (255.5, 0.0), (-256.0, 0.0), (math.nextafter(-256.0, -INF), 0.0)]
    units = [1.0, 0.25, 1e-3, 64.0, math.nextafter(64.0, INF), 0.0, -1.0, NAN, INF, 5e-324]
    jobs = [[x, y, u] for x, y in centres for u in units]
    for MH, MW in ((1, 1), (1, 7), (7, 1), (24, 31), (600, 600)):
        want = both(planner, MH, MW, jobs, (1.0, 2.0, 4.0))
        assert {int(line.split()[0]) for line in want.split("\n")[1:]} == {0, 1, 2}
    assert both(planner, 1, 1, [[-256.0, 0.0, 64.0], [math.nextafter(-256.0, -INF), 0.0, 64.0]], (4.0,)).split("\n")[1:] == [
        " ".join(["0 0 0 0 0 1", (65536.0).hex()] + [(0.0).hex()] * 7), " ".join(["2 0 -1 0 -1 0"] + [(0.0).hex()] * 8)]


def test_strips_and_shapes_just_below_2_31_pixels(planner):
    big = (1 << 31) - 1
    for MH, MW in ((1, big), (big, 1), (2, (1 << 30) - 1), (32768, 65535), (46340, 46340)):
        last = (float(MW - 1), float(MH - 1))
        jobs = [[0.0, 0.0, 1.0], [last[0], last[1], 1.0], [last[0] + 3.0, last[1], 1.0], [last[0] + 2.0, last[1] + 2.0, 1.0], [last[0] + 256.0, last[1], 64.0],
                [last[0] / 2, last[1] / 2, 64.0], [last[0], last[1] + 256.0, 64.0], [last[0] + 257.0, last[1], 64.0], [float(big), float(big), 64.0],
                [4e9, 0.0, 1.0], [0.0, -4e9, 1.0], [1e300, 1e300, 1.0]]
        want = both(planner, MH, MW, jobs, (1.0, 2.0, 4.0)).split("\n")
        assert want[0] == "ok %d" % sum(line.startswith("0 ") for line in want[1:])
        assert want[2].split()[:6] == ["0", str(max(MW - 5, 0)), str(MW - 1), str(max(MH - 5, 0)), str(MH - 1), "1"]
        assert want[5].split()[:6] == ["0", str(MW - 1), str(MW - 1), str(max(MH - 257, 0)), str(MH - 1), "1"]


def test_argument_errors_and_their_messages(planner):
    jobs, f = [[3.0, 4.0, 1.0]], (1.0, 2.0)
    assert both(planner, 9, 9, jobs, f).startswith("ok 1")
    for MH, MW in ((0, 9), (9, 0), (-1, 9), (9, -5), (0, 0)):
        assert both(planner, MH, MW, jobs, f) == "error " + BAD_SHAPE
    for MH, MW in ((1 << 16, 1 << 15), (1 << 30, 2), ((1 << 31) - 1, (1 << 31) - 1), (46341, 46341), (2, 1 << 30)):
        assert both(planner, MH, MW, jobs, f) == "error " + TOO_LARGE
    for n in (-1, PR.JOBS_MAX + 1, -(1 << 31), (1 << 31) - 1):
        assert both(planner, 9, 9, [], f, n=n) == "error " + BAD_N
    for K in (0, -1, 9, 64):
        assert both(planner, 9, 9, jobs, (1.0,) * max(K, 0), K=K) == "error " + BAD_K
        assert both(planner, 9, 9, [], (1.0,) * max(K, 0), K=K) == "error " + BAD_K
    for nulls in ("m", "j", "f", "o", "mjfo"):
        assert both(planner, 9, 9, jobs, f, nulls) == "error " + NULL
        assert both(planner, 9, 9, [], f, nulls) == "ok 0"        # n == 0: no pointer is looked at, the factors only when given
    for bad in ((0.0, 1.0), (-1.0, 1.0), (1.0, 1.0), (2.0, 1.0), (1.0, NAN), (NAN, 1.0), (1.0, INF), (-INF, 1.0), (1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 7.0),
                (5e-324, 5e-324), (0.0,), (NAN,), (INF,)):
        assert both(planner, 9, 9, jobs, bad) == "error " + BAD_FACTORS
        assert both(planner, 9, 9, [], bad) == "error " + BAD_FACTORS
    # the order of the checks: shape, size, n, K, pointers, factors
    assert both(planner, 0, 9, [], (2.0, 1.0), "m", n=-1, K=2) == "error " + BAD_SHAPE
    assert both(planner, 1 << 16, 1 << 15, [], (2.0, 1.0), "m", n=-1, K=2) == "error " + TOO_LARGE
    assert both(planner, 9, 9, [], (2.0, 1.0), "m", n=-1, K=2) == "error " + BAD_N
    assert both(planner, 9, 9, jobs, (), "m", K=0) == "error " + BAD_K
    assert both(planner, 9, 9, jobs, (2.0, 1.0), "o") == "error " + NULL
    # the limits themselves are in range
    assert both(planner, 9, 9, jobs, (1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0)).startswith("ok 1") and both(planner, 9, 9, jobs, (5e-324, 1e-323)).startswith("ok 1")


def test_a_long_job_table(planner):
    i = np.arange(70 * 70 * 5)
    jobs = np.stack([(i % 70).astype(np.float64) - 3.0, (i // 70 % 70).astype(np.float64) - 3.0, 1.0 + (i % 5)], axis=1).tolist()
    assert both(planner, 64, 64, jobs, (1.0,)).startswith("ok ")
