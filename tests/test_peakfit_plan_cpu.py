"""plan_peak_fits (caesar_yolo_amd/csrc/cy_measure_plan.cpp) on the CPU against the rules restated in tests/peakfit_ref.py with
Python integers: statuses, windows, the clipped flag, the neighbour lists with their order and ties, the crowded flag, the squared
radius and the start relative to the window, for the job tables of tests/peakfit_cases.py, images of one row or column and just
below 2^31 pixels, every argument error with its message in the planner's order, and a table of 70 000 jobs.  The planner is linked
into tests/host/peakfit_plan_main.cpp, built here with AddressSanitizer and UBSan and run as a child process; a sanitizer report ends
the child with a non-zero status and fails the test."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import peakfit_cases as PC
import peakfit_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "caesar_yolo_amd", "csrc")
BAD_SHAPE, TOO_LARGE, BAD_N, BAD_ITER, NULL = ("MH, MW > 0 required", "image of 2^31 pixels or more", "n outside 0 .. CY_PFIT_JOBS_MAX",
                                                "max_iter outside 1 .. 256", "null argument")
INF, NAN = float("inf"), float("nan")
START = [1.0, 0.0, 0.0, 0.25, 0.0, 0.25]


def job_line(st, x0, x1, y0, y1, clipped, neigh, count, job):
    if st:
        return "%d 0 -1 0 -1 0 0 0" % st + " -1" * PR.NEIGH_MAX + " " + " ".join([(0.0).hex()] * 3)
    return " ".join(["%d %d %d %d %d %d %d %d" % (st, x0, x1, y0, y1, clipped, len(neigh), int(count > PR.NEIGH_MAX))] +
                    [str(f) for f in neigh + [-1] * (PR.NEIGH_MAX - len(neigh))] +
                    [(float(job[2]) * float(job[2])).hex(), (float(job[6]) - float(x0)).hex(), (float(job[7]) - float(y0)).hex()])


def expected(MH, MW, jobs, max_iter=64, nulls="-", n=None, only=None):
    """What peakfit_plan_main prints (without its last line); the checks in the planner's order.  only: the jobs whose lines are
    wanted (the other lines are None)."""
    n = len(jobs) if n is None else n
    if MH <= 0 or MW <= 0:
        return ["error " + BAD_SHAPE]
    if MH * MW >= 1 << 31:
        return ["error " + TOO_LARGE]
    if not 0 <= n <= PR.JOBS_MAX:
        return ["error " + BAD_N]
    if not 1 <= max_iter <= 256:
        return ["error " + BAD_ITER]
    if n > 0 and set(nulls) & set("mjo"):
        return ["error " + NULL]
    if n == 0:
        return ["ok 0", "run"]
    win, neigh, count = PR.plan(jobs, MH, MW, only)
    lines = [job_line(*win[e], neigh[e], count[e], jobs[e]) if count[e] >= 0 else None for e in range(n)]
    run = [str(e) for e in range(n) if win[e, 0] == 0]
    return ["ok %d" % len(run)] + lines + [" ".join(["run"] + run)]


def _canon(line):
    """A job line of the program with its %a numbers in Python's spelling."""
    t = line.split()
    return line if t[0] in ("ok", "error", "run", "plan_ms") else " ".join(t[:-3] + [float.fromhex(v).hex() for v in t[-3:]])


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """The sanitized program, built once: the clang++ beside hipcc, else g++; no compiler is a failure."""
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    near = [os.path.join(os.path.dirname(hipcc), d, "clang++") for d in (".", "../llvm/bin", "../lib/llvm/bin")]
    cxx = next((c for c in near if os.path.exists(c)), None) or shutil.which("g++")
    assert cxx, "no clang++ beside hipcc and no g++: the planner cannot be checked"
    exe = str(tmp_path_factory.mktemp("peakfit_plan") / "peakfit_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "host", "peakfit_plan_main.cpp"), os.path.join(CSRC, "cy_measure_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(MH, MW, jobs, max_iter=64, nulls="-", n=None):
        n = len(jobs) if n is None else n
        text = " ".join(float(v).hex() if math.isfinite(v) else repr(float(v)) for j in jobs for v in j)
        r = subprocess.run([exe, str(MH), str(MW), str(n), str(max_iter), nulls], input=text, capture_output=True, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, "%s: exit %d\n%s" % ((MH, MW, n, max_iter, nulls), r.returncode, r.stderr[-4000:])
        lines = [_canon(line) for line in r.stdout.strip().split("\n")]
        ms = None
        if lines[-1].startswith("plan_ms"):
            ms = float(lines.pop().split()[1])
        return lines, ms
    return run


def both(planner, MH, MW, jobs, max_iter=64, nulls="-", n=None):
    want = expected(MH, MW, [list(j) for j in jobs], max_iter, nulls, n)
    got, _ = planner(MH, MW, jobs, max_iter, nulls, n)
    assert got == want, (MH, MW, max_iter, nulls, n)
    return want


@pytest.mark.parametrize("g", PC.groups(), ids=lambda g: g.name)
def test_the_cases(planner, g):
    MH, MW = g.map.shape
    want = both(planner, MH, MW, g.jobs.tolist(), g.max_iter)
    # the plan is that of the reference rows the GPU test compares with
    rows = PC.reference(g)[0] if g.name != "r256" else None
    for e, line in enumerate(want[1:-1]):
        t = [int(v) for v in line.split()[:8]]
        if rows is not None:
            assert t[0] == (0 if rows[e, 0] in (0, 2, 3, 4) else rows[e, 0])
            assert (t[1:5] == rows[e, 32:36].tolist() and t[5:8] == rows[e, 36:39].tolist()) if t[0] == 0 else rows[e, 32:36].tolist() == [-1.0] * 4
    for nm, (nn, crowded) in getattr(g, "expect", {}).items():
        t = want[1 + g.names.index(nm)].split()
        assert (int(t[6]), int(t[7])) == (nn, crowded), nm
    if g.name == "neigh":
        ix = {nm: i for i, nm in enumerate(g.names)}
        line = lambda nm: [int(v) for v in want[1 + ix[nm]].split()[8:16]]
        assert line("crowd") == [ix["ring%d" % t] for t in range(8)]                  # twelve at one distance: the first eight by index
        assert line("at2r")[:2] == [ix["at2r_y"], -1] and line("at2r_x") == [-1] * 8 and line("same_a")[0] == ix["same_b"] and line("same_b")[0] == ix["same_a"]
        assert line("turned_away") == [-1] * 8


def test_order_and_ties_of_the_neighbour_list(planner):
    # around e = job 0: equal distances keep the index order, a nearer one comes first whatever its index, the ninth is dropped
    ring = [(3, 4), (-3, 4), (5, 0), (0, -5), (4, 3), (-4, -3), (0, 5), (-5, 0), (3, -4)]
    jobs = [[50.0, 50.0, 6.0, 0.0, 1.0] + START] + [[50.0 + x, 50.0 + y, 1.0, 0.0, 1.0] + START for x, y in ring] + [[51.0, 50.0, 1.0, 0.0, -1.0] + START]
    want = both(planner, 100, 100, jobs)
    t = want[1].split()
    assert t[6:8] == ["8", "1"] and [int(v) for v in t[8:16]] == [10, 1, 2, 3, 4, 5, 6, 7]
    # R_f does not count for e's list: the relation is not symmetric
    jobs = [[20.0, 20.0, 10.0, 0.0, 1.0] + START, [35.0, 20.0, 2.0, 0.0, 1.0] + START]
    want = both(planner, 64, 64, jobs)
    assert want[1].split()[6:9] == ["1", "0", "1"] and want[2].split()[6:9] == ["0", "0", "-1"]
    # a tiny radius whose square underflows has no neighbour, not even a coincident one
    jobs = [[20.0, 20.0, 1e-200, 0.0, 1.0] + START, [20.0, 20.0, 3.0, 0.0, 1.0] + START]
    want = both(planner, 64, 64, jobs)
    assert want[1].split()[6] == "0" and want[2].split()[6] == "1"


def test_centres_and_radii_on_other_shapes(planner):
    centres = [(3.0, 4.0), (0.5, 0.5), (0.49999999999999994, 0.0), (-0.5, 0.0), (255.5, 0.0), (-256.0, 0.0), (math.nextafter(-256.0, -INF), 0.0),
               (1e300, 0.0), (NAN, 1.0), (1.0, INF), (6.0, -3.0), (30.0, 23.0)]
    radii = [1.0, 0.25, 1e-3, 256.0, math.nextafter(256.0, INF), 0.0, -1.0, NAN, INF, 5e-324, 44.0]
    jobs = [[x, y, R, 0.0, 1.0] + START for x, y in centres for R in radii] + [[3.0, 4.0, 2.0, b, s] + START for b, s in ((NAN, 1.0), (0.0, 0.0), (0.0, -1.0), (INF, -1.0), (0.0, 1.5))]
    for MH, MW in ((1, 1), (1, 7), (7, 1), (24, 31), (600, 600)):
        want = both(planner, MH, MW, jobs)
        assert {int(line.split()[0]) for line in want[1:-1]} == {0, 1, 5}
    want = both(planner, 1, 1, [[-256.0, 0.0, 256.0, 0.0, 1.0] + START, [math.nextafter(-256.0, -INF), 0.0, 256.0, 0.0, 1.0] + START])
    assert want[1].split()[:6] == ["0", "0", "0", "0", "0", "1"] and want[2].split()[0] == "5"


def test_strips_and_shapes_just_below_2_31_pixels(planner):
    big = (1 << 31) - 1
    for MH, MW in ((1, big), (big, 1), (2, (1 << 30) - 1), (32768, 65535), (46340, 46340)):
        last = (float(MW - 1), float(MH - 1))
        jobs = [[x, y, R, 0.0, 1.0] + START for x, y, R in (
            (0.0, 0.0, 4.0), (last[0], last[1], 4.0), (last[0] + 3.0, last[1], 4.0), (last[0] + 2.0, last[1] + 2.0, 4.0), (last[0] + 256.0, last[1], 256.0),
            (last[0] / 2, last[1] / 2, 256.0), (last[0], last[1] + 256.0, 256.0), (last[0] + 257.0, last[1], 256.0), (float(big), float(big), 256.0),
            (4e9, 0.0, 4.0), (0.0, -4e9, 4.0), (1e300, 1e300, 4.0))]
        want = both(planner, MH, MW, jobs)
        assert want[0] == "ok %d" % sum(line.startswith("0 ") for line in want[1:-1])
        assert want[2].split()[:6] == ["0", str(max(MW - 5, 0)), str(MW - 1), str(max(MH - 5, 0)), str(MH - 1), "1"]
        assert want[5].split()[:6] == ["0", str(MW - 1), str(MW - 1), str(max(MH - 257, 0)), str(MH - 1), "1"]


def test_argument_errors_and_their_messages(planner):
    jobs = [[3.0, 4.0, 2.0, 0.0, 1.0] + START]
    assert both(planner, 9, 9, jobs)[0] == "ok 1"
    for MH, MW in ((0, 9), (9, 0), (-1, 9), (9, -5), (0, 0)):
        assert both(planner, MH, MW, jobs) == ["error " + BAD_SHAPE]
    for MH, MW in ((1 << 16, 1 << 15), (1 << 30, 2), ((1 << 31) - 1, (1 << 31) - 1), (46341, 46341), (2, 1 << 30)):
        assert both(planner, MH, MW, jobs) == ["error " + TOO_LARGE]
    for n in (-1, PR.JOBS_MAX + 1, -(1 << 31), (1 << 31) - 1):
        assert both(planner, 9, 9, [], n=n) == ["error " + BAD_N]
    for it in (0, -1, 257, 1 << 20):
        assert both(planner, 9, 9, jobs, max_iter=it) == ["error " + BAD_ITER]
        assert both(planner, 9, 9, [], max_iter=it) == ["error " + BAD_ITER]          # also without a job
    for nulls in ("m", "j", "o", "mjo"):
        assert both(planner, 9, 9, jobs, nulls=nulls) == ["error " + NULL]
        assert both(planner, 9, 9, [], nulls=nulls) == ["ok 0", "run"]              # n == 0: no pointer is looked at
    # the order of the checks: shape, size, n, max_iter, pointers
    assert both(planner, 0, 9, [], 0, "m", n=-1) == ["error " + BAD_SHAPE]
    assert both(planner, 1 << 16, 1 << 15, [], 0, "m", n=-1) == ["error " + TOO_LARGE]
    assert both(planner, 9, 9, [], 0, "m", n=-1) == ["error " + BAD_N]
    assert both(planner, 9, 9, jobs, 0, "m") == ["error " + BAD_ITER]
    assert both(planner, 9, 9, jobs, 1, "o") == ["error " + NULL]
    assert both(planner, 9, 9, jobs, 256)[0] == "ok 1" and both(planner, 9, 9, jobs, 1)[0] == "ok 1"      # the limits themselves are in range


def test_a_long_job_table(planner):
    """70 000 jobs on 600 x 600, radii 1 .. 12, some turned away: every status and window against the restatement, the neighbour
    lists of every 97th job, and the planner's own time.  A search that compared every pair would need 4.9e9 distance tests."""
    rng = np.random.default_rng(70000)
    n = 70000
    jobs = np.zeros((n, PR.JOB_FIELDS))
    jobs[:, 0], jobs[:, 1] = rng.uniform(-8.0, 608.0, n), rng.uniform(-8.0, 608.0, n)
    jobs[:, 2] = rng.integers(1, 13, n).astype(np.float64)
    jobs[:, 4], jobs[:, 5:] = 1.0, START
    jobs[rng.integers(0, n, 700), 2] = -1.0
    jobs[rng.integers(0, n, 700), 0] = NAN
    jobs[:n // 2:1000, :2] = jobs[1:n // 2:1000, :2]                                     # coincident pairs
    only = list(range(0, n, 97))
    want = expected(600, 600, jobs.tolist(), only=only)
    got, ms = planner(600, 600, jobs.tolist())
    assert got[0] == want[0] and got[-1] == want[-1]
    win = [" ".join(line.split()[:6]) for line in got[1:-1]]
    ref = PR.plan(jobs, 600, 600, only=[])[0]
    assert win == ["%d %d %d %d %d %d" % (tuple(r) if r[0] == 0 else (r[0], 0, -1, 0, -1, 0)) for r in ref]
    for e in only:
        assert got[1 + e] == want[1 + e], e
    crowded = sum(int(got[1 + e].split()[7]) for e in only)
    assert crowded > len(only) // 2, "the table is meant to be crowded"
    print("plan_peak_fits: %d jobs in %.0f ms (sanitized build)" % (n, ms))
    assert ms < 10000.0, "the planner took %.0f ms for %d jobs: a quadratic search?" % (ms, n)
