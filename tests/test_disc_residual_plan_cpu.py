"""The host side of cy_disc_residuals on the CPU: plan_peak_fits as that entry calls it (max_iter 1) and disc_residual_row
(caesar_yolo_amd/csrc/cy_measure_plan.cpp), linked into tests/host/disc_residual_plan_main.cpp, built here with AddressSanitizer and
UBSan and run as a child process; a sanitizer report ends the child with a non-zero status and fails the test.  The program puts a
recognisable stand-in where the kernel's rows would be, so the test sees which fields a row takes over and which the plan decides:
for the job tables of tests/disc_residual_cases.py against tests/disc_residual_ref.py, n = 0, every status, every argument error
with its message in the entry's order, and a table of 2^20 jobs."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import disc_residual_cases as DC
import disc_residual_ref as DR
import peakfit_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "caesar_yolo_amd", "csrc")
BAD_SHAPE, TOO_LARGE, BAD_N, NULL = "MH, MW > 0 required", "image of 2^31 pixels or more", "n outside 0 .. CY_PFIT_JOBS_MAX", "null argument"
INF, NAN = float("inf"), float("nan")


def stand_in(t):
    return [1000.0 * t + f + 0.5 for f in range(DR.FIELDS)]


def expected(MH, MW, jobs, nulls="-", n=None):
    """What disc_residual_plan_main prints without COLS: the first line, then the rows; the checks in the entry's order."""
    n = len(jobs) if n is None else n
    if MH <= 0 or MW <= 0:
        return "error " + BAD_SHAPE, None
    if MH * MW >= 1 << 31:
        return "error " + TOO_LARGE, None
    if not 0 <= n <= PR.JOBS_MAX:
        return "error " + BAD_N, None
    if n > 0 and set(nulls) & set("mjo"):
        return "error " + NULL, None
    if n == 0:
        return "ok 0", np.zeros((0, DR.FIELDS))
    win, neigh, _ = PR.plan(jobs, MH, MW)
    rows, t = np.zeros((n, DR.FIELDS)), 0
    for e in range(n):
        st, x0, x1, y0, y1, clipped = (int(v) for v in win[e])
        if st:
            rows[e, 0], rows[e, [6, 7, 10, 11, 12, 13]] = st, -1.0
            continue
        rows[e] = stand_in(t)
        rows[e, 10:16] = [x0, x1, y0, y1, clipped, len(neigh[e])]
        t += 1
    return "ok %d" % t, rows


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """The sanitized program, built once: the clang++ beside hipcc, else g++; no compiler is a failure."""
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    near = [os.path.join(os.path.dirname(hipcc), d, "clang++") for d in (".", "../llvm/bin", "../lib/llvm/bin")]
    cxx = next((c for c in near if os.path.exists(c)), None) or shutil.which("g++")
    assert cxx, "no clang++ beside hipcc and no g++: the planner cannot be checked"
    exe = str(tmp_path_factory.mktemp("disc_residual_plan") / "disc_residual_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "host", "disc_residual_plan_main.cpp"), os.path.join(CSRC, "cy_measure_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(MH, MW, jobs, nulls="-", n=None, cols=None):
        n = len(jobs) if n is None else n
        text = " ".join(float(v).hex() if math.isfinite(v) else repr(float(v)) for j in jobs for v in j)
        r = subprocess.run([exe, str(MH), str(MW), str(n), nulls] + ([str(cols)] if cols else []), input=text, capture_output=True, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, "%s: exit %d\n%s" % ((MH, MW, n, nulls, cols), r.returncode, r.stderr[-4000:])
        return r.stdout.strip().split("\n")
    return run


def rows_of(lines):
    return np.array([[float.fromhex(v) for v in line.split()] for line in lines], np.float64).reshape(-1, DR.FIELDS)


def both(planner, MH, MW, jobs, nulls="-", n=None):
    head, rows = expected(MH, MW, [list(j) for j in jobs], nulls, n)
    got = planner(MH, MW, jobs, nulls, n)
    assert got[0] == head, (MH, MW, nulls, n, got[0])
    if rows is None:
        assert len(got) == 1
    else:
        assert np.array_equal(rows_of(got[1:]), rows), (MH, MW, nulls, n)
    return head, rows


@pytest.mark.parametrize("g", DC.groups(), ids=lambda g: g.name)
def test_the_cases(planner, g):
    MH, MW = g.map.shape
    head, rows = both(planner, MH, MW, g.jobs.tolist())
    # the fields the plan decides are those of the reference rows the GPU test compares with; the others are the kernel's, taken over
    ref = DR.disc_residuals(g.map, g.model, g.jobs)[0]
    plan_fields = [10, 11, 12, 13, 14, 15]
    assert np.array_equal(rows[:, plan_fields], ref[:, plan_fields]) and head == "ok %d" % int((ref[:, 0] == 0).sum())
    turned = ref[:, 0] != 0
    assert np.array_equal(rows[turned], ref[turned])          # statuses 1 and 5: the whole row is the host's
    t = 0
    for e in np.nonzero(~turned)[0]:
        assert rows[e, :10].tolist() == stand_in(t)[:10]
        t += 1


def test_every_status_on_other_shapes(planner):
    centres = [(0.0, 0.0), (3.5, 2.5), (-6.0, 0.0), (math.nextafter(-6.0, -INF), 0.0), (0.0, 1e300), (NAN, 0.0), (0.0, -INF), (8.25, 7.75)]
    fields = [(6.0, 0.0, 1.0), (1.0, 0.5, -1.0), (256.0, 0.0, 1.0), (math.nextafter(256.0, INF), 0.0, 1.0), (0.0, 0.0, 1.0), (-1.0, 0.0, 1.0), (NAN, 0.0, 1.0),
              (6.0, INF, 1.0), (6.0, NAN, 1.0), (6.0, 0.0, 0.0), (6.0, 0.0, 2.0), (6.0, 0.0, NAN), (5e-324, 0.0, 1.0)]
    jobs = [[x, y, R, bkg, sign, NAN, INF, -INF, 0.0, 0.0, 0.0] for x, y in centres for R, bkg, sign in fields]       # the start is ignored
    for MH, MW in ((1, 1), (1, 7), (7, 1), (24, 31)):
        _, rows = both(planner, MH, MW, jobs)
        assert set(rows[:, 0][rows[:, 10] < 0].astype(int)) == {1, 5} and (rows[:, 10] >= 0).any()
    assert both(planner, 9, 9, [])[0] == "ok 0"


def test_argument_errors_and_their_messages(planner):
    jobs = [[3.0, 4.0, 2.0, 0.0, 1.0, 1.0, 3.0, 4.0, 0.25, 0.0, 0.25]]
    assert both(planner, 9, 9, jobs)[0] == "ok 1"
    for MH, MW in ((0, 9), (9, 0), (-1, 9), (9, -5), (0, 0)):
        assert both(planner, MH, MW, jobs)[0] == "error " + BAD_SHAPE
    for MH, MW in ((1 << 16, 1 << 15), (1 << 30, 2), ((1 << 31) - 1, (1 << 31) - 1), (46341, 46341), (2, 1 << 30)):
        assert both(planner, MH, MW, jobs)[0] == "error " + TOO_LARGE
    for n in (-1, PR.JOBS_MAX + 1, -(1 << 31), (1 << 31) - 1):
        assert both(planner, 9, 9, [], n=n)[0] == "error " + BAD_N
    for nulls in ("m", "j", "o", "mjo"):
        assert both(planner, 9, 9, jobs, nulls)[0] == "error " + NULL
        assert both(planner, 9, 9, [], nulls)[0] == "ok 0"      # n == 0: no pointer is looked at
    # the order of the checks: shape, size, n, pointers
    assert both(planner, 0, 9, [], "m", n=-1)[0] == "error " + BAD_SHAPE
    assert both(planner, 1 << 16, 1 << 15, [], "m", n=-1)[0] == "error " + TOO_LARGE
    assert both(planner, 9, 9, [], "m", n=-1)[0] == "error " + BAD_N
    # just below the limit of the image
    assert both(planner, 46340, 46340, [[46339.0, 46339.0, 2.0, 0.0, 1.0] + [0.0] * 6])[1][0, 10:14].tolist() == [46337, 46339, 46337, 46339]


def test_the_longest_job_table(planner):
    """2^20 jobs on a lattice of 65536 columns, made by the program: what the lattice gives is known in closed form."""
    n, cols, rows_ = PR.JOBS_MAX, 65536, 16
    MH, MW = 3 * rows_, 3 * cols
    got = planner(MH, MW, [], n=n, cols=cols)
    i = np.arange(n)
    st1, st5 = i % 7 == 6, (i % 11 == 10) & (i % 7 != 6)       # status 1 is decided before status 5
    ok = ~(st1 | st5)
    ix, iy = i % cols, i // cols
    cx, cy = 3.0 * ix + 0.25, 3.0 * iy + 0.5
    x0, x1 = np.maximum(np.ceil(cx - 2.0), 0), np.minimum(np.floor(cx + 2.0), MW - 1)
    y0, y1 = np.maximum(np.ceil(cy - 2.0), 0), np.minimum(np.floor(cy + 2.0), MH - 1)
    clipped = (np.ceil(cx - 2.0) < 0) | (np.floor(cx + 2.0) > MW - 1) | (np.ceil(cy - 2.0) < 0) | (np.floor(cy + 2.0) > MH - 1)
    grid = ok.reshape(rows_, cols)
    nn = np.zeros((rows_, cols), np.int64)                     # the lattice neighbours at 3 px (D2 = 9 < 16); the diagonal ones are at D2 = 18
    nn[:, 1:] += grid[:, :-1]
    nn[:, :-1] += grid[:, 1:]
    nn[1:, :] += grid[:-1, :]
    nn[:-1, :] += grid[1:, :]
    nn = nn.ravel()
    assert got[0] == "ok %d" % ok.sum()
    assert got[1] == "counts %d %d %d" % (ok.sum(), st1.sum(), st5.sum())
    assert got[2] == "sums %d %d %d %d" % (nn[ok].sum(), (x1 - x0 + 1)[ok].sum(), (y1 - y0 + 1)[ok].sum(), clipped[ok].sum())
    assert got[3] == "wrong 0"
    shown = rows_of(got[4:])
    run_index = np.cumsum(ok) - 1
    for r, e in zip(shown, (0, 1, cols, n - 1)):
        if ok[e]:
            assert r[:10].tolist() == stand_in(int(run_index[e]))[:10] and r[10:].tolist() == [x0[e], x1[e], y0[e], y1[e], float(clipped[e]), float(nn[e])], e
        else:
            assert r[0] == (1 if st1[e] else 5) and r[10] == -1, e
    assert ok[0] and ok[1] and ok[cols] and shown.shape[0] == 4
