"""The host side of cy_forced_fit on the CPU: plan_forced and forced_row (caesar_yolo_amd/csrc/cy_measure_plan.cpp), linked into
tests/host/forced_plan_main.cpp, built here with AddressSanitizer and UBSan and run as a child process; a sanitizer report ends the
child with a non-zero status and fails the test.  The program puts a recognisable stand-in where the kernel's rows would be, so the
test sees which fields a row takes over and which the plan decides: for the job tables of tests/forced_cases.py against
tests/forced_ref.py (every status, a duplicate chain, more than seven neighbours with a tie in distance), n = 0, every argument
error with its message in the entry's order, and a table of 2^20 jobs."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import forced_cases as FC
import forced_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "caesar_yolo_amd", "csrc")
NULL, BAD_SHAPE, TOO_LARGE, BAD_NSIGMA, BAD_FIT_BKG, BAD_N = ("null argument", "MH, MW > 0 required", "image of 2^31 pixels or more", "nsigma outside [1, 8]",
                                                            "fit_bkg must be 0 or 1", "n outside 0 .. CY_FORCED_JOBS_MAX")
INF, NAN = float("inf"), float("nan")
PLAN_FIELDS = [3, 4, 5, 6, 17, 18, 19, 20, 21]


def stand_in(t):
    return [1000.0 * t + f + 0.5 for f in range(FR.FIELDS)]


def expected(MH, MW, jobs, nsigma=3.0, fit_bkg=1, nulls="-", n=None):
    """What forced_plan_main prints without COLS: the first line, the rows and the neighbour lists; the checks in the entry's order."""
    n = len(jobs) if n is None else n
    if "m" in nulls:
        return "error " + NULL, None, None
    if MH <= 0 or MW <= 0:
        return "error " + BAD_SHAPE, None, None
    if MH * MW >= 1 << 31:
        return "error " + TOO_LARGE, None, None
    if not 1.0 <= nsigma <= 8.0:
        return "error " + BAD_NSIGMA, None, None
    if fit_bkg not in (0, 1):
        return "error " + BAD_FIT_BKG, None, None
    if not 0 <= n <= FR.JOBS_MAX:
        return "error " + BAD_N, None, None
    if n > 0 and set(nulls) & set("jo"):
        return "error " + NULL, None, None
    if n == 0:
        return "ok 0", np.zeros((0, FR.FIELDS)), []
    plans = FR.plan(np.array(jobs, np.float64), nsigma, MH, MW)
    rows, t = np.zeros((n, FR.FIELDS)), 0
    for e, pl in enumerate(plans):
        if pl["status"] in (1, 3):
            rows[e, 0], rows[e, 17:21] = pl["status"], -1.0
            continue
        rows[e] = stand_in(t)
        nn = len(pl["neigh"])
        rows[e, PLAN_FIELDS] = [1 + nn + fit_bkg, nn, pl["crowded"], pl["ndup"], *pl["rect"], 1.0 if pl["status"] == 2 else 0.0]
        t += 1
    return "ok %d" % t, rows, [pl["neigh"] for pl in plans]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """The sanitized program, built once: the clang++ beside hipcc, else g++; no compiler is a failure."""
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    near = [os.path.join(os.path.dirname(hipcc), d, "clang++") for d in (".", "../llvm/bin", "../lib/llvm/bin")]
    cxx = next((c for c in near if os.path.exists(c)), None) or shutil.which("g++")
    assert cxx, "no clang++ beside hipcc and no g++: the planner cannot be checked"
    exe = str(tmp_path_factory.mktemp("forced_plan") / "forced_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "host", "forced_plan_main.cpp"), os.path.join(CSRC, "cy_measure_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(MH, MW, jobs, nsigma=3.0, fit_bkg=1, nulls="-", n=None, cols=None):
        n = len(jobs) if n is None else n
        text = " ".join(float(v).hex() if math.isfinite(v) else repr(float(v)) for j in jobs for v in j)
        r = subprocess.run([exe, str(MH), str(MW), str(n), repr(float(nsigma)), str(fit_bkg), nulls] + ([str(cols)] if cols else []), input=text,
                           capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, "%s: exit %d\n%s" % ((MH, MW, n, nsigma, fit_bkg, nulls, cols), r.returncode, r.stderr[-4000:])
        return r.stdout.strip().split("\n")
    return run


def rows_of(lines):
    return np.array([[float.fromhex(v) for v in line.split()] for line in lines], np.float64).reshape(-1, FR.FIELDS)


def both(planner, MH, MW, jobs, nsigma=3.0, fit_bkg=1, nulls="-", n=None):
    head, rows, neigh = expected(MH, MW, [list(j) for j in jobs], nsigma, fit_bkg, nulls, n)
    got = planner(MH, MW, jobs, nsigma, fit_bkg, nulls, n)
    assert got[0] == head, (MH, MW, nsigma, fit_bkg, nulls, n, got[0])
    if rows is None:
        assert len(got) == 1
    elif len(rows):
        assert np.array_equal(rows_of(got[1::2]), rows), (MH, MW, nsigma, fit_bkg)
        assert [[int(v) for v in line.split()[1:]] for line in got[2::2]] == neigh
    return head, rows, neigh


@pytest.mark.parametrize("g", [g for g in FC.groups() if g.name not in ("main_offset", "main_no_rms")], ids=lambda g: g.name)
def test_the_cases(planner, g):
    MH, MW = g.map.shape
    head, rows, neigh = both(planner, MH, MW, g.jobs.tolist(), g.nsigma, g.fit_bkg)
    # the fields the plan decides are those of the reference rows the GPU test compares with; the others are the kernel's, taken over
    ref = FR.forced_fit(g.map, g.rms, g.jobs, g.nsigma, g.fit_bkg)[0]
    run = np.isin(ref[:, 0], (0, 2, 4, 5))
    assert head == "ok %d" % int(run.sum())
    if not len(g.names):
        return
    assert np.array_equal(rows[:, PLAN_FIELDS], ref[:, PLAN_FIELDS])
    assert np.array_equal(rows[~run], ref[~run])              # statuses 1 and 3: the whole row is the host's
    for t, e in enumerate(np.nonzero(run)[0]):
        keep = [f for f in range(FR.FIELDS) if f not in PLAN_FIELDS]
        assert rows[e, keep].tolist() == [stand_in(t)[f] for f in keep]


def test_duplicates_ties_and_more_than_seven_neighbours(planner):
    g = FC.by_name("main_64x96")
    _, rows, neigh = both(planner, 64, 96, g.jobs.tolist())
    at = g.names.index
    assert neigh[at("dup2_0")] == [] and rows[at("dup2_0"), 6] == 1 and rows[at("dup2_1"), 6] == 1
    d3, dn = at("dup3_0"), at("dup3_neighbour")
    assert [neigh[d3 + t] for t in range(3)] == [[dn]] * 3 and neigh[dn] == [d3] and rows[dn, 6] == 2       # the chain: the second and third repeat a kept one
    c0 = at("crowd_0")
    assert all(len(neigh[c0 + t]) == 7 and rows[c0 + t, 5] == 1 and rows[c0 + t, 3] == 9 for t in range(10))
    assert neigh[c0][:2] == [c0 + 1, c0 + 2]                  # +-2.5 px: equal distances, the lower index first
    assert neigh[at("close_a")] == [at("close_b"), at("close_third")]
    # eight jobs on one spot and a ninth beside them: seven duplicates each, one neighbour
    same = [FC.job(10.0, 10.0, 1.5, 1.2, 0.3)] * 8 + [FC.job(12.0, 10.0)]
    _, rows, neigh = both(planner, 32, 32, same)
    assert rows[:8, 6].tolist() == [7.0] * 8 and neigh[:8] == [[8]] * 8 and neigh[8] == [0] and rows[8, 6] == 7


def test_every_status_on_other_shapes(planner):
    centres = [(0.0, 0.0), (3.5, 2.5), (-6.0, 0.0), (math.nextafter(-6.0, -INF), 0.0), (0.0, 1e300), (NAN, 0.0), (0.0, -INF), (8.25, 7.75), (-300.0, 3.0), (300.5, 290.0)]
    shapes = [(0.25, 0.0, 0.25, 0.0), (0.5, 0.2, 0.3, 1.0), (1e-6, 0.0, 1e-6, 0.0), (1e-6, 0.0, 0.25, 0.0), (0.0, 0.0, 0.25, 0.0), (-1.0, 0.0, 0.25, 0.0),
              (0.25, 0.25, 0.25, 0.0), (0.25, 0.3, 0.25, 0.0), (NAN, 0.0, 0.25, 0.0), (0.25, INF, 0.25, 0.0), (0.25, 0.0, 0.25, NAN), (0.25, 0.0, 0.25, INF),
              (5e-324, 0.0, 5e-324, 0.0), (1e300, 0.0, 1e300, 0.0)]
    jobs = [[x, y, a, b, c, bkg] for x, y in centres for a, b, c, bkg in shapes]
    for MH, MW in ((1, 1), (1, 7), (7, 1), (24, 31), (600, 700)):
        for nsigma in (1.0, 3.0, 8.0):
            _, rows, _ = both(planner, MH, MW, jobs, nsigma, 0)
            turned = rows[:, 17] < 0
            assert set(rows[turned, 0].astype(int)) == {1, 3} and (~turned).any()
    _, rows, _ = both(planner, 600, 700, jobs)
    assert (rows[:, 21] == 1).any() and (rows[:, 18] - rows[:, 17]).max() == 513            # capped: at most 514 columns
    assert both(planner, 9, 9, [])[0] == "ok 0"


def test_argument_errors_and_their_messages(planner):
    jobs = [FC.job(3.0, 4.0)]
    assert both(planner, 9, 9, jobs)[0] == "ok 1"
    for MH, MW in ((0, 9), (9, 0), (-1, 9), (9, -5), (0, 0)):
        assert both(planner, MH, MW, jobs)[0] == "error " + BAD_SHAPE
    for MH, MW in ((1 << 16, 1 << 15), (1 << 30, 2), ((1 << 31) - 1, (1 << 31) - 1), (46341, 46341), (2, 1 << 30)):
        assert both(planner, MH, MW, jobs)[0] == "error " + TOO_LARGE
    for nsigma in (0.0, math.nextafter(1.0, 0.0), math.nextafter(8.0, INF), -3.0, INF, NAN):
        assert both(planner, 9, 9, jobs, nsigma)[0] == "error " + BAD_NSIGMA
    for nsigma in (1.0, 8.0):
        assert both(planner, 9, 9, jobs, nsigma)[0] == "ok 1"
    for fb in (-1, 2, 7):
        assert both(planner, 9, 9, jobs, 3.0, fb)[0] == "error " + BAD_FIT_BKG
    for n in (-1, FR.JOBS_MAX + 1, -(1 << 31), (1 << 31) - 1):
        assert both(planner, 9, 9, [], n=n)[0] == "error " + BAD_N
    for nulls in ("m", "j", "o", "mjo", "jo"):
        assert both(planner, 9, 9, jobs, nulls=nulls)[0] == "error " + NULL
    assert both(planner, 9, 9, [], nulls="m")[0] == "error " + NULL      # the map is asked for even with n == 0
    assert both(planner, 9, 9, [], nulls="jo")[0] == "ok 0"              # n == 0: no host pointer is looked at
    # the order of the checks: map, shape, size, nsigma, fit_bkg, n, host pointers
    assert both(planner, 0, 9, [], 0.0, 2, "m", n=-1)[0] == "error " + NULL
    assert both(planner, 0, 1 << 30, [], 0.0, 2, "jo", n=-1)[0] == "error " + BAD_SHAPE
    assert both(planner, 1 << 16, 1 << 15, [], 0.0, 2, "jo", n=-1)[0] == "error " + TOO_LARGE
    assert both(planner, 9, 9, [], 0.0, 2, "jo", n=-1)[0] == "error " + BAD_NSIGMA
    assert both(planner, 9, 9, [], 3.0, 2, "jo", n=-1)[0] == "error " + BAD_FIT_BKG
    assert both(planner, 9, 9, [], 3.0, 1, "jo", n=-1)[0] == "error " + BAD_N
    # just below the limit of the image
    assert both(planner, 46340, 46340, [FC.job(46339.0, 46339.0, 0.5, 0.5)])[1][0, 17:21].tolist() == [46337, 46339, 46337, 46339]


def test_the_longest_job_table(planner):
    """2^20 jobs on a lattice of 65536 columns, made by the program: what the lattice gives is known in closed form.  Sigma 0.5 and
    nsigma 3 give half-widths of 2: a rectangle spans columns 5 ix - 2 .. 5 ix + 3 and rows 6 iy - 2 .. 6 iy + 3, so it shares one
    column with its neighbours in the row and no row with the rows beside it."""
    n, cols, rows_ = FR.JOBS_MAX, 65536, 16
    MH, MW = 6 * rows_, 5 * cols
    got = planner(MH, MW, [], 3.0, 1, n=n, cols=cols)
    i = np.arange(n)
    st1, st3 = i % 7 == 6, (i % 11 == 10) & (i % 7 != 6)       # status 1 is decided before status 3
    ok = ~(st1 | st3)
    ix, iy = i % cols, i // cols
    x0, x1 = np.maximum(5 * ix - 2, 0), np.minimum(5 * ix + 3, MW - 1)
    y0, y1 = np.maximum(6 * iy - 2, 0), np.minimum(6 * iy + 3, MH - 1)
    grid = ok.reshape(rows_, cols)
    nn = np.zeros((rows_, cols), np.int64)
    nn[:, 1:] += grid[:, :-1]
    nn[:, :-1] += grid[:, 1:]
    nn = nn.ravel()
    assert got[0] == "ok %d" % ok.sum()
    assert got[1] == "counts %d %d %d" % (ok.sum(), st1.sum(), st3.sum())
    assert got[2] == "sums %d %d %d 0 0" % (nn[ok].sum(), (x1 - x0 + 1)[ok].sum(), (y1 - y0 + 1)[ok].sum())
    assert got[3] == "wrong 0"
    shown = rows_of(got[4:])
    run_index = np.cumsum(ok) - 1
    for r, e in zip(shown, (0, 1, cols, n - 1)):
        if ok[e]:
            want = stand_in(int(run_index[e]))
            for f, v in zip(PLAN_FIELDS, [2.0 + nn[e], nn[e], 0, 0, x0[e], x1[e], y0[e], y1[e], 0]):
                want[f] = float(v)
            assert r.tolist() == want, e
        else:
            assert r[0] == (1 if st1[e] else 3) and r[17] == -1, e
    assert ok[0] and ok[1] and ok[cols] and shown.shape[0] == 4
