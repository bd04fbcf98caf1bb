"""plan_peak_groups and peak_group_rows (caesar_yolo_amd/csrc/cy_measure_plan.cpp) on the CPU against the rules restated in
tests/peakgroup_ref.py with Python integers and a grid search of its own: links with the strict boundary and ties, groups, slots and
windows, the outside-neighbour lists, the starts relative to the group window, the rows the host writes, for the job tables of
tests/peakgroup_cases.py, images of one row or column and just below 2^31 pixels, every argument error with its message in the
planner's order, and a table of 70 000 jobs.  The planner is linked into tests/host/peakgroup_plan_main.cpp, built here with
AddressSanitizer and UBSan, as tests/test_peakfit_plan_cpu.py builds its own, and run as a child process; a sanitizer report ends the
child with a non-zero status and fails the test."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import peakfit_ref as PR
import peakgroup_cases as GC
import peakgroup_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "caesar_yolo_amd", "csrc")
BAD_SHAPE, TOO_LARGE, BAD_N, BAD_ITER, BAD_LINK, NULL = ("MH, MW > 0 required", "image of 2^31 pixels or more", "n outside 0 .. CY_PFIT_JOBS_MAX",
                                                          "max_iter outside 1 .. 256", "link outside (0, 2]", "null argument")
INF, NAN = float("inf"), float("nan")
START = [1.0, 0.0, 0.0, 0.25, 0.0, 0.25]
ROWS_MAX = 1000


def _hex(v):
    return float(v).hex() if math.isfinite(v) else repr(float(v))


def expected(MH, MW, jobs, link=1.5, max_iter=64, nulls="-", n=None, only=None):
    """What peakgroup_plan_main prints (without its last line); the checks in the planner's order.  only: the jobs whose outside
    lists are wanted (the group lines of groups with another member are None)."""
    n = len(jobs) if n is None else n
    if MH <= 0 or MW <= 0:
        return ["error " + BAD_SHAPE]
    if MH * MW >= 1 << 31:
        return ["error " + TOO_LARGE]
    if not 0 <= n <= PR.JOBS_MAX:
        return ["error " + BAD_N]
    if not 1 <= max_iter <= 256:
        return ["error " + BAD_ITER]
    if not (math.isfinite(link) and 0.0 < link <= 2.0):
        return ["error " + BAD_LINK]
    if n > 0 and set(nulls) & set("mjo"):
        return ["error " + NULL]
    if n == 0:
        return ["ok 0"]
    jobs = np.asarray(jobs, np.float64).reshape(n, PR.JOB_FIELDS)
    P = GR.plan(jobs, MH, MW, link, only)
    win, group, size, slot, status = P["win"], P["group"], P["size"], P["slot"], P["status"]
    ids = [g for g in range(n) if status[g] == 0 and group[g] == g]
    job_of = {g: t for t, g in enumerate(ids)}
    only_set = None if only is None else set(only)
    lines = ["ok %d" % len(ids)]
    lines += ["%d %d %d %d %d %d" % (status[e], group[e], size[e], slot[e], P["nlinked"][e], job_of[group[e]] if status[e] == 0 else -1) for e in range(n)]
    rows = np.zeros((n, GR.FIELDS))
    for e in range(n):
        rows[e, 0] = status[e]
        if status[e] in (1, 5):
            rows[e, 36:40] = -1.0
    members_of = {}
    for e in range(n):
        if status[e] in (0, 6, 7):
            members_of.setdefault(int(group[e]), []).append(e)
    for g, members in members_of.items():
        box = GR.group_window(win, members)
        for e in members:
            rows[e, 5:8] = [g, size[e], slot[e]]
            rows[e, 36:41], rows[e, 42] = box, P["nlinked"][e]
            if status[e] == 7:
                rows[e, 8:14] = jobs[e, 5:11]
    for t, g in enumerate(ids):
        members = members_of[g]
        x0, x1, y0, y1, _ = GR.group_window(win, members)
        if only_set is not None and not set(members) <= only_set:
            lines.append(None)
            continue
        parts = ["group %d %s %d %d %d %d %s %s" % (len(members), " ".join(str(m) for m in members + [-1] * (GR.MAX_MEMBERS - len(members))), x0, x1, y0, y1,
                                                 _hex(jobs[g, 3]), _hex(jobs[g, 4]))]
        for s, e in enumerate(members):
            out = [f for f in P["neigh"][e] if f not in members]
            parts.append("%d %s %s %s" % (len(out), " ".join(str(f) for f in out + [-1] * (PR.NEIGH_MAX - len(out))), _hex(jobs[e, 6] - float(x0)), _hex(jobs[e, 7] - float(y0))))
            rows[e, 0], rows[e, 41] = (0.0, 7.0) if t % 2 else (3.0, 7.0)
            rows[e, 8:14] = jobs[e, 5:11] if t % 2 == 0 else [9.0, 1.5 + float(x0), 2.5 + float(y0), 0.0, 0.0, 0.0]
        lines.append(" | ".join(parts))
    if n <= ROWS_MAX:
        lines += ["row " + " ".join(_hex(v) for v in r) for r in rows]
    return lines


def _canon(line):
    """A line of the program with its %a numbers in Python's spelling."""
    t = line.split()
    if t[0] == "row":
        return "row " + " ".join(_hex(float.fromhex(v) if "x" in v else float(v)) for v in t[1:])
    if t[0] != "group":
        return line
    out = []
    for k, v in enumerate(t):
        out.append(_hex(float.fromhex(v) if "x" in v else float(v)) if ("x" in v or v in ("nan", "inf", "-inf")) else v)
    return " ".join(out)


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """The sanitized program, built once: the clang++ beside hipcc, else g++; no compiler is a failure."""
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    near = [os.path.join(os.path.dirname(hipcc), d, "clang++") for d in (".", "../llvm/bin", "../lib/llvm/bin")]
    cxx = next((c for c in near if os.path.exists(c)), None) or shutil.which("g++")
    assert cxx, "no clang++ beside hipcc and no g++: the planner cannot be checked"
    exe = str(tmp_path_factory.mktemp("peakgroup_plan") / "peakgroup_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "host", "peakgroup_plan_main.cpp"), os.path.join(CSRC, "cy_measure_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(MH, MW, jobs, link=1.5, max_iter=64, nulls="-", n=None):
        n = len(jobs) if n is None else n
        text = " ".join(_hex(v) for j in jobs for v in j)
        r = subprocess.run([exe, str(MH), str(MW), str(n), str(max_iter), _hex(link), nulls], input=text, capture_output=True, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, "%s: exit %d\n%s" % ((MH, MW, n, link, max_iter, nulls), r.returncode, r.stderr[-4000:])
        lines = [_canon(line) for line in r.stdout.strip().split("\n")]
        ms = None
        if lines[-1].startswith("plan_ms"):
            ms = float(lines.pop().split()[1])
        return lines, ms
    return run


def both(planner, MH, MW, jobs, link=1.5, max_iter=64, nulls="-", n=None):
    want = expected(MH, MW, [list(j) for j in jobs], link, max_iter, nulls, n)
    got, _ = planner(MH, MW, jobs, link, max_iter, nulls, n)
    assert len(got) == len(want), (MH, MW, link, max_iter, nulls, n, got[:3], want[:3])
    for a, b in zip(got, want):
        assert a == b, (MH, MW, link, max_iter, nulls, n)
    return want


@pytest.mark.parametrize("g", GC.groups() + [GC.random(1)], ids=lambda g: g.name)
def test_the_cases(planner, g):
    MH, MW = g.map.shape
    want = both(planner, MH, MW, g.jobs.tolist(), g.link, g.max_iter)
    n = len(g.names)
    # the plan is that of the reference rows the GPU test compares with
    rows = GC.reference(g)[0][0]
    for e, line in enumerate(want[1:1 + n]):
        t = [int(v) for v in line.split()]
        assert t[0] == (0 if rows[e, 0] in (0, 2, 3, 4) else rows[e, 0])
        if t[0] not in (1, 5):
            assert t[1:4] == rows[e, 5:8].tolist() and t[4] == rows[e, 42]
    if g.name == "edge":
        ix = {nm: i for i, nm in enumerate(g.names)}
        st = lambda nm: [int(v) for v in want[1 + ix[nm]].split()]
        assert st("at_lm_a")[0] == st("at_lm_b")[0] == 6 and st("in_lm_a")[:3] == [0, ix["in_lm_a"], 2] and st("in_lm_b")[:4] == [0, ix["in_lm_a"], 2, 1]
        assert st("same_a")[4] == st("same_b")[4] == 1 and st("hole_near")[0] == 6 and st("chain5_2")[:5] == [7, ix["chain5_0"], 5, 2, 2]
        groups = {int(line.split()[2]): line for line in want[1 + n:] if line.startswith("group")}
        hole = groups[ix["hole_pair_a"]].split(" | ")
        assert hole[1].split()[:2] == ["1", str(ix["hole_near"])] and hole[2].split()[:2] == ["1", str(ix["hole_near"])]        # the hole is outside both
        share = groups[ix["share_a"]].split(" | ")
        assert share[1].split()[0] == "0" and share[2].split()[:2] == ["1", str(ix["share_out"])]


def test_links_ties_and_chains(planner):
    J = lambda x, y, R=6.0, sign=1.0: [x, y, R, 0.0, sign] + START
    st = lambda want, e: [int(v) for v in want[1 + e].split()]
    # the strict boundary on both axes and the diagonal (3-4-5 scaled: exactly 9), one ulp inside, and with link = 2 at 2 R
    jobs = [J(20.0, 20.0), J(29.0, 20.0), J(60.0, 20.0), J(60.0, 29.0), J(100.0, 20.0), J(105.4, 27.2), J(20.0, 60.0), J(math.nextafter(29.0, 0.0), 60.0)]
    want = both(planner, 100, 140, jobs)
    assert [st(want, e)[0] for e in range(8)] == [6, 6, 6, 6] + [st(want, 4)[0]] * 2 + [0, 0] and want[0] == "ok %d" % (1 + (st(want, 4)[0] == 0))
    want = both(planner, 100, 140, [J(20.0, 20.0), J(32.0, 20.0), J(60.0, 20.0), J(math.nextafter(72.0, 0.0), 20.0)], link=2.0)
    assert [st(want, e)[0] for e in range(4)] == [6, 6, 0, 0]
    # the larger radius decides, from either index order; different signs never link; coincident centres do
    want = both(planner, 100, 140, [J(20.0, 20.0, 2.0), J(30.0, 20.0, 8.0), J(60.0, 20.0, 8.0), J(70.0, 20.0, 2.0), J(100.0, 20.0), J(103.0, 20.0, sign=-1.0),
                                    J(20.0, 60.0), J(20.0, 60.0), J(60.0, 60.0, 6.0), J(60.0, 60.0, 6.0, sign=-1.0)])
    assert [st(want, e)[0] for e in range(10)] == [0, 0, 0, 0, 6, 6, 0, 0, 6, 6] and st(want, 7)[:5] == [0, 6, 2, 1, 1]
    # a chain of four is one job, of five none; a star of four around a centre is one job whose centre has three links
    chain = lambda k, y: [J(10.0 + 8.0 * t, y) for t in range(k)]
    want = both(planner, 100, 140, chain(4, 20.0) + chain(5, 50.0) + [J(60.0, 80.0), J(68.0, 80.0), J(52.0, 80.0), J(60.0, 88.0)])
    assert want[0] == "ok 2" and [st(want, e)[0] for e in range(13)] == [0] * 4 + [7] * 5 + [0] * 4
    assert st(want, 9)[4] == 3 and st(want, 3)[:5] == [0, 0, 4, 3, 1] and st(want, 8)[:4] == [7, 4, 5, 4]
    # groups interleaved in index order keep the lowest index as id and the index order as slots
    want = both(planner, 100, 140, [J(10.0, 20.0), J(60.0, 20.0), J(15.0, 20.0), J(65.0, 20.0), J(20.0, 20.0)])
    assert [st(want, e)[1:4] for e in range(5)] == [[0, 3, 0], [1, 2, 0], [0, 3, 1], [1, 2, 1], [0, 3, 2]]
    # a member's outside neighbours beyond eight: the kept ones of plan_peak_fits only; a job turned away is nobody's member
    ring = [J(52.0 + 11.5 * math.cos(a), 50.0 + 11.5 * math.sin(a), 1.0) for a in np.linspace(0.0, 2 * math.pi, 12, endpoint=False)]      # 9.5 px away at least
    want = both(planner, 100, 140, [J(50.0, 50.0), J(54.0, 50.0)] + ring + [J(52.0, 50.0, -1.0), J(NAN, 50.0)])
    assert st(want, 0)[:3] == [0, 0, 2] and st(want, 14)[0] == 1 and st(want, 15)[0] == 5


def test_shapes_of_one_row_or_column_and_just_below_2_31_pixels(planner):
    J = lambda x, y, R=4.0: [x, y, R, 0.0, 1.0] + START
    for MH, MW in ((1, 1), (1, 40), (40, 1)):
        want = both(planner, MH, MW, [J(0.0, 0.0), J(3.0, 0.0), J(0.0, 3.0), J(30.0, 0.0), J(0.0, 30.0), J(33.0, 2.0), J(200.0, 200.0)])
        assert want[0].startswith("ok ")
    big = (1 << 31) - 1
    for MH, MW in ((1, big), (big, 1), (2, (1 << 30) - 1), (32768, 65535), (46340, 46340)):
        lx, ly = float(MW - 1), float(MH - 1)
        jobs = [J(0.0, 0.0), J(3.0, 2.0), J(lx, ly), J(lx - 3.0, ly), J(lx + 2.0, ly + 2.0), J(lx / 2, ly / 2, 256.0), J(lx / 2 + 300.0, ly / 2, 256.0),
                J(lx / 2 + 600.0, ly / 2 + 1.0, 256.0), J(lx / 2 + 900.0, ly / 2, 256.0), J(lx + 257.0, ly, 256.0), J(4e9, 0.0)]
        want = both(planner, MH, MW, jobs)
        t = [int(v) for v in want[1 + 2].split()]
        assert t[0] == 0 and t[2] >= 2                          # the pair at the last pixel is a group (with the one beyond it, where that one is fitted)
        if MW >= 2000:                                          # a chain of four R = 256 discs 300 px apart: one job, 1413 columns wide
            wide = next(line for line in want if line.startswith("group 4 5 6 7 8"))
            x0, x1 = (int(v) for v in wide.split()[6:8])
            assert x1 - x0 in (1411, 1412)


def test_argument_errors_and_their_messages(planner):
    jobs = [[3.0, 4.0, 2.0, 0.0, 1.0] + START, [4.0, 4.0, 2.0, 0.0, 1.0] + START]
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
    for link in (0.0, -1.5, NAN, INF, -INF, math.nextafter(2.0, 3.0), 5e-324 * 0.0):
        assert both(planner, 9, 9, jobs, link=link) == ["error " + BAD_LINK]
        assert both(planner, 9, 9, [], link=link) == ["error " + BAD_LINK]            # also without a job
    for nulls in ("m", "j", "o", "mjo"):
        assert both(planner, 9, 9, jobs, nulls=nulls) == ["error " + NULL]
        assert both(planner, 9, 9, [], nulls=nulls) == ["ok 0"]                       # n == 0: no pointer is looked at
    # the order of the checks: shape, size, n, max_iter, link, pointers
    assert both(planner, 0, 9, [], 0.0, 0, "m", n=-1) == ["error " + BAD_SHAPE]
    assert both(planner, 1 << 16, 1 << 15, [], 0.0, 0, "m", n=-1) == ["error " + TOO_LARGE]
    assert both(planner, 9, 9, [], 0.0, 0, "m", n=-1) == ["error " + BAD_N]
    assert both(planner, 9, 9, jobs, 0.0, 0, "m") == ["error " + BAD_ITER]
    assert both(planner, 9, 9, jobs, 0.0, 1, "m") == ["error " + BAD_LINK]
    assert both(planner, 9, 9, jobs, 2.0, 1, "o") == ["error " + NULL]
    assert both(planner, 9, 9, jobs, 2.0, 256)[0] == "ok 1" and both(planner, 9, 9, jobs, 5e-324, 1)[0] == "ok 0"      # the limits themselves are in range


def test_a_long_job_table(planner):
    """70 000 jobs on 6000 x 6000, radii 1 .. 8, some turned away, holes among the peaks: every status, group, size, slot and link
    count against the restatement, the group jobs whose members are among every 97th job and their neighbours in full, and the
    planner's own time.  A search that compared every pair would need 4.9e9 distance tests."""
    rng = np.random.default_rng(70001)
    n = 70000
    jobs = np.zeros((n, PR.JOB_FIELDS))
    jobs[:, 0], jobs[:, 1] = rng.uniform(-8.0, 6008.0, n), rng.uniform(-8.0, 6008.0, n)
    jobs[:, 2] = rng.integers(1, 9, n).astype(np.float64)
    jobs[:, 4], jobs[:, 5:] = np.where(rng.uniform(size=n) < 0.2, -1.0, 1.0), START
    jobs[rng.integers(0, n, 700), 2] = -1.0
    jobs[rng.integers(0, n, 700), 0] = NAN
    jobs[:n // 2:1000, :2] = jobs[1:n // 2:1000, :2]                                     # coincident pairs
    P = GR.plan(jobs, 6000, 6000, 1.5, only=[])
    picked = sorted({int(m) for e in range(0, n, 97) if P["status"][e] == 0 for m in np.nonzero(P["group"] == P["group"][e])[0]})
    want = expected(6000, 6000, jobs.tolist(), only=picked)
    got, ms = planner(6000, 6000, jobs.tolist())
    assert len(got) == len(want) and got[:1 + n] == want[:1 + n]
    checked = 0
    for a, b in zip(got[1 + n:], want[1 + n:]):
        if b is not None:
            assert a == b
            checked += 1
    sizes = np.bincount(P["size"][(P["status"] != 1) & (P["status"] != 5) & (P["slot"] == 0)])
    print("plan_peak_groups: %d jobs in %.0f ms (sanitized build); groups by size %s, %d group jobs compared in full" % (n, ms, sizes.tolist(), checked))
    assert checked >= 100 and sizes[2:5].sum() >= 5000 and sizes[5:].sum() >= 50, "the table is meant to hold groups of every size"
    assert ms < 10000.0, "the planner took %.0f ms for %d jobs: a quadratic search?" % (ms, n)
