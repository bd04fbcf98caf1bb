"""The host-side planner of the measurement entries (caesar_yolo_amd/csrc/cy_measure_plan.cpp) on the CPU: box windows, the island
table, the fit and blend job tables with their lists and host-decided rows, and the messages of rejected inputs.  The planner is
linked into tests/host/measure_plan_main.cpp, built here with AddressSanitizer and UBSan and run as a child process, one case
file in, one result file out; a sanitizer report ends the child with a non-zero status and fails the test."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import blend_cases
import fit_cases
from caesar_yolo_amd import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "caesar_yolo_amd", "csrc")
MAXC, FIT_F, BLEND_F = 16, 32, 36
OFF_MSG = "h_mask_off disagrees with the areas of the box windows"
FIT_JOB = [("list_off", np.int64, 1), ("npos", np.uint32, 1), ("x0", np.int32, 1), ("y0", np.int32, 1), ("W", np.uint32, 1), ("A", np.uint32, 1),
           ("row", np.int32, 1), ("bkg", np.float64, 1), ("p0", np.float64, 6)]
BLEND_JOB = FIT_JOB[:6] + [("row0", np.int32, 1), ("M", np.int32, 1), ("comp", np.int32, 4), ("bkg", np.float64, 1), ("p0", np.float64, 24)]
OUTPUTS = {"sources": [("win", np.int32, 8)],
           "islands": [("win", np.int32, 4), ("off", np.int64, 2), ("totals", np.int64, 1)],
           "fit": FIT_JOB + [("list", np.uint32, 1), ("win0", np.int32, 2), ("large", np.int8, 1), ("back", np.float64, MAXC * FIT_F)],
           "blend": BLEND_JOB + [("list", np.uint32, 1), ("win0", np.int32, 2), ("rows", np.float64, MAXC * BLEND_F),
                                 ("back", np.float64, MAXC * BLEND_F)]}
OUTPUTS["deblend"] = OUTPUTS["islands"]


@pytest.fixture(scope="session")
def planner(tmp_path_factory):
    """The sanitized program, built once: the clang++ beside hipcc, else g++; no compiler is a failure."""
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    near = [os.path.join(os.path.dirname(hipcc), d, "clang++") for d in (".", "../llvm/bin", "../lib/llvm/bin")]
    cxx = next((c for c in near if os.path.exists(c)), None) or shutil.which("g++")
    assert cxx, "no clang++ beside hipcc and no g++: the planner cannot be checked"
    d = tmp_path_factory.mktemp("measure_plan")
    exe = str(d / "measure_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "host", "measure_plan_main.cpp"), os.path.join(CSRC, "cy_measure_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    count = [0]

    def run(mode, MH, MW, boxes, thr=None, ncomp=None, bkg=None, start=None, mask_off=None, mask=None, ring=0):
        """-> dict of the planner's arrays (one row per job / source), or the error message."""
        boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
        blobs = [boxes, thr, ncomp, bkg, start, mask_off, mask]
        types = [np.float64, np.float64, np.int32, np.float64, np.float64, np.int64, np.uint8]
        count[0] += 1
        case, res = str(d / ("case%d.bin" % count[0])), str(d / ("out%d.bin" % count[0]))
        with open(case, "wb") as f:
            f.write(struct.pack("<5i", MH, MW, len(boxes), ring, int(mask_off is not None)))
            for b, t in zip(blobs, types):
                raw = b"" if b is None else np.ascontiguousarray(b, t).tobytes()
                f.write(struct.pack("<q", len(raw)) + raw)
        r = subprocess.run([exe, mode, case, res], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, "%s: exit %d\n%s" % (mode, r.returncode, r.stderr[-4000:])
        raw = open(res, "rb").read()
        os.remove(case), os.remove(res)
        if struct.unpack_from("<i", raw)[0]:
            return raw[4:].decode()
        out, pos = {}, 4
        for name, t, width in OUTPUTS[mode]:
            nbytes = struct.unpack_from("<q", raw, pos)[0]
            a = np.frombuffer(raw, t, nbytes // np.dtype(t).itemsize, pos + 8)
            out[name] = a.reshape(-1, width) if width > 1 else a
            pos += 8 + nbytes
        assert pos == len(raw)
        return out
    return run


# ---- windows
def constructed_boxes(MH, MW):
    nan, inf = float("nan"), float("inf")
    b = [[nan, 5, 20, 30], [5, nan, 20, 30], [5, 5, nan, 30], [5, 5, 20, nan],                       # a NaN edge
         [-inf, 5, 20, 30], [5, -inf, 20, 30], [5, 5, inf, 30], [5, 5, 20, inf], [-inf, -inf, inf, inf], [inf, 5, inf, 30], [5, 5, -inf, 30],
         [-30, 5, -0.5, 30], [MW - 0.5, 5, MW + 30, 30], [5, -30, 20, -0.5], [5, MH - 0.5, 20, MH + 30],   # outside on each side
         [10.2, 5, 10.8, 30], [5, 10.2, 20, 10.8], [10.2, 10.2, 10.8, 10.8],                          # between two pixel centres
         [0, 0, 0, 0], [MW - 1, 0, MW - 1, 0], [0, MH - 1, 0, MH - 1], [MW - 1, MH - 1, MW - 1, MH - 1],   # 1 x 1 at each corner
         [-0.5, -0.5, 0.5, 0.5], [MW - 1.5, MH - 1.5, MW + 3, MH + 3],
         [0, 0, MW - 1, MH - 1], [-10, -10, MW + 10, MH + 10],                                        # the whole image
         [20, 30, 10, 40], [10, 40, 20, 30]]                                                          # x2 < x1, y2 < y1
    return np.array(b, np.float64)


def expected_windows(boxes, MH, MW):
    """win[n][4] {x0, x1, y0, y1} from measure.box_window."""
    out = []
    for b in boxes:
        x0, y0, h, w = measure.box_window(b, MH, MW)
        out.append([x0, x0 + w - 1, y0, y0 + h - 1] if h * w else [0, -1, 0, -1])
    return np.array(out, np.int32).reshape(-1, 4)


def all_boxes():
    MH, MW = fit_cases.MH, fit_cases.MW
    return np.concatenate([fit_cases.drawn()[1].arrays()[0], blend_cases.drawn()[1].arrays()[0], constructed_boxes(MH, MW)]), MH, MW


def test_windows_equal_box_window(planner):
    boxes, MH, MW = all_boxes()
    want = expected_windows(boxes, MH, MW)
    thr = np.tile([2.0, 1.0, 0.0, 2.0], (len(boxes), 1))
    for mode, stride in (("islands", 3), ("deblend", 4)):
        got = planner(mode, MH, MW, boxes, thr=thr[:, :stride])
        assert np.array_equal(got["win"], want), mode
    assert (want[:, 1] < want[:, 0]).sum() >= 15 and ((want[:, 1] == want[:, 0]) & (want[:, 3] == want[:, 2])).sum() >= 6
    for ring in (0, 8, 1000):
        got = planner("sources", MH, MW, boxes, ring=ring)["win"]
        assert np.array_equal(got[:, :4], want)
        grown = np.stack([np.maximum(0, want[:, 0] - ring), np.minimum(MW - 1, want[:, 1] + ring),
                          np.maximum(0, want[:, 2] - ring), np.minimum(MH - 1, want[:, 3] + ring)], 1)
        assert np.array_equal(got[:, 4:], grown)


def test_island_table_paths_and_running_sums(planner):
    """LDS up to 4096 pixels, a workspace offset from 4097, too large above 2^24; nws and nmask as running sums."""
    MH, MW = 4097, 4096
    boxes = np.array([[0, 0, 63, 63], [5, 0, 5, 4096], [100, 100, 99, 120], [10, 10, 109, 109], [0, 0, 4095, 4095], [0, 0, 4095, 4096],
                      [7, 7, 70, 70], [1, 1, 64, 65]], np.float64)
    area = np.array([4096, 4097, 0, 10000, 1 << 24, (1 << 24) + 4096, 4096, 64 * 65])
    for mode, stride in (("islands", 3), ("deblend", 4)):
        got = planner(mode, MH, MW, boxes, thr=np.tile([2.0, 2.0, 0.0, 0.0][:stride], (len(boxes), 1)))
        win = got["win"].astype(np.int64)
        assert np.array_equal(np.where(win[:, 1] < win[:, 0], 0, (win[:, 1] - win[:, 0] + 1) * (win[:, 3] - win[:, 2] + 1)), area)
        in_ws = (area > 4096) & (area <= 1 << 24)
        ws_off = np.cumsum(np.where(in_ws, area, 0)) - np.where(in_ws, area, 0)
        assert np.array_equal(got["off"][:, 0], np.where(area > 1 << 24, -2, np.where(in_ws, ws_off, -1)))
        assert np.array_equal(got["off"][:, 1], np.cumsum(area) - area)
        assert got["totals"].tolist() == [int(area[in_ws].sum()), int(area.sum())]
        assert got["off"][:, 0].tolist() == [-1, 0, -1, 4097, 14097, -2, -1, 14097 + (1 << 24)]


# ---- fit and blend jobs
def random_masks():
    """>= 200 label masks, 1 x 1 to 40 x 40 with one-row and one-column windows among them: bytes 0, 1 .. ncomp (components), ncomp + 1
    .. 16 (beyond ncomp: no component) and 255, as blocks of random size so that groups of every size occur."""
    rng = np.random.default_rng(31)
    shapes = [(1, 1), (1, 2), (2, 1), (1, 40), (40, 1), (1, 17), (23, 1), (40, 40), (2, 2), (3, 40), (40, 3)]
    shapes += [tuple(int(v) for v in rng.integers(1, 41, 2)) for _ in range(229)]
    line = np.array([[1, 2, 0, 3, 3, 4, 255, 2, 0, 1]], np.uint8)           # a one-row and a one-column window holding groups {0, 1} and {2, 3}
    masks, ncomp = [line, np.ascontiguousarray(line.T)], [4, 4]
    for t, (h, w) in enumerate(shapes):
        nc = int(rng.integers(0, 17)) if t % 8 else 16
        cell = int(rng.integers(1, 6))
        labels = rng.choice(np.arange(1, 17), int(rng.integers(1, 17)), replace=False)         # few labels: small groups
        values = np.concatenate([np.zeros(1 + int(rng.integers(0, 60))), labels, [255]]).astype(np.uint8)
        coarse = rng.choice(values, (-(-h // cell), -(-w // cell)))
        masks.append(np.ascontiguousarray(np.kron(coarse, np.ones((cell, cell), np.uint8))[:h, :w]))
        ncomp.append(nc)
    return masks, ncomp


def shelf_scene(masks, rng, MH=40):
    """Every mask as the window of its own box, side by side in one image; boxes with random sub-pixel edges around the windows."""
    x, boxes = 0, []
    for m in masks:
        h, w = m.shape
        e = rng.uniform(0.0, 0.99, 4)
        boxes.append([x - e[0], -e[1] if h < MH else -3.0, x + w - 1 + e[2], h - 1 + e[3]])
        x += w
    return np.array(boxes), MH, x


def fit_inputs(boxes, masks, ncomp, MH, MW, rng):
    for b, m in zip(boxes, masks):
        assert measure.box_window(b, MH, MW)[2:] == m.shape or m.size == 0
    off = np.concatenate([[0], np.cumsum([m.size for m in masks])]).astype(np.int64)
    mask = np.concatenate([m.reshape(-1) for m in masks]) if off[-1] else np.zeros(0, np.uint8)
    return dict(ncomp=np.asarray(ncomp, np.int32), bkg=rng.normal(size=len(masks)), mask_off=off, mask=mask)


def scenes():
    """[(name, MH, MW, boxes, ncomp, start, masks)]: the drawn cases of the fit and blend tests and the random masks."""
    rng = np.random.default_rng(32)
    out = []
    for name, mod in (("fit_drawn", fit_cases), ("blend_drawn", blend_cases)):
        boxes, _, ncomp, start, masks = mod.drawn()[1].arrays()
        out.append((name, fit_cases.MH, fit_cases.MW, boxes, ncomp, start, masks))
    masks, ncomp = random_masks()
    boxes, MH, MW = shelf_scene(masks, rng)
    out.append(("random", MH, MW, boxes, ncomp, rng.normal(50.0, 30.0, (len(masks), MAXC, 6)), masks))
    return out


def expected_back(host_rows, job_rows, start, win0, width, par):
    """What the entry returns when the device answers with the test program's made-up table (status r % 5, field f of row r =
    1000 r + f): the jobs' rows with the centre moved by the window origin, or, for status 3 and 4, the start as given."""
    out = np.array(host_rows, np.float64).reshape(-1, width)
    start = np.asarray(start, np.float64).reshape(-1, 6)
    for r in job_rows:
        out[r] = 1000.0 * r + np.arange(width)
        out[r, 0] = r % 5
        if r % 5 in (3, 4):
            out[r, par:par + 6] = start[r]
        else:
            out[r, par + 1:par + 3] += win0[r // MAXC]
    return out


def check_common(job, i, b, m, MH, MW, bkg):
    x0, y0, h, w = measure.box_window(b, MH, MW)
    want = (x0, y0, w, h * w) if h * w else (0, 0, 1, 1)
    assert (job["x0"], job["y0"], job["W"], job["A"]) == want and job["bkg"] == bkg[i]
    return x0, y0


def test_fit_jobs(planner):
    rng = np.random.default_rng(33)
    for name, MH, MW, boxes, ncomp, start, masks in scenes():
        inp = fit_inputs(boxes, masks, ncomp, MH, MW, rng)
        got = planner("fit", MH, MW, boxes, start=start, **inp)
        assert not isinstance(got, str), got
        assert len(got["row"]) == int(np.sum(ncomp)) and not got["large"].any(), name
        assert np.array_equal(got["win0"], expected_windows(boxes, MH, MW)[:, [0, 2]])
        j = at = 0
        for i, (b, m) in enumerate(zip(boxes, masks)):
            for k in range(int(ncomp[i])):
                job = {f: got[f][j] for f, _, _ in FIT_JOB}
                x0, y0 = check_common(job, i, b, m, MH, MW, inp["bkg"])
                want = np.flatnonzero(m.ravel() == k + 1)
                assert job["row"] == i * MAXC + k and job["list_off"] == at and job["npos"] == want.size, (name, i, k)
                assert np.array_equal(got["list"][at:at + want.size], want), (name, i, k)
                s = np.array(start[i][k], np.float64)
                s[1:3] -= (x0, y0)
                assert np.array_equal(job["p0"], s, equal_nan=True), (name, i, k)
                at += want.size
                j += 1
        assert at == got["list"].size
        want = expected_back(np.zeros((len(boxes) * MAXC, FIT_F)), got["row"], start, got["win0"], FIT_F, 5)
        assert np.array_equal(got["back"].reshape(-1, FIT_F), want, equal_nan=True), name


def diagonal_only_pairs(m, nc):
    """Pairs of components (indices) that touch through a diagonal and through no edge."""
    m = m.astype(np.int64)

    def pairs(a, b):
        ok = (a >= 1) & (a <= nc) & (b >= 1) & (b <= nc) & (a != b)
        return {(min(p, q) - 1, max(p, q) - 1) for p, q in zip(a[ok], b[ok])}
    edge = pairs(m[:, :-1], m[:, 1:]) | pairs(m[:-1, :], m[1:, :])
    return (pairs(m[:-1, :-1], m[1:, 1:]) | pairs(m[:-1, 1:], m[1:, :-1])) - edge


def test_blend_jobs(planner):
    rng = np.random.default_rng(34)
    seen = {"over": 0, "single": 0, "jobs": 0, "diagonal": 0, "row": 0, "column": 0}
    for name, MH, MW, boxes, ncomp, start, masks in scenes():
        inp = fit_inputs(boxes, masks, ncomp, MH, MW, rng)
        got = planner("blend", MH, MW, boxes, start=start, **inp)
        assert not isinstance(got, str), got
        rows = got["rows"].reshape(len(boxes), MAXC, BLEND_F)
        assert np.array_equal(got["win0"], expected_windows(boxes, MH, MW)[:, [0, 2]])
        j = at = 0
        for i, (b, m) in enumerate(zip(boxes, masks)):
            nc = int(ncomp[i])
            h, w = measure.box_window(b, MH, MW)[2:]
            groups = measure.blend_groups(m, h, w, nc)
            if name == "blend_drawn" and blend_cases.drawn()[1].names[i] in blend_cases.GROUPS:
                assert groups[:, 0].tolist() == blend_cases.GROUPS[blend_cases.drawn()[1].names[i]]
            want = np.zeros((MAXC, BLEND_F))
            want[:nc, 5:8] = groups
            want[:nc, 0] = np.where(groups[:, 1] == 1, 6.0, np.where(groups[:, 1] > 4, 5.0, 0.0))
            over = np.flatnonzero(groups[:, 1] > 4)
            want[over, 8:14] = np.asarray(start[i], np.float64)[over]
            assert np.array_equal(rows[i], want, equal_nan=True), (name, i)
            if name == "random":
                seen["over"] += over.size
                seen["single"] += int((groups[:, 1] == 1).sum())
                diag = diagonal_only_pairs(m, nc)
                seen["diagonal"] += sum(groups[p, 0] == groups[q, 0] for p, q in diag)
                seen["row"] += int(h == 1 and w > 1 and (groups[:, 1] > 1).any())
                seen["column"] += int(w == 1 and h > 1 and (groups[:, 1] > 1).any())
            for g in sorted(set(groups[(groups[:, 1] > 1) & (groups[:, 1] <= 4), 0].tolist())):
                members = np.flatnonzero(groups[:, 0] == g)
                job = {f: got[f][j] for f, _, _ in BLEND_JOB}
                x0, y0 = check_common(job, i, b, m, MH, MW, inp["bkg"])
                assert job["row0"] == i * MAXC and job["M"] == members.size and job["comp"][0] == g, (name, i, g)
                assert job["comp"][:members.size].tolist() == members.tolist() and not job["comp"][members.size:].any()
                lst = np.flatnonzero(np.isin(m.ravel(), members + 1))
                assert job["list_off"] == at and job["npos"] == lst.size and np.array_equal(got["list"][at:at + lst.size], lst), (name, i, g)
                s = np.zeros((4, 6))
                s[:members.size] = np.asarray(start[i], np.float64)[members]
                s[:members.size, 1:3] -= (x0, y0)
                assert np.array_equal(job["p0"].reshape(4, 6), s, equal_nan=True), (name, i, g)
                at += lst.size
                j += 1
                seen["jobs"] += name == "random"
        assert j == len(got["M"]) and at == got["list"].size, name
        job_rows = [r0 + c for r0, M, comp in zip(got["row0"], got["M"], got["comp"]) for c in comp[:M]]
        want = expected_back(got["rows"], job_rows, start, got["win0"], BLEND_F, 8)
        assert np.array_equal(got["back"].reshape(-1, BLEND_F), want, equal_nan=True), name
    # the random set holds what it is there for: groups above the limit, singletons, joint jobs, components joined through a
    # diagonal alone, and groups inside a one-row and inside a one-column window
    assert seen["over"] >= 20 and seen["single"] >= 100 and seen["jobs"] >= 50 and seen["diagonal"] >= 20 and seen["row"] >= 1 and seen["column"] >= 1, seen


@pytest.mark.parametrize("mode", ["fit", "blend"])
def test_window_above_the_largest_area(planner, mode):
    """A window of more than 2^24 pixels is byte-checked but collects nothing: no job, no list entry, status 1 for its components;
    the sources around it are planned as usual."""
    MH, MW = 4097, 4096
    rng = np.random.default_rng(37)
    small = np.array([[1, 2], [0, 2]], np.uint8)
    big = rng.choice(np.array([0, 1, 2, 3, 16, 255], np.uint8), (MH, MW))
    boxes = np.array([[10, 10, 11, 11], [-1, -1, MW, MH], [20, 20, 21, 21]], np.float64)
    masks, ncomp = [small, big, small], [2, 3, 2]
    start = rng.normal(50.0, 30.0, (3, MAXC, 6))
    inp = fit_inputs(boxes, masks, ncomp, MH, MW, rng)
    got = planner(mode, MH, MW, boxes, start=start, **inp)
    assert not isinstance(got, str), got
    assert got["win0"].tolist() == [[10, 10], [0, 0], [20, 20]]
    if mode == "fit":
        assert got["large"].tolist() == [0, 1, 0] and got["row"].tolist() == [0, 1, 2 * MAXC, 2 * MAXC + 1]
        assert got["list"].tolist() == [0, 1, 3, 0, 1, 3] and got["list_off"].tolist() == [0, 1, 3, 4] and got["A"].tolist() == [4] * 4
    else:
        rows = got["rows"].reshape(3, MAXC, BLEND_F)
        want = np.zeros((MAXC, BLEND_F))
        want[:3, 0] = 1.0
        assert np.array_equal(rows[1], want)
        assert got["row0"].tolist() == [0, 2 * MAXC] and got["M"].tolist() == [2, 2] and got["list"].tolist() == [0, 1, 3, 0, 1, 3]
        assert rows[0, :2, 5:8].tolist() == [[0, 2, 0], [0, 2, 1]] and np.array_equal(rows[0], rows[2])
    big[-1, -1] = 17                                         # its last byte is still looked at
    inp["mask"] = np.concatenate([m.reshape(-1) for m in masks])
    assert planner(mode, MH, MW, boxes, start=start, **inp) == "mask byte in 17 .. 254"


# ---- rejected inputs
def small_case(rng):
    masks = [np.array([[1, 2, 0], [0, 2, 255]], np.uint8), np.array([[3, 3], [16, 1]], np.uint8), np.array([[2]], np.uint8)]
    boxes, MH, MW = shelf_scene(masks, rng, MH=2)
    return masks, boxes, MH, MW, rng.normal(size=(3, MAXC, 6))


@pytest.mark.parametrize("mode", ["fit", "blend"])
def test_rejected_fit_inputs(planner, mode):
    rng = np.random.default_rng(35)
    masks, boxes, MH, MW, start = small_case(rng)

    def run(ncomp=(2, 3, 2), edit=None, off=None):
        ms = [m.copy() for m in masks]
        if edit:
            ms[edit[0]].ravel()[edit[1]] = edit[2]
        inp = fit_inputs(boxes, ms, ncomp, MH, MW, rng)
        if off is not None:
            inp["mask_off"] = inp["mask_off"] + np.asarray(off)
        return planner(mode, MH, MW, boxes, start=start, **inp)
    assert not isinstance(run(), str)
    assert not isinstance(run(edit=(1, 3, 16)), str) and not isinstance(run(edit=(2, 0, 255)), str) and not isinstance(run(ncomp=(0, 16, 0)), str)
    for byte in (17, 254, 100):
        for src, q in ((0, 0), (1, 3), (2, 0)):
            assert run(edit=(src, q, byte)) == "mask byte in 17 .. 254"
    for bad in (-1, 17):
        for src in range(3):
            nc = [2, 3, 2]
            nc[src] = bad
            assert run(ncomp=nc) == "h_ncomp outside 0 .. CY_DBL_MAX_COMP"
    for off in ([0, 0, 0, 1], [0, 0, 0, -1], [0, 1, 0, 0], [1, 1, 1, 1], [0, 0, -1, 0]):
        assert run(off=off) == OFF_MSG
    # the first failing source decides; within a source ncomp comes before the offsets and the offsets before the bytes
    assert run(ncomp=(2, 17, 2), off=[0, 0, 1, 0]) == "h_ncomp outside 0 .. CY_DBL_MAX_COMP"
    assert run(ncomp=(2, 3, 17), off=[0, 0, 1, 0]) == OFF_MSG
    assert run(edit=(1, 0, 17), off=[0, 0, 1, 0]) == OFF_MSG
    assert run(edit=(0, 0, 17), off=[0, 0, 1, 0]) == "mask byte in 17 .. 254"


@pytest.mark.parametrize("mode,stride", [("islands", 3), ("deblend", 4)])
def test_rejected_island_inputs(planner, mode, stride):
    rng = np.random.default_rng(36)
    masks, boxes, MH, MW, _ = small_case(rng)
    good_off = np.array([0, 6, 10, 11], np.int64)

    def run(low=(), off=None):
        thr = np.tile([3.0, 3.0, 0.5, 4.0][:stride], (3, 1))
        for i in low:
            thr[i, 0] = np.nextafter(3.0, 0.0)
        return planner(mode, MH, MW, boxes, thr=thr, mask_off=None if off is None else good_off + np.asarray(off))
    assert not isinstance(run(), str) and not isinstance(run(off=[0, 0, 0, 0]), str)
    for low in ((0,), (2,), (0, 2)):
        assert run(low=low) == "seed_thr below merge_thr" and run(low=low, off=[0, 0, 0, 0]) == "seed_thr below merge_thr"
    for off in ([0, 0, 0, 1], [0, 1, 0, 0], [-1, 0, 0, 0]):
        assert run(off=off) == OFF_MSG
    # a source's thresholds are looked at before its offsets; an earlier source's offsets before a later source's thresholds
    assert run(low=(1,), off=[0, 0, 1, 0]) == "seed_thr below merge_thr"
    assert run(low=(2,), off=[0, 0, 1, 0]) == OFF_MSG
    assert run(low=(2,), off=[0, 0, 0, 1]) == "seed_thr below merge_thr"
