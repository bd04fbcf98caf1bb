"""cy_deblend_islands on the GPU against the numpy / explicit-walk reference (tests/deblend_ref.py) on the 2048 x 2048 synthetic
mosaic of tests/test_gpu_islands.py (same recipe: NaN strip on the right, all-zero block in the middle) with windows of its own
drawn in, blended pairs (two stamps 3 to 6 pixels apart) and one crowded field.

Thresholds: bkg + 5 rms / bkg + 2.5 rms / bkg + 5 rms from the REFERENCE's measurement rows (tests/measure_ref.py, ring 8) unless a
constructed case says otherwise.  Comparison, for EVERY source (none skipped):
  mask bytes equal; every field of the row and npix, peak, x_peak, y_peak, main, nsummits of every component row equal: they are
  sets, counts and selections; rows at and beyond ncomp zero;
  S Sx Sy Sxx Syy Sxy   both sides add the same float64 terms in some order, so |gpu - ref| <= 2 m 2^-53 sum|t_i| with m = npix
                        of the component and sum|t_i| from the reference.  Derived, not tuned;
  npix equal to field [3] of cy_measure_islands on the GPU for the same boxes and thresholds."""
import ctypes as C

import numpy as np
import pytest
import torch

import deblend_ref
import island_ref
import measure_ref
from gpu_common import detector

pytestmark = pytest.mark.gpu

N = 2048
LDS_MAX = 4096                               # windows of up to this many pixels keep their two words per pixel in LDS
LO = np.float32(0.01)
DRAWN_THR = [0.5, 0.2, 0.0, 0.5]             # seed, merge, bkg, peak of the drawn windows: LO is nothing
STEP = np.float32(2.0 ** -20)                # ramp step: every 0.25 + k * STEP below 0.5 is an fp32 number


def serpentine_path(n):
    """(y, x) of the pixels of tests/test_gpu_islands.py's n x n serpentine in path order, from [0, 0] to its far end."""
    path, right = [], True
    for y in range(0, n, 2):
        xs = range(n) if right else range(n - 1, -1, -1)
        path += [(y, x) for x in xs]
        if y + 1 < n:
            path.append((y + 1, n - 1 if right else 0))
        right = not right
    return path


def ramp(n):
    a = np.full((n, n), LO, np.float32)
    for k, (y, x) in enumerate(serpentine_path(n)):
        a[y, x] = np.float32(0.25) + np.float32(k) * STEP
    return a


def strip(vals):
    """3 x (len + 2) window: the values in the middle row, LO around them."""
    a = np.full((3, len(vals) + 2), LO, np.float32)
    a[1, 1:-1] = np.array(vals, np.float32)
    return a


G = float(LO)
BUMPS5 = strip([.3, .6, .9, .6, .3, .3, .6, .8, .6, .3])                 # peaks 5 apart, saddle 0.3
BUMPS2 = strip([.3, .9, .6, .8, .3])                                     # peaks 2 apart
EQUI = strip([.9, .3, .5, .3, .8])                                       # the 0.5 summit is 2 from both peaks
TWO_ISL = strip([.9, .3, G, G, .6, .3])                                  # the second island's top is below 0.85
PEAKS17 = strip(sum(([0.9 - 0.01 * k, .3, .3] for k in range(17)), []))  # 17 peaks 3 apart in one island
U_SHAPE = np.full((5, 5), LO, np.float32)
U_SHAPE[1:4, 1] = U_SHAPE[1:4, 3] = U_SHAPE[3, 1:4] = np.float32(0.9)
LATTICE = np.full((11, 11), LO, np.float32)
LATTICE[1::2, 1::2] = np.float32(0.6) + np.arange(25, dtype=np.float32).reshape(5, 5) / 128
DIAGONAL = np.full((8, 8), LO, np.float32)
DIAGONAL[1:3, 1:3] = DIAGONAL[3:5, 3:5] = np.float32(0.3)
DIAGONAL[1, 1] = DIAGONAL[4, 4] = np.float32(0.9)
DRAWN = {  # name -> (array, row, column)
    "bumps5": (BUMPS5, 1600, 100), "bumps2": (BUMPS2, 1600, 120), "equi": (EQUI, 1600, 140), "two_isl": (TWO_ISL, 1600, 160),
    "u": (U_SHAPE, 1610, 120), "lattice": (LATTICE, 1630, 100), "peaks17": (PEAKS17, 1630, 120), "diagonal": (DIAGONAL, 1630, 230),
    "ramp63": (ramp(63), 1650, 100), "ramp301": (ramp(301), 1720, 100),
}


def box_of(name):
    a, y, x = DRAWN[name]
    return [float(x), float(y), float(x + a.shape[1] - 1), float(y + a.shape[0] - 1)]


def stamp(img, cy, cx, amp, sigma=1.2):
    y0, x0 = int(round(cy)), int(round(cx))
    yy, xx = np.mgrid[y0 - 5:y0 + 6, x0 - 5:x0 + 6]
    img[y0 - 5:y0 + 6, x0 - 5:x0 + 6] += (amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sigma * sigma))).astype(np.float32)


def make_image():
    from caesar_yolo_amd import synth
    img = synth.make_mosaic(n=N, seed=7)                  # NaN strip: columns 1984..2047; zero block: [1024, 1536) x [1024, 1536)
    img[300:303, 400:405] = np.float32(0.25)              # the stamps of tests/test_gpu_measure.py::scene
    img[310, 420] = img[312, 418] = np.float32(0.5)
    img[600:640, 700:740] = np.float32(0.125)
    img[1200:1203, 1100:1103] = np.float32(0.75)
    img[800, 800] = np.float32(-1.0)
    # blended pairs and one crowded field, in units of the noise of the upper left quarter
    q = img[:1000, :1000].astype(np.float64)
    noise = np.float32(1.4826 * np.median(np.abs(q - np.median(q))))
    rng = np.random.default_rng(11)
    for _ in range(400):
        cy, cx = rng.uniform(20, 1000), rng.uniform(20, 1950)
        ang, sep = rng.uniform(0, np.pi), rng.uniform(3, 6)
        a1, a2 = rng.uniform(15, 60, 2) * noise
        stamp(img, cy, cx, a1)
        stamp(img, cy + sep * np.sin(ang), cx + sep * np.cos(ang), a2)
    for _ in range(150):                                  # crowded field [1100, 1250) x [200, 350)
        stamp(img, rng.uniform(1100, 1250), rng.uniform(200, 350), rng.uniform(15, 60) * noise)
    holes = np.random.default_rng(3).integers(0, N, (40000, 2))
    holes = holes[holes[:, 0] >= 1040]
    img[holes[:, 0], holes[:, 1]] = 0.0
    img[1005, 30] = 0.0
    img[1620:1630, 200:210] = np.float32(0.25)            # plateau
    for a, y, x in DRAWN.values():
        img[y:y + a.shape[0], x:x + a.shape[1]] = a
    return img


@pytest.fixture(scope="module")
def scene():
    img = make_image()
    host = np.where(np.isfinite(img), img, np.float32(0)).astype(np.float32)     # what cy_mosaic_prepare leaves
    det = detector("fp32", max_batch=1, max_imgsz=160)
    dev = det.mosaic_to_device(img)
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), host)
    return det, dev, host


def compare(got, gcomp, gmasks, ref, rcomp, rmasks, mags, what):
    """-> the largest |diff| / bound over the sums."""
    assert got.shape == ref.shape and gcomp.shape == rcomp.shape and len(gmasks) == len(rmasks) == ref.shape[0]
    worst = 0.0
    for i in range(ref.shape[0]):
        assert gmasks[i].shape == rmasks[i].shape and gmasks[i].dtype == np.uint8, "%s, source %d: mask shape %s, reference %s" % (
            what, i, gmasks[i].shape, rmasks[i].shape)
        assert gmasks[i].tobytes() == rmasks[i].tobytes(), "%s, source %d: %d mask bytes differ" % (what, i, (gmasks[i] != rmasks[i]).sum())
        for f in range(len(deblend_ref.FIELDS)):
            assert got[i, f] == ref[i, f], "%s, source %d: %s = %r on the GPU, %r in the reference" % (
                what, i, deblend_ref.FIELDS[f], got[i, f], ref[i, f])
        nc = int(ref[i, 3])
        assert not gcomp[i, nc:].any(), "%s, source %d: a component row at or beyond ncomp = %d is not zero" % (what, i, nc)
        for k in range(nc):
            for f in (0, 1, 2, 3, 10, 11):
                assert gcomp[i, k, f] == rcomp[i, k, f], "%s, source %d, component %d: %s = %r on the GPU, %r in the reference" % (
                    what, i, k, deblend_ref.COMP_FIELDS[f], gcomp[i, k, f], rcomp[i, k, f])
            m = rcomp[i, k, 0]
            for f, mag in zip(deblend_ref.SUMS, mags[i, k]):
                bound = 2.0 * m * 2.0 ** -53 * mag
                diff = abs(gcomp[i, k, f] - rcomp[i, k, f])
                assert diff <= bound, "%s, source %d, component %d: %s = %r on the GPU, %r in the reference, |diff| %g > bound %g (m = %d)" % (
                    what, i, k, deblend_ref.COMP_FIELDS[f], gcomp[i, k, f], rcomp[i, k, f], diff, bound, m)
                if bound > 0:
                    worst = max(worst, diff / bound)
    return worst


def run_and_compare(det, dev, host, boxes, thr4, conn, radius, what, ref=None):
    boxes, thr4 = np.asarray(boxes, np.float64), np.asarray(thr4, np.float64)
    ref = ref or deblend_ref.deblend(host, boxes, thr4, conn, radius)
    got, gcomp, gmasks = det.deblend_islands(dev, boxes, thr4, conn=conn, radius=radius, return_masks=True)
    ms = det.deblend_kernel_ms()
    worst = compare(got, gcomp, gmasks, ref[0], ref[1], ref[2], ref[3], what)
    isl = det.measure_islands(dev, boxes, thr4[:, :3], conn=conn)
    assert np.array_equal(got[:, 4], isl[:, 3]), "%s: npix differs from cy_measure_islands" % what
    rows_only, comp_only = det.deblend_islands(dev, boxes, thr4, conn=conn, radius=radius)    # without the mask output: the same rows
    assert rows_only.tobytes() == got.tobytes() and comp_only.tobytes() == gcomp.tobytes()
    return ref, worst, ms


def sigma_thresholds(host, boxes):
    meas, _ = measure_ref.measure(host, boxes, 8)
    return deblend_ref.thresholds(meas, 5.0, 2.5, 5.0)


def drawn_cases():
    """name -> (box, thresholds, radius)"""
    t = DRAWN_THR
    flat = [0.25, 0.25, 0.0, 0.25]
    return {
        "two bumps with a saddle": (box_of("bumps5"), t, 2),
        "two bumps, peaks within r": (box_of("bumps2"), t, 2),
        "two bumps, peaks within 2, radius 1": (box_of("bumps2"), t, 1),
        "two bumps, radius 8": (box_of("bumps5"), t, 8),
        "flat plateau": ([198.0, 1618.0, 211.0, 1631.0], flat, 2),
        "U-shaped plateau": (box_of("u"), t, 2),
        "summit equidistant from two kept peaks": (box_of("equi"), t, 2),
        "two islands, one below peak_thr": (box_of("two_isl"), [0.5, 0.2, 0.0, 0.85], 2),
        "two bumps, peak_thr NaN": (box_of("bumps5"), [0.5, 0.2, 0.0, np.nan], 2),
        "two bumps, peak_thr +inf": (box_of("bumps5"), [0.5, 0.2, 0.0, np.inf], 2),
        "lattice of 25 isolated seeds": (box_of("lattice"), t, 1),
        "17 peaks in one island": (box_of("peaks17"), t, 2),
        "ramp serpentine 63": (box_of("ramp63"), flat, 2),
        "ramp serpentine 301": (box_of("ramp301"), flat, 2),
        "diagonal touch": (box_of("diagonal"), t, 2),
    }


def check_drawn(name, conn, row, comp, mask):
    """The cases are what their names say (on the reference side, so that a wrong construction fails here and not silently)."""
    r = dict(zip(deblend_ref.FIELDS, row))
    counts = (r["status"], r["nsummits"], r["npeaks"], r["ncomp"], r["npix"], r["npix_unassigned"])
    if name in ("two bumps with a saddle", "two bumps, peaks within 2, radius 1"):
        assert counts == (0, 2, 2, 2, mask.shape[1] - 2, 0) and comp[0, 1] == np.float32(.9) and comp[1, 1] == np.float32(.8)
        assert comp[0, 10] == comp[1, 10] == 1 and comp[0, 11] == comp[1, 11] == 1
    elif name in ("two bumps, peaks within r", "two bumps, radius 8", "two bumps, peak_thr NaN", "two bumps, peak_thr +inf"):
        assert counts == (0, 2, 1, 1, mask.shape[1] - 2, 0) and comp[0, 11] == 2 and set(mask[1, 1:-1].tolist()) == {1}
    elif name == "flat plateau":
        assert counts == (0, 1, 1, 1, 100, 0) and (comp[0, 2], comp[0, 3]) == (200, 1620)       # ties by index: the first pixel
    elif name == "U-shaped plateau":
        assert counts == (0, 2, 1, 1, 7, 0) and (comp[0, 2], comp[0, 3]) == (121, 1611)
    elif name == "summit equidistant from two kept peaks":
        assert counts == (0, 3, 2, 2, 5, 0) and mask[1].tolist() == [0, 1, 1, 1, 2, 2, 0] and comp[0, 11] == 2 and comp[1, 11] == 1
    elif name == "two islands, one below peak_thr":
        assert counts == (0, 2, 2, 2, 4, 0) and comp[1, 1] == np.float32(.6) and comp[0, 10] == 1 and comp[1, 10] == 0
    elif name == "lattice of 25 isolated seeds":
        assert counts == (2, 25, 25, 16, 25, 9) and (mask == 255).sum() == 9 and comp[15, 0] == 1
    elif name == "17 peaks in one island":
        assert counts == (2, 17, 17, 16, 51, 0) and comp[15, 11] == 2 and comp[:, 11].sum() == 17 and comp[:, 10].sum() == 16
    elif name.startswith("ramp serpentine"):
        n = mask.shape[0]
        assert counts == (0, 1, 1, 1, (n + 1) // 2 * n + n // 2, 0) and comp[0, 11] == 1
        ey, ex = serpentine_path(n)[-1]
        assert (comp[0, 2] - 100, comp[0, 3] - (1650 if n == 63 else 1720)) == (ex, ey)
    elif name == "diagonal touch":
        # conn 4: the corner pixel of the lower block sees only equal neighbours with a higher index: a third summit
        assert counts == (0, 2 if conn == 8 else 3, 2, 2, 8, 0) and comp[0, 10] == 1 and comp[1, 10] == (1 if conn == 8 else 0)
    else:
        raise AssertionError(name)


def scene_boxes():
    """The scene boxes of tests/test_gpu_islands.py, with the 5 / 2.5 / 5 sigma thresholds of the reference's own bkg and rms."""
    return {
        "across the NaN strip": [1960.0, 900.0, 2010.0, 930.0],
        "across the zero block's edge": [1000.0, 1000.0, 1060.0, 1050.0],
        "inside the zero block": [1300.0, 1300.0, 1330.0, 1320.0],
        "island in the zero block (blank ring)": [1100.0, 1200.0, 1102.0, 1202.0],
        "partly outside, left top": [-15.5, -7.25, 9.5, 11.0],
        "partly outside, right bottom": [N - 90.0, N - 12.0, N + 40.0, N + 30.0],
        "wholly outside, left": [-50.0, 100.0, -20.0, 130.0],
        "wholly outside, far": [-1e12, -1e12, -1e11, -1e11],
        "fractional, no pixel centre in x": [100.2, 200.0, 100.8, 210.0],
        "one pixel": [50.0, 60.0, 50.0, 60.0],
        "peak tie in one block": [395.0, 295.0, 410.0, 306.0],
        "peak tie across rows": [410.0, 305.0, 425.0, 315.0],
        "64 x 64: the largest LDS window": [700.0, 100.0, 763.0, 163.0],
        "65 x 64: the smallest workspace window": [700.0, 200.0, 764.0, 263.0],
        "large window": [200.5, 300.5, 1700.0, 1500.0],
        "whole image": [-3.0, -3.0, N + 3.0, N + 3.0],
    }


@pytest.mark.parametrize("conn", [8, 4])
def test_constructed_windows(scene, conn):
    det, dev, host = scene
    cases = drawn_cases()
    assert 63 * 63 <= LDS_MAX < 301 * 301
    for radius in sorted({v[2] for v in cases.values()}):
        names = [k for k, v in cases.items() if v[2] == radius]
        (rows, comps, masks, _), worst, ms = run_and_compare(det, dev, host, [cases[k][0] for k in names], [cases[k][1] for k in names],
                                                             conn, radius, "conn %d, radius %d" % (conn, radius))
        for i, k in enumerate(names):
            check_drawn(k, conn, rows[i], comps[i], masks[i])
        print("conn %d, radius %d: %d drawn windows equal; kernel %.3f ms" % (conn, radius, len(names), ms))


@pytest.mark.parametrize("conn", [8, 4])
def test_scene_boxes(scene, conn):
    det, dev, host = scene
    named = scene_boxes()
    boxes = np.array(list(named.values()), np.float64)
    (rows, comps, masks, _), worst, ms = run_and_compare(det, dev, host, boxes, sigma_thresholds(host, boxes), conn, 2, "scene, conn %d" % conn)
    r = {k: dict(zip(deblend_ref.FIELDS, rows[i])) for i, k in enumerate(named)}
    rm = dict(zip(named, masks))
    for k in named:
        if k.startswith("wholly outside") or k.startswith("fractional"):
            assert rm[k].shape == (0, 0) and not rows[list(named).index(k)].any()
    assert rm["across the NaN strip"].shape == (31, 51) and not rm["across the NaN strip"][:, 24:].any()
    assert rm["across the zero block's edge"].shape == (51, 61) and not rm["across the zero block's edge"][24:, 24:].any()
    assert r["inside the zero block"]["ncomp"] == 0 and rm["inside the zero block"].size == 31 * 21
    d = r["island in the zero block (blank ring)"]                # a 3 x 3 plateau: ties by index, one summit
    assert (d["nsummits"], d["ncomp"], d["npix"]) == (1, 1, 9)
    assert rm["64 x 64: the largest LDS window"].size == LDS_MAX and rm["65 x 64: the smallest workspace window"].size == LDS_MAX + 64
    assert rm["large window"].shape == (1200, 1500) and r["large window"]["status"] == 2 and r["large window"]["npeaks"] > 50
    assert rm["whole image"].shape == (N, N) and r["whole image"]["npix"] > 1000000 and r["whole image"]["status"] == 2
    assert (rows[:, 0] != 1).all()                                 # the supported maximum (2^24 pixels) is above the whole image
    print("conn %d: %d scene boxes equal, largest |diff| / bound of the sums %.3g; kernel %.3f ms" % (conn, len(named), worst, ms))


def random_boxes():
    rng = np.random.default_rng(20261017)
    n = 2000
    w, h = rng.integers(3, 201, n), rng.integers(3, 201, n)
    x1, y1 = rng.uniform(-40, N + 20, n), rng.uniform(-40, N + 20, n)
    frac = rng.random(n) < 0.5
    x1, y1 = np.where(frac, x1, np.floor(x1)), np.where(frac, y1, np.floor(y1))
    return np.stack([x1, y1, x1 + w, y1 + h], 1)


# measured on the reference (conn 8 / conn 4): sources with two or more components, with a summit that is no kept peak, with status 2
FLOORS = {8: (800, 700, 70), 4: (800, 850, 70)}             # measured: 859 / 795 / 81 and 861 / 963 / 81


@pytest.mark.parametrize("conn", [8, 4])
def test_random_boxes(scene, conn):
    det, dev, host = scene
    boxes = random_boxes()
    thr4 = sigma_thresholds(host, boxes)
    ref = deblend_ref.deblend(host, boxes, thr4, conn, 2)
    rows = ref[0]
    multi, demoted, trunc = int((rows[:, 3] >= 2).sum()), int((rows[:, 1] > rows[:, 3]).sum()), int((rows[:, 0] == 2).sum())
    print("conn %d: %d of 2000 reference sources with two or more components, %d with a demoted summit, %d with status 2" % (conn, multi, demoted, trunc))
    f = FLOORS[conn]
    assert min(f) > 0 and multi >= f[0] and demoted >= f[1] and trunc >= f[2]
    assert (rows[:, 0] != 1).all()
    _, worst, ms = run_and_compare(det, dev, host, boxes, thr4, conn, 2, "random, conn %d" % conn, ref=ref)
    lds = sum(m.size <= LDS_MAX for m in ref[2])
    print("conn %d: 2000 random boxes (%d in LDS): masks, counts and peaks equal, largest |diff| / bound of the sums %.3g; kernel %.3f ms" % (
        conn, lds, worst, ms))


def test_arguments_and_determinism(scene):
    det, dev, host = scene
    from caesar_yolo_amd import lib as L
    from caesar_yolo_amd import measure
    lib = L.load()
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
    named = scene_boxes()
    boxes = np.array(list(named.values())[:-2], np.float64)        # without the two large windows
    n = boxes.shape[0]
    thr = np.ascontiguousarray(sigma_thresholds(host, boxes))
    out = np.zeros((n, L.CY_DBL_FIELDS), np.float64)
    comp = np.zeros((n, L.CY_DBL_MAX_COMP, L.CY_DBL_COMP_FIELDS), np.float64)
    off = np.zeros(n + 1, np.int64)
    np.cumsum([np.prod(measure.box_window(b, N, N)[2:]) for b in boxes], out=off[1:])
    mask = np.zeros(int(off[-1]), np.uint8)
    args = lambda n=n, conn=8, radius=2, img=dev.data_ptr(), mh=N, mw=N, b=boxes.ctypes.data_as(dp), t=thr.ctypes.data_as(dp), \
        o=out.ctypes.data_as(dp), c=comp.ctypes.data_as(dp), m=C.c_void_p(mask.ctypes.data), f=off.ctypes.data_as(lp), ctx=det.ctx: (
            ctx, C.c_void_p(img), mh, mw, b, t, n, conn, radius, o, c, m, f, det._stream())
    assert lib.cy_deblend_islands(*args()) == 0
    assert lib.cy_deblend_islands(*args(m=None, f=None)) == 0                     # no mask wanted
    rows, comps, masks = det.deblend_islands(dev, np.zeros((0, 4)), np.zeros((0, 4)), return_masks=True)
    assert rows.shape == (0, L.CY_DBL_FIELDS) and comps.shape == (0, L.CY_DBL_MAX_COMP, L.CY_DBL_COMP_FIELDS) and masks == []
    assert lib.cy_deblend_islands(*args(n=0)) == 0                                # CY_OK, nothing launched
    bad_row0 = thr.copy(); bad_row0[0, 0], bad_row0[0, 1] = 1.0, 2.0
    assert lib.cy_deblend_islands(*args(n=0, t=bad_row0.ctypes.data_as(dp))) == 0 # n == 0 is answered before the rows are read
    assert lib.cy_deblend_islands(*args(n=0, b=None, t=None, o=None, c=None, img=None)) == 0
    assert lib.cy_deblend_islands(*args(t=bad_row0.ctypes.data_as(dp))) == -1
    assert lib.cy_deblend_islands(*args(mh=65536, mw=32768)) == -1                # an image of 2^31 pixels: refused before anything is read
    assert lib.cy_deblend_islands(*args(mh=32768, mw=65536, m=None, f=None)) == -1
    for bad in (dict(conn=6), dict(conn=0), dict(radius=0), dict(radius=9), dict(radius=-1), dict(mh=0), dict(mw=-5), dict(img=None), dict(b=None),
                dict(t=None), dict(o=None), dict(c=None), dict(ctx=None), dict(n=-3), dict(f=None)):
        assert lib.cy_deblend_islands(*args(**bad)) == -1, bad                    # CY_ERR_ARG
    off2 = off.copy(); off2[3:] += 1                                              # offsets that disagree with the window areas
    assert lib.cy_deblend_islands(*args(f=off2.ctypes.data_as(lp))) == -1
    off3 = off + 1
    assert lib.cy_deblend_islands(*args(f=off3.ctypes.data_as(lp))) == -1
    thr2 = thr.copy(); thr2[5, 0], thr2[5, 1] = 1.0, 2.0                          # seed_thr < merge_thr
    assert lib.cy_deblend_islands(*args(t=thr2.ctypes.data_as(dp))) == -1
    with pytest.raises(L.CyError):
        det.deblend_islands(dev, boxes, thr, conn=5)
    with pytest.raises(L.CyError):
        det.deblend_islands(dev, boxes, thr, radius=9)
    with pytest.raises(L.CyError):
        det.deblend_islands(dev, boxes, thr[:-1])
    a, ac, am = det.deblend_islands(dev, boxes, thr, return_masks=True)
    b, bc, bm = det.deblend_islands(dev, boxes, thr, return_masks=True)
    assert a.tobytes() == b.tobytes() and ac.tobytes() == bc.tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(am, bm))
    assert a.tobytes() == out.tobytes() and ac.tobytes() == comp.tobytes()        # run-to-run: the same bytes
    assert det.deblend_kernel_ms() > 0


def test_window_above_the_supported_maximum():
    """The supported maximum is 2^24 pixels per window: a 4096 x 4096 window is measured (workspace path, 2 x 64 MiB of words), a
    4096 x 4097 one gets status 1, zeros and an all-zero mask, and the call with both succeeds.  Needs an image of its own: the
    2048 x 2048 scene is below the maximum."""
    H, W = 4097, 4096
    assert (H - 1) * W == island_ref.MAX_AREA
    host = np.zeros((H, W), np.float32)                              # blank but for two blobs and a lone candidate
    host[10:14, 10:14] = np.float32(0.3); host[11, 12] = np.float32(0.9)
    host[4090:4094, 4085:4095] = np.float32(0.3); host[4092, 4090] = np.float32(1.5); host[4092, 4087] = np.float32(0.75)
    host[2000, 2000] = np.float32(0.3)
    det = detector("fp32", max_batch=1, max_imgsz=160)
    dev = torch.from_numpy(host).cuda()
    boxes = np.array([[0.0, 0.0, W - 1.0, H - 1.0], [0.0, 0.0, W - 1.0, H - 2.0], [-np.inf, 5.0, 20.0, np.inf]], np.float64)
    thr = np.array([DRAWN_THR] * 3, np.float64)
    ref = deblend_ref.deblend(host, boxes, thr, 8, 2)
    rows, comps, masks, _ = ref
    assert rows[0, 0] == 1 and not rows[0, 1:].any() and not comps[0].any() and masks[0].shape == (H, W) and not masks[0].any()
    # five summits: the three drawn peaks and the first pixel of either 0.3 plateau, which the radius test demotes
    assert tuple(rows[1, :6]) == (0, 5, 3, 3, 16 + 40, 0) and comps[1, 0, 1] == 1.5 and comps[1, 2, 1] == 0.75 and comps[1, 1, 10] == 0
    assert tuple(rows[2, :6]) == (0, 2, 1, 1, 16, 0) and masks[2].shape == (H - 5, 21)
    run_and_compare(det, dev, host, boxes, thr, 8, 2, "supported maximum", ref=ref)
    print("a 2^24-pixel window measured, one row more gets status 1; kernel %.3f ms" % det.deblend_kernel_ms())
