"""cy_measure_islands on the GPU against the numpy / flood-fill reference (tests/island_ref.py) on the 2048 x 2048 synthetic mosaic
of tests/test_gpu_measure.py (same recipe: NaN strip on the right, all-zero block in the middle) with a few windows drawn in.

Thresholds: bkg + 5 rms / bkg + 2.5 rms from the REFERENCE's measurement rows (tests/measure_ref.py, ring 8) unless a constructed
case says otherwise.  Comparison, for EVERY source (none skipped):
  mask bytes equal; status, counts and bounding box (fields 0-9) and the reserved fields equal: they are sets and counts;
  S Sx Sy Sxx Syy Sxy S_main   both sides add the same float64 terms in some order, so |gpu - ref| <= 2 m 2^-53 sum|t_i| with
                               m = npix of the island set and sum|t_i| from the reference.  Derived, not tuned.
Labelling sweeps: the kernel makes five sweeps over a window whatever its components look like (cy_islands.hip); the two
serpentines (a component whose longest path is half the window's area) are here to show that."""
import ctypes as C

import numpy as np
import pytest
import torch

import island_ref
import measure_ref
from gpu_common import detector

pytestmark = pytest.mark.gpu

N = 2048
LDS_MAX = 4096                               # windows of up to this many pixels are labelled in LDS (cy_kernels.h: ISL_LDS_MAX)
LO, MID, HI = np.float32(0.01), np.float32(0.3), np.float32(0.9)
DRAWN_THR = [0.5, 0.2, 0.0]                  # seed, merge, bkg of the drawn windows: LO is nothing, MID a candidate, HI a seed


def serpentine(n):
    """n x n (n odd) boolean array: every second row full, joined at alternating ends: ONE component, one pixel wide."""
    p = np.zeros((n, n), bool)
    p[0::2, :] = True
    p[1::4, n - 1] = True
    p[3::4, 0] = True
    return p


def draw(rows):
    v = {".": LO, "o": MID, "X": HI}
    return np.array([[v[c] for c in r] for r in rows], np.float32)


DIAGONAL = ["........",
            ".Xo.....",
            ".oo.....",
            "...oo...",
            "...oX...",
            "........",
            "........",
            "........"]
BLOBS = ["Xo......",
         "oo......",
         "........",
         "...ooo..",
         "...ooo..",
         "........",
         "..ooXo..",
         "..oooo.."]


def make_image():
    from caesar_yolo_amd import synth
    img = synth.make_mosaic(n=N, seed=7)                  # NaN strip: columns 1984..2047; zero block: [1024, 1536) x [1024, 1536)
    img[300:303, 400:405] = np.float32(0.25)              # the stamps of tests/test_gpu_measure.py::scene
    img[310, 420] = img[312, 418] = np.float32(0.5)
    img[600:640, 700:740] = np.float32(0.125)
    img[1200:1203, 1100:1103] = np.float32(0.75)
    img[800, 800] = np.float32(-1.0)
    holes = np.random.default_rng(3).integers(0, N, (40000, 2))
    holes = holes[holes[:, 0] >= 1040]
    img[holes[:, 0], holes[:, 1]] = 0.0
    img[1005, 30] = 0.0
    # the drawn windows of this test (rows 1600.., left of the NaN strip, below the zero block, above no stamp of the list above)
    img[1600:1608, 100:108] = draw(DIAGONAL)
    img[1600:1608, 120:128] = draw(BLOBS)
    s63, s301 = serpentine(63), serpentine(301)
    img[1620:1683, 100:163] = np.where(s63, MID, LO)
    img[1682, 162] = HI                                   # the seed at the far end of the path
    img[1700:2001, 100:401] = np.where(s301, MID, LO)
    img[2000, 400] = HI
    img[1620:1630, 200:210] = np.float32(0.25)            # plateau
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


def compare(got, gmasks, ref, rmasks, mags, what):
    """-> the largest |diff| / bound over the sums."""
    assert got.shape == ref.shape and len(gmasks) == len(rmasks) == ref.shape[0]
    worst = 0.0
    for i in range(ref.shape[0]):
        assert gmasks[i].shape == rmasks[i].shape and gmasks[i].dtype == np.uint8, "%s, source %d: mask shape %s, reference %s" % (
            what, i, gmasks[i].shape, rmasks[i].shape)
        assert gmasks[i].tobytes() == rmasks[i].tobytes(), "%s, source %d: %d mask bytes differ" % (what, i, (gmasks[i] != rmasks[i]).sum())
        for f in tuple(range(10)) + (17, 18, 19):
            assert got[i, f] == ref[i, f], "%s, source %d: %s = %r on the GPU, %r in the reference" % (
                what, i, island_ref.FIELDS[f], got[i, f], ref[i, f])
        m = ref[i, 3]
        for f, mag in zip(island_ref.SUMS, mags[i]):
            bound = 2.0 * m * 2.0 ** -53 * mag
            diff = abs(got[i, f] - ref[i, f])
            assert diff <= bound, "%s, source %d: %s = %r on the GPU, %r in the reference, |diff| %g > bound %g (m = %d)" % (
                what, i, island_ref.FIELDS[f], got[i, f], ref[i, f], diff, bound, m)
            if bound > 0:
                worst = max(worst, diff / bound)
    return worst


def sigma_thresholds(host, boxes):
    meas, _ = measure_ref.measure(host, boxes, 8)
    return island_ref.thresholds(meas, 5.0, 2.5)


def drawn_cases():
    """name -> (box, thresholds)"""
    up = float(np.nextafter(np.float32(0.25), np.float32(1)))
    return {
        "diagonal touch": ([100.0, 1600.0, 107.0, 1607.0], DRAWN_THR),
        "seeded and unseeded blobs": ([120.0, 1600.0, 127.0, 1607.0], DRAWN_THR),
        "blob cut by the window": ([123.0, 1603.0, 127.0, 1607.0], DRAWN_THR),
        "serpentine 63": ([100.0, 1620.0, 162.0, 1682.0], DRAWN_THR),
        "serpentine 301": ([100.0, 1700.0, 400.0, 2000.0], DRAWN_THR),
        "plateau at merge_thr": ([198.0, 1618.0, 211.0, 1631.0], [0.25, 0.25, 0.0]),
        "plateau just below merge_thr": ([198.0, 1618.0, 211.0, 1631.0], [up, up, 0.0]),
        "plateau, seed_thr = +inf": ([198.0, 1618.0, 211.0, 1631.0], [np.inf, 0.25, 0.0]),
        "plateau, NaN merge_thr": ([198.0, 1618.0, 211.0, 1631.0], [0.25, np.nan, 0.0]),
        "plateau, NaN seed_thr": ([198.0, 1618.0, 211.0, 1631.0], [np.nan, 0.25, 0.0]),
    }


def scene_boxes():
    """Boxes measured with the 5 / 2.5 sigma thresholds of the reference's own bkg and rms (names as in tests/test_gpu_measure.py)."""
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


def constructed_reference(host, conn):
    """Boxes, thresholds and the reference's results of the constructed cases, each checked to be what its name says."""
    drawn, named = drawn_cases(), scene_boxes()
    names = list(drawn) + list(named)
    boxes = np.array([v[0] for v in drawn.values()] + list(named.values()), np.float64)
    thr = np.concatenate([np.array([v[1] for v in drawn.values()], np.float64), sigma_thresholds(host, np.array(list(named.values())))])
    ref, rmasks, mags = island_ref.islands(host, boxes, thr, conn)
    r = {k: dict(zip(island_ref.FIELDS, ref[i])) for i, k in enumerate(names)}
    rm = dict(zip(names, rmasks))
    # the cases are what their names say (on the reference side, so that a wrong construction fails here and not silently)
    d = r["diagonal touch"]
    assert (d["nislands"], d["npix"], d["npix_main"]) == ((1, 8, 8) if conn == 8 else (2, 8, 4))
    d = r["seeded and unseeded blobs"]
    assert d["nislands"] == 2 and d["npix"] == 4 + 8 and d["npix_main"] == 4 and not rm["seeded and unseeded blobs"][3:5, 3:6].any()
    assert d["nborder"] == 3 + 4
    d = r["blob cut by the window"]
    assert d["nislands"] == 1 and d["npix"] == 6 and d["nborder"] == 3 + 1 and rm["blob cut by the window"].shape == (5, 5)
    for k, n in (("serpentine 63", 63), ("serpentine 301", 301)):
        assert np.array_equal(rm[k], 2 * serpentine(n).astype(np.uint8)) and r[k]["nislands"] == 1 and r[k]["nseed"] == 1
        assert r[k]["npix"] == (n + 1) // 2 * n + n // 2
    assert 63 * 63 <= LDS_MAX < 301 * 301
    d = r["plateau at merge_thr"]
    assert d["npix"] == 100 and d["nseed"] == 100 and d["nborder"] == 0 and (d["xmin"], d["xmax"], d["ymin"], d["ymax"]) == (200, 209, 1620, 1629)
    for k in ("plateau just below merge_thr", "plateau, seed_thr = +inf", "plateau, NaN merge_thr", "plateau, NaN seed_thr"):
        assert r[k]["nseed"] == 0 and r[k]["npix"] == 0 and r[k]["xmin"] == -1 and not rm[k].any() and rm[k].shape == (14, 14)
    for k in names:
        if k.startswith("wholly outside") or k.startswith("fractional"):
            assert rm[k].shape == (0, 0) and r[k]["npix"] == 0 and r[k]["xmin"] == -1
    assert rm["across the NaN strip"].shape == (31, 51) and not rm["across the NaN strip"][:, 24:].any()
    assert rm["across the zero block's edge"].shape == (51, 61) and not rm["across the zero block's edge"][24:, 24:].any()
    assert r["inside the zero block"]["nseed"] == 0 and rm["inside the zero block"].size == 31 * 21
    d = r["island in the zero block (blank ring)"]                # blank ring: bkg = rms = 0, every valid pixel is a seed
    assert d["npix"] == 9 and d["nseed"] == 9 and d["nborder"] == 8
    assert rm["partly outside, left top"].shape == (12, 10) and rm["partly outside, right bottom"].shape == (12, 90)
    assert rm["64 x 64: the largest LDS window"].size == LDS_MAX and rm["65 x 64: the smallest workspace window"].size == LDS_MAX + 64
    assert rm["large window"].shape == (1200, 1500) and r["large window"]["nislands"] > 50
    assert rm["whole image"].shape == (N, N) and r["whole image"]["npix"] > 1000000      # no ring: bkg = rms = 0, every pixel >= 0 is a seed
    assert (ref[:, 0] == 0).all()                                  # the supported maximum (2^24 pixels) is above the whole image
    return names, boxes, thr, ref, rmasks, mags


@pytest.mark.parametrize("conn", [8, 4])
def test_constructed_windows(scene, conn):
    det, dev, host = scene
    names, boxes, thr, ref, rmasks, mags = constructed_reference(host, conn)
    got, gmasks = det.measure_islands(dev, boxes, thr, conn=conn, return_masks=True)
    ms = det.islands_kernel_ms()
    worst = compare(got, gmasks, ref, rmasks, mags, "conn %d" % conn)
    rows_only = det.measure_islands(dev, boxes, thr, conn=conn)    # without the mask output: the same rows
    assert rows_only.tobytes() == got.tobytes()
    print("conn %d: %d constructed windows equal, largest |diff| / bound of the sums %.3g; kernel %.3f ms" % (conn, len(names), worst, ms))


def random_boxes():
    rng = np.random.default_rng(20261016)                           # tests/test_gpu_measure.py::test_random_boxes
    n = 2000
    w, h = rng.integers(3, 201, n), rng.integers(3, 201, n)
    x1, y1 = rng.uniform(-40, N + 20, n), rng.uniform(-40, N + 20, n)
    frac = rng.random(n) < 0.5
    x1, y1 = np.where(frac, x1, np.floor(x1)), np.where(frac, y1, np.floor(y1))
    return np.stack([x1, y1, x1 + w, y1 + h], 1)


@pytest.mark.parametrize("conn", [8, 4])
def test_random_boxes(scene, conn):
    det, dev, host = scene
    boxes = random_boxes()
    thr = sigma_thresholds(host, boxes)
    ref, rmasks, mags = island_ref.islands(host, boxes, thr, conn)
    if conn == 8:
        assert (ref[:, 1] > 0).sum() >= 800 and (ref[:, 2] >= 2).sum() >= 300 and (ref[:, 5] > 0).sum() >= 400
    assert (ref[:, 0] == 0).all()
    got, gmasks = det.measure_islands(dev, boxes, thr, conn=conn, return_masks=True)
    ms = det.islands_kernel_ms()
    worst = compare(got, gmasks, ref, rmasks, mags, "random, conn %d" % conn)
    lds = sum(m.size <= LDS_MAX for m in rmasks)
    print("conn %d: 2000 random boxes (%d labelled in LDS, %d with a seed, %d with two or more islands, %d touching the border): masks and "
          "counts equal, largest |diff| / bound of the sums %.3g; kernel %.3f ms" % (
              conn, lds, (ref[:, 1] > 0).sum(), (ref[:, 2] >= 2).sum(), (ref[:, 5] > 0).sum(), worst, ms))


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
    out = np.zeros((n, L.CY_ISL_FIELDS), np.float64)
    off = np.zeros(n + 1, np.int64)
    np.cumsum([np.prod(measure.box_window(b, N, N)[2:]) for b in boxes], out=off[1:])
    mask = np.zeros(int(off[-1]), np.uint8)
    args = lambda n=n, conn=8, img=dev.data_ptr(), mh=N, mw=N, b=boxes.ctypes.data_as(dp), t=thr.ctypes.data_as(dp), o=out.ctypes.data_as(dp), \
        m=C.c_void_p(mask.ctypes.data), f=off.ctypes.data_as(lp), ctx=det.ctx: (ctx, C.c_void_p(img), mh, mw, b, t, n, conn, o, m, f, det._stream())
    assert lib.cy_measure_islands(*args()) == 0
    assert lib.cy_measure_islands(*args(m=None, f=None)) == 0                     # no mask wanted
    rows, masks = det.measure_islands(dev, np.zeros((0, 4)), np.zeros((0, 3)), return_masks=True)
    assert rows.shape == (0, L.CY_ISL_FIELDS) and masks == []
    assert lib.cy_measure_islands(*args(n=0)) == 0                                # CY_OK, nothing launched
    bad_row0 = thr.copy(); bad_row0[0, 0], bad_row0[0, 1] = 1.0, 2.0
    assert lib.cy_measure_islands(*args(n=0, t=bad_row0.ctypes.data_as(dp))) == 0 # n == 0 is answered before the rows are read
    assert lib.cy_measure_islands(*args(t=bad_row0.ctypes.data_as(dp))) == -1
    assert lib.cy_measure_islands(*args(mh=65536, mw=32768)) == -1                # an image of 2^31 pixels: refused before anything is read
    assert lib.cy_measure_islands(*args(mh=32768, mw=65536, m=None, f=None)) == -1
    for bad in (dict(conn=6), dict(conn=0), dict(mh=0), dict(mw=-5), dict(img=None), dict(b=None), dict(t=None), dict(o=None), dict(ctx=None),
                dict(n=-3), dict(f=None)):
        assert lib.cy_measure_islands(*args(**bad)) == -1, bad                    # CY_ERR_ARG
    off2 = off.copy(); off2[3:] += 1                                              # offsets that disagree with the window areas
    assert lib.cy_measure_islands(*args(f=off2.ctypes.data_as(lp))) == -1
    off3 = off + 1
    assert lib.cy_measure_islands(*args(f=off3.ctypes.data_as(lp))) == -1
    thr2 = thr.copy(); thr2[5, 0], thr2[5, 1] = 1.0, 2.0                          # seed_thr < merge_thr
    assert lib.cy_measure_islands(*args(t=thr2.ctypes.data_as(dp))) == -1
    with pytest.raises(L.CyError):
        det.measure_islands(dev, boxes, thr, conn=5)
    with pytest.raises(L.CyError):
        det.measure_islands(dev, boxes, thr[:-1])
    a, am = det.measure_islands(dev, boxes, thr, return_masks=True)
    b, bm = det.measure_islands(dev, boxes, thr, return_masks=True)
    assert a.tobytes() == b.tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(am, bm))      # run-to-run: the same bytes
    assert a.tobytes() == out.tobytes()
    assert det.islands_kernel_ms() > 0


def test_window_above_the_supported_maximum():
    """The supported maximum is 2^24 pixels per window: a 4096 x 4096 window is measured (workspace path, 64 MiB of labels), a
    4096 x 4097 one gets status 1, zeros and an all-zero mask, and the call with both succeeds.  Needs an image of its own: the
    2048 x 2048 scene is below the maximum.  The third box has infinite edges (an ordinary edge beyond the image)."""
    H, W = 4097, 4096
    assert (H - 1) * W == island_ref.MAX_AREA
    host = np.zeros((H, W), np.float32)                              # blank but for two blobs and a lone candidate
    host[10:14, 10:14] = MID; host[11, 12] = HI
    host[4090:4094, 4085:4095] = MID; host[4092, 4090] = np.float32(1.5)
    host[2000, 2000] = MID
    det = detector("fp32", max_batch=1, max_imgsz=160)
    dev = torch.from_numpy(host).cuda()
    boxes = np.array([[0.0, 0.0, W - 1.0, H - 1.0], [0.0, 0.0, W - 1.0, H - 2.0], [-np.inf, 5.0, 20.0, np.inf]], np.float64)
    thr = np.array([DRAWN_THR] * 3, np.float64)
    ref, rmasks, mags = island_ref.islands(host, boxes, thr, 8)
    assert ref[0, 0] == 1 and not ref[0, 1:6].any() and (ref[0, 6:10] == -1).all() and not ref[0, 10:].any()
    assert rmasks[0].shape == (H, W) and not rmasks[0].any()
    assert ref[1, 0] == 0 and ref[1, 2] == 2 and ref[1, 3] == 16 + 40 and ref[1, 4] == 40 and rmasks[1].shape == (H - 1, W)
    assert ref[2, 0] == 0 and rmasks[2].shape == (H - 5, 21) and ref[2, 2] == 1 and ref[2, 3] == 16
    got, gmasks = det.measure_islands(dev, boxes, thr, conn=8, return_masks=True)
    compare(got, gmasks, ref, rmasks, mags, "supported maximum")
    assert det.measure_islands(dev, boxes, thr, conn=8).tobytes() == got.tobytes()
    print("a 2^24-pixel window measured, one row more gets status 1; kernel %.3f ms" % det.islands_kernel_ms())
