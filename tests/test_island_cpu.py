"""Host side of --measure_islands: the numpy reference of the GPU tests (tests/island_ref.py) on hand-drawn 8 x 8 windows and, where
scipy is installed, against scipy.ndimage.label on the 2000 random boxes of the GPU test; measure.annotate_islands on constructed
rows; the exports and the CLI flags."""
import json
import os
import sys

import numpy as np
import pytest

import island_ref
import measure_ref
from caesar_yolo_amd import measure
from caesar_yolo_amd.wcs import WCS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX8 = [0.0, 0.0, 7.0, 7.0]
THR = [5.0, 2.0, 1.0]                      # seed, merge, bkg


def _img(rows):
    """8 x 8 float32 image from strings: '.' 1.0 (below merge), 'o' 3.0 (candidate), 'X' 9.0 (seed), '_' 0.0 (blank)."""
    v = {".": 1.0, "o": 3.0, "X": 9.0, "_": 0.0}
    return np.array([[v[c] for c in r] for r in rows], np.float32)


def _one(img, box=BOX8, thr=THR, conn=8):
    rows, masks, mags = island_ref.islands(img, [box], [thr], conn)
    return dict(zip(island_ref.FIELDS, rows[0])), masks[0], mags[0]


def test_diagonal_touch_is_one_component_at_8_and_two_at_4():
    img = _img(["........",
                ".Xo.....",
                ".oo.....",
                "...oo...",
                "...oX...",
                "........",
                "........",
                "........"])
    r, m, _ = _one(img, conn=8)
    assert r["nislands"] == 1 and r["npix"] == 8 and r["npix_main"] == 8 and r["nseed"] == 2 and (m == 2).sum() == 8
    r, m, _ = _one(img, conn=4)
    assert r["nislands"] == 2 and r["npix"] == 8 and r["npix_main"] == 4
    assert (m[1:3, 1:3] == 2).all() and (m[3:5, 3:5] == 1).all()            # the first of the two equal peaks is the main island's
    assert (r["xmin"], r["xmax"], r["ymin"], r["ymax"]) == (1, 4, 1, 4) and r["nborder"] == 0


def test_unseeded_blob_is_left_out():
    img = _img(["Xo......",
                "oo......",
                "........",
                "...ooo..",
                "...ooo..",
                "........",
                "......oX",
                "......oo"])
    img[7, 7] = 10.0                                                       # the peak: the main island is the bottom right one
    r, m, mags = _one(img)
    assert r["nislands"] == 2 and r["nseed"] == 3 and r["npix"] == 8 and r["npix_main"] == 4
    assert (m[3:5, 3:6] == 0).all() and m.sum() == 4 * 1 + 4 * 2 and (m[6:, 6:] == 2).all() and (m[:2, :2] == 1).all()
    assert r["nborder"] == 6 and (r["xmin"], r["xmax"], r["ymin"], r["ymax"]) == (0, 7, 0, 7)
    # w = v - 1: 8 + 3 * 2 in the first blob, 9 + 8 + 2 * 2 in the second
    assert r["S"] == 14 + 21 and r["S_main"] == 21 and mags[0] == 35
    # Sx = sum w dx: first blob 8*0 + 2*1 + 2*0 + 2*1 = 4; second 2*6 + 8*7 + 2*6 + 9*7 = 143
    assert r["Sx"] == 147 and r["Sy"] == 4 + (2 * 6 + 8 * 6 + 2 * 7 + 9 * 7)
    assert r["Sxx"] == 4 + (2 * 36 + 8 * 49 + 2 * 36 + 9 * 49) and r["Sxy"] == 2 + (2 * 36 + 8 * 42 + 2 * 42 + 9 * 49)


def test_window_cuts_a_blob_and_single_pixel():
    img = _img(["........",
                "........",
                "..oooo..",
                "..oXXo..",
                "..oooo..",
                "........",
                "......X.",
                "........"])
    r, m, _ = _one(img, box=[3.0, 3.0, 7.0, 7.0])                          # window columns 3..7, rows 3..7: the blob is cut
    assert m.shape == (5, 5) and r["npix"] == 6 + 1 and r["npix_main"] == 6 and r["nislands"] == 2
    assert r["nborder"] == 4 and (r["xmin"], r["xmax"], r["ymin"], r["ymax"]) == (3, 6, 3, 6)
    assert r["Sx"] == 8 * 0 + 8 * 1 + 2 * 2 + 2 * (0 + 1 + 2) + 8 * 3      # window-relative dx
    r, m, _ = _one(img, box=[6.0, 6.0, 6.0, 6.0])
    assert m.shape == (1, 1) and m[0, 0] == 2 and r["npix"] == 1 and r["nborder"] == 1 and r["S"] == 8 and r["Sxx"] == 0


def test_thresholds_blanks_and_empty_windows():
    img = _img(["........",
                ".oo.....",
                ".o_X....",
                "........",
                "........",
                "........",
                "........",
                "........"])
    r, m, _ = _one(img, conn=4)                                            # the blank pixel separates the seed from the blob at conn 4
    assert r["nislands"] == 1 and r["npix"] == 1
    r, m, _ = _one(img, conn=8)
    assert r["nislands"] == 1 and r["npix"] == 4
    r, m, _ = _one(img, thr=[3.0, 3.0, 1.0])                               # >= : a pixel exactly at the threshold is in
    assert r["nseed"] == 4 and r["npix"] == 4
    for thr in ([np.inf, 2.0, 1.0], [np.nan, 2.0, 1.0], [5.0, np.nan, 1.0]):
        r, m, mags = _one(img, thr=thr)
        assert r["nseed"] == 0 and r["npix"] == 0 and r["xmin"] == -1 and r["status"] == 0 and not m.any() and not mags.any()
    r, m, _ = _one(img, box=[-9.0, -9.0, -2.0, 3.0])
    assert m.shape == (0, 0) and r["npix"] == 0 and r["ymax"] == -1 and r["status"] == 0


def _random_boxes(N=2048):
    rng = np.random.default_rng(20261016)                                   # tests/test_gpu_measure.py::test_random_boxes
    n = 2000
    w, h = rng.integers(3, 201, n), rng.integers(3, 201, n)
    x1, y1 = rng.uniform(-40, N + 20, n), rng.uniform(-40, N + 20, n)
    frac = rng.random(n) < 0.5
    x1, y1 = np.where(frac, x1, np.floor(x1)), np.where(frac, y1, np.floor(y1))
    return np.stack([x1, y1, x1 + w, y1 + h], 1)


def test_reference_equals_scipy_label_on_the_random_boxes():
    ndi = pytest.importorskip("scipy.ndimage")
    from caesar_yolo_amd import synth
    img = synth.make_mosaic(n=2048, seed=7)
    host = np.where(np.isfinite(img), img, np.float32(0)).astype(np.float32)
    boxes = _random_boxes()
    meas, _ = measure_ref.measure(host, boxes, 8)
    thr = island_ref.thresholds(meas)
    seeded = 0
    for conn, st in ((8, np.ones((3, 3), int)), (4, None)):
        rows, masks, _ = island_ref.islands(host, boxes, thr, conn)
        for b, t, r, m in zip(boxes, thr, rows, masks):
            if m.size == 0:
                continue
            bx0, bx1 = measure_ref.window(b[0], b[2], 2048)
            by0, by1 = measure_ref.window(b[1], b[3], 2048)
            win = host[by0:by1 + 1, bx0:bx1 + 1].astype(np.float64)
            cand = (win != 0) & (win >= t[1])
            lab, _ = ndi.label(cand, structure=st)
            ids = np.unique(lab[cand & (win >= t[0])])
            assert np.array_equal(m > 0, np.isin(lab, ids) & cand) and r[2] == ids.size
            seeded += ids.size > 0
    assert seeded > 1600


def _row(w, status=0.0, nseed=1.0):
    """Raw row of an island set given as a 2-D array of weights (0 = not in the set), as island_ref computes it."""
    iy, ix = np.nonzero(w)
    wt, dx, dy = w[iy, ix].astype(np.float64), ix.astype(np.float64), iy.astype(np.float64)
    r = np.zeros(20)
    r[0], r[1], r[2], r[3], r[4], r[5] = status, nseed, 1, iy.size, iy.size, 0
    r[6:10] = ix.min() + 100, ix.max() + 100, iy.min() + 200, iy.max() + 200
    r[10:17] = wt.sum(), (wt * dx).sum(), (wt * dy).sum(), (wt * dx * dx).sum(), (wt * dy * dy).sum(), (wt * dx * dy).sum(), wt.sum()
    return r


def _src():
    return {"name": "S1", "x1": 100.0, "x2": 110.0, "y1": 200.0, "y2": 210.0, "class_id": 0, "class_name": "c", "score": 0.9, "edge": 0}


def _ann(row, beam=4.0, wcs=None, origin=(0, 0)):
    return measure.annotate_islands([_src()], np.array([row]), [[100.0, 200.0]], beam, wcs, origin)[0]


def test_annotate_islands_shapes():
    yy, xx = np.mgrid[0:11, 0:11]
    blob = np.where((xx - 5) ** 2 + (yy - 5) ** 2 <= 16, 1.0 + 20 - (xx - 5) ** 2 - (yy - 5) ** 2, 0.0)
    s = _ann(_row(blob))
    assert set(measure.ISLAND_KEYS) <= set(s) and len(measure.ISLAND_KEYS) == 18
    assert s["major"] == s["minor"] > 0 and s["pa"] == 0.0
    assert s["x_isl"] == 105.0 and s["y_isl"] == 205.0
    assert s["island_count"] == 1 and s["island_npix"] == int((blob > 0).sum()) and s["island_border"] is False
    assert (s["island_x1"], s["island_x2"], s["island_y1"], s["island_y2"]) == (101, 109, 201, 209)
    assert s["island_flux_sum"] == blob.sum() and s["island_flux"] == blob.sum() / 4.0 and s["island_flux_main"] == blob.sum() / 4.0
    assert s["ra_isl"] is None and s["dec_isl"] is None
    k = 7
    line = np.zeros((9, 9)); line[3, 1:1 + k] = 2.0                        # along x
    s = _ann(_row(line))
    var = (k * k - 1) / 12.0                                               # variance of k equal weights one pixel apart
    assert s["pa"] == 0.0 and s["minor"] == 0.0 and s["major"] == measure.FWHM * np.sqrt(var)
    s = _ann(_row(line.T))                                                 # along y
    assert s["pa"] == 90.0 and s["minor"] == 0.0 and s["major"] == measure.FWHM * np.sqrt(var)
    s = _ann(_row(np.diag(np.full(k, 2.0))))                               # along the diagonal, +x towards +y
    assert s["pa"] == 45.0 and s["minor"] == 0.0 and s["major"] == measure.FWHM * np.sqrt(2 * var)
    s = _ann(_row(np.diag(np.full(k, 2.0))[::-1]))                         # the other diagonal
    assert s["pa"] == -45.0 and s["minor"] == 0.0
    # the keys the catalog had before are untouched
    assert (s["x1"], s["y1"], s["x2"], s["y2"], s["score"], s["edge"]) == (100.0, 200.0, 110.0, 210.0, 0.9, 0)


def test_annotate_islands_degenerate_rows_and_sky():
    yy, xx = np.mgrid[0:5, 0:5]
    r = _row(np.ones((5, 5)))
    r[5] = 16
    s = _ann(r, beam=0)
    assert s["island_border"] is True and s["island_flux"] is None and s["island_flux_main"] is None and s["island_flux_sum"] == 25.0
    assert json.loads(json.dumps(s))["island_flux"] is None
    r0 = r.copy(); r0[10:17] = 0.0                                          # S == 0: no position, no shape
    s = _ann(r0)
    assert s["island_flux_sum"] == 0.0 and s["island_flux"] == 0.0 and s["island_npix"] == 25
    assert all(s[k] is None for k in ("x_isl", "y_isl", "ra_isl", "dec_isl", "major", "minor", "pa"))
    none = np.zeros(20); none[6:10] = -1                                    # no seed
    s = _ann(none)
    assert (s["island_count"], s["island_npix"], s["island_npix_main"], s["island_border"]) == (0, 0, 0, False)
    assert all(s[k] is None for k in measure.ISLAND_KEYS[4:])
    big = none.copy(); big[0] = 1.0                                         # window above the supported maximum
    s = _ann(big)
    assert all(s[k] is None for k in measure.ISLAND_KEYS)
    assert measure.annotate_islands([], np.zeros((0, 20)), np.zeros((0, 2)), 1.0, None) == []
    with open(os.path.join(ROOT, "tests", "golden", "wcs.json")) as fp:
        w = WCS(json.load(fp)["tan"]["header"])
    s = _ann(r, wcs=w, origin=(10, 20))
    a, d = w.wcs_pix2world(102.0 + 10.0, 202.0 + 20.0, 0)
    assert s["x_isl"] == 102.0 and s["y_isl"] == 202.0 and s["ra_isl"] == float(a) and s["dec_isl"] == float(d)


def test_box_window_is_the_reference_window():
    for box in ([0.5, 0.5, 2.2, 2.9], [-15.5, -7.25, 9.5, 11.0], [100.2, 200.0, 100.8, 210.0], [-50.0, 100.0, -20.0, 130.0],
                [2000.0, 2040.0, 2100.0, 2100.0], [-1e12, -1e12, -1e11, -1e11], [2047.0, 2047.0, 2047.5, 2050.0], [2047.2, 0.0, 2050.0, 5.0]):
        x0, x1 = measure_ref.window(box[0], box[2], 2048)
        y0, y1 = measure_ref.window(box[1], box[3], 2048)
        want = (x0, y0, y1 - y0 + 1, x1 - x0 + 1) if x1 >= x0 and y1 >= y0 else (0, 0, 0, 0)
        assert measure.box_window(box, 2048, 2048) == want
    # a NaN edge makes the window empty; an infinite edge is an ordinary edge beyond the image (window_1d of the library)
    inf = np.inf
    assert measure.box_window([np.nan, 0.0, 5.0, 5.0], 2048, 2048) == (0, 0, 0, 0)
    assert measure.box_window([0.0, 0.0, 5.0, np.nan], 2048, 2048) == (0, 0, 0, 0)
    assert measure.box_window([-inf, 10.5, 5.0, inf], 1024, 2048) == (0, 11, 1024 - 11, 6)      # (box, MH, MW) -> (wx0, wy0, h, w)
    assert measure.box_window([-inf, -inf, inf, inf], 100, 200) == (0, 0, 100, 200)
    assert measure.box_window([inf, 0.0, inf, 5.0], 2048, 2048) == (0, 0, 0, 0)
    assert measure.box_window([0.0, -inf, 5.0, -inf], 2048, 2048) == (0, 0, 0, 0)
    assert measure.box_window([3.0, 3.0, -inf, 9.0], 2048, 2048) == (0, 0, 0, 0)
    assert all(type(v) is int for v in measure.box_window([-inf, 10.5, 5.0, inf], 2048, 1024))


def test_island_thresholds_are_bkg_plus_k_rms():
    src = [{"bkg": 0.5, "rms": 0.25}, {"bkg": -1e-3, "rms": 3e-4}, {"bkg": 2.0, "rms": 0.0}]
    t = measure.island_thresholds(src, 5.0, 2.5)
    assert t.dtype == np.float64 and t.shape == (3, 3)
    for s, row in zip(src, t):
        assert tuple(row) == (s["bkg"] + 5.0 * s["rms"], s["bkg"] + 2.5 * s["rms"], s["bkg"])
    t = measure.island_thresholds(src, 4.0, 2.0)
    assert tuple(t[0]) == (1.5, 1.0, 0.5) and tuple(t[2]) == (2.0, 2.0, 2.0)
    rows = np.array([[0, 0, s["bkg"], s["rms"]] for s in src])
    assert np.array_equal(t, island_ref.thresholds(rows, 4.0, 2.0))          # the reference's own, from measurement rows


def test_exports_and_fields():
    from caesar_yolo_amd import lib as L
    from caesar_yolo_amd.model import HipDetector
    assert "cy_measure_islands" in L.EXPORTS and "cy_islands_kernel_ms" in L.EXPORTS
    assert L.CY_ISL_FIELDS == len(L.ISL_NAMES) == len(island_ref.FIELDS) == 20
    assert tuple(L.ISL_NAMES) == tuple(island_ref.FIELDS)
    assert callable(HipDetector.measure_islands) and callable(HipDetector.islands_kernel_ms)
    hdr = open(os.path.join(ROOT, "include", "caesar_yolo_hip.h")).read()
    assert "#define CY_ISL_FIELDS 20" in hdr


def test_cli_flags():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import run
    a = run.parse_args(["--weights=seeded:l:5"])
    assert a.measure_islands is False and a.island_seed_sigma == 5.0 and a.island_merge_sigma == 2.5 and a.island_conn == 8
    a = run.parse_args(["--weights=seeded:l:5", "--measure_islands", "--island_seed_sigma", "4", "--island_merge_sigma=3", "--island_conn", "4"])
    assert a.measure_islands is True and a.island_seed_sigma == 4.0 and a.island_merge_sigma == 3.0 and a.island_conn == 4
    with pytest.raises(SystemExit):
        run.parse_args(["--weights=seeded:l:5", "--island_conn", "6"])
    fits = os.path.join(ROOT, "tests", "golden", "galaxy0001.fits")
    ok = run.parse_args(["--weights=seeded:l:5", "--image=" + fits, "--measure_islands", "--island_seed_sigma=3", "--island_merge_sigma=3"])
    assert run.validate_args(ok) == 0
    bad = run.parse_args(["--weights=seeded:l:5", "--image=" + fits, "--measure_islands", "--island_seed_sigma=2", "--island_merge_sigma=3"])
    assert run.validate_args(bad) == -1
    idle = run.parse_args(["--weights=seeded:l:5", "--image=" + fits, "--island_seed_sigma=2", "--island_merge_sigma=3"])
    assert run.validate_args(idle) == 0                                     # without --measure_islands the two options are not read
    from caesar_yolo_amd.config import CONFIG
    assert CONFIG["measure_islands"] is False and CONFIG["island_seed_sigma"] == 5.0 and CONFIG["island_merge_sigma"] == 2.5
    assert CONFIG["island_conn"] == 8
