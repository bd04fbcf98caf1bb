"""Host side of --measure_sources: measure.annotate on hand-written raw rows, the CLI flags, and the numpy reference of the
GPU tests (tests/measure_ref.py) on a 5x5 array worked out by hand."""
import json
import os
import sys

import numpy as np

import measure_ref
from caesar_yolo_amd import measure
from caesar_yolo_amd.wcs import WCS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "wcs.json")) as fp:
    WCS_CASES = json.load(fp)


def _src(x1, y1, x2, y2):
    return {"name": "S1", "x1": float(x1), "x2": float(x2), "y1": float(y1), "y2": float(y2), "class_id": 0, "class_name": "c",
            "score": 0.9, "edge": 0}


#            npix nring bkg  rms  peak xp  yp  sum   sw   swx    swy   reserved
ROW = [12.0, 40.0, 0.5, 0.25, 4.5, 11.0, 21.0, 30.0, 8.0, 84.0, 172.0, 0.0]


def test_annotate_derives_every_key():
    s = measure.annotate([_src(10, 20, 13, 23)], np.array([ROW]), beam_area=4.0, wcs=None)[0]
    assert set(measure.KEYS) <= set(s)
    assert s["npix"] == 12 and isinstance(s["npix"], int) and s["bkg"] == 0.5 and s["rms"] == 0.25 and s["peak"] == 4.5
    assert s["x_peak"] == 11 and s["y_peak"] == 21
    assert s["x0"] == 84.0 / 8.0 and s["y0"] == 172.0 / 8.0
    assert s["snr"] == (4.5 - 0.5) / 0.25
    assert s["flux_sum"] == 30.0 and s["flux"] == 30.0 / 4.0
    assert s["ra"] is None and s["dec"] is None
    # the keys the catalog had before are untouched
    assert (s["x1"], s["y1"], s["x2"], s["y2"], s["score"], s["edge"]) == (10.0, 20.0, 13.0, 23.0, 0.9, 0)


def test_annotate_degenerate_rows():
    row = list(ROW)
    row[8] = row[9] = row[10] = 0.0                     # sw == 0: no pixel above the background -> the centre of the box
    row[3] = 0.0                                        # rms == 0 -> snr 0
    s = measure.annotate([_src(10, 20, 13, 24)], np.array([row]), beam_area=0, wcs=None)[0]
    assert s["x0"] == 11.5 and s["y0"] == 22.0
    assert s["snr"] == 0.0
    assert s["flux"] is None and s["flux_sum"] == 30.0   # beam_area == 0: no flux in beam units
    assert json.loads(json.dumps(s))["flux"] is None     # null in the catalog file
    empty = [0.0, 0.0, 0.0, 0.0, 0.0, -1.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    s = measure.annotate([_src(-30, -30, -20, -20)], np.array([empty]), beam_area=2.0, wcs=None)[0]
    assert s["npix"] == 0 and s["x_peak"] == -1 and s["y_peak"] == -1 and s["flux"] == 0.0 and s["snr"] == 0.0
    assert measure.annotate([], np.zeros((0, 12)), 1.0, None) == []


def test_annotate_sky_position_and_crop_origin():
    w = WCS(WCS_CASES["tan"]["header"])
    s = measure.annotate([_src(10, 20, 13, 23)], np.array([ROW]), beam_area=4.0, wcs=w)[0]
    a, d = w.wcs_pix2world(84.0 / 8.0, 172.0 / 8.0, 0)
    assert s["ra"] == float(a) and s["dec"] == float(d)
    # a crop origin moves the sky position, not the pixel position
    t = measure.annotate([_src(10, 20, 13, 23)], np.array([ROW]), beam_area=4.0, wcs=w, origin=(100, 200))[0]
    a2, d2 = w.wcs_pix2world(84.0 / 8.0 + 100.0, 172.0 / 8.0 + 200.0, 0)
    assert t["ra"] == float(a2) and t["dec"] == float(d2) and (t["ra"], t["dec"]) != (s["ra"], s["dec"])
    assert t["x0"] == s["x0"] and t["y0"] == s["y0"]
    # the golden world coordinates of that header (astropy): the pixel the fixture lists maps where astropy put it
    x, y = WCS_CASES["tan"]["x"][0], WCS_CASES["tan"]["y"][0]
    row = list(ROW)
    row[9], row[10] = x * row[8], y * row[8]
    g = measure.annotate([_src(0, 0, 1, 1)], np.array([row]), 1.0, w)[0]
    assert abs((g["ra"] - WCS_CASES["tan"]["world_0"][0][0] + 180.0) % 360.0 - 180.0) <= 1e-9
    assert abs(g["dec"] - WCS_CASES["tan"]["world_0"][1][0]) <= 1e-9


def test_cli_flags():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import run
    a = run.parse_args(["--weights=seeded:l:5"])
    assert a.measure_sources is False and a.measure_ring == 8
    a = run.parse_args(["--weights=seeded:l:5", "--measure_sources", "--measure_ring", "3"])
    assert a.measure_sources is True and a.measure_ring == 3
    from caesar_yolo_amd.config import CONFIG
    assert CONFIG["measure_sources"] is False and CONFIG["measure_ring"] == 8


# 5x5 image; blank pixels (0, NaN) are invalid.  Worked by hand below.
IMG = np.array([[1.0, 2.0, 3.0, 4.0, 5.0],
                [6.0, 9.0, 9.0, 0.0, 7.0],
                [8.0, 2.0, 9.0, 1.0, 3.0],
                [np.nan, 5.0, 4.0, 2.0, 6.0],
                [1.0, 3.0, 2.0, 8.0, 4.0]], np.float32)


def test_reference_on_a_hand_worked_array():
    # box [0.5, 0.5, 2.2, 2.9]: ix in [1, 2], iy in [1, 2] -> pixels 9 9 / 2 9; ring 1 = the 4x4 frame around them minus the box:
    # row 0: 1 2 3 4 | row 1: 6, 0(blank) | row 2: 8, 1 | row 3: NaN(blank) 5 4 2  -> 10 valid: 1 1 2 2 3 4 4 5 6 8
    rows, mags = measure_ref.measure(IMG, [[0.5, 0.5, 2.2, 2.9]], ring=1)
    r = dict(zip(measure_ref.FIELDS, rows[0]))
    assert r["npix"] == 4 and r["nring"] == 10
    assert r["bkg"] == 3.5                                     # even count: (3 + 4) / 2
    # deviations 2.5 2.5 1.5 1.5 0.5 0.5 0.5 1.5 2.5 4.5 -> sorted .5 .5 .5 1.5 1.5 | 1.5 2.5 2.5 2.5 4.5 -> median 1.5
    assert r["rms"] == 1.4826 * 1.5
    assert r["peak"] == 9.0 and (r["x_peak"], r["y_peak"]) == (1.0, 1.0)      # three 9s: the first in row-major order
    assert r["sum"] == 5.5 + 5.5 - 1.5 + 5.5                   # v - bkg
    assert r["sw"] == 16.5 and r["swx"] == 5.5 * 1 + 5.5 * 2 + 5.5 * 2 and r["swy"] == 5.5 * 1 + 5.5 * 1 + 5.5 * 2
    assert list(mags[0]) == [18.0, 16.5, 27.5, 22.0]
    # ring 1 around the one-pixel box at (4, 4), clipped by the corner: 2 6 8 -> odd count
    rows, _ = measure_ref.measure(IMG, [[4.0, 4.0, 4.0, 4.0]], ring=1)
    r = dict(zip(measure_ref.FIELDS, rows[0]))
    assert r["npix"] == 1 and r["nring"] == 3 and r["bkg"] == 6.0 and r["rms"] == 1.4826 * 2.0
    assert r["peak"] == 4.0 and r["sum"] == -2.0 and r["sw"] == 0.0 and r["swx"] == 0.0
    # a box on the blank pixels only, one without a pixel centre, one outside the image
    rows, _ = measure_ref.measure(IMG, [[3.0, 1.0, 3.0, 1.0], [1.2, 1.2, 1.8, 1.8], [-9.0, -9.0, -2.0, -2.0], [7.0, 0.0, 9.0, 3.0]], ring=0)
    for row in rows:
        r = dict(zip(measure_ref.FIELDS, row))
        assert r["npix"] == 0 and r["nring"] == 0 and r["peak"] == 0.0 and r["x_peak"] == -1.0 and r["y_peak"] == -1.0
        assert r["sum"] == r["sw"] == r["bkg"] == r["rms"] == 0.0
    # ring 0 is no ring; a ring of blank pixels only gives bkg = rms = 0
    rows, _ = measure_ref.measure(IMG, [[0.0, 0.0, 4.0, 4.0]], ring=0)
    assert rows[0][0] == 23 and rows[0][1] == 0 and rows[0][2] == 0.0 and rows[0][4] == 9.0 and (rows[0][5], rows[0][6]) == (1.0, 1.0)


def test_detector_wrapper_and_export_are_declared():
    from caesar_yolo_amd import lib as L
    from caesar_yolo_amd.model import HipDetector
    assert "cy_measure_sources" in L.EXPORTS and L.CY_MEAS_FIELDS == len(L.MEAS_NAMES) == len(measure_ref.FIELDS) == 12
    assert tuple(L.MEAS_NAMES) == tuple(measure_ref.FIELDS)
    assert callable(HipDetector.measure_sources)
