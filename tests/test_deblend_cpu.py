"""The reference of the source components (tests/deblend_ref.py) against a second, independent formulation and its own invariants;
measure.annotate_components on hand-made rows; the command line's handling of --deblend_islands.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest

import deblend_ref
import island_ref
from caesar_yolo_amd import measure
from caesar_yolo_amd.wcs import WCS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def descending_basins(win, cand, inset, conn):
    """The second formulation: the island pixels visited in descending rank; a pixel with no higher-ranked candidate neighbour
    opens a basin, any other inherits the basin of its highest-ranked such neighbour.  Every candidate neighbour of an island
    pixel is an island pixel, so it was visited before when it ranks higher.  -> summit [h * w] (-1 elsewhere)."""
    h, w = win.shape
    nb = island_ref.NB8 if conn == 8 else island_ref.NB4
    pix = [(-float(win[y, x]), y * w + x) for y, x in zip(*np.nonzero(inset))]
    pix.sort()
    top = np.full(h * w, -1, np.int64)
    for key in pix:
        p = key[1]
        y, x = divmod(p, w)
        higher = [(-float(win[y + dy, x + dx]), (y + dy) * w + x + dx) for dy, dx in nb
                  if 0 <= y + dy < h and 0 <= x + dx < w and cand[y + dy, x + dx]]
        higher = [k for k in higher if k < key]
        top[p] = top[min(higher)[1]] if higher else p
        assert top[p] >= 0
    return top


def random_window(rng, h, w, plateaus):
    win = rng.normal(0.0, 1.0, (h, w)).astype(np.float32)
    for _ in range(3):
        cy, cx, a, sg = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(3, 9), rng.uniform(0.8, 2.5)
        yy, xx = np.mgrid[0:h, 0:w]
        win += (a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sg * sg))).astype(np.float32)
    if plateaus:
        win = (np.round(win * 2) / 2).astype(np.float32)                    # many equal values: ties by index
    win[rng.random((h, w)) < 0.03] = 0.0                                    # blanks
    return win


@pytest.mark.parametrize("conn", [8, 4])
def test_walk_equals_the_descending_rank_formulation(conn):
    rng = np.random.default_rng(20261017 + conn)
    nsplit = 0
    for t in range(60):
        h, w = int(rng.integers(1, 24)), int(rng.integers(1, 24))
        win = random_window(rng, h, w, plateaus=t % 2 == 1)
        thr4 = (2.5, 1.0, 0.0, 2.5)
        row, comp, mask, mags, ex = deblend_ref.deblend_one(win, [0, 0, w - 1, h - 1], thr4, conn, radius=1 + t % 3, full=True)
        irow, imask, _ = island_ref.islands_one(win, [0, 0, w - 1, h - 1], thr4[:3], conn)
        assert row[4] == irow[3]
        if irow[1] == 0:
            assert not row.any() and not comp.any() and not mask.any()
            continue
        cand = (win != 0) & (win.astype(np.float64) >= thr4[1])
        top = descending_basins(win, cand, imask > 0, conn)
        assert np.array_equal(top, ex["summit"])                            # basins and summits identical
        summits = np.unique(top[top >= 0])
        assert row[1] == summits.size and set(ex["peaks"]) <= set(summits.tolist())
        nsplit += row[3] >= 2
    assert nsplit >= 5


def invariants(win, thr4, conn, radius):
    h, w = win.shape
    box = [0, 0, w - 1, h - 1]
    row, comp, mask, mags = deblend_ref.deblend_one(win, box, thr4, conn, radius)
    irow, imask, imags = island_ref.islands_one(win, box, thr4[:3], conn)
    nc = int(row[3])
    assert row[4] == irow[3] and comp[:nc, 0].sum() + row[5] == irow[3]     # component npix + unassigned = island npix
    assert not comp[nc:].any() and nc == min(int(row[2]), deblend_ref.MAX_COMP) and (row[0] == 2) == (row[2] > deblend_ref.MAX_COMP)
    assert np.array_equal(mask > 0, imask > 0)
    for k in range(nc):
        assert (mask == k + 1).sum() == comp[k, 0]                          # mask bytes against the rows
        py, px = int(comp[k, 3]), int(comp[k, 2])
        assert mask[py, px] == k + 1 and win[py, px] == comp[k, 1]
        assert (imask[mask == k + 1] == 2).all() == bool(comp[k, 10]) and len(set(imask[mask == k + 1].tolist())) == 1
    assert (mask == deblend_ref.UNASSIGNED).sum() == row[5] and set(np.unique(mask).tolist()) <= set(range(nc + 1)) | {255}
    if nc:
        assert (np.diff(comp[:nc, 1]) <= 0).all()                           # components in descending peak order
        assert comp[:nc, 11].sum() <= row[1] and (comp[:nc, 11] >= 1).all()
    if row[5] == 0:
        assert comp[:nc, 11].sum() == row[1]
        # the components' sums add up to the island's within the rounding bound of adding npix terms in another order
        for j, f in enumerate(island_ref.SUMS[:6]):
            assert abs(comp[:nc, deblend_ref.SUMS[j]].sum() - irow[f]) <= 2.0 * irow[3] * 2.0 ** -53 * imags[j]
        main = comp[:nc, 10] == 1
        assert comp[:nc, 0][main].sum() == irow[4]                          # the main components tile the main island
        assert abs(comp[:nc, 4][main].sum() - irow[16]) <= 2.0 * irow[3] * 2.0 ** -53 * imags[6]
        assert np.array_equal(np.isin(mask, 1 + np.flatnonzero(main)), imask == 2)
    return row


def test_invariants_on_random_windows():
    rng = np.random.default_rng(5)
    n2 = 0
    for t in range(40):
        h, w = int(rng.integers(6, 40)), int(rng.integers(6, 40))
        win = random_window(rng, h, w, plateaus=t % 3 == 0)
        for conn in (8, 4):
            row = invariants(win, (2.5, 1.0, 0.1, [2.5, np.nan, np.inf, 0.5][t % 4]), conn, 1 + t % 4)
            n2 += row[3] >= 2
    lattice = np.full((11, 11), 0.01, np.float32)
    lattice[1::2, 1::2] = 1.0 + np.arange(25, dtype=np.float32).reshape(5, 5) / 32
    row = invariants(lattice, (0.5, 0.2, 0.0, 0.5), 8, 1)
    assert tuple(row[:6]) == (2, 25, 25, 16, 25, 9)
    assert n2 >= 20


def _comp_row(vals, x0=0, y0=0, main=1, nsum=1):
    vals = np.asarray(vals, np.float64)
    yy, xx = np.mgrid[0:vals.shape[0], 0:vals.shape[1]].astype(np.float64)
    k = int(np.argmax(vals))
    return np.array([(vals != 0).sum(), vals.max(), x0 + k % vals.shape[1], y0 + k // vals.shape[1], vals.sum(), (vals * xx).sum(),
                     (vals * yy).sum(), (vals * xx * xx).sum(), (vals * yy * yy).sum(), (vals * xx * yy).sum(), main, nsum], np.float64)


def test_annotate_components():
    a = np.zeros((5, 7)); a[2, 1:6] = [1, 2, 4, 2, 1]                       # horizontal bar centred on (3, 2)
    b = np.zeros((5, 7)); b[4, 6] = 3.0
    comp = np.zeros((3, 16, 12))
    comp[0, 0], comp[0, 1] = _comp_row(a, 100, 200, 1, 2), _comp_row(b, 100, 200, 0, 1)
    comp[1, 0] = _comp_row(a, 100, 200); comp[1, 0, 4:10] = 0.0             # S == 0
    raw = np.array([[0, 3, 2, 2, 6, 0, 0, 0], [2, 1, 17, 1, 5, 4, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0]], np.float64)
    src = [{"x1": 100.0, "y1": 200.0, "x2": 106.0, "y2": 204.0, "score": 0.9} for _ in range(3)]
    with open(os.path.join(ROOT, "tests", "golden", "wcs.json")) as fp:
        w = WCS(json.load(fp)["tan"]["header"])
    out = measure.annotate_components(src, raw, comp, [[100, 200]] * 3, 2.0, w, origin=(10, 20))
    s = out[0]
    assert (s["npeaks"], s["ncomponents"], s["components_truncated"], s["components_unassigned_npix"]) == (2, 2, False, 0)
    c0, c1 = s["components"]
    assert set(c0) == set(measure.COMPONENT_ITEM_KEYS)
    assert (c0["x"], c0["y"], c0["peak"], c0["x_peak"], c0["y_peak"], c0["npix"], c0["flux_sum"], c0["flux"]) == (103.0, 202.0, 4.0, 103, 202, 5, 10.0, 5.0)
    assert c0["main"] is True and c0["nsummits"] == 2 and c1["main"] is False
    assert (c0["major"], c0["minor"], c0["pa"]) == measure.island_shape(*comp[0, 0, 4:10]) and c0["minor"] == 0.0 and c0["pa"] == 0.0
    ra, dec = w.wcs_pix2world(103.0 + 10.0, 202.0 + 20.0, 0)
    assert c0["ra"] == float(ra) and c0["dec"] == float(dec)
    assert (c1["x"], c1["y"], c1["npix"], c1["major"]) == (106.0, 204.0, 1, 0.0)
    s = out[1]                                                              # truncated, S == 0
    assert s["components_truncated"] is True and s["npeaks"] == 17 and s["components_unassigned_npix"] == 4 and len(s["components"]) == 1
    c = s["components"][0]
    assert all(c[k] is None for k in ("x", "y", "ra", "dec", "major", "minor", "pa")) and c["flux_sum"] == 0.0 and c["flux"] == 0.0 and c["peak"] == 4.0
    s = out[2]                                                              # no seed
    assert (s["npeaks"], s["ncomponents"], s["components_truncated"], s["components_unassigned_npix"], s["components"]) == (0, 0, False, 0, [])
    json.dumps(out)
    big = raw[:1].copy(); big[0, 0] = 1.0                                   # window above the supported maximum
    s = measure.annotate_components([dict(src[0])], big, comp[:1], [[0, 0]], 0, None)[0]
    assert all(s[k] is None for k in measure.COMPONENT_KEYS)
    s = measure.annotate_components([dict(src[0])], raw[:1], comp[:1], [[100, 200]], 0, None)[0]      # no beam, no WCS
    assert s["components"][0]["flux"] is None and s["components"][0]["ra"] is None and s["components"][0]["x"] == 103.0
    assert measure.annotate_components([], np.zeros((0, 8)), np.zeros((0, 16, 12)), np.zeros((0, 2)), 1.0, None) == []


def test_deblend_thresholds():
    src = [{"bkg": 0.5, "rms": 0.25, "bkg_map": 1.0, "rms_map": 0.5}, {"bkg": -1e-3, "rms": 3e-4, "bkg_map": 0.0, "rms_map": 0.0}]
    t = measure.deblend_thresholds(src, 5.0, 2.5, 4.0)
    assert t.dtype == np.float64 and t.shape == (2, 4)
    for s, r in zip(src, t):
        assert tuple(r) == (s["bkg"] + 5.0 * s["rms"], s["bkg"] + 2.5 * s["rms"], s["bkg"], s["bkg"] + 4.0 * s["rms"])
    assert np.array_equal(t[:, :3], measure.island_thresholds(src, 5.0, 2.5))
    t = measure.deblend_thresholds(src, 5.0, 2.5, 3.0, use_map=True)
    assert tuple(t[0]) == (3.5, 2.25, 1.0, 2.5) and tuple(t[1]) == (0.0, 0.0, 0.0, 0.0)
    rows = np.array([[0, 0, s["bkg"], s["rms"]] for s in src])
    assert np.array_equal(measure.deblend_thresholds(src, 5.0, 2.5, 4.0), deblend_ref.thresholds(rows, 5.0, 2.5, 4.0))
    assert measure.deblend_config({"island_seed_sigma": 4.0}) == (4.0, 2)
    assert measure.deblend_config({"island_seed_sigma": 4.0, "deblend_peak_sigma": 3.0, "deblend_radius": 5}) == (3.0, 5)


def test_exports_and_fields():
    from caesar_yolo_amd import lib as L
    from caesar_yolo_amd.model import HipDetector
    assert "cy_deblend_islands" in L.EXPORTS and "cy_deblend_kernel_ms" in L.EXPORTS
    assert L.CY_DBL_FIELDS == len(L.DBL_NAMES) == len(deblend_ref.FIELDS) == 8 and tuple(L.DBL_NAMES) == deblend_ref.FIELDS
    assert L.CY_DBL_COMP_FIELDS == len(L.DBL_COMP_NAMES) == len(deblend_ref.COMP_FIELDS) == 12 and tuple(L.DBL_COMP_NAMES) == deblend_ref.COMP_FIELDS
    assert L.CY_DBL_MAX_COMP == deblend_ref.MAX_COMP == 16
    assert callable(HipDetector.deblend_islands) and callable(HipDetector.deblend_kernel_ms)
    hdr = open(os.path.join(ROOT, "include", "caesar_yolo_hip.h")).read()
    assert "#define CY_DBL_MAX_COMP 16" in hdr and "#define CY_DBL_FIELDS 8" in hdr and "#define CY_DBL_COMP_FIELDS 12" in hdr


def test_cli_flags():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import run
    a = run.parse_args(["--weights=seeded:l:5"])
    assert a.deblend_islands is False and a.measure_islands is False and a.deblend_radius == 2 and a.deblend_peak_sigma == 5.0
    a = run.parse_args(["--weights=seeded:l:5", "--deblend_islands"])
    assert a.deblend_islands is True and a.measure_islands is True           # the implication
    a = run.parse_args(["--weights=seeded:l:5", "--deblend_islands", "--island_seed_sigma", "4"])
    assert a.deblend_peak_sigma == 4.0                                      # the default follows the seed threshold
    a = run.parse_args(["--weights=seeded:l:5", "--deblend_islands", "--island_seed_sigma", "4", "--deblend_peak_sigma=6.5", "--deblend_radius", "8"])
    assert a.deblend_peak_sigma == 6.5 and a.deblend_radius == 8 and a.island_seed_sigma == 4.0
    for r in ("0", "9", "-1"):
        with pytest.raises(SystemExit):
            run.parse_args(["--weights=seeded:l:5", "--deblend_radius", r])
    fits = os.path.join(ROOT, "tests", "golden", "galaxy0001.fits")
    bad = run.parse_args(["--weights=seeded:l:5", "--image=" + fits, "--deblend_islands", "--island_seed_sigma=2", "--island_merge_sigma=3"])
    assert run.validate_args(bad) == -1                                     # the implied island step checks its thresholds
    from caesar_yolo_amd.config import CONFIG
    assert CONFIG["deblend_islands"] is False and CONFIG["deblend_peak_sigma"] is None and CONFIG["deblend_radius"] == 2
