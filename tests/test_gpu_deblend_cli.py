"""--deblend_islands end to end through scripts/run.py on the 2048 x 2048 synthetic FITS mosaic of tests/test_gpu_islands_cli.py
(same recipe), tiled and serial, with and without --bkg_map: without the switch the catalog is what it was; with it every source
carries measure.COMPONENT_KEYS beside the others, and they are what the reference (tests/deblend_ref.py on the host image,
thresholds from the catalog's own bkg and rms, or bkg_map and rms_map) and measure.annotate_components give.

Comparison rules: counts, flags, peak values and peak positions equal; flux_sum within 2 m 2^-53 sum|t_i| of the reference (m = npix
of the component); x = wx0 + Sx / S within (B_Sx + |Sx / S| B_S) / (|S| - B_S) plus the rounding of the division and the addition;
flux, ra, dec are float64 functions of values the catalog itself holds and must equal them exactly; major, minor, pa within the
bounds tests/test_gpu_islands_cli.py derives from those of the sums (shape_bounds, on the component's sums)."""
import copy
import json

import numpy as np
import pytest

import deblend_ref
from test_gpu_islands_cli import COMMON, EPS, N, OLD_KEYS, TILED, WCS_CARDS, _run, _strip, shape_bounds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mosaic(tmp_path_factory):
    from caesar_yolo_amd import synth, utils
    from caesar_yolo_amd.wcs import WCS
    d = tmp_path_factory.mktemp("deblend_cli")
    img = synth.make_mosaic(n=N, seed=11)
    path = str(d / "sky.fits")
    utils.write_fits_image(path, img, synth.FITS_CARDS + WCS_CARDS)
    _, header = utils.read_fits_image(path)
    host = np.where(np.isfinite(img), img, np.float32(0)).astype(np.float32)
    c = dict(synth.FITS_CARDS)
    beam = np.pi * c["BMAJ"] * c["BMIN"] / (4 * np.log(2)) / np.abs(c["CDELT1"] * c["CDELT2"])       # SFinder._beam_info
    return d, path, host, beam, WCS(header)


@pytest.fixture(scope="module")
def tiled(mosaic):
    """The one-rank tiled run without a switch, with --deblend_islands and with --deblend_islands --bkg_map."""
    d, path = mosaic[0], mosaic[1]
    dirs = []
    for name, extra in (("off", []), ("dbl", ["--deblend_islands"]), ("map", ["--deblend_islands", "--bkg_map", "--deblend_peak_sigma=4", "--deblend_radius=3"])):
        (d / name).mkdir()
        _run(["--image=" + path] + TILED + extra, str(d / name))
        dirs.append(d / name)
    return dirs


def _check(sources, host, beam, wcs, origin, k_seed=5.0, k_merge=2.5, k_peak=5.0, conn=8, radius=2, use_map=False):
    """Every source's component keys against the reference on `host` (the analysed image; origin = where it sits in the FITS frame).
    -> (sources with two or more components, components compared)"""
    from caesar_yolo_amd import measure
    boxes = measure.boxes_of(sources)
    kb, kr = ("bkg_map", "rms_map") if use_map else ("bkg", "rms")
    thr4 = deblend_ref.thresholds(np.array([[0.0, 0.0, s[kb], s[kr]] for s in sources], np.float64).reshape(-1, 4), k_seed, k_merge, k_peak)
    rows, comps, _, mags = deblend_ref.deblend(host, boxes, thr4, conn, radius)
    win0 = np.array([measure.box_window(b, host.shape[0], host.shape[1])[:2] for b in boxes], np.float64)
    want = measure.annotate_components(copy.deepcopy(_strip(sources, measure.COMPONENT_KEYS)), rows, comps, win0, beam, wcs, origin)
    multi = ncmp = 0
    for i, (s, w) in enumerate(zip(sources, want)):
        assert set(s) == set(w), (sorted(s), sorted(w))
        for k in ("npeaks", "ncomponents", "components_truncated", "components_unassigned_npix"):
            assert s[k] == w[k] and type(s[k]) is type(w[k]), "source %d %s: %r in the catalog, %r from the reference" % (i, k, s[k], w[k])
        assert s["ncomponents"] == len(s["components"]) == len(w["components"])
        assert s["island_npix"] == rows[i, 4] and sum(c["npix"] for c in s["components"]) + s["components_unassigned_npix"] == s["island_npix"]
        multi += s["ncomponents"] >= 2
        for k, (c, v) in enumerate(zip(s["components"], w["components"])):
            assert set(c) == set(measure.COMPONENT_ITEM_KEYS)
            for f in ("peak", "x_peak", "y_peak", "npix", "main", "nsummits"):
                assert c[f] == v[f] and type(c[f]) is type(v[f]), "source %d component %d %s: %r in the catalog, %r from the reference" % (i, k, f, c[f], v[f])
            m = comps[i, k, 0]
            b_S, b_Sx, b_Sy = (2.0 * m * EPS * t for t in mags[i, k, :3])
            assert abs(c["flux_sum"] - v["flux_sum"]) <= b_S
            assert c["flux"] == c["flux_sum"] / beam
            S = abs(comps[i, k, 4])
            if v["x"] is None or S - b_S <= 0:
                assert comps[i, k, 4] == 0 and all(c[f] is None for f in ("x", "y", "ra", "dec", "major", "minor", "pa"))
                continue
            for f, b, j in (("x", b_Sx, 5), ("y", b_Sy, 6)):
                q = abs(comps[i, k, j] / comps[i, k, 4])
                bound = (b + q * b_S) / (S - b_S) + 4 * EPS * (q + abs(v[f]))
                assert abs(c[f] - v[f]) <= bound, "source %d component %d %s: %r in the catalog, %r from the reference, bound %g" % (i, k, f, c[f], v[f], bound)
            a, d = wcs.wcs_pix2world(c["x"] + origin[0], c["y"] + origin[1], 0)
            assert c["ra"] == float(a) and c["dec"] == float(d)
            assert np.isfinite([c["major"], c["minor"], c["pa"]]).all() and c["major"] >= c["minor"] >= 0 and -90 < c["pa"] <= 90
            pseudo = np.zeros(20)
            pseudo[3], pseudo[10:16] = m, comps[i, k, 4:10]
            b_major, b_minor, b_pa = shape_bounds(pseudo, mags[i, k], v)
            assert abs(c["major"] - v["major"]) <= b_major and abs(c["minor"] - v["minor"]) <= b_minor
            if b_pa is not None:
                assert abs((c["pa"] - v["pa"] + 90.0) % 180.0 - 90.0) <= b_pa
            ncmp += 1
    return multi, ncmp


def test_tiled_catalog_with_and_without_the_switch(mosaic, tiled):
    from caesar_yolo_amd import measure
    d, path, host, beam, wcs = mosaic
    off, dbl, bmap = tiled
    raw_off = open(off / "catalog_sky.json", "rb").read()
    cat_off, cat_dbl, cat_map = json.loads(raw_off), json.load(open(dbl / "catalog_sky.json")), json.load(open(bmap / "catalog_sky.json"))
    assert len(cat_off["sources"]) > 20
    new = set(measure.COMPONENT_KEYS)
    assert all(set(s) == OLD_KEYS for s in cat_off["sources"])                                    # no switch: exactly the old keys
    base = OLD_KEYS | set(measure.KEYS) | set(measure.ISLAND_KEYS)                                # the switch implies the island step
    assert not base & new and not set(measure.BKG_KEYS) & new
    assert all(set(s) == base | new for s in cat_dbl["sources"])
    assert all(set(s) == base | new | set(measure.BKG_KEYS) for s in cat_map["sources"])
    dump = lambda src: json.dumps({"sources": src}, indent=2, sort_keys=True).encode()
    assert dump(_strip(cat_dbl["sources"], measure.COMPONENT_KEYS + measure.ISLAND_KEYS + measure.KEYS)) == raw_off
    assert open(dbl / "ds9_sky.reg", "rb").read() == open(off / "ds9_sky.reg", "rb").read()       # DS9 output unchanged
    multi, ncmp = _check(cat_dbl["sources"], host, beam, wcs, (0, 0))
    multi2, ncmp2 = _check(cat_map["sources"], host, beam, wcs, (0, 0), k_peak=4.0, radius=3, use_map=True)
    assert ncmp > 10 and ncmp2 > 10
    print("%d sources: %d / %d components compared without / with --bkg_map, %d / %d sources with two or more" % (
        len(cat_dbl["sources"]), ncmp, ncmp2, multi, multi2))


@pytest.mark.parametrize("bkg_map", [False, True])
def test_serial_crop(mosaic, tiled, bkg_map):
    from caesar_yolo_amd import measure
    d, path, host, beam, wcs = mosaic
    ser = d / ("serial_map" if bkg_map else "serial")
    ser.mkdir()
    # the crop = the 256 x 256 tile of the tiled run that holds the most sources with a component
    per_tile = {}
    for s in json.load(open(tiled[1] / "catalog_sky.json"))["sources"]:
        t = (int(s["x1"]) // 256, int(s["y1"]) // 256)
        if s["ncomponents"] and not s["merged"] and not s["edge"] and t != (0, 0) and t == (int(s["x2"]) // 256, int(s["y2"]) // 256):
            per_tile[t] = per_tile.get(t, 0) + 1
    (tx, ty), _ = max(per_tile.items(), key=lambda kv: (kv[1], kv[0]))
    xmin, xmax, ymin, ymax = tx * 256, tx * 256 + 256, ty * 256, ty * 256 + 256
    _run(["--image=" + path] + COMMON + ["--xmin=%d" % xmin, "--xmax=%d" % xmax, "--ymin=%d" % ymin, "--ymax=%d" % ymax, "--deblend_islands",
                                         "--island_seed_sigma=4", "--island_merge_sigma=2", "--island_conn=4", "--deblend_radius=1"]
         + (["--bkg_map", "--bkg_cell=64"] if bkg_map else []), str(ser))
    objs = json.load(open(ser / "out_sky.json"))["objs"]
    assert len(objs) > 0 and all(set(measure.KEYS) | set(measure.ISLAND_KEYS) | set(measure.COMPONENT_KEYS) <= set(o) for o in objs)
    # catalog coordinates are relative to the crop; the crop's origin enters the sky position only; the peak threshold follows
    # --island_seed_sigma
    multi, ncmp = _check(objs, np.ascontiguousarray(host[ymin:ymax, xmin:xmax]), beam, wcs, (xmin, ymin), 4.0, 2.0, 4.0, 4, 1, use_map=bkg_map)
    have = [c for o in objs for c in (o["components"] or []) if c["x"] is not None]
    assert ncmp > 0 and have and all(0 <= c["x"] <= xmax - xmin and 0 <= c["x_peak"] < xmax - xmin and 0 <= c["y_peak"] < ymax - ymin for c in have)
    a, dd = wcs.wcs_pix2world(have[0]["x"], have[0]["y"], 0)
    assert (float(a), float(dd)) != (have[0]["ra"], have[0]["dec"])               # the sky position is NOT the crop-relative pixel's
