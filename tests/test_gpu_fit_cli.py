"""--fit_components end to end through scripts/run.py on the 2048 x 2048 synthetic FITS mosaic of tests/test_gpu_islands_cli.py
(same recipe), tiled and serial, each with and without --bkg_map.  Every component carries measure.FIT_KEYS; their values equal
the deblend and fit steps of a measure.Chain started on the written catalog's boxes (the kernels are deterministic and
the host arithmetic is the same code, so equal means equal); and a run with only --deblend_islands writes the catalog the
--fit_components run writes with the fit_ keys deleted, byte for byte: the switch adds keys and changes nothing else."""
import copy
import json

import numpy as np
import pytest
import torch

from gpu_common import detector
from test_gpu_islands_cli import COMMON, N, TILED, WCS_CARDS, _run, _strip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mosaic(tmp_path_factory):
    from caesar_yolo_amd import synth, utils
    from caesar_yolo_amd.wcs import WCS
    d = tmp_path_factory.mktemp("fit_cli")
    img = synth.make_mosaic(n=N, seed=11)
    path = str(d / "sky.fits")
    utils.write_fits_image(path, img, synth.FITS_CARDS + WCS_CARDS)
    _, header = utils.read_fits_image(path)
    c = dict(synth.FITS_CARDS)
    beam = np.pi * c["BMAJ"] * c["BMIN"] / (4 * np.log(2)) / np.abs(c["CDELT1"] * c["CDELT2"])       # SFinder._beam_info
    return d, path, img, beam, WCS(header)


def _no_fit(sources):
    out = copy.deepcopy(sources)
    for s in out:
        for c in s.get("components") or []:
            for k in [k for k in c if k.startswith("fit_")]:
                del c[k]
    return out


def _direct(sources, img, beam, wcs, origin, use_map, k_seed=5.0, k_merge=2.5, k_peak=5.0, conn=8, radius=2, max_iter=64):
    """The component and fit steps called directly on the catalog's boxes, from its own bkg / rms keys."""
    from caesar_yolo_amd import measure
    det = detector("fp32", max_batch=1, max_imgsz=160)
    dev = det.mosaic_to_device(np.ascontiguousarray(img))
    torch.cuda.synchronize()
    want = copy.deepcopy(_strip(sources, measure.COMPONENT_KEYS))
    config = {"bkg_map": use_map, "island_seed_sigma": k_seed, "island_merge_sigma": k_merge, "deblend_peak_sigma": k_peak, "island_conn": conn,
              "deblend_radius": radius, "fit_max_iter": max_iter}
    chain = measure.Chain(det, dev, want, config, beam, wcs, wcs_origin=origin)
    chain.deblend()
    chain.fit()
    return want, chain.fit_rows


def _check(sources, want, rows):
    from caesar_yolo_amd import measure
    ncmp = nfit = 0
    for s, w in zip(sources, want):
        assert (s["components"] is None) == (w["components"] is None)
        for c, d in zip(s["components"] or [], w["components"] or []):
            assert set(measure.FIT_KEYS) <= set(c)
            assert c == d, (c, d)
            ncmp += 1
            nfit += c["fit_status"] == 0
    assert nfit > 0 and measure.fit_iterations(rows)[0] >= nfit
    return ncmp, nfit


@pytest.fixture(scope="module")
def tiled(mosaic):
    d, path = mosaic[0], mosaic[1]
    dirs = {}
    for name, extra in (("dbl", ["--deblend_islands"]), ("fit", ["--fit_components"]),
                        ("map", ["--fit_components", "--bkg_map", "--deblend_peak_sigma=4", "--fit_max_iter=40"])):
        (d / name).mkdir()
        _run(["--image=" + path] + TILED + extra, str(d / name))
        dirs[name] = d / name
    return dirs


def test_tiled(mosaic, tiled):
    from caesar_yolo_amd import measure
    d, path, img, beam, wcs = mosaic
    raw_dbl = open(tiled["dbl"] / "catalog_sky.json", "rb").read()
    cat_fit = json.load(open(tiled["fit"] / "catalog_sky.json"))["sources"]
    cat_map = json.load(open(tiled["map"] / "catalog_sky.json"))["sources"]
    assert b"fit_" not in raw_dbl and len(cat_fit) > 20
    # without the switch: the same command with only --deblend_islands writes these bytes
    assert json.dumps({"sources": _no_fit(cat_fit)}, indent=2, sort_keys=True).encode() == raw_dbl
    ncmp, nfit = _check(cat_fit, *_direct(cat_fit, img, beam, wcs, (0, 0), False))
    ncmp2, nfit2 = _check(cat_map, *_direct(cat_map, img, beam, wcs, (0, 0), True, k_peak=4.0, max_iter=40))
    assert ncmp > 20 and ncmp2 > 20
    fitted = [c for s in cat_fit for c in s["components"] or [] if c["fit_status"] == 0]
    assert all(c["fit_flux"] is not None and c["fit_ra"] is not None and c["fit_major"] >= c["fit_minor"] > 0 for c in fitted)
    assert any(c["fit_flux_err"] is not None for c in fitted)


@pytest.mark.parametrize("bkg_map", [False, True])
def test_serial_crop(mosaic, tiled, bkg_map):
    from caesar_yolo_amd import measure
    d, path, img, beam, wcs = mosaic
    ser = d / ("serial_map" if bkg_map else "serial")
    ser.mkdir()
    per_tile = {}                                             # the crop = the tile of the tiled run with the most fitted components
    for s in json.load(open(tiled["fit"] / "catalog_sky.json"))["sources"]:
        t = (int(s["x1"]) // 256, int(s["y1"]) // 256)
        if s["ncomponents"] and not s["merged"] and not s["edge"] and t != (0, 0) and t == (int(s["x2"]) // 256, int(s["y2"]) // 256):
            per_tile[t] = per_tile.get(t, 0) + sum(c["fit_status"] == 0 for c in s["components"])
    (tx, ty), _ = max(per_tile.items(), key=lambda kv: (kv[1], kv[0]))
    xmin, xmax, ymin, ymax = tx * 256, tx * 256 + 256, ty * 256, ty * 256 + 256
    args = ["--image=" + path] + COMMON + ["--xmin=%d" % xmin, "--xmax=%d" % xmax, "--ymin=%d" % ymin, "--ymax=%d" % ymax]
    extra = ["--island_seed_sigma=4", "--island_merge_sigma=2", "--island_conn=4", "--deblend_radius=1"] + (["--bkg_map", "--bkg_cell=64"] if bkg_map else [])
    _run(args + ["--fit_components"] + extra, str(ser))
    objs = json.load(open(ser / "out_sky.json"))["objs"]
    (ser / "dbl").mkdir()
    _run(args + ["--deblend_islands"] + extra, str(ser / "dbl"))
    plain = json.load(open(ser / "dbl" / "out_sky.json"))["objs"]
    assert "fit_" not in json.dumps(plain) and _no_fit(objs) == plain
    crop = np.ascontiguousarray(img[ymin:ymax, xmin:xmax])
    want, rows = _direct(objs, crop, beam, wcs, (xmin, ymin), bkg_map, 4.0, 2.0, 4.0, 4, 1)
    ncmp, nfit = _check(objs, want, rows)
    have = [c for o in objs for c in (o["components"] or []) if c["fit_status"] == 0]
    near = [c for c in have if abs(c["fit_x"] - c["x_peak"]) <= 2 and abs(c["fit_y"] - c["y_peak"]) <= 2]       # crop-relative pixels, as the peaks
    assert have and len(near) >= len(have) // 2
    a, dd = wcs.wcs_pix2world(have[0]["fit_x"], have[0]["fit_y"], 0)
    assert (float(a), float(dd)) != (have[0]["fit_ra"], have[0]["fit_dec"])       # the sky position is NOT the crop-relative pixel's
