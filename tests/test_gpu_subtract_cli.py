"""--subtract_peaks end to end through scripts/run.py on the 1024 x 1024 synthetic FITS mosaic of tests/test_gpu_peaks_cli.py (three
isolated blobs of 200 times the noise that no box needs to hold), tiled and serial, with --fit_blends --bkg_map --residual_map
--residual_peaks --residual_holes --fit_peak_groups --save_residual_maps.
  - with "residual_peaks_left" / "residual_holes_left" removed, the gres_ keys stripped from the entries and res_npeaks_left,
    res_nholes_left from the sources, the catalog equals the catalog written without the switch byte for byte
  - the lists, the gres_ keys and the two counts equal those of a measure.Chain started on the catalog's boxes with subtract() called
    last (the kernels are deterministic and the host arithmetic is the same code, so equal means equal)
  - peakmodel_<name>.fits / resid2_<name>.fits hold the bytes of that chain's maps, and are written only with the switch
  - subtract_ms and its companions are in the stats only with the switch
  - every blob that lies in no box is a fitted residual peak that was subtracted, and no entry of either left list lies within 3 px of it
  - the serial run's lists are in the frame of its crop."""
import json
import os

import numpy as np
import pytest
import torch

from gpu_common import detector
from test_disc_residual_cpu import SUBTRACT_STATS
from test_gpu_islands_cli import COMMON, _strip
from test_gpu_peaks_cli import SOURCE_KEYS, mosaic  # noqa: F401  (the fixture: the mosaic with the blobs)
from test_gpu_residual_cli import N, TILED, _run, _without

pytestmark = pytest.mark.gpu

PLAIN = ["--fit_blends", "--bkg_map", "--residual_map", "--residual_peaks", "--residual_holes", "--fit_peak_groups", "--save_residual_maps"]
SUBTRACT = PLAIN + ["--subtract_peaks"]
LEFT = ("residual_peaks_left", "residual_holes_left")
STEPS = ("deblend", "fit", "blend", "residual", "peaks", "peak_fits", "peak_groups", "subtract")


def _direct(sources, img, beam, wcs, origin, cell):
    """The steps from the components on, then the searches, the fits, the groups and subtract(), called directly on the catalog's
    boxes and its own bkg_map / rms_map keys.  -> the chain (its sources annotated)."""
    from caesar_yolo_amd import measure
    det = detector("fp32", max_batch=1, max_imgsz=160)
    dev = det.mosaic_to_device(np.ascontiguousarray(img))
    torch.cuda.synchronize()
    want = _without(_strip(sources, SOURCE_KEYS + measure.SOURCE_LEFT_KEYS))
    config = {"bkg_map": True, "bkg_cell": cell, "residual_peaks": True, "residual_holes": True, "fit_peak_groups": True, "subtract_peaks": True}
    chain = measure.Chain(det, dev, want, config, beam, wcs, wcs_origin=origin)
    chain.mesh, _ = measure.fill_mesh(det.measure_background(dev, cell=cell, k=3.0, niter=3), 64)
    for step in STEPS:
        getattr(chain, step)()
    return chain


def _plain_of(doc, key):
    from caesar_yolo_amd import measure
    out = {k: v for k, v in doc.items() if k not in LEFT}
    out[key] = _strip(doc[key], measure.SOURCE_LEFT_KEYS)
    for name in ("residual_peaks", "residual_holes"):
        out[name] = _strip(doc[name], measure.GRES_KEYS)
    return json.dumps(out, indent=2, sort_keys=True).encode()


def _check(doc, key, d, name, img, beam, wcs, origin, cell):
    from caesar_yolo_amd import measure, utils
    chain = _direct(doc[key], img, beam, wcs, origin, cell)
    lists = json.loads(json.dumps(measure.peak_lists(chain)))
    assert list(lists) == ["residual_peaks", "residual_holes"] + list(LEFT)
    for nm in lists:
        assert doc[nm] == lists[nm], nm
    for s, w in zip(doc[key], chain.sources):
        for k in measure.SOURCE_LEFT_KEYS:
            assert s[k] == w[k], (k, s[k], w[k])
    for nm, cnt in zip(LEFT, measure.SOURCE_LEFT_KEYS):
        assert all(tuple(sorted(p)) == tuple(sorted(measure.PEAK_KEYS)) for p in doc[nm])
        for s in doc[key]:
            assert s[cnt] == sum(s["x1"] <= p["x_peak"] <= s["x2"] and s["y1"] <= p["y_peak"] <= s["y2"] for p in doc[nm])
    assert all(p["peak"] > 0 for p in doc[LEFT[0]]) and all(p["peak"] < 0 for p in doc[LEFT[1]])
    for tag, m in (("peakmodel_", chain.peak_model), ("resid2_", chain.resid2), ("model_", chain.model), ("resid_", chain.resid)):
        got = utils.read_fits_image(str(d / (tag + name + ".fits")))[0]
        assert np.asarray(got, np.float32).tobytes() == m.cpu().numpy().tobytes(), tag
    fitted = [p for nm in ("residual_peaks", "residual_holes") for p in doc[nm]]
    assert fitted and all(p["gres_subtracted"] is not None for p in fitted)
    return chain


@pytest.fixture(scope="module")
def tiled(mosaic):  # noqa: F811
    d, path = mosaic[0], mosaic[1]
    dirs = {}
    for name, extra in (("plain2", PLAIN), ("subtract", SUBTRACT)):
        (d / name).mkdir()
        _run(["--image=" + path] + TILED + extra, str(d / name))
        dirs[name] = d / name
    return dirs


def test_tiled(mosaic, tiled):  # noqa: F811
    d, path, img, beam, wcs, blobs = mosaic
    raw_plain = open(tiled["plain2"] / "catalog_sky.json", "rb").read()
    doc = json.load(open(tiled["subtract"] / "catalog_sky.json"))
    assert set(doc) == {"sources", "residual_peaks", "residual_holes"} | set(LEFT)
    assert b"gres_" not in raw_plain and b"_left" not in raw_plain and b"gblend_" in raw_plain
    assert _plain_of(doc, "sources") == raw_plain
    assert not os.path.exists(tiled["plain2"] / "resid2_catalog_sky.fits") and not os.path.exists(tiled["plain2"] / "peakmodel_catalog_sky.fits")
    chain = _check(doc, "sources", tiled["subtract"], "catalog_sky", img, beam, wcs, (0, 0), 128)
    seen = [json.load(open(tiled[k] / "stats.json")) for k in ("plain2", "subtract")]
    assert not set(seen[0]) & SUBTRACT_STATS and "peakgroup_ms" in seen[0] and SUBTRACT_STATS <= set(seen[1])
    st = chain.subtract_stats
    for k in SUBTRACT_STATS:
        assert seen[1][k] >= 0
        if not k.endswith("_ms"):
            assert seen[1][k] == st[k], k
    assert (seen[1]["left_peaks"], seen[1]["left_holes"]) == (len(doc[LEFT[0]]), len(doc[LEFT[1]])) and seen[1]["subtract_rendered"] >= 1
    print("tiled %d x %d: %d sources, %d peaks and %d holes fitted, %d selected, %d rendered, %d wandered; left: %d peaks, %d holes" % (
        N, N, len(doc["sources"]), len(doc["residual_peaks"]), len(doc["residual_holes"]), st["subtract_selected"], st["subtract_rendered"],
        st["subtract_wandered"], st["left_peaks"], st["left_holes"]))
    for cx, cy in blobs:
        boxed = [s for s in doc["sources"] if s["x1"] <= cx <= s["x2"] and s["y1"] <= cy <= s["y2"]]
        near = [p for p in doc["residual_peaks"] if abs(p["x_peak"] - cx) <= 1 and abs(p["y_peak"] - cy) <= 1 and p["in_source"] is None]
        if boxed:
            continue
        assert near and near[0]["gres_subtracted"] is True and near[0]["gres_npix"] > 0, (cx, cy)
        assert not [p for nm in LEFT for p in doc[nm] if np.hypot(p["x_peak"] - cx, p["y_peak"] - cy) <= 3.0], (cx, cy)
        print("blob at (%d, %d): snr %.1f, subtracted from its %s fit, gres_ratio %.3g" % (cx, cy, near[0]["snr"], near[0]["gres_source"], near[0]["gres_ratio"]))


def test_serial_crop(mosaic, tiled):  # noqa: F811
    d, path, img, beam, wcs, blobs = mosaic
    fitted = json.load(open(tiled["subtract"] / "catalog_sky.json"))["residual_peaks"]
    per_tile = {}                                             # the crop = the tile of the tiled run with the most subtracted peaks (not the first)
    for p in fitted:
        t = (p["x_peak"] // 256, p["y_peak"] // 256)
        if t != (0, 0) and p["gres_subtracted"]:
            per_tile[t] = per_tile.get(t, 0) + 1
    (tx, ty), _ = max(per_tile.items(), key=lambda kv: (kv[1], kv[0]))
    xmin, xmax, ymin, ymax = tx * 256, tx * 256 + 256, ty * 256, ty * 256 + 256
    args = ["--image=" + path] + COMMON + ["--xmin=%d" % xmin, "--xmax=%d" % xmax, "--ymin=%d" % ymin, "--ymax=%d" % ymax, "--bkg_cell=64"]
    docs = {}
    for name, extra in (("plain2", PLAIN), ("subtract", SUBTRACT)):
        (d / ("serial_" + name)).mkdir()
        _run(args + extra, str(d / ("serial_" + name)))
        docs[name] = open(d / ("serial_" + name) / "out_sky.json", "rb").read()
    doc = json.loads(docs["subtract"])
    assert set(doc) == {"image_id", "objs", "residual_peaks", "residual_holes"} | set(LEFT)
    assert b"gres_" not in docs["plain2"] and b"_left" not in docs["plain2"]
    assert _plain_of(doc, "objs") == docs["plain2"]
    crop = np.ascontiguousarray(img[ymin:ymax, xmin:xmax])
    chain = _check(doc, "objs", d / "serial_subtract", "out_sky", crop, beam, wcs, (xmin, ymin), 64)
    print("serial crop x %d.. y %d..: %d sources, %d selected, %d rendered; left: %d peaks, %d holes" % (
        xmin, ymin, len(doc["objs"]), chain.subtract_stats["subtract_selected"], chain.subtract_stats["subtract_rendered"],
        chain.subtract_stats["left_peaks"], chain.subtract_stats["left_holes"]))
    for p in doc["residual_peaks"] + doc["residual_holes"]:    # the frame of the crop, which is the frame of its boxes
        if p["gres_x_max"] is not None:
            assert 0 <= p["gres_x_max"] < xmax - xmin and 0 <= p["gres_y_max"] < ymax - ymin
            assert abs(p["gres_x_max"] - p["x"]) <= 6.0 and abs(p["gres_y_max"] - p["y"]) <= 6.0
    for p in doc[LEFT[0]] + doc[LEFT[1]]:
        assert 0 <= p["x_peak"] < xmax - xmin and 0 <= p["y_peak"] < ymax - ymin
