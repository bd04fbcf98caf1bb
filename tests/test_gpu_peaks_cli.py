"""--residual_peaks --residual_holes end to end through scripts/run.py on the 1024 x 1024 synthetic FITS mosaic of
tests/test_gpu_residual_cli.py plus three isolated blobs of 200 times the noise, tiled and serial, with --fit_blends --bkg_map
--residual_map.
  - with "residual_peaks" / "residual_holes" removed and res_npeaks, res_peak_snr, res_nholes, res_hole_snr stripped from the sources
    the catalog equals the catalog without the two switches byte for byte
  - the two lists and the four keys equal those of a measure.Chain started on the catalog's boxes, peaks() called after residual() (the
    kernels are deterministic and the host arithmetic is the same code, so equal means equal)
  - peaks_ms and its companions are in the stats only with the switch, and peaks_found >= peaks_kept
  - every blob is either inside a catalog box or within 1 px of a kept peak that lies in no source: true whatever the seeded detector
    boxed
  - the serial run's lists are in the frame of its crop."""
import json
import os

import numpy as np
import pytest
import torch

from gpu_common import detector
from test_gpu_islands_cli import COMMON, WCS_CARDS, _strip
from test_gpu_residual_cli import N, TILED, _run, _without

pytestmark = pytest.mark.gpu

NOISE, BLOB_SIGMA = 1e-4, 2.0                                 # synth.make_mosaic's noise
SOURCE_KEYS = ("res_npeaks", "res_peak_snr", "res_nholes", "res_hole_snr")
STAT_KEYS = tuple(p + k for p in ("peaks_", "holes_") for k in ("ms", "kernel_ms", "found", "kept", "truncated"))
PLAIN = ["--fit_blends", "--bkg_map", "--residual_map"]
PEAKS = PLAIN + ["--residual_peaks", "--residual_holes"]


def isolated_positions(img, count=3, half=24, limit=6.0 * NOISE):
    """The first `count` centres of a 64-pixel grid, in row-major order, whose (2 half + 1)^2 window is finite and below `limit`
    everywhere: empty sky, far from every synthetic source."""
    out = []
    for cy in range(64, img.shape[0] - 64, 64):
        for cx in range(64, img.shape[1] - 64, 64):
            w = img[cy - half:cy + half + 1, cx - half:cx + half + 1]
            if np.isfinite(w).all() and np.abs(w).max() < limit and all(abs(cx - x) + abs(cy - y) >= 192 for x, y in out):
                out.append((cx, cy))
                if len(out) == count:
                    return out
    raise AssertionError("the mosaic has no %d empty windows" % count)


@pytest.fixture(scope="module")
def mosaic(tmp_path_factory):
    from caesar_yolo_amd import synth, utils
    from caesar_yolo_amd.wcs import WCS
    d = tmp_path_factory.mktemp("peaks_cli")
    img = synth.make_mosaic(n=N, seed=11)
    blobs = isolated_positions(img)
    yy, xx = np.mgrid[0:N, 0:N].astype(np.float64)
    for cx, cy in blobs:
        img += (200.0 * NOISE * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * BLOB_SIGMA ** 2))).astype(np.float32)
    path = str(d / "sky.fits")
    utils.write_fits_image(path, img, synth.FITS_CARDS + WCS_CARDS)
    _, header = utils.read_fits_image(path)
    c = dict(synth.FITS_CARDS)
    beam = np.pi * c["BMAJ"] * c["BMIN"] / (4 * np.log(2)) / np.abs(c["CDELT1"] * c["CDELT2"])       # SFinder._beam_info
    return d, path, img, beam, WCS(header), blobs


def _direct(sources, img, beam, wcs, origin, cell):
    """The steps from the components on and then peaks(), called directly on the catalog's boxes and its own bkg_map / rms_map keys
    (as tests/test_gpu_residual_cli.py does for the residual step).  -> (the sources so annotated, peak list, hole list)."""
    from caesar_yolo_amd import measure
    det = detector("fp32", max_batch=1, max_imgsz=160)
    dev = det.mosaic_to_device(np.ascontiguousarray(img))
    torch.cuda.synchronize()
    want = _without(_strip(sources, SOURCE_KEYS))
    config = {"bkg_map": True, "bkg_cell": cell, "residual_peaks": True, "residual_holes": True}
    chain = measure.Chain(det, dev, want, config, beam, wcs, wcs_origin=origin)
    chain.mesh, _ = measure.fill_mesh(det.measure_background(dev, cell=cell, k=3.0, niter=3), 64)
    for step in ("deblend", "fit", "blend", "residual", "peaks"):
        getattr(chain, step)()
    return want, chain.peak_list, chain.hole_list, chain.peak_stats


def _check(doc, key, img, beam, wcs, origin, cell):
    sources = doc[key]
    want, peaks, holes, stats = _direct(sources, img, beam, wcs, origin, cell)
    assert doc["residual_peaks"] == json.loads(json.dumps(peaks)) and doc["residual_holes"] == json.loads(json.dumps(holes))
    for s, w in zip(sources, want):
        assert set(SOURCE_KEYS) <= set(s)
        for k in SOURCE_KEYS:
            assert s[k] == w[k], (k, s[k], w[k])
    for lst, nkey, skey in ((doc["residual_peaks"], "res_npeaks", "res_peak_snr"), (doc["residual_holes"], "res_nholes", "res_hole_snr")):
        assert [p["snr"] for p in lst] == sorted((p["snr"] for p in lst), reverse=True)
        for i, s in enumerate(sources):
            inside = [p["snr"] for p in lst if s["x1"] <= p["x_peak"] <= s["x2"] and s["y1"] <= p["y_peak"] <= s["y2"]]
            assert s[nkey] == len(inside) and s[skey] == (max(inside) if inside else None), (i, nkey)
        for p in lst:
            first = [i for i, s in enumerate(sources) if s["x1"] <= p["x_peak"] <= s["x2"] and s["y1"] <= p["y_peak"] <= s["y2"]]
            assert p["in_source"] == (first[0] if first else None)
    assert all(p["peak"] > 0 for p in doc["residual_peaks"]) and all(p["peak"] < 0 for p in doc["residual_holes"])
    return stats


@pytest.fixture(scope="module")
def tiled(mosaic):
    d, path = mosaic[0], mosaic[1]
    dirs = {}
    for name, extra in (("plain", PLAIN), ("peaks", PEAKS)):
        (d / name).mkdir()
        _run(["--image=" + path] + TILED + extra, str(d / name))
        dirs[name] = d / name
    return dirs


def _plain_of(doc, key):
    out = {k: v for k, v in doc.items() if k not in ("residual_peaks", "residual_holes")}
    out[key] = _strip(doc[key], SOURCE_KEYS)
    return json.dumps(out, indent=2, sort_keys=True).encode()


def test_tiled(mosaic, tiled):
    d, path, img, beam, wcs, blobs = mosaic
    raw_plain = open(tiled["plain"] / "catalog_sky.json", "rb").read()
    doc = json.load(open(tiled["peaks"] / "catalog_sky.json"))
    assert set(doc) == {"sources", "residual_peaks", "residual_holes"}
    assert b"residual_peaks" not in raw_plain and b"res_npeaks" not in raw_plain and b"hole" not in raw_plain
    assert _plain_of(doc, "sources") == raw_plain
    stats = _check(doc, "sources", img, beam, wcs, (0, 0), 128)
    seen = [json.load(open(tiled[k] / "stats.json")) for k in ("plain", "peaks")]
    assert not [k for k in seen[0] if k.startswith("peaks_") or k.startswith("holes_")] and "residual_ms" in seen[0]
    assert all(seen[1][k] >= 0 for k in STAT_KEYS)
    for pre, lst in (("peaks_", doc["residual_peaks"]), ("holes_", doc["residual_holes"])):
        assert seen[1][pre + "found"] >= seen[1][pre + "kept"] == len(lst) and seen[1][pre + "truncated"] == 0
        assert (seen[1][pre + "found"], seen[1][pre + "kept"]) == (stats[pre + "found"], stats[pre + "kept"])
    print("tiled %d x %d: %d sources, peaks found %d kept %d (%d in no source), holes found %d kept %d" % (
        N, N, len(doc["sources"]), seen[1]["peaks_found"], seen[1]["peaks_kept"], sum(p["in_source"] is None for p in doc["residual_peaks"]),
        seen[1]["holes_found"], seen[1]["holes_kept"]))
    for cx, cy in blobs:
        boxed = [s for s in doc["sources"] if s["x1"] <= cx <= s["x2"] and s["y1"] <= cy <= s["y2"]]
        near = [p for p in doc["residual_peaks"] if abs(p["x_peak"] - cx) <= 1 and abs(p["y_peak"] - cy) <= 1 and p["in_source"] is None]
        print("blob at (%d, %d): %s" % (cx, cy, "inside a box" if boxed else "a residual peak of snr %.1f" % near[0]["snr"] if near else "lost"))
        assert boxed or near, (cx, cy)


def test_serial_crop(mosaic, tiled):
    d, path, img, beam, wcs, blobs = mosaic
    per_tile = {}                                             # the crop = the tile of the tiled run with the most rendered components
    for s in json.load(open(tiled["peaks"] / "catalog_sky.json"))["sources"]:
        t = (int(s["x1"]) // 256, int(s["y1"]) // 256)
        if s["ncomponents"] and t != (0, 0) and t == (int(s["x2"]) // 256, int(s["y2"]) // 256):
            per_tile[t] = per_tile.get(t, 0) + sum(c["rendered"] for c in s["components"])
    (tx, ty), _ = max(per_tile.items(), key=lambda kv: (kv[1], kv[0]))
    xmin, xmax, ymin, ymax = tx * 256, tx * 256 + 256, ty * 256, ty * 256 + 256
    args = ["--image=" + path] + COMMON + ["--xmin=%d" % xmin, "--xmax=%d" % xmax, "--ymin=%d" % ymin, "--ymax=%d" % ymax, "--bkg_cell=64"]
    docs = {}
    for name, extra in (("plain", PLAIN), ("peaks", PEAKS)):
        (d / ("serial_" + name)).mkdir()
        _run(args + extra, str(d / ("serial_" + name)))
        docs[name] = open(d / ("serial_" + name) / "out_sky.json", "rb").read()
    doc = json.loads(docs["peaks"])
    assert set(doc) == {"image_id", "objs", "residual_peaks", "residual_holes"}
    assert b"residual_peaks" not in docs["plain"] and b"res_npeaks" not in docs["plain"] and b"hole" not in docs["plain"]
    assert _plain_of(doc, "objs") == docs["plain"]
    crop = np.ascontiguousarray(img[ymin:ymax, xmin:xmax])
    stats = _check(doc, "objs", crop, beam, wcs, (xmin, ymin), 64)
    print("serial crop x %d.. y %d..: %d sources, peaks found %d kept %d, holes found %d kept %d" % (
        xmin, ymin, len(doc["objs"]), stats["peaks_found"], stats["peaks_kept"], stats["holes_found"], stats["holes_kept"]))
    for p in doc["residual_peaks"] + doc["residual_holes"]:    # the frame of the crop, which is the frame of its boxes
        assert 0 <= p["x_peak"] < xmax - xmin and 0 <= p["y_peak"] < ymax - ymin
        assert abs(p["x"] - p["x_peak"]) <= 2 and abs(p["y"] - p["y_peak"]) <= 2
