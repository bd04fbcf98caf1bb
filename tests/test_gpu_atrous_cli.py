"""--residual_scales end to end through scripts/run.py on the 1024 x 1024 synthetic FITS mosaic of tests/test_gpu_residual_cli.py plus
two wide faint blobs on empty sky (peak 1.5 times the noise, sigma 9 px), tiled and serial, with --fit_blends --bkg_map --residual_map.
  - with "residual_scale_peaks" removed and res_nscale_peaks, res_scale_peak_snr stripped from the sources the catalog equals the
    catalog of a run without the switch byte for byte
  - the list and the two keys equal those of a measure.Chain started on the catalog's boxes, scale_peaks() called after residual() (the
    kernels are deterministic and the host arithmetic is the same code, so equal means equal)
  - the wav<j>_<name>.fits files of --save_scale_maps hold the planes of that chain, bit for bit, one per searched scale
  - scales_ms and its companions are in the stats only with the switch
  - the list is in decreasing snr; every entry's in_source and every source's keys follow from the boxes
  - the serial run's list is in the frame of its crop."""
import json
import os

import numpy as np
import pytest
import torch

from gpu_common import detector
from test_gpu_islands_cli import COMMON, WCS_CARDS, _strip
from test_gpu_peaks_cli import NOISE, isolated_positions
from test_gpu_residual_cli import N, TILED, _run, _without

pytestmark = pytest.mark.gpu

J, FIRST = 4, 2
SOURCE_KEYS = ("res_nscale_peaks", "res_scale_peak_snr")
STAT_KEYS = ("scales_ms", "atrous_kernel_ms", "scales_background_kernel_ms", "scales_peaks_kernel_ms", "scales_found", "scales_kept",
             "scales_strongest", "scales_truncated")
PLAIN = ["--fit_blends", "--bkg_map", "--residual_map"]
SCALES = PLAIN + ["--residual_scales=%d" % J, "--save_scale_maps"]


@pytest.fixture(scope="module")
def mosaic(tmp_path_factory):
    from caesar_yolo_amd import synth, utils
    from caesar_yolo_amd.wcs import WCS
    d = tmp_path_factory.mktemp("atrous_cli")
    img = synth.make_mosaic(n=N, seed=11)
    blobs = isolated_positions(img, count=2, half=40)
    yy, xx = np.mgrid[0:N, 0:N].astype(np.float64)
    for cx, cy in blobs:
        img += (1.5 * NOISE * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * 9.0 ** 2))).astype(np.float32)
    path = str(d / "sky.fits")
    utils.write_fits_image(path, img, synth.FITS_CARDS + WCS_CARDS)
    _, header = utils.read_fits_image(path)
    c = dict(synth.FITS_CARDS)
    beam = np.pi * c["BMAJ"] * c["BMIN"] / (4 * np.log(2)) / np.abs(c["CDELT1"] * c["CDELT2"])       # SFinder._beam_info
    return d, path, img, beam, WCS(header), blobs


def _direct(sources, img, beam, wcs, origin, cell):
    """The steps from the components on and then scale_peaks(), called directly on the catalog's boxes and its own bkg_map / rms_map
    keys (as tests/test_gpu_peaks_cli.py does for the pixel search).  -> (the sources so annotated, the chain)."""
    from caesar_yolo_amd import measure
    det = detector("fp32", max_batch=1, max_imgsz=160)
    dev = det.mosaic_to_device(np.ascontiguousarray(img))
    torch.cuda.synchronize()
    want = _without(_strip(sources, SOURCE_KEYS))
    config = {"bkg_map": True, "bkg_cell": cell, "residual_scales": J, "residual_scale_first": FIRST, "save_scale_maps": True}
    chain = measure.Chain(det, dev, want, config, beam, wcs, wcs_origin=origin)
    chain.mesh, _ = measure.fill_mesh(det.measure_background(dev, cell=cell, k=3.0, niter=3), 64)
    for step in ("deblend", "fit", "blend", "residual", "scale_peaks"):
        getattr(chain, step)()
    return want, chain


def _check(doc, key, out_dir, name, img, beam, wcs, origin, cell):
    from caesar_yolo_amd import utils
    sources, lst = doc[key], doc["residual_scale_peaks"]
    want, chain = _direct(sources, img, beam, wcs, origin, cell)
    assert lst == json.loads(json.dumps(chain.scale_list))
    for s, w in zip(sources, want):
        for k in SOURCE_KEYS:
            assert s[k] == w[k], (k, s[k], w[k])
    assert [p["snr"] for p in lst] == sorted((p["snr"] for p in lst), reverse=True)
    assert all(FIRST <= p["scale"] <= J and p["step"] == 1 << (p["scale"] - 1) and p["snr"] >= 5.0 and p["peak"] > 0 for p in lst)
    for i, s in enumerate(sources):
        inside = [p["snr"] for p in lst if s["x1"] <= p["x_peak"] <= s["x2"] and s["y1"] <= p["y_peak"] <= s["y2"]]
        assert s["res_nscale_peaks"] == len(inside) and s["res_scale_peak_snr"] == (max(inside) if inside else None), i
    for p in lst:
        first = [i for i, s in enumerate(sources) if s["x1"] <= p["x_peak"] <= s["x2"] and s["y1"] <= p["y_peak"] <= s["y2"]]
        assert p["in_source"] == (first[0] if first else None)
    # the saved planes: one file per searched scale and no other, equal to the chain's planes
    files = sorted(f for f in os.listdir(out_dir) if f.startswith("wav"))
    assert files == ["wav%d_%s.fits" % (j, name) for j in range(FIRST, J + 1)]
    for j in range(FIRST, J + 1):
        plane, _ = utils.read_fits_image(os.path.join(out_dir, "wav%d_%s.fits" % (j, name)))
        got, ref = np.ascontiguousarray(plane, np.float32), chain.scale_planes[j].cpu().numpy()
        assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), j
    return chain.scale_stats


def _plain_of(doc, key):
    out = {k: v for k, v in doc.items() if k != "residual_scale_peaks"}
    out[key] = _strip(doc[key], SOURCE_KEYS)
    return json.dumps(out, indent=2, sort_keys=True).encode()


@pytest.fixture(scope="module")
def tiled(mosaic):
    d, path = mosaic[0], mosaic[1]
    dirs = {}
    for name, extra in (("plain", PLAIN), ("scales", SCALES)):
        (d / name).mkdir()
        _run(["--image=" + path] + TILED + extra, str(d / name))
        dirs[name] = d / name
    return dirs


def test_tiled(mosaic, tiled):
    d, path, img, beam, wcs, blobs = mosaic
    raw_plain = open(tiled["plain"] / "catalog_sky.json", "rb").read()
    doc = json.load(open(tiled["scales"] / "catalog_sky.json"))
    assert set(doc) == {"sources", "residual_scale_peaks"}
    assert b"scale" not in raw_plain and not [f for f in os.listdir(tiled["plain"]) if f.startswith("wav")]
    assert _plain_of(doc, "sources") == raw_plain
    stats = _check(doc, "sources", str(tiled["scales"]), "catalog_sky", img, beam, wcs, (0, 0), 128)
    seen = [json.load(open(tiled[k] / "stats.json")) for k in ("plain", "scales")]
    assert not [k for k in seen[0] if k.startswith("scales_") or k.startswith("atrous_")] and "residual_ms" in seen[0]
    assert not [k for k in seen[1] if k.startswith("peaks_")]            # the pixel search stays off
    assert set(seen[0]) | set(STAT_KEYS) == set(seen[1]) and all(seen[1][k] >= 0 for k in STAT_KEYS)
    lst = doc["residual_scale_peaks"]
    assert seen[1]["scales_found"] >= seen[1]["scales_kept"] == len(lst) >= seen[1]["scales_strongest"] == sum(p["strongest"] for p in lst)
    assert (seen[1]["scales_found"], seen[1]["scales_kept"], seen[1]["scales_truncated"]) == (stats["scales_found"], stats["scales_kept"], 0)
    print("tiled %d x %d: %d sources, scale peaks found %d kept %d strongest %d (%d in no source)" % (
        N, N, len(doc["sources"]), seen[1]["scales_found"], seen[1]["scales_kept"], seen[1]["scales_strongest"], sum(p["in_source"] is None for p in lst)))
    for cx, cy in blobs:
        near = [p for p in lst if abs(p["x_peak"] - cx) <= 4 and abs(p["y_peak"] - cy) <= 4]
        print("blob at (%d, %d): %s" % (cx, cy, [(p["scale"], round(p["snr"], 1), p["strongest"]) for p in near]))


def test_serial_crop(mosaic, tiled):
    d, path, img, beam, wcs, blobs = mosaic
    per_tile = {}                                             # the crop = the tile of the tiled run with the most rendered components
    for s in json.load(open(tiled["scales"] / "catalog_sky.json"))["sources"]:
        t = (int(s["x1"]) // 256, int(s["y1"]) // 256)
        if s["ncomponents"] and t != (0, 0) and t == (int(s["x2"]) // 256, int(s["y2"]) // 256):
            per_tile[t] = per_tile.get(t, 0) + sum(c["rendered"] for c in s["components"])
    (tx, ty), _ = max(per_tile.items(), key=lambda kv: (kv[1], kv[0]))
    xmin, xmax, ymin, ymax = tx * 256, tx * 256 + 256, ty * 256, ty * 256 + 256
    args = ["--image=" + path] + COMMON + ["--xmin=%d" % xmin, "--xmax=%d" % xmax, "--ymin=%d" % ymin, "--ymax=%d" % ymax, "--bkg_cell=64"]
    docs = {}
    for name, extra in (("plain", PLAIN), ("scales", SCALES)):
        (d / ("serial_" + name)).mkdir()
        _run(args + extra, str(d / ("serial_" + name)))
        docs[name] = open(d / ("serial_" + name) / "out_sky.json", "rb").read()
    doc = json.loads(docs["scales"])
    assert set(doc) == {"image_id", "objs", "residual_scale_peaks"}
    assert b"scale" not in docs["plain"] and _plain_of(doc, "objs") == docs["plain"]
    crop = np.ascontiguousarray(img[ymin:ymax, xmin:xmax])
    stats = _check(doc, "objs", str(d / "serial_scales"), "out_sky", crop, beam, wcs, (xmin, ymin), 64)
    print("serial crop x %d.. y %d..: %d sources, scale peaks found %d kept %d strongest %d" % (
        xmin, ymin, len(doc["objs"]), stats["scales_found"], stats["scales_kept"], stats["scales_strongest"]))
    for p in doc["residual_scale_peaks"]:                     # the frame of the crop, which is the frame of its boxes
        assert 0 <= p["x_peak"] < 256 and 0 <= p["y_peak"] < 256 and abs(p["x"] - p["x_peak"]) <= 8 and abs(p["y"] - p["y_peak"]) <= 8
