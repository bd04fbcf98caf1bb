"""--peak_apertures end to end through scripts/run.py on the 1024 x 1024 synthetic FITS mosaic of tests/test_gpu_atrous_cli.py (two wide
faint blobs on empty sky added), tiled and serial, with --fit_blends --bkg_map --residual_map --residual_peaks --residual_scales 4.
  - with the ap_ keys stripped from the entries of the peak lists the catalog equals the catalog of the same run without the flag,
    byte for byte
  - a run without the flag is not touched by the other aperture options: its catalog is that of a run that names none of them
  - the lists equal those of a measure.Chain started on the catalog's boxes with peaks(), scale_peaks() and apertures() called after
    residual() (the kernels are deterministic and the host arithmetic is the same code, so equal means equal)
  - apertures_ms and its companions are in the stats only with the flag
  - the serial run measures in the frame of its crop."""
import json

import numpy as np
import pytest
import torch

from gpu_common import detector
from test_gpu_atrous_cli import mosaic  # noqa: F401  (the fixture)
from test_gpu_islands_cli import COMMON, _strip
from test_gpu_residual_cli import TILED, _run, _without

pytestmark = pytest.mark.gpu

J = 4
LISTS = ("residual_peaks", "residual_scale_peaks")
STAT_KEYS = ("apertures_ms", "aperture_kernel_ms", "apertures_jobs", "apertures_measured", "apertures_clipped")
SEARCH = ["--fit_blends", "--bkg_map", "--residual_map", "--residual_peaks", "--residual_scales=%d" % J]
OPTIONS = ["--aperture_unit=1.5", "--aperture_radii=1,2,3", "--aperture_annulus=5"]
APERTURES = SEARCH + ["--peak_apertures"] + OPTIONS


def _direct(sources, img, beam, wcs, origin, cell):
    """The steps from the components on, then the searches and apertures(), called directly on the catalog's boxes -> the chain."""
    from caesar_yolo_amd import measure
    det = detector("fp32", max_batch=1, max_imgsz=160)
    dev = det.mosaic_to_device(np.ascontiguousarray(img))
    torch.cuda.synchronize()
    want = _without(_strip(sources, measure.SOURCE_PEAK_KEYS + measure.SOURCE_SCALE_KEYS))
    config = {"bkg_map": True, "bkg_cell": cell, "residual_peaks": True, "residual_scales": J, "peak_apertures": True, "aperture_unit": 1.5,
              "aperture_radii": "1,2,3", "aperture_annulus": 5.0}
    chain = measure.Chain(det, dev, want, config, beam, wcs, wcs_origin=origin)
    chain.mesh, _ = measure.fill_mesh(det.measure_background(dev, cell=cell, k=3.0, niter=3), 64)
    for step in ("deblend", "fit", "blend", "residual", "peaks", "scale_peaks", "apertures"):
        getattr(chain, step)()
    return chain


def _plain_of(doc):
    from caesar_yolo_amd import measure
    out = dict(doc)
    for k in LISTS:
        out[k] = _strip(doc[k], measure.APERTURE_KEYS)
    return json.dumps(out, indent=2, sort_keys=True).encode()


def _check(doc, key, img, beam, wcs, origin, cell):
    from caesar_yolo_amd import measure
    chain = _direct(doc[key], img, beam, wcs, origin, cell)
    want = json.loads(json.dumps(measure.peak_lists(chain)))
    for k in LISTS:
        assert doc[k] == want[k], k
        for p in doc[k]:
            assert set(measure.APERTURE_KEYS) <= set(p) and p["ap_status"] in (0, 2)
            if p["ap_status"] == 0:
                step = p.get("step", 1)
                assert p["ap_radius"] == [1.5 * step, 3.0 * step, 4.5 * step] and len(p["ap_flux"]) == len(p["ap_snr"]) == 3
                assert p["ap_npix"] == sorted(p["ap_npix"]) and all(e >= 0 for e in p["ap_flux_err"])
                assert p["ap_best"] is None or p["ap_snr"][p["ap_best"]] == max(v for v in p["ap_snr"] if v is not None)
    assert sum(len(doc[k]) for k in LISTS) > 0
    return chain.aperture_stats


@pytest.fixture(scope="module")
def tiled(mosaic):  # noqa: F811
    d, path = mosaic[0], mosaic[1]
    dirs = {}
    for name, extra in (("search", SEARCH), ("options", SEARCH + OPTIONS), ("apertures", APERTURES)):
        (d / ("ap_" + name)).mkdir()
        _run(["--image=" + path] + TILED + extra, str(d / ("ap_" + name)))
        dirs[name] = d / ("ap_" + name)
    return dirs


def test_tiled(mosaic, tiled):  # noqa: F811
    d, path, img, beam, wcs, blobs = mosaic
    raw = {k: open(tiled[k] / "catalog_sky.json", "rb").read() for k in tiled}
    assert raw["options"] == raw["search"] and b"ap_" not in raw["search"]      # without the flag: the catalog it was
    doc = json.load(open(tiled["apertures"] / "catalog_sky.json"))
    assert set(doc) == {"sources"} | set(LISTS) and _plain_of(doc) == raw["search"]
    stats = _check(doc, "sources", img, beam, wcs, (0, 0), 128)
    seen = [json.load(open(tiled[k] / "stats.json")) for k in ("search", "apertures")]
    assert not set(seen[0]) & set(STAT_KEYS) and set(seen[0]) | set(STAT_KEYS) == set(seen[1]) and all(seen[1][k] >= 0 for k in STAT_KEYS)
    n = sum(len(doc[k]) for k in LISTS)
    assert (seen[1]["apertures_jobs"], seen[1]["apertures_measured"], seen[1]["apertures_clipped"]) == (
        n, stats["apertures_measured"], stats["apertures_clipped"]) and stats["apertures_jobs"] == n
    print("tiled: %d entries measured of %d, %d clipped, aperture_kernel_ms %.3f, apertures_ms %.1f" % (
        seen[1]["apertures_measured"], n, seen[1]["apertures_clipped"], seen[1]["aperture_kernel_ms"], seen[1]["apertures_ms"]))


def test_serial_crop(mosaic, tiled):  # noqa: F811
    d, path, img, beam, wcs, blobs = mosaic
    cx, cy = blobs[0]                                         # a crop around the first blob, so that the scale list is not empty
    xmin, ymin = int(min(max(cx - 128, 0), img.shape[1] - 256)), int(min(max(cy - 128, 0), img.shape[0] - 256))
    xmax, ymax = xmin + 256, ymin + 256
    args = ["--image=" + path] + COMMON + ["--xmin=%d" % xmin, "--xmax=%d" % xmax, "--ymin=%d" % ymin, "--ymax=%d" % ymax, "--bkg_cell=64"]
    docs = {}
    for name, extra in (("search", SEARCH), ("apertures", APERTURES)):
        (d / ("ap_serial_" + name)).mkdir()
        _run(args + extra, str(d / ("ap_serial_" + name)))
        docs[name] = open(d / ("ap_serial_" + name) / "out_sky.json", "rb").read()
    doc = json.loads(docs["apertures"])
    assert set(doc) == {"image_id", "objs"} | set(LISTS)
    assert b"ap_" not in docs["search"] and _plain_of(doc) == docs["search"]
    crop = np.ascontiguousarray(img[ymin:ymax, xmin:xmax])
    stats = _check(doc, "objs", crop, beam, wcs, (xmin, ymin), 64)
    print("serial crop x %d.. y %d..: %d jobs, %d measured, %d clipped" % (xmin, ymin, stats["apertures_jobs"], stats["apertures_measured"], stats["apertures_clipped"]))
    for k in LISTS:                                           # the frame of the crop: every window inside it
        for p in doc[k]:
            assert 0 <= p["x"] < 256 and 0 <= p["y"] < 256
