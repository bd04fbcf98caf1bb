"""--fit_peaks end to end through scripts/run.py on the 1024 x 1024 synthetic FITS mosaic of tests/test_gpu_atrous_cli.py (two wide
faint blobs on empty sky added), tiled and serial, with --fit_blends --bkg_map --residual_map --residual_peaks --residual_scales 4
--peak_apertures.
  - with the gfit_ keys stripped from the entries of the peak lists the catalog equals the catalog of the same run without the flag,
    byte for byte
  - a run without the flag is not touched by the other peak-fit options: its catalog is that of a run that names none of them
  - the lists equal those of a measure.Chain started on the catalog's boxes with peaks(), scale_peaks(), apertures() and peak_fits()
    called after residual() (the kernels are deterministic and the host arithmetic is the same code, so equal means equal)
  - peakfit_ms and its companions are in the stats only with the flag
  - the serial run fits in the frame of its crop."""
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
STAT_KEYS = ("peakfit_ms", "peakfit_kernel_ms", "peakfit_jobs", "peakfit_converged", "peakfit_niter_mean", "peakfit_niter_max", "peakfit_crowded")
SEARCH = ["--fit_blends", "--bkg_map", "--residual_map", "--residual_peaks", "--residual_scales=%d" % J, "--peak_apertures"]
OPTIONS = ["--fit_peaks_radius=5", "--fit_peaks_sigma=2", "--fit_peaks_max_iter=40"]
FITS = SEARCH + ["--fit_peaks"] + OPTIONS


def _direct(sources, img, beam, wcs, origin, cell):
    """The steps from the components on, then the searches, apertures() and peak_fits(), called directly on the catalog's boxes."""
    from caesar_yolo_amd import measure
    det = detector("fp32", max_batch=1, max_imgsz=160)
    dev = det.mosaic_to_device(np.ascontiguousarray(img))
    torch.cuda.synchronize()
    want = _without(_strip(sources, measure.SOURCE_PEAK_KEYS + measure.SOURCE_SCALE_KEYS))
    config = {"bkg_map": True, "bkg_cell": cell, "residual_peaks": True, "residual_scales": J, "peak_apertures": True, "fit_peaks": True,
              "fit_peaks_radius": 5.0, "fit_peaks_sigma": 2.0, "fit_peaks_max_iter": 40}
    chain = measure.Chain(det, dev, want, config, beam, wcs, wcs_origin=origin)
    chain.mesh, _ = measure.fill_mesh(det.measure_background(dev, cell=cell, k=3.0, niter=3), 64)
    for step in ("deblend", "fit", "blend", "residual", "peaks", "scale_peaks", "apertures", "peak_fits"):
        getattr(chain, step)()
    return chain


def _plain_of(doc):
    from caesar_yolo_amd import measure
    out = dict(doc)
    for k in LISTS:
        out[k] = _strip(doc[k], measure.GFIT_KEYS)
    return json.dumps(out, indent=2, sort_keys=True).encode()


def _check(doc, key, img, beam, wcs, origin, cell):
    from caesar_yolo_amd import measure
    chain = _direct(doc[key], img, beam, wcs, origin, cell)
    want = json.loads(json.dumps(measure.peak_lists(chain)))
    nfit = 0
    for k in LISTS:
        assert doc[k] == want[k], k
        for p in doc[k]:
            assert set(measure.GFIT_KEYS) <= set(p)
            if not p.get("strongest", True):
                assert all(p[g] is None for g in measure.GFIT_KEYS)
                continue
            nfit += 1
            assert p["gfit_status"] in (0, 2, 3, 4) and p["gfit_radius"] == 5.0 * p.get("step", 1) and p["gfit_bkg"] == p["ap_bkg"] and p["gfit_niter"] <= 40
            if p["gfit_status"] in (0, 2):
                assert p["gfit_peak"] > 0 and p["gfit_major"] >= p["gfit_minor"] > 0 and p["gfit_npix"] >= 7
    assert nfit > 0 and chain.peakfit_stats["peakfit_jobs"] == nfit
    return chain.peakfit_stats


@pytest.fixture(scope="module")
def tiled(mosaic):  # noqa: F811
    d, path = mosaic[0], mosaic[1]
    dirs = {}
    for name, extra in (("search", SEARCH), ("options", SEARCH + OPTIONS), ("fits", FITS)):
        (d / ("pf_" + name)).mkdir()
        _run(["--image=" + path] + TILED + extra, str(d / ("pf_" + name)))
        dirs[name] = d / ("pf_" + name)
    return dirs


def test_tiled(mosaic, tiled):  # noqa: F811
    d, path, img, beam, wcs, blobs = mosaic
    raw = {k: open(tiled[k] / "catalog_sky.json", "rb").read() for k in tiled}
    assert raw["options"] == raw["search"] and b"gfit_" not in raw["search"]      # without the flag: the catalog it was
    doc = json.load(open(tiled["fits"] / "catalog_sky.json"))
    assert set(doc) == {"sources"} | set(LISTS) and _plain_of(doc) == raw["search"]
    stats = _check(doc, "sources", img, beam, wcs, (0, 0), 128)
    seen = [json.load(open(tiled[k] / "stats.json")) for k in ("search", "fits")]
    assert not set(seen[0]) & set(STAT_KEYS) and set(seen[0]) | set(STAT_KEYS) == set(seen[1]) and all(seen[1][k] >= 0 for k in STAT_KEYS)
    for k in ("peakfit_jobs", "peakfit_converged", "peakfit_niter_mean", "peakfit_niter_max", "peakfit_crowded"):
        assert seen[1][k] == stats[k], k
    print("tiled: %d jobs, %d converged, niter mean %.1f max %d, %d crowded, peakfit_kernel_ms %.3f, peakfit_ms %.1f" % (
        seen[1]["peakfit_jobs"], seen[1]["peakfit_converged"], seen[1]["peakfit_niter_mean"], seen[1]["peakfit_niter_max"], seen[1]["peakfit_crowded"],
        seen[1]["peakfit_kernel_ms"], seen[1]["peakfit_ms"]))


def test_serial_crop(mosaic, tiled):  # noqa: F811
    d, path, img, beam, wcs, blobs = mosaic
    cx, cy = blobs[0]                                         # a crop around the first blob, so that the scale list is not empty
    xmin, ymin = int(min(max(cx - 128, 0), img.shape[1] - 256)), int(min(max(cy - 128, 0), img.shape[0] - 256))
    xmax, ymax = xmin + 256, ymin + 256
    args = ["--image=" + path] + COMMON + ["--xmin=%d" % xmin, "--xmax=%d" % xmax, "--ymin=%d" % ymin, "--ymax=%d" % ymax, "--bkg_cell=64"]
    docs = {}
    for name, extra in (("search", SEARCH), ("fits", FITS)):
        (d / ("pf_serial_" + name)).mkdir()
        _run(args + extra, str(d / ("pf_serial_" + name)))
        docs[name] = open(d / ("pf_serial_" + name) / "out_sky.json", "rb").read()
    doc = json.loads(docs["fits"])
    assert set(doc) == {"image_id", "objs"} | set(LISTS)
    assert b"gfit_" not in docs["search"] and _plain_of(doc) == docs["search"]
    crop = np.ascontiguousarray(img[ymin:ymax, xmin:xmax])
    stats = _check(doc, "objs", crop, beam, wcs, (xmin, ymin), 64)
    print("serial crop x %d.. y %d..: %d jobs, %d converged" % (xmin, ymin, stats["peakfit_jobs"], stats["peakfit_converged"]))
    for k in LISTS:                                           # the frame of the crop
        for p in doc[k]:
            if p["gfit_status"] in (0, 2):
                assert -16 * p.get("step", 1) <= p["gfit_x"] < 256 + 16 * p.get("step", 1)
