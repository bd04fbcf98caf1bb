"""--fit_peak_groups end to end through scripts/run.py on the 1024 x 1024 synthetic FITS mosaic of tests/test_gpu_atrous_cli.py, tiled
and serial, with --fit_blends --bkg_map --residual_map --residual_peaks --residual_scales 4 --peak_apertures --fit_peaks.
  - with the gblend_ keys stripped from the entries of the peak lists the catalog equals the catalog of the same run without the
    flag, byte for byte
  - a run without the flag is not touched by --fit_peaks_link: its catalog is that of a run that does not name it
  - the flag alone implies --fit_peaks: the same catalog as with both
  - the lists equal those of a measure.Chain started on the catalog's boxes with peaks(), scale_peaks(), apertures(), peak_fits() and
    peak_groups() called after residual() (the kernels are deterministic and the host arithmetic is the same code, so equal means
    equal)
  - peakgroup_ms and its companions are in the stats only with the flag
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
STAT_KEYS = ("peakgroup_ms", "peakgroup_kernel_ms", "peakgroup_jobs", "peakgroup_members", "peakgroup_converged", "peakgroup_niter_mean",
             "peakgroup_niter_max", "peakgroup_over_limit")
SEARCH = ["--fit_blends", "--bkg_map", "--residual_map", "--residual_peaks", "--residual_scales=%d" % J, "--peak_apertures"]
FITS = SEARCH + ["--fit_peaks"]
LINK = 1.75
GROUPS = SEARCH + ["--fit_peak_groups", "--fit_peaks_link=%g" % LINK]       # --fit_peaks comes with it


def _direct(sources, img, beam, wcs, origin, cell):
    """The steps from the components on, then the searches, apertures(), peak_fits() and peak_groups(), called directly on the
    catalog's boxes."""
    from caesar_yolo_amd import measure
    det = detector("fp32", max_batch=1, max_imgsz=160)
    dev = det.mosaic_to_device(np.ascontiguousarray(img))
    torch.cuda.synchronize()
    want = _without(_strip(sources, measure.SOURCE_PEAK_KEYS + measure.SOURCE_SCALE_KEYS))
    config = {"bkg_map": True, "bkg_cell": cell, "residual_peaks": True, "residual_scales": J, "peak_apertures": True, "fit_peak_groups": True,
              "fit_peaks_link": LINK}
    chain = measure.Chain(det, dev, want, config, beam, wcs, wcs_origin=origin)
    chain.mesh, _ = measure.fill_mesh(det.measure_background(dev, cell=cell, k=3.0, niter=3), 64)
    for step in ("deblend", "fit", "blend", "residual", "peaks", "scale_peaks", "apertures", "peak_fits", "peak_groups"):
        getattr(chain, step)()
    return chain


def _plain_of(doc):
    from caesar_yolo_amd import measure
    out = dict(doc)
    for k in LISTS:
        out[k] = _strip(doc[k], measure.GBLEND_KEYS)
    return json.dumps(out, indent=2, sort_keys=True).encode()


def _check(doc, key, img, beam, wcs, origin, cell):
    from caesar_yolo_amd import measure
    chain = _direct(doc[key], img, beam, wcs, origin, cell)
    want = json.loads(json.dumps(measure.peak_lists(chain)))
    njob = nmember = 0
    for k in LISTS:
        assert doc[k] == want[k], k
        for i, p in enumerate(doc[k]):
            assert set(measure.GBLEND_KEYS) <= set(p) and set(measure.GFIT_KEYS) <= set(p)
            if not p.get("strongest", True):
                assert all(p[g] is None for g in measure.GBLEND_KEYS)
                continue
            st = p["gblend_status"]
            assert st in (0, 2, 3, 4, 6, 7) and p["gblend_niter"] <= 64
            first = doc[k][p["gblend_group"]]
            assert first["gblend_slot"] == 0 and first["gblend_size"] == p["gblend_size"] and first["gblend_status"] == st and p["gblend_group"] <= i
            if st == 6:
                assert p["gblend_group"] == i and p["gblend_size"] == 1 and all(p["gblend_" + g[5:]] == p[g] for g in measure.GFIT_KEYS[9:])
            if st in (0, 2, 3, 4):
                assert 2 <= p["gblend_size"] <= 4 and p["gblend_npix"] == first["gblend_npix"]
                njob, nmember = njob + (p["gblend_slot"] == 0), nmember + 1
            if st in (0, 2):
                assert p["gblend_peak"] > 0 and p["gblend_major"] >= p["gblend_minor"] > 0 and p["gblend_npix"] >= 6 * p["gblend_size"] + 1
            if st in (3, 4, 7):
                assert p["gblend_peak"] is None and p["gblend_size"] >= 2
    assert njob > 0 and (chain.peakgroup_stats["peakgroup_jobs"], chain.peakgroup_stats["peakgroup_members"]) == (njob, nmember)
    return chain.peakgroup_stats


@pytest.fixture(scope="module")
def tiled(mosaic):  # noqa: F811
    d, path = mosaic[0], mosaic[1]
    dirs = {}
    for name, extra in (("fits", FITS), ("link", FITS + ["--fit_peaks_link=0.5"]), ("groups", GROUPS)):
        (d / ("pg_" + name)).mkdir()
        _run(["--image=" + path] + TILED + extra, str(d / ("pg_" + name)))
        dirs[name] = d / ("pg_" + name)
    return dirs


def test_tiled(mosaic, tiled):  # noqa: F811
    d, path, img, beam, wcs, blobs = mosaic
    raw = {k: open(tiled[k] / "catalog_sky.json", "rb").read() for k in tiled}
    assert raw["link"] == raw["fits"] and b"gblend_" not in raw["fits"] and b"gfit_" in raw["fits"]      # without the flag: the catalog it was
    doc = json.load(open(tiled["groups"] / "catalog_sky.json"))
    assert set(doc) == {"sources"} | set(LISTS) and _plain_of(doc) == raw["fits"]
    stats = _check(doc, "sources", img, beam, wcs, (0, 0), 128)
    seen = [json.load(open(tiled[k] / "stats.json")) for k in ("fits", "groups")]
    assert not set(seen[0]) & set(STAT_KEYS) and set(seen[0]) | set(STAT_KEYS) == set(seen[1]) and all(seen[1][k] >= 0 for k in STAT_KEYS)
    for k in STAT_KEYS[2:]:
        assert seen[1][k] == stats[k], k
    print("tiled: %d group jobs of %d members, %d converged, niter mean %.1f max %d, %d groups above the limit, peakgroup_kernel_ms %.3f, peakgroup_ms %.1f" % (
        seen[1]["peakgroup_jobs"], seen[1]["peakgroup_members"], seen[1]["peakgroup_converged"], seen[1]["peakgroup_niter_mean"], seen[1]["peakgroup_niter_max"],
        seen[1]["peakgroup_over_limit"], seen[1]["peakgroup_kernel_ms"], seen[1]["peakgroup_ms"]))


def test_serial_crop(mosaic, tiled):  # noqa: F811
    d, path, img, beam, wcs, blobs = mosaic
    cx, cy = blobs[0]                                         # a crop around the first blob, so that the scale list is not empty
    xmin, ymin = int(min(max(cx - 128, 0), img.shape[1] - 256)), int(min(max(cy - 128, 0), img.shape[0] - 256))
    xmax, ymax = xmin + 256, ymin + 256
    args = ["--image=" + path] + COMMON + ["--xmin=%d" % xmin, "--xmax=%d" % xmax, "--ymin=%d" % ymin, "--ymax=%d" % ymax, "--bkg_cell=64"]
    docs = {}
    for name, extra in (("fits", FITS), ("groups", GROUPS)):
        (d / ("pg_serial_" + name)).mkdir()
        _run(args + extra, str(d / ("pg_serial_" + name)))
        docs[name] = open(d / ("pg_serial_" + name) / "out_sky.json", "rb").read()
    doc = json.loads(docs["groups"])
    assert set(doc) == {"image_id", "objs"} | set(LISTS)
    assert b"gblend_" not in docs["fits"] and _plain_of(doc) == docs["fits"]
    crop = np.ascontiguousarray(img[ymin:ymax, xmin:xmax])
    stats = _check(doc, "objs", crop, beam, wcs, (xmin, ymin), 64)
    print("serial crop x %d.. y %d..: %d group jobs, %d converged" % (xmin, ymin, stats["peakgroup_jobs"], stats["peakgroup_converged"]))
    for k in LISTS:                                           # the frame of the crop
        for p in doc[k]:
            if p["gblend_status"] in (0, 2):
                assert -16 * p.get("step", 1) <= p["gblend_x"] < 256 + 16 * p.get("step", 1)
