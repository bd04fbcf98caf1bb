"""The job-type measurement entries on the 46341 x 46339 map of tests/bigmap_cases.py: jobs on patches that hold pixel 2^29, 2^30,
3 * 2^29 and the last pixel of a map just below 2^31 pixels, and on the decoys 2^30 pixels before them that a wrapped byte offset
would read instead.

Every entry gets the jobs of all patches and decoys in one call.  The reference is the entry's existing tests/*_ref.py on the host
twin, and the comparison is the entry's existing rule, imported from its GPU test (or from residual_ref for the residual
statistics): no tolerance is new here.  The boxes, discs and apertures named `corner` leave the image at its far corner on the
`end` patch.  tests/test_bigmap_cases_cpu.py shows that a result read from a decoy would not pass.

No skip path: when the maps cannot be allocated the tests error."""
import numpy as np
import pytest
import torch

import bigmap_cases as B
import residual_ref
import test_gpu_aperture
import test_gpu_blend
import test_gpu_deblend
import test_gpu_fit
import test_gpu_islands
import test_gpu_measure
import test_gpu_peakfit
import test_gpu_peakgroup
from gpu_common import detector

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene():
    det = detector("fp32", max_batch=1, max_imgsz=160)
    maps = {"img": B.device(det.tdev)}
    yield det, maps
    maps.clear()
    torch.cuda.empty_cache()


def second_map(det, maps, key, of):
    """A second map of the shape, built on first use and freed with the module's."""
    if key not in maps:
        maps[key] = B.device(det.tdev, of)
    return maps[key]


def test_the_device_twin_holds_the_patches(scene):
    det, maps = scene
    dev = maps["img"]
    assert dev.shape == (B.MH, B.MW) and dev.numel() < 1 << 31
    for nm, (y0, x0) in B.PLACES.items():
        t = B.top(nm)
        assert np.array_equal(dev[y0 + t:y0 + B.P, x0:x0 + B.P].cpu().numpy(), B.patch(nm)[0][t:]), nm
    for nm, index in B.THRESHOLD_PIXEL.items():
        y, x = B.rc(index)
        assert float(dev.view(-1)[index]) == float(B.host()[y, x]) != 0.0, nm
    assert int(torch.count_nonzero(dev)) == sum(int(np.count_nonzero(B.patch(nm)[0][B.top(nm):])) for nm in B.PLACES)


@pytest.mark.parametrize("ring", [0, 8])
def test_measure_sources(scene, ring):
    det, maps = scene
    ref, mags = B.measure_reference(ring)
    got = det.measure_sources(maps["img"], B.all_boxes(), ring=ring)
    test_gpu_measure.compare(got, ref, mags, "big map, ring %d" % ring)
    print("measure_sources, ring %d: %d boxes; kernel %.3f ms" % (ring, len(ref), det.measure_kernel_ms()))


def test_measure_islands(scene):
    det, maps = scene
    ref, rmasks, mags = B.island_reference()
    got, gmasks = det.measure_islands(maps["img"], B.all_boxes(), B.thresholds()[:, :3], conn=8, return_masks=True)
    worst = test_gpu_islands.compare(got, gmasks, ref, rmasks, mags, "big map")
    print("measure_islands: %d boxes, largest |diff| / bound %.3g; kernel %.3f ms" % (len(ref), worst, det.islands_kernel_ms()))


def test_deblend_islands(scene):
    det, maps = scene
    ref, rcomp, rmasks, mags = B.deblend_reference()
    got, gcomp, gmasks = det.deblend_islands(maps["img"], B.all_boxes(), B.thresholds(), conn=8, radius=2, return_masks=True)
    worst = test_gpu_deblend.compare(got, gcomp, gmasks, ref, rcomp, rmasks, mags, "big map")
    print("deblend_islands: %d boxes, largest |diff| / bound %.3g; kernel %.3f ms" % (len(ref), worst, det.deblend_kernel_ms()))


def test_fit_components(scene):
    det, maps = scene
    bkg, ncomp, start, masks = B.fit_inputs()
    ref = B.fit_reference()[0]
    got = det.fit_components(maps["img"], B.all_boxes(), bkg, ncomp, start, masks)
    njobs, n0, worst = test_gpu_fit.compare(got, ref, ncomp, start, 64, "big map")
    assert njobs == int(ncomp.sum()) and n0 == njobs                   # none left out, all converged (the CPU test says so of the reference)
    print("fit_components: %d jobs, worst parameter difference %.3g TOL; kernel %.3f ms" % (njobs, worst, det.fit_kernel_ms()))


def test_fit_blends(scene):
    det, maps = scene
    bkg, ncomp, start, masks = B.blend_inputs()
    ref = B.blend_reference()[0][0]
    got = det.fit_blends(maps["img"], B.all_boxes(), bkg, ncomp, start, masks)
    nrows, n0, worst, worst_c = test_gpu_blend.compare(got, ref, ncomp, start, 64, "big map")
    assert nrows == int(ncomp.sum()) and n0 >= 2 * len(B.PLACES)
    print("fit_blends: %d rows, %d with status 0, worst %.3g TOL, C %.3g TOL_C; kernel %.3f ms" % (nrows, n0, worst, worst_c, det.blend_kernel_ms()))


def test_measure_residuals(scene):
    det, maps = scene
    model = second_map(det, maps, "model", lambda nm: B.patch(nm)[1])
    ref, ab = B.residual_reference()
    got = det.measure_residuals(maps["img"], model, B.all_boxes(), B.thresholds()[:, 2], B.island_reference()[1])
    residual_ref.compare_stats(got, ref, ab, B.job_names(B.BOX_NAMES))
    print("measure_residuals: %d boxes; kernel %.3f ms" % (len(ref), det.residual_kernel_ms()))
    del model, maps["model"]
    torch.cuda.empty_cache()


@pytest.mark.parametrize("with_rms", [True, False], ids=["rms", "no_rms"])
def test_aperture_sums(scene, with_rms):
    det, maps = scene
    rms = second_map(det, maps, "rms", B.rms_patch) if with_rms else None
    got = det.aperture_sums(maps["img"], rms, B.all_aperture_jobs(), B.FACTORS)
    test_gpu_aperture.assert_rows("big map", got, B.aperture_reference(with_rms))
    print("aperture_sums (%s): %d jobs; kernel %.3f ms" % ("rms" if with_rms else "no rms", len(got), det.aperture_kernel_ms()))
    if with_rms:
        del rms, maps["rms"]
        torch.cuda.empty_cache()


def test_fit_peaks(scene):
    det, maps = scene
    jobs, res = B.all_peak_jobs(), B.peakfit_reference()
    got = det.fit_peaks(maps["img"], jobs)
    n0, worst = test_gpu_peakfit.compare("big map", B.job_names(B.PEAK_NAMES), jobs, got, res, 64)
    assert n0 == len(jobs)
    print("fit_peaks: %d jobs, worst parameter difference %.3g TOL; kernel %.3f ms" % (n0, worst, det.peakfit_kernel_ms()))


def test_fit_peak_groups(scene):
    det, maps = scene
    jobs, (res, _) = B.group_jobs(), B.peakgroup_reference()
    got = det.fit_peak_groups(maps["img"], jobs, link=B.LINK)
    n0, worst, worst_c = test_gpu_peakgroup.compare("big map", B.job_names(B.PEAK_NAMES), jobs, got, res, 64)
    assert n0 == 4 * len(B.PLACES)                                     # the two linked pairs of every patch
    print("fit_peak_groups: %d rows in groups, worst %.3g TOL, C %.3g TOL_C; kernel %.3f ms" % (n0, worst, worst_c, det.peakgroup_kernel_ms()))
