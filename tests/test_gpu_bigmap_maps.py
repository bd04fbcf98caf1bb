"""The entries that walk the whole map, on the 46341 x 46339 map of tests/bigmap_cases.py: cy_measure_background (the LDS form and
the re-reading form), cy_expand_background, cy_render_gaussians, cy_find_peaks (both signs), cy_atrous_step (step 1 and 64) and
cy_mosaic_prepare.

Only the crops around the patches are copied back.  Each is compared with the entry's reference on the crop (bigmap_cases: it
equals the reference on the full image, shown on a stand-in by tests/test_bigmap_cases_cpu.py) under the entry's existing rule.
Everything outside the crops has to be exactly what a blank input gives (0; for cy_mosaic_prepare: unchanged), counted on the
device over every pixel that is not in a crop: that is what catches a store at a wrapped address.

At most three maps of the shape are live at a time.  No skip path: when the maps cannot be allocated the tests error."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import bigmap_cases as B
import residual_ref as RR
import test_gpu_atrous
import test_gpu_background
import test_gpu_peaks
from caesar_yolo_amd import measure
from gpu_common import detector

pytestmark = pytest.mark.gpu
BAND = 4096                       # rows per count: bounds what a count over a column range may allocate


@pytest.fixture(scope="module")
def scene():
    det = detector("fp32", max_batch=1, max_imgsz=160)
    maps = {"img": B.device(det.tdev)}
    yield det, maps
    maps.clear()
    torch.cuda.empty_cache()


def nonzero_outside(t, crop_table):
    """The number of non-zero (or NaN) values of the device map t outside the crops, over every such pixel."""
    total, seen = 0, 0
    for a, b, cols in B.outside_ranges(crop_table):
        for y in range(a, b, BAND):
            y1 = min(b, y + BAND)
            for x0, x1 in cols:
                total += int(torch.count_nonzero(t[y:y1, x0:x1]))
                seen += (y1 - y) * (x1 - x0)
    assert seen + sum((c[1] - c[0]) * (c[3] - c[2]) for c in crop_table.values()) == B.MH * B.MW
    return total


def back(t, c):
    return t[c[0]:c[1], c[2]:c[3]].cpu().numpy()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


@pytest.mark.parametrize("cell", [128, 300])
def test_measure_background(scene, cell):
    det, maps = scene
    assert 128 * 128 <= 16384 < 300 * 300                       # BKG_LDS_MAX: cell 128 is the LDS form, cell 300 re-reads its cell
    table = B.crops(0, cell)
    got, wall = timed(lambda: det.measure_background(maps["img"], cell=cell, k=3.0, niter=3))
    assert got.shape == (-(-B.MH // cell), -(-B.MW // cell), 8)
    inside = np.zeros(got.shape[:2], bool)
    for nm, c in table.items():
        ref, (cy0, cx0) = B.background_on_crop(B.host(), c, cell, 3.0, 3)
        assert (ref[:, :, 0] > 0).any(), nm
        sub = np.ascontiguousarray(got[cy0:cy0 + ref.shape[0], cx0:cx0 + ref.shape[1]])
        test_gpu_background.assert_rows_equal(sub, ref, "%s, cell %d" % (nm, cell))
        inside[cy0:cy0 + ref.shape[0], cx0:cx0 + ref.shape[1]] = True
    assert (got[~inside][:, 0] == 0).all(), "a cell outside the crops holds valid pixels"
    blank = np.array([0, 0, 0, 0, -np.inf, np.inf, 0, 0], np.float64)
    assert np.array_equal(got[~inside], np.broadcast_to(blank, got[~inside].shape))
    print("measure_background, cell %d: %d cells in the crops equal, %d blank; kernel %.3f ms, wall %.1f ms" % (
        cell, int(inside.sum()), int((~inside).sum()), det.background_kernel_ms(), wall))


@pytest.mark.parametrize("plane", ["bkg", "rms"])
def test_expand_background(scene, plane):
    det, maps = scene
    cell = 128
    ncy, ncx = -(-B.MH // cell), -(-B.MW // cell)
    rng = np.random.default_rng(5)
    mesh = np.stack([rng.normal(1e-4, 1e-5, (ncy, ncx)), rng.uniform(1e-4, 2e-4, (ncy, ncx))], 2)
    out, wall = timed(lambda: det.expand_background(mesh, cell, (B.MH, B.MW), want=(plane,)))
    t = out[("bkg", "rms").index(plane)]
    assert out[1 - ("bkg", "rms").index(plane)] is None and t.shape == (B.MH, B.MW)
    k = ("bkg", "rms").index(plane)

    def expect(x, y):
        with np.errstate(over="ignore"):
            return np.ascontiguousarray(measure.sample_mesh(mesh, cell, np.asarray(x, np.float64), np.asarray(y, np.float64))[..., k].astype(np.float32))

    def same(g, w, what):
        bad = g.view(np.uint32) != w.view(np.uint32)
        assert not bad.any(), "%s %s: %d pixels differ, first at %s: %r on the GPU, %r expected" % (plane, what, int(bad.sum()), np.argwhere(bad)[0], g[bad][0], w[bad][0])

    xs = np.arange(B.MW)
    for y in (0, B.rc(1 << 29)[0], B.rc(1 << 30)[0], B.MH - 1):
        same(t[y].cpu().numpy(), expect(xs, np.full(B.MW, y)), "row %d" % y)
    ys = np.arange(B.MH)
    for x in (B.MW - 2, B.MW - 1):
        same(t[:, x].cpu().numpy(), expect(np.full(B.MH, x), ys), "column %d" % x)
    idx = np.sort(np.random.default_rng(6).integers(0, B.MH * B.MW, 100000))
    idx[-1] = B.MH * B.MW - 1
    g = t.view(-1)[torch.from_numpy(idx).to(t.device)].cpu().numpy()
    same(g, expect(idx % B.MW, idx // B.MW), "sample")
    assert len(np.unique(g)) > 1000
    print("expand_background, %s: 4 rows, 2 columns and 100000 sampled pixels equal; wall %.1f ms" % (plane, wall))


@pytest.mark.parametrize("want", ["model", "resid"])
def test_render_gaussians(scene, want):
    det, maps = scene
    comp = B.render_components()
    table = B.crops(B.HALO_RENDER)
    (rows, model, resid), wall = timed(lambda: det.render_gaussians(maps["img"], comp, B.NSIGMA, None, (want,)))
    t = model if want == "model" else resid
    assert (model is None) != (resid is None)
    worst = 0.0
    for nm, c in table.items():
        r_rows, r_model, r_resid = B.render_on_crop(B.host(), comp, c, (B.MH, B.MW))
        assert np.array_equal(rows, r_rows), nm
        g = back(t, c).astype(np.float64)
        x, bound = (r_model, RR.model_bound(r_model)) if want == "model" else (r_resid, RR.resid_bound(r_resid, r_model))
        d = np.abs(g - x)
        assert (d <= bound).all(), "%s: %s off by %g of its bound at %s" % (nm, want, (d / bound).max(), np.unravel_index(np.argmax(d / bound), d.shape))
        assert np.abs(x).max() > 1.0
        worst = max(worst, float((d / bound).max()))
    assert (rows[:, 0] == 0).all() and nonzero_outside(t, table) == 0
    print("render_gaussians, %s: %d components, largest difference %.3f of the bound, 0 outside the crops; kernel %.3f ms, wall %.1f ms" % (
        want, len(comp), worst, det.render_kernel_ms(), wall))


@pytest.mark.parametrize("sign", [1, -1])
def test_find_peaks(scene, sign):
    det, maps = scene
    if "rms" not in maps:
        maps["rms"] = B.device(det.tdev, B.rms_patch)
    table = B.crops(B.HALO_PEAKS)
    want, absum = B.merged_peaks(B.host(), B.host_rms(), table, 5.0, sign)
    per_patch = {nm: len(B.peaks_on_crop(B.host(), B.host_rms(), c, 5.0, sign)[0]) for nm, c in table.items()}
    assert min(per_patch.values()) >= 1, per_patch
    (rows, total), wall = timed(lambda: det.find_peaks(maps["img"], maps["rms"], 5.0, B.RADIUS_PEAKS, sign))
    worst = test_gpu_peaks.check_rows("big map, sign %d" % sign, rows, total, want, absum)
    print("find_peaks, sign %d: %d peaks, largest difference of a sum %.3f of its bound; kernel %.3f ms, wall %.1f ms" % (
        sign, total, worst, det.peaks_kernel_ms(), wall))
    if sign == -1:
        del maps["rms"]
        torch.cuda.empty_cache()


@pytest.mark.parametrize("step", [1, 64])
def test_atrous_step(scene, step):
    det, maps = scene
    table = B.crops(B.halo_atrous(step))
    for name in ("smooth", "detail"):                            # one output map at a time
        (smooth, detail), wall = timed(lambda: det.atrous_step(maps["img"], step, want=(name,)))
        t = smooth if name == "smooth" else detail
        for nm, c in table.items():
            ref = B.atrous_on_crop(B.host(), c, step)[0 if name == "smooth" else 1]
            test_gpu_atrous.assert_bits("%s, step %d" % (nm, step), name, back(t, c), ref)
        assert nonzero_outside(t, table) == 0
        print("atrous_step %d, %s: the crops equal bit for bit, 0 outside; kernel %.3f ms, wall %.1f ms" % (step, name, det.atrous_kernel_ms(), wall))
        del smooth, detail, t
        torch.cuda.empty_cache()


def test_mosaic_prepare(scene):
    """A map of its own: every patch as big-endian words with NaN and +-inf put in; after the call the patches hold the pixels with
    the non-finite ones blank, and everything else is still 0."""
    det, maps = scene

    def raw(nm):
        px = B.patch(nm)[0].copy()
        px[3, 5], px[64, 64], px[127, 127], px[126, 0] = np.nan, np.inf, -np.inf, np.nan
        return px.astype(">f4").view("<f4")                      # the bytes of the big-endian file, as the upload carries them

    def expected(nm):
        px = B.patch(nm)[0].copy()
        px[3, 5] = px[64, 64] = px[127, 127] = px[126, 0] = 0.0
        return px
    t = B.device(det.tdev, raw)
    _, wall = timed(lambda: det._chk(det.lib.cy_mosaic_prepare(det.ctx, det._p(t), t.numel(), 1, det._stream())))
    for nm, (y0, x0) in B.PLACES.items():
        first = B.top(nm)
        got = t[y0 + first:y0 + B.P, x0:x0 + B.P].cpu().numpy()
        assert np.array_equal(got.view(np.uint32), expected(nm)[first:].view(np.uint32)), nm
    assert nonzero_outside(t, B.crops(0)) == 0
    print("mosaic_prepare: the patches are what the host conversion gives, 0 outside; wall %.1f ms" % wall)
