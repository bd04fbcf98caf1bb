"""cy_render_gaussians and cy_measure_residuals on the GPU against their numpy float64 restatement (tests/residual_ref.py) on the
inputs of tests/residual_cases.py.

Render: the status / rectangle rows are host float64 and integers: equal.  Both maps are compared on EVERY pixel, none skipped, with
x the reference's float64 value and TOL_M = residual_ref.TOL_M (measured on the CPU between the reference's own exp variants, times
16; tests/test_residual_cpu.py recomputes it):
    |model_gpu - x| <= 2^-24 |x| (1 + TOL_M) + TOL_M |x| + 2^-149
    |resid_gpu - x| <= 2^-24 (|x| + TOL_M model) + TOL_M model + 2^-149
(the fp32 rounding of a float64 value that is itself within TOL_M of the reference's).  Nothing here was tuned on the GPU.
Statistics: the reference is given the GPU's own model map, so r is two rounded operations on both sides: counts, maxabs_isl and
its position are equal; the five sums add the same float64 terms in another order, so |gpu - ref| <= 2 m 2^-53 sum|t_i| with m the
number of terms and sum|t_i| from the reference (as tests/test_gpu_islands.py derives)."""
import ctypes as C

import numpy as np
import pytest
import torch

import residual_cases as RC
import residual_ref as RR
from gpu_common import detector

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det():
    return detector("fp32", max_batch=1, max_imgsz=160)


def upload(det, a):
    """The array as it is, NaN included."""
    dev = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(det.tdev)
    torch.cuda.synchronize()
    return dev


@pytest.fixture(scope="module")
def resident(det):
    return ({k: upload(det, v) for k, v in RC.images().items()}, {k: upload(det, v) for k, v in RC.backgrounds().items()})


def check_maps(name, rows, model, resid, want):
    r_rows, r_model, r_resid = RC.reference()[name]
    assert np.array_equal(rows, r_rows), "%s: rows\n%s\nreference\n%s" % (name, rows, r_rows)
    worst = [0.0, 0.0]
    assert (model is not None) == ("model" in want) and (resid is not None) == ("resid" in want), name
    if model is not None:
        g = model.cpu().numpy().astype(np.float64)
        d, bound = np.abs(g - r_model), RR.model_bound(r_model)
        worst[0] = float((d / bound).max())
        assert (d <= bound).all(), "%s: model off by %g of its bound at %s" % (name, worst[0], np.unravel_index(np.argmax(d / bound), d.shape))
    if resid is not None:
        g = resid.cpu().numpy().astype(np.float64)
        d, bound = np.abs(g - r_resid), RR.resid_bound(r_resid, r_model)
        worst[1] = float((d / bound).max())
        assert (d <= bound).all(), "%s: residual off by %g of its bound at %s" % (name, worst[1], np.unravel_index(np.argmax(d / bound), d.shape))
    return worst


@pytest.mark.parametrize("case", RC.render_cases(), ids=lambda c: c[0])
def test_render_case(det, resident, case):
    name, key, comp, nsigma, with_bkg, want = case
    imgs, bkgs = resident
    rows, model, resid = det.render_gaussians(imgs[key], comp, nsigma, bkgs[key] if with_bkg else None, want)
    worst = check_maps(name, rows, model, resid, want)
    print("%s: largest difference %.3f (model) %.3f (residual) of the bound" % (name, worst[0], worst[1]))
    # a second call gives the same bytes
    rows2, model2, resid2 = det.render_gaussians(imgs[key], comp, nsigma, bkgs[key] if with_bkg else None, want)
    assert rows2.tobytes() == rows.tobytes()
    for a, b in ((model, model2), (resid, resid2)):
        assert a is None or a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), name


def test_unaligned_pointers_give_the_same_bytes(det, resident):
    """Image B (MW % 4 == 0) once more through buffers that start 4 bytes after a 16-byte boundary: the pixel-by-pixel path on the
    inputs of the 16-byte path."""
    imgs, bkgs = resident
    name, key, comp, nsigma, _, want = next(c for c in RC.render_cases() if c[0] == "chunk130_B")
    MH, MW = imgs[key].shape

    def shifted(t):
        buf = torch.empty(MH * MW + 1, dtype=torch.float32, device=det.tdev)
        buf[1:] = t.reshape(-1)
        return buf[1:].view(MH, MW)
    _, m0, r0 = det.render_gaussians(imgs[key], comp, nsigma, bkgs[key], want)
    rows, m1, r1 = det.render_gaussians(shifted(imgs[key]), comp, nsigma, shifted(bkgs[key]), want)
    assert m1.data_ptr() % 16 == 0 and shifted(imgs[key]).data_ptr() % 16 == 4
    check_maps(name, rows, m1, r1, want)
    assert m0.cpu().numpy().tobytes() == m1.cpu().numpy().tobytes() and r0.cpu().numpy().tobytes() == r1.cpu().numpy().tobytes()


def test_statistics(det, resident):
    imgs, bkgs = resident
    img = RC.images()["S"]
    boxes, bkg, masks, names = RC.stats_case()
    _, model, _ = det.render_gaussians(imgs["S"], RC.scene()[1], 5.0, None, ("model",))
    got = det.measure_residuals(imgs["S"], model, boxes, bkg, masks)
    ref, ab = RR.residual_stats(img, model.cpu().numpy(), boxes, bkg, masks)
    RR.compare_stats(got, ref, ab, names)
    k = names.index("max_twice")
    assert got[k, 7] == 49.75 and got[k, 8:10].tolist() == [497.0, 33.0]
    assert got[names.index("empty"), 1] == 0 and got[names.index("blank"), 1] == 0 and got[names.index("blank"), 8] == -1
    assert det.measure_residuals(imgs["S"], model, boxes, bkg, masks).tobytes() == got.tobytes()
    assert det.measure_residuals(imgs["S"], model, np.zeros((0, 4)), np.zeros(0), []).shape == (0, RR.RES_FIELDS)


def test_render_arguments(det, resident):
    from caesar_yolo_amd import lib as L
    imgs, bkgs = resident
    dev, MH, MW = imgs["A"], 70, 75
    comp = np.ascontiguousarray(RC.grid_components(3))
    rows = np.zeros((3, L.CY_RND_FIELDS))
    model = torch.empty((MH, MW), dtype=torch.float32, device=det.tdev)
    resid = torch.empty_like(model)
    dp = C.POINTER(C.c_double)

    def call(**kw):
        a = dict(img=det._p(dev), mh=MH, mw=MW, c=comp.ctypes.data_as(dp), m=3, ns=5.0, b=det._p(bkgs["A"]), mo=det._p(model), re=det._p(resid),
                 r=rows.ctypes.data_as(dp))
        a.update(kw)
        return det.lib.cy_render_gaussians(det.ctx, a["img"], a["mh"], a["mw"], a["c"], a["m"], a["ns"], a["b"], a["mo"], a["re"], a["r"], det._stream())

    assert call() == 0
    ref = det.render_gaussians(dev, comp, 5.0, bkgs["A"])
    assert rows.tobytes() == ref[0].tobytes() and model.cpu().numpy().tobytes() == ref[1].cpu().numpy().tobytes()
    assert call(m=0, c=None, r=None) == 0 and call(b=None) == 0 and call(mo=None) == 0 and call(re=None) == 0
    for bad in (dict(ns=0.999), dict(ns=8.001), dict(ns=float("nan")), dict(mh=0), dict(mw=-1), dict(img=None), dict(mo=None, re=None),
                dict(mh=65536, mw=32768), dict(m=-1), dict(m=(1 << 20) + 1), dict(c=None), dict(r=None)):
        assert call(**bad) == -1, bad
    # a tile table above 2^27 entries: 2^20 components of 289 tiles each (both half-widths capped, in the middle of a 600 x 600
    # image); the planner refuses before anything is queued
    wide = np.tile(np.array([[1.0, 300.0, 300.0, 1e-6, 0.0, 1e-6]]), (1 << 20, 1))
    big_rows = np.zeros((1 << 20, L.CY_RND_FIELDS))
    flat = torch.zeros((600, 600), dtype=torch.float32, device=det.tdev)
    out = torch.empty_like(flat)
    rc = det.lib.cy_render_gaussians(det.ctx, det._p(flat), 600, 600, wide.ctypes.data_as(dp), 1 << 20, 5.0, None, det._p(out), None,
                                     big_rows.ctypes.data_as(dp), det._stream())
    assert rc == -1 and b"2^27" in det.lib.cy_last_error(det.ctx)
    with pytest.raises(L.CyError):
        det.render_gaussians(dev, comp, 5.0, bkgs["B"])
    with pytest.raises(L.CyError):
        det.render_gaussians(dev, comp, 5.0, None, want=())


def test_residual_arguments(det, resident):
    from caesar_yolo_amd import lib as L
    imgs, _ = resident
    dev = imgs["S"]
    MH, MW = RC.images()["S"].shape
    boxes, bkg, masks, _ = RC.stats_case()
    n = len(boxes)
    model = torch.zeros((MH, MW), dtype=torch.float32, device=det.tdev)
    off = np.zeros(n + 1, np.int64)
    np.cumsum([m.size for m in masks], out=off[1:])
    mask = np.concatenate([m.reshape(-1) for m in masks])
    out = np.zeros((n, L.CY_RES_FIELDS))
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_longlong)

    def call(**kw):
        a = dict(img=det._p(dev), mo=det._p(model), mh=MH, mw=MW, b=boxes.ctypes.data_as(dp), g=bkg.ctypes.data_as(dp), n=n,
                 m=C.c_void_p(mask.ctypes.data), f=off.ctypes.data_as(lp), o=out.ctypes.data_as(dp))
        a.update(kw)
        return det.lib.cy_measure_residuals(det.ctx, a["img"], a["mo"], a["mh"], a["mw"], a["b"], a["g"], a["n"], a["m"], a["f"], a["o"], det._stream())

    assert call() == 0
    assert out.tobytes() == det.measure_residuals(dev, model, boxes, bkg, masks).tobytes()
    assert call(n=0) == 0 and call(n=0, img=None, mo=None, b=None, g=None, m=None, f=None, o=None) == 0
    for k in ("img", "mo", "b", "g", "m", "f", "o"):
        assert call(**{k: None}) == -1, k
    for bad in (dict(mh=0), dict(mw=-1), dict(mh=65536, mw=32768), dict(n=-1)):
        assert call(**bad) == -1, bad
    off2 = off.copy()
    off2[1] += 1
    assert call(f=off2.ctypes.data_as(lp)) == -1
    with pytest.raises(L.CyError):
        det.measure_residuals(dev, model, boxes, bkg[:-1], masks)
    with pytest.raises(L.CyError):
        det.measure_residuals(dev, model, boxes, bkg, masks[:-1] + [masks[-1][:-1]])


def test_kernel_ms_before_first_call():
    """A context of its own: -1 before the first call, >= 0 after it."""
    from caesar_yolo_amd.model import HipDetector
    from gpu_common import seeded_weights
    d = HipDetector(seeded_weights("l", 5)[0], device=0, precision="fp32", max_batch=1, max_imgsz=160)
    assert d.render_kernel_ms() == -1.0 and d.residual_kernel_ms() == -1.0
    dev = upload(d, RC.images()["A"])
    _, model, _ = d.render_gaussians(dev, RC.grid_components(3), 5.0, None, ("model",))
    assert d.render_kernel_ms() >= 0.0 and d.residual_kernel_ms() == -1.0
    d.measure_residuals(dev, model, [[2.0, 2.0, 20.0, 20.0]], [0.5], [np.ones((19, 19), np.uint8)])
    assert d.residual_kernel_ms() >= 0.0


def test_window_above_the_maximum(det):
    """A window of more than 2^24 pixels: status 1 and nothing measured, beside an ordinary window."""
    n = 4104                                                      # 4104 x 4104 = 16 842 816 > 2^24
    img = np.full((n, n), 0.001, np.float32)
    comp = np.array([RC.gauss_params(40.0, 210.3, 111.8, 2.0, 2.0, 0.0), RC.gauss_params(30.0, 218.1, 112.4, 2.0, 1.5, 40.0)])
    img[100:124, 200:229] += RR.model_map(comp, RR.rectangles(comp, 5.0, n, n), n, n)[100:124, 200:229].astype(np.float32)
    dev = upload(det, img)
    rows, model, _ = det.render_gaussians(dev, comp, 5.0, None, ("model",))
    assert rows[:, 0].tolist() == [0.0, 0.0]
    boxes = np.array([[0, 0, n - 1, n - 1], [200, 100, 228, 123]], np.float64)
    small = np.ones((24, 29), np.uint8)
    big = np.zeros((n, n), np.uint8)
    big[100:124, 200:229] = small
    got = det.measure_residuals(dev, model, boxes, [0.0, 0.0], [big, small])
    assert got[0].tolist() == [1.0, 0, 0, 0, 0, 0, 0, 0, -1.0, -1.0, 0, 0]
    ref, ab = RR.residual_stats(img[:200, :300], model[:200, :300].cpu().numpy(), boxes[1:], [0.0], [small])
    assert np.array_equal(got[1, [0, 1, 2, 7, 8, 9]], ref[0, [0, 1, 2, 7, 8, 9]])
    for f, t in ((3, 0), (4, 1), (5, 2), (6, 3), (10, 4)):
        assert abs(got[1, f] - ref[0, f]) <= 2.0 * ref[0, 1] * 2.0 ** -53 * ab[0, t]
