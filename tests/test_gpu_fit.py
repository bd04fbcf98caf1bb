"""cy_fit_components on the GPU against the numpy float64 restatement of the same algorithm (tests/fit_ref.py, its "tree" variant:
the kernel's own association of the sums) on the inputs of tests/fit_cases.py.

Every job compares status, npix and niter <= max_iter.  On status 0 it also compares the six parameters within
|dp_j| <= TOL (|p_j| + 1e-3), and F and the 21 entries of H within TOL times their magnitude (F: |F| + 1e-3 A^2 npix, a
thousandth of the sum of squares of a model of that amplitude on every pixel; H_ij: sqrt(H_ii H_jj)).  TOL is fit_ref.TOL: 16 times the largest difference between the reference's own
variants on these very inputs, measured on the CPU (tests/test_fit_cpu.py recomputes it) over the jobs that are compared with it.  Jobs that were not fitted (status
3, 4) report their start bit for bit.
A. drawn cases: none is left out.  B. 300 random boxes: a job may be left out only when the reference's variants disagree on
its status or the reference's cond(H) exceeds 1e10, and at most 2 % of the jobs are.  C. arguments and limits."""
import ctypes as C

import numpy as np
import pytest
import torch

import fit_cases
import fit_ref
from gpu_common import detector

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det():
    return detector("fp32", max_batch=1, max_imgsz=160)


def upload(det, img):
    """The image as it is, NaN included (mosaic_to_device would blank them; the kernel's validity test sees both kinds)."""
    dev = torch.from_numpy(np.ascontiguousarray(img, np.float32)).to(det.tdev)
    torch.cuda.synchronize()
    return dev


def compare(got, ref, ncomp, start, max_iter, what, skip=None, status_only=()):
    """-> (jobs compared, jobs with status 0 compared, largest parameter difference in units of TOL).  status_only: sources whose
    jobs compare status, npix and niter alone."""
    assert got.shape == ref.shape
    njobs = n0 = 0
    worst = 0.0
    for i in range(ref.shape[0]):
        assert not got[i, int(ncomp[i]):].any(), "%s, source %d: a row at or beyond ncomp is not zero" % (what, i)
        for k in range(int(ncomp[i])):
            if skip is not None and skip[i, k]:
                continue
            g, r = got[i, k], ref[i, k]
            tag = "%s, source %d component %d" % (what, i, k)
            njobs += 1
            assert g[0] == r[0], "%s: status %g, reference %g (niter %g / %g)" % (tag, g[0], r[0], g[1], r[1])
            assert g[2] == r[2], "%s: npix %g, reference %g" % (tag, g[2], r[2])
            assert 0 <= g[1] <= max_iter and g[1] == int(g[1]), "%s: niter %g" % (tag, g[1])
            if r[0] in (3.0, 4.0):
                assert g[1] == 0 and np.array_equal(g[5:11], start[i, k], equal_nan=True) and not g[3:5].any() and not g[11:].any(), tag
            if r[0] == 2.0:
                assert np.isfinite(g[3:]).all(), tag
            if r[0] != 0.0 or i in status_only:
                continue
            n0 += 1
            d = np.abs(g[5:11] - r[5:11]) / (np.abs(r[5:11]) + 1e-3)
            worst = max(worst, float(d.max()) / fit_ref.TOL)
            assert (d <= fit_ref.TOL).all(), "%s: parameters %s, reference %s, difference %s > TOL %g" % (tag, g[5:11], r[5:11], d, fit_ref.TOL)
            diag = np.sqrt(np.abs(r[[11, 17, 22, 26, 29, 31]]))
            for t, (a, b) in enumerate(fit_ref.IU):
                assert abs(g[11 + t] - r[11 + t]) <= fit_ref.TOL * max(diag[a] * diag[b], 1e-300), "%s: H%d%d %r, reference %r" % (
                    tag, a, b, g[11 + t], r[11 + t])
            assert abs(g[3] - r[3]) <= fit_ref.TOL * (abs(r[3]) + 1e-3 * r[5] * r[5] * r[2]), "%s: F %r, reference %r" % (tag, g[3], r[3])
    return njobs, n0, worst


# ---- A. drawn cases
def test_drawn_cases(det):
    img, c, res, one, res1 = fit_cases.drawn_reference()
    dev = upload(det, img)
    boxes, bkg, ncomp, start, masks = c.arrays()
    got = det.fit_components(dev, boxes, bkg, ncomp, start, masks)
    assert det.fit_kernel_ms() >= 0.0
    # the flat patch has no Gaussian in it: the fit runs a, b, c towards 0 until a step is small, cond(H) = 3e33, and what it must
    # do is end with the reference's status
    njobs, n0, worst = compare(got, res[0], ncomp, start, 64, "drawn", status_only=[c.names.index(nm) for nm in fit_cases.STATUS_ONLY])
    print("drawn: %d jobs, %d with status 0, worst parameter difference %.3g TOL" % (njobs, n0, worst))
    assert njobs == int(ncomp.sum()) and n0 >= 34
    st = {nm: got[i, :max(c.ncomp[i], 1), 0].tolist() for i, nm in enumerate(c.names)}
    assert st["pix6"] == [3.0] and st["pix7"][0] in (0.0, 2.0) and st["inadmissible"] == [4.0] * 4 and st["empty"] == [3.0]
    assert not got[c.names.index("ncomp0")].any()
    # the two sides of the LDS boundary, on the same data
    a, b = got[c.names.index("wide4096"), 0], got[c.names.index("wide4097"), 0]
    assert a[2] == 4096 and b[2] == 4097 and a[0] == b[0] == 0
    assert np.all(np.abs(a[5:11] - b[5:11]) <= fit_ref.TOL * (np.abs(a[5:11]) + 1e-3))
    assert got[c.names.index("wide6400"), 0, 2] == 6400
    # the same call twice: byte-equal
    again = det.fit_components(dev, boxes, bkg, ncomp, start, masks)
    assert got.tobytes() == again.tobytes()
    # max_iter = 1
    boxes1, bkg1, ncomp1, start1, masks1 = c.arrays(one)
    got1 = det.fit_components(dev, boxes1, bkg1, ncomp1, start1, masks1, max_iter=1)
    njobs1, _, _ = compare(got1, res1[0], ncomp1, start1, 1, "max_iter 1")
    assert njobs1 == int(ncomp1.sum()) and (got1[:, 0, 1] == 1).all() and (got1[:, 0, 0] == 2).all()


# ---- B. random cases
def test_random_boxes(det):
    img, boxes, thr4, (bkg, ncomp, start_ref, masks_ref), rr = fit_cases.random_reference()
    dev = det.mosaic_to_device(img)
    torch.cuda.synchronize()
    rows, comp, masks = det.deblend_islands(dev, boxes, thr4, conn=8, radius=2, return_masks=True)
    assert all(np.array_equal(a, b) for a, b in zip(masks, masks_ref)) and np.array_equal(rows[:, 3], ncomp)
    gb, gn, start = fit_cases.random_inputs(img, boxes, thr4, rows, comp)
    # the starts come from the GPU's component sums, the reference's from tests/deblend_ref.py's: equal up to the sums' rounding
    assert np.allclose(start, start_ref, rtol=1e-9, atol=1e-9)
    got = det.fit_components(dev, boxes, gb, gn, start, masks)
    skip = fit_cases.excluded(rr, ncomp)
    total = int(ncomp.sum())
    assert skip.sum() <= 0.02 * total, "%d of %d jobs left out" % (skip.sum(), total)
    njobs, n0, worst = compare(got, rr[0], ncomp, start, 64, "random", skip)
    print("random: %d jobs compared, %d left out, %d with status 0, worst parameter difference %.3g TOL" % (njobs, skip.sum(), n0, worst))
    assert n0 >= fit_cases.MIN_STATUS0 and int((ncomp > 1).sum()) >= fit_cases.MIN_MULTI


# ---- C. arguments and limits
def test_arguments_and_limits(det):
    from caesar_yolo_amd import lib as L
    img, c = fit_cases.drawn()
    dev = upload(det, img)
    sel = [c.names.index("clean_circ"), c.names.index("blend2")]
    boxes, bkg, ncomp, start, masks = c.arrays(sel)
    n = len(sel)
    off = np.zeros(n + 1, np.int64)
    np.cumsum([m.size for m in masks], out=off[1:])
    mask = np.concatenate([m.reshape(-1) for m in masks])
    out = np.zeros((n, 16, L.CY_FIT_FIELDS))
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    lib = det.lib

    def call(**kw):
        a = dict(img=det._p(dev), mh=fit_cases.MH, mw=fit_cases.MW, b=boxes.ctypes.data_as(dp), g=bkg.ctypes.data_as(dp), nc=ncomp.ctypes.data_as(ip),
                 s=start.ctypes.data_as(dp), n=n, it=64, m=C.c_void_p(mask.ctypes.data), f=off.ctypes.data_as(lp), o=out.ctypes.data_as(dp))
        a.update(kw)
        return lib.cy_fit_components(det.ctx, a["img"], a["mh"], a["mw"], a["b"], a["g"], a["nc"], a["s"], a["n"], a["it"], a["m"], a["f"], a["o"],
                                     det._stream())

    assert call() == 0
    ref = det.fit_components(dev, boxes, bkg, ncomp, start, masks)
    assert out.tobytes() == ref.tobytes()
    assert call(n=0) == 0 and call(n=0, b=None, g=None, nc=None, s=None, m=None, f=None, o=None, img=None) == 0
    for k in ("img", "b", "g", "nc", "s", "m", "f", "o"):
        assert call(**{k: None}) == -1, k
    for bad in (dict(mh=0), dict(mw=-1), dict(mh=65536, mw=32768), dict(it=0), dict(it=257), dict(n=-1)):
        assert call(**bad) == -1, bad
    for v in (-1, 17):
        nc2 = ncomp.copy()
        nc2[1] = v
        assert call(nc=nc2.ctypes.data_as(ip)) == -1
    off2 = off.copy()
    off2[1] += 1
    assert call(f=off2.ctypes.data_as(lp)) == -1
    for v in (17, 254):
        m2 = mask.copy()
        m2[5] = v
        assert call(m=C.c_void_p(m2.ctypes.data)) == -1
    m2 = mask.copy()
    m2[5] = 255                                                   # unassigned: allowed, belongs to no job
    assert call(m=C.c_void_p(m2.ctypes.data)) == 0
    with pytest.raises(L.CyError):
        det.fit_components(dev, boxes, bkg, ncomp, start, masks, max_iter=0)
    with pytest.raises(L.CyError):
        det.fit_components(dev, boxes, bkg[:-1], ncomp, start, masks)
    with pytest.raises(L.CyError):
        det.fit_components(dev, boxes, bkg, ncomp, start, [masks[0], masks[1][:-1]])
    empty = det.fit_components(dev, np.zeros((0, 4)), np.zeros(0), np.zeros(0, np.int32), np.zeros((0, 16, 6)), [])
    assert empty.shape == (0, 16, L.CY_FIT_FIELDS)


def test_kernel_ms_before_first_call():
    """A context of its own: -1 before the first call that launches, >= 0 after it; a call without a job leaves it alone."""
    from caesar_yolo_amd.model import HipDetector
    from gpu_common import seeded_weights
    d = HipDetector(seeded_weights("l", 5)[0], device=0, precision="fp32", max_batch=1, max_imgsz=160)
    assert d.fit_kernel_ms() == -1.0
    img, c = fit_cases.drawn()
    dev = upload(d, img)
    i = c.names.index("ncomp0")
    d.fit_components(dev, *c.arrays([i]))
    assert d.fit_kernel_ms() == -1.0
    d.fit_components(dev, *c.arrays([c.names.index("clean_pa30")]))
    assert d.fit_kernel_ms() >= 0.0


def test_window_above_the_maximum(det):
    """A window of more than 2^24 pixels: status 1 on every component row below ncomp, nothing else, beside an ordinary source."""
    n = 4104                                                      # 4104 x 4104 = 16 842 816 > 2^24
    img = np.full((n, n), 0.001, np.float32)
    g = fit_cases.gauss((21, 21), 30.0, 10.2, 9.9, 2.0, 1.5, 30.0).astype(np.float32)
    img[100:121, 200:221] = g
    dev = upload(det, img)
    boxes = np.array([[0, 0, n - 1, n - 1], [200, 100, 220, 120]], np.float64)
    big = np.zeros((n, n), np.uint8)
    big[100:121, 200:221] = 1
    small = np.ones((21, 21), np.uint8)
    start = np.zeros((2, 16, 6))
    start[:, :2] = fit_cases.moment_start(img[100:121, 200:221], small, 0, 0.0, 200, 100)
    got = det.fit_components(dev, boxes, [0.0, 0.0], [2, 1], start, [big, small])
    assert got[0, :2, 0].tolist() == [1.0, 1.0] and not got[0, :, 1:].any() and not got[0, 2:].any()
    ref = fit_ref.fit_components(img, boxes[1:], [0.0], [1], start[1:], [small])
    compare(got[1:], ref, [1], start[1:], 64, "beside the large window")
