"""cy_fit_blends on the GPU against the numpy float64 restatement of the same algorithm (tests/blend_ref.py, its "seq" variant: the
kernel's own association of the sums) on the inputs of tests/blend_cases.py.

Every row below ncomp compares status, npix, group, nmembers, slot, cov_ok and niter <= max_iter.  On status 0 it also compares the
member's six parameters within |dp_j| <= TOL (|p_j| + 1e-3), F within TOL (|F| + 1e-3 A^2 npix) and the 21 entries of its block
of C within TOL_C sqrt(C_ii C_jj).  TOL and TOL_C are blend_ref's: 16 times the largest difference between the reference's own
variants on these very inputs, measured on the CPU (tests/test_blend_cpu.py recomputes them).  Rows that were not fitted (status 3,
4, 5) report their start bit for bit; status 6 rows and rows beyond ncomp are zero as defined.
A. drawn cases: none is left out.  B. 300 random boxes: a row may be left out only when the reference's variants disagree on its
status or the reference's cond(H) exceeds 1e10, and at most 2 % of the fitted rows are.  C. arguments and limits."""
import ctypes as C

import numpy as np
import pytest
import torch

import blend_cases
import blend_ref
import fit_cases
from gpu_common import detector

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def det():
    return detector("fp32", max_batch=1, max_imgsz=160)


def upload(det, img):
    """The image as it is, NaN included."""
    dev = torch.from_numpy(np.ascontiguousarray(img, np.float32)).to(det.tdev)
    torch.cuda.synchronize()
    return dev


def compare(got, ref, ncomp, start, max_iter, what, skip=None):
    """-> (rows compared, rows with status 0 compared, largest parameter difference in units of TOL, largest C difference in
    units of TOL_C)."""
    assert got.shape == ref.shape
    nrows = n0 = 0
    worst = worst_c = 0.0
    for i in range(ref.shape[0]):
        assert not got[i, int(ncomp[i]):].any(), "%s, source %d: a row at or beyond ncomp is not zero" % (what, i)
        for k in range(int(ncomp[i])):
            if skip is not None and skip[i, k]:
                continue
            g, r = got[i, k], ref[i, k]
            tag = "%s, source %d component %d" % (what, i, k)
            nrows += 1
            assert g[0] == r[0], "%s: status %g, reference %g (niter %g / %g)" % (tag, g[0], r[0], g[1], r[1])
            assert g[2] == r[2], "%s: npix %g, reference %g" % (tag, g[2], r[2])
            assert np.array_equal(g[5:8], r[5:8]), "%s: group, nmembers, slot %s, reference %s" % (tag, g[5:8], r[5:8])
            assert g[14] == r[14], "%s: cov_ok %g, reference %g" % (tag, g[14], r[14])
            assert 0 <= g[1] <= max_iter and g[1] == int(g[1]), "%s: niter %g" % (tag, g[1])
            if r[0] in (3.0, 4.0, 5.0):
                assert g[1] == 0 and np.array_equal(g[8:14], start[i, k], equal_nan=True) and not g[3:5].any() and not g[14:].any(), tag
            if r[0] == 6.0:
                assert g[5] == k and g[6] == 1 and not g[1:5].any() and not g[7:].any(), tag
            if r[0] == 1.0:
                assert not g[1:].any(), tag
            if r[0] == 2.0:
                assert np.isfinite(g).all(), tag
            if r[0] != 0.0:
                continue
            n0 += 1
            d = np.abs(g[8:14] - r[8:14]) / (np.abs(r[8:14]) + 1e-3)
            worst = max(worst, float(d.max()) / blend_ref.TOL)
            assert (d <= blend_ref.TOL).all(), "%s: parameters %s, reference %s, difference %s > TOL %g" % (tag, g[8:14], r[8:14], d, blend_ref.TOL)
            assert abs(g[3] - r[3]) <= blend_ref.TOL * (abs(r[3]) + 1e-3 * r[8] * r[8] * r[2]), "%s: F %r, reference %r" % (tag, g[3], r[3])
            if r[14]:
                diag = np.sqrt(np.abs(r[[15, 21, 26, 30, 33, 35]]))
                for t, (a, b) in enumerate(blend_ref.IU):
                    dc = abs(g[15 + t] - r[15 + t]) / max(diag[a] * diag[b], 1e-300)
                    worst_c = max(worst_c, dc / blend_ref.TOL_C)
                    assert dc <= blend_ref.TOL_C, "%s: C%d%d %r, reference %r" % (tag, a, b, g[15 + t], r[15 + t])
    return nrows, n0, worst, worst_c


# ---- A. drawn cases
def test_drawn_cases(det):
    img, c, (res, _), one, (res1, _) = blend_cases.drawn_reference()
    dev = upload(det, img)
    boxes, bkg, ncomp, start, masks = c.arrays()
    got = det.fit_blends(dev, boxes, bkg, ncomp, start, masks)
    assert det.blend_kernel_ms() >= 0.0
    nrows, n0, worst, worst_c = compare(got, res[0], ncomp, start, 64, "drawn")
    print("drawn: %d rows, %d with status 0, worst parameter difference %.3g TOL, worst C difference %.3g TOL_C" % (nrows, n0, worst, worst_c))
    assert nrows == int(ncomp.sum()) and n0 >= 40
    for nm, want in blend_cases.STATUS.items():
        st = got[c.names.index(nm), :len(want), 0].tolist()
        assert all(w is None and s in (0.0, 2.0) or s == w for s, w in zip(st, want)), (nm, st)
    for nm, want in blend_cases.GROUPS.items():
        assert got[c.names.index(nm), :len(want), 5].tolist() == want, nm
    assert not got[c.names.index("ncomp0")].any()
    i = c.names.index("pix13")
    assert got[i, 0, 2] == 13 and got[i, 0, 0] in (0.0, 2.0) and got[c.names.index("pix12"), 0, 2] == 12
    # the two sides of the LDS boundary, on the same data
    a, b = got[c.names.index("wide4096")], got[c.names.index("wide4097")]
    assert a[0, 2] == 4096 and b[0, 2] == 4097 and a[0, 0] == b[0, 0] == 0
    assert np.all(np.abs(a[:2, 8:14] - b[:2, 8:14]) <= 1e-3 * (np.abs(a[:2, 8:14]) + 1e-3))       # one pixel more among 4096
    assert got[c.names.index("wide6400"), 0, 2] == 6400
    # the same call twice: byte-equal
    again = det.fit_blends(dev, boxes, bkg, ncomp, start, masks)
    assert got.tobytes() == again.tobytes()
    # max_iter = 1
    boxes1, bkg1, ncomp1, start1, masks1 = c.arrays(one)
    got1 = det.fit_blends(dev, boxes1, bkg1, ncomp1, start1, masks1, max_iter=1)
    nrows1, _, _, _ = compare(got1, res1[0], ncomp1, start1, 1, "max_iter 1")
    assert nrows1 == int(ncomp1.sum()) and (got1[:, 0, 1] == 1).all()


# ---- B. random cases
def test_random_boxes(det):
    img, boxes, thr4, (bkg, ncomp, start_ref, masks_ref), (rr, cond) = blend_cases.random_reference()
    dev = det.mosaic_to_device(img)
    torch.cuda.synchronize()
    rows, comp, masks = det.deblend_islands(dev, boxes, thr4, conn=8, radius=2, return_masks=True)
    assert all(np.array_equal(a, b) for a, b in zip(masks, masks_ref)) and np.array_equal(rows[:, 3], ncomp)
    # the reference's starts (its own single fits) are given to the GPU as they are: the comparison is of the joint fit alone
    got = det.fit_blends(dev, boxes, bkg, ncomp, start_ref, masks)
    skip = blend_cases.excluded(rr, cond, ncomp)
    fitted = int(np.isin(rr[0][:, :, 0], (0.0, 2.0))[np.arange(16)[None, :] < ncomp[:, None]].sum())
    assert skip.sum() <= 0.02 * fitted, "%d of %d fitted rows left out" % (skip.sum(), fitted)
    nrows, n0, worst, worst_c = compare(got, rr[0], ncomp, start_ref, 64, "random", skip)
    print("random: %d rows compared, %d left out, %d with status 0, worst parameter difference %.3g TOL, C %.3g TOL_C" % (
        nrows, skip.sum(), n0, worst, worst_c))
    assert n0 >= 100


# ---- C. arguments and limits
def test_arguments_and_limits(det):
    from caesar_yolo_amd import lib as L
    img, c = blend_cases.drawn()
    dev = upload(det, img)
    sel = [c.names.index("pair_resolved"), c.names.index("chain3")]
    boxes, bkg, ncomp, start, masks = c.arrays(sel)
    n = len(sel)
    off = np.zeros(n + 1, np.int64)
    np.cumsum([m.size for m in masks], out=off[1:])
    mask = np.concatenate([m.reshape(-1) for m in masks])
    out = np.zeros((n, 16, L.CY_BLEND_FIELDS))
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    lib = det.lib

    def call(**kw):
        a = dict(img=det._p(dev), mh=fit_cases.MH, mw=fit_cases.MW, b=boxes.ctypes.data_as(dp), g=bkg.ctypes.data_as(dp), nc=ncomp.ctypes.data_as(ip),
                 s=start.ctypes.data_as(dp), n=n, it=64, m=C.c_void_p(mask.ctypes.data), f=off.ctypes.data_as(lp), o=out.ctypes.data_as(dp))
        a.update(kw)
        return lib.cy_fit_blends(det.ctx, a["img"], a["mh"], a["mw"], a["b"], a["g"], a["nc"], a["s"], a["n"], a["it"], a["m"], a["f"], a["o"],
                                 det._stream())

    assert call() == 0
    ref = det.fit_blends(dev, boxes, bkg, ncomp, start, masks)
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
    m2[5] = 255                                                   # unassigned: allowed, links nothing
    assert call(m=C.c_void_p(m2.ctypes.data)) == 0
    with pytest.raises(L.CyError):
        det.fit_blends(dev, boxes, bkg, ncomp, start, masks, max_iter=0)
    with pytest.raises(L.CyError):
        det.fit_blends(dev, boxes, bkg[:-1], ncomp, start, masks)
    with pytest.raises(L.CyError):
        det.fit_blends(dev, boxes, bkg, ncomp, start, [masks[0], masks[1][:-1]])
    empty = det.fit_blends(dev, np.zeros((0, 4)), np.zeros(0), np.zeros(0, np.int32), np.zeros((0, 16, 6)), [])
    assert empty.shape == (0, 16, L.CY_BLEND_FIELDS)


def test_kernel_ms_before_first_call():
    """A context of its own: -1 before the first call that launches, >= 0 after it; a call without a job leaves it alone."""
    from caesar_yolo_amd.model import HipDetector
    from gpu_common import seeded_weights
    d = HipDetector(seeded_weights("l", 5)[0], device=0, precision="fp32", max_batch=1, max_imgsz=160)
    assert d.blend_kernel_ms() == -1.0
    img, c = blend_cases.drawn()
    dev = upload(d, img)
    got = d.fit_blends(dev, *c.arrays([c.names.index(nm) for nm in ("ncomp0", "row_gap", "chain5", "empty")]))
    assert d.blend_kernel_ms() == -1.0 and got[1, :2, 0].tolist() == [6.0, 6.0] and got[2, :5, 0].tolist() == [5.0] * 5
    d.fit_blends(dev, *c.arrays([c.names.index("pair_ellipses")]))
    assert d.blend_kernel_ms() >= 0.0


def test_window_above_the_maximum(det):
    """A window of more than 2^24 pixels: status 1 on every component row below ncomp, nothing else, beside an ordinary blend."""
    n = 4104                                                      # 4104 x 4104 = 16 842 816 > 2^24
    img = np.full((n, n), 0.001, np.float32)
    comps = [(40.0, 10.3, 11.8, 2.0, 2.0, 0.0), (30.0, 18.1, 12.4, 2.0, 2.0, 0.0)]
    g = sum(fit_cases.gauss((24, 29), *cc) for cc in comps).astype(np.float32)
    img[100:124, 200:229] = g
    dev = upload(det, img)
    boxes = np.array([[0, 0, n - 1, n - 1], [200, 100, 228, 123]], np.float64)
    small = blend_cases.basins((24, 29), comps, g, 0.5)
    big = np.zeros((n, n), np.uint8)
    big[100:124, 200:229] = small
    start = np.zeros((2, 16, 6))
    start[:, :2] = [fit_cases.truth_params(cc[0] * 0.9, 200 + cc[1] + 0.3, 100 + cc[2] - 0.2, *cc[3:]) for cc in comps]
    got = det.fit_blends(dev, boxes, [0.0, 0.0], [2, 2], start, [big, small])
    assert got[0, :2, 0].tolist() == [1.0, 1.0] and not got[0, :, 1:].any() and not got[0, 2:].any()
    ref = blend_ref.fit_blends(img, boxes[1:], [0.0], [2], start[1:], [small])
    compare(got[1:], ref, [2], start[1:], 64, "beside the large window")
