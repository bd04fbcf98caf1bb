"""cy_measure_background and cy_expand_background on the GPU against the float64 numpy reference (tests/bkg_ref.py: a sort per
cell) and measure.sample_mesh, on the 2048 x 2048 synthetic mosaic of tests/test_gpu_measure.py (NaN strip on the right, all-zero
block in the middle, isolated blank pixels) with a constant patch wider than a cell, a gradient region and a bright stamp added.

Comparison: every field of every cell is a count, a selection or one rounded float64 operation on selections, so none depends on the
order in which pixels are visited: all eight fields of EVERY cell equal the reference bit for bit (none skipped).  The expanded maps
are the float64 expression of sample_mesh rounded to fp32 on both sides: equal bit for bit at every pixel."""
import ctypes as C

import numpy as np
import pytest
import torch

import bkg_ref
from gpu_common import detector

pytestmark = pytest.mark.gpu

N = 2048
CELLS = (64, 100, 128, 300, 4096)         # 100: partial edge cells of 48; 300: beyond the LDS form; 4096: one partial cell = the image


def make_scene():
    from caesar_yolo_amd import synth
    img = synth.make_mosaic(n=N, seed=7)                  # NaN strip: columns 1984..2047; zero block: [1024, 1536) x [1024, 1536)
    img[300:303, 400:405] = np.float32(0.25)
    img[310, 420] = img[312, 418] = np.float32(0.5)
    img[600:640, 700:740] = np.float32(0.125)
    img[1200:1203, 1100:1103] = np.float32(0.75)
    img[800, 800] = np.float32(-1.0)
    holes = np.random.default_rng(3).integers(0, N, (40000, 2))      # isolated blank pixels (about 1 %) in the rows from 1040 on
    holes = holes[holes[:, 0] >= 1040]
    img[holes[:, 0], holes[:, 1]] = 0.0
    img[1005, 30] = 0.0
    img[1300:1940, 100:740] = np.float32(0.125)           # a constant patch that holds whole cells of 64, 100, 128 and 300 pixels
    img[100:400, 1200:1700] += (np.arange(500, dtype=np.float32) * np.float32(2e-6))[None, :]      # a gradient across several cells
    img[690:695, 1500:1505] = np.float32(10.0)            # a bright stamp: 25 pixels that the first clip removes
    return img


@pytest.fixture(scope="module")
def scene():
    img = make_scene()
    host = np.where(np.isfinite(img), img, np.float32(0)).astype(np.float32)     # what cy_mosaic_prepare leaves
    det = detector("fp32", max_batch=1, max_imgsz=160)
    dev = det.mosaic_to_device(img)
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), host)
    return det, dev, host


def assert_rows_equal(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float64, (what, got.shape, ref.shape)
    a, b = got.view(np.uint64), ref.view(np.uint64)
    if not np.array_equal(a, b):
        cy, cx, f = (int(v[0]) for v in np.nonzero(a != b))
        raise AssertionError("%s: %d of %d values differ; first: cell (%d, %d) %s = %r on the GPU, %r in the reference (GPU row %s, reference row %s)" % (
            what, int((a != b).sum()), a.size, cy, cx, bkg_ref.FIELDS[f], got[cy, cx, f], ref[cy, cx, f], got[cy, cx], ref[cy, cx]))


@pytest.mark.parametrize("k", [3.0, 2.5])
@pytest.mark.parametrize("niter", [0, 1, 3, 10])
@pytest.mark.parametrize("cell", CELLS)
def test_cells_equal_the_reference(scene, cell, niter, k):
    det, dev, host = scene
    ref = bkg_ref.background(host, cell, k, niter)
    got = det.measure_background(dev, cell=cell, k=k, niter=niter)
    ncy = ncx = -(-N // cell)
    assert ref.shape == (ncy, ncx, 8)
    r = lambda cy, cx: dict(zip(bkg_ref.FIELDS, ref[cy, cx]))
    # the scene is what it claims to be, on the reference side
    if niter == 0:
        assert np.all(ref[:, :, 0] == ref[:, :, 1]) and np.all(ref[:, :, 6] == 0) and np.all(np.isneginf(ref[:, :, 4])) and np.all(np.isposinf(ref[:, :, 5]))
    else:
        assert np.all(ref[:, :, 6] <= niter) and np.all(ref[:, :, 1] <= ref[:, :, 0])
        assert (ref[:, :, 6] > 0).any()
    if cell == 4096:
        assert ref.shape[:2] == (1, 1) and ref[0, 0, 0] == np.count_nonzero(host)
    if cell in (64, 128):
        zc = r(1280 // cell, 1280 // cell)                   # inside the zero block
        assert zc["n0"] == 0 and zc["n"] == 0 and zc["bkg"] == 0 and zc["rms"] == 0 and zc["L"] == -np.inf and zc["H"] == np.inf
        nc = r(0, ncx - 1)                                   # inside the NaN strip (64) / half in it (128)
        assert nc["n0"] == (0 if cell == 64 else 64 * 128)
    if cell == 100:
        assert r(0, ncx - 1)["n0"] == 0 and r(ncy - 1, 0)["n0"] <= 48 * 100 and r(ncy - 1, 0)["n0"] > 0      # partial edge cells
    cc = {64: (21, 2), 100: (14, 2), 128: (11, 1), 300: (5, 1)}.get(cell)
    if cc:                                                   # a cell wholly inside the constant patch
        p = r(*cc)
        assert p["n0"] == cell * cell and p["n"] == p["n0"] and p["bkg"] == 0.125 and p["rms"] == 0.0 and p["rounds"] == 0
    if cell in (64, 128) and niter >= 1:
        s = r(690 // cell, 1500 // cell)                     # the bright stamp is clipped away
        assert s["rounds"] >= 1 and s["H"] < 10.0 and s["n"] <= s["n0"] - 25
    assert_rows_equal(got, ref, "cell %d, niter %d, k %g" % (cell, niter, k))
    print("cell %d niter %d k %g: %d cells equal bit for bit; kernel %.3f ms" % (cell, niter, k, ncy * ncx, det.background_kernel_ms()))


def test_image_one_row_taller_than_a_multiple_of_the_cell(scene):
    det, dev, host = scene
    for rows, cell in ((1025, 64), (1281, 128), (601, 300)):
        sub = dev[:rows].contiguous()
        ref = bkg_ref.background(host[:rows], cell, 3.0, 3)
        assert ref.shape[0] == rows // cell + 1 and 0 < ref[-1, 0, 0] <= cell
        assert_rows_equal(det.measure_background(sub, cell=cell, k=3.0, niter=3), ref, "%d rows, cell %d" % (rows, cell))


def test_arguments_and_determinism(scene):
    det, dev, host = scene
    from caesar_yolo_amd import lib as L
    lib = L.load()
    dp = C.POINTER(C.c_double)
    out = np.zeros((32, 32, L.CY_BKG_FIELDS), np.float64)
    args = lambda cell=64, k=3.0, niter=3, img=dev.data_ptr(), mh=N, mw=N, o=out.ctypes.data_as(dp), ctx=det.ctx: (
        ctx, C.c_void_p(img) if img is not None else None, mh, mw, cell, C.c_double(k), niter, o, det._stream())
    assert lib.cy_measure_background(*args()) == 0
    for bad in (dict(cell=3), dict(cell=4097), dict(cell=0), dict(cell=-64), dict(k=0.0), dict(k=-1.0), dict(k=float("nan")), dict(niter=-1),
                dict(niter=33), dict(mh=0), dict(mw=-5), dict(mh=65536, mw=32768), dict(img=None), dict(o=None), dict(ctx=None)):
        assert lib.cy_measure_background(*args(**bad)) == -1, bad          # CY_ERR_ARG
    with pytest.raises(L.CyError):
        det.measure_background(dev, cell=2)
    with pytest.raises(L.CyError):
        det.measure_background(dev, k=float("nan"))
    with pytest.raises(L.CyError):
        det.measure_background(dev.double())
    for cell in (64, 300):
        a = det.measure_background(dev, cell=cell, k=3.0, niter=3)
        b = det.measure_background(dev, cell=cell, k=3.0, niter=3)
        assert a.tobytes() == b.tobytes()                                  # run to run: the same bytes
    assert det.background_kernel_ms() > 0
    # cy_expand_background
    mesh = np.zeros((32, 32, 2), np.float64)
    bk, rm = torch.empty((N, N), dtype=torch.float32, device=dev.device), torch.empty((N, N), dtype=torch.float32, device=dev.device)
    eargs = lambda m=mesh.ctypes.data_as(dp), ncy=32, ncx=32, cell=64, mh=N, mw=N, b=bk.data_ptr(), r=rm.data_ptr(), ctx=det.ctx: (
        ctx, m, ncy, ncx, cell, mh, mw, C.c_void_p(b) if b else None, C.c_void_p(r) if r else None, det._stream())
    assert lib.cy_expand_background(*eargs()) == 0
    assert lib.cy_expand_background(*eargs(b=None)) == 0 and lib.cy_expand_background(*eargs(r=None)) == 0
    for bad in (dict(b=None, r=None), dict(m=None), dict(ctx=None), dict(ncy=31), dict(ncx=33), dict(cell=128), dict(cell=3), dict(cell=4097),
                dict(mh=0), dict(mw=-1), dict(mh=65536, mw=32768, ncy=1024, ncx=512)):
        assert lib.cy_expand_background(*eargs(**bad)) == -1, bad
    with pytest.raises(L.CyError):
        det.expand_background(mesh, 100, (N, N))


def expected_maps(mesh, cell, MH, MW):
    from caesar_yolo_amd import measure
    x, y = np.meshgrid(np.arange(MW, dtype=np.float64), np.arange(MH, dtype=np.float64))
    with np.errstate(over="ignore"):
        return measure.sample_mesh(mesh, cell, x, y).astype(np.float32)


@pytest.mark.parametrize("cell", [64, 100])
def test_expansion_of_the_whole_image(scene, cell):
    from caesar_yolo_amd import measure
    det, dev, host = scene
    mesh, ndef = measure.fill_mesh(bkg_ref.background(host, cell, 3.0, 3), 64)
    assert 0 < ndef < mesh.shape[0] * mesh.shape[1]           # some cells were filled (zero block, NaN strip)
    want = expected_maps(mesh, cell, N, N)
    bkg, rms = det.expand_background(mesh, cell, (N, N))
    torch.cuda.synchronize()
    for name, g, plane in (("bkg", bkg, 0), ("rms", rms, 1)):
        g = g.cpu().numpy()
        w = np.ascontiguousarray(want[:, :, plane])
        assert g.dtype == np.float32 and g.shape == (N, N)
        bad = g.view(np.uint32) != w.view(np.uint32)
        assert not bad.any(), "cell %d %s: %d pixels differ, first at %s: %r on the GPU, %r expected" % (
            cell, name, int(bad.sum()), tuple(np.argwhere(bad)[0]), g[bad][0], w[bad][0])
        assert len(np.unique(w)) > 1000                     # the map is not flat: the comparison says something
    # constant outside the outermost centres
    c = (cell - 1) / 2.0
    b = bkg.cpu().numpy()
    assert np.all(b[0, :int(c) + 1] == np.float32(mesh[0, 0, 0])) and np.all(b[:int(c) + 1, 0] == np.float32(mesh[0, 0, 0]))
    only, none = det.expand_background(mesh, cell, (N, N), want=("rms",))
    assert only is None and np.array_equal(none.cpu().numpy().view(np.uint32), np.ascontiguousarray(want[:, :, 1]).view(np.uint32))


@pytest.mark.parametrize("shape", [(50, 2048), (2048, 50), (40, 37)])
def test_expansion_of_one_row_or_one_column_of_cells(scene, shape):
    det, dev, host = scene
    MH, MW = shape
    cell = 64
    ncy, ncx = -(-MH // cell), -(-MW // cell)
    assert 1 in (ncy, ncx)
    rng = np.random.default_rng(5)
    mesh = np.stack([rng.normal(1e-4, 1e-5, (ncy, ncx)), rng.uniform(1e-4, 2e-4, (ncy, ncx))], 2)
    want = expected_maps(mesh, cell, MH, MW)
    bkg, rms = det.expand_background(mesh, cell, shape)
    torch.cuda.synchronize()
    assert np.array_equal(bkg.cpu().numpy().view(np.uint32), np.ascontiguousarray(want[:, :, 0]).view(np.uint32))
    assert np.array_equal(rms.cpu().numpy().view(np.uint32), np.ascontiguousarray(want[:, :, 1]).view(np.uint32))
    if ncy == 1:                                             # one row of cells: every image row is the same
        assert np.array_equal(want[0], want[-1])
