"""cy_measure_sources on the GPU against the float64 numpy reference (tests/measure_ref.py) on a 2048 x 2048 synthetic mosaic
(NaN strip on the right, all-zero block in the middle) with a few equal-valued pixels stamped in.

Comparison, for EVERY box (none skipped):
  npix, nring, peak, x_peak, y_peak, bkg, rms   equal, bit for bit: counts, selections and a median do not depend on the order
                                                in which the pixels are visited;
  sum, sw, swx, swy   both sides add the same m float64 terms t_i in some order, so each is within (m - 1) 2^-53 sum|t_i| of the
                      exact value: |gpu - ref| <= 2 m 2^-53 sum|t_i| with sum|t_i| from the reference.  Derived, not tuned."""
import ctypes as C

import numpy as np
import pytest
import torch

import measure_ref
from gpu_common import detector

pytestmark = pytest.mark.gpu

N = 2048
EXACT = (0, 1, 2, 3, 4, 5, 6, 11)         # npix nring bkg rms peak x_peak y_peak reserved
SUMS = (7, 8, 9, 10)                      # sum sw swx swy


@pytest.fixture(scope="module")
def scene():
    from caesar_yolo_amd import synth
    img = synth.make_mosaic(n=N, seed=7)                  # NaN strip: columns 1984..2047; zero block: [1024, 1536) x [1024, 1536)
    img[300:303, 400:405] = np.float32(0.25)              # peak tie: 15 equal pixels above everything around
    img[310, 420] = img[312, 418] = np.float32(0.5)       # peak tie across rows: (418, 312) comes after (420, 310)
    img[600:640, 700:740] = np.float32(0.125)             # a constant patch: constant ring (rms == 0), no pixel above bkg (sw == 0)
    img[1200:1203, 1100:1103] = np.float32(0.75)          # an island inside the zero block: its ring is blank
    img[800, 800] = np.float32(-1.0)                      # a pixel below everything around it
    holes = np.random.default_rng(3).integers(0, N, (40000, 2))      # isolated blank pixels (about 1 %) in the rows from 1040 on
    holes = holes[holes[:, 0] >= 1040]
    img[holes[:, 0], holes[:, 1]] = 0.0
    img[1005, 30] = 0.0                                   # ... and this one: makes the count of the "odd ring" case odd
    host = np.where(np.isfinite(img), img, np.float32(0)).astype(np.float32)     # what cy_mosaic_prepare leaves
    det = detector("fp32", max_batch=1, max_imgsz=160)
    dev = det.mosaic_to_device(img)
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), host)
    return det, dev, host


def constructed_boxes():
    b = {
        "one pixel": [50.0, 60.0, 50.0, 60.0],
        "fractional edges": [100.3, 200.7, 131.9, 222.1],
        "fractional, no pixel centre in x": [100.2, 200.0, 100.8, 210.0],
        "left border": [0.0, 500.0, 12.0, 520.0],
        "top border": [500.0, 0.0, 520.0, 9.0],
        "bottom border": [500.0, N - 10.0, 530.0, N - 1.0],
        "right border (inside the NaN strip)": [N - 20.0, 700.0, N - 1.0, 720.0],
        "corner 00": [0.0, 0.0, 6.0, 6.0],
        "corner 0N": [0.0, N - 7.0, 6.0, N - 1.0],
        "corner N0 (NaN strip)": [N - 7.0, 0.0, N - 1.0, 6.0],
        "corner NN (NaN strip)": [N - 7.0, N - 7.0, N - 1.0, N - 1.0],
        "partly outside, left top": [-15.5, -7.25, 9.5, 11.0],
        "partly outside, right bottom": [N - 90.0, N - 12.0, N + 40.0, N + 30.0],
        "wholly outside, left": [-50.0, 100.0, -20.0, 130.0],
        "wholly outside, beyond the corner": [N + 5.0, N + 5.0, N + 50.0, N + 60.0],
        "wholly outside, far": [-1e12, -1e12, -1e11, -1e11],
        "inside the zero block": [1300.0, 1300.0, 1330.0, 1320.0],
        "island in the zero block (blank ring)": [1100.0, 1200.0, 1102.0, 1202.0],
        "across the NaN strip": [1960.0, 900.0, 2010.0, 930.0],
        "across the zero block's edge": [1000.0, 1000.0, 1060.0, 1050.0],
        "nothing above bkg": [800.0, 800.0, 800.0, 800.0],
        "constant ring and box": [715.0, 615.0, 722.0, 622.0],
        "peak tie in one block": [395.0, 295.0, 410.0, 306.0],
        "peak tie across rows": [410.0, 305.0, 425.0, 315.0],
        "even ring": [900.0, 900.0, 909.0, 909.0],           # ring 8: 26^2 - 10^2 = 576 pixels, all valid noise
        "odd ring": [35.0, 1000.0, 45.0, 1010.0],           # ring 8: 27^2 - 11^2 - the blank pixel at (30, 1005) = 607
        "large window": [200.5, 300.5, 1700.0, 1500.0],      # about 1500 x 1200, spans the zero block
        "whole image": [-3.0, -3.0, N + 3.0, N + 3.0],
    }
    return b


def compare(got, ref, mags, what):
    assert got.shape == ref.shape
    for i in range(ref.shape[0]):
        for f in EXACT:
            assert got[i, f] == ref[i, f], "%s, box %d: %s = %r on the GPU, %r in the reference" % (
                what, i, measure_ref.FIELDS[f], got[i, f], ref[i, f])
        m = ref[i, 0]                                      # terms of the sums = valid pixels of the box window
        for f, mag in zip(SUMS, mags[i]):
            bound = 2.0 * m * 2.0 ** -53 * mag
            assert abs(got[i, f] - ref[i, f]) <= bound, "%s, box %d: %s = %r on the GPU, %r in the reference, |diff| %g > bound %g (m = %d)" % (
                what, i, measure_ref.FIELDS[f], got[i, f], ref[i, f], abs(got[i, f] - ref[i, f]), bound, m)


@pytest.mark.parametrize("ring", [0, 1, 8, 64])
def test_constructed_boxes(scene, ring):
    det, dev, host = scene
    named = constructed_boxes()
    boxes = np.array(list(named.values()), np.float64)
    ref, mags = measure_ref.measure(host, boxes, ring)
    got = det.measure_sources(dev, boxes, ring=ring)
    r = {k: dict(zip(measure_ref.FIELDS, ref[i])) for i, k in enumerate(named)}
    # the cases are what their names say (on the reference side, so that a wrong construction fails here and not silently)
    assert r["one pixel"]["npix"] == 1
    assert r["fractional, no pixel centre in x"]["npix"] == 0 and r["fractional, no pixel centre in x"]["nring"] == 0
    for k in named:
        if k.startswith("wholly outside"):
            assert r[k]["npix"] == 0 and r[k]["nring"] == 0 and r[k]["x_peak"] == -1
    assert r["inside the zero block"]["npix"] == 0 and r["inside the zero block"]["x_peak"] == -1
    assert r["island in the zero block (blank ring)"]["npix"] == 9 and r["island in the zero block (blank ring)"]["nring"] == 0
    assert r["right border (inside the NaN strip)"]["npix"] == 0
    assert 0 < r["across the NaN strip"]["npix"] < 51 * 31
    assert r["peak tie in one block"]["peak"] == 0.25 and (r["peak tie in one block"]["x_peak"], r["peak tie in one block"]["y_peak"]) == (400, 300)
    assert r["peak tie across rows"]["peak"] == 0.5 and (r["peak tie across rows"]["x_peak"], r["peak tie across rows"]["y_peak"]) == (420, 310)
    assert r["large window"]["npix"] > 1500000
    assert r["nothing above bkg"]["npix"] == 1 and r["nothing above bkg"]["sw"] == 0.0 and r["nothing above bkg"]["sum"] < 0
    if ring in (1, 8):
        assert r["constant ring and box"]["rms"] == 0.0 and r["constant ring and box"]["bkg"] == 0.125
        assert r["constant ring and box"]["sw"] == 0.0 and r["constant ring and box"]["npix"] == 64
    if ring == 8:
        assert r["even ring"]["nring"] == 576 and r["odd ring"]["nring"] == 607
    if ring == 0:
        assert all(v["nring"] == 0 and v["bkg"] == 0.0 and v["rms"] == 0.0 for v in r.values())
    compare(got, ref, mags, "ring %d" % ring)
    print("ring %d: %d constructed boxes equal; kernel %.3f ms" % (ring, len(named), det.measure_kernel_ms()))


def test_random_boxes(scene):
    det, dev, host = scene
    rng = np.random.default_rng(20261016)
    n = 2000
    w, h = rng.integers(3, 201, n), rng.integers(3, 201, n)
    x1, y1 = rng.uniform(-40, N + 20, n), rng.uniform(-40, N + 20, n)
    frac = rng.random(n) < 0.5                                  # half of them with integer edges, as catalog boxes have
    x1, y1 = np.where(frac, x1, np.floor(x1)), np.where(frac, y1, np.floor(y1))
    boxes = np.stack([x1, y1, x1 + w, y1 + h], 1)
    ref, mags = measure_ref.measure(host, boxes, 8)
    got = det.measure_sources(dev, boxes, ring=8)
    assert (ref[:, 0] > 0).sum() > 1500 and (ref[:, 1] % 2 == 1).sum() > 100 and (ref[:, 1] % 2 == 0).sum() > 100
    compare(got, ref, mags, "random")
    worst = max(abs(got[i, f] - ref[i, f]) / (2.0 * ref[i, 0] * 2.0 ** -53 * mags[i, j]) for i in range(n) if ref[i, 0] > 0
                for j, f in enumerate(SUMS) if mags[i, j] > 0)
    print("2000 random boxes: exact fields equal, largest |diff| / bound of the sums %.3g; kernel %.3f ms" % (worst, det.measure_kernel_ms()))


def test_arguments_and_determinism(scene):
    det, dev, host = scene
    from caesar_yolo_amd import lib as L
    lib = L.load()
    dp = C.POINTER(C.c_double)
    boxes = np.array(list(constructed_boxes().values()), np.float64)
    out = np.zeros((boxes.shape[0], L.CY_MEAS_FIELDS), np.float64)
    args = lambda n=boxes.shape[0], ring=8, img=dev.data_ptr(), mh=N, mw=N, b=boxes.ctypes.data_as(dp), o=out.ctypes.data_as(dp), ctx=det.ctx: (
        ctx, C.c_void_p(img), mh, mw, b, n, ring, o, det._stream())
    assert det.measure_sources(dev, np.zeros((0, 4)), ring=8).shape == (0, L.CY_MEAS_FIELDS)
    assert lib.cy_measure_sources(*args(n=0)) == 0                               # CY_OK, nothing launched
    assert lib.cy_measure_sources(*args(ring=-1)) == -1                          # CY_ERR_ARG
    assert lib.cy_measure_sources(*args(mh=0)) == -1 and lib.cy_measure_sources(*args(mw=-5)) == -1
    assert lib.cy_measure_sources(*args(img=None)) == -1
    assert lib.cy_measure_sources(*args(b=None)) == -1 and lib.cy_measure_sources(*args(o=None)) == -1
    assert lib.cy_measure_sources(*args(ctx=None)) == -1
    assert lib.cy_measure_sources(*args(n=-3)) == -1
    with pytest.raises(L.CyError):
        det.measure_sources(dev, boxes, ring=-2)
    a = det.measure_sources(dev, boxes, ring=8)
    b = det.measure_sources(dev, boxes, ring=8)
    assert a.tobytes() == b.tobytes()                                            # run-to-run: the same bytes
    assert det.measure_kernel_ms() > 0
