"""Background mesh without a GPU: the numpy reference (tests/bkg_ref.py) against hand-computed cells, measure.sample_mesh against
scipy's linear interpolation and at its clamped borders, measure.fill_mesh on constructed masks, the host-side annotation, the
exported symbols, the CLI flags, and a statistical sanity check of the estimator itself."""
import math
import os
import sys
from statistics import NormalDist

import numpy as np
import pytest

import bkg_ref
from caesar_yolo_amd import lib as L
from caesar_yolo_amd import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def row(px, k, niter):
    return dict(zip(bkg_ref.FIELDS, bkg_ref.cell_stats(np.array(px, np.float32), k, niter)))


def test_reference_two_valid_pixels():
    r = row([[1.0, 0.0], [float("nan"), 3.0]], 3.0, 3)
    # med = (1 + 3) / 2, both deviations 1: sig = 1.4826; the clip at 2 +- 3 * 1.4826 keeps both
    assert r == dict(n0=2, n=2, bkg=2.0, rms=1.4826, L=2.0 - 3.0 * 1.4826, H=2.0 + 3.0 * 1.4826, rounds=0, reserved=0)
    r = row([[1.0, 0.0], [float("nan"), 3.0]], 0.5, 3)
    # k = 0.5: the interval 2 +- 0.7413 holds neither; the empty set is not clipped again
    assert r == dict(n0=2, n=0, bkg=0.0, rms=0.0, L=2.0 - 0.5 * 1.4826, H=2.0 + 0.5 * 1.4826, rounds=1, reserved=0)


def test_reference_constant_majority_with_outliers():
    px = [5.0] * 10 + [100.0, -50.0, 7.0]
    for niter in (1, 3):
        r = row(px, 3.0, niter)
        # median 5, more than half of the deviations are 0: sig == 0 keeps exactly the pixels equal to the median
        assert r == dict(n0=13, n=10, bkg=5.0, rms=0.0, L=5.0, H=5.0, rounds=1, reserved=0)
    assert px.count(5.0) == 10


def test_reference_all_blank_cell():
    for niter in (0, 3):
        r = row([[0.0, float("nan")], [float("inf"), -0.0], [float("-inf"), 0.0]], 3.0, niter)
        assert r == dict(n0=0, n=0, bkg=0.0, rms=0.0, L=-INF, H=INF, rounds=0, reserved=0)


def test_reference_one_bright_pixel_and_niter_zero():
    px = [1, 2, 3, 4, 5, 6, 7, 8, 1000]
    # median 5; deviations 0 1 1 2 2 3 3 4 995: MAD 2
    sig = 1.4826 * 2.0
    assert row(px, 3.0, 0) == dict(n0=9, n=9, bkg=5.0, rms=sig, L=-INF, H=INF, rounds=0, reserved=0)
    # the clip at 5 +- 3 sig = [-3.8956, 13.8956] removes the 1000; the eight left: median (4 + 5) / 2, deviations .5 .5 1.5 1.5 2.5
    # 2.5 3.5 3.5: MAD (1.5 + 2.5) / 2 = 2 again
    L1, H1 = 5.0 - 3.0 * sig, 5.0 + 3.0 * sig
    assert L1 < 1 and 8 < H1 < 1000
    assert row(px, 3.0, 1) == dict(n0=9, n=8, bkg=4.5, rms=sig, L=L1, H=H1, rounds=1, reserved=0)
    # the second clip, 4.5 +- 3 sig, lowers H and not L and removes nothing: a fixed point, every later clip is the same
    for niter in (2, 3, 32):
        assert row(px, 3.0, niter) == dict(n0=9, n=8, bkg=4.5, rms=sig, L=L1, H=4.5 + 3.0 * sig, rounds=1, reserved=0)


def test_reference_mesh_layout_and_partial_cells():
    img = np.arange(1, 10 * 13 + 1, dtype=np.float32).reshape(10, 13)
    out = bkg_ref.background(img, 4, 3.0, 0)
    assert out.shape == (3, 4, 8)
    assert out[:, :, 0].tolist() == [[16, 16, 16, 4], [16, 16, 16, 4], [8, 8, 8, 2]]
    assert out[2, 3, 2] == (img[8, 12] + img[9, 12]) / 2 and out[0, 0, 2] == np.median(img[:4, :4])


def test_sample_mesh_against_scipy_at_interior_points():
    """Against scipy's RegularGridInterpolator (linear) on the grid of the cell centres, at points between the outermost centres.
    Tolerance, with eps = 2^-52 and M the largest |mesh value|: each side forms the value with at most five roundings in a row
    (weight, product, three sums) of quantities <= M, so the two differ by at most 2 * 5 * (eps / 2) * M = 5 eps M: 8 eps M asked,
    a few ulp of M.  That is all when the coordinates are exact: a power-of-two cell and positions on a 1/16 grid make
    (x - centre) / cell exact on both sides.  For any other cell, t = (x - c) / cell carries two roundings, |dt| <= eps * t <= eps * nc
    per axis and side, and the value moves by at most 2 M per unit of a fraction: 2 sides * 2 M * eps * (ncx + ncy) more."""
    from scipy.interpolate import RegularGridInterpolator
    rng = np.random.default_rng(1)
    eps = np.finfo(np.float64).eps
    for cell, ncy, ncx in ((128, 16, 16), (64, 5, 33), (8, 40, 3), (100, 21, 5), (7, 3, 40)):
        mesh = rng.normal(0.0, 1.0, (ncy, ncx))
        yc, xc = np.arange(ncy) * cell + (cell - 1) / 2.0, np.arange(ncx) * cell + (cell - 1) / 2.0
        f = RegularGridInterpolator((yc, xc), mesh, method="linear")
        x, y = rng.uniform(xc[0], xc[-1], 5000), rng.uniform(yc[0], yc[-1], 5000)
        exact = cell & (cell - 1) == 0
        if exact:
            x, y = np.clip(np.round(x * 16) / 16, xc[0], xc[-1]), np.clip(np.round(y * 16) / 16, yc[0], yc[-1])
        x[:ncx], y[:ncx] = xc, yc[rng.integers(0, ncy, ncx)]                       # the centres themselves
        got = measure.sample_mesh(mesh, cell, x, y)
        tol = eps * np.abs(mesh).max() * (8 if exact else 8 + 4 * (ncx + ncy))
        err = np.abs(got - f(np.stack([y, x], 1))).max()
        print("cell %d, %d x %d: largest |diff| %.3g, tolerance %.3g" % (cell, ncy, ncx, err, tol))
        assert err <= tol
        assert np.array_equal(got[:ncx], mesh[np.round((y[:ncx] - yc[0]) / cell).astype(int), np.arange(ncx)])     # a centre returns its cell


def test_sample_mesh_borders_shapes_and_planes():
    mesh = np.array([[1.0, 2.0, 4.0], [10.0, 20.0, 40.0]])
    cell = 10                                                                      # centres x 4.5 14.5 24.5, y 4.5 14.5
    s = lambda x, y: measure.sample_mesh(mesh, cell, x, y)
    # constant outside the outermost centres, in both axes and at the corners
    assert s(-100.0, -100.0) == 1.0 and s(0.0, 0.0) == 1.0 and s(4.5, 4.5) == 1.0
    assert s(29.0, 0.0) == 4.0 and s(1e9, 4.5) == 4.0 and s(24.5, 19.0) == 40.0 and s(0.0, 1e9) == 10.0 and s(99.0, 99.0) == 40.0
    assert s(9.5, 0.0) == 1.5 and s(19.5, 4.5) == 3.0 and s(4.5, 9.5) == 5.5 and s(0.0, 9.5) == 5.5
    assert s(9.5, 9.5) == (1.5 * 0.5 + 15.0 * 0.5)
    # the last centre uses the last pair of cells with fraction 1
    assert s(24.5, 14.5) == 40.0 and s(24.5, 4.5) == 4.0
    # arrays of any one shape; planes are interpolated independently
    x, y = np.meshgrid(np.arange(30.0), np.arange(20.0))
    both = measure.sample_mesh(np.stack([mesh, -2.0 * mesh], 2), cell, x, y)
    assert both.shape == (20, 30, 2) and np.array_equal(both[:, :, 0], s(x, y)) and np.array_equal(both[:, :, 1], -2.0 * s(x, y))
    # one row / one column / one cell
    assert np.array_equal(measure.sample_mesh(mesh[:1], cell, x, y), measure.sample_mesh(mesh[:1], cell, x, np.zeros_like(y)))
    assert np.array_equal(measure.sample_mesh(mesh[:, :1], cell, x, y), measure.sample_mesh(mesh[:, :1], cell, np.zeros_like(x), y))
    assert np.all(measure.sample_mesh(mesh[:1, :1], cell, x, y) == 1.0)


def _raw(n, bkg, rms):
    raw = np.zeros(np.shape(n) + (8,), np.float64)
    raw[..., 0] = raw[..., 1] = n
    raw[..., 2], raw[..., 3] = bkg, rms
    return raw


def test_fill_mesh():
    # a tie along a row: the middle cell is one step from both neighbours -> the smaller row-major index
    mesh, nd = measure.fill_mesh(_raw([[64, 63, 64]], [[1.0, 9.0, 3.0]], [[0.1, 0.9, 0.3]]), 64)
    assert nd == 2 and mesh[:, :, 0].tolist() == [[1.0, 1.0, 3.0]] and mesh[:, :, 1].tolist() == [[0.1, 0.1, 0.3]]
    # a tie across rows: (0, 1) and (1, 0) are both one step from (0, 0) and from (1, 1); (0, 1) has the smaller index
    mesh, nd = measure.fill_mesh(_raw([[0, 100], [100, 0]], [[7.0, 1.0], [2.0, 7.0]], [[7.0, 0.1], [0.2, 7.0]]), 64)
    assert nd == 2 and mesh[:, :, 0].tolist() == [[1.0, 1.0], [2.0, 1.0]] and mesh[:, :, 1].tolist() == [[0.1, 0.1], [0.2, 0.1]]
    # the nearer one wins over the smaller index: squared distances 1 + 0 against 0 + 4
    n = np.zeros((3, 3)); n[0, 0] = n[2, 2] = 64
    b = np.zeros((3, 3)); b[0, 0], b[2, 2] = 1.0, 2.0
    mesh, nd = measure.fill_mesh(_raw(n, b, b), 64)
    assert mesh[:, :, 0].tolist() == [[1.0, 1.0, 1.0], [1.0, 1.0, 2.0], [1.0, 2.0, 2.0]]
    # a single defined cell fills the mesh
    n = np.zeros((4, 5)); n[2, 3] = 1000
    mesh, nd = measure.fill_mesh(_raw(n, np.full((4, 5), 3.5), np.full((4, 5), 0.25)) * (n[..., None] > 0), 64)
    assert nd == 1 and np.all(mesh[:, :, 0] == 3.5) and np.all(mesh[:, :, 1] == 0.25)
    # none: zeros, and the caller is told
    mesh, nd = measure.fill_mesh(_raw(np.full((2, 2), 63), np.ones((2, 2)), np.ones((2, 2))), 64)
    assert nd == 0 and not mesh.any() and mesh.shape == (2, 2, 2)
    # the count that matters is n (after the clips), not n0; min_pix is honoured
    raw = _raw([[100, 100]], [[1.0, 2.0]], [[1.0, 2.0]]); raw[0, 1, 1] = 10
    assert measure.fill_mesh(raw, 64)[0][:, :, 0].tolist() == [[1.0, 1.0]] and measure.fill_mesh(raw, 10)[0][:, :, 0].tolist() == [[1.0, 2.0]]


def test_annotate_background_and_thresholds():
    mesh = np.zeros((2, 3, 2)); mesh[:, :, 0] = [[1.0, 2.0, 4.0], [10.0, 20.0, 40.0]]; mesh[:, :, 1] = 0.5
    mesh[0, 2, 1] = 0.0
    src = [dict(x1=100.0, y1=50.0, x2=110.0, y2=60.0, npix=5, x_peak=109, y_peak=54, peak=3.0, bkg=0.1, rms=0.2),      # origin (100, 50)
           dict(x1=100.0, y1=50.0, x2=119.0, y2=69.0, npix=0, x_peak=-1, y_peak=-1, peak=0.0, bkg=0.0, rms=0.0),
           dict(x1=120.0, y1=50.0, x2=129.0, y2=51.0, npix=3, x_peak=129, y_peak=50, peak=9.0, bkg=0.0, rms=0.0)]
    measure.annotate_background(src, mesh, 10, origin=(100, 50))
    assert src[0]["bkg_map"] == measure.sample_mesh(mesh[:, :, 0], 10, 9.0, 4.0) == 1.0 * (1.0 - 0.45) + 2.0 * 0.45 and src[0]["rms_map"] == 0.5
    assert src[0]["snr_map"] == (3.0 - src[0]["bkg_map"]) / 0.5 and abs(src[0]["bkg_map"] - 1.45) < 1e-15 and src[0]["bkg"] == 0.1 and src[0]["rms"] == 0.2       # the ring values stay
    assert src[1]["bkg_map"] == measure.sample_mesh(mesh[:, :, 0], 10, 9.5, 9.5) and src[1]["snr_map"] == (0.0 - src[1]["bkg_map"]) / 0.5
    assert src[2]["bkg_map"] == 4.0 and src[2]["rms_map"] == 0.0 and src[2]["snr_map"] == 0.0
    assert set(src[0]) - {"x1", "y1", "x2", "y2", "npix", "x_peak", "y_peak", "peak", "bkg", "rms"} == set(measure.BKG_KEYS)
    ring, mp = measure.island_thresholds(src, 5.0, 2.5), measure.island_thresholds(src, 5.0, 2.5, use_map=True)
    assert ring[0].tolist() == [0.1 + 5.0 * 0.2, 0.1 + 2.5 * 0.2, 0.1] and mp[0].tolist() == [src[0]["bkg_map"] + 5.0 * 0.5, src[0]["bkg_map"] + 2.5 * 0.5, src[0]["bkg_map"]]
    assert measure.annotate_background([], mesh, 10) == []


def test_exports_and_python_surface():
    for name in ("cy_measure_background", "cy_background_kernel_ms", "cy_expand_background"):
        assert name in L.EXPORTS and hasattr(L.load(), name)
    assert L.CY_BKG_FIELDS == len(L.BKG_NAMES) == len(bkg_ref.FIELDS) == 8 and tuple(L.BKG_NAMES) == tuple(bkg_ref.FIELDS)
    from caesar_yolo_amd.model import HipDetector
    assert callable(HipDetector.measure_background) and callable(HipDetector.expand_background) and callable(HipDetector.background_kernel_ms)
    hdr = open(os.path.join(ROOT, "include", "caesar_yolo_hip.h")).read()
    assert "#define CY_BKG_FIELDS 8" in hdr
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    assert "cy_background.hip" in G.HIP_SOURCES and os.path.isfile(os.path.join(G.CSRC, "cy_background.hip"))
    assert not set(measure.BKG_KEYS) & (set(measure.KEYS) | set(measure.ISLAND_KEYS))


def test_cli_flags():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import run
    a = run.parse_args(["--weights=seeded:l:5"])
    assert (a.bkg_map, a.save_bkg_maps, a.bkg_cell, a.bkg_clip_sigma, a.bkg_clip_iters, a.bkg_min_pix) == (False, False, 128, 3.0, 3, 64)
    a = run.parse_args(["--weights=seeded:l:5", "--bkg_map", "--bkg_cell", "64", "--bkg_clip_sigma=2.5", "--bkg_clip_iters", "10", "--bkg_min_pix=16",
                        "--save_bkg_maps"])
    assert (a.bkg_map, a.save_bkg_maps, a.bkg_cell, a.bkg_clip_sigma, a.bkg_clip_iters, a.bkg_min_pix) == (True, True, 64, 2.5, 10, 16)
    fits = os.path.join(ROOT, "tests", "golden", "galaxy0001.fits")
    base = ["--weights=seeded:l:5", "--image=" + fits]
    assert run.validate_args(run.parse_args(base + ["--bkg_map"])) == 0
    assert run.validate_args(run.parse_args(base + ["--bkg_map", "--bkg_cell=4", "--bkg_clip_iters=0"])) == 0
    assert run.validate_args(run.parse_args(base + ["--bkg_map", "--bkg_cell=4096", "--bkg_clip_iters=32"])) == 0
    for bad in (["--bkg_cell=3"], ["--bkg_cell=4097"], ["--bkg_clip_sigma=0"], ["--bkg_clip_sigma=-1"], ["--bkg_clip_sigma=nan"],
                ["--bkg_clip_iters=-1"], ["--bkg_clip_iters=33"], ["--bkg_min_pix=0"]):
        assert run.validate_args(run.parse_args(base + ["--bkg_map"] + bad)) == -1, bad
    from caesar_yolo_amd.config import CONFIG
    assert CONFIG["bkg_map"] is False and CONFIG["save_bkg_maps"] is False
    assert (CONFIG["bkg_cell"], CONFIG["bkg_clip_sigma"], CONFIG["bkg_clip_iters"], CONFIG["bkg_min_pix"]) == (128, 3.0, 3, 64)
    assert measure.background_config({}) == (128, 3.0, 3, 64)
    assert measure.background_config(dict(bkg_cell=64, bkg_clip_sigma=2.5, bkg_clip_iters=1, bkg_min_pix=8)) == (64, 2.5, 1, 8)
    doc = run.__doc__
    assert "--bkg_map" in doc and "--save_bkg_maps" in doc
    assert "--bkg_map" in open(os.path.join(ROOT, "README.md")).read()


def clipped_sigma_factor(k, niter):
    """E[rms] / sigma of the estimator on normal noise, large n: s_0 = 1 (1.4826 = 1 / Phi^-1(3/4)); clip j keeps |x| <= c = k s_j
    sigma, and the median m of |x| of a normal truncated at c solves 2 Phi(m) - 1 = (2 Phi(c) - 1) / 2; s_{j+1} = 1.4826 m."""
    nd, s = NormalDist(), 1.4826 * NormalDist().inv_cdf(0.75)
    c = float("inf")
    for _ in range(niter):
        c = min(c, k * s)
        s = 1.4826 * nd.inv_cdf(0.5 + (2.0 * nd.cdf(c) - 1.0) / 4.0)
    return s


@pytest.mark.parametrize("k,niter", [(3.0, 0), (3.0, 3), (2.5, 3), (3.0, 10)])
def test_mesh_rms_recovers_a_stamped_sigma(k, niter):
    """Pure normal noise of standard deviation SIGMA (fp32 pixels, no sources): the rms of a full cell is the MAD-based sigma of
    n = cell^2 pixels.  The sample median of |x - med| at the quartile point q = Phi^-1(3/4) = 0.6745 of a density
    f(q) = 2 phi(q) = 0.6356 has the standard error 1 / (2 f(q) sqrt(n)) = 0.7867 / sqrt(n); times 1.4826: SE = 1.1664 sigma /
    sqrt(n).  Clipping at k moves the expectation to clipped_sigma_factor(k, niter) * sigma (0.99685 for k = 3 after one clip,
    0.99675 from the third on; 0.98556 and 0.98386 for k = 2.5), computed from the normal distribution above; the clipped sample is
    smaller by the factor 2 Phi(c) - 1 >= 0.98, which the sqrt(n) below takes from the cell's own n.  Margin: 5 SE for each of the
    256 cells (probability of a false alarm about 256 * 6e-7), and 5 SE / sqrt(256) for their mean; the O(1 / n) bias of a sample
    median and the fp32 rounding of the pixels are two orders of magnitude below that.  Not tuned."""
    SIGMA, cell, n_img = 3.0e-4, 128, 2048
    img = (np.random.default_rng(2026).standard_normal((n_img, n_img)) * SIGMA).astype(np.float32)
    out = bkg_ref.background(img, cell, k, niter)
    n, rms, bkg = out[:, :, 1], out[:, :, 3], out[:, :, 2]
    assert np.all(out[:, :, 0] == cell * cell)
    want = clipped_sigma_factor(k, niter) * SIGMA
    assert 0.98 < want / SIGMA <= 1.0 + 1e-4 and (niter == 0) == (abs(want / SIGMA - 1.0) < 1e-4)
    se = 1.1664 * SIGMA / np.sqrt(n)
    assert np.all(np.abs(rms - want) <= 5.0 * se), np.abs((rms - want) / se).max()
    assert abs(rms.mean() - want) <= 5.0 * se.mean() / math.sqrt(rms.size), (rms.mean() - want) / (se.mean() / math.sqrt(rms.size))
    # the median of n normal pixels: standard error sqrt(pi / 2) sigma / sqrt(n)
    assert np.all(np.abs(bkg) <= 5.0 * math.sqrt(math.pi / 2.0) * SIGMA / np.sqrt(n))
    print("k %g niter %d: factor %.5f, largest |rms - want| / SE %.2f, mean off by %.2f SE of the mean" % (
        k, niter, want / SIGMA, np.abs((rms - want) / se).max(), (rms.mean() - want) / (se.mean() / math.sqrt(rms.size))))
