"""The reference of the component fits (tests/fit_ref.py) against truth and against scipy, the host helpers of
caesar_yolo_amd/measure.py, the command line's handling of --fit_components, the library's exports, and the measurement of the
tolerance the GPU tests use.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

import fit_cases
import fit_ref
from caesar_yolo_amd import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _job(img, c, i, k=0):
    x0, y0, h, w = measure.box_window(c.boxes[i], *img.shape)
    yy, xx = np.nonzero(c.masks[i].reshape(h, w) == k + 1)
    v = img[y0:y0 + h, x0:x0 + w][yy, xx]
    ok = (v != 0) & np.isfinite(v)
    return x0, y0, xx[ok].astype(np.float64), yy[ok].astype(np.float64), v[ok].astype(np.float64) - c.bkg[i]


def _jac(p, dx, dy):
    A, x0, y0, a, b, c = p
    u, v = dx - x0, dy - y0
    e = np.exp(-0.5 * (a * u * u + 2 * b * u * v + c * v * v))
    m = A * e
    return m, np.stack([e, m * (a * u + b * v), m * (b * u + c * v), -0.5 * m * u * u, -m * u * v, -0.5 * m * v * v], 1)


# ---- 1. against truth
def test_reference_against_truth():
    """Noiseless float32 stamps: the data are the model rounded to fp32, |delta_i| <= 2^-24 |y_i|, so to first order the
    least-squares solution moves by at most sum_i |(H^-1 J^T)_ji| 2^-24 |y_i| in parameter j; twice that is allowed (second
    order, and the convergence criterion)."""
    img, c, res, _, _ = fit_cases.drawn_reference()
    assert len(c.truth) == 5
    for i, tp in c.truth.items():
        row = res[0][i, 0]
        assert row[0] == 0 and row[2] == 441
        x0, y0, dx, dy, y = _job(img, c, i)
        rel = tp.copy()
        rel[1] -= x0
        rel[2] -= y0
        m, J = _jac(rel, dx, dy)
        bound = 2.0 * (np.abs(np.linalg.solve(J.T @ J, J.T)) @ (2.0 ** -24 * np.abs(m)))
        assert np.all(np.abs(row[5:11] - tp) <= bound + 1e-12), (c.names[i], np.abs(row[5:11] - tp), bound)


# ---- 2. against scipy
def test_reference_against_scipy():
    """Noisy stamps: both minimise the same sum of squares.  scipy stops at xtol = ftol = gtol = 1e-15; the two minima agree to the
    square root of the reference's own criterion (F flat to 1e-14 F around the minimum: parameters to 1e-7 relative of their
    scale), taken against the Gauss-Newton scale sqrt(diag(H^-1) F)."""
    so = pytest.importorskip("scipy.optimize")
    img, c, res, _, _ = fit_cases.drawn_reference()
    names = [nm for nm in c.names if nm.startswith("noisy_")] + ["blend2", "invalid_inside"]
    done = 0
    for nm in names:
        i = c.names.index(nm)
        for k in range(c.ncomp[i]):
            row = res[0][i, k]
            assert row[0] == 0
            x0, y0, dx, dy, y = _job(img, c, i, k)
            p0 = c.start[i][k].copy()
            p0[1] -= x0
            p0[2] -= y0
            sol = so.least_squares(lambda p: _jac(p, dx, dy)[0] - y, p0, jac=lambda p: _jac(p, dx, dy)[1] * [1, 1, 1, 1, 1, 1],
                                   method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
            got = row[5:11].copy()
            got[1] -= x0
            got[2] -= y0
            _, J = _jac(sol.x, dx, dy)
            scale = np.sqrt(np.diag(np.linalg.inv(J.T @ J)) * max(2.0 * sol.cost, 1e-30))
            assert np.all(np.abs(got - sol.x) <= 1e-7 * (np.abs(sol.x) + scale) + 1e-12), (nm, k, got, sol.x)
            assert abs(row[3] - 2.0 * sol.cost) <= 1e-10 * row[3]
            done += 1
    assert done == 8


# ---- 3. host helpers
def test_gaussian_shape_against_eigen():
    rng = np.random.default_rng(3)
    for _ in range(200):
        s1, s2, th = rng.uniform(1.0, 5.0), rng.uniform(0.5, 1.0), rng.uniform(-np.pi / 2, np.pi / 2)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        P = np.linalg.inv(R @ np.diag([s1 * s1, s2 * s2]) @ R.T)
        major, minor, pa = measure.gaussian_shape(P[0, 0], P[0, 1], P[1, 1])
        w, V = np.linalg.eigh(np.linalg.inv(P))
        assert abs(major - measure.FWHM * math.sqrt(w[1])) <= 1e-9 * major and abs(minor - measure.FWHM * math.sqrt(w[0])) <= 1e-9 * minor
        ang = math.degrees(math.atan2(V[1, 1], V[0, 1]))
        assert min(abs((pa - ang + 90.0) % 180.0 - 90.0), 180.0) <= 1e-6 and -90.0 < pa <= 90.0
    assert measure.gaussian_shape(0.25, 0.0, 0.25) == (measure.FWHM * 2.0, measure.FWHM * 2.0, 0.0)
    # the pa convention of island_shape: the moments of the same Gaussian give the same angle
    P = np.linalg.inv(np.array([[4.0, 1.5], [1.5, 2.0]]))
    assert abs(measure.gaussian_shape(P[0, 0], P[0, 1], P[1, 1])[2] - measure.island_shape(1.0, 0.0, 0.0, 4.0, 2.0, 1.5)[2]) <= 1e-9


def test_fit_start_floors_and_fallbacks():
    row = np.zeros(12)
    row[:] = [50, 10.5, 15, 26, 100, 500, 600, 2600 + 400, 3700 + 100, 3050 + 100, 1, 1]       # cxx = 4 + 1, cyy = 1 + 1, cxy = 1 + 0.5...
    S, Sx, Sy, Sxx, Syy, Sxy = row[4:10]
    s = measure.fit_start(row, 0.5, (10, 20))
    cov = np.array([[Sxx / S - 25, Sxy / S - 30], [Sxy / S - 30, Syy / S - 36]])
    P = np.linalg.inv(cov)
    assert np.allclose(s, [10.0, 15.0, 26.0, P[0, 0], P[0, 1], P[1, 1]], rtol=1e-12, atol=1e-12)
    thin = row.copy()
    thin[7:10] = [S * (25 + 4.0), S * (36 + 0.01), S * 30]     # variance 0.01 px^2 in y: floored at 0.25
    s = measure.fit_start(thin, 0.0, (0, 0))
    assert np.allclose(s[3:], [0.25, 0.0, 4.0], rtol=1e-12, atol=1e-12)
    point = row.copy()
    point[7:10] = [S * 25, S * 36, S * 30]                     # a single pixel: both eigenvalues floored
    assert np.allclose(measure.fit_start(point, 0.0, (0, 0))[3:], [4.0, 0.0, 4.0], atol=1e-12)
    for bad in (0.0, -3.0, np.nan, np.inf):
        r = row.copy()
        r[4] = bad
        assert measure.fit_start(r, 0.5, (10, 20)).tolist() == [10.0, 15.0, 26.0, 1.0, 0.0, 1.0]
    r = row.copy()
    r[7] = np.nan
    assert measure.fit_start(r, 0.5, (10, 20)).tolist() == [10.0, 15.0, 26.0, 1.0, 0.0, 1.0]
    # leading axes broadcast: [n, 16, 12] rows with bkg [n] and win0 [n, 2]
    many = np.zeros((3, 16, 12))
    many[1, 2] = row
    out = measure.fit_start(many, np.array([0.0, 0.5, 0.0]), np.array([[0, 0], [10, 20], [1, 1]]))
    assert out.shape == (3, 16, 6) and np.array_equal(out[1, 2], measure.fit_start(row, 0.5, (10, 20)))
    assert out[0, 0].tolist() == [0.0, 0.0, 0.0, 1.0, 0.0, 1.0]


def _hand_rows():
    fit = np.zeros((2, 16, 32))
    p = [8.0, 30.5, 40.25, 0.3, 0.05, 0.2]
    _, J = _jac(np.array(p), np.arange(25.0, 36.0).repeat(11), np.tile(np.arange(35.0, 46.0), 11))
    H = J.T @ J
    fit[0, 0] = [0, 9, 121, 2.5, 1e-6] + p + list(H[np.triu_indices(6)])
    fit[0, 1] = [3, 0, 5, 0, 0] + p + [0.0] * 21
    fit[1, 0] = [2, 64, 40, 1.0, 1e3] + p + list(H[np.triu_indices(6)])
    fit[1, 1] = [4, 0, 30, 0, 0, np.nan] + p[1:] + [0.0] * 21
    fit[1, 2] = [1] + [0.0] * 31
    src = [{"rms": 0.5, "rms_map": 0.25, "components": [{}, {}]}, {"rms": 0.5, "rms_map": 0.25, "components": [{}, {}, {}]}]
    return fit, src, p, H


class _Wcs:
    def wcs_pix2world(self, x, y, o):
        return 100.0 + 0.01 * x, -40.0 + 0.01 * y


def test_annotate_fits_on_hand_made_rows():
    fit, src, p, H = _hand_rows()
    measure.annotate_fits(src, fit, 12.0, _Wcs(), origin=(5, 7))
    a = src[0]["components"][0]
    assert set(measure.FIT_KEYS) <= set(a) and (a["fit_status"], a["fit_niter"], a["fit_npix"]) == (0, 9, 121)
    assert a["fit_chi2"] == 2.5 / 0.25 and (a["fit_peak"], a["fit_x"], a["fit_y"]) == (8.0, 30.5, 40.25)
    assert (a["fit_ra"], a["fit_dec"]) == (100.0 + 0.01 * 35.5, -40.0 + 0.01 * 47.25)
    assert (a["fit_major"], a["fit_minor"], a["fit_pa"]) == measure.gaussian_shape(0.3, 0.05, 0.2)
    assert a["fit_flux"] == 2 * math.pi * 8.0 / math.sqrt(0.3 * 0.2 - 0.05 ** 2) / 12.0
    cov = 0.25 * np.linalg.inv(H)
    assert np.allclose([a["fit_peak_err"], a["fit_x_err"], a["fit_y_err"]], np.sqrt(np.diag(cov)[:3]), rtol=1e-9)
    for d, st in ((src[0]["components"][1], 3), (src[1]["components"][1], 4), (src[1]["components"][2], 1)):
        assert d["fit_status"] == st and all(d[k] is None for k in measure.FIT_KEYS[3:])
    b = src[1]["components"][0]
    assert b["fit_status"] == 2 and b["fit_niter"] == 64 and b["fit_peak"] == 8.0           # the last accepted p is reported
    # without beam, WCS or rms the keys that need them are None; use_map takes rms_map
    fit, src, _, _ = _hand_rows()
    src[0].pop("rms")
    measure.annotate_fits(src, fit, None, None)
    a = src[0]["components"][0]
    assert a["fit_flux"] is None and a["fit_flux_err"] is None and a["fit_ra"] is None and a["fit_chi2"] is None and a["fit_peak_err"] is None
    assert a["fit_peak"] == 8.0
    fit, src, _, _ = _hand_rows()
    measure.annotate_fits(src, fit, 12.0, None, use_map=True)
    assert src[0]["components"][0]["fit_chi2"] == 2.5 / 0.0625
    assert measure.fit_iterations(fit) == (2, 36.5, 64)


def test_fit_flux_err_against_finite_difference():
    fit, src, p, H = _hand_rows()
    measure.annotate_fits(src, fit, 12.0, None)
    cov = 0.25 * np.linalg.inv(H)
    g = np.zeros(6)
    for j in range(6):
        h = 1e-6 * (abs(p[j]) + 1e-3)
        hi, lo = list(p), list(p)
        hi[j] += h
        lo[j] -= h
        g[j] = (measure.fit_flux(hi, 12.0) - measure.fit_flux(lo, 12.0)) / (2 * h)
    assert np.allclose(g, measure.fit_flux_grad(p, 12.0), rtol=1e-7, atol=1e-9)
    assert abs(src[0]["components"][0]["fit_flux_err"] - math.sqrt(g @ cov @ g)) <= 1e-6 * src[0]["components"][0]["fit_flux_err"]


# ---- 4. command line and exports
def test_cli_flags():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import run
    from caesar_yolo_amd.config import CONFIG
    a = run.parse_args(["--weights=seeded:l:5"])
    assert a.fit_components is False and a.fit_max_iter == 64 and a.deblend_islands is False
    a = run.parse_args(["--weights=seeded:l:5", "--fit_components"])
    assert a.fit_components and a.deblend_islands and a.measure_islands                  # the implications
    assert run.parse_args(["--weights=seeded:l:5", "--fit_components", "--fit_max_iter", "256"]).fit_max_iter == 256
    for bad in ("0", "257", "x"):
        with pytest.raises(SystemExit):
            run.parse_args(["--weights=seeded:l:5", "--fit_max_iter", bad])
    assert CONFIG["fit_components"] is False and CONFIG["fit_max_iter"] == 64


def test_exports():
    from caesar_yolo_amd import lib as L
    from caesar_yolo_amd.model import HipDetector
    assert "cy_fit_components" in L.EXPORTS and "cy_fit_kernel_ms" in L.EXPORTS
    assert L.CY_FIT_FIELDS == len(L.FIT_NAMES) == len(fit_ref.FIELDS) == 32 and tuple(L.FIT_NAMES) == fit_ref.FIELDS
    assert callable(HipDetector.fit_components) and callable(HipDetector.fit_kernel_ms)
    hdr = open(os.path.join(ROOT, "include", "caesar_yolo_hip.h")).read()
    assert "#define CY_FIT_FIELDS 32" in hdr and "int cy_fit_components(" in hdr and "int cy_fit_kernel_ms(" in hdr
    so = L.load()                                             # the built library: raises when it is missing
    assert hasattr(so, "cy_fit_components") and hasattr(so, "cy_fit_kernel_ms")


# ---- 5. the tolerance of the GPU tests
def test_tolerance_measurement():
    """The largest difference between any two of the reference's variants over every GPU test case, on the jobs all of them end
    with status 0: at most TOL / 16 (= fit_ref.MEASURED).  Also what tests/test_gpu_fit.py relies on for the random scene: the
    reference alone leaves out at most 2 % of the jobs, and the floors on status-0 jobs and multi-component sources hold."""
    img, c, res, one, res1 = fit_cases.drawn_reference()
    # the jobs the GPU test compares on status alone (fit_cases.STATUS_ONLY) are left out: a tolerance measured on a job
    # that is not compared with it would only widen the bound for the others
    keep = np.array([0 if nm in fit_cases.STATUS_ONLY else c.ncomp[i] for i, nm in enumerate(c.names)])
    w_drawn, n_drawn, _ = fit_ref.spread(res, keep)
    differ = fit_ref.spread(res, c.ncomp)[2]
    assert not differ.any() and n_drawn >= 34
    w_one, _, differ1 = fit_ref.spread(res1, [c.ncomp[i] for i in one])
    assert not differ1.any()
    _, _, _, (bkg, ncomp, start, masks), rr = fit_cases.random_reference()
    w_rand, n_rand, _ = fit_ref.spread(rr, ncomp)
    skip = fit_cases.excluded(rr, ncomp)
    print("variant spread: drawn %.4g (%d jobs), max_iter 1 %.4g, random %.4g (%d jobs); left out %d of %d" % (
        w_drawn, n_drawn, w_one, w_rand, n_rand, skip.sum(), ncomp.sum()))
    assert max(w_drawn, w_one, w_rand) <= fit_ref.TOL / 16 and fit_ref.TOL == 16 * fit_ref.MEASURED
    assert max(w_drawn, w_one, w_rand) >= fit_ref.MEASURED / 4, "MEASURED is stale: the tolerance is wider than the rule gives"
    assert skip.sum() <= 0.02 * ncomp.sum()
    jobs = np.arange(16)[None, :] < ncomp[:, None]
    assert int((rr[0][:, :, 0][jobs] == 0).sum()) - int(skip.sum()) >= fit_cases.MIN_STATUS0 and int((ncomp > 1).sum()) >= fit_cases.MIN_MULTI
    assert len(ncomp) == fit_cases.N_RANDOM == 300
