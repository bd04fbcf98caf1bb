"""The reference of the joint fits of blends (tests/blend_ref.py) against truth, against the single fits and against scipy, the host
helpers of caesar_yolo_amd/measure.py, the command line's handling of --fit_blends, the library's exports, and the measurement of
the tolerance the GPU tests use.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

import blend_cases
import blend_ref
from caesar_yolo_amd import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _job(img, c, i, members):
    x0, y0, h, w = measure.box_window(c.boxes[i], *img.shape)
    yy, xx = np.nonzero(np.isin(c.masks[i].reshape(h, w), [k + 1 for k in members]))
    v = img[y0:y0 + h, x0:x0 + w][yy, xx]
    ok = (v != 0) & np.isfinite(v)
    return x0, y0, xx[ok].astype(np.float64), yy[ok].astype(np.float64), v[ok].astype(np.float64) - c.bkg[i]


def _jac(p, dx, dy):
    """Model and Jacobian [npix, 6 M] of the sum of the Gaussians p [M, 6], written independently of the reference."""
    m, cols = 0.0, []
    for A, x0, y0, a, b, c in np.asarray(p).reshape(-1, 6):
        u, v = dx - x0, dy - y0
        e = np.exp(-0.5 * (a * u * u + 2 * b * u * v + c * v * v))
        g = A * e
        m = m + g
        cols += [e, g * (a * u + b * v), g * (b * u + c * v), -0.5 * g * u * u, -g * u * v, -0.5 * g * v * v]
    return m, np.stack(cols, 1)


# ---- 1. the grouping
def _brute_groups(mask, ncomp):
    h, w = mask.shape
    adj = [[k == l for l in range(ncomp)] for k in range(ncomp)]
    for y in range(h):
        for x in range(w):
            k = int(mask[y, x]) - 1
            if not 0 <= k < ncomp:
                continue
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if 0 <= y + dy < h and 0 <= x + dx < w:
                        l = int(mask[y + dy, x + dx]) - 1
                        if 0 <= l < ncomp:
                            adj[k][l] = True
    for m in range(ncomp):                                   # transitive closure
        for k in range(ncomp):
            for l in range(ncomp):
                adj[k][l] = adj[k][l] or (adj[k][m] and adj[m][l])
    out = []
    for k in range(ncomp):
        members = [l for l in range(ncomp) if adj[k][l]]
        out.append([members[0], len(members), members.index(k)])
    return np.array(out, np.int64).reshape(ncomp, 3)


def test_blend_groups_against_brute_force():
    img, c = blend_cases.drawn()
    for i, nm in enumerate(c.names):
        h, w = measure.box_window(c.boxes[i], *img.shape)[2:]
        got = measure.blend_groups(c.masks[i], h, w, c.ncomp[i])
        assert np.array_equal(got, _brute_groups(c.masks[i].reshape(h, w), c.ncomp[i])), nm
        if nm in blend_cases.GROUPS:
            assert got[:, 0].tolist() == blend_cases.GROUPS[nm], nm
    # bytes above ncomp link nothing: the same mask with one component fewer
    i = c.names.index("chain3")
    h, w = c.masks[i].shape
    assert measure.blend_groups(c.masks[i], h, w, 2)[:, 1].tolist() == [2, 2] and measure.blend_groups(c.masks[i], h, w, 1).tolist() == [[0, 1, 0]]
    assert measure.blend_groups(np.zeros((0, 0), np.uint8), 0, 0, 2).tolist() == [[0, 1, 0], [1, 1, 0]]


# ---- 2. against truth and against the single fits
def test_reference_against_truth_and_single_fits():
    """Noiseless float32 blends: the data are the model rounded to fp32, |delta_i| <= 2^-24 |y_i|, so to first order the
    least-squares solution moves by at most sum_i |(H^-1 J^T)_ji| 2^-24 |y_i| in parameter j; twice that is allowed (second order,
    and the convergence criterion): the bound of tests/test_fit_cpu.py on 6 M parameters.  And the point of the step: the joint
    fit's largest parameter error is smaller than the single fits' on the same components; with noise, its largest flux error."""
    img, c, (res, _), _, _ = blend_cases.drawn_reference()
    clean = [i for i in c.truth if i not in c.noisy]
    assert len(clean) == 6 and len(c.noisy) == 3
    for i in clean:
        M = c.ncomp[i]
        rows, tp = res[0][i, :M], c.truth[i]
        assert (rows[:, 0] == 0).all() and (rows[:, 6] == M).all()
        x0, y0, dx, dy, y = _job(img, c, i, range(M))
        rel = tp.copy()
        rel[:, 1] -= x0
        rel[:, 2] -= y0
        m, J = _jac(rel, dx, dy)
        bound = 2.0 * (np.abs(np.linalg.solve(J.T @ J, J.T)) @ (2.0 ** -24 * np.abs(m)))
        err = np.abs(rows[:, 8:14] - tp)
        assert np.all(err.ravel() <= bound + 1e-12), (c.names[i], err, bound)
        single = np.abs(c.single[i][:M, 5:11] - tp)
        assert err.max() < single.max(), (c.names[i], err.max(), single.max())
    for i in c.noisy:
        M = c.ncomp[i]
        flux = lambda p: np.array([measure.fit_flux(q, 1.0) for q in p])
        joint = np.abs(flux(res[0][i, :M, 8:14]) - flux(c.truth[i]))
        single = np.abs(flux(c.single[i][:M, 5:11]) - flux(c.truth[i]))
        assert joint.max() < single.max(), (c.names[i], joint, single)


# ---- 3. against scipy
def test_reference_against_scipy():
    """Noisy blends: both minimise the same sum of squares.  As in tests/test_fit_cpu.py the two minima agree to the square root
    of the reference's own criterion, taken against the Gauss-Newton scale sqrt(diag(H^-1) F)."""
    so = pytest.importorskip("scipy.optimize", reason="scipy is not installed")
    img, c, (res, _), _, _ = blend_cases.drawn_reference()
    done = 0
    for nm in ("noisy_resolved", "noisy_overlap", "noisy_unequal"):     # with noise: F is a sum of squares of the noise, not of roundings
        i = c.names.index(nm)
        M = c.ncomp[i]
        rows = res[0][i, :M]
        assert (rows[:, 0] == 0).all()
        x0, y0, dx, dy, y = _job(img, c, i, range(M))
        p0 = c.start[i][:M].copy()
        p0[:, 1] -= x0
        p0[:, 2] -= y0
        sol = so.least_squares(lambda p: _jac(p, dx, dy)[0] - y, p0.ravel(), jac=lambda p: _jac(p, dx, dy)[1], method="lm",
                               xtol=1e-15, ftol=1e-15, gtol=1e-15)
        got = rows[:, 8:14].copy()
        got[:, 1] -= x0
        got[:, 2] -= y0
        _, J = _jac(sol.x, dx, dy)
        scale = np.sqrt(np.diag(np.linalg.inv(J.T @ J)) * max(2.0 * sol.cost, 1e-30))
        assert np.all(np.abs(got.ravel() - sol.x) <= 1e-7 * (np.abs(sol.x) + scale) + 1e-12), (nm, got, sol.x)
        assert abs(rows[0, 3] - 2.0 * sol.cost) <= 1e-10 * rows[0, 3]
        # the reported blocks are those of inv(J^T J)
        C = np.linalg.inv(J.T @ J)
        for s in range(M):
            blk = C[6 * s:6 * s + 6, 6 * s:6 * s + 6]
            assert np.allclose(rows[s, 15:36], blk[np.triu_indices(6)], rtol=1e-5, atol=1e-5 * np.abs(np.diag(blk)).max())
        done += 1
    assert done == 3


# ---- 4. host helpers
def test_blend_start():
    fit = np.zeros((2, 16, 32))
    comp = np.zeros((2, 16, 12))
    comp[:, :3] = [50, 10.5, 15, 26, 100, 500, 600, 2600 + 400, 3700 + 100, 3050 + 100, 1, 1]
    fit[0, 0, :11] = [0, 5, 40, 1.0, 1e-6, 9.0, 14.5, 25.5, 0.3, 0.02, 0.2]
    fit[0, 1, :11] = [2, 64, 40, 1.0, 1e3, 8.0, 13.5, 24.5, 0.4, 0.01, 0.3]
    fit[0, 2, :11] = [3, 0, 5, 0, 0, 7.0, 1.0, 2.0, 1.0, 0.0, 1.0]
    fit[1, 0, :11] = [4, 0, 9, 0, 0, np.nan, 1.0, 2.0, 1.0, 0.0, 1.0]
    got = measure.blend_start(fit, comp, np.array([0.5, 0.5]), np.array([[10, 20], [10, 20]]))
    moment = measure.fit_start(comp, np.array([0.5, 0.5]), np.array([[10, 20], [10, 20]]))
    assert got.shape == (2, 16, 6)
    assert got[0, 0].tolist() == fit[0, 0, 5:11].tolist() and got[0, 1].tolist() == fit[0, 1, 5:11].tolist()
    assert np.array_equal(got[0, 2], moment[0, 2]) and np.array_equal(got[1, 0], moment[1, 0]) and np.array_equal(got[1, 5], moment[1, 5])


class _Wcs:
    def wcs_pix2world(self, x, y, o):
        return 100.0 + 0.01 * x, -40.0 + 0.01 * y


def _hand_rows():
    p = [[8.0, 30.5, 40.25, 0.3, 0.05, 0.2], [5.0, 35.5, 41.0, 0.25, -0.03, 0.3]]
    _, J = _jac(np.array(p), np.arange(25.0, 42.0).repeat(11), np.tile(np.arange(35.0, 46.0), 17))
    C = np.linalg.inv(J.T @ J)
    rows = np.zeros((2, 16, 36))
    for s in range(2):
        rows[0, s] = [0, 9, 187, 2.5, 1e-6, 0, 2, s] + p[s] + [1] + list(C[6 * s:6 * s + 6, 6 * s:6 * s + 6][np.triu_indices(6)])
    rows[0, 2, [0, 5, 6]] = [6, 2, 1]
    rows[1, 0] = [3, 0, 9, 0, 0, 0, 2, 0] + p[0] + [0.0] * 22
    rows[1, 1] = [4, 0, 30, 0, 0, 0, 2, 1, np.nan] + p[1][1:] + [0.0] * 22
    rows[1, 2] = [5, 0, 0, 0, 0, 2, 5, 0] + p[0] + [0.0] * 22
    rows[1, 3] = [1] + [0.0] * 35
    rows[1, 4] = [2, 64, 50, 1.0, 1e3, 4, 2, 0] + p[1] + [0.0] * 22           # fitted, but no covariance
    lone = {"fit_" + k[6:]: float(t) for t, k in enumerate(measure.BLEND_KEYS[5:])}
    src = [{"rms": 0.5, "rms_map": 0.25, "components": [{}, {}, dict(lone)]},
           {"rms": 0.5, "rms_map": 0.25, "components": [{}, {}, {}, {}, {}]}]
    return rows, src, p, C, lone


def test_annotate_blends_on_hand_made_rows():
    rows, src, p, C, lone = _hand_rows()
    measure.annotate_blends(src, rows, 12.0, _Wcs(), origin=(5, 7))
    a, b = src[0]["components"][:2]
    assert set(measure.BLEND_KEYS) <= set(a) and len(measure.BLEND_KEYS) == 19
    assert (a["blend_group"], a["blend_size"], a["blend_status"], a["blend_niter"], a["blend_npix"]) == (0, 2, 0, 9, 187)
    assert a["blend_chi2"] == 2.5 / 0.25 == b["blend_chi2"] and (b["blend_peak"], b["blend_x"], b["blend_y"]) == (5.0, 35.5, 41.0)
    assert (a["blend_ra"], a["blend_dec"]) == (100.0 + 0.01 * 35.5, -40.0 + 0.01 * 47.25)
    assert (b["blend_major"], b["blend_minor"], b["blend_pa"]) == measure.gaussian_shape(0.25, -0.03, 0.3)
    assert b["blend_flux"] == measure.fit_flux(p[1], 12.0)
    for s, d in enumerate((a, b)):
        cov = 0.25 * C[6 * s:6 * s + 6, 6 * s:6 * s + 6]                       # the member's own block, times rms^2
        assert np.allclose([d["blend_peak_err"], d["blend_x_err"], d["blend_y_err"]], np.sqrt(np.diag(cov)[:3]), rtol=1e-12)
        g = measure.fit_flux_grad(p[s], 12.0)
        assert abs(d["blend_flux_err"] - math.sqrt(g @ cov @ g)) <= 1e-12 * d["blend_flux_err"]
    # alone: the value keys repeat the component's fit_ values
    l = src[0]["components"][2]
    assert (l["blend_status"], l["blend_group"], l["blend_size"]) == (6, 2, 1)
    assert all(l[k] == lone["fit_" + k[6:]] for k in measure.BLEND_KEYS[5:])
    # not fitted: the value keys are None
    for d, st in zip(src[1]["components"][:4], (3, 4, 5, 1)):
        assert d["blend_status"] == st and all(d[k] is None for k in measure.BLEND_KEYS[5:])
    assert src[1]["components"][2]["blend_size"] == 5
    e = src[1]["components"][4]
    assert e["blend_status"] == 2 and e["blend_peak"] == 5.0 and e["blend_peak_err"] is None and e["blend_flux_err"] is None
    # without beam, WCS or rms the keys that need them are None; use_map takes rms_map; a lone component without fit_ keys gives None
    rows, src, _, _, _ = _hand_rows()
    src[0].pop("rms")
    src[0]["components"][2] = {}
    measure.annotate_blends(src, rows, None, None)
    a = src[0]["components"][0]
    assert a["blend_flux"] is None and a["blend_ra"] is None and a["blend_chi2"] is None and a["blend_peak_err"] is None and a["blend_peak"] == 8.0
    assert all(src[0]["components"][2][k] is None for k in measure.BLEND_KEYS[5:])
    rows, src, _, _, _ = _hand_rows()
    measure.annotate_blends(src, rows, 12.0, None, use_map=True)
    assert src[0]["components"][0]["blend_chi2"] == 2.5 / 0.0625
    assert measure.blend_stats(rows) == (2, 36.5, 64, 1) and measure.blend_stats(np.zeros((3, 16, 36))) == (0, 0.0, 0, 0)


# ---- 5. command line and exports
def test_cli_flags():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import run
    from caesar_yolo_amd.config import CONFIG
    a = run.parse_args(["--weights=seeded:l:5"])
    assert a.fit_blends is False and a.fit_components is False
    a = run.parse_args(["--weights=seeded:l:5", "--fit_components"])
    assert a.fit_blends is False and a.fit_components
    a = run.parse_args(["--weights=seeded:l:5", "--fit_blends", "--fit_max_iter", "100"])
    assert a.fit_blends and a.fit_components and a.deblend_islands and a.measure_islands and a.fit_max_iter == 100       # the implications
    assert CONFIG["fit_blends"] is False


def test_exports():
    from caesar_yolo_amd import lib as L
    from caesar_yolo_amd.model import HipDetector
    assert "cy_fit_blends" in L.EXPORTS and "cy_blend_kernel_ms" in L.EXPORTS
    assert L.CY_BLEND_FIELDS == len(L.BLEND_NAMES) == len(blend_ref.FIELDS) == 36 and tuple(L.BLEND_NAMES) == blend_ref.FIELDS
    assert L.CY_BLEND_MAX_MEMBERS == blend_ref.MAX_MEMBERS == 4
    assert callable(HipDetector.fit_blends) and callable(HipDetector.blend_kernel_ms)
    hdr = open(os.path.join(ROOT, "include", "caesar_yolo_hip.h")).read()
    assert "#define CY_BLEND_FIELDS 36" in hdr and "#define CY_BLEND_MAX_MEMBERS 4" in hdr
    assert "int cy_fit_blends(" in hdr and "int cy_blend_kernel_ms(" in hdr
    so = L.load()                                             # the built library: raises when it is missing
    assert hasattr(so, "cy_fit_blends") and hasattr(so, "cy_blend_kernel_ms")


# ---- 6. and 7. the tolerance and the condition of the GPU tests
def test_tolerance_measurement():
    """The largest difference between any two of the reference's variants over every row the GPU test compares on parameters
    (status 0 in all variants): at most blend_ref.MEASURED; TOL is 16 times the recorded value.  The same for the entries of C
    relative to sqrt(C_ii C_jj): at most MEASURED_C, which is not larger than MEASURED, so C is compared with TOL.  And what
    tests/test_gpu_blend.py relies on for the random scene: the reference alone leaves out at most 2 % of the fitted rows."""
    img, c, (res, cond), one, (res1, _) = blend_cases.drawn_reference()
    w_drawn, c_drawn, n_drawn, differ = blend_ref.spread(res, c.ncomp)
    assert not differ.any() and n_drawn >= 40
    w_one, c_one, _, differ1 = blend_ref.spread(res1, [c.ncomp[i] for i in one])
    assert not differ1.any()
    _, _, _, (bkg, ncomp, start, masks), (rr, rcond) = blend_cases.random_reference()
    skip = blend_cases.excluded(rr, rcond, ncomp)
    w_rand, c_rand, n_rand, _ = blend_ref.spread(rr, ncomp, ~skip)
    rows = np.arange(16)[None, :] < ncomp[:, None]
    fitted = int((rows & np.isin(rr[0][:, :, 0], (0.0, 2.0))).sum())
    print("variant spread: drawn %.4g / C %.4g (%d rows), max_iter 1 %.4g, random %.4g / C %.4g (%d rows); left out %d of %d fitted rows" % (
        w_drawn, c_drawn, n_drawn, w_one, w_rand, c_rand, n_rand, skip.sum(), fitted))
    worst, worst_c = max(w_drawn, w_one, w_rand), max(c_drawn, c_one, c_rand)
    assert worst <= blend_ref.MEASURED and blend_ref.TOL == 16 * blend_ref.MEASURED
    assert worst >= blend_ref.MEASURED / 4, "MEASURED is stale: the tolerance is wider than the rule gives"
    assert worst_c <= blend_ref.MEASURED_C <= blend_ref.MEASURED and blend_ref.TOL_C == blend_ref.TOL
    assert skip.sum() <= 0.02 * fitted and fitted >= 200 and n_rand >= 100
    assert len(ncomp) == 300
