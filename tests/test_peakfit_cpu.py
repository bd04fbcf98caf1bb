"""The peak fits (--fit_peaks) on the CPU: the float64 reference of cy_fit_peaks (tests/peakfit_ref.py) against the truth of the drawn
cases and against scipy on the same pixel sets, the measurement of the tolerance the GPU test uses, and the host side: config,
plan(), the command line, annotate_peak_fits on hand-made rows, the exports and Chain.run on the replay detector."""
import json
import os
import sys

import numpy as np
import pytest

import peakfit_cases as PC
import peakfit_ref as PR
from caesar_yolo_amd import lib as L
from caesar_yolo_amd import measure
from test_aperture_cpu import ApertureReplay
from test_measure_chain_cpu import KERNEL_MS, SHAPE, Replay, _setup, _stat_keys, Z
from test_peaks_cpu import PEAK_STEPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAKFIT_STATS = {"peakfit_ms", "peakfit_kernel_ms", "peakfit_jobs", "peakfit_converged", "peakfit_niter_mean", "peakfit_niter_max", "peakfit_crowded"}


# ---- the reference
def test_reference_against_the_truth_of_the_drawn_cases():
    g = PC.drawn()
    rows = PC.reference(g)[0]
    assert len(g.truth) >= 10
    for e, want in g.truth.items():
        # noiseless data rounded to float32 (6e-8 relative) on at least 35 pixels: measured at most 1e-6
        assert rows[e, 0] == 0 and np.all(np.abs(rows[e, 5:11] - want) <= 5e-6 * (np.abs(want) + 1e-3)), (g.names[e], rows[e, 5:11], want)
    st = dict(zip(g.names, rows[:, 0]))
    npix = dict(zip(g.names, rows[:, 2]))
    assert (st["r1"], npix["r1"]) == (3, 5) and (st["pix6"], npix["pix6"]) == (3, 6) and (st["pix7"], npix["pix7"]) == (0, 7)
    assert [st["inadmissible%d" % t] for t in range(4)] == [4] * 4 and npix["inadmissible1"] == 5          # status 4 wins over status 3
    assert (st["all_zero"], npix["all_zero"]) == (3, 0) and npix["invalid_inside"] == 149 - 6
    for nm in ("r0", "r_neg", "r_nan", "r_inf", "r_above", "sign0", "sign2", "sign_nan", "bkg_nan", "bkg_inf", "r0_centre_nan"):
        assert st[nm] == 1, nm
    for nm in ("centre_1e300", "centre_nan", "centre_nan_y", "centre_inf", "centre_minf", "outside_far"):
        assert st[nm] == 5, nm
    for e in np.nonzero(np.isin(rows[:, 0], (1, 5)))[0]:
        assert rows[e, 32:36].tolist() == [-1.0] * 4 and not rows[e, 1:32].any() and not rows[e, 36:].any()
    for e in np.nonzero(np.isin(rows[:, 0], (3, 4)))[0]:
        assert np.array_equal(rows[e, 5:11], g.jobs[e, 5:11], equal_nan=True) and not rows[e, 3:5].any() and not rows[e, 11:32].any() and rows[e, 1] == 0
    clipped = dict(zip(g.names, rows[:, 36]))
    assert clipped["corner"] == clipped["edge"] == clipped["outside"] == 1 and clipped["clean_pa0"] == 0
    one = PC.reference(PC.one_iter())[0]
    assert (one[:, 0] == 2).all() and (one[:, 1] == 1).all()


def test_a_hole_is_its_negated_peak():
    g = PC.drawn()
    rows = PC.reference(g)[0]
    a, b = rows[g.names.index("peak_of_hole")], rows[g.names.index("hole")]
    assert a[0] == b[0] == 0 and g.jobs[g.names.index("hole"), 4] == -1.0
    # the fit runs relative to the window: the same bits but for the centre, which is moved by the cell's offset
    assert np.array_equal(a[[0, 1, 2, 3, 4, 5, 8, 9, 10]], b[[0, 1, 2, 3, 4, 5, 8, 9, 10]]) and np.array_equal(a[11:32], b[11:32])
    assert np.allclose(a[6:8] - a[[32, 34]], b[6:8] - b[[32, 34]], rtol=0, atol=1e-12) and a[5] > 0


def test_sharing_a_disc():
    g = PC.neigh()
    rows = PC.reference(g)[0]
    ix = {nm: i for i, nm in enumerate(g.names)}
    for nm, (nn, crowded) in g.expect.items():
        assert (rows[ix[nm], 37], rows[ix[nm], 38]) == (nn, crowded), nm
    full = rows[ix["alone"], 2]                                # 113 pixels in a disc of radius 6 around a pixel centre
    assert full == 113 and rows[ix["same_a"], 2] == rows[ix["same_b"], 2] == full and rows[ix["same_a"], 39] == 0      # every pixel ties
    # the pixels of column 23 are equidistant from (20, 20) and (26, 20): both jobs count them
    a, b = rows[ix["tie_a"]], rows[ix["tie_b"]]
    ma = PR.members(g.jobs[ix["tie_a"]], a[32:36], [g.jobs[ix["tie_b"], :2]])[0].reshape(13, 13)
    mb = PR.members(g.jobs[ix["tie_b"]], b[32:36], [g.jobs[ix["tie_a"], :2]])[0].reshape(13, 13)
    shared = ma[:, 23 - int(a[32])] & mb[:, 23 - int(b[32])]
    assert shared.sum() == 11 and a[2] == ma.sum() and b[2] == mb.sum() and a[2] + a[39] == full == b[2] + b[39]
    assert rows[ix["at2r"], 39] >= 1 and rows[ix["at2r_x"], 39] == 0
    assert rows[ix["crowd"], 39] > 0 and all(rows[ix["ring%d" % t], 0] == 3 for t in range(12))
    # both sides of the staging switch hold the same blob: the fits agree far inside the noise
    r44, r46 = PC.reference(PC.staging(44))[0], PC.reference(PC.staging(46))[0]
    assert (r44[:, 32:36] == [[11, 99, 11, 99], [76, 164, 10, 98]]).all() and (r46[:, 33] - r46[:, 32] + 1 == 93).all()
    assert 89 * 89 <= PR.LDS_MAX < 93 * 93 and (r44[:, 0] == 0).all() and (r46[:, 0] == 0).all() and (r44[:, 37] == 1).all()
    assert np.all(np.abs(r44[:, 5:11] - r46[:, 5:11]) <= 1e-3 * (np.abs(r44[:, 5:11]) + 1e-3))
    big = PC.reference(PC.r256())[0]
    assert big[0, 0] == 0 and big[0, 32:36].tolist() == [44.0, 556.0, 44.0, 556.0] and big[0, 36] == 0


def test_reference_against_scipy_on_the_same_pixels():
    from scipy.optimize import least_squares
    n = 0
    for g, which in ((PC.drawn(), ("noisy_pa0", "noisy_pa30", "noisy_pa135", "hole", "invalid_inside", "corner")), (PC.neigh(), ("pair5_a", "pair5_b", "tie_a", "crowd"))):
        rows = PC.reference(g)[0]
        win, neigh, _ = PR.plan(g.jobs, *g.map.shape)
        for nm in which:
            e = g.names.index(nm)
            job, (x0, x1, y0, y1) = g.jobs[e], win[e, 1:5]
            mine, _, dx, dy = PR.members(job, (x0, x1, y0, y1), [g.jobs[f, :2] for f in neigh[e]])
            v = g.map[y0:y1 + 1, x0:x1 + 1].ravel()
            ok = mine & (v != 0) & np.isfinite(v)
            assert ok.sum() == rows[e, 2]
            y = job[4] * (v[ok].astype(np.float64) - job[3])

            def resid(p):
                u, w = dx[ok] - p[1], dy[ok] - p[2]
                return y - p[0] * np.exp(-0.5 * (p[3] * u * u + 2.0 * p[4] * u * w + p[5] * w * w))
            p0 = rows[e, 5:11].copy()
            p0[1] -= x0
            p0[2] -= y0
            sol = least_squares(resid, p0 * [1.02, 1.0, 1.0, 0.97, 1.0, 1.03] + [0, 0.05, -0.05, 0, 0.01, 0], xtol=1e-15, ftol=1e-15, gtol=1e-15)
            # two minimisers of one sum of squares: both stop where a step is below 1e-10 of a parameter
            assert np.all(np.abs(sol.x - p0) <= 1e-7 * (np.abs(p0) + 1e-3)), (nm, sol.x, p0)
            # F of noiseless data is the float32 rounding of the pixels, 1e-11: of the order of what a step of 1e-7 changes
            assert rows[e, 3] < 1e-9 or abs(2.0 * sol.cost - rows[e, 3]) <= 1e-9 * rows[e, 3]
            n += 1
    assert n == 10


# ---- the tolerance
def test_the_measured_tolerance_and_the_left_out_share():
    worst = 0.0
    for g in PC.groups():
        res = PC.reference(g)
        keep = [e for e, nm in enumerate(g.names) if nm not in PC.STATUS_ONLY]
        w, all0, differ = PR.spread(res, keep)
        assert not differ.any(), (g.name, [g.names[e] for e in np.nonzero(differ)[0]])      # no drawn job on which the variants disagree
        for e in keep:                                        # ... or on which only some of them converge
            assert len({r[e, 0] for r in res}) == 1, g.names[e]
        worst = max(worst, w)
    for seed in PC.SEEDS:
        g = PC.random(seed)
        res = PC.reference(g)
        w, all0, _ = PR.spread(res)
        out = PC.excluded(g)
        n = len(g.names)
        print("random scene, seed %d: %d jobs, %d left out (%.1f %%), all variants converged on %d, spread %.3g" % (seed, n, out.sum(), 100.0 * out.sum() / n, all0.sum(), w))
        assert n >= 170 and out.sum() <= PC.LEFT_OUT_MAX * n and all0.sum() >= 0.95 * n
        assert (res[0][:, 37] >= 1).sum() >= 40 and (res[0][:, 39] > 0).sum() >= 40          # a crowded scene: discs are shared
        worst = max(worst, w)
    print("largest spread between two variants: %.4g (MEASURED %.4g, TOL %.4g)" % (worst, PR.MEASURED, PR.TOL))
    assert 0.9 * PR.MEASURED <= worst <= PR.MEASURED and PR.TOL == 16 * PR.MEASURED
    assert "%.3g" % PR.TOL in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- config, plan() and the command line
def test_peakfit_config():
    assert measure.peakfit_config({}) == (6.0, 1.5, 64) and not measure.wants_peak_fits({})
    assert measure.wants_peak_fits({"fit_peaks": True}) and not measure.wants_peak_fits({"fit_peaks": False})
    assert measure.peakfit_config({"fit_peaks_radius": 4, "fit_peaks_sigma": "2.5", "fit_peaks_max_iter": 256}) == (4.0, 2.5, 256)
    assert measure.peakfit_config({"fit_peaks_max_iter": 1})[2] == 1
    for bad in ({"fit_peaks_radius": 0.0}, {"fit_peaks_radius": -1.0}, {"fit_peaks_radius": float("nan")}, {"fit_peaks_radius": float("inf")},
                {"fit_peaks_sigma": 0.0}, {"fit_peaks_sigma": -2.0}, {"fit_peaks_sigma": float("nan")}, {"fit_peaks_sigma": float("inf")},
                {"fit_peaks_max_iter": 0}, {"fit_peaks_max_iter": 257}, {"fit_peaks_max_iter": -3}, {"fit_peaks_max_iter": 2.5}, {"fit_peaks_max_iter": True}):
        with pytest.raises(ValueError):
            measure.peakfit_config(bad)
    # the defaults at the last scale: 6 * 32 = 192 <= 256
    assert measure.peakfit_config({})[0] * (1 << (measure.SCALES_MAX - 1)) == 192 <= L.CY_PFIT_RADIUS_MAX


def test_plan_with_and_without_the_switch():
    from test_measure_chain_cpu import IMPLIED
    for flag, steps in IMPLIED.items():
        assert measure.plan({flag: True}) == steps == measure.plan({flag: True, "fit_peaks": False}), flag
        assert set(measure.plan({flag: True, "fit_peaks": True})) == set(steps) | set(PEAK_STEPS)
    assert measure.plan({}) == () == measure.plan({"fit_peaks": False, "fit_peaks_radius": -1})
    assert measure.plan({"fit_peaks": True}) == PEAK_STEPS == measure.plan({"peak_apertures": True}) == measure.plan({"fit_peaks": True, "peak_apertures": True})
    assert measure.plan({"fit_peaks": True, "fit_blends": True}) == measure.STEPS
    assert not measure.wants_peaks({"fit_peaks": True}) and not measure.wants_scales({"fit_peaks": True}) and not measure.wants_apertures({"fit_peaks": True})


def test_flags_parse_and_imply():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import run
    w = "--weights=seeded:l:5"
    base = run.measure_config(run.parse_args([w]))
    assert (base["fit_peaks"], base["fit_peaks_radius"], base["fit_peaks_sigma"], base["fit_peaks_max_iter"]) == (False, 6.0, 1.5, 64)
    assert measure.plan(base) == () and not measure.wants_peak_fits(base) and measure.peakfit_config(base) == measure.peakfit_config({})
    args = run.parse_args([w, "--fit_peaks"])                   # alone: the pixel search comes with it
    config = run.measure_config(args)
    assert measure.wants_peak_fits(config) and config["residual_peaks"] is True and not config["residual_holes"] and config["residual_scales"] == 0
    assert not config["peak_apertures"] and measure.plan(config) == PEAK_STEPS and args.residual_map and args.bkg_map and args.fit_components
    for search in (["--residual_scales=3"], ["--residual_holes"]):     # with a search of its own: that one, and no other
        config = run.measure_config(run.parse_args([w, "--fit_peaks"] + search))
        assert measure.wants_peak_fits(config) and config["residual_peaks"] is False and measure.plan(config) == PEAK_STEPS
    args = run.parse_args([w, "--fit_peaks", "--fit_peaks_radius=4.5", "--fit_peaks_sigma", "2", "--fit_peaks_max_iter=9", "--peak_apertures"])
    assert measure.peakfit_config(run.measure_config(args)) == (4.5, 2.0, 9) and args.peak_apertures and args.residual_peaks
    for bad in (["--fit_peaks_radius=0"], ["--fit_peaks_radius=-1"], ["--fit_peaks_radius=nan"], ["--fit_peaks_sigma=0"], ["--fit_peaks_sigma=inf"],
                ["--fit_peaks_max_iter=0"], ["--fit_peaks_max_iter=257"]):
        with pytest.raises(SystemExit):
            run.parse_args([w, "--fit_peaks"] + bad)
    with pytest.raises(SystemExit):
        run.parse_args([w, "--fit_peaks_radius=abc"])
    assert run.parse_args([w, "--fit_peaks_radius=-1"]).fit_peaks is False       # without the switch the values are not looked at
    for flag in ("fit_peaks", "fit_peaks_radius", "fit_peaks_sigma", "fit_peaks_max_iter"):
        assert "--" + flag in run.__doc__ and flag in run.MEASURE_KEYS, flag
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--fit_peaks" in readme and "--fit_peaks_radius" in readme


def test_exports():
    assert {"cy_fit_peaks", "cy_peakfit_kernel_ms"} <= set(L.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "caesar_yolo_hip.h")).read()
    for name, text in (("CY_PFIT_JOB_FIELDS", "11"), ("CY_PFIT_FIELDS", "40"), ("CY_PFIT_RADIUS_MAX", "256"), ("CY_PFIT_NEIGH_MAX", "8"), ("CY_PFIT_JOBS_MAX", "(1 << 20)")):
        assert any(line.split()[:3] == ["#define", name, text.split()[0]] for line in hdr.split("\n")) and getattr(L, name) == eval(text), name
    assert "int cy_fit_peaks(cy_ctx* ctx, const float* d_map, int MH, int MW, const double* h_jobs" in hdr
    assert "int cy_peakfit_kernel_ms(const cy_ctx* ctx, double* out_ms);" in hdr
    assert len(L.PFIT_NAMES) == L.CY_PFIT_FIELDS == PR.FIELDS and L.PFIT_NAMES == PR.NAMES and L.PFIT_NAMES[:32] == L.FIT_NAMES
    assert len(L.PFIT_JOB_NAMES) == L.CY_PFIT_JOB_FIELDS == PR.JOB_FIELDS and L.PFIT_JOB_NAMES == PR.JOB_NAMES
    lib = L.load()
    assert hasattr(lib, "cy_fit_peaks") and hasattr(lib, "cy_peakfit_kernel_ms")
    jobs = open(os.path.join(ROOT, "caesar_yolo_amd", "csrc", "cy_measure_jobs.h")).read()
    for text in ("PFIT_JOB_FIELDS = 11;", "PFIT_FIELDS = 40;", "PFIT_RADIUS_MAX = 256;", "PFIT_NEIGH_MAX = 8;", "PFIT_JOBS_MAX = 1 << 20;", "struct PeakFitJob {"):
        assert text in jobs
    csrc = os.path.join(ROOT, "caesar_yolo_amd", "csrc")
    lm, fit, pf = (open(os.path.join(csrc, f)).read() for f in ("cy_lm.h", "cy_fit.hip", "cy_peakfit.hip"))
    for text in ("constexpr int hidx(int i, int j)", "bool lm_solve(const double* cur, const double lam, double* d)"):      # stated once, shared
        assert text in lm and text not in fit and text not in pf
    assert "lm_iterate(" in pf and "gauss_terms(" in pf and "#pragma clang fp contract(off)" in pf and "atomic" not in pf.replace("No atomics", "").replace("no atomics", "") and "asm" not in pf.replace("inline assembly", "")
    import __graft_entry__ as ge
    assert "cy_peakfit.hip" in ge.HIP_SOURCES and "cy_measure_plan.cpp" in ge.CXX_SOURCES
    from caesar_yolo_amd.model import HipDetector
    assert callable(HipDetector.fit_peaks) and callable(HipDetector.peakfit_kernel_ms)


# ---- annotate_peak_fits on hand-made rows
def _row(status, p=(2.0, 10.0, 20.0, 0.5, 0.1, 0.25), niter=7, npix=50, F=4.0, nex=3, nn=2, crowded=0, clipped=1):
    r = np.zeros(L.CY_PFIT_FIELDS)
    r[0], r[1], r[2] = status, niter if status in (0, 2) else 0, 0 if status in (1, 5) else npix
    if status in (0, 2):
        r[3], r[4] = F, 1e-5
        H = np.diag([50.0, 40.0, 30.0, 20.0, 10.0, 5.0]) + 0.5
        r[11:32] = H[np.triu_indices(6)]
    if status not in (1, 5):
        r[5:11] = p
        r[32:40] = [4, 16, 14, 26, clipped, nn, crowded, nex]
    else:
        r[32:36] = -1.0
    return r


def test_annotate_peak_fits_on_hand_made_rows():
    from caesar_yolo_amd.wcs import WCS
    wcs = WCS(json.loads(str(Z["wcs_header"])))
    statuses = [0, 2, 1, 3, 4, 5]
    rows = np.stack([_row(s) for s in statuses])
    jobs = np.array([[10.0, 20.0, 6.0, 0.125, 1.0, 2.0, 10.0, 20.0, 0.4, 0.0, 0.4]] * len(statuses))
    rms = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 0.5])
    for sign in (1.0, -1.0):
        entries = [{"x": 1.0, "keep": i} for i in statuses]
        out = measure.annotate_peak_fits(entries, rows, jobs, rms, sign, 12.5, wcs, (3.0, 4.0))
        assert out is entries and all(set(d) == {"x", "keep"} | set(measure.GFIT_KEYS) for d in entries)
        head = ("gfit_status", "gfit_niter", "gfit_npix", "gfit_nexcluded", "gfit_nneigh", "gfit_crowded", "gfit_clipped", "gfit_radius", "gfit_bkg")
        for d, s in zip(entries, statuses):
            assert d["gfit_status"] == s and d["gfit_radius"] == 6.0 and d["gfit_bkg"] == 0.125 and type(d["gfit_npix"]) is int
            if s in (0, 2):
                ref = {}
                measure._gaussian_keys(ref, "fit_", rows[0][:32], measure.FIT.F, measure._FIT_PARAMS, measure.fit_covariance, 0.5, 12.5, wcs, 3.0, 4.0)
                want = {"g" + k: v for k, v in ref.items()}
                want["gfit_peak"], want["gfit_flux"] = sign * want["gfit_peak"], sign * want["gfit_flux"]
                assert {k: d[k] for k in want} == want and d["gfit_peak"] == sign * 2.0 and d["gfit_chi2"] == 16.0 and d["gfit_flux_err"] > 0 and d["gfit_ra"] is not None
                assert (d["gfit_niter"], d["gfit_npix"], d["gfit_nexcluded"], d["gfit_nneigh"], d["gfit_crowded"], d["gfit_clipped"]) == (7, 50, 3, 2, 0, 1)
            else:
                assert all(d[k] is None for k in measure.GFIT_KEYS if k not in head), s
                assert d["gfit_npix"] == (0 if s in (1, 5) else 50) and d["gfit_niter"] == 0
    # no beam, no WCS, no noise: the keys that need them stay None
    d = measure.annotate_peak_fits([{}], rows[:1], jobs[:1], [float("nan")], 1.0, 0, None)[0]
    assert d["gfit_flux"] is None and d["gfit_ra"] is None and d["gfit_chi2"] is None and d["gfit_peak_err"] is None and d["gfit_major"] > d["gfit_minor"] > 0
    # entries that were not fitted: every key None
    entries = [{"strongest": t != 1} for t in range(3)]
    measure.annotate_peak_fits(entries, rows[:2], jobs[:2], rms[:2], 1.0, 12.5, None, select=[0, 2])
    assert entries[0]["gfit_status"] == 0 and entries[2]["gfit_status"] == 2 and all(entries[1][k] is None for k in measure.GFIT_KEYS)
    assert measure.peak_fit_stats(rows) == (6, 1, 7.0, 7, 0) and measure.peak_fit_stats(np.zeros((0, L.CY_PFIT_FIELDS))) == (0, 0, 0.0, 0, 0)
    json.dumps(entries)


def test_peak_fit_jobs():
    entries = [{"x": 40.5, "y": 30.25, "peak": 3.0, "x_peak": 40, "y_peak": 30},
               {"x": 50.0, "y": 60.0, "peak": -2.0, "step": 4, "ap_bkg": 0.5, "x_peak": 50, "y_peak": 60},
               {"x": 9.0, "y": 8.0, "peak": 1.5, "ap_bkg": None, "x_peak": 9, "y_peak": 8}]
    jobs = measure.peak_fit_jobs(entries, 1.0, 6.0, 1.5, [2.5, 0.25, float("nan")], (37, 21))
    a1, a4 = 1.0 / (1.5 * 1.5), 1.0 / (6.0 * 6.0)
    assert jobs.tolist() == [[3.5, 9.25, 6.0, 0.0, 1.0, 2.5, 3.5, 9.25, a1, 0.0, a1], [13.0, 39.0, 24.0, 0.5, 1.0, 2.0, 13.0, 39.0, a4, 0.0, a4],
                             [-28.0, -13.0, 6.0, 0.0, 1.0, 1.5, -28.0, -13.0, a1, 0.0, a1]]
    holes = measure.peak_fit_jobs(entries[:2], -1.0, 6.0, 1.5, [-2.5, 0.75], (0, 0))
    assert holes[:, 4].tolist() == [-1.0, -1.0] and holes[:, 5].tolist() == [2.5, 2.0]      # -(v - bkg), and |peak| where that is not > 0


# ---- Chain.run on the replay detector
class PeakFitReplay(ApertureReplay):
    """ApertureReplay plus fit_peaks: hand-made rows (job i: status i % 3 * 2, so 0, 2, 4), every argument kept."""

    def __init__(self, scenario):
        ApertureReplay.__init__(self, scenario)
        self.pfit_args = []

    def fit_peaks(self, map_dev, jobs, max_iter=64):
        self.calls.append("fit_peaks")
        jobs = np.array(jobs, np.float64)
        self.pfit_args.append(dict(map_dev=map_dev, jobs=jobs, max_iter=max_iter))
        return np.stack([_row(i % 3 * 2, p=(j[5], j[6] + 0.5, j[7] - 0.25, 0.5, 0.1, 0.25), crowded=int(i == 0)) for i, j in enumerate(jobs)])


def test_chain_without_the_switch_is_what_it_was():
    base_calls = None
    for extra in ({}, {"fit_peaks": False, "fit_peaks_radius": -1.0, "fit_peaks_max_iter": 0}):     # not looked at without the switch
        s, kw = _setup("B")
        config = dict(s["config"], **extra)
        det, stats = Replay("B"), {}                          # has no fit_peaks: a call would raise
        chain = measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], config, **kw).run(measure.plan(config), stats)
        assert measure.plan(config) == measure.plan(s["config"])
        base_calls = base_calls or list(det.calls)
        assert det.calls == base_calls and det.calls[-1] == "measure_residuals"
        assert set(stats) == _stat_keys(measure.plan(config), json.loads(str(Z["B/stats"]))) and not set(stats) & PEAKFIT_STATS
        assert chain.peakfit_rows is None and chain.peakfit_stats is None and measure.peak_lists(chain) == {}
        assert [{k: v for k, v in o.items()} for o in json.loads(json.dumps(s["sources"]))] == json.loads(str(Z["B/catalog"]))
    # searches and apertures without the switch: the lists carry no gfit key and nothing is called after the apertures
    s, kw = _setup("B")
    config = dict(s["config"], residual_peaks=True, residual_scales=3, peak_apertures=True)
    det = ApertureReplay("B")                                 # no fit_peaks either
    chain = measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], config, **kw).run(measure.plan(config), {})
    assert chain.peak_list and chain.scale_list and not [k for d in chain.peak_list + chain.scale_list for k in d if k.startswith("gfit_")]
    assert det.calls[-1] == "aperture_sums"


@pytest.mark.parametrize("searches,apertures", [("peaks", False), ("holes", True), ("scales", False), ("all", True), ("none", False)])
def test_chain_with_the_switch(searches, apertures):
    s, kw = _setup("B")
    J = 4
    on = {"peaks": dict(residual_peaks=True), "holes": dict(residual_holes=True), "scales": dict(residual_scales=J),
          "all": dict(residual_peaks=True, residual_holes=True, residual_scales=J), "none": {}}[searches]
    config = dict(s["config"], fit_peaks=True, fit_peaks_radius=5.0, fit_peaks_sigma=2.0, fit_peaks_max_iter=33, peak_apertures=apertures,
                  residual_peaks_max=10, **on)
    plain_steps = measure.plan(s["config"])
    assert measure.plan(config) == plain_steps                # the same steps: the fits are no step
    det0 = PeakFitReplay("B")
    s0, _ = _setup("B")
    stats0 = {}
    chain0 = measure.Chain(det0, np.zeros(SHAPE, np.float32), s0["sources"], dict(config, fit_peaks=False), **kw).run(plain_steps, stats0)
    det, src, stats = PeakFitReplay("B"), s["sources"], {}
    chain = measure.Chain(det, np.zeros(SHAPE, np.float32), src, config, **kw).run(plain_steps, stats)
    names = {"peaks": ["residual_peaks"], "holes": ["residual_peaks", "residual_holes"], "scales": ["residual_scale_peaks"],
             "all": ["residual_peaks", "residual_holes", "residual_scale_peaks"], "none": []}[searches]
    # the order: everything the run without the switch called, then the rms map once and one call per list
    assert "fit_peaks" not in det0.calls and det.calls[:len(det0.calls)] == det0.calls
    assert det.calls[len(det0.calls):] == (["expand_background"] + ["fit_peaks"] * len(names) if names else [])
    lists = measure.peak_lists(chain)
    assert [k for k in ("residual_peaks", "residual_holes", "residual_scale_peaks") if k in lists] == names and list(chain.peakfit_rows) == names
    bx, by = kw["box_origin"]
    njobs = 0
    for name, a in zip(names, det.pfit_args):
        entries = lists[name]
        sign = -1.0 if name == "residual_holes" else 1.0
        select = [i for i, d in enumerate(entries) if d.get("strongest", True)]
        assert chain.peakfit_select[name] == select and len(select) >= 1
        assert a["map_dev"] is chain.resid and a["max_iter"] == 33 and a["jobs"].shape == (len(select), L.CY_PFIT_JOB_FIELDS)
        before = chain0.peak_list if name == "residual_peaks" else chain0.hole_list if name == "residual_holes" else chain0.scale_list
        for t, i in enumerate(select):
            d, j = entries[i], a["jobs"][t]
            step = d.get("step", 1)
            bkg = d["ap_bkg"] if apertures and d["ap_bkg"] is not None else 0.0
            # the replay's residual map is 0: A0 = sign * (0 - bkg) is not > 0 unless the background is negative
            A0 = sign * (0.0 - bkg) if sign * (0.0 - bkg) > 0 else abs(d["peak"])
            assert j.tolist() == [d["x"] - bx, d["y"] - by, 5.0 * step, bkg, sign, A0, d["x"] - bx, d["y"] - by, 1.0 / (2.0 * step) ** 2, 0.0, 1.0 / (2.0 * step) ** 2]
        rows = chain.peakfit_rows[name]
        assert rows.shape == (len(select), L.CY_PFIT_FIELDS) and np.array_equal(chain.peakfit_jobs[name], a["jobs"])
        moved = rows.copy()
        moved[:, [6, 32, 33]] += bx
        moved[:, [7, 34, 35]] += by
        want = measure.annotate_peak_fits([{} for _ in entries], moved, a["jobs"], np.zeros(len(select)), sign, kw["beam_area"], kw["wcs"], kw["wcs_origin"], select)
        for i, (d, w, d0) in enumerate(zip(entries, want, before)):
            assert set(d) == set(d0) | set(measure.GFIT_KEYS) and {k: d[k] for k in d0} == d0 and {k: d[k] for k in measure.GFIT_KEYS} == w
            if i not in select:
                assert all(d[k] is None for k in measure.GFIT_KEYS)
        first = entries[select[0]]
        assert first["gfit_status"] == 0 and first["gfit_x"] == first["x"] + 0.5 and first["gfit_y"] == first["y"] - 0.25 and first["gfit_radius"] == 5.0 * first.get("step", 1)
        assert (first["gfit_peak"] > 0) == (sign > 0) and (first["gfit_flux"] > 0) == (sign > 0) and first["gfit_chi2"] is None      # the replay's rms map is 0
        njobs += len(select)
    assert json.loads(json.dumps(src)) == json.loads(json.dumps(s0["sources"]))
    old = {k for k in stats if k not in PEAKFIT_STATS}
    assert set(stats) == old | PEAKFIT_STATS and old == set(stats0)
    every = np.concatenate([chain.peakfit_rows[n] for n in names]) if names else np.zeros((0, L.CY_PFIT_FIELDS))
    assert (stats["peakfit_jobs"], stats["peakfit_converged"], stats["peakfit_crowded"]) == (njobs, int((every[:, 0] == 0).sum()), len(names))
    assert stats["peakfit_kernel_ms"] == len(names) * KERNEL_MS and stats["peakfit_ms"] >= 0.0
    assert stats["peakfit_niter_max"] == (7 if njobs else 0) and stats["peakfit_niter_mean"] == (7.0 if njobs else 0.0)
    json.dumps(lists)


def test_chain_fits_nothing_without_the_residual_step():
    s, kw = _setup("B")
    config = dict(s["config"], fit_peaks=True, residual_peaks=True)
    det, stats = PeakFitReplay("B"), {}
    steps = tuple(k for k in measure.plan(config) if k not in ("blend", "residual"))
    chain = measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], config, **kw).run(steps, stats)
    assert "fit_peaks" not in det.calls and not set(stats) & PEAKFIT_STATS and chain.peakfit_rows is None
    with pytest.raises(ValueError):
        measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], dict(config, fit_peaks_max_iter=300), **kw)
