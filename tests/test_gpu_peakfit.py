"""cy_fit_peaks on the GPU against the numpy float64 restatement of the same algorithm (tests/peakfit_ref.py, its "tree" variant: the
kernel's own association of the sums) on the inputs of tests/peakfit_cases.py.

Every job compares, exactly: npix, the window, clipped, nneigh, crowded and nexcluded, and the status where the reference's
variants agree on it (they do on every drawn job).  Where all variants converge it also compares the six parameters within
|dp_j| <= TOL (|p_j| + 1e-3), and F and the 21 entries of H within TOL times their own scale (F: |F| + 1e-3 A^2 npix; H_ij:
sqrt(H_ii H_jj)), as tests/test_gpu_fit.py does.  TOL is peakfit_ref.TOL: 16 times the largest difference between the reference's own
variants on these very inputs, measured on the CPU (tests/test_peakfit_cpu.py recomputes it).  Jobs that were not fitted (status 3,
4) report their start bit for bit; jobs the planner turned away (1, 5) report the window as -1 and zeros elsewhere.
No drawn job is left out but the flat patch, which compares status and npix alone.  Of the random scene a job may be left out when
the variants disagree on its status, one of them stopped at a limit, or cond(H) exceeds 1e10; at most 2 % of the jobs are."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import atrous_chain_ref as ACR
import peakfit_cases as PC
import peakfit_ref as PR
from caesar_yolo_amd import lib as L
from caesar_yolo_amd import measure
from gpu_common import detector

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def det():
    return detector("fp32", max_batch=1, max_imgsz=160)


def upload(det, a):
    """The map as it is, NaN and inf included."""
    dev = torch.from_numpy(np.ascontiguousarray(a, np.float32).copy()).to(det.tdev)
    torch.cuda.synchronize()
    return dev


def compare(what, names, jobs, got, res, max_iter, skip=None, status_only=()):
    """res: the reference's rows per variant, the kernel's association first.  -> (jobs compared on parameters, the largest
    parameter difference in units of TOL)."""
    ref = res[0]
    assert got.shape == ref.shape, what
    n0, worst = 0, 0.0
    for e, nm in enumerate(names):
        g, r = got[e], ref[e]
        tag = "%s, job %d (%s)" % (what, e, nm)
        agree = len({q[e, 0] for q in res}) == 1
        assert np.array_equal(g[32:40], r[32:40]), "%s: window .. nexcluded %s, reference %s" % (tag, g[32:40], r[32:40])
        assert g[2] == r[2], "%s: npix %g, reference %g" % (tag, g[2], r[2])
        assert 0 <= g[1] <= max_iter and g[1] == int(g[1]), "%s: niter %g" % (tag, g[1])
        if agree:
            assert g[0] == r[0], "%s: status %g, reference %g (niter %g / %g)" % (tag, g[0], r[0], g[1], r[1])
        else:
            assert g[0] in {q[e, 0] for q in res}, "%s: status %g is none of the variants'" % (tag, g[0])
        if g[0] in (1.0, 5.0):
            assert g[32:36].tolist() == [-1.0] * 4 and not g[1:32].any() and not g[36:].any(), tag
        if g[0] in (3.0, 4.0):
            assert g[1] == 0 and np.array_equal(g[5:11], jobs[e, 5:11], equal_nan=True) and not g[3:5].any() and not g[11:32].any(), tag
        if g[0] in (0.0, 2.0):
            assert np.isfinite(g).all() and g[5] > 0, tag
        if not all(q[e, 0] == 0.0 for q in res) or nm in status_only or (skip is not None and skip[e]):
            continue
        n0 += 1
        d = np.abs(g[5:11] - r[5:11]) / (np.abs(r[5:11]) + 1e-3)
        worst = max(worst, float(d.max()) / PR.TOL)
        assert (d <= PR.TOL).all(), "%s: parameters %s, reference %s, difference %s > TOL %g" % (tag, g[5:11], r[5:11], d, PR.TOL)
        diag = np.sqrt(np.abs(r[[11, 17, 22, 26, 29, 31]]))
        for t, (a, b) in enumerate(PR.FR.IU):
            assert abs(g[11 + t] - r[11 + t]) <= PR.TOL * max(diag[a] * diag[b], 1e-300), "%s: H%d%d %r, reference %r" % (tag, a, b, g[11 + t], r[11 + t])
        assert abs(g[3] - r[3]) <= PR.TOL * (abs(r[3]) + 1e-3 * r[5] * r[5] * r[2]), "%s: F %r, reference %r" % (tag, g[3], r[3])
    return n0, worst


# ---- the drawn cases
@pytest.mark.parametrize("g", [g for g in PC.groups() if g.name != "r256"], ids=lambda g: g.name)
def test_case(det, g):
    res = PC.reference(g)
    dev = upload(det, g.map)
    got = det.fit_peaks(dev, g.jobs, max_iter=g.max_iter)
    assert det.peakfit_kernel_ms() > 0.0
    n0, worst = compare(g.name, g.names, g.jobs, got, res, g.max_iter, status_only=PC.STATUS_ONLY)
    print("%s: %d jobs, %d compared on parameters, worst difference %.3g TOL" % (g.name, len(g.names), n0, worst))
    assert n0 >= {"drawn": 18, "one_iter": 0, "r44": 2, "r46": 2, "neigh": 12}[g.name]
    # the map is only read; the same call twice: byte-equal
    assert dev.cpu().numpy().tobytes() == g.map.tobytes()
    assert det.fit_peaks(dev, g.jobs, max_iter=g.max_iter).tobytes() == got.tobytes(), "%s: a second call gave other bytes" % g.name
    if g.name == "drawn":
        a, b = got[g.names.index("peak_of_hole")], got[g.names.index("hole")]
        assert np.array_equal(a[[0, 1, 2, 3, 4, 5, 8, 9, 10]], b[[0, 1, 2, 3, 4, 5, 8, 9, 10]]) and np.array_equal(a[11:32], b[11:32])      # a hole is its negated peak
    if g.name == "one_iter":
        assert (got[:, 0] == 2).all() and (got[:, 1] == 1).all()


def test_both_sides_of_the_staging_switch(det):
    """R = 44 keeps the window in LDS, R = 46 evaluates membership in every sweep: both meet the reference alike (test_case), and on
    the one blob they hold, each differs from the other as the reference's rows do."""
    g44, g46 = PC.staging(44), PC.staging(46)
    dev = upload(det, g44.map)
    a, b = det.fit_peaks(dev, g44.jobs), det.fit_peaks(dev, g46.jobs)
    ra, rb = PC.reference(g44)[0], PC.reference(g46)[0]
    assert ((a[:, 33] - a[:, 32] + 1) * (a[:, 35] - a[:, 34] + 1) == 89 * 89).all() and ((b[:, 33] - b[:, 32] + 1) * (b[:, 35] - b[:, 34] + 1) == 93 * 93).all()
    assert 89 * 89 <= PR.LDS_MAX < 93 * 93 and (a[:, 0] == 0).all() and (b[:, 0] == 0).all()
    scale = np.abs(ra[:, 5:11]) + 1e-3
    assert np.all(np.abs((a[:, 5:11] - b[:, 5:11]) - (ra[:, 5:11] - rb[:, 5:11])) <= 2 * PR.TOL * scale)


def test_the_largest_radius(det):
    """R = 256 in 600 x 600: 513 x 513 window pixels.  The reference's "tree" variant alone (the other variants agree with it:
    tests/test_peakfit_cpu.py)."""
    g = PC.r256()
    ref = PR.fit_peaks(g.map, g.jobs, g.max_iter)
    got = det.fit_peaks(upload(det, g.map), g.jobs, max_iter=g.max_iter)
    n0, worst = compare(g.name, g.names, g.jobs, got, [ref], g.max_iter)
    assert n0 == 1 and got[0, 2] == ref[0, 2] > 200000 and got[0, 32:36].tolist() == [44.0, 556.0, 44.0, 556.0]
    print("r256: npix %d, worst difference %.3g TOL" % (got[0, 2], worst))


# ---- the random scene
def test_random_scene(det):
    g = PC.random(PC.GPU_SEED)
    res = PC.reference(g)
    skip = PC.excluded(g)
    n = len(g.names)
    assert skip.sum() <= PC.LEFT_OUT_MAX * n, "%d of %d jobs left out" % (skip.sum(), n)
    got = det.fit_peaks(upload(det, g.map), g.jobs)
    n0, worst = compare(g.name, g.names, g.jobs, got, res, 64, skip)
    print("random: %d jobs, %d left out, %d compared on parameters, worst difference %.3g TOL" % (n, skip.sum(), n0, worst))
    assert n0 >= 0.95 * n and (got[:, 37] >= 1).sum() >= 40


# ---- arguments
def test_argument_errors_leave_the_rows_untouched(det):
    g = PC.neigh()
    dev = upload(det, g.map)
    MH, MW = g.map.shape
    n = g.jobs.shape[0]
    jobs = np.ascontiguousarray(g.jobs)
    out = np.full((n, L.CY_PFIT_FIELDS), -7.5, np.float64)
    dp = C.POINTER(C.c_double)
    good = dict(ctx=det.ctx, m=det._p(dev), MH=MH, MW=MW, j=jobs.ctypes.data_as(dp), n=n, it=64, o=out.ctypes.data_as(dp))

    def call(**kw):
        a = dict(good, **kw)
        return det.lib.cy_fit_peaks(a["ctx"], a["m"], a["MH"], a["MW"], a["j"], a["n"], a["it"], a["o"], det._stream())
    bad = [dict(ctx=None), dict(m=None), dict(j=None), dict(o=None), dict(MH=0), dict(MW=0), dict(MH=-3), dict(MW=-1), dict(MH=1 << 16, MW=1 << 15),
           dict(MH=(1 << 31) - 1, MW=(1 << 31) - 1), dict(n=-1), dict(n=L.CY_PFIT_JOBS_MAX + 1), dict(it=0), dict(it=-1), dict(it=257)]
    for kw in bad:
        assert call(**kw) == -1, kw                          # CY_ERR_ARG
        torch.cuda.synchronize()
        assert (out == -7.5).all(), kw
    for kw, text in ((dict(m=None), b"null argument"), (dict(MH=0), b"MH, MW > 0"), (dict(MH=1 << 16, MW=1 << 15), b"2^31"), (dict(n=-1), b"n outside"),
                     (dict(it=257), b"max_iter outside"),
                     # the order of the checks: shape, size, n, max_iter, pointers
                     (dict(MH=0, MW=1 << 30, n=-1, it=0, m=None), b"MH, MW > 0"), (dict(MH=1 << 16, MW=1 << 15, n=-1, it=0, m=None), b"2^31"),
                     (dict(n=-1, it=0, m=None), b"n outside"), (dict(it=0, m=None), b"max_iter outside")):
        assert call(**kw) == -1
        assert text in det.lib.cy_last_error(det.ctx), (kw, det.lib.cy_last_error(det.ctx))
    # n == 0 is no error and writes nothing, whatever the pointers (max_iter still counts)
    assert call(n=0) == 0 and call(n=0, m=None, j=None, o=None) == 0 and call(n=0, it=0) == -1 and (out == -7.5).all()
    assert call() == 0
    assert out.tobytes() == det.fit_peaks(dev, g.jobs).tobytes()
    # a table of jobs the planner turns away launches nothing and still answers
    away = np.array([PC.job(5.0, 5.0, -1.0, PC.start_of(1.0, 5.0, 5.0)), PC.job(float("nan"), 5.0, 2.0, PC.start_of(1.0, 5.0, 5.0))])
    rows = det.fit_peaks(dev, away)
    assert rows[:, 0].tolist() == [1.0, 5.0] and (rows[:, 32:36] == -1.0).all() and not rows[:, 1:32].any() and not rows[:, 36:].any()
    for badcall in (lambda: det.fit_peaks(dev, g.jobs, max_iter=0), lambda: det.fit_peaks(dev.double(), g.jobs), lambda: det.fit_peaks(dev.cpu(), g.jobs),
                    lambda: det.fit_peaks(dev[:, :-1], g.jobs)):
        with pytest.raises(L.CyError):
            badcall()
    assert det.fit_peaks(dev, np.zeros((0, L.CY_PFIT_JOB_FIELDS))).shape == (0, L.CY_PFIT_FIELDS)


def test_kernel_time_is_kept():
    from caesar_yolo_amd.model import HipDetector
    from gpu_common import seeded_weights
    fresh = HipDetector(seeded_weights("l", 5)[0], device=0, precision="fp32", max_batch=1, max_imgsz=160)      # a context of its own
    assert fresh.peakfit_kernel_ms() == -1.0
    g = PC.neigh()
    dev = upload(fresh, g.map)
    fresh.fit_peaks(dev, np.zeros((0, L.CY_PFIT_JOB_FIELDS)))
    fresh.fit_peaks(dev, np.array([PC.job(5.0, 5.0, -1.0, PC.start_of(1.0, 5.0, 5.0))]))
    assert fresh.peakfit_kernel_ms() == -1.0                  # no job that is fitted, no launch
    fresh.fit_peaks(dev, g.jobs)
    assert fresh.peakfit_kernel_ms() > 0.0
    fresh.close()


# ---- cy_fit_components still gives its bytes
def test_component_fit_bytes_are_what_they_were(det):
    """hidx and lm_solve moved from cy_fit.hip to cy_lm.h word for word: cy_fit_components gives the bytes it gave.  The golden rows
    are those of the drawn case clean_pa30 of tests/fit_cases.py, as the GPU gave them in a run in which tests/test_gpu_fit.py
    compared them with the float64 reference."""
    import fit_cases
    img, c = fit_cases.drawn()
    sel = [c.names.index("clean_pa30")]
    boxes, bkg, ncomp, start, masks = c.arrays(sel)
    dev = torch.from_numpy(np.ascontiguousarray(img, np.float32)).to(det.tdev)
    got = det.fit_components(dev, boxes, bkg, ncomp, start, masks)
    want = np.load(os.path.join(ROOT, "tests", "golden", "fit_components_clean_pa30.npy"))
    assert got.shape == want.shape and got[0, 0, 0] == 0 and got.tobytes() == want.tobytes()


# ---- the chain
def test_chain_fits_what_the_searches_list(det):
    img, sources = ACR.scene()
    config = dict(ACR.CONFIG, residual_holes=True, peak_apertures=True, fit_peaks=True, fit_peaks_radius=6.0, fit_peaks_sigma=1.5, residual_peaks_sigma=4.0, residual_peaks_min_above=1)
    plain, _ = ACR.run(det, upload(det, img), [dict(s) for s in sources], dict(config, fit_peaks=False))
    chain, stats = ACR.run(det, upload(det, img), sources, config)
    resid = chain.resid.cpu().numpy()
    rms = det.expand_background(chain.mesh, chain.cell, img.shape, want=("rms",))[1].cpu().numpy()
    lists, before = measure.peak_lists(chain), measure.peak_lists(plain)
    assert set(lists) == set(before) == {"residual_peaks", "residual_holes", "residual_scale_peaks"} and len(lists["residual_scale_peaks"]) >= 2
    assert list(chain.peakfit_rows) == [k for k in ("residual_peaks", "residual_holes", "residual_scale_peaks") if lists[k]]
    njobs = nconv = 0
    for name, rows in chain.peakfit_rows.items():
        entries, sign = lists[name], -1.0 if name == "residual_holes" else 1.0
        select = [i for i, d in enumerate(entries) if d.get("strongest", True)]
        assert chain.peakfit_select[name] == select
        chosen = [entries[i] for i in select]
        iy, ix = np.array([d["y_peak"] for d in chosen]), np.array([d["x_peak"] for d in chosen])
        jobs = measure.peak_fit_jobs(chosen, sign, 6.0, 1.5, resid[iy, ix].astype(np.float64))
        assert np.array_equal(jobs, chain.peakfit_jobs[name]) and (jobs[:, 3] == [d["ap_bkg"] for d in chosen]).all() and (jobs[:, 4] == sign).all()
        res = PR.fit_variants(resid, jobs, 64)
        n0, worst = compare(name, ["%s[%d]" % (name, i) for i in select], jobs, rows, res, 64)
        print("%s: %d entries, %d fitted, %d compared on parameters, worst difference %.3g TOL" % (name, len(entries), len(select), n0, worst))
        want = measure.annotate_peak_fits([{} for _ in entries], rows, jobs, rms[iy, ix].astype(np.float64), sign, 0, None, (0, 0), select)
        for d, w, d0 in zip(entries, want, before[name]):
            assert {k: d[k] for k in measure.GFIT_KEYS} == w and {k: v for k, v in d.items() if k not in measure.GFIT_KEYS} == d0
            assert tuple(d) == tuple(d0) + measure.GFIT_KEYS
        for d in chosen:
            if d["gfit_status"] == 0:
                assert (d["gfit_peak"] > 0) == (sign > 0) and d["gfit_major"] >= d["gfit_minor"] > 0 and d["gfit_chi2"] > 0 and d["gfit_peak_err"] > 0
        njobs, nconv = njobs + len(select), nconv + int((rows[:, 0] == 0).sum())
    assert (stats["peakfit_jobs"], stats["peakfit_converged"]) == (njobs, nconv) and njobs >= 2      # the two blobs at least
    assert stats["peakfit_kernel_ms"] > 0.0 and stats["peakfit_ms"] > 0.0 and stats["peakfit_niter_max"] <= 64
    # the two blobs: a strongest scale peak each, fitted on a disc of six steps, wide
    for x0, y0 in ACR.BLOBS:
        near = [p for p in lists["residual_scale_peaks"] if p["strongest"] and np.hypot(p["x_peak"] - x0, p["y_peak"] - y0) <= 4.0]
        assert len(near) == 1 and near[0]["gfit_radius"] == 6.0 * near[0]["step"] and near[0]["gfit_status"] in (0, 2)
        print("blob at (%d, %d): scale %d, gfit_status %d, peak %.3g, major %.3g, minor %.3g (drawn: peak 1.5, FWHM %.3g)" % (
            x0, y0, near[0]["scale"], near[0]["gfit_status"], near[0]["gfit_peak"], near[0]["gfit_major"], near[0]["gfit_minor"], measure.FWHM * ACR.BLOB_SIGMA))
    assert plain.peakfit_rows is None and not [k for lst in before.values() for d in lst for k in d if k.startswith("gfit_")]
    assert sources == plain.sources
