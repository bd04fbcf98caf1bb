"""cy_fit_peak_groups on the GPU against the numpy float64 restatement of the same algorithm (tests/peakgroup_ref.py, its "seq" variant:
the kernel's own association of the sums) on the inputs of tests/peakgroup_cases.py.

Every job compares, exactly: status (where the reference's variants agree on it; they do on every drawn job), npix, group,
nmembers, slot, the window, clipped, nexcluded, nlinked and cov_ok.  Where all variants converge it also compares the six
parameters within |dp_j| <= TOL (|p_j| + 1e-3), F within TOL (|F| + 1e-3 A^2 npix) and the 21 entries of the member's block of C
within TOL_C sqrt(C_ii C_jj).  TOL and TOL_C are peakgroup_ref's: 16 times the largest difference between the reference's own
variants on these very inputs, measured on the CPU (tests/test_peakgroup_cpu.py recomputes them).  Rows that were not fitted
(status 3, 4, 7) report their start bit for bit; rows of statuses 1 and 5 report the window as -1 and zeros elsewhere.
No drawn job is left out but the coincident pair, which compares status and npix alone.  Of the random scene a group job may be
left out when the variants disagree on its status, one of them stopped at a limit, or cond(H) exceeds 1e10; at most 2 % are."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import atrous_chain_ref as ACR
import blend_cases
import peakfit_cases as PC
import peakgroup_cases as GC
import peakgroup_ref as GR
from caesar_yolo_amd import lib as L
from caesar_yolo_amd import measure
from gpu_common import detector

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = [0, 2, 5, 6, 7, 14] + list(range(36, 44))          # status npix group nmembers slot cov_ok, the window .. reserved


@pytest.fixture(scope="module")
def det():
    return detector("fp32", max_batch=1, max_imgsz=160)


def upload(det, a):
    """The map as it is, NaN and inf included."""
    dev = torch.from_numpy(np.ascontiguousarray(a, np.float32).copy()).to(det.tdev)
    torch.cuda.synchronize()
    return dev


def compare(what, names, jobs, got, res, max_iter, skip=None, status_only=()):
    """res: the reference's rows per variant, the kernel's association first.  -> (rows compared on parameters, the largest parameter
    difference in units of TOL, the largest C difference in units of TOL_C)."""
    ref = res[0]
    assert got.shape == ref.shape, what
    n0, worst, worst_c = 0, 0.0, 0.0
    for e, nm in enumerate(names):
        g, r = got[e], ref[e]
        tag = "%s, job %d (%s)" % (what, e, nm)
        sts = {q[e, 0] for q in res}
        if len(sts) == 1:
            assert g[0] == r[0], "%s: status %g, reference %g (niter %g / %g)" % (tag, g[0], r[0], g[1], r[1])
        else:
            assert g[0] in sts, "%s: status %g is none of the variants'" % (tag, g[0])
        for f in EXACT[1:]:
            if f == 14 and (len(sts) > 1 or nm in status_only):
                continue
            assert g[f] == r[f], "%s: %s %g, reference %g" % (tag, L.PGRP_NAMES[f], g[f], r[f])
        assert 0 <= g[1] <= max_iter and g[1] == int(g[1]), "%s: niter %g" % (tag, g[1])
        if g[0] in (1.0, 5.0):
            assert g[36:40].tolist() == [-1.0] * 4 and not g[1:36].any() and not g[40:].any(), tag
        if g[0] == 6.0:
            assert g[5] == e and g[6] == 1 and not g[1:5].any() and not g[7:36].any() and g[41] == 0, tag
        if g[0] in (3.0, 4.0, 7.0):
            assert g[1] == 0 and np.array_equal(g[8:14], jobs[e, 5:11], equal_nan=True) and not g[3:5].any() and not g[14:36].any(), tag
        if g[0] in (0.0, 2.0):
            assert np.isfinite(g).all() and g[8] > 0, tag
        if sts != {0.0} or nm in status_only or (skip is not None and skip[e]):
            continue
        n0 += 1
        d = np.abs(g[8:14] - r[8:14]) / (np.abs(r[8:14]) + 1e-3)
        worst = max(worst, float(d.max()) / GR.TOL)
        assert (d <= GR.TOL).all(), "%s: parameters %s, reference %s, difference %s > TOL %g" % (tag, g[8:14], r[8:14], d, GR.TOL)
        assert abs(g[3] - r[3]) <= GR.TOL * (abs(r[3]) + 1e-3 * r[8] * r[8] * r[2]), "%s: F %r, reference %r" % (tag, g[3], r[3])
        if r[14]:
            diag = np.sqrt(np.abs(r[[15, 21, 26, 30, 33, 35]]))
            for t, (a, b) in enumerate(GR.IU):
                dc = abs(g[15 + t] - r[15 + t]) / max(diag[a] * diag[b], 1e-300)
                worst_c = max(worst_c, dc / GR.TOL_C)
                assert dc <= GR.TOL_C, "%s: C%d%d %r, reference %r" % (tag, a, b, g[15 + t], r[15 + t])
    return n0, worst, worst_c


# ---- the drawn cases
@pytest.mark.parametrize("g", GC.groups(), ids=lambda g: g.name)
def test_case(det, g):
    res, _ = GC.reference(g)
    dev = upload(det, g.map)
    got = det.fit_peak_groups(dev, g.jobs, link=g.link, max_iter=g.max_iter)
    assert det.peakgroup_kernel_ms() > 0.0
    n0, worst, worst_c = compare(g.name, g.names, g.jobs, got, res, g.max_iter, status_only=GC.STATUS_ONLY)
    print("%s: %d jobs, %d compared on parameters, worst difference %.3g TOL, C %.3g TOL_C" % (g.name, len(g.names), n0, worst, worst_c))
    assert n0 >= {"clean": 17, "noisy": 17, "one_iter": 0, "edge": 14, "mw403": 4, "stage_lo": 2, "stage_hi": 2}[g.name]
    # the map is only read; the same call twice: byte-equal
    assert dev.cpu().numpy().tobytes() == g.map.tobytes()
    assert det.fit_peak_groups(dev, g.jobs, link=g.link, max_iter=g.max_iter).tobytes() == got.tobytes(), "%s: a second call gave other bytes" % g.name
    if g.name in ("clean", "noisy"):
        for nm, M in GC.LAYOUT_GROUPS.items():
            e = g.names.index(nm)
            assert got[e, 5] == e and got[e, 6] == M and got[e, 0] == 0, nm
    if g.name == "edge":
        for nm, (st, M) in GC.EDGE_EXPECT.items():
            e = g.names.index(nm)
            assert (got[e, 0] in (0.0, 2.0) if st is None else got[e, 0] == st) and got[e, 6] == M, (nm, got[e, :8])
        a, b = (got[[g.names.index(p + "_a"), g.names.index(p + "_b")]] for p in ("peak_pair", "neg_pair"))
        same = [0, 1, 2, 3, 4, 6, 7, 8, 11, 12, 13] + list(range(14, 36))
        assert np.array_equal(a[:, same], b[:, same]) and np.array_equal(a[:, 9] + 40.0, b[:, 9]) and np.array_equal(a[:, 10], b[:, 10])      # a hole pair is its negated peak pair
        assert got[g.names.index("share_a"), 41] > 0 and got[g.names.index("hole_pair_a"), 41] > 0
    if g.name == "one_iter":
        assert (got[:, 0] == 2).all() and (got[:, 1] == 1).all()
    if g.name == "mw403":
        assert (got[:, 40] == 1).all() and got[0, 37] == 402


def test_both_sides_of_the_staging_switch(det):
    """A group window of 6161 pixels is staged in LDS, one of 10 611 evaluates membership in every sweep: both meet the reference
    alike (test_case), and on the blobs they share each differs from the other as the reference's rows do."""
    lo, hi = GC.stage_lo(), GC.stage_hi()
    a, b = det.fit_peak_groups(upload(det, lo.map), lo.jobs), det.fit_peak_groups(upload(det, hi.map), hi.jobs)
    ra, rb = GC.reference(lo)[0][0], GC.reference(hi)[0][0]
    assert ((a[:, 37] - a[:, 36] + 1) * (a[:, 39] - a[:, 38] + 1) == 101 * 61).all() and ((b[:, 37] - b[:, 36] + 1) * (b[:, 39] - b[:, 38] + 1) == 131 * 81).all()
    assert 101 * 61 <= GR.LDS_MAX < 131 * 81 and (a[:, 0] == 0).all() and (b[:, 0] == 0).all()
    scale = np.abs(ra[:, [8, 11, 12, 13]]) + 1e-3           # the second blob is drawn 10 px further on in stage_hi: A and the shape
    da, db = a[:, [8, 11, 12, 13]] - b[:, [8, 11, 12, 13]], ra[:, [8, 11, 12, 13]] - rb[:, [8, 11, 12, 13]]
    assert np.all(np.abs(da - db) <= 2 * GR.TOL * scale)


# ---- the random scene
def test_random_scene(det):
    g = GC.random(GC.GPU_SEED)
    res, _ = GC.reference(g)
    skip, gj = GC.excluded(g), GC.group_jobs(res)
    njobs = len({int(r[5]) for r in res[0][gj]})
    left = len({int(r[5]) for r in res[0][gj & skip]})
    assert left <= GC.LEFT_OUT_MAX * njobs, "%d of %d group jobs left out" % (left, njobs)
    got = det.fit_peak_groups(upload(det, g.map), g.jobs, link=g.link)
    n0, worst, worst_c = compare(g.name, g.names, g.jobs, got, res, 64, skip)
    print("random: %d jobs, %d group jobs, %d left out, %d rows compared on parameters, worst difference %.3g TOL, C %.3g TOL_C" % (
        len(g.names), njobs, left, n0, worst, worst_c))
    assert njobs >= 40 and n0 >= 0.95 * gj.sum()


# ---- arguments
def test_argument_errors_leave_the_rows_untouched(det):
    g = GC.noisy()
    dev = upload(det, g.map)
    MH, MW = g.map.shape
    n = g.jobs.shape[0]
    jobs = np.ascontiguousarray(g.jobs)
    out = np.full((n, L.CY_PGRP_FIELDS), -7.5, np.float64)
    dp = C.POINTER(C.c_double)
    good = dict(ctx=det.ctx, m=det._p(dev), MH=MH, MW=MW, j=jobs.ctypes.data_as(dp), n=n, lk=1.5, it=64, o=out.ctypes.data_as(dp))

    def call(**kw):
        a = dict(good, **kw)
        return det.lib.cy_fit_peak_groups(a["ctx"], a["m"], a["MH"], a["MW"], a["j"], a["n"], a["lk"], a["it"], a["o"], det._stream())
    bad = [dict(ctx=None), dict(m=None), dict(j=None), dict(o=None), dict(MH=0), dict(MW=0), dict(MH=-3), dict(MW=-1), dict(MH=1 << 16, MW=1 << 15),
           dict(MH=(1 << 31) - 1, MW=(1 << 31) - 1), dict(n=-1), dict(n=L.CY_PFIT_JOBS_MAX + 1), dict(it=0), dict(it=-1), dict(it=257),
           dict(lk=0.0), dict(lk=-1.0), dict(lk=float("nan")), dict(lk=float("inf")), dict(lk=float(np.nextafter(2.0, 3.0)))]
    for kw in bad:
        assert call(**kw) == -1, kw                          # CY_ERR_ARG
        torch.cuda.synchronize()
        assert (out == -7.5).all(), kw
    for kw, text in ((dict(m=None), b"null argument"), (dict(MH=0), b"MH, MW > 0"), (dict(MH=1 << 16, MW=1 << 15), b"2^31"), (dict(n=-1), b"n outside"),
                     (dict(it=257), b"max_iter outside"), (dict(lk=0.0), b"link outside"),
                     # the order of the checks: shape, size, n, max_iter, link, pointers
                     (dict(MH=0, MW=1 << 30, n=-1, it=0, lk=0.0, m=None), b"MH, MW > 0"), (dict(MH=1 << 16, MW=1 << 15, n=-1, it=0, lk=0.0, m=None), b"2^31"),
                     (dict(n=-1, it=0, lk=0.0, m=None), b"n outside"), (dict(it=0, lk=0.0, m=None), b"max_iter outside"), (dict(lk=3.0, m=None), b"link outside")):
        assert call(**kw) == -1
        assert text in det.lib.cy_last_error(det.ctx), (kw, det.lib.cy_last_error(det.ctx))
    # n == 0 is no error and writes nothing, whatever the pointers (max_iter and link still count)
    assert call(n=0) == 0 and call(n=0, m=None, j=None, o=None) == 0 and call(n=0, it=0) == -1 and call(n=0, lk=0.0) == -1 and (out == -7.5).all()
    assert call(lk=2.0) == 0
    assert call() == 0
    assert out.tobytes() == det.fit_peak_groups(dev, g.jobs).tobytes()
    for badcall in (lambda: det.fit_peak_groups(dev, g.jobs, max_iter=0), lambda: det.fit_peak_groups(dev, g.jobs, link=2.5), lambda: det.fit_peak_groups(dev.double(), g.jobs),
                    lambda: det.fit_peak_groups(dev.cpu(), g.jobs), lambda: det.fit_peak_groups(dev[:, :-1], g.jobs)):
        with pytest.raises(L.CyError):
            badcall()
    assert det.fit_peak_groups(dev, np.zeros((0, L.CY_PFIT_JOB_FIELDS))).shape == (0, L.CY_PGRP_FIELDS)


def test_kernel_time_is_kept_and_a_call_without_a_group_launches_nothing():
    from caesar_yolo_amd.model import HipDetector
    from gpu_common import seeded_weights
    fresh = HipDetector(seeded_weights("l", 5)[0], device=0, precision="fp32", max_batch=1, max_imgsz=160)      # a context of its own
    assert fresh.peakgroup_kernel_ms() == -1.0
    g = GC.edge()
    dev = upload(fresh, g.map)
    fresh.fit_peak_groups(dev, np.zeros((0, L.CY_PFIT_JOB_FIELDS)))
    sel = [g.names.index(nm) for nm in ("at_lm_a", "at_lm_b", "away_status1", "away_status5", "share_out") + tuple("chain5_%d" % t for t in range(5))]
    rows = fresh.fit_peak_groups(dev, g.jobs[sel])
    assert fresh.peakgroup_kernel_ms() == -1.0                # lone jobs, jobs turned away and a group of five: no launch
    assert rows[:, 0].tolist() == [6.0, 6.0, 1.0, 5.0, 6.0] + [7.0] * 5 and rows[5:, 6].tolist() == [5.0] * 5 and rows[5:, 5].tolist() == [5.0] * 5
    assert np.array_equal(rows[5:, 8:14], g.jobs[sel][5:, 5:11]) and (rows[2:4, 36:40] == -1.0).all()
    fresh.fit_peak_groups(dev, g.jobs)
    assert fresh.peakgroup_kernel_ms() > 0.0
    fresh.close()


# ---- the chain
PAIR = ((30.0, 200.2, 60.4), (20.0, 204.1, 63.5))          # (peak, x, y) of two planted Gaussians of sigma 1.6 px, 5 px apart


def test_chain_fits_a_planted_pair_jointly(det):
    from fit_cases import gauss
    img, sources = ACR.scene()
    img = (img + sum(gauss(img.shape, a, x, y, 1.6, 1.6, 0.0) for a, x, y in PAIR)).astype(np.float32)
    config = dict(ACR.CONFIG, residual_scales=0, save_scale_maps=False, residual_holes=True, peak_apertures=True, fit_peak_groups=True,
                  residual_peaks_sigma=4.0, residual_peaks_min_above=1)
    plain, _ = ACR.run(det, upload(det, img), [dict(s) for s in sources], dict(config, fit_peak_groups=False, fit_peaks=True))
    chain, stats = ACR.run(det, upload(det, img), sources, config)
    resid = chain.resid.cpu().numpy()
    lists, before = measure.peak_lists(chain), measure.peak_lists(plain)
    assert set(lists) == set(before) == {"residual_peaks", "residual_holes"} and list(chain.peakgroup_rows) == [k for k in ("residual_peaks", "residual_holes") if lists[k]]
    every = []
    for name, rows in chain.peakgroup_rows.items():
        entries, sign, select = lists[name], -1.0 if name == "residual_holes" else 1.0, chain.peakfit_select[name]
        jobs = measure.peak_group_jobs(chain.peakfit_jobs[name], chain.peakfit_rows[name])
        assert np.array_equal(jobs, chain.peakgroup_jobs[name]) and np.array_equal(chain.peakfit_rows[name], plain.peakfit_rows[name])
        fitted = np.isin(chain.peakfit_rows[name][:, 0], (0.0, 2.0))
        assert np.array_equal(jobs[fitted, 5:11], chain.peakfit_rows[name][fitted, 5:11]) and np.array_equal(jobs[~fitted], chain.peakfit_jobs[name][~fitted])
        res, cond = GR.fit_variants(resid, jobs, 1.5, 64)
        n0, worst, worst_c = compare(name, ["%s[%d]" % (name, i) for i in select], jobs, rows, res, 64, GR.excluded(res, cond))
        print("%s: %d entries, %d rows of group jobs, %d compared on parameters, worst difference %.3g TOL, C %.3g TOL_C" % (
            name, len(entries), int(GC.group_jobs(res).sum()), n0, worst, worst_c))
        want = measure.annotate_peak_groups([dict(d) for d in before[name]], rows, chain.peakfit_rms[name], sign, 0, None, (0, 0), select)
        for d, w, d0 in zip(entries, want, before[name]):
            assert d == w and {k: v for k, v in d.items() if k not in measure.GBLEND_KEYS} == d0 and tuple(d) == tuple(d0) + measure.GBLEND_KEYS
        every.append(rows)
    # the planted pair: one group, both members fitted together, each closer to its truth than 0.3 px
    peaks = lists["residual_peaks"]
    found = [min(range(len(peaks)), key=lambda i: np.hypot(peaks[i]["x"] - x, peaks[i]["y"] - y)) for _, x, y in PAIR]
    a, b = (peaks[i] for i in found)
    assert found[0] != found[1] and a["gblend_group"] == b["gblend_group"] == min(found) and a["gblend_status"] == b["gblend_status"] == 0 and a["gblend_size"] >= 2
    for d, (amp, x, y) in zip((a, b), PAIR):
        joint, single = np.hypot(d["gblend_x"] - x, d["gblend_y"] - y), np.hypot(d["gfit_x"] - x, d["gfit_y"] - y)
        print("planted peak %g at (%.1f, %.1f): joint fit %.3f px and peak %.2f, single fit %.3f px and peak %.2f" % (amp, x, y, joint, d["gblend_peak"], single, d["gfit_peak"]))
        assert joint < 0.3 and abs(d["gblend_peak"] - amp) < 0.15 * amp and d["gblend_peak_err"] > 0 and d["gblend_major"] >= d["gblend_minor"] > 0
    every = np.concatenate(every)
    assert (stats["peakgroup_jobs"], stats["peakgroup_members"], stats["peakgroup_converged"], stats["peakgroup_niter_mean"], stats["peakgroup_niter_max"],
            stats["peakgroup_over_limit"]) == measure.peak_group_stats(every) and stats["peakgroup_jobs"] >= 1
    assert stats["peakgroup_kernel_ms"] > 0.0 and stats["peakgroup_ms"] > 0.0 and stats["peakfit_jobs"] == every.shape[0]
    assert plain.peakgroup_rows is None and not [k for lst in before.values() for d in lst for k in d if k.startswith("gblend_")]
    assert sources == plain.sources


# ---- cy_fit_blends and cy_fit_peaks still give their bytes
def test_blend_and_peak_fit_bytes_are_what_they_were(det):
    """The multi-Gaussian sweep, factor, lm_solve, pair_of and the covariance blocks moved from cy_blend.hip to cy_lm_multi.h, and Disc /
    member() from cy_peakfit.hip to cy_disc.h, word for word: cy_fit_blends and cy_fit_peaks give the bytes they gave.  The golden
    rows are those of the drawn blend cases (tests/blend_cases.py) and of the `neigh` group (tests/peakfit_cases.py) as the GPU gave
    them before the move."""
    img, c = blend_cases.drawn()
    got = det.fit_blends(upload(det, img), *c.arrays())
    want = np.load(os.path.join(ROOT, "tests", "golden", "fit_blends_drawn.npy"))
    assert got.shape == want.shape and (got[:, :, 0] == 0).sum() >= 400 and got.tobytes() == want.tobytes()
    g = PC.neigh()
    got = det.fit_peaks(upload(det, g.map), g.jobs, max_iter=g.max_iter)
    want = np.load(os.path.join(ROOT, "tests", "golden", "fit_peaks_neigh.npy"))
    assert got.shape == want.shape and (got[:, 0] == 0).sum() >= 12 and got.tobytes() == want.tobytes()
