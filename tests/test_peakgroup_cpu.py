"""The joint fits of neighbouring peaks (--fit_peak_groups) on the CPU: the float64 reference of cy_fit_peak_groups
(tests/peakgroup_ref.py) against the truth of the clean drawn cases and against the single fits, the measurement of the tolerance the
GPU test uses, and the host side: config, plan(), the command line, the exports, annotate_peak_groups on hand-made rows and
Chain.run on the replay detector."""
import json
import os
import sys

import numpy as np
import pytest

import blend_ref as BR
import peakfit_ref as PR
import peakgroup_cases as GC
import peakgroup_ref as GR
from caesar_yolo_amd import lib as L
from caesar_yolo_amd import measure
from test_measure_chain_cpu import KERNEL_MS, SHAPE, _setup, Z
from test_peakfit_cpu import PEAKFIT_STATS, PeakFitReplay
from test_peakfit_cpu import _row as pfit_row
from test_peaks_cpu import PEAK_STEPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAKGROUP_STATS = {"peakgroup_ms", "peakgroup_kernel_ms", "peakgroup_jobs", "peakgroup_members", "peakgroup_converged", "peakgroup_niter_mean",
                   "peakgroup_niter_max", "peakgroup_over_limit"}


# ---- the reference
def test_reference_against_the_truth_and_the_single_fits():
    g = GC.clean()
    rows = GC.reference(g)[0][0]
    single = PR.fit_peaks(g.map, g.jobs, 64)
    assert len(g.truth) == len(g.names) == 17
    err = lambda p, want: float(np.max(np.abs(p - want) / (np.abs(want) + 1e-3)))
    for e, want in g.truth.items():
        # noiseless data rounded to float32 (6e-8 relative): measured at most 1.4e-7; the bound is that of the single fits' test
        assert rows[e, 0] == 0 and np.all(np.abs(rows[e, 8:14] - want) <= 5e-6 * (np.abs(want) + 1e-3)), (g.names[e], rows[e, 8:14], want)
        assert single[e, 0] == 0 and err(rows[e, 8:14], want) < err(single[e, 5:11], want), g.names[e]
    # the bias of the single fits is what the issue measured: large at 4 px, small at 7 px
    ix = {nm: i for i, nm in enumerate(g.names)}
    bias = {nm: float(np.hypot(*(single[ix[nm], 6:8] - g.truth[ix[nm]][1:3]))) for nm in ("pair4_b", "pair5_b", "pair7_b")}
    print("position error of the fainter member's single fit: %s px; of the joint fit at most %.2g px" % (
        {k: round(v, 3) for k, v in bias.items()}, max(np.hypot(*(rows[e, 9:11] - t[1:3])) for e, t in g.truth.items())))
    assert bias["pair4_b"] > 0.5 > bias["pair5_b"] > 0.1 > bias["pair7_b"]
    for nm, M in GC.LAYOUT_GROUPS.items():
        assert rows[ix[nm], 5] == ix[nm] and rows[ix[nm], 6] == M and rows[ix[nm], 1] <= 8
    assert rows[ix["corner_a"], 40] == 1 and rows[ix["r12"], 36:40].tolist() == [108.0, 136.0, 48.0, 72.0] and rows[ix["chain3_b"], 42] == 2


def test_the_structure_of_the_edge_cases():
    g = GC.edge()
    rows = GC.reference(g)[0][0]
    ix = {nm: i for i, nm in enumerate(g.names)}
    for nm, (st, M) in GC.EDGE_EXPECT.items():
        r = rows[ix[nm]]
        assert (r[0] in (0.0, 2.0) if st is None else r[0] == st) and r[6] == M, (nm, r[:8])
    assert rows[ix["share_a"], 41] > 0 and rows[ix["hole_pair_a"], 41] > 0 and rows[ix["away_a"], 41] == 0
    assert rows[ix["r1_a"], 2] == 8 and np.array_equal(rows[ix["bad_b"], 8:14], g.jobs[ix["bad_b"], 5:11]) and rows[ix["bad_a"], 2] > 13
    assert np.array_equal(rows[ix["chain5_3"], 8:14], g.jobs[ix["chain5_3"], 5:11]) and rows[ix["chain5_3"], 5:8].tolist() == [ix["chain5_0"], 5, 3]
    valid = np.isfinite(g.map) & (g.map != 0)
    assert (~valid[79:92, 94:112]).sum() == 6 and rows[ix["invalid_a"], 2] == rows[ix["share_a"], 2] + rows[ix["share_a"], 41] - 6
    a, b = rows[[ix["peak_pair_a"], ix["peak_pair_b"]]], rows[[ix["neg_pair_a"], ix["neg_pair_b"]]]
    same = [0, 1, 2, 3, 4, 6, 7, 8, 10, 11, 12, 13] + list(range(14, 36))
    assert np.array_equal(a[:, same], b[:, same]) and np.all(np.abs(a[:, 9] + 40.0 - b[:, 9]) <= 1e-12)
    # both sides of the staging switch are what they are meant to be
    lo, hi = GC.reference(GC.stage_lo())[0][0], GC.reference(GC.stage_hi())[0][0]
    assert (lo[0, 37] - lo[0, 36] + 1) * (lo[0, 39] - lo[0, 38] + 1) == 6161 <= GR.LDS_MAX < 10611 == (hi[0, 37] - hi[0, 36] + 1) * (hi[0, 39] - hi[0, 38] + 1)


# ---- the tolerance
def test_the_measured_tolerance_and_the_left_out_share():
    worst = worst_c = 0.0
    for g in GC.groups():
        res, _ = GC.reference(g)
        out, gj = GC.excluded(g), GC.group_jobs(res)
        keep = gj & ~np.isin(g.names, GC.STATUS_ONLY)
        for e in np.nonzero(keep)[0]:                         # no drawn job on which the variants disagree
            assert len({r[e, 0] for r in res}) == 1, (g.name, g.names[e])
        if g.max_iter > 1:
            assert not (out & keep).any(), (g.name, [g.names[e] for e in np.nonzero(out & keep)[0]])      # no drawn case is left out
        w, wc, _ = GR.spread(res, keep)
        worst, worst_c = max(worst, w), max(worst_c, wc)
    for seed, njobs_min in zip(GC.SEEDS, (45, 50, 48)):
        g = GC.random(seed)
        res, cond = GC.reference(g)
        out, gj = GC.excluded(g), GC.group_jobs(res)
        njobs = len({int(r[5]) for r in res[0][gj]})
        left = len({int(r[5]) for r in res[0][gj & out]})
        w, wc, n0 = GR.spread(res, gj & ~out)
        print("filtered random scene, seed %d: %d jobs, %d group jobs, %d left out, all variants converged on %d rows, spread %.3g (C %.3g), cond(H) <= %.3g" % (
            seed, len(g.names), njobs, left, n0, w, wc, cond[gj].max()))
        assert njobs >= njobs_min and left <= GC.LEFT_OUT_MAX * njobs and n0 >= 0.95 * gj.sum()
        worst, worst_c = max(worst, w), max(worst_c, wc)
    print("largest spread between two variants: %.4g (MEASURED %.4g, TOL %.4g); of C %.4g (MEASURED_C %.4g, TOL_C %.4g)" % (
        worst, GR.MEASURED, GR.TOL, worst_c, GR.MEASURED_C, GR.TOL_C))
    assert 0.9 * GR.MEASURED <= worst <= GR.MEASURED and GR.TOL == 16 * GR.MEASURED
    assert 0.9 * GR.MEASURED_C <= worst_c <= GR.MEASURED_C and GR.TOL_C == 16 * GR.MEASURED_C
    assert GR.VARIANTS is BR.VARIANTS and "%.3g" % GR.TOL in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- config, plan() and the command line
def test_peakgroup_config():
    assert measure.peakgroup_config({}) == 1.5 and not measure.wants_peak_groups({})
    assert measure.wants_peak_groups({"fit_peak_groups": True}) and not measure.wants_peak_groups({"fit_peak_groups": False})
    assert measure.peakgroup_config({"fit_peaks_link": "0.75"}) == 0.75 and measure.peakgroup_config({"fit_peaks_link": 2}) == 2.0
    for bad in (0.0, -1.0, float("nan"), float("inf"), 2.0000001):
        with pytest.raises(ValueError):
            measure.peakgroup_config({"fit_peaks_link": bad})
    assert measure.peakgroup_config({}) * measure.peakfit_config({})[0] == 9.0         # with R = 6 it links entries closer than 9 px


def test_plan_with_and_without_the_switch():
    from test_measure_chain_cpu import IMPLIED
    for flag, steps in IMPLIED.items():
        assert measure.plan({flag: True}) == steps == measure.plan({flag: True, "fit_peak_groups": False}), flag
        assert set(measure.plan({flag: True, "fit_peak_groups": True})) == set(steps) | set(PEAK_STEPS)
    assert measure.plan({}) == () == measure.plan({"fit_peak_groups": False, "fit_peaks_link": -1})
    assert measure.plan({"fit_peak_groups": True}) == PEAK_STEPS == measure.plan({"fit_peaks": True}) == measure.plan({"fit_peak_groups": True, "fit_peaks": True})
    assert not measure.wants_peaks({"fit_peak_groups": True}) and not measure.wants_peak_fits({"fit_peak_groups": True})


def test_flags_parse_and_imply():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import run
    w = "--weights=seeded:l:5"
    base = run.measure_config(run.parse_args([w]))
    assert (base["fit_peak_groups"], base["fit_peaks_link"], base["fit_peaks"]) == (False, 1.5, False)
    assert measure.plan(base) == () and not measure.wants_peak_groups(base)
    args = run.parse_args([w, "--fit_peak_groups"])             # alone: the single fits and the pixel search come with it
    config = run.measure_config(args)
    assert measure.wants_peak_groups(config) and measure.wants_peak_fits(config) and config["residual_peaks"] is True and not config["residual_holes"]
    assert measure.plan(config) == PEAK_STEPS and args.residual_map and args.bkg_map and args.fit_components and not config["peak_apertures"]
    config = run.measure_config(run.parse_args([w, "--fit_peak_groups", "--residual_scales=3", "--fit_peaks_link", "0.5"]))
    assert config["fit_peaks"] is True and config["residual_peaks"] is False and measure.peakgroup_config(config) == 0.5
    for bad in (["--fit_peaks_link=0"], ["--fit_peaks_link=-1"], ["--fit_peaks_link=nan"], ["--fit_peaks_link=2.5"], ["--fit_peaks_radius=0"]):
        with pytest.raises(SystemExit):
            run.parse_args([w, "--fit_peak_groups"] + bad)
    with pytest.raises(SystemExit):
        run.parse_args([w, "--fit_peaks_link=abc"])
    assert run.parse_args([w, "--fit_peaks", "--fit_peaks_link=-1"]).fit_peak_groups is False       # without the switch the value is not looked at
    for flag in ("fit_peak_groups", "fit_peaks_link"):
        assert "--" + flag in run.__doc__ and flag in run.MEASURE_KEYS, flag
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--fit_peak_groups" in readme and "--fit_peaks_link" in readme and "gblend_" in readme


def test_exports():
    assert {"cy_fit_peak_groups", "cy_peakgroup_kernel_ms"} <= set(L.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "caesar_yolo_hip.h")).read()
    assert any(line.split()[:3] == ["#define", "CY_PGRP_FIELDS", "44"] for line in hdr.split("\n")) and L.CY_PGRP_FIELDS == 44 == GR.FIELDS
    assert "int cy_fit_peak_groups(cy_ctx* ctx, const float* d_map, int MH, int MW, const double* h_jobs" in hdr
    assert "int cy_peakgroup_kernel_ms(const cy_ctx* ctx, double* out_ms);" in hdr
    assert len(L.PGRP_NAMES) == L.CY_PGRP_FIELDS and L.PGRP_NAMES == GR.NAMES and L.PGRP_NAMES[:36] == L.BLEND_NAMES
    lib = L.load()
    assert hasattr(lib, "cy_fit_peak_groups") and hasattr(lib, "cy_peakgroup_kernel_ms")
    csrc = os.path.join(ROOT, "caesar_yolo_amd", "csrc")
    jobs, multi, disc, blend, pf, pg, plan = (open(os.path.join(csrc, f)).read() for f in (
        "cy_measure_jobs.h", "cy_lm_multi.h", "cy_disc.h", "cy_blend.hip", "cy_peakfit.hip", "cy_peakgroup.hip", "cy_measure_plan.cpp"))
    assert "PGRP_FIELDS = 44;" in jobs and "struct PeakGroupJob {" in jobs
    for text in ("void multi_sweep(", "bool factor(MultiSmem& s", "bool lm_solve(MultiSmem& s", "void pair_of(int q"):      # stated once, shared
        assert text in multi and text not in blend and text not in pg
    assert "struct Disc {" in disc and "bool member(const Disc& d" in disc and "struct Disc" not in pf and "struct Disc" not in pg
    for src in (blend, pg):
        assert '#include "cy_lm_multi.h"' in src and "multi_sweep(" in src and "multi_iterate(" in src and "#pragma clang fp contract(off)" in src
    assert '#include "cy_disc.h"' in pf and '#include "cy_disc.h"' in pg
    assert "atomic" not in pg.replace("no atomics", "") and "asm" not in pg.replace("inline assembly", "")
    assert "const char* plan_peak_groups(" in plan and plan.count("std::sort(") == 1          # one sorted-by-column stretch, shared
    import __graft_entry__ as ge
    assert "cy_peakgroup.hip" in ge.HIP_SOURCES
    from caesar_yolo_amd.model import HipDetector
    assert callable(HipDetector.fit_peak_groups) and callable(HipDetector.peakgroup_kernel_ms)


# ---- annotate_peak_groups on hand-made rows
def _row(status, group=0, size=2, slot=0, p=(2.0, 10.0, 20.0, 0.5, 0.1, 0.25), niter=7, npix=90, F=4.0, nex=3, nlinked=1, clipped=1):
    r = np.zeros(L.CY_PGRP_FIELDS)
    r[0] = status
    if status in (1, 5):
        r[36:40] = -1.0
        return r
    r[5:8] = [group, size, slot]
    r[36:43] = [4, 22, 14, 26, clipped, 0, nlinked]
    if status == 6:
        return r
    if status == 7:
        r[8:14] = p
        return r
    r[2], r[8:14], r[41] = npix, p, nex
    if status in (0, 2):
        r[1], r[3], r[4], r[14] = niter, F, 1e-5, 1.0
        C = np.diag([0.02, 0.01, 0.03, 0.004, 0.002, 0.001]) + 1e-4
        r[15:36] = C[np.triu_indices(6)]
    return r


def test_annotate_peak_groups_on_hand_made_rows():
    from caesar_yolo_amd.wcs import WCS
    wcs = WCS(json.loads(str(Z["wcs_header"])))
    # entries 0, 1: a fitted pair; 2: alone; 3, 4: statuses 1 and 5; 5, 6: a pair that was not fitted (3, 4); 7: of a group above the limit; 8: limit reached
    rows = np.stack([_row(0, 0, 2, 0), _row(0, 0, 2, 1, p=(1.0, 14.0, 21.0, 0.4, 0.0, 0.3)), _row(6, 2, 1, 0, nlinked=0), _row(1), _row(5),
                     _row(3, 5, 2, 0), _row(4, 5, 2, 1), _row(7, 7, 5, 0), _row(2, 8, 2, 0)])
    statuses = [0, 0, 6, 1, 5, 3, 4, 7, 2]
    rms = np.full(len(statuses), 0.5)
    jobs = np.array([[10.0, 20.0, 6.0, 0.125, 1.0, 2.0, 10.0, 20.0, 0.4, 0.0, 0.4]] * len(statuses))
    head = ("gblend_group", "gblend_size", "gblend_slot", "gblend_status", "gblend_niter", "gblend_npix", "gblend_nexcluded")
    for sign in (1.0, -1.0):
        entries = [{"x": 1.0, "keep": i} for i in range(len(statuses))]
        measure.annotate_peak_fits(entries, np.stack([pfit_row(0)] * len(statuses)), jobs, rms, sign, 12.5, wcs, (3.0, 4.0))
        before = json.loads(json.dumps(entries))
        out = measure.annotate_peak_groups(entries, rows, rms, sign, 12.5, wcs, (3.0, 4.0))
        assert out is entries and all(tuple(d) == tuple(d0) + measure.GBLEND_KEYS and {k: d[k] for k in d0} == d0 for d, d0 in zip(entries, before))
        for i, (d, s) in enumerate(zip(entries, statuses)):
            assert d["gblend_status"] == s and type(d["gblend_npix"]) is int
            if s in (1, 5):
                assert (d["gblend_group"], d["gblend_size"], d["gblend_slot"]) == (None, None, None)
            else:
                assert (d["gblend_group"], d["gblend_size"], d["gblend_slot"]) == (int(rows[i, 5]), int(rows[i, 6]), int(rows[i, 7]))
            if s in (0, 2):
                ref = {}
                measure._gaussian_keys(ref, "blend_", rows[i][:36], measure.BLEND.F, measure._BLEND_PARAMS, measure.blend_covariance, 0.5, 12.5, wcs, 3.0, 4.0)
                want = {"g" + k: v for k, v in ref.items()}
                want["gblend_peak"], want["gblend_flux"] = sign * want["gblend_peak"], sign * want["gblend_flux"]
                assert {k: d[k] for k in want} == want and d["gblend_chi2"] == 16.0 and d["gblend_flux_err"] > 0 and d["gblend_ra"] is not None
                assert d["gblend_peak_err"] == 0.5 * np.sqrt(rows[i, 15]) and (d["gblend_niter"], d["gblend_npix"], d["gblend_nexcluded"]) == (7, 90, 3)
            elif s == 6:
                assert all(d["gblend_" + k[5:]] == d[k] for k in measure.GFIT_KEYS[measure.GFIT_KEYS.index("gfit_chi2"):]) and d["gblend_peak"] == sign * 2.0
                assert (d["gblend_niter"], d["gblend_npix"], d["gblend_nexcluded"]) == (0, 0, 0)
            else:
                assert all(d[k] is None for k in measure.GBLEND_KEYS if k not in head), s
        assert entries[0]["gblend_x"] == 10.0 and entries[1]["gblend_x"] == 14.0 and entries[1]["gblend_slot"] == 1
    assert set(k[len("gblend_"):] for k in measure.GBLEND_KEYS[7:]) == set(k[len("gfit_"):] for k in measure.GFIT_KEYS[9:])      # the namesakes
    # no beam, no WCS, no noise: the keys that need them stay None
    d = measure.annotate_peak_groups([{}], rows[:1], [float("nan")], 1.0, 0, None)[0]
    assert d["gblend_flux"] is None and d["gblend_ra"] is None and d["gblend_chi2"] is None and d["gblend_peak_err"] is None and d["gblend_major"] > d["gblend_minor"] > 0
    # entries without a job: every key None; the group is the index of the entry in its list
    entries = [{"strongest": t != 1} for t in range(3)]
    measure.annotate_peak_groups(entries, rows[:2], rms[:2], 1.0, 12.5, None, select=[0, 2])
    assert all(entries[1][k] is None for k in measure.GBLEND_KEYS) and entries[2]["gblend_group"] == 0 and entries[2]["gblend_slot"] == 1
    measure.annotate_peak_groups(entries, np.stack([_row(0, 1, 2, 0), _row(0, 1, 2, 1)])[::-1], rms[:2], 1.0, 12.5, None, select=[0, 2])
    assert entries[0]["gblend_group"] == 2 == entries[2]["gblend_group"]
    # three group jobs (the fitted pair, the pair that was not fitted, the one at the limit) with five rows, one converged, one group above the limit
    assert measure.peak_group_stats(rows) == (3, 5, 1, 7.0, 7, 1) and measure.peak_group_stats(np.zeros((0, L.CY_PGRP_FIELDS))) == (0, 0, 0, 0.0, 0, 0)
    json.dumps(entries)


def test_peak_group_jobs():
    jobs = np.array([[10.0, 20.0, 6.0, 0.125, 1.0, 2.0, 10.0, 20.0, 0.4, 0.0, 0.4]] * 4)
    rows = np.stack([pfit_row(0, p=(3.0, 10.5, 19.5, 0.3, 0.05, 0.2)), pfit_row(2, p=(4.0, 11.0, 21.0, 0.5, 0.0, 0.5)), pfit_row(3), pfit_row(5)])
    got = measure.peak_group_jobs(jobs, rows)
    assert got[:, :5].tolist() == jobs[:, :5].tolist() and got[0, 5:].tolist() == [3.0, 10.5, 19.5, 0.3, 0.05, 0.2] and got[1, 5:].tolist() == [4.0, 11.0, 21.0, 0.5, 0.0, 0.5]
    assert got[2:].tolist() == jobs[2:].tolist() and jobs[0, 5] == 2.0         # not fitted: the start that was asked for; the input is left alone


# ---- Chain.run on the replay detector
class PeakGroupReplay(PeakFitReplay):
    """PeakFitReplay plus fit_peak_groups: hand-made rows (pairs of jobs 0-1, 2-3, ..; a last odd job is alone), every argument kept."""

    def __init__(self, scenario):
        PeakFitReplay.__init__(self, scenario)
        self.pgrp_args = []

    def fit_peak_groups(self, map_dev, jobs, link=1.5, max_iter=64):
        self.calls.append("fit_peak_groups")
        jobs = np.array(jobs, np.float64)
        self.pgrp_args.append(dict(map_dev=map_dev, jobs=jobs, link=link, max_iter=max_iter))
        n = len(jobs)
        return np.stack([_row(6, i, 1, 0, nlinked=0) if i == n - 1 and n % 2 else _row(0, i - i % 2, 2, i % 2, p=(j[5], j[6] + 0.25, j[7], 0.5, 0.1, 0.25))
                         for i, j in enumerate(jobs)])

    def peakgroup_kernel_ms(self):
        return KERNEL_MS


def test_chain_without_the_switch_is_what_it_was():
    s, kw = _setup("B")
    config = dict(s["config"], fit_peaks=True, residual_peaks=True, residual_holes=True, residual_scales=3, residual_peaks_max=10)
    det0, stats0 = PeakFitReplay("B"), {}                     # has no fit_peak_groups: a call would raise
    chain0 = measure.Chain(det0, np.zeros(SHAPE, np.float32), s["sources"], config, **kw).run(measure.plan(config), stats0)
    s1, _ = _setup("B")
    det1, stats1 = PeakFitReplay("B"), {}
    extra = {"fit_peak_groups": False, "fit_peaks_link": -3.0}         # not looked at without the switch
    chain1 = measure.Chain(det1, np.zeros(SHAPE, np.float32), s1["sources"], dict(config, **extra), **kw).run(measure.plan(dict(config, **extra)), stats1)
    assert det1.calls == det0.calls and det0.calls[-1] == "fit_peaks" and set(stats1) == set(stats0) and not set(stats0) & PEAKGROUP_STATS
    assert chain0.peakgroup_rows is None and chain0.peakgroup_stats is None
    lists0, lists1 = measure.peak_lists(chain0), measure.peak_lists(chain1)
    assert json.dumps(lists0) == json.dumps(lists1) and not [k for lst in lists0.values() for d in lst for k in d if k.startswith("gblend_")]
    assert json.dumps(s["sources"]) == json.dumps(s1["sources"])


@pytest.mark.parametrize("searches", ["peaks", "all", "none"])
def test_chain_with_the_switch(searches):
    s, kw = _setup("B")
    on = {"peaks": dict(residual_peaks=True), "all": dict(residual_peaks=True, residual_holes=True, residual_scales=4), "none": {}}[searches]
    config = dict(s["config"], fit_peak_groups=True, fit_peaks_link=1.25, fit_peaks_max_iter=33, residual_peaks_max=10, **on)      # fit_peaks is implied
    steps = measure.plan(config)
    assert steps == measure.plan(dict(config, fit_peaks=True, fit_peak_groups=False))
    s0, _ = _setup("B")
    det0, stats0 = PeakFitReplay("B"), {}
    chain0 = measure.Chain(det0, np.zeros(SHAPE, np.float32), s0["sources"], dict(config, fit_peaks=True, fit_peak_groups=False), **kw).run(steps, stats0)
    det, stats = PeakGroupReplay("B"), {}
    chain = measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], config, **kw).run(steps, stats)
    names = {"peaks": ["residual_peaks"], "all": ["residual_peaks", "residual_holes", "residual_scale_peaks"], "none": []}[searches]
    # the order: everything the run with --fit_peaks alone called, then one call per list
    assert det.calls[:len(det0.calls)] == det0.calls and det.calls[len(det0.calls):] == ["fit_peak_groups"] * len(names)
    lists, lists0 = measure.peak_lists(chain), measure.peak_lists(chain0)
    assert list(chain.peakgroup_rows) == names == list(chain.peakfit_rows)
    bx, by = kw["box_origin"]
    every = []
    for name, a in zip(names, det.pgrp_args):
        entries, sign = lists[name], -1.0 if name == "residual_holes" else 1.0
        select, single, asked = chain.peakfit_select[name], chain.peakfit_rows[name], chain.peakfit_jobs[name]
        assert a["map_dev"] is chain.resid and a["link"] == 1.25 and a["max_iter"] == 33 and a["jobs"].shape == (len(select), L.CY_PFIT_JOB_FIELDS)
        # the start of every job the single fit ended on (the replay: status 0 and 2 of 0, 2, 4) is that fit's, in the pixel frame
        for t in range(len(select)):
            assert a["jobs"][t, :5].tolist() == asked[t, :5].tolist()
            assert a["jobs"][t, 5:].tolist() == (single[t, 5:11] if single[t, 0] in (0, 2) else asked[t, 5:]).tolist()
        assert np.array_equal(chain.peakgroup_jobs[name], a["jobs"])
        rows = chain.peakgroup_rows[name]
        moved = rows.copy()
        moved[:, [9, 36, 37]] += bx
        moved[:, [10, 38, 39]] += by
        want = measure.annotate_peak_groups([dict(d) for d in lists0[name]], moved, np.zeros(len(select)), sign, kw["beam_area"], kw["wcs"], kw["wcs_origin"], select)
        for i, (d, w, d0) in enumerate(zip(entries, want, lists0[name])):
            assert tuple(d) == tuple(d0) + measure.GBLEND_KEYS and {k: d[k] for k in d0} == d0 and d == w
            if i not in select:
                assert all(d[k] is None for k in measure.GBLEND_KEYS)
        first = entries[select[0]]
        if len(select) > 1:
            assert first["gblend_status"] == 0 and first["gblend_group"] == select[0] and first["gblend_x"] == first["gfit_x"] + 0.25 and (first["gblend_peak"] > 0) == (sign > 0)
        if len(select) % 2:
            last = entries[select[-1]]
            assert last["gblend_status"] == 6 and last["gblend_group"] == select[-1] and last["gblend_x"] == last["gfit_x"] and last["gblend_peak"] == last["gfit_peak"]
        every.append(rows)
    assert json.dumps(s["sources"]) == json.dumps(s0["sources"])
    old = {k for k in stats if k not in PEAKGROUP_STATS}
    assert set(stats) == old | PEAKGROUP_STATS and old == set(stats0) and PEAKFIT_STATS <= old
    every = np.concatenate(every) if every else np.zeros((0, L.CY_PGRP_FIELDS))
    njobs = int(((every[:, 0] == 0) & (every[:, 7] == 0)).sum())
    assert (stats["peakgroup_jobs"], stats["peakgroup_members"], stats["peakgroup_converged"], stats["peakgroup_over_limit"]) == (njobs, 2 * njobs, njobs, 0)
    launched = sum(bool((chain.peakgroup_rows[n][:, 0] == 0).any()) for n in names)
    assert stats["peakgroup_kernel_ms"] == launched * KERNEL_MS and stats["peakgroup_ms"] >= 0.0
    assert stats["peakgroup_niter_max"] == (7 if njobs else 0) and stats["peakgroup_niter_mean"] == (7.0 if njobs else 0.0)
    json.dumps(lists)


def test_chain_fits_no_group_without_the_residual_step():
    s, kw = _setup("B")
    config = dict(s["config"], fit_peak_groups=True, residual_peaks=True)
    det, stats = PeakGroupReplay("B"), {}
    steps = tuple(k for k in measure.plan(config) if k not in ("blend", "residual"))
    chain = measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], config, **kw).run(steps, stats)
    assert "fit_peak_groups" not in det.calls and "fit_peaks" not in det.calls and not set(stats) & PEAKGROUP_STATS and chain.peakgroup_rows is None
    with pytest.raises(ValueError):
        measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], dict(config, fit_peaks_link=2.5), **kw)
