"""The second residual on the CPU: the two statements of the reference of cy_disc_residuals against each other, the host side of
--subtract_peaks on hand-made rows (peak_render_selection, annotate_peak_residuals), the plan, the flags and the exports, Chain.run on
the replay detectors, and the whole chain on the numpy references for a scene with a blended pair."""
import json
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import disc_residual_cases as DC
import disc_residual_ref as DR
import peakfit_ref as PR
import peakgroup_ref as GR
import peaks_chain_ref as CR
from caesar_yolo_amd import lib as L
from caesar_yolo_amd import measure
from test_measure_chain_cpu import KERNEL_MS, SHAPE, _setup
from test_peakfit_cpu import PEAKFIT_STATS, PeakFitReplay
from test_peakfit_cpu import _row as pfit_row
from test_peakgroup_cpu import PEAKGROUP_STATS, PeakGroupReplay
from test_peakgroup_cpu import _row as pgrp_row
from test_peaks_cpu import PEAK_STEPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBTRACT_STATS = {"subtract_ms", "subtract_render_kernel_ms", "disc_residual_kernel_ms", "subtract_selected", "subtract_rendered", "subtract_wandered",
                  "subtract_duplicates", "left_peaks_kernel_ms", "left_peaks", "left_holes", "left_truncated"}
PLANTED = ((30.0, 100.2, 60.4), (20.0, 104.1, 63.5))         # amplitude, x, y of the planted pair of sigma 1.6 px
PLANTED_SIGMA = 1.6
PLACES = (CR.UNBOXED, (100, 60), (104, 63))                  # what the pixel search lists on that scene


# ---- the reference, stated twice
@pytest.mark.parametrize("name", [g.name for g in DC.groups()])
def test_the_two_restatements_agree(name):
    g = DC.by_name(name)
    rows, ab = DR.disc_residuals(g.map, g.model, g.jobs)
    rows2, ab2 = DR.disc_residuals_loops(g.map, g.model, g.jobs)
    assert rows.shape == (len(g.names), DR.FIELDS) == rows2.shape
    assert np.array_equal(rows[:, DR.EXACT], rows2[:, DR.EXACT])
    DR.compare(rows2, rows, ab, g.names)                      # the sums: np.sum pairs its terms, the loops add them one by one
    assert np.allclose(ab, ab2, rtol=1e-12, atol=0.0)


def test_the_cases_hold_what_they_are_for():
    rows = {g.name: dict(zip(g.names, DR.disc_residuals(g.map, g.model, g.jobs)[0])) for g in DC.groups()}
    F = SimpleNamespace(**{n: i for i, n in enumerate(DR.NAMES)})
    assert DR.NAMES == L.DRES_NAMES and DR.FIELDS == L.CY_DRES_FIELDS
    t = rows["tiny_1x1"]
    assert t["on_it"][[F.status, F.npix, F.sum, F.maxabs, F.x_max, F.y_max, F.model_sum]].tolist() == [0, 1, 2.0, 2.0, 0, 0, 0.5]
    assert t["off"][F.status] == 5 and t["off"][F.wx0] == -1 and t["off"][F.x_max] == -1 and t["off"][F.npix] == 0
    a = rows["tiny_1x7"]["all"]
    assert a[F.npix] + a[F.nexcluded] == 5 and a[F.clipped] == 1 and a[F.nneigh] == 2      # 0 and NaN are not valid; the two others take their shares
    o = rows["odd_70x75"]
    assert o["r1_int"][F.npix] == 5 and o["r1_half"][F.npix] == 0 + 4 and o["r6_inside"][F.clipped] == 0
    assert o["r6_corner"][F.clipped] == 1 == o["r6_corner0"][F.clipped] and o["r6_outside"][F.status] == 0 and o["r6_outside"][F.wx0] == 0
    assert o["r6_below"][F.status] == 5 == o["r6_far"][F.status] == o["r6_nan_centre"][F.status]
    assert all(o[k][F.status] == 1 for k in ("r_nan", "r_zero", "r_257", "sign_zero", "bkg_inf")) and o["start_nan"][F.status] == 0
    for variant in ("main_64x96", "main_no_model", "main_offset"):
        m = rows[variant]
        assert m["pair_a"][F.nneigh] == 1 == m["pair_b"][F.nneigh] and m["pair_a"][F.nexcluded] > 0
        # the tie column x = 12 belongs to both: the two shares overlap in exactly the valid pixels of that column inside both discs
        assert m["pair_a"][F.npix] + m["pair_b"][F.npix] > 113 + m["pair_b"][F.nexcluded]
        assert m["coincident_a"][F.npix] == m["coincident_b"][F.npix] == 81 and m["coincident_a"][F.nexcluded] == 0
        assert m["r12"][F.nneigh] == 3 and m["r6_beside_r12"][F.nneigh] == 0 and m["r12"][F.nexcluded] > 0
        assert m["hole"][F.status] == 0 and m["invalid_inside"][F.npix] == 113 - 4
        assert m["no_valid_pixel"][[F.status, F.npix, F.maxabs, F.x_max, F.y_max]].tolist() == [0, 0, 0, -1, -1]
        assert m["equal_maxima"][[F.maxabs, F.x_max, F.y_max]].tolist() == [9.0, 62, 19]
        assert (m["pair_a"][F.model_sum] == 0.0) == (variant == "main_no_model")
    assert all(r[F.nneigh] == 8 for r in rows["crowded"].values())            # nine others within one radius: crowded
    r = rows["r256_520x515"]["r256"]
    assert r[[F.wx0, F.wx1, F.wy0, F.wy1]].tolist() == [1, 513, 2, 514] and r[F.npix] > 180000 and r[F.nneigh] == 1 and r[F.clipped] == 0      # 513 x 513
    assert rows["empty"] == {}


def test_the_largest_window_is_reached():
    """An R = 256 job on an integer centre inside the image: the 513 x 513 window."""
    win = PR.window(257.0, 258.0, 256.0, 0.0, 1.0, 520, 515)
    assert win == (0, 1, 513, 2, 514, 0)


# ---- peak_render_selection on hand-made rows
def _chain(fits, jobs, groups=None, select=None):
    """What peak_render_selection() reads of a chain: {name: rows}, {name: jobs}, {name: group rows} or None."""
    select = select or {k: list(range(len(v))) for k, v in fits.items()}
    return SimpleNamespace(peakfit_rows={k: np.stack(v) for k, v in fits.items()}, peakfit_jobs={k: np.array(v, np.float64) for k, v in jobs.items()},
                           peakgroup_rows=None if groups is None else {k: np.stack(v) for k, v in groups.items()}, peakfit_select=select)


def _job(cx, cy, R=6.0, sign=1.0):
    return [cx, cy, R, 0.0, sign, 1.0, cx, cy, 0.4, 0.0, 0.4]


def test_selection_prefers_the_group_fit_and_skips_what_was_not_fitted():
    P1, P2 = (3.0, 10.5, 20.5, 0.3, 0.05, 0.2), (4.0, 10.25, 20.0, 0.5, 0.0, 0.5)
    fits = {"residual_peaks": [pfit_row(0, p=P1)] * 4 + [pfit_row(2, p=P1)] + [pfit_row(s, p=P1) for s in (3, 4, 1, 5)]}
    jobs = {"residual_peaks": [_job(10.0, 20.0)] * 9}
    groups = {"residual_peaks": [pgrp_row(0, 0, 2, 0, p=P2), pgrp_row(2, 0, 2, 1, p=P2), pgrp_row(6, 2, 1, 0), pgrp_row(3, 3, 2, 0), pgrp_row(7, 4, 5, 0, p=P2),
                                 pgrp_row(0, 5, 2, 0, p=P2), pgrp_row(4, 5, 2, 1), pgrp_row(1), pgrp_row(5)]}
    select = {"residual_peaks": [0, 2, 3, 5, 6, 7, 8, 9, 11]}         # entry indices are not row indices
    comp, index, counts = measure.peak_render_selection(_chain(fits, jobs, groups, select))
    # rows 0, 1: the group fit (0, 2); row 2: status 6 carries no parameters, the single fit; rows 3, 4: group 3 / 7, the single fit (0, 2);
    # row 5: the group fit although the single one was not fitted; rows 6, 7, 8: neither
    assert index == [("residual_peaks", i) for i in (0, 2, 3, 5, 6, 7)] and counts["sources"] == ["group", "group", "single", "single", "single", "group"]
    assert comp.tolist() == [list(P2), list(P2), list(P1), list(P1), list(P1), list(P2)] and (counts["wandered"], counts["duplicates"]) == (0, 0)
    # without the groups: the single fits alone
    comp, index, counts = measure.peak_render_selection(_chain(fits, jobs, None, select))
    assert index == [("residual_peaks", i) for i in (0, 2, 3, 5, 6)] and set(counts["sources"]) == {"single"} and comp.tolist() == [list(P1)] * 5
    # no list at all
    comp, index, counts = measure.peak_render_selection(_chain({}, {}))
    assert comp.shape == (0, 6) and index == [] and counts == {"wandered": 0, "duplicates": 0, "sources": []}


def test_selection_wander_rule_at_the_radius():
    R = 6.0
    up = math.nextafter(R, math.inf)
    # the job's centre is (0, 0), so that the differences the rule forms are exactly the numbers written here
    cases = [(R, 0.0, True), (up, 0.0, False), (0.0, -R, True), (0.0, -up, False), (3.6, 4.8, None), (float("nan"), 0.0, False)]
    kept = []
    for x, y, keep in cases:
        fits = {"residual_peaks": [pfit_row(0, p=(2.0, x, y, 0.5, 0.1, 0.25))]}
        comp, index, counts = measure.peak_render_selection(_chain(fits, {"residual_peaks": [_job(0.0, 0.0, R)]}))
        dx, dy = x, y
        want = keep if keep is not None else dx * dx + dy * dy <= R * R        # 3.6^2 + 4.8^2 against 36 as float64 rounds it
        assert (len(index) == 1) == want and counts["wandered"] == (0 if want else 1), (x, y)
        kept.append(want)
    assert kept[:4] == [True, False, True, False]


def test_selection_duplicate_rule_at_the_radius_and_hole_sign():
    P = (2.0, 0.0, 0.0, 0.5, 0.1, 0.25)                        # fitted centres on the axes, so that the differences the rule forms are exact
    fits = {"residual_peaks": [pfit_row(0, p=P)], "residual_holes": [pfit_row(0, p=(1.5, 100.0, 0.0, 0.4, 0.0, 0.4))]}
    jobs = {"residual_peaks": [_job(0.0, 0.0)], "residual_holes": [_job(100.0, 0.0, 6.0, -1.0)]}
    R = 24.0
    up = math.nextafter(R, math.inf)
    # scale jobs of R = 24 around centres at exactly R and one ulp beyond R from the pixel peak at (0, 0), and from the hole at (100, 0)
    scale_centres = [(R, 0.0), (-up, 0.0), (0.0, R), (100.0, R), (100.0, -up)]
    for k, (cx, cy) in enumerate(scale_centres):
        f = dict(fits, residual_scale_peaks=[pfit_row(0, p=(5.0, cx + 1.0, cy - 1.0, 0.01, 0.0, 0.01))])
        j = dict(jobs, residual_scale_peaks=[_job(cx, cy, R)])
        comp, index, counts = measure.peak_render_selection(_chain(f, j, None, dict(residual_peaks=[0], residual_holes=[0], residual_scale_peaks=[3])))
        dup = k in (0, 2, 3)
        assert counts["duplicates"] == int(dup) and counts["wandered"] == 0, k
        assert index == [("residual_peaks", 0), ("residual_holes", 0)] + ([] if dup else [("residual_scale_peaks", 3)])
        assert comp[0].tolist() == list(P) and comp[1].tolist() == [-1.5, 100.0, 0.0, 0.4, 0.0, 0.4]      # the hole is rendered negative
        if not dup:
            assert comp[2].tolist() == [5.0, cx + 1.0, cy - 1.0, 0.01, 0.0, 0.01]
    # a pixel entry that was left out (it wandered) shadows no scale entry; the lists are walked in their fixed order whatever the dict's
    f = {"residual_scale_peaks": [pfit_row(0, p=(5.0, 50.0, 60.0, 0.01, 0.0, 0.01))], "residual_peaks": [pfit_row(0, p=(2.0, 57.0, 60.0, 0.5, 0.1, 0.25))]}
    j = {"residual_scale_peaks": [_job(50.0, 60.0, R)], "residual_peaks": [_job(50.0, 60.0)]}
    comp, index, counts = measure.peak_render_selection(_chain(f, j))
    assert index == [("residual_scale_peaks", 0)] and (counts["wandered"], counts["duplicates"]) == (1, 0)
    f["residual_peaks"] = [pfit_row(0, p=(2.0, 55.0, 60.0, 0.5, 0.1, 0.25))]
    comp, index, counts = measure.peak_render_selection(_chain(f, j))
    assert index == [("residual_peaks", 0)] and (counts["wandered"], counts["duplicates"]) == (0, 1)


# ---- annotate_peak_residuals on hand-made rows
def _dres(status, npix=50, s=5.0, ss=8.0, mx=1.5, x=12, y=23, model=25.0):
    r = np.zeros(L.CY_DRES_FIELDS)
    r[0] = status
    if status:
        r[[6, 7, 10, 11, 12, 13]] = -1.0
        return r
    r[1:9] = [npix, 3, s, ss, mx, x, y, model] if npix else [0, 3, 0.0, 0.0, 0.0, -1, -1, 0.0]
    r[10:16] = [4, 16, 17, 29, 1, 2]
    return r


def test_annotate_peak_residuals_on_hand_made_rows():
    rows = np.stack([_dres(0), _dres(0), _dres(0, npix=0), _dres(1), _dres(5), _dres(0), _dres(0)])
    rms = [0.5, 0.5, 0.5, 0.5, 0.5, 0.0, float("nan")]
    picked = {0: ("group", 0), 2: ("single", 2), 3: ("single", 3), 5: ("group", 1)}
    select = [0, 2, 3, 4, 5, 7, 8]
    entries = [{"x": 1.0, "keep": i} for i in range(9)]
    before = json.loads(json.dumps(entries))
    out = measure.annotate_peak_residuals(entries, rows, rms, picked, 12.5, (3.0, 4.0), select)
    assert out is entries and all(tuple(d) == tuple(d0) + measure.GRES_KEYS and {k: d[k] for k in d0} == d0 for d, d0 in zip(entries, before))
    assert all(entries[i][k] is None for i in (1, 6) for k in measure.GRES_KEYS)                    # never fitted: every key None
    d = entries[0]
    assert (d["gres_subtracted"], d["gres_source"], d["gres_render_status"], d["gres_npix"]) == (True, "group", 0, 50) and type(d["gres_npix"]) is int
    assert (d["gres_mean"], d["gres_rms"], d["gres_max"], d["gres_x_max"], d["gres_y_max"]) == (0.1, math.sqrt(8.0 / 50), 1.5, 15, 27)
    assert d["gres_ratio"] == math.sqrt(8.0 / 50) / 0.5 and d["gres_chi2"] == 32.0 and d["gres_model_flux"] == 2.0
    assert (entries[2]["gres_subtracted"], entries[2]["gres_source"], entries[2]["gres_render_status"]) == (True, "single", 2)      # capped half-width: rendered
    d = entries[3]                                            # chosen, skipped by the renderer (status 3), and no valid pixel in its share
    assert (d["gres_subtracted"], d["gres_source"], d["gres_render_status"], d["gres_npix"]) == (False, "single", 3, 0)
    assert all(d[k] is None for k in measure.GRES_KEYS[4:])
    for i in (4, 5):                                          # the planner's statuses 1 and 5
        d = entries[i]
        assert d["gres_npix"] == 0 and all(d[k] is None for k in measure.GRES_KEYS[4:]) and d["gres_subtracted"] is False and d["gres_source"] == (None if i == 4 else "group")
        assert d["gres_render_status"] == (None if i == 4 else 1)
    for i in (7, 8):                                          # rms 0 or NaN: the two keys that divide by it stay None
        d = entries[i]
        assert d["gres_ratio"] is None and d["gres_chi2"] is None and d["gres_rms"] == math.sqrt(8.0 / 50) and d["gres_model_flux"] == 2.0
        assert (d["gres_subtracted"], d["gres_source"], d["gres_render_status"]) == (False, None, None)
    d = measure.annotate_peak_residuals([{}], rows[:1], rms[:1], {}, 0)[0]      # no beam, no origin, select None
    assert d["gres_model_flux"] is None and (d["gres_x_max"], d["gres_y_max"]) == (12, 23) and d["gres_chi2"] == 32.0
    json.dumps(entries)


# ---- plan, flags, exports
def test_plan_with_and_without_the_switch():
    from test_measure_chain_cpu import IMPLIED
    for flag, steps in IMPLIED.items():
        assert measure.plan({flag: True}) == steps == measure.plan({flag: True, "subtract_peaks": False}), flag
        assert set(measure.plan({flag: True, "subtract_peaks": True})) == set(steps) | set(PEAK_STEPS)
    assert measure.plan({}) == () == measure.plan({"subtract_peaks": False})
    assert measure.plan({"subtract_peaks": True}) == PEAK_STEPS == measure.plan({"fit_peaks": True})
    assert measure.wants_subtract({"subtract_peaks": True}) and not measure.wants_subtract({}) and not measure.wants_peaks({"subtract_peaks": True})
    assert not measure.wants_peak_fits({"subtract_peaks": True})                # the chain implies the fits, the config key stays what it was


def test_flags_parse_and_imply():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import run
    w = "--weights=seeded:l:5"
    base = run.measure_config(run.parse_args([w]))
    assert base["subtract_peaks"] is False and measure.plan(base) == () and not measure.wants_subtract(base)
    args = run.parse_args([w, "--subtract_peaks"])             # alone: the single fits and the pixel search come with it
    config = run.measure_config(args)
    assert config["subtract_peaks"] is True and config["fit_peaks"] is True and config["residual_peaks"] is True and not config["fit_peak_groups"]
    assert not config["residual_holes"] and config["residual_scales"] == 0 and measure.plan(config) == PEAK_STEPS and args.residual_map and args.bkg_map
    config = run.measure_config(run.parse_args([w, "--subtract_peaks", "--fit_peak_groups", "--residual_scales=3"]))
    assert config["fit_peaks"] and config["fit_peak_groups"] and config["residual_peaks"] is False and measure.plan(config) == PEAK_STEPS
    with pytest.raises(SystemExit):
        run.parse_args([w, "--subtract_peaks", "--fit_peaks_radius=-1"])       # the implied switch checks its values
    assert "--subtract_peaks" in run.__doc__ and "subtract_peaks" in run.MEASURE_KEYS
    assert "--subtract_peaks" in open(os.path.join(ROOT, "README.md")).read()


def test_exports():
    assert {"cy_disc_residuals", "cy_disc_residual_kernel_ms", "cy_render_signed_gaussians"} <= set(L.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "caesar_yolo_hip.h")).read()
    assert any(line.split()[:3] == ["#define", "CY_DRES_FIELDS", "16"] for line in hdr.split("\n")) and L.CY_DRES_FIELDS == 16 == DR.FIELDS
    assert "int cy_disc_residuals(cy_ctx* ctx, const float* d_map, const float* d_model /* or NULL */, int MH, int MW," in hdr
    assert "int cy_disc_residual_kernel_ms(const cy_ctx* ctx, double* out_ms);" in hdr
    assert len(L.DRES_NAMES) == L.CY_DRES_FIELDS and L.DRES_NAMES == DR.NAMES
    lib = L.load()
    assert hasattr(lib, "cy_disc_residuals") and hasattr(lib, "cy_disc_residual_kernel_ms") and hasattr(lib, "cy_render_signed_gaussians")
    assert "int cy_render_signed_gaussians(cy_ctx* ctx, const float* d_img, int MH, int MW, const double* h_comp" in hdr
    jobs = open(os.path.join(ROOT, "caesar_yolo_amd", "csrc", "cy_measure_jobs.h")).read()
    assert "DRES_FIELDS = 16;" in jobs
    import __graft_entry__ as ge
    assert "cy_disc_residual.hip" in ge.HIP_SOURCES
    from caesar_yolo_amd.model import HipDetector
    assert callable(HipDetector.disc_residuals) and callable(HipDetector.disc_residual_kernel_ms)


# ---- Chain.run on the replay detector
class SubtractReplay(PeakGroupReplay):
    """PeakGroupReplay plus the second render_gaussians call and disc_residuals: hand-made rows, every argument kept."""

    def __init__(self, scenario):
        PeakGroupReplay.__init__(self, scenario)
        self.render2_args, self.dres_args = [], []

    def render_gaussians(self, img, comp, nsigma=5.0, bkg_dev=None, signed=False):
        if "render_gaussians" not in self.calls:
            assert not signed                                 # the residual step renders as it did
            return PeakGroupReplay.render_gaussians(self, img, comp, nsigma, bkg_dev)
        assert signed is True                                 # the second residual: holes carry a negative amplitude
        self.calls.append("render_gaussians")
        comp = np.array(comp, np.float64)
        self.render2_args.append(dict(img=img, comp=comp, nsigma=nsigma, bkg_dev=bkg_dev))
        rows = np.zeros((len(comp), L.CY_RND_FIELDS))
        rows[1::3, 0] = 3.0                                   # every third component from the second on misses the image
        return rows, np.zeros(SHAPE, np.float32), np.zeros(SHAPE, np.float32)

    def disc_residuals(self, map_dev, model_dev, jobs):
        self.calls.append("disc_residuals")
        jobs = np.array(jobs, np.float64)
        self.dres_args.append(dict(map_dev=map_dev, model_dev=model_dev, jobs=jobs))
        return np.stack([_dres(5 if i == 1 else 0, npix=40 + i, x=int(j[0]), y=int(j[1])) for i, j in enumerate(jobs)])


def test_chain_without_the_switch_is_what_it_was():
    s, kw = _setup("B")
    config = dict(s["config"], fit_peak_groups=True, residual_peaks=True, residual_holes=True, residual_scales=3, residual_peaks_max=10, save_residual_maps=False)
    det0, stats0 = PeakGroupReplay("B"), {}                   # has no disc_residuals: a call would raise
    chain0 = measure.Chain(det0, np.zeros(SHAPE, np.float32), s["sources"], config, **kw).run(measure.plan(config), stats0)
    s1, _ = _setup("B")
    det1, stats1 = PeakGroupReplay("B"), {}
    chain1 = measure.Chain(det1, np.zeros(SHAPE, np.float32), s1["sources"], dict(config, subtract_peaks=False), **kw).run(measure.plan(dict(config, subtract_peaks=False)), stats1)
    assert det1.calls == det0.calls and det0.calls[-1] == "fit_peak_groups" and det0.calls.count("render_gaussians") == 1
    assert set(stats1) == set(stats0) and not set(stats0) & SUBTRACT_STATS and PEAKGROUP_STATS <= set(stats0)
    assert chain0.resid2 is None and chain0.peak_model is None and chain0.disc_rows is None and chain0.subtract_stats is None and chain0.left_peak_list is None
    lists0, lists1 = measure.peak_lists(chain0), measure.peak_lists(chain1)
    assert json.dumps(lists0) == json.dumps(lists1) and list(lists0) == ["residual_peaks", "residual_holes", "residual_scale_peaks"]
    assert not [k for lst in lists0.values() for d in lst for k in d if k.startswith("gres_")]
    assert json.dumps(s["sources"]) == json.dumps(s1["sources"]) and not [k for o in s["sources"] for k in o if k in measure.SOURCE_LEFT_KEYS]


@pytest.mark.parametrize("searches,groups", [("peaks", True), ("peaks", False), ("all", True), ("all", False), ("none", True)])
def test_chain_with_the_switch(searches, groups):
    s, kw = _setup("B")
    on = {"peaks": dict(residual_peaks=True), "all": dict(residual_peaks=True, residual_holes=True, residual_scales=4), "none": {}}[searches]
    config = dict(s["config"], subtract_peaks=True, fit_peak_groups=groups, residual_peaks_sigma=4.0, residual_peaks_radius=3, residual_peaks_max=10,
                  **on)                  # fit_peaks is implied
    steps = measure.plan(config)
    assert steps == measure.plan(dict(config, fit_peaks=True, subtract_peaks=False))
    s0, _ = _setup("B")
    det0, stats0 = PeakGroupReplay("B"), {}
    chain0 = measure.Chain(det0, np.zeros(SHAPE, np.float32), s0["sources"], dict(config, fit_peaks=True, subtract_peaks=False), **kw).run(steps, stats0)
    det, stats = SubtractReplay("B"), {}
    chain = measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], config, **kw).run(steps, stats)
    names = {"peaks": ["residual_peaks"], "all": ["residual_peaks", "residual_holes", "residual_scale_peaks"], "none": []}[searches]
    # the order: everything the run without the switch called, then the render, one call per list, the rms map and the two searches
    assert det.calls[:len(det0.calls)] == det0.calls
    assert det.calls[len(det0.calls):] == ["render_gaussians"] + ["disc_residuals"] * len(names) + ["expand_background", "find_peaks", "find_peaks"]
    assert list(chain.disc_rows) == names == list(chain.peakfit_rows)
    # the render: the selection of the chain's own rows, on the first residual, without a background, with the nsigma of the residual step
    comp, index, counts = measure.peak_render_selection(chain)
    a = det.render2_args[0]
    assert len(det.render2_args) == 1 and a["img"] is chain.resid and a["bkg_dev"] is None and a["nsigma"] == float(config.get("residual_nsigma", 5.0)) and np.array_equal(a["comp"], comp)
    assert np.array_equal(chain.subtract_comp, comp) and chain.subtract_index == index and chain.resid2 is not chain.resid and chain.peak_model is not chain.model
    # the group fit where the replay gave one (a list's last odd job is alone: status 6, the single fit)
    rows_of = lambda nm, i: chain.peakgroup_rows[nm][chain.peakfit_select[nm].index(i)] if groups else None
    assert counts["sources"] == ["group" if groups and rows_of(nm, i)[0] in (0, 2) else "single" for nm, i in index]
    assert (not groups) == (chain.peakgroup_rows is None)
    # the replay puts the strongest scale peak on the pixel peak: it is left out as a duplicate, and the same emission is subtracted once
    assert counts["duplicates"] == (1 if searches == "all" else 0) and counts["wandered"] == 0
    if names:
        assert index and all(nm in names for nm, _ in index)
        holes = [k for k, (nm, _) in enumerate(index) if nm == "residual_holes"]
        assert all(comp[k, 0] < 0 for k in holes) and all(comp[k, 0] > 0 for k in range(len(index)) if k not in holes)
    # the selection is in the pixel frame: the first component is the first entry's fit, not yet moved by box_origin
    bx, by = kw["box_origin"]
    if names:
        first = measure.peak_lists(chain)["residual_peaks"][index[0][1]]
        assert comp[0, 1] == first["gblend_x" if groups else "gfit_x"] - bx and comp[0, 2] == first["gblend_y" if groups else "gfit_y"] - by
    lists, lists0 = measure.peak_lists(chain), measure.peak_lists(chain0)
    assert list(lists) == names + ["residual_peaks_left", "residual_holes_left"] and list(lists0) == names
    render_rows = chain.subtract_render_rows
    for name, a in zip(names, det.dres_args):
        assert a["map_dev"] is chain.resid2 and a["model_dev"] is chain.peak_model and np.array_equal(a["jobs"], chain.peakfit_jobs[name])
        select, raw = chain.peakfit_select[name], chain.disc_rows[name]
        picked = {i: (src, int(r[0])) for (nm, i), src, r in zip(index, counts["sources"], render_rows) if nm == name}
        want = measure.annotate_peak_residuals([dict(d) for d in lists0[name]], raw, np.zeros(len(select)), picked, kw["beam_area"], kw["box_origin"], select)
        for i, (d, w, d0) in enumerate(zip(lists[name], want, lists0[name])):
            assert tuple(d) == tuple(d0) + measure.GRES_KEYS and {k: d[k] for k in d0} == d0 and d == w
            if i not in select:
                assert all(d[k] is None for k in measure.GRES_KEYS)
        d = lists[name][select[0]]
        assert d["gres_npix"] == 40 and d["gres_x_max"] == int(chain.peakfit_jobs[name][0, 0]) + int(bx) and d["gres_ratio"] is None      # the replay's rms map is 0
        assert d["gres_subtracted"] is (picked.get(select[0], (None, None))[1] == 0)
        if len(select) > 1:
            assert lists[name][select[1]]["gres_npix"] == 0 and lists[name][select[1]]["gres_rms"] is None
    assert len(det.dres_args) == len(names)
    # the searches of the second residual: both signs, the pixel search's threshold, radius and cap, the rms map expanded just before
    left = det.peak_args[-2:]
    assert [p["sign"] for p in left] == [1, -1] and all(p["map_dev"] is chain.resid2 and p["rms_dev"] is det.rms for p in left)
    assert all((p["k_sigma"], p["radius"], p["cap"]) == (4.0, 3, 10) for p in left)
    for key, sign, cnt in (("residual_peaks_left", 1, "res_npeaks_left"), ("residual_holes_left", -1, "res_nholes_left")):
        moved = chain.left_rows[sign].copy()
        moved[:, 0] += bx
        moved[:, 1] += by
        probe = [dict(o) for o in s0["sources"]]
        want = measure.annotate_peaks(probe, moved, 7, int(config.get("residual_peaks_min_above", 3)), kw["beam_area"], kw["wcs"], kw["wcs_origin"], holes=sign < 0)
        assert lists[key] == want and all(tuple(d) == measure.PEAK_KEYS for d in lists[key])
        nkey = "res_nholes" if sign < 0 else "res_npeaks"
        assert [o[cnt] for o in s["sources"]] == [o[nkey] for o in probe]
    assert stats["left_truncated"] == 2 and (stats["left_peaks"], stats["left_holes"]) == (len(lists["residual_peaks_left"]), len(lists["residual_holes_left"]))
    # the sources: what they were, plus the two counts; the first search's keys are untouched
    for o, o0 in zip(s["sources"], s0["sources"]):
        assert tuple(o) == tuple(o0) + measure.SOURCE_LEFT_KEYS and {k: o[k] for k in o0} == o0
    old = {k for k in stats if k not in SUBTRACT_STATS}
    assert set(stats) == old | SUBTRACT_STATS and old == set(stats0) and PEAKFIT_STATS <= old
    assert (stats["subtract_selected"], stats["subtract_wandered"], stats["subtract_duplicates"]) == (len(index), counts["wandered"], counts["duplicates"])
    assert stats["subtract_rendered"] == int((render_rows[:, 0] == 0).sum()) and stats["subtract_render_kernel_ms"] == KERNEL_MS
    assert stats["disc_residual_kernel_ms"] == len(names) * KERNEL_MS and stats["left_peaks_kernel_ms"] == 2 * KERNEL_MS and stats["subtract_ms"] >= 0.0
    json.dumps(lists)


def test_chain_subtracts_nothing_without_the_residual_step(tmp_path):
    s, kw = _setup("B")
    config = dict(s["config"], subtract_peaks=True, residual_peaks=True)
    det, stats = SubtractReplay("B"), {}
    steps = tuple(k for k in measure.plan(config) if k not in ("blend", "residual"))
    chain = measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], config, **kw).run(steps, stats)
    assert "disc_residuals" not in det.calls and "fit_peaks" not in det.calls and not set(stats) & SUBTRACT_STATS and chain.resid2 is None
    assert list(measure.peak_lists(chain)) == []


def test_save_maps_writes_the_second_pair_only_with_the_switch(tmp_path, monkeypatch):
    written = []
    monkeypatch.setattr(measure, "_save_maps", lambda tags, maps, path: written.append((tags, maps, path)))
    fake = SimpleNamespace(save_bkg=False, save_residual=True, save_scales=False, scale_planes=None, model="m", resid="r", peak_model=None, resid2=None)
    measure.Chain.save_maps(fake, "cat.json")
    assert written == [(("model_", "resid_"), ("m", "r"), "cat.json")]
    fake.peak_model, fake.resid2 = "pm", "r2"
    measure.Chain.save_maps(fake, "cat.json")
    assert written[1:] == [(("model_", "resid_"), ("m", "r"), "cat.json"), (("peakmodel_", "resid2_"), ("pm", "r2"), "cat.json")]
    fake.save_residual = False
    measure.Chain.save_maps(fake, "cat.json")
    assert len(written) == 3


# ---- the chain on the numpy references: a blended pair beside the scene of the residual-peak tests
class RefDetector(CR.RefDetector):
    """The stand-in of tests/peaks_chain_ref.py plus the references of the fits, the group fits and the disc residuals."""

    def render_gaussians(self, img, comp, nsigma=5.0, bkg_dev=None, signed=False):
        if not signed:
            return CR.RefDetector.render_gaussians(self, img, comp, nsigma, bkg_dev)
        rows, model, resid = DR.render_signed(img, comp, nsigma, bkg_dev)
        return rows, model.astype(np.float32), resid.astype(np.float32)

    def fit_peaks(self, map_dev, jobs, max_iter=64):
        return PR.fit_peaks(map_dev, jobs, max_iter)

    def fit_peak_groups(self, map_dev, jobs, link=1.5, max_iter=64):
        return GR.fit_peak_groups(map_dev, jobs, link, max_iter)

    def disc_residuals(self, map_dev, model_dev, jobs):
        return DR.disc_residuals(map_dev, model_dev, jobs)[0]


def pair_scene():
    """-> (image float32 [160, 160], the source list): the scene of peaks_chain_ref plus the planted pair."""
    img, sources = CR.scene()
    yy, xx = np.mgrid[0:CR.SIDE, 0:CR.SIDE].astype(np.float64)
    img = img.astype(np.float64)
    for A, x0, y0 in PLANTED:
        img += A * np.exp(-((xx - x0) ** 2 + (yy - y0) ** 2) / (2 * PLANTED_SIGMA ** 2))
    return img.astype(np.float32), sources


def pair_config(groups):
    return dict(CR.CONFIG, residual_holes=True, subtract_peaks=True, fit_peak_groups=groups, residual_nsigma=5.0, residual_peaks_sigma=5.0,
                residual_peaks_radius=2)


def check_pair(lists, groups):
    """The statements of the chain-level tests (CPU and GPU) on the lists of a run over pair_scene()."""
    found = [(d["x_peak"], d["y_peak"]) for d in lists["residual_peaks"]]
    assert found == list(PLACES) and lists["residual_holes"] == [], found
    near = lambda d, p, r: math.hypot(d["x_peak"] - p[0], d["y_peak"] - p[1]) <= r
    left, holes = lists["residual_peaks_left"], lists["residual_holes_left"]
    if groups:
        # the group fit explains the pair: nothing is left, in either sign, within 12 px of the three positions
        assert not [d for d in left + holes for p in PLACES if near(d, p, 12.0)], (left, holes)
        for d in lists["residual_peaks"]:
            assert d["gres_subtracted"] is True and 0.5 < d["gres_ratio"] < 1.5, d
        assert [d["gres_source"] for d in lists["residual_peaks"]] == ["single", "group", "group"]
    else:
        # the single fits are biased by each other's wing and over-subtract: a hole between the two members, no peak near the pair
        assert [d for d in holes if near(d, (102, 62), 3.0)], holes
        assert not [d for d in left for p in PLACES[1:] if near(d, p, 12.0)], left
        assert [d["gres_source"] for d in lists["residual_peaks"]] == ["single"] * 3


@pytest.mark.parametrize("groups", [True, False])
def test_chain_on_the_references(groups):
    img, sources = pair_scene()
    config, stats = pair_config(groups), {}
    chain = measure.Chain(RefDetector(), img, sources, config).run(measure.plan(config), stats)
    lists = measure.peak_lists(chain)
    check_pair(lists, groups)
    assert stats["subtract_selected"] == stats["subtract_rendered"] == 3 and stats["subtract_wandered"] == 0 == stats["subtract_duplicates"]
    assert sources[0]["res_npeaks_left"] == 0 and sources[0]["res_nholes_left"] == 0 and sources[0]["res_npeaks"] == 0
    # the first residual is what it was, the second holds the noise: its standard deviation is that of the unit noise
    assert float(np.std(chain.resid)) > 1.5 and (0.9 < float(np.std(chain.resid2)) < 1.1) and np.allclose(chain.resid2, chain.resid - chain.peak_model, rtol=0.0, atol=1e-5)


# ---- the big map: what a wrapped pixel offset would read
def test_a_result_read_from_the_decoy_would_not_pass():
    """On the 46341 x 46339 twin of tests/bigmap_cases.py a kernel whose 32-bit pixel offset wrapped reads, for a patch beyond
    pixel 2^30, the decoy 2^30 pixels before it.  The rows of the decoy's jobs are not the rows of the patch's jobs under the rule of
    the GPU test, in the map (maxabs, the sums) and in the model (model_sum), so tests/test_gpu_bigmap_disc_residual.py would fail."""
    import bigmap_cases as B
    jobs = B.all_peak_jobs()
    ref, ab = DR.disc_residuals(B.host(), B.host_model(), jobs)
    per = len(B.PEAK_NAMES)
    assert ref.shape == (per * len(B.names()), DR.FIELDS) and (ref[:, 0] == 0).all() and (ref[:, 1] > 0).all()
    for nm, decoy in B.DECOY_OF.items():
        mine, other = ref[B.rows_of(nm, per)], ref[B.rows_of(decoy, per)]
        for j in range(per):
            assert mine[j, 5] != other[j, 5], (nm, B.PEAK_NAMES[j])                               # maxabs is compared exactly
            for f, t in DR.SUMS:
                bound = 2.0 * mine[j, 1] * 2.0 ** -53 * ab[B.rows_of(nm, per)][j, t]
                assert abs(mine[j, f] - other[j, f]) > bound, (nm, B.PEAK_NAMES[j], f)
    # with the model map left out the model sums are 0: the map's decoys still differ
    assert not DR.disc_residuals(B.host(), None, jobs[:per])[0][:, 8].any()


HOLE = (-25.0, 40.3, 120.6)                                   # amplitude, x, y of a planted hole of sigma 1.6 px, far from everything else


def hole_scene():
    """pair_scene() plus a planted hole."""
    img, sources = pair_scene()
    yy, xx = np.mgrid[0:CR.SIDE, 0:CR.SIDE].astype(np.float64)
    A, x0, y0 = HOLE
    img = img.astype(np.float64) + A * np.exp(-((xx - x0) ** 2 + (yy - y0) ** 2) / (2 * PLANTED_SIGMA ** 2))
    return img.astype(np.float32), sources


def check_hole(lists):
    """The statements of the chain-level tests (CPU and GPU) on the lists of a run over hole_scene(): the hole is listed, fitted,
    rendered with a negative amplitude and subtracted, and nothing of it is left in either sign."""
    holes = [d for d in lists["residual_holes"] if math.hypot(d["x_peak"] - HOLE[1], d["y_peak"] - HOLE[2]) <= 1.5]
    assert len(holes) == 1, lists["residual_holes"]
    d = holes[0]
    assert d["gfit_status"] == 0 and d["gfit_peak"] < 0 and (d["gres_subtracted"], d["gres_render_status"]) == (True, 0), d
    assert 0.5 < d["gres_ratio"] < 1.5 and d["gres_model_flux"] is None and abs(d["gres_max"]) < 5.0 * d["rms"], d
    left = lists["residual_peaks_left"] + lists["residual_holes_left"]
    assert not [p for p in left if math.hypot(p["x_peak"] - HOLE[1], p["y_peak"] - HOLE[2]) <= 12.0], left


def test_a_hole_is_rendered_negative_and_subtracted():
    """The reference of the signed render admits a hole's negative amplitude where residual_ref.render (cy_render_gaussians) turns
    it away with status 1; on the references the chain subtracts the planted hole and finds nothing left of it."""
    import residual_ref as RR
    comp = np.array([[-1.5, 80.0, 60.0, 0.4, 0.0, 0.4], [2.0, 30.0, 40.0, 0.4, 0.0, 0.4], [0.0, 50.0, 50.0, 0.4, 0.0, 0.4]])
    img = np.ones((120, 160), np.float32)
    rows, model, resid = DR.render_signed(img, comp, 5.0)
    plain = RR.render(img, comp, 5.0)
    assert rows[:, 0].tolist() == [0.0, 0.0, 1.0] and plain[0][:, 0].tolist() == [1.0, 0.0, 1.0]
    assert model[60, 80] == -1.5 and model[40, 30] == 2.0 and resid[60, 80] == 2.5 and np.array_equal(np.maximum(model, 0.0), plain[1])
    img, sources = hole_scene()
    config, stats = pair_config(True), {}
    chain = measure.Chain(RefDetector(), img, sources, config).run(measure.plan(config), stats)
    lists = measure.peak_lists(chain)
    check_hole(lists)
    assert (stats["subtract_selected"], stats["subtract_rendered"]) == (4, 4) and float(chain.peak_model.min()) < -15.0
    k = chain.subtract_index.index(("residual_holes", 0))
    assert chain.subtract_comp[k, 0] < 0 and chain.subtract_render_rows[k, 0] == 0
