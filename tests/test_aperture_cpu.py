"""--peak_apertures without a GPU: the two restatements of cy_aperture_sums (tests/aperture_ref.py) against each other on every
constructed case, what the cases are for, annotate_apertures on hand-made rows, the config and the command line, plan(), the
symbols of the header in lib.py, and Chain.run on the replay detector of tests/test_atrous_cpu.py: without the switch the calls and
stats keys it made before, with it the order of the calls and every call's map, jobs, units and factor table."""
import json
import os
import sys

import numpy as np
import pytest

import aperture_cases as PC
import aperture_ref as PR
from caesar_yolo_amd import lib as L
from caesar_yolo_amd import measure
from test_atrous_cpu import ScaleReplay
from test_measure_chain_cpu import KERNEL_MS, SHAPE, Replay, _setup, _stat_keys, Z
from test_peaks_cpu import PEAK_STEPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APERTURE_STATS = {"apertures_ms", "aperture_kernel_ms", "apertures_jobs", "apertures_measured", "apertures_clipped"}
H, F = L.CY_APER_HEAD, L.CY_APER_RING_FIELDS


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- the reference
@pytest.mark.parametrize("name", PC.NAMES)
def test_the_two_restatements_agree(name):
    c = PC.case(name)
    for with_rms in (True, False):
        want = PC.rows(name, with_rms)
        got = PR.reference_loops(c.map, c.rms if with_rms else None, c.jobs, c.factors)
        assert want.shape == (c.jobs.shape[0], PR.FIELDS) and np.array_equal(bits(got), bits(want)), with_rms
    assert np.array_equal(PC.rows(name, False)[:, H + 3::F], np.zeros((c.jobs.shape[0], PR.RINGS_MAX)))     # no rms map: svar 0


def test_median_rule():
    m = PR.median_rule
    assert m([]) == 0.0 and m([3.0]) == 3.0 and m([1.0, 4.0]) == 2.5 and m([5.0, 1.0, 3.0]) == 3.0 and m([1.0, 2.0, 2.0, 9.0]) == 2.0
    assert m([1.0, 1.0, 3.0, 3.0]) == 2.0 and m([-PC.FLT_MAX, PC.FLT_MAX]) == 0.0 and m([PC.FLT_MAX, PC.FLT_MAX]) == PC.FLT_MAX


def test_the_cases_hold_what_they_are_for():
    assert L.CY_APER_FIELDS == PR.FIELDS == 40 and (PR.RINGS_MAX, PR.RADIUS_MAX, PR.HEAD, PR.RING_FIELDS, PR.JOBS_MAX) == (8, 256, 8, 4, 1 << 20)
    st = lambda name: PC.rows(name)[:, 0].tolist()
    assert st("image_1x1") == [0, 0, 0, 0, 2, 2] and PC.rows("image_1x1")[4, 1:5].tolist() == [-1, -1, -1, -1]      # r = 0.2 around (0.5, 0.5) holds no pixel
    r = PC.rows("centres")
    assert r[:12, 0].tolist() == [0.0] * 12 and r[12:19, 0].tolist() == [2.0] * 7 and r[19:, 0].tolist() == [2.0, 0.0, 0.0]
    assert r[4, 5] == 0.0 and r[0, 5] == 1.0 and r[0, 1:5].tolist() == [0, 5, 0, 5] and r[7, 1:5].tolist() == [0, 4, 0, 10]
    assert (PC.rows("rings_1")[:, H + F:] == 0).all() and (PC.rows("rings_8")[4, H::F] > 0).all()
    # ring 2 of radius 5 around an integer centre: 81 - 29 pixels with the twelve boundary pixels, twelve fewer one ulp below
    a, b = PC.rows("boundary5")[0], PC.rows("boundary5_below")[0]
    assert (a[H], a[H + F], a[H + 2 * F]) == (29, 81 - 29, 113 - 81) and (b[H], b[H + F], b[H + 2 * F]) == (29, 81 - 29 - 12, 113 - 81 + 12)
    r = PC.rows("radius_limits")
    assert r[:, 0].tolist() == [1, 1, 1, 1, 1, 1, 0, 1, 0, 1, 0, 1] and r[6, 1:6].tolist() == [0, 39, 0, 39, 1] and r[8, 1:5].tolist() == [20, 20, 19, 19]
    for area in (255, 256, 257, 1025):
        x = PC.rows("area_%d" % area)[0]
        assert x[0] == 0 and (x[2] - x[1] + 1) * (x[4] - x[3] + 1) == area
    x = PC.rows("largest")[0]
    assert x[1:6].tolist() == [44, 556, 44, 555, 0] and x[H:H + 3 * F:F].sum() > 190000
    x = PC.rows("pixel_values")[0]
    assert np.isfinite(x).all() and x[H:H + 3 * F:F].sum() == 64 - 4 * 5            # NaN, +-inf and +-0 do not count
    n = {k: PC.rows("annulus_" + k)[0] for k in ("0", "1", "2", "even", "odd", "equal", "ties", "split", "ties_odd")}
    assert [n[k][H + F] for k in ("0", "1", "2", "even", "odd", "equal", "ties", "split", "ties_odd")] == [0, 1, 2, 24, 23, 24, 20, 24, 7]
    assert n["0"][6:8].tolist() == [0, 0] and n["1"][6:8].tolist() == [4, 0] and n["2"][6:8].tolist() == [1.25, 2.75]
    assert n["equal"][6:8].tolist() == [7, 0] and n["ties"][6:8].tolist() == [2, 0.5] and n["split"][6:8].tolist() == [2, 1] and n["ties_odd"][6:8].tolist() == [2, 0]
    x = PC.rows("rms_values")[0]
    assert 0 < x[H + 3] < 1e77 and np.isfinite(x).all()
    r = PC.rows("many_jobs")
    assert r.shape[0] == 70000 > 65535 and set(r[:, 0].tolist()) == {0.0, 2.0} and r[:, 5].sum() > 0
    # the exact scene: integers everywhere, the pedestal as background, twice the disc's pixels as flux from its radius on
    x = PC.rows("exact_scene")[0]
    disc = 113
    assert x[6:8].tolist() == [3.0, 0.0] and (x == np.round(x)).all() and x[H:H + 3 * F:F].sum() == disc
    d = measure.annotate_apertures([{}], x[None], 5, 0)[0]
    assert d["ap_flux_sum"][2:] == [2.0 * disc] * 3 and d["ap_flux_sum"][:2] == [2.0 * 13, 2.0 * 49] and d["ap_npix"][:3] == [13, 49, disc]


# ---- annotate_apertures
def _aper_row(status, rings, med=0.0, mad=0.0, clipped=0):
    r = np.zeros(L.CY_APER_FIELDS)
    r[0], r[1:5], r[5], r[6], r[7] = status, ((2, 9, 3, 10) if status == 0 else (-1,) * 4), clipped, med, mad
    for k, f in enumerate(rings):
        r[H + F * k:H + F * k + 4] = f
    return r


def test_annotate_apertures_on_hand_made_rows():
    assert measure.APERTURE_KEYS == ("ap_status", "ap_clipped", "ap_radius", "ap_npix", "ap_sum", "ap_bkg", "ap_bkg_rms", "ap_nbkg", "ap_flux_sum",
                                     "ap_flux", "ap_flux_err", "ap_snr", "ap_best")
    assert tuple(L.APER_NAMES) == ("status", "x0", "x1", "y0", "y1", "clipped", "bkg_med", "bkg_mad") and measure.APER.bkg_mad == 7
    big = 2.0 ** 53
    rows = np.stack([
        _aper_row(0, [(5, 10.0, 30.0, 4.0), (8, 12.0, 20.0, 12.0), (16, 3.0, 9.0, 20.0), (40, 41.0, 50.0, 9.0)], med=0.5, mad=2.0, clipped=1),
        _aper_row(0, [(1, big, 0, 0.0), (1, 1.0, 0, 4.0), (1, 1.0, 0, 0.0), (0, 0, 0, 0)]),      # order of the sums; zero errors; empty annulus
        _aper_row(1, []), _aper_row(2, []),
        _aper_row(0, [(4, 8.0, 0, 4.0), (12, 8.0, 0, 12.0), (20, -6.0, 0, 48.0), (9, 0, 0, 0)])])     # equal snr at 0 and 1
    entries = [{"x": float(i), "keep": i} for i in range(5)]
    radii = np.arange(15, dtype=np.float64).reshape(5, 3)
    out = measure.annotate_apertures(entries, rows, 3, 4.0, radii)
    assert out is entries and all(set(d) == {"x", "keep"} | set(measure.APERTURE_KEYS) and d["keep"] == i for i, d in enumerate(out))
    a = out[0]
    assert (a["ap_status"], a["ap_clipped"], a["ap_bkg"], a["ap_bkg_rms"], a["ap_nbkg"]) == (0, 1, 0.5, 1.482602218505602 * 2.0, 40)
    assert a["ap_radius"] == [0.0, 1.0, 2.0] and a["ap_npix"] == [5, 13, 29] and a["ap_sum"] == [10.0, 22.0, 25.0]
    assert a["ap_flux_sum"] == [7.5, 15.5, 10.5] and a["ap_flux"] == [7.5 / 4, 15.5 / 4, 10.5 / 4] and a["ap_flux_err"] == [1.0, 2.0, 3.0]
    assert a["ap_snr"] == [1.875, 1.9375, 0.875] and a["ap_best"] == 1
    assert all(type(v) is int for v in a["ap_npix"]) and type(a["ap_status"]) is int
    b = out[1]
    assert b["ap_sum"] == [big, (big + 1.0), (big + 1.0) + 1.0] == [big, big, big] and b["ap_npix"] == [1, 2, 3] and b["ap_nbkg"] == 0      # not big + 2
    assert b["ap_flux_err"] == [0.0, 1.0, 1.0] and b["ap_snr"] == [None, big / 4, big / 4] and b["ap_best"] == 1 and b["ap_bkg_rms"] == 0.0
    for d, st in ((out[2], 1), (out[3], 2)):
        assert d["ap_status"] == st and d["ap_clipped"] == 0 and (d["ap_bkg"], d["ap_bkg_rms"], d["ap_nbkg"]) == (0.0, 0.0, 0)
        assert all(d[k] is None for k in ("ap_radius", "ap_npix", "ap_sum", "ap_flux_sum", "ap_flux", "ap_flux_err", "ap_snr", "ap_best"))
    assert out[4]["ap_snr"] == [2.0, 2.0, 0.625] and out[4]["ap_best"] == 0                     # the first of equal ones
    json.dumps(out)
    for ba in (0, None, -1.0):                                    # no beam: sums, no flux
        d = measure.annotate_apertures([{}], rows[:1], 3, ba)[0]
        assert d["ap_flux_sum"] == [7.5, 15.5, 10.5] and d["ap_radius"] is None
        assert all(d[k] is None for k in ("ap_flux", "ap_flux_err", "ap_snr", "ap_best"))
    d = measure.annotate_apertures([{}], rows[1:2], 3, 1.0)[0]
    assert d["ap_snr"] == [None, big / 2, big / 2]
    d = measure.annotate_apertures([{}], _aper_row(0, [(1, 1.0, 1.0, 0.0), (3, 0, 0, 0)])[None], 1, 2.0)[0]      # no error anywhere: no best
    assert d["ap_snr"] == [None] and d["ap_best"] is None and d["ap_nbkg"] == 3
    with pytest.raises(AssertionError):
        measure.annotate_apertures([{}], rows, 3, 1.0)


# ---- config, plan() and the command line
def test_aperture_config():
    assert measure.aperture_config({}) == (1.0, (1.0, 2.0, 3.0, 4.0), 6.0) and not measure.wants_apertures({})
    assert measure.wants_apertures({"peak_apertures": True}) and not measure.wants_apertures({"peak_apertures": False})
    c = {"aperture_unit": 2.5, "aperture_radii": " 0.5, 1 ,7e0", "aperture_annulus": 7.5}
    assert measure.aperture_config(c) == (2.5, (0.5, 1.0, 7.0), 7.5)
    assert measure.aperture_config({"aperture_radii": [1, 2.5], "aperture_annulus": 3}) == (1.0, (1.0, 2.5), 3.0)
    assert measure.aperture_config({"aperture_radii": "1,2,3,4,5,6,7", "aperture_annulus": 8})[1] == (1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0)
    for bad in ({"aperture_radii": ""}, {"aperture_radii": "1,,2"}, {"aperture_radii": "1,2,"}, {"aperture_radii": "a,b"}, {"aperture_radii": "2,1"},
                {"aperture_radii": "1,1"}, {"aperture_radii": "0,1"}, {"aperture_radii": "-1,1"}, {"aperture_radii": "1,nan"}, {"aperture_radii": "1,inf"},
                {"aperture_radii": "1,2,3,4,5,6,7,8", "aperture_annulus": 9}, {"aperture_radii": []}, {"aperture_radii": 3},
                {"aperture_annulus": 4.0}, {"aperture_annulus": 3.0}, {"aperture_annulus": float("nan")}, {"aperture_annulus": float("inf")},
                {"aperture_unit": 0.0}, {"aperture_unit": -1.0}, {"aperture_unit": float("nan")}, {"aperture_unit": float("inf")}):
        with pytest.raises(ValueError):
            measure.aperture_config(bad)
    # the defaults at the last scale: 6 * 32 = 192 <= 256
    unit, factors, annulus = measure.aperture_config({})
    assert annulus * unit * (1 << (measure.SCALES_MAX - 1)) == 192 <= L.CY_APER_RADIUS_MAX


def test_plan_with_and_without_the_switch():
    from test_measure_chain_cpu import IMPLIED
    for flag, steps in IMPLIED.items():
        assert measure.plan({flag: True}) == steps == measure.plan({flag: True, "peak_apertures": False}), flag
        assert set(measure.plan({flag: True, "peak_apertures": True})) == set(steps) | set(PEAK_STEPS)
    assert measure.plan({}) == () == measure.plan({"peak_apertures": False, "aperture_radii": "1,2"})
    assert measure.plan({"peak_apertures": True}) == PEAK_STEPS == measure.plan({"residual_peaks": True})
    assert measure.plan({"peak_apertures": True, "residual_scales": 3}) == PEAK_STEPS and measure.plan({"peak_apertures": True, "fit_blends": True}) == measure.STEPS
    assert not measure.wants_peaks({"peak_apertures": True}) and not measure.wants_scales({"peak_apertures": True})     # it turns no search on


def test_flags_parse_and_imply():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import run
    w = "--weights=seeded:l:5"
    base = run.measure_config(run.parse_args([w]))
    assert (base["peak_apertures"], base["aperture_unit"], base["aperture_radii"], base["aperture_annulus"]) == (False, 1.0, "1,2,3,4", 6.0)
    assert measure.plan(base) == () and not measure.wants_apertures(base) and measure.aperture_config(base) == measure.aperture_config({})
    args = run.parse_args([w, "--peak_apertures"])              # alone: the pixel search comes with it
    config = run.measure_config(args)
    assert measure.wants_apertures(config) and config["residual_peaks"] is True and not config["residual_holes"] and config["residual_scales"] == 0
    assert measure.plan(config) == PEAK_STEPS and args.residual_map and args.bkg_map and args.fit_components and not args.fit_blends
    for search in (["--residual_scales=3"], ["--residual_holes"]):     # with a search of its own: that one, and no other
        config = run.measure_config(run.parse_args([w, "--peak_apertures"] + search))
        assert measure.wants_apertures(config) and config["residual_peaks"] is False and measure.plan(config) == PEAK_STEPS
    args = run.parse_args([w, "--peak_apertures", "--aperture_unit=1.5", "--aperture_radii=1,2.5", "--aperture_annulus", "4"])
    assert measure.aperture_config(run.measure_config(args)) == (1.5, (1.0, 2.5), 4.0)
    for bad in (["--aperture_radii=1,,2"], ["--aperture_radii=2,1"], ["--aperture_radii=x"], ["--aperture_radii="], ["--aperture_radii=1,2,3,4,5,6,7,8", "--aperture_annulus=9"],
                ["--aperture_annulus=4"], ["--aperture_annulus=nan"], ["--aperture_unit=0"], ["--aperture_unit=-2"], ["--aperture_unit=inf"]):
        with pytest.raises(SystemExit):
            run.parse_args([w, "--peak_apertures"] + bad)
    with pytest.raises(SystemExit):
        run.parse_args([w, "--aperture_unit=abc"])
    assert run.parse_args([w, "--aperture_radii=2,1"]).peak_apertures is False       # without the switch the list is not looked at
    for flag in ("peak_apertures", "aperture_unit", "aperture_radii", "aperture_annulus"):
        assert "--" + flag in run.__doc__ and flag in run.MEASURE_KEYS, flag
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--peak_apertures" in readme and "--aperture_radii" in readme and "test_aperture_plan_cpu" in readme


def test_exports():
    assert {"cy_aperture_sums", "cy_aperture_kernel_ms"} <= set(L.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "caesar_yolo_hip.h")).read()
    for name, text in (("CY_APER_RINGS_MAX", "8"), ("CY_APER_RADIUS_MAX", "256"), ("CY_APER_HEAD", "8"), ("CY_APER_RING_FIELDS", "4"),
                       ("CY_APER_FIELDS", "(CY_APER_HEAD + CY_APER_RING_FIELDS * CY_APER_RINGS_MAX)"), ("CY_APER_JOBS_MAX", "(1 << 20)")):
        assert "#define %s %s" % (name, text) in hdr and getattr(L, name) == eval(text, {k: getattr(L, k) for k in dir(L) if k.startswith("CY_APER")}), name
    assert "int cy_aperture_sums(cy_ctx* ctx, const float* d_map, const float* d_rms /* or NULL */, int MH, int MW," in hdr
    assert "int cy_aperture_kernel_ms(const cy_ctx* ctx, double* out_ms);" in hdr
    lib = L.load()
    assert hasattr(lib, "cy_aperture_sums") and hasattr(lib, "cy_aperture_kernel_ms")
    jobs = open(os.path.join(ROOT, "caesar_yolo_amd", "csrc", "cy_measure_jobs.h")).read()
    for text in ("APER_RINGS_MAX = 8;", "APER_RADIUS_MAX = 256;", "APER_HEAD = 8;", "APER_RING_FIELDS = 4;", "APER_JOBS_MAX = 1 << 20;", "struct AperJob {"):
        assert text in jobs
    import __graft_entry__ as ge
    assert "cy_aperture.hip" in ge.HIP_SOURCES and "cy_measure_plan.cpp" in ge.CXX_SOURCES
    from caesar_yolo_amd.model import HipDetector
    assert callable(HipDetector.aperture_sums) and callable(HipDetector.aperture_kernel_ms)


# ---- Chain.run on the replay detector
class ApertureReplay(ScaleReplay):
    """ScaleReplay plus aperture_sums: hand-made rows (job i: measured unless i is odd, clipped when i is 0), every argument kept."""

    def __init__(self, scenario):
        ScaleReplay.__init__(self, scenario)
        self.aper_args = []

    def aperture_sums(self, map_dev, rms_dev, jobs, factors):
        self.calls.append("aperture_sums")
        jobs = np.array(jobs, np.float64)
        self.aper_args.append(dict(map_dev=map_dev, rms_dev=rms_dev, jobs=jobs, factors=tuple(factors)))
        K = len(factors)
        return np.stack([_aper_row(i & 1, [(k + 1, 2.0 * (k + 1), 4.0, 1.0) for k in range(K)] if not i & 1 else [], med=0.25, clipped=int(i == 0))
                         for i in range(jobs.shape[0])])


def test_chain_without_the_switch_is_what_it_was():
    base_calls = None
    for extra in ({}, {"peak_apertures": False, "aperture_radii": "3,2,1", "aperture_unit": -1.0}):     # not looked at without the switch
        s, kw = _setup("B")
        config = dict(s["config"], **extra)
        det, stats = Replay("B"), {}                          # has no aperture_sums: a call would raise
        chain = measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], config, **kw).run(measure.plan(config), stats)
        assert measure.plan(config) == measure.plan(s["config"])
        base_calls = base_calls or list(det.calls)
        assert det.calls == base_calls and det.calls[-1] == "measure_residuals"
        assert set(stats) == _stat_keys(measure.plan(config), json.loads(str(Z["B/stats"]))) and not set(stats) & APERTURE_STATS
        assert chain.aperture_rows is None and chain.aperture_stats is None and measure.peak_lists(chain) == {}
        assert [{k: v for k, v in o.items()} for o in json.loads(json.dumps(s["sources"]))] == json.loads(str(Z["B/catalog"]))
    # a search without the switch: the lists carry no aperture key
    s, kw = _setup("B")
    config = dict(s["config"], residual_peaks=True, residual_scales=3)
    det = ScaleReplay("B")                                    # no aperture_sums either
    chain = measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], config, **kw).run(measure.plan(config), {})
    assert chain.peak_list and chain.scale_list and not [k for d in chain.peak_list + chain.scale_list for k in d if k.startswith("ap_")]


@pytest.mark.parametrize("searches", ["peaks", "holes", "scales", "all", "none"])
def test_chain_with_the_switch(searches):
    s, kw = _setup("B")
    J = 4
    on = {"peaks": dict(residual_peaks=True), "holes": dict(residual_holes=True), "scales": dict(residual_scales=J),
          "all": dict(residual_peaks=True, residual_holes=True, residual_scales=J), "none": {}}[searches]
    config = dict(s["config"], peak_apertures=True, aperture_unit=1.5, aperture_radii="1,2.5", aperture_annulus=4.0, residual_peaks_max=10, **on)
    plain_steps = measure.plan(s["config"])
    assert measure.plan(config) == plain_steps                # the same steps: the apertures are no step
    # the same run without the switch, for the keys the entries had before
    det0 = ApertureReplay("B")
    s0, _ = _setup("B")
    chain0 = measure.Chain(det0, np.zeros(SHAPE, np.float32), s0["sources"], dict(config, peak_apertures=False), **kw).run(plain_steps, {})
    det, src, stats = ApertureReplay("B"), s["sources"], {}
    chain = measure.Chain(det, np.zeros(SHAPE, np.float32), src, config, **kw).run(plain_steps, stats)
    names = {"peaks": ["residual_peaks"], "holes": ["residual_peaks", "residual_holes"], "scales": ["residual_scale_peaks"],
             "all": ["residual_peaks", "residual_holes", "residual_scale_peaks"], "none": []}[searches]
    # the order: everything the run without the switch called, then the rms map once and one call per list
    assert "aperture_sums" not in det0.calls and det.calls[:len(det0.calls)] == det0.calls
    assert det.calls[len(det0.calls):] == (["expand_background"] + ["aperture_sums"] * len(names) if names else [])
    lists = measure.peak_lists(chain)
    assert [k for k in ("residual_peaks", "residual_holes", "residual_scale_peaks") if k in lists] == names and list(chain.aperture_rows) == names
    bx, by = kw["box_origin"]
    nrows = 0
    for name, a in zip(names, det.aper_args):
        entries = lists[name]
        steps = [d.get("step", 1) for d in entries]
        assert steps == ([2, 4, 8] if name == "residual_scale_peaks" else [1])
        assert a["map_dev"] is chain.resid and a["rms_dev"] is det.rms and a["factors"] == (1.0, 2.5, 4.0)
        assert a["jobs"].tolist() == [[d["x"] - bx, d["y"] - by, 1.5 * st] for d, st in zip(entries, steps)] == [[3.5, 4.0, 1.5 * st] for st in steps]
        rows = chain.aperture_rows[name]
        assert rows.shape == (len(entries), L.CY_APER_FIELDS)
        want = measure.annotate_apertures([{} for _ in entries], rows, 2, kw["beam_area"], [[1.5 * st, 3.75 * st] for st in steps])
        before = chain0.peak_list if name == "residual_peaks" else chain0.hole_list if name == "residual_holes" else chain0.scale_list
        for d, w, d0 in zip(entries, want, before):
            assert set(d) == set(d0) | set(measure.APERTURE_KEYS) and {k: d[k] for k in d0} == d0 and {k: d[k] for k in measure.APERTURE_KEYS} == w
        assert [d["ap_status"] for d in entries] == [i & 1 for i in range(len(entries))] and entries[0]["ap_radius"] == [1.5 * steps[0], 3.75 * steps[0]]
        assert entries[0]["ap_npix"] == [1, 3] and entries[0]["ap_nbkg"] == 3 and entries[0]["ap_bkg"] == 0.25
        nrows += len(entries)
    if det.atrous_args:                                       # after the scales: ScaleReplay keeps the arguments
        e = det.expand_args[-1]
        assert e["want"] == ("rms",) and e["shape"] == SHAPE and e["cell"] == chain.cell and e["mesh"] is chain.mesh
    elif names:                                               # else Replay checked them against the recorded call
        assert det.wants[-1] == (len(det0.calls), ("rms",))
    # the sources and the other stats are what the run without the switch gave
    assert json.loads(json.dumps(src)) == json.loads(json.dumps(s0["sources"]))
    old = {k for k in stats if k not in APERTURE_STATS}
    assert set(stats) == old | APERTURE_STATS and old == _stat_keys(plain_steps, json.loads(str(Z["B/stats"]))) | {
        k for k in stats if k.startswith(("peaks_", "holes_", "scales_", "atrous_"))}
    measured = sum(1 for name in names for i in range(len(lists[name])) if not i & 1)
    assert (stats["apertures_jobs"], stats["apertures_measured"], stats["apertures_clipped"]) == (nrows, measured, len(names))
    assert stats["aperture_kernel_ms"] == len(names) * KERNEL_MS and stats["apertures_ms"] >= 0.0
    json.dumps(lists)


def test_chain_takes_no_apertures_without_the_residual_step():
    s, kw = _setup("B")
    config = dict(s["config"], peak_apertures=True, residual_peaks=True)
    det, stats = ApertureReplay("B"), {}
    steps = tuple(k for k in measure.plan(config) if k not in ("blend", "residual"))
    chain = measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], config, **kw).run(steps, stats)
    assert "aperture_sums" not in det.calls and not set(stats) & APERTURE_STATS and chain.aperture_rows is None
    with pytest.raises(ValueError):
        measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], dict(config, aperture_radii="2,1"), **kw)
