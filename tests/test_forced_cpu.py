"""Forced photometry on the CPU: the two restatements of tests/forced_ref.py against each other, the reference against planted truth,
the host helpers of caesar_yolo_amd/measure.py (forced_jobs, annotate_forced, forced_alpha, the header readers), plan(), the flags,
the exports, and Chain.run on the replay detector of tests/test_measure_chain_cpu.py without the switch (same calls, stats keys,
JSON) and with it (order and every argument of the calls)."""
import json
import math
import os
import sys

import numpy as np
import pytest

import forced_cases as FC
import forced_ref as FR
from caesar_yolo_amd import lib as L
from caesar_yolo_amd import measure
from test_measure_chain_cpu import IMPLIED, KERNEL_MS, SHAPE, Replay, _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESIDUAL_STEPS = ("measure", "islands", "deblend", "fit", "residual")


# ---- the reference
@pytest.mark.parametrize("g", [g for g in FC.groups() if not g.big], ids=lambda g: g.name)
def test_the_two_restatements_agree(g):
    """Whole arrays against nested loops: the exact fields equal, the others within the bounds the GPU is held to; and the loops with
    every exp moved by +-2 ulp stay inside them too, which is what the constant of the bound was derived for."""
    ref, aux = FR.forced_fit(g.map, g.rms, g.jobs, g.nsigma, g.fit_bkg)
    names = ["%s / %s" % (g.name, nm) for nm in g.names]
    for nudge in (0, 2, -2):
        loops, _ = FR.forced_fit(g.map, g.rms, g.jobs, g.nsigma, g.fit_bkg, nudge=nudge, loops=True)
        FR.compare(loops, ref, aux, names)


def test_the_cases_hold_what_they_are_for():
    g = FC.by_name("main_64x96")
    ref, aux = FR.forced_fit(g.map, g.rms, g.jobs, g.nsigma, g.fit_bkg)
    row = lambda nm: ref[g.names.index(nm)]
    assert set(ref[:, 0].astype(int)) == {0, 1, 3, 4, 5}
    assert [row(n)[0] for n in ("misses", "centre_1e300", "nan_x0", "negative_a", "bb_ge_ac", "inf_bkg")] == [3, 3, 1, 1, 1, 1]
    assert row("no_valid_pixel")[[0, 1]].tolist() == [5, 0] and row("npix_K_minus_1")[[0, 1, 3]].tolist() == [5, 1, 2]
    assert row("bad_pixels")[2] == 4 and row("isolated")[2] == 4 and row("isolated")[4] == 0      # four bad pixels, four bad rms values
    assert row("dup2_0")[[4, 6]].tolist() == [0, 1] and row("dup3_0")[[4, 6]].tolist() == [1, 2] and row("dup3_neighbour")[[4, 6]].tolist() == [1, 2]
    # the jobs 1e-9 px apart: the second pivot is far below the rule's 2^-40, status 4 with counts and sums, zeros for the solution
    for n in ("close_a", "close_b", "close_third"):
        assert row(n)[0] == 4 and row(n)[1] > 0 and row(n)[13] > 0 and not row(n)[[7, 8, 9, 10, 11, 12, 16]].any()
    S = aux[g.names.index("close_a")]["S"]
    t = S[2, 2] - (S[1, 2] / math.sqrt(S[1, 1])) ** 2
    assert abs(t) / S[2, 2] < 2.0 ** -45
    assert all(row("crowd_%d" % t)[[3, 4, 5]].tolist() == [9, 7, 1] for t in range(10))
    no_rms = FR.forced_fit(g.map, None, g.jobs, g.nsigma, g.fit_bkg)[0]
    assert no_rms[g.names.index("isolated"), 2] == 0 and no_rms[g.names.index("bad_pixels"), 2] == 4
    cap, _ = FR.forced_fit(*FC.by_name("capped_520x515")[1:6])
    assert cap[0, [0, 17, 18, 19, 20, 21]].tolist() == [2, 1, 514, 1, 514, 1] and cap[0, 1] == 514 * 514 and cap[1, 0] == 0
    assert FR.forced_fit(*FC.by_name("map_1x1")[1:6])[0][:, 0].tolist() == [5, 3]
    assert FR.forced_fit(*FC.by_name("map_1x1_no_bkg")[1:6])[0][:, 0].tolist() == [0, 3]
    assert FR.forced_fit(*FC.by_name("n0")[1:6])[0].shape == (0, FR.FIELDS)


def test_planted_truth_on_the_random_scene():
    """The quoted error is the scatter: the rms of (amp - truth) / sqrt(amp_var) over all jobs lies in [0.75, 1.35].  A numpy
    prototype of the definition gave 0.93 to 1.11 on seeds 1 to 5.  Without the fitted constant it gave 1.9 (the 0.3 offset of the
    scene goes into the amplitudes), which is why fit_bkg is the default; that value is printed and asserted to be worse."""
    img, rms, jobs, truth = FC.random_scene(1)
    assert 230 <= len(jobs) <= 245
    ref, aux = FR.forced_fit(img, rms, jobs, 3.0, 1)
    assert np.isin(ref[:, 0], (0, 2)).all()
    pull = (ref[:, 7] - truth) / np.sqrt(ref[:, 8])
    value = float(np.sqrt((pull ** 2).mean()))
    conds = np.array([a["cond"] for a in aux])
    flat = FR.forced_fit(img, rms, jobs, 3.0, 0)[0]
    value0 = float(np.sqrt((((flat[:, 7] - truth) / np.sqrt(flat[:, 8])) ** 2).mean()))
    print("random scene, %d jobs: pull rms %.3f with the constant, %.3f without; scaled cond median %.3g, max %.3g" % (
        len(jobs), value, value0, np.median(conds), conds.max()))
    assert 0.75 <= value <= 1.35 and value0 > 1.35 and conds.max() < 1e4


def test_solution_bound_covers_a_perturbed_system():
    g = FC.by_name("main_64x96")
    ref, aux = FR.forced_fit(g.map, g.rms, g.jobs, g.nsigma, g.fit_bkg)
    a = aux[g.names.index("crowd_3")]
    S, x = a["S"], a["x"]
    rng = np.random.default_rng(3)
    dS = 1e-9 * np.abs(S)
    bound = FR.solution_bound(S[1:, 1:], x, dS[1:, 1:], dS[0, 1:])
    for _ in range(20):
        e = rng.uniform(-1, 1, S.shape)
        P = S + dS * (e + e.T) / 2
        x2 = np.linalg.solve(P[1:, 1:], P[0, 1:])
        assert (np.abs(x2 - x) <= 1.001 * bound + 1e-13 * np.abs(x).max()).all()


# ---- the host helpers
def _frow(status, amp=10.0, var=0.04, boff=0.5, npix=50, nneigh=1, crowded=0, chi2=40.0, corr=0.2):
    r = np.zeros(L.CY_FORCED_FIELDS)
    F = measure.FORCED
    r[F.status], r[F.npix], r[F.nneigh], r[F.crowded] = status, npix, nneigh, crowded
    if status in (0, 2):
        r[F.amp], r[F.amp_var], r[F.bkg_off], r[F.chi2], r[F.corr_max] = amp, var, boff, chi2, corr
    return r


def _sources():
    return [{"bkg": 1.0, "bkg_map": 2.0, "rms": 0.5, "rms_map": 0.25, "components": [{"x_peak": 1}, {"x_peak": 2}]},
            {"bkg": 3.0, "bkg_map": 4.0, "rms": 0.7, "rms_map": 0.35, "components": [{"x_peak": 3}]},
            {"bkg": 5.0, "bkg_map": 6.0, "rms": 0.9, "rms_map": 0.45, "components": None}]


def test_forced_jobs():
    comp = np.array([[9.0, 10.5, 20.25, 0.3, 0.01, 0.4], [7.0, 50.0, 60.0, 0.2, 0.0, 0.2]])
    index = np.array([[0, 1], [1, 0]])
    src = _sources()
    j = measure.forced_jobs(comp, index, src)
    assert j.shape == (2, L.CY_FORCED_JOB_FIELDS) and np.array_equal(j[:, :5], comp[:, 1:]) and j[:, 5].tolist() == [1.0, 3.0]
    assert measure.forced_jobs(comp, index, src, use_map=True)[:, 5].tolist() == [2.0, 4.0]
    mesh = np.zeros((2, 2, 2))
    mesh[:, :, 0] = [[1.0, 2.0], [3.0, 4.0]]
    j = measure.forced_jobs(comp, index, src, mesh=mesh, cell=64)
    assert j[:, 5].tolist() == [float(v) for v in measure.sample_mesh(mesh[:, :, 0], 64, comp[:, 1], comp[:, 2])] and j[0, 5] == 1.0
    assert measure.forced_jobs(comp, index, src, mesh=0.0)[:, 5].tolist() == [0.0, 0.0]
    assert measure.forced_jobs(np.zeros((0, 6)), np.zeros((0, 2)), src).shape == (0, L.CY_FORCED_JOB_FIELDS)
    assert L.FORCED_JOB_NAMES == ("x0", "y0", "a", "b", "c", "bkg")


def test_annotate_forced_on_hand_made_rows():
    src = _sources()
    index = np.array([[0, 1], [1, 0]])
    jobs = np.array([[10.5, 20.25, 0.25, 0.0, 0.25, 1.0], [50.0, 60.0, 0.2, 0.05, 0.3, 3.0]])
    m0 = dict(tag="self", rows=np.stack([_frow(0), _frow(4)]), jobs=jobs, beam_area=8.0, freq=1.0e9, err_scale=np.array([0.5, 0.7]))
    m1 = dict(tag="b", rows=np.stack([_frow(2, amp=5.0, var=0.01, boff=-0.25), _frow(0, amp=3.0)]), jobs=jobs + [0, 0, 0, 0, 0, 1.0], beam_area=0,
              freq=None, err_scale=None)
    measure.annotate_forced(src, index, [m0, m1])
    assert src[0]["components"][0]["forced"] is None and "forced" not in src[2]      # not rendered; a source without components is left alone
    f = src[0]["components"][1]["forced"]
    assert [e["image"] for e in f] == ["self", "b"] and all(tuple(e) == measure.FORCED_KEYS for e in f)
    fac = 2.0 * math.pi / math.sqrt(0.25 * 0.25) / 8.0
    assert f[0] == dict(image="self", status=0, npix=50, nneigh=1, crowded=0, peak=10.0, peak_err=math.sqrt(0.04) * 0.5, bkg=1.5, chi2=40.0, corr_max=0.2,
                        flux=10.0 * fac, flux_err=math.sqrt(0.04) * 0.5 * fac)
    assert f[1] == dict(image="b", status=2, npix=50, nneigh=1, crowded=0, peak=5.0, peak_err=None, bkg=1.75, chi2=40.0, corr_max=0.2, flux=None, flux_err=None)
    g = src[1]["components"][0]["forced"]
    assert g[0] == dict(image="self", status=4, npix=50, nneigh=1, crowded=0, peak=None, peak_err=None, bkg=None, chi2=None, corr_max=None, flux=None,
                        flux_err=None)
    assert g[1]["peak"] == 3.0 and g[1]["bkg"] == 4.5
    assert not any(k in c for s in src[:2] for c in s["components"] for k in measure.FORCED_ALPHA_KEYS)       # one frequency: no alpha keys
    m0["err_scale"] = np.array([0.0, 0.7])                    # an unweighted fit of a source without a noise: the value stays, the errors go
    measure.annotate_forced(src, index, [m0, m1])
    f = src[0]["components"][1]["forced"][0]
    assert f["peak"] == 10.0 and f["peak_err"] is None and f["flux"] == 10.0 * fac and f["flux_err"] is None
    json.dumps(src)


def test_alpha_on_hand_made_fluxes():
    # two points: the line through them; sigma_alpha from the weights: var = sum w / Delta
    nu1, nu2, S1 = 1.0e9, 2.0e9, 10.0
    S2 = S1 * (nu2 / nu1) ** -0.7
    a, e, n = measure.forced_alpha([(nu1, S1, 0.1), (nu2, S2, 0.2)])
    w1, w2 = (S1 / 0.1) ** 2, (S2 / 0.2) ** 2
    assert n == 2 and a == pytest.approx(-0.7, abs=1e-12) and e == pytest.approx(math.sqrt(1 / w1 + 1 / w2) / math.log(2.0), rel=1e-12)
    # three points on a line, and one off it pulls by its weight
    a, e, n = measure.forced_alpha([(nu, 5.0 * (nu / 1e9) ** 0.3, 0.05) for nu in (1e9, 1.5e9, 3e9)])
    assert n == 3 and a == pytest.approx(0.3, abs=1e-12)
    # one point, a non-positive flux, a missing error, the same frequency twice: no slope
    assert measure.forced_alpha([(nu1, S1, 0.1)]) == (None, None, None)
    assert measure.forced_alpha([(nu1, S1, 0.1), (nu2, -1.0, 0.1)]) == (None, None, None)
    assert measure.forced_alpha([(nu1, S1, 0.1), (nu2, S2, None)]) == (None, None, None)
    assert measure.forced_alpha([(nu1, S1, 0.1), (nu1, S2, 0.1)]) == (None, None, None)
    assert measure.forced_alpha([]) == (None, None, None)
    # through annotate_forced: fluxes when every map with a frequency has a beam, else peaks; the map without a frequency stays out
    jobs = np.array([[10.0, 20.0, 0.25, 0.0, 0.25, 0.0]])
    index = np.array([[0, 0]])

    def maps(beam2):
        return [dict(tag="self", rows=np.stack([_frow(0, amp=S1, var=0.01)]), jobs=jobs, beam_area=4.0, freq=nu1, err_scale=np.ones(1)),
                dict(tag="x", rows=np.stack([_frow(0, amp=99.0)]), jobs=jobs, beam_area=4.0, freq=None, err_scale=np.ones(1)),
                dict(tag="b", rows=np.stack([_frow(0, amp=S2, var=0.04)]), jobs=jobs, beam_area=beam2, freq=nu2, err_scale=np.ones(1))]
    src = [{"components": [{}]}]
    measure.annotate_forced(src, index, maps(0))
    c = src[0]["components"][0]
    assert c["forced_alpha"] == pytest.approx(-0.7, abs=1e-12) and c["forced_alpha_n"] == 2 and c["forced"][2]["flux"] is None
    measure.annotate_forced(src, index, maps(8.0))            # twice the beam: half the flux at nu2, one more unit of slope down
    c = src[0]["components"][0]
    assert c["forced_alpha"] == pytest.approx(-1.7, abs=1e-12) and c["forced_alpha_err"] > 0
    one = maps(4.0)
    one[2]["rows"] = np.stack([_frow(5)])
    measure.annotate_forced(src, index, one)
    c = src[0]["components"][0]
    assert (c["forced_alpha"], c["forced_alpha_err"], c["forced_alpha_n"]) == (None, None, None)


def test_header_readers():
    h = {"CDELT1": -0.001, "CDELT2": 0.001, "BMAJ": 0.005, "BMIN": 0.004, "BPA": 10.0}
    assert measure.header_beam_area(h) == pytest.approx(math.pi * 0.005 * 0.004 / (4 * math.log(2)) / 1e-6, rel=1e-14)
    assert measure.header_beam_area({k: v for k, v in h.items() if k != "BPA"}) == 0 and measure.header_beam_area(None) == 0
    assert measure.header_frequency({"RESTFRQ": 1.4e9, "FREQ": 9e8}) == 1.4e9 and measure.header_frequency({"RESTFREQ": 2e9, "FREQ": 9e8}) == 2e9
    assert measure.header_frequency({"FREQ": 9e8, "CTYPE3": "FREQ", "CRVAL3": 1e9}) == 9e8
    assert measure.header_frequency({"CTYPE3": "STOKES", "CRVAL3": 1.0, "CTYPE4": "FREQ-LSR", "CRVAL4": 3e9}) == 3e9
    assert measure.header_frequency({"CTYPE3": "FREQ", "CRVAL3": 1e9, "CTYPE4": "FREQ", "CRVAL4": 3e9}) == 1e9
    assert measure.header_frequency({"CTYPE3": "STOKES", "CRVAL3": 1.0}) is None and measure.header_frequency({}) is None and measure.header_frequency(None) is None
    assert measure.header_frequency({"FREQ": "n/a"}) is None and measure.header_frequency({"FREQ": 0.0}) is None
    # a continuum map's RESTFRQ = 0, or a value that is no number, is passed over for the next keyword
    assert measure.header_frequency({"RESTFRQ": 0.0, "FREQ": 9e8}) == 9e8 and measure.header_frequency({"RESTFRQ": "n/a", "CTYPE3": "FREQ", "CRVAL3": 1e9}) == 1e9
    assert measure.header_frequency({"RESTFRQ": float("nan"), "RESTFREQ": -1.0, "FREQ": float("inf")}) is None


# ---- plan, flags, exports
def test_plan_with_and_without_the_switch():
    for flag, steps in IMPLIED.items():
        assert measure.plan({flag: True}) == steps == measure.plan({flag: True, "forced_fit": False, "forced_images": ""}), flag
        assert set(measure.plan({flag: True, "forced_fit": True})) == set(steps) | set(RESIDUAL_STEPS)
    assert measure.plan({}) == () == measure.plan({"forced_fit": False})
    assert measure.plan({"forced_fit": True}) == RESIDUAL_STEPS == measure.plan({"save_residual_maps": True}) == measure.plan({"forced_images": "a.fits"})
    assert measure.wants_forced({"forced_fit": True}) and measure.wants_forced({"forced_images": ["a.fits"]}) and not measure.wants_forced({})
    assert measure.forced_config({}) == (3.0, True, []) and measure.forced_config({"forced_images": "a.fits, b.fits", "forced_nsigma": 2, "forced_fit_bkg": 0}) == (
        2.0, False, ["a.fits", "b.fits"])


def test_flags_parse_and_imply():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import run
    w = "--weights=seeded:l:5"
    base = run.measure_config(run.parse_args([w]))
    assert base["forced_fit"] is False and base["forced_images"] == "" and measure.plan(base) == () and not measure.wants_forced(base)
    args = run.parse_args([w, "--forced_fit"])
    config = run.measure_config(args)
    assert config["forced_fit"] is True and measure.plan(config) == RESIDUAL_STEPS and args.residual_map and not args.bkg_map
    assert (config["forced_nsigma"], config["forced_fit_bkg"]) == (3.0, 1)
    args = run.parse_args([w, "--forced_images", "a.fits,b.fits", "--forced_nsigma", "2.5", "--forced_fit_bkg", "0"])
    config = run.measure_config(args)
    assert config["forced_fit"] is True and measure.forced_config(config) == (2.5, False, ["a.fits", "b.fits"]) and args.residual_map
    for bad in (["--forced_fit", "--forced_nsigma=0.5"], ["--forced_fit", "--forced_nsigma=9"], ["--forced_fit", "--forced_fit_bkg=2"]):
        with pytest.raises(SystemExit):
            run.parse_args([w] + bad)
    for flag in ("forced_fit", "forced_images", "forced_nsigma", "forced_fit_bkg"):
        assert "--" + flag in run.__doc__ and flag in run.MEASURE_KEYS, flag
    assert "--forced_fit" in open(os.path.join(ROOT, "README.md")).read()


def test_exports():
    assert {"cy_forced_fit", "cy_forced_kernel_ms"} <= set(L.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "caesar_yolo_hip.h")).read()
    defines = [line.split()[:3] for line in hdr.split("\n") if line.startswith("#define CY_FORCED")]
    assert ["#define", "CY_FORCED_FIELDS", "24"] in defines and ["#define", "CY_FORCED_JOB_FIELDS", "6"] in defines and ["#define", "CY_FORCED_NEIGH_MAX", "7"] in defines
    assert (L.CY_FORCED_FIELDS, L.CY_FORCED_JOB_FIELDS, L.CY_FORCED_NEIGH_MAX, L.CY_FORCED_JOBS_MAX) == (24, 6, 7, 1 << 20) == (FR.FIELDS, FR.JOB_FIELDS, FR.NEIGH_MAX, FR.JOBS_MAX)
    assert "int cy_forced_fit(cy_ctx* ctx, const float* d_map, const float* d_rms /* or NULL */, int MH, int MW," in hdr
    assert "int cy_forced_kernel_ms(const cy_ctx* ctx, double* out_ms);" in hdr
    assert len(L.FORCED_NAMES) == L.CY_FORCED_FIELDS and L.FORCED_NAMES == FR.NAMES
    lib = L.load()
    assert hasattr(lib, "cy_forced_fit") and hasattr(lib, "cy_forced_kernel_ms")
    jobs = open(os.path.join(ROOT, "caesar_yolo_amd", "csrc", "cy_measure_jobs.h")).read()
    assert "FORCED_FIELDS = 24;" in jobs and "FORCED_NEIGH_MAX = 7;" in jobs
    import __graft_entry__ as ge
    assert "cy_forced.hip" in ge.HIP_SOURCES
    from caesar_yolo_amd.model import HipDetector
    assert callable(HipDetector.forced_fit) and callable(HipDetector.forced_kernel_ms)


# ---- Chain.run on the replay detector
class ForcedReplay(Replay):
    """Replay plus forced_fit, and the mesh calls on the other maps: hand-made rows, every argument kept."""

    def __init__(self, scenario, ndef_of=None):
        Replay.__init__(self, scenario)
        self.forced_args, self.map_meshes, self.ndef_of, self.uploads, self.turned_away = [], [], ndef_of or {}, [], None

    def upload(self, name):
        def up(det):
            assert det is self
            self.calls.append("upload")
            t = np.full(SHAPE, float(len(self.uploads) + 1), np.float32)
            self.uploads.append((name, t))
            return t
        return up

    def _other(self, img):
        return next((nm for nm, t in self.uploads if t is img), None)

    def measure_background(self, img, cell=128, k=3.0, niter=3):
        nm = self._other(img)
        if nm is None:
            return Replay.measure_background(self, img, cell, k, niter)
        self.calls.append("measure_background")
        ncy, ncx = -(-SHAPE[0] // cell), -(-SHAPE[1] // cell)
        raw = np.zeros((ncy, ncx, L.CY_BKG_FIELDS))
        raw[:, :, measure.BKG.n] = 1000 if self.ndef_of.get(nm, 1) else 0
        raw[:, :, measure.BKG.bkg] = 0.125 * (1 + np.arange(ncy * ncx).reshape(ncy, ncx))
        raw[:, :, measure.BKG.rms] = 2.0
        self.map_meshes.append(dict(name=nm, cell=cell, k=k, niter=niter, raw=raw))
        return raw

    def expand_background(self, mesh, cell, shape, want=("bkg", "rms")):
        if self.map_meshes and np.array_equal(mesh, measure.fill_mesh(self.map_meshes[-1]["raw"])[0]):
            self.calls.append("expand_background")
            self.map_meshes[-1]["expanded"] = (want, tuple(shape))
            self.rms_other = np.full(shape, 2.0, np.float32)
            return None, self.rms_other
        out = Replay.expand_background(self, mesh, cell, shape, want)
        self.rms_self = out[1]
        return out

    def render_gaussians(self, img, comp, nsigma=5.0, bkg_dev=None):
        rows, model, resid = Replay.render_gaussians(self, img, comp, nsigma, bkg_dev)
        if self.turned_away is not None:                      # the render call turns one selected component away
            rows = np.array(rows, np.float64)
            rows[self.turned_away, 0] = 3.0
        return rows, model, resid

    def forced_fit(self, map_dev, rms_dev, jobs, nsigma=3.0, fit_bkg=True):
        self.calls.append("forced_fit")
        jobs = np.array(jobs, np.float64)
        self.forced_args.append(dict(map_dev=map_dev, rms_dev=rms_dev, jobs=jobs, nsigma=nsigma, fit_bkg=fit_bkg))
        call = len(self.forced_args)
        return np.stack([_frow((0, 2, 4, 5, 0)[i % 5], amp=10.0 * call + i, var=0.01 * (i + 1), crowded=i % 2) for i in range(len(jobs))]).reshape(len(jobs), L.CY_FORCED_FIELDS)


def test_chain_without_the_switch_is_what_it_was():
    s, kw = _setup("B")
    det0, stats0 = Replay("B"), {}                            # has no forced_fit: a call would raise
    chain0 = measure.Chain(det0, np.zeros(SHAPE, np.float32), s["sources"], s["config"], **kw).run(measure.plan(s["config"]), stats0)
    s1, _ = _setup("B")
    config = dict(s1["config"], forced_fit=False, forced_images="", forced_nsigma=2.0, forced_fit_bkg=0)
    det1, stats1 = Replay("B"), {}
    chain1 = measure.Chain(det1, np.zeros(SHAPE, np.float32), s1["sources"], config, **kw).run(measure.plan(config), stats1)
    assert measure.plan(config) == measure.plan(s["config"]) and det1.calls == det0.calls and "forced_fit" not in det0.calls
    assert set(stats1) == set(stats0) and not set(stats0) & set(measure.FORCED_STATS)
    assert chain0.forced_rows is None and chain0.forced_images is None and chain0.forced_stats is None
    assert measure.peak_lists(chain0) == {} == measure.peak_lists(chain1)
    assert json.dumps(s["sources"]) == json.dumps(s1["sources"])
    assert not [k for o in s["sources"] for c in o["components"] or [] for k in c if k.startswith("forced")]


@pytest.mark.parametrize("scenario", ["A", "B"])
def test_chain_with_the_switch(scenario):
    s, kw = _setup(scenario)
    s0, _ = _setup(scenario)
    det0, stats0 = Replay(scenario), {}
    chain0 = measure.Chain(det0, np.zeros(SHAPE, np.float32), s0["sources"], s0["config"], **kw).run(measure.plan(s0["config"]), stats0)
    config = dict(s["config"], forced_fit=True, forced_nsigma=2.5, forced_fit_bkg=0, image_path="field.fits")
    det, stats = ForcedReplay(scenario, ndef_of={"second": 1, "third": 0}), {}
    others = [dict(tag="second", path="dir/second.fits", freq=2.0e9, beam_area=6.0, upload=det.upload("second")),
              dict(tag="third", path="third.fits", freq=None, beam_area=0, upload=det.upload("third"))]
    img = np.zeros(SHAPE, np.float32)
    steps = measure.plan(config)
    assert steps == measure.plan(s0["config"])                # the fixture's configs ask for the residual step already
    chain = measure.Chain(det, img, s["sources"], config, freq=1.0e9, forced_maps=others, **kw).run(steps, stats)
    weighted = scenario == "B"
    # the order: everything the run without the switch called, then per map its calls
    assert det.calls[:len(det0.calls)] == det0.calls
    assert det.calls[len(det0.calls):] == (["expand_background"] if weighted else []) + ["forced_fit"] + \
        ["upload", "measure_background", "expand_background", "forced_fit"] + ["upload", "measure_background", "forced_fit"]
    # the components are the rendered ones, in the pixel frame
    comp, index, _ = measure.render_selection(s0["sources"], chain0.fit_pixel_rows, chain0.blend_pixel_rows)
    assert np.array_equal(chain.render_comp, comp) and np.array_equal(chain.render_index, index) and len(comp) >= 2
    assert np.array_equal(chain.forced_comp, comp) and np.array_equal(chain.forced_index, index)       # the recorded render rows are all status 0
    a0, a1, a2 = det.forced_args
    assert all(a["nsigma"] == 2.5 and a["fit_bkg"] is False for a in det.forced_args)
    assert a0["map_dev"] is img and (a0["rms_dev"] is det.rms_self if weighted else a0["rms_dev"] is None)
    assert np.array_equal(a0["jobs"], measure.forced_jobs(comp, index, s0["sources"], weighted))
    assert a0["jobs"][:, 5].tolist() == [s0["sources"][i]["bkg_map" if weighted else "bkg"] for i in index[:, 0]]
    # the second map: its own mesh with the chain's parameters, its rms map, the mesh sampled at the centres
    m1, m2 = det.map_meshes
    assert a1["map_dev"] is det.uploads[0][1] and a1["rms_dev"] is det.rms_other and m1["name"] == "second" and m1["expanded"] == (("rms",), SHAPE)
    assert (m1["cell"], m1["k"], m1["niter"]) == (chain.cell, chain.clip_sigma, chain.clip_iters) == (m2["cell"], m2["k"], m2["niter"])
    mesh1 = measure.fill_mesh(m1["raw"], chain.min_pix)[0]
    assert np.array_equal(a1["jobs"], measure.forced_jobs(comp, index, s0["sources"], mesh=mesh1, cell=chain.cell)) and a1["jobs"][:, 5].min() >= 0.125
    # the third map has no defined cell: unweighted, bkg 0, errors None
    assert a2["map_dev"] is det.uploads[1][1] and a2["rms_dev"] is None and not a2["jobs"][:, 5].any() and np.array_equal(a2["jobs"][:, :5], comp[:, 1:])
    assert "expanded" not in m2
    # the catalog: what annotate_forced gives for these rows; everything else is what it was
    scale = np.ones(len(comp)) if weighted else np.array([s0["sources"][i]["rms"] for i in index[:, 0]], np.float64)
    probe, _ = _setup(scenario)
    probe = json.loads(json.dumps(s0["sources"]))
    maps = [dict(tag="self", rows=chain.forced_rows["self"], jobs=a0["jobs"], beam_area=kw["beam_area"], freq=1.0e9, err_scale=scale),
            dict(tag="second", rows=chain.forced_rows["second"], jobs=a1["jobs"], beam_area=6.0, freq=2.0e9, err_scale=np.ones(len(comp))),
            dict(tag="third", rows=chain.forced_rows["third"], jobs=a2["jobs"], beam_area=0, freq=None, err_scale=None)]
    measure.annotate_forced(probe, index, maps)
    assert json.loads(json.dumps(s["sources"])) == probe
    rendered = {(int(i), int(k)) for i, k in index}
    for i, (o, o0) in enumerate(zip(s["sources"], s0["sources"])):
        assert {k: v for k, v in o.items() if k != "components"} == {k: v for k, v in o0.items() if k != "components"}
        for k, (c, c0) in enumerate(zip(o["components"] or [], o0["components"] or [])):
            assert {key: v for key, v in c.items() if not key.startswith("forced")} == c0
            if (i, k) not in rendered:
                assert c["forced"] is None and "forced_alpha" not in c
                continue
            assert [e["image"] for e in c["forced"]] == ["self", "second", "third"] and tuple(c)[-4:] == ("forced",) + measure.FORCED_ALPHA_KEYS
            assert all(e["peak_err"] is None for e in c["forced"][2:]) and all(e["flux"] is None for e in c["forced"][2:])
            t = [tuple(r) for r in index.tolist()].index((i, k))
            if t % 5 in (0, 1, 4):
                assert c["forced"][0]["peak"] == 10.0 + t and c["forced"][1]["peak"] == 20.0 + t
                assert c["forced"][0]["peak_err"] == math.sqrt(0.01 * (t + 1)) * scale[t]
                assert (c["forced"][0]["flux"] is None) == (not kw["beam_area"])
                assert c["forced_alpha_n"] == 2 and c["forced_alpha"] is not None
            else:
                assert c["forced"][0]["peak"] is None and c["forced_alpha_n"] is None
    lists = measure.peak_lists(chain)
    assert lists == {"forced_images": [
        dict(tag="self", path="field.fits", freq=1.0e9, beam_area=float(kw["beam_area"] or 0), mesh_ndef=chain.ndef if weighted else None),
        dict(tag="second", path="dir/second.fits", freq=2.0e9, beam_area=6.0, mesh_ndef=m1["raw"].shape[0] * m1["raw"].shape[1]),
        dict(tag="third", path="third.fits", freq=None, beam_area=0.0, mesh_ndef=0)]}
    json.dumps(lists)
    # the stats: the old keys with their old counts, plus the seven new ones
    old = {k for k in stats if k not in measure.FORCED_STATS}
    assert set(stats) == old | set(measure.FORCED_STATS) and old == set(stats0)
    assert {k: stats[k] for k in old if not k.endswith("_ms")} == {k: stats0[k] for k in old if not k.endswith("_ms")}
    m = len(comp)
    status = np.concatenate([chain.forced_rows[t][:, 0] for t in ("self", "second", "third")])
    assert (stats["forced_maps"], stats["forced_jobs"]) == (3, 3 * m) and stats["forced_kernel_ms"] == 3 * KERNEL_MS and stats["forced_ms"] >= 0.0
    assert stats["forced_fitted"] == int(np.isin(status, (0, 2)).sum()) and stats["forced_singular"] == int((status == 4).sum())
    assert stats["forced_crowded"] == 3 * (m // 2)


def test_a_component_the_render_call_turned_away_is_not_forced():
    s, kw = _setup("A")
    det = ForcedReplay("A")
    det.turned_away = 1
    config = dict(s["config"], forced_fit=True)
    chain = measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], config, **kw).run(measure.plan(config), {})
    keep = np.arange(len(chain.render_comp)) != 1
    assert np.array_equal(chain.forced_comp, chain.render_comp[keep]) and np.array_equal(chain.forced_index, chain.render_index[keep])
    assert np.array_equal(det.forced_args[0]["jobs"][:, :5], chain.render_comp[keep][:, 1:])
    i, k = (int(v) for v in chain.render_index[1])
    c = s["sources"][i]["components"][k]
    assert c["rendered"] is False and c["render_status"] == 3 and c["forced"] is None
    assert all((c["forced"] is None) == (not c["rendered"]) for o in s["sources"] for c in o["components"] or [])


def test_a_map_of_another_shape_is_refused():
    s, kw = _setup("A")
    det = ForcedReplay("A")
    bad = dict(tag="bad", path="bad.fits", freq=None, beam_area=0, upload=lambda d: np.zeros((SHAPE[0], SHAPE[1] + 1), np.float32))
    config = dict(s["config"], forced_fit=True)
    with pytest.raises(L.CyError):
        measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], config, forced_maps=[bad], **kw).run(measure.plan(config), {})


def test_chain_forces_nothing_without_the_residual_step():
    s, kw = _setup("A")
    det, stats = ForcedReplay("A"), {}
    chain = measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], dict(s["config"], forced_fit=True), **kw).run(("measure", "islands"), stats)
    assert det.calls == ["measure_sources", "measure_islands"] and chain.forced_rows is None and not set(stats) & set(measure.FORCED_STATS)
