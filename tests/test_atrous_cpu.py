"""The a trous decomposition and the scale search without a GPU: the two restatements of tests/atrous_ref.py against each other on the
small cases of tests/atrous_cases.py, annotate_scale_peaks on hand-made rows, plan() and the command line for the new flags, the
library's exports, measure.Chain.run on the replay detector of tests/test_measure_chain_cpu.py with and without the switch, and the
chain scene of tests/atrous_chain_ref.py on the numpy references."""
import json
import os
import sys

import numpy as np
import pytest

import atrous_cases as AC
import atrous_chain_ref as ACR
import atrous_ref as AR
from caesar_yolo_amd import lib as L
from caesar_yolo_amd import measure
from test_measure_chain_cpu import IMPLIED, KERNEL_MS, SHAPE, Replay, _setup, _stat_keys, Z
from test_peaks_cpu import PEAK_STEPS, FakeWCS, PeakReplay, _row, _sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE_STATS = {"scales_ms", "atrous_kernel_ms", "scales_background_kernel_ms", "scales_peaks_kernel_ms", "scales_found", "scales_kept",
               "scales_strongest", "scales_truncated"}
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the reference
@pytest.mark.parametrize("name", AC.LOOPS)
def test_the_two_restatements_agree(name):
    c = AC.case(name)
    smooth, detail = AC.reference()[name]
    s2, d2 = AR.atrous_loops(c.map, c.step)
    assert np.array_equal(bits(smooth), bits(s2)) and np.array_equal(bits(detail), bits(d2))
    assert not np.isnan(smooth).any() and not np.isnan(detail).any()


def test_fold():
    assert [AR.fold_int(i, 1) for i in (-5, 0, 9)] == [0, 0, 0] and AR.fold(np.array([-5, 0, 9]), 1).tolist() == [0, 0, 0]
    assert [AR.fold_int(i, 2) for i in range(-3, 4)] == [1, 0, 1, 0, 1, 0, 1]
    assert [AR.fold_int(i, 5) for i in range(-9, 14)] == [1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3]
    for N in (1, 2, 3, 7, 75):
        i = np.arange(-300, 300)
        assert AR.fold(i, N).tolist() == [AR.fold_int(int(v), N) for v in i] and AR.fold(i, N).min() >= 0 and AR.fold(i, N).max() <= N - 1


def test_the_cases_hold_what_they_are_for():
    ref = AC.reference()
    names = [c.name for c in AC.cases()]
    assert len(set(names)) == len(names)
    for h, w in AC.TINY:
        for s in AC.TINY_STEPS:
            assert "%dx%d_s%d" % (h, w, s) in ref
    assert np.array_equal(bits(ref["1x1_s64"][0]), bits(AC.case("1x1_s64").map)) and not bits(ref["1x1_s64"][1]).any()
    # a unit impulse returns the 5 x 5 kernel: every pixel collects the taps whose folded position is the impulse
    k2 = np.outer(AR.H, AR.H)
    for name, (y0, x0) in AC.IMPULSES.items():
        for s in (1, 2):
            want = np.zeros((17, 19), np.float64)
            for y in range(17):
                for x in range(19):
                    want[y, x] = sum(k2[dy, dx] for dy in range(5) for dx in range(5)
                                     if (AR.fold_int(y + (dy - 2) * s, 17), AR.fold_int(x + (dx - 2) * s, 19)) == (y0, x0))
            smooth, detail = ref["impulse_%s_s%d" % (name, s)]
            assert np.array_equal(smooth, want.astype(np.float32)) and (want > 0).sum() == {"corner": 9, "edge": 15, "interior": 25}[name], (name, s)
            assert np.array_equal(detail, (AC.case("impulse_%s_s%d" % (name, s)).map - want).astype(np.float32))
    inner = ref["impulse_interior_s2"][0]
    assert inner.sum() == 1.0 and np.array_equal(inner[4:13:2, 5:14:2], k2.astype(np.float32)) and inner[8, 9] == 0.140625
    assert ref["impulse_corner_s1"][0][0, 0] == 0.140625 and ref["impulse_corner_s1"][0][1, 1] == 0.0625 and ref["impulse_corner_s1"][0][2, 0] == 0.0625 * 0.375
    # a constant plane: smooth is the constant, detail exactly 0
    for name in ("constant_s1", "constant_s8"):
        assert np.array_equal(bits(ref[name][0]), bits(AC.case(name).map)) and not bits(ref[name][1]).any()
    # values of every kind; non-finite inputs count as 0, so no output is NaN; a detail may overflow
    m = AC.special_map()
    assert np.isnan(m).sum() == 2 and np.isinf(m).sum() == 2 and (m == 0).sum() == 4 and (np.abs(m[np.isfinite(m)]) > 1e38).sum() == 31
    assert ((m != 0) & (np.abs(m) < 1.1754944e-38)).sum() == 3
    for s in (1, 3):
        assert np.isfinite(ref["special_s%d" % s][0]).all() and not np.isnan(ref["special_s%d" % s][1]).any()
    assert ref["special_s1"][1][16, 16] == np.inf and np.isfinite(ref["special_s3"][1]).all()
    # geometry: one pixel beyond one and two column blocks and row chunks, and more work items than workgroups
    shape = lambda n: AC.case(n).map.shape
    assert shape("cols_and_1")[1] == AC.COLS + 1 and shape("two_cols_and_1")[1] == 2 * AC.COLS + 1
    assert shape("chunk_and_1")[0] == AC.CHUNK + 1 and shape("two_chunks_and_1")[0] == 2 * AC.CHUNK + 1
    assert -(-shape("chunk_and_1_s2")[0] // 2) == AC.CHUNK + 1 and shape("two_chunks_and_1_s2")[0] // 2 == 2 * AC.CHUNK + 1
    for name in ("tall_s1", "tall_s3"):
        assert AC.items(shape(name)[0], shape(name)[1], AC.case(name).step) > AC.GRID_MAX
    assert AC.items(64, 96, 1) == 1 and AC.items(65, 257, 1) == 4 and AC.items(5, 31, 64) == 5
    # w_1 + ... + w_J + c_J is the map again (up to the fp32 roundings of the planes)
    img = AC.case("70x75_s1").map
    pl = AR.planes(img, 4)
    back = pl[-1][0].astype(np.float64) + sum(w.astype(np.float64) for _, w in pl)
    assert np.abs(back - img).max() <= 4 * 2.0 ** -24 * np.abs(img).max()


# ---- annotate_scale_peaks
def test_annotate_scale_peaks_on_hand_made_rows():
    # steps: scale 2 -> 2, scale 4 -> 8.  Distances are measured between peak pixels, limit 2 max(step_e, step_f), inclusive
    lv2 = np.array([
        _row(100, 100, 10.0, 1.0, 5, 40.0, 36.0, 9.0, -18.0),     # snr 10: the strongest of its neighbourhood
        _row(104, 100, 9.0, 1.0, 5, 30.0, 30.0, 0.0, 0.0),        # snr 9, |dx| = 4 = 2 * 2 of the first: not strongest
        _row(105, 104, 8.0, 1.0, 5, 30.0, 30.0, 0.0, 0.0),        # snr 8, |dx| = 5 of the first, but |dx| = 1, |dy| = 4 of the second (itself not strongest): not strongest
        _row(105, 109, 7.0, 1.0, 5, 30.0, 30.0, 0.0, 0.0),        # snr 7, |dy| = 5 of the third, one beyond: strongest
        _row(300, 300, 6.0, 1.0, 2, 30.0, 30.0, 0.0, 0.0),        # nabove below min_above: dropped, and shadows nothing
        _row(25, 25, 6.0, 1.0, 4, 12.0, 12.0, 0.0, 0.0),          # snr 6, equal to the scale-4 row below: scale 2 comes first, in boxes 0 and 1
    ], np.float64)
    lv4 = np.array([
        _row(200, 200, 12.0, 1.0, 9, 99.0, 99.0, 0.0, 0.0),       # snr 12, leads the list
        _row(41, 25, 6.0, 1.0, 9, 50.0, 50.0, 0.0, 0.0),          # snr 6, |dx| = 16 of (25, 25), which comes first on equal snr: not strongest
        _row(300, 317, 5.0, 1.0, 9, 50.0, 50.0, 0.0, 0.0),        # snr 5; the dropped row is no rival: strongest
        _row(216, 217, 4.0, 1.0, 9, 50.0, 50.0, 0.0, 0.0),        # snr 4, |dx| = 16 but |dy| = 17 of (200, 200), one beyond: strongest
    ], np.float64)
    src = _sources()
    out = measure.annotate_scale_peaks(src, [(2, 2, lv2, 6), (4, 8, lv4, 9)], 3, 4.0, FakeWCS(), origin=(1000, 2000))
    assert [tuple(d) for d in out] == [measure.SCALE_PEAK_KEYS] * 9 and measure.SCALE_PEAK_KEYS[:len(measure.PEAK_KEYS)] == measure.PEAK_KEYS
    got = [(d["scale"], d["step"], d["x_peak"], d["y_peak"], d["snr"], d["strongest"]) for d in out]
    assert got == [(4, 8, 200, 200, 12.0, True), (2, 2, 100, 100, 10.0, True), (2, 2, 104, 100, 9.0, False), (2, 2, 105, 104, 8.0, False),
                   (2, 2, 105, 109, 7.0, True), (2, 2, 25, 25, 6.0, True), (4, 8, 41, 25, 6.0, False), (4, 8, 300, 317, 5.0, True),
                   (4, 8, 216, 217, 4.0, True)]
    d = out[1]
    assert (d["x"], d["y"]) == (100.25, 99.5) and (d["ra"], d["dec"]) == (100.0 + 1100.25 / 10.0, -40.0 + 2099.5 / 10.0)
    assert (d["peak"], d["rms"], d["npix"], d["nabove"], d["flux_sum"], d["flux"], d["in_source"]) == (10.0, 1.0, 25, 5, 40.0, 10.0, 2)
    assert type(d["scale"]) is int and type(d["step"]) is int and type(d["strongest"]) is bool
    assert [d["in_source"] for d in out[5:7]] == [0, None]
    assert [(s["res_nscale_peaks"], s["res_scale_peak_snr"]) for s in src] == [(1, 6.0), (1, 6.0), (4, 10.0)]
    assert not [k for s in src for k in s if k in measure.SOURCE_PEAK_KEYS + measure.SOURCE_HOLE_KEYS]
    json.dumps(out)
    # across scales the limit is 2 * the larger step: |dx| = 17 at steps 8 and 2 keeps both, exactly 16 does not
    for x, want in ((117, [True, True]), (116, [True, False]), (84, [True, False]), (83, [True, True])):
        far = measure.annotate_scale_peaks([], [(2, 2, lv2[:1], 1), (4, 8, np.array([_row(x, 100, 12.0, 1.0, 9, 1.0, 1.0, 0.0, 0.0)]), 1)], 3, 0, None)
        assert [d["strongest"] for d in far] == want and [d["scale"] for d in far] == [4, 2], x
    # within one scale the limit is that scale's: 2 * 2
    one = measure.annotate_scale_peaks([], [(2, 2, lv2[:2], 2)], 3, 0, None)
    assert [d["strongest"] for d in one] == [True, False] and all(d["flux"] is None and d["ra"] is None and d["dec"] is None for d in one)
    # min_above 1 keeps the dropped row: (300, 317) is 17 rows from it and stays strongest; at 16 rows it does not
    kept = measure.annotate_scale_peaks([], [(2, 2, lv2, 6), (4, 8, lv4, 9)], 1, 0, None)
    assert len(kept) == 10 and [d["strongest"] for d in kept if d["x_peak"] == 300] == [True, True]
    near = lv4.copy()
    near[2, 1] = 316.0
    kept = measure.annotate_scale_peaks([], [(2, 2, lv2, 6), (4, 8, near, 9)], 1, 0, None)
    assert [d["strongest"] for d in kept if d["x_peak"] == 300] == [True, False]
    # empty inputs: no level, levels without rows, no source
    assert measure.annotate_scale_peaks([], [], 3, 4.0, None) == []
    src = _sources()
    assert measure.annotate_scale_peaks(src, [(2, 2, np.zeros((0, L.CY_PEAK_FIELDS)), 0), (3, 4, np.zeros((0, L.CY_PEAK_FIELDS)), 0)], 3, 4.0, None) == []
    assert [(s["res_nscale_peaks"], s["res_scale_peak_snr"]) for s in src] == [(0, None)] * 3


def test_strongest_rule_against_the_pairwise_loop():
    """300 random entries per scale on a 100 x 100 field, dense enough that most are shadowed: the bisection form against all pairs."""
    rng = np.random.default_rng(4)
    levels = []
    for j in (1, 2, 4):
        xy, v = rng.integers(0, 100, (300, 2)), rng.integers(5, 40, 300).astype(np.float64)       # many equal snr
        levels.append((j, 1 << (j - 1), np.array([_row(x, y, s, 1.0, 9, 1.0, 1.0, 0.0, 0.0) for (x, y), s in zip(xy, v)]), 300))
    out = measure.annotate_scale_peaks([], levels, 3, 0, None)
    key = [(-d["snr"], d["scale"], d["y_peak"], d["x_peak"]) for d in out]
    assert len(out) == 900 and key == sorted(key)
    for i, e in enumerate(out):
        near = [f for f in out[:i] if max(abs(e["x_peak"] - f["x_peak"]), abs(e["y_peak"] - f["y_peak"])) <= 2 * max(e["step"], f["step"])]
        assert e["strongest"] == (not near), i
    assert 5 < sum(d["strongest"] for d in out) < 200


def test_annotate_peaks_is_what_it_was():
    """The helpers annotate_peaks now shares give the rows of tests/test_peaks_cpu.py the dicts they gave before."""
    rows = np.array([_row(25, 25, 12.0, 2.0, 5, 40.0, 36.0, 9.0, -18.0), _row(12, 30, 16.0, 2.0, 3, 50.0, 50.0, 0.0, 25.0)], np.float64)
    src = _sources()
    out = measure.annotate_peaks(src, rows, 2, 3, 4.0, None)
    assert [tuple(d) for d in out] == [measure.PEAK_KEYS] * 2 and [d["in_source"] for d in out] == [0, 0]
    assert out[1] == {"x_peak": 25, "y_peak": 25, "x": 25.25, "y": 24.5, "ra": None, "dec": None, "peak": 12.0, "rms": 2.0, "snr": 6.0, "npix": 25,
                      "nabove": 5, "flux_sum": 40.0, "flux": 10.0, "in_source": 0}
    assert [(s["res_npeaks"], s["res_peak_snr"]) for s in src] == [(2, 8.0), (1, 6.0), (0, None)] and "res_nscale_peaks" not in src[0]


# ---- plan() and the command line
def test_plan_and_steps():
    assert measure.STEPS == ("measure", "background", "islands", "deblend", "fit", "blend", "residual")
    for flag, steps in IMPLIED.items():
        assert measure.plan({flag: True}) == steps and not measure.wants_scales({flag: True}), flag
        assert measure.plan({flag: True, "residual_scales": 0}) == steps
    for flag in ("residual_peaks", "residual_holes"):
        assert measure.plan({flag: True}) == PEAK_STEPS and not measure.wants_scales({flag: True})
    for J in (1, 4, 6):
        assert measure.plan({"residual_scales": J}) == PEAK_STEPS and measure.wants_scales({"residual_scales": J})
        assert not measure.wants_peaks({"residual_scales": J})
        assert measure.plan({"residual_scales": J, "fit_blends": True}) == measure.STEPS
    assert measure.plan({}) == () and not measure.wants_scales({}) and not measure.wants_scales({"residual_scales": 0})
    assert measure.scales_config({}) == (0, 2, 5.0) and measure.scales_config({"residual_scales": 4, "residual_scale_first": 3, "residual_scales_sigma": 4.5}) == (4, 3, 4.5)
    assert [measure.scale_cell(32, s) for s in (1, 2, 4, 8, 16, 32)] == [32, 32, 64, 128, 256, 512] and measure.scale_cell(128, 4) == 128
    assert measure.scale_cell(4096, 32) == 4096 and measure.scale_cell(64, 512) == 4096
    assert [measure.scale_radius(2, s) for s in (1, 2, 4, 8, 16, 32)] == [2, 2, 4, 8, 8, 8] and measure.scale_radius(5, 2) == 5


def test_flags_parse_and_imply():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import run
    w = "--weights=seeded:l:5"
    base = run.measure_config(run.parse_args([w]))
    assert (base["residual_scales"], base["residual_scale_first"], base["residual_scales_sigma"], base["save_scale_maps"]) == (0, 2, 5.0, False)
    assert measure.plan(base) == () and not measure.wants_scales(base) and measure.scales_config(base) == measure.scales_config({})
    args = run.parse_args([w, "--residual_scales=4"])
    config = run.measure_config(args)
    assert config["residual_scales"] == 4 and measure.plan(config) == PEAK_STEPS and measure.wants_scales(config) and not measure.wants_peaks(config)
    assert args.residual_map and args.bkg_map and args.fit_components and not args.fit_blends and not args.residual_peaks
    args = run.parse_args([w, "--residual_scales", "6", "--residual_scale_first", "6", "--residual_scales_sigma", "4.5", "--save_scale_maps"])
    assert measure.scales_config(run.measure_config(args)) == (6, 6, 4.5) and run.measure_config(args)["save_scale_maps"] is True
    assert run.parse_args([w, "--residual_scales=1", "--residual_scale_first=1"]).residual_scale_first == 1
    for bad in (["--residual_scales=7"], ["--residual_scales=-1"], ["--residual_scales=2.5"], ["--residual_scales=4", "--residual_scale_first=5"],
                ["--residual_scales=4", "--residual_scale_first=0"], ["--residual_scales=1"]):
        with pytest.raises(SystemExit):
            run.parse_args([w] + bad)
    run.parse_args([w, "--residual_scale_first=9"])           # without the switch the first scale is not looked at
    for flag in ("residual_scales", "residual_scale_first", "residual_scales_sigma", "save_scale_maps"):
        assert "--" + flag in run.__doc__ and flag in run.MEASURE_KEYS, flag
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--residual_scales" in readme and "--save_scale_maps" in readme


def test_sigma_out_of_range_is_refused(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import run
    fits = tmp_path / "x.fits"
    fits.write_bytes(b"")
    ok = run.parse_args(["--weights=seeded:l:5", "--image=%s" % fits, "--residual_scales=4"])
    assert run.validate_args(ok) == 0
    for sigma in ("0", "-1", "nan", "inf"):
        assert run.validate_args(run.parse_args(["--weights=seeded:l:5", "--image=%s" % fits, "--residual_scales_sigma=" + sigma])) == -1


def test_exports():
    assert {"cy_atrous_step", "cy_atrous_kernel_ms"} <= set(L.EXPORTS) and L.CY_ATROUS_STEP_MAX == AR.STEP_MAX == 64
    lib = L.load()
    assert hasattr(lib, "cy_atrous_step") and hasattr(lib, "cy_atrous_kernel_ms")
    hdr = open(os.path.join(ROOT, "include", "caesar_yolo_hip.h")).read()
    assert "#define CY_ATROUS_STEP_MAX 64" in hdr and "int cy_atrous_step(cy_ctx* ctx, const float* d_in, int MH, int MW, int step," in hdr
    assert "int cy_atrous_kernel_ms(const cy_ctx* ctx, double* out_ms);" in hdr
    jobs = open(os.path.join(ROOT, "caesar_yolo_amd", "csrc", "cy_measure_jobs.h")).read()
    for text in ("ATR_STEP_MAX = 64;", "ATR_COLS = %d;" % AC.COLS, "ATR_CHUNK = %d;" % AC.CHUNK, "ATR_GRID_MAX = 1 << 13;"):
        assert text in jobs
    assert AC.GRID_MAX == 1 << 13
    import __graft_entry__ as ge
    assert "cy_atrous.hip" in ge.HIP_SOURCES


# ---- Chain.run on the replay detector
class ScaleReplay(PeakReplay):
    """PeakReplay plus atrous_step: from its first call on, measure_background and expand_background answer with hand-made meshes
    (the recorded ones belong to the image), and find_peaks with two rows per plane; every argument kept."""

    def __init__(self, scenario):
        PeakReplay.__init__(self, scenario)
        self.atrous_args, self.mesh_args, self.expand_args, self.planes = [], [], [], []

    def atrous_step(self, in_dev, step, want=("smooth", "detail"), out=(None, None)):
        self.calls.append("atrous_step")
        self.atrous_args.append(dict(in_dev=in_dev, step=step, want=tuple(want), out=tuple(out)))
        smooth = out[0] if out[0] is not None else np.zeros(SHAPE, np.float32)
        detail = out[1] if out[1] is not None else np.zeros(SHAPE, np.float32)
        self.planes.append((smooth, detail))
        return smooth, detail

    def measure_background(self, img, cell=128, k=3.0, niter=3):
        if not self.atrous_args:
            return PeakReplay.measure_background(self, img, cell, k, niter)
        self.calls.append("measure_background")
        self.mesh_args.append(dict(img=img, cell=cell, k=k, niter=niter))
        raw = np.zeros((-(-SHAPE[0] // cell), -(-SHAPE[1] // cell), L.CY_BKG_FIELDS), np.float64)
        raw[:, :, measure.BKG.n], raw[:, :, measure.BKG.rms] = 1e6, float(cell)
        return raw

    def expand_background(self, mesh, cell, shape, want=("bkg", "rms")):
        if not self.atrous_args:
            return PeakReplay.expand_background(self, mesh, cell, shape, want)
        self.calls.append("expand_background")
        self.expand_args.append(dict(mesh=mesh, cell=cell, shape=tuple(shape), want=tuple(want)))
        self.rms = np.zeros(shape, np.float32)
        return None, self.rms

    def find_peaks(self, map_dev, rms_dev, k_sigma=5.0, radius=2, sign=1, cap=65536):
        assert rms_dev is self.rms
        return PeakReplay.find_peaks(self, map_dev, rms_dev, k_sigma, radius, sign, cap)


def test_chain_without_the_switch_is_what_it_was():
    base_calls = None
    for extra in ({}, {"residual_scales": 0, "save_scale_maps": True}):
        s, kw = _setup("B")
        config = dict(s["config"], **extra)
        det, stats = Replay("B"), {}                          # has no atrous_step and no find_peaks: a call would raise
        chain = measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], config, **kw).run(measure.plan(config), stats)
        assert measure.plan(config) == measure.plan(s["config"])
        base_calls = base_calls or list(det.calls)
        assert det.calls == base_calls and det.calls[-1] == "measure_residuals" and "atrous_step" not in det.calls
        assert set(stats) == _stat_keys(measure.plan(config), json.loads(str(Z["B/stats"]))) and not set(stats) & SCALE_STATS
        assert chain.scale_list is None and chain.scale_planes is None and measure.peak_lists(chain) == {}
        assert not [k for o in s["sources"] for k in o if k in measure.SOURCE_SCALE_KEYS]
        assert [{k: v for k, v in o.items()} for o in json.loads(json.dumps(s["sources"]))] == json.loads(str(Z["B/catalog"]))


@pytest.mark.parametrize("save", [False, True])
@pytest.mark.parametrize("peaks", [False, True])
def test_chain_with_the_switch(peaks, save):
    s, kw = _setup("B")
    J, first = 5, 2
    config = dict(s["config"], residual_scales=J, residual_scale_first=first, residual_scales_sigma=4.0, residual_peaks=peaks, residual_peaks_radius=3,
                  residual_peaks_max=10, save_scale_maps=save)
    plain_steps = measure.plan(s["config"])
    assert measure.plan(config) == plain_steps                # the same steps: the search is no step
    det, src, stats = ScaleReplay("B"), s["sources"], {}
    chain = measure.Chain(det, np.zeros(SHAPE, np.float32), src, config, **kw).run(plain_steps, stats)
    # the order: the recorded chain, then the pixel search when asked for, then per scale the level and, from `first` on, its search
    tail = det.calls[det.calls.index("measure_residuals") + 1:]
    per_scale = lambda j: ["atrous_step"] + (["measure_background", "expand_background", "find_peaks"] if j >= first else [])
    assert tail == (["expand_background", "find_peaks"] if peaks else []) + [c for j in range(1, J + 1) for c in per_scale(j)]
    # the levels: c_0 is the residual map, every level reads the smooth plane of the one before, two smooth maps in turn
    a = det.atrous_args
    assert [x["step"] for x in a] == [1, 2, 4, 8, 16] and all(x["want"] == ("smooth", "detail") for x in a)
    assert a[0]["in_dev"] is chain.resid and all(a[j]["in_dev"] is det.planes[j - 1][0] for j in range(1, J))
    assert a[0]["out"][0] is None and a[1]["out"][0] is None and all(a[j]["out"][0] is det.planes[j - 2][0] for j in range(2, J))
    assert len({id(p[0]) for p in det.planes}) == 2 and all(a[j]["in_dev"] is not a[j]["out"][0] for j in range(J))
    if save:                                                  # every plane a map of its own, kept for save_maps()
        assert all(x["out"][1] is None for x in a) and len({id(p[1]) for p in det.planes}) == J
        assert sorted(chain.scale_planes) == [2, 3, 4, 5] and all(chain.scale_planes[j] is det.planes[j - 1][1] for j in (2, 3, 4, 5))
    else:                                                     # one detail map, written again by every level
        assert a[0]["out"][1] is None and all(a[j]["out"][1] is det.planes[0][1] for j in range(1, J)) and chain.scale_planes == {}
    # the search of every plane: cell, clip parameters, the mesh expanded at that cell to the rms map alone, radius, threshold, cap
    bkg_cell, clip_k, clip_n, _ = measure.background_config(config)
    want_cell, want_radius = [max(bkg_cell, 16 * st) for st in (2, 4, 8, 16)], [3, 4, 8, 8]
    assert [m["cell"] for m in det.mesh_args] == want_cell and all((m["k"], m["niter"]) == (clip_k, clip_n) for m in det.mesh_args)
    assert all(m["img"] is det.planes[j][1] for j, m in zip(range(1, J), det.mesh_args))
    assert [e["cell"] for e in det.expand_args] == want_cell and all(e["want"] == ("rms",) and e["shape"] == SHAPE for e in det.expand_args)
    assert all(e["mesh"].shape[:2] == (-(-SHAPE[0] // c), -(-SHAPE[1] // c)) and (e["mesh"][:, :, 1] == c).all() for e, c in zip(det.expand_args, want_cell))
    sp = det.peak_args[1 if peaks else 0:]
    assert [(p["k_sigma"], p["radius"], p["sign"], p["cap"]) for p in sp] == [(4.0, r, 1, 10) for r in want_radius]
    assert all(p["map_dev"] is det.planes[j][1] for j, p in zip(range(1, J), sp))
    if peaks:
        assert (det.peak_args[0]["k_sigma"], det.peak_args[0]["radius"], det.peak_args[0]["map_dev"]) == (5.0, 3, chain.resid)
    assert [(lv["scale"], lv["step"], lv["searched"], lv.get("cell"), lv.get("radius")) for lv in chain.scale_levels] == [
        (1, 1, False, None, None)] + [(j, 1 << (j - 1), True, c, r) for j, c, r in zip((2, 3, 4, 5), want_cell, want_radius)]
    # the catalog is the recorded one plus the two keys (and those of the pixel search)
    want = json.loads(str(Z["B/catalog"]))
    extra = measure.SOURCE_SCALE_KEYS + (measure.SOURCE_PEAK_KEYS if peaks else ())
    assert all(set(o) == set(w) | set(extra) for o, w in zip(src, want))
    assert [{k: v for k, v in o.items() if k not in extra} for o in json.loads(json.dumps(src))] == want
    # two rows per plane, moved to catalog coordinates; min_above 3 drops the second; the four that stay lie on one pixel
    bx, by = kw["box_origin"]
    assert [(d["scale"], d["step"], d["x_peak"], d["y_peak"], d["strongest"]) for d in chain.scale_list] == [
        (j, 1 << (j - 1), 3 + bx, 4 + by, j == 2) for j in (2, 3, 4, 5)]
    assert chain.scale_list[0]["x"] == 3 + bx + 0.5 and all(r.shape == (2, L.CY_PEAK_FIELDS) and r[0, 0] == 3.0 for r in chain.scale_rows.values())
    new = SCALE_STATS | ({"peaks_" + k for k in ("ms", "kernel_ms", "found", "kept", "truncated")} if peaks else set())
    assert set(stats) == _stat_keys(plain_steps, json.loads(str(Z["B/stats"]))) | new
    assert (stats["scales_found"], stats["scales_kept"], stats["scales_strongest"], stats["scales_truncated"]) == (28, 4, 1, 4)
    assert (stats["atrous_kernel_ms"], stats["scales_background_kernel_ms"], stats["scales_peaks_kernel_ms"]) == (5 * KERNEL_MS, 4 * KERNEL_MS, 4 * KERNEL_MS)
    lists = measure.peak_lists(chain)
    assert set(lists) == ({"residual_peaks", "residual_scale_peaks"} if peaks else {"residual_scale_peaks"})
    assert lists["residual_scale_peaks"] is chain.scale_list and chain.hole_list is None


def test_chain_does_not_search_without_the_residual_step():
    s, kw = _setup("B")
    config = dict(s["config"], residual_scales=4)
    det, stats = ScaleReplay("B"), {}
    steps = tuple(k for k in measure.plan(config) if k not in ("blend", "residual"))
    chain = measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], config, **kw).run(steps, stats)
    assert "atrous_step" not in det.calls and not set(stats) & SCALE_STATS and chain.scale_list is None


def test_save_maps_writes_the_searched_planes(tmp_path, monkeypatch):
    written = {}
    from caesar_yolo_amd import utils
    monkeypatch.setattr(utils, "write_fits_image", lambda path, a: written.__setitem__(os.path.basename(path), a))

    class Dev(object):                                        # what _save_maps asks of a device map
        def __init__(self, a):
            self.a = a

        def cpu(self):
            return self

        def numpy(self):
            return self.a
    chain = measure.Chain(None, np.zeros((4, 4), np.float32), [], {"residual_scales": 3, "save_scale_maps": True})
    chain.scale_planes = {3: Dev(np.full((4, 4), 3.0)), 2: Dev(np.full((4, 4), 2.0))}
    chain.save_maps(str(tmp_path / "catalog_x.json"))
    assert sorted(written) == ["wav2_catalog_x.fits", "wav3_catalog_x.fits"] and written["wav3_catalog_x.fits"][0, 0] == 3.0
    written.clear()
    chain = measure.Chain(None, np.zeros((4, 4), np.float32), [], {"residual_scales": 3})
    chain.scale_planes = {}
    chain.save_maps(str(tmp_path / "catalog_x.json"))
    assert written == {}


# ---- the chain scene on the references
def test_chain_scene_on_the_references():
    """The scene of the chain-level GPU test (tests/test_gpu_atrous.py) with the numpy references in place of the detector: the
    references alone satisfy both of its statements at this seed."""
    img, sources = ACR.scene()
    assert img.dtype == np.float32 and img.shape == (256, 256)
    chain, stats = ACR.run(ACR.RefDetector(), img, sources)
    ACR.check(chain.peak_list, chain.scale_list)
    # no pixel of the residual reaches 5 rms anywhere near the blobs; the pixel search finds nothing at all at this seed
    assert stats["peaks_found"] == 0 and chain.peak_list == []
    top = [p for p in chain.scale_list if p["strongest"]]
    assert [(p["scale"], p["x_peak"], p["y_peak"]) for p in top] == [(5, 90, 99), (5, 181, 170)] and [round(p["snr"], 1) for p in top] == [16.9, 13.7]
    assert stats["scales_found"] >= stats["scales_kept"] == len(chain.scale_list) == 4 and stats["scales_strongest"] == 2 and stats["scales_truncated"] == 0
    assert sources[0]["ncomponents"] == 1 and sources[0]["components"][0]["fit_status"] == 0
    assert sources[0]["res_nscale_peaks"] == 0 and sources[0]["res_scale_peak_snr"] is None
    assert sorted(chain.scale_planes) == [2, 3, 4, 5] and set(measure.peak_lists(chain)) == {"residual_peaks", "residual_scale_peaks"}
    # scale_peaks() alone on a preset map, as the GPU test runs it: the same planes as the plain decomposition
    alone = measure.Chain(ACR.RefDetector(), img, [], ACR.CONFIG)
    alone.resid = img
    alone.scale_peaks()
    for j, (c, w) in enumerate(AR.planes(img, 5), 1):
        assert j == 1 or np.array_equal(bits(alone.scale_planes[j]), bits(w))
    assert len(alone.scale_list) >= 4
