"""The residual-peak search without a GPU: the numpy reference (tests/peaks_ref.py) against an independent pixel-by-pixel loop on the
small cases of tests/peaks_cases.py, annotate_peaks on hand-made rows, plan() and the command line for the new switches, the
library's exports, and measure.Chain.run on the replay detector of tests/test_measure_chain_cpu.py with and without the switch."""
import json
import os
import sys

import numpy as np
import pytest

import peaks_cases as PC
import peaks_chain_ref as CR
import peaks_ref as PR
from caesar_yolo_amd import lib as L
from caesar_yolo_amd import measure
from test_measure_chain_cpu import IMPLIED, KERNEL_MS, SHAPE, Replay, _setup, _stat_keys, Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_STEPS = ("measure", "background", "islands", "deblend", "fit", "residual")


# ---- the reference
@pytest.mark.parametrize("name", PC.BRUTE_FORCE)
def test_reference_equals_the_pixel_loop(name):
    c = PC.case(name)
    rows, absum = PC.reference()[name]
    want = PR.brute_force(c.map, c.rms, c.k_sigma, c.radius, c.sign)
    assert rows.shape == want.shape
    exact = [0, 1, 2, 3, 4, 5, 6, 11]
    assert np.array_equal(rows[:, exact], want[:, exact])
    assert (np.abs(rows[:, PR.SUMS] - want[:, PR.SUMS]) <= PR.sum_bound(want, absum)).all()


def test_the_cases_hold_what_they_are_for():
    ref = {k: v[0] for k, v in PC.reference().items()}
    xy = lambda name: {(int(r[0]), int(r[1])) for r in ref[name]}
    assert len(ref["lattice"]) == 2304 and len(ref["none"]) == 0 and len(ref["1x1"]) == 1 and len(ref["1x1_below"]) == 0
    assert ref["1x1"][0].tolist() == [0, 0, 7, 1, 7, 1, 1, 7, 7, 0, 0, 0]
    # one peak per plateau, its first pixel; equal maxima 3 apart both, 2 apart the first only
    assert xy("ties") == {(4, 3), (5, 12), (8, 12), (5, 18), (20, 22), (20, 25), (20, 30)}
    # the threshold, the rms under a spike, a neighbour without noise, invalid neighbours
    assert xy("validity") == {(5, 5), (25, 5), (25, 25), (5, 35), (15, 35), (25, 35), (35, 35)}
    rows = {(int(r[0]), int(r[1])): r for r in ref["validity"]}
    assert rows[(25, 25)][5] == 25 and rows[(25, 25)][6] == 1           # the neighbour of 8 with rms 0 is valid but not above
    assert rows[(5, 35)][5] == 23 and rows[(35, 35)][5] == 23           # two invalid neighbours each
    # corners and edges: clipped neighbourhoods
    e = {(int(r[0]), int(r[1])): int(r[5]) for r in ref["edges_r2"]}
    assert e == {(0, 0): 9, (20, 0): 15, (40, 0): 9, (0, 15): 15, (20, 15): 25, (40, 15): 15, (0, 29): 9, (20, 29): 15, (40, 29): 9}
    assert {int(r[5]) for r in ref["edges_r8"]} == {81, 9 * 17, 17 * 17}
    for nseg, name in ((1, "one_segment_and_1"), (2, "two_segments_and_1")):
        for b in range(1, nseg + 1):
            assert {(b * PC.SEG - 1, 0), (b * PC.SEG, 4), (b * PC.SEG - 1, 8)} <= xy(name) and (b * PC.SEG, 8) not in xy(name)
    # more segments than the grid has workgroups, peaks in both iterations of the same workgroups
    for name in ("tall_8", "tall_5"):
        assert PC.case(name).map.shape[0] > PC.GRID_MAX and PC.case(name).map.shape[1] <= PC.SEG
        assert {(1, 3), (1, 50), (1, PC.GRID_MAX + 3), (1, PC.GRID_MAX + 50)} <= xy(name) and len(ref[name]) > 40
    # holes: the peaks of the negated map, v negated
    c = PC.case("70x75_holes")
    neg, _ = PR.find_peaks(-c.map, c.rms, c.k_sigma, c.radius, 1)
    neg[:, 2] = -neg[:, 2]
    assert len(neg) > 10 and np.array_equal(neg, ref["70x75_holes"])


# ---- annotate_peaks
def _row(x, y, v, rms, nabove, total, sw, swx, swy, npix=25):
    return [x, y, v, rms, abs(v) / rms, npix, nabove, total, sw, swx, swy, 0.0]


class FakeWCS(object):
    def wcs_pix2world(self, x, y, origin):
        assert origin == 0
        return 100.0 + x / 10.0, -40.0 + y / 10.0


def _sources():
    # boxes 0 and 1 overlap in [20, 30] x [20, 30]
    return [{"x1": 10.0, "y1": 10.0, "x2": 30.0, "y2": 30.0}, {"x1": 20.0, "y1": 20.0, "x2": 40.0, "y2": 40.0}, {"x1": 100.0, "y1": 100.0, "x2": 110.0, "y2": 110.0}]


def test_annotate_peaks_on_hand_made_rows():
    rows = np.array([
        _row(25, 25, 12.0, 2.0, 5, 40.0, 36.0, 9.0, -18.0),       # snr 6, in boxes 0 and 1
        _row(12, 30, 16.0, 2.0, 3, 50.0, 50.0, 0.0, 25.0),        # snr 8, on the edge of box 0
        _row(60, 60, 6.0, 1.0, 9, 20.0, 20.0, 5.0, 5.0),          # snr 6 again: stays behind the first
        _row(105, 105, 30.0, 1.0, 2, 90.0, 90.0, 0.0, 0.0),       # nabove below min_above: dropped
        _row(41, 40, 7.0, 1.0, 4, 21.0, 21.0, 0.0, 0.0),          # snr 7, one pixel outside box 1
    ], np.float64)
    src = _sources()
    out = measure.annotate_peaks(src, rows, 9, 3, 4.0, FakeWCS(), origin=(1000, 2000))
    assert [tuple(d) for d in out] == [measure.PEAK_KEYS] * 4
    assert [(d["x_peak"], d["y_peak"]) for d in out] == [(12, 30), (41, 40), (25, 25), (60, 60)]
    assert [d["snr"] for d in out] == [8.0, 7.0, 6.0, 6.0] and [d["in_source"] for d in out] == [0, None, 0, None]
    d = out[2]
    assert (d["x"], d["y"]) == (25.25, 24.5) and (d["ra"], d["dec"]) == (100.0 + 1025.25 / 10.0, -40.0 + 2024.5 / 10.0)
    assert (d["peak"], d["rms"], d["npix"], d["nabove"], d["flux_sum"], d["flux"]) == (12.0, 2.0, 25, 5, 40.0, 10.0)
    assert type(d["x_peak"]) is int and type(d["npix"]) is int and type(d["nabove"]) is int
    assert [(s["res_npeaks"], s["res_peak_snr"]) for s in src] == [(2, 8.0), (1, 6.0), (0, None)]
    assert not [k for s in src for k in s if "hole" in k]
    json.dumps(out)
    # no beam, no WCS; min_above 1 keeps the fourth row, which then leads
    src = _sources()
    out = measure.annotate_peaks(src, rows, 5, 1, 0, None)
    assert out[0]["x_peak"] == 105 and out[0]["in_source"] == 2 and src[2]["res_npeaks"] == 1 and src[2]["res_peak_snr"] == 30.0
    assert all(d["flux"] is None and d["ra"] is None and d["dec"] is None for d in out) and len(out) == 5
    # holes: the row's sums are of the negated map; v stays signed
    hole = np.array([_row(25, 25, -12.0, 2.0, 5, 40.0, 36.0, 9.0, -18.0)], np.float64)
    src = _sources()
    out = measure.annotate_peaks(src, hole, 1, 3, 4.0, None, holes=True)
    assert (out[0]["peak"], out[0]["snr"], out[0]["flux_sum"], out[0]["flux"], out[0]["x"]) == (-12.0, 6.0, -40.0, -10.0, 25.25)
    assert [(s["res_nholes"], s["res_hole_snr"]) for s in src] == [(1, 6.0), (1, 6.0), (0, None)] and "res_npeaks" not in src[0]
    # nothing found, and no source
    assert measure.annotate_peaks([], np.zeros((0, L.CY_PEAK_FIELDS)), 0, 3, 4.0, None) == []
    assert len(measure.annotate_peaks([], rows, 5, 3, 4.0, None)) == 4


# ---- plan() and the command line
def test_plan_and_steps():
    assert measure.STEPS == ("measure", "background", "islands", "deblend", "fit", "blend", "residual")
    for flag, steps in IMPLIED.items():
        assert measure.plan({flag: True}) == steps and not measure.wants_peaks({flag: True}), flag
    for flag in ("residual_peaks", "residual_holes"):
        assert measure.plan({flag: True}) == PEAK_STEPS and measure.wants_peaks({flag: True})
        assert measure.plan({flag: True, "fit_blends": True}) == measure.STEPS
    assert not measure.wants_peaks({}) and not measure.wants_peaks({"residual_peaks": False})
    assert set(measure.plan({"residual_peaks": True})) <= set(measure.STEPS)


def test_flags_parse_and_imply():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import run
    base = run.measure_config(run.parse_args(["--weights=seeded:l:5"]))
    assert (base["residual_peaks"], base["residual_holes"]) == (False, False) and measure.plan(base) == ()
    assert measure.peaks_config(base) == measure.peaks_config({}) == (5.0, 2, 3, 65536)
    for flag in ("residual_peaks", "residual_holes"):
        args = run.parse_args(["--weights=seeded:l:5", "--" + flag])
        config = run.measure_config(args)
        assert config[flag] is True and measure.plan(config) == PEAK_STEPS and measure.wants_peaks(config)
        assert args.residual_map and args.bkg_map and args.fit_components and not args.fit_blends
    args = run.parse_args(["--weights=seeded:l:5", "--residual_peaks", "--residual_peaks_sigma=4.5", "--residual_peaks_radius=3",
                           "--residual_peaks_min_above=1", "--residual_peaks_max=100"])
    assert measure.peaks_config(run.measure_config(args)) == (4.5, 3, 1, 100)
    with pytest.raises(SystemExit):
        run.parse_args(["--weights=seeded:l:5", "--residual_peaks_radius=9"])
    for flag in ("residual_peaks", "residual_peaks_sigma", "residual_peaks_radius", "residual_peaks_min_above", "residual_peaks_max", "residual_holes"):
        assert "--" + flag in run.__doc__, flag


def test_exports():
    assert {"cy_find_peaks", "cy_peaks_kernel_ms"} <= set(L.EXPORTS)
    assert L.CY_PEAK_FIELDS == len(L.PEAK_NAMES) == PR.FIELDS == 12 and (L.CY_PEAK_RADIUS_MAX, L.CY_PEAK_CAP_MAX) == (8, 1 << 20)
    assert L.PEAK_NAMES == ("x", "y", "v", "rms", "snr", "npix", "nabove", "sum", "sw", "swx", "swy", "reserved")
    lib = L.load()
    assert hasattr(lib, "cy_find_peaks") and hasattr(lib, "cy_peaks_kernel_ms")
    hdr = open(os.path.join(ROOT, "include", "caesar_yolo_hip.h")).read()
    for text in ("#define CY_PEAK_FIELDS 12", "#define CY_PEAK_RADIUS_MAX 8", "#define CY_PEAK_CAP_MAX (1 << 20)"):
        assert text in hdr


# ---- Chain.run on the replay detector
class PeakReplay(Replay):
    """Replay plus find_peaks: two hand-made rows per search, the arguments kept."""

    def __init__(self, scenario):
        Replay.__init__(self, scenario)
        self.wants, self.peak_args = [], []

    def expand_background(self, mesh, cell, shape, want=("bkg", "rms")):
        self.wants.append((len(self.calls), tuple(want)))
        out = Replay.expand_background(self, mesh, cell, shape, want)
        self.rms = out[1]
        return out

    def find_peaks(self, map_dev, rms_dev, k_sigma=5.0, radius=2, sign=1, cap=65536):
        self.calls.append("find_peaks")
        self.peak_args.append(dict(map_dev=map_dev, rms_dev=rms_dev, k_sigma=k_sigma, radius=radius, sign=sign, cap=cap))
        rows = np.array([_row(3, 4, sign * 9.0, 1.0, 4, 30.0, 30.0, 15.0, 0.0), _row(50, 60, sign * 20.0, 2.0, 1, 60.0, 60.0, 0.0, 0.0)], np.float64)
        return rows, 7


def test_chain_without_the_switch_is_what_it_was():
    s, kw = _setup("B")
    det, stats = Replay("B"), {}                              # has no find_peaks: a call would raise
    chain = measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], s["config"], **kw).run(measure.plan(s["config"]), stats)
    assert "find_peaks" not in det.calls and det.calls.count("expand_background") == 1
    assert not [k for k in stats if k.startswith("peaks_") or k.startswith("holes_")]
    assert chain.peak_list is None and chain.hole_list is None and measure.peak_lists(chain) == {} and measure.peak_lists(None) == {}
    assert not [k for o in s["sources"] for k in o if k in measure.SOURCE_PEAK_KEYS + measure.SOURCE_HOLE_KEYS]


@pytest.mark.parametrize("holes", [False, True])
def test_chain_with_the_switch(holes):
    s, kw = _setup("B")
    config = dict(s["config"], residual_peaks=True, residual_peaks_sigma=4.0, residual_peaks_radius=3, residual_peaks_max=10, residual_holes=holes)
    plain_steps = measure.plan(s["config"])
    assert measure.plan(config) == plain_steps                # the same steps: the search is no step
    det, src, stats = PeakReplay("B"), s["sources"], {}
    chain = measure.Chain(det, np.zeros(SHAPE, np.float32), src, config, **kw).run(plain_steps, stats)
    n = 2 if holes else 1
    assert det.calls.count("find_peaks") == n and det.calls.count("expand_background") == 2
    after = det.calls.index("measure_residuals")
    assert [w for _, w in det.wants] == [("bkg",), ("rms",)] and det.wants[1][0] > after and det.calls.index("find_peaks") > after
    for a, sign in zip(det.peak_args, (1, -1)):
        assert a["map_dev"] is chain.resid and a["rms_dev"] is det.rms and (a["k_sigma"], a["radius"], a["sign"], a["cap"]) == (4.0, 3, sign, 10)
    # the catalog is the recorded one plus the two keys per search
    want = json.loads(str(Z["B/catalog"]))
    extra = measure.SOURCE_PEAK_KEYS + (measure.SOURCE_HOLE_KEYS if holes else ())
    assert all(set(o) == set(w) | set(extra) for o, w in zip(src, want))
    assert [{k: v for k, v in o.items() if k not in extra} for o in json.loads(json.dumps(src))] == want
    # rows move from the pixels of the image to catalog coordinates (box_origin); min_above 3 drops the second row
    bx, by = kw["box_origin"]
    assert len(chain.peak_list) == 1 and (chain.peak_list[0]["x_peak"], chain.peak_list[0]["y_peak"]) == (3 + bx, 4 + by)
    assert chain.peak_list[0]["x"] == 3 + bx + 0.5 and chain.peak_list[0]["peak"] == 9.0
    counts = json.loads(str(Z["B/stats"]))
    new = {p + k for p in (("peaks_", "holes_") if holes else ("peaks_",)) for k in ("ms", "kernel_ms", "found", "kept", "truncated")}
    assert set(stats) == _stat_keys(plain_steps, counts) | new
    assert (stats["peaks_found"], stats["peaks_kept"], stats["peaks_truncated"], stats["peaks_kernel_ms"]) == (7, 1, 1, KERNEL_MS)
    lists = measure.peak_lists(chain)
    assert set(lists) == ({"residual_peaks", "residual_holes"} if holes else {"residual_peaks"})
    if holes:
        assert chain.hole_list[0]["peak"] == -9.0 and chain.hole_list[0]["flux_sum"] == -30.0 and stats["holes_found"] == 7
    else:
        assert chain.hole_list is None


def test_chain_does_not_search_without_the_residual_step():
    s, kw = _setup("B")
    config = dict(s["config"], residual_peaks=True)
    det, stats = PeakReplay("B"), {}
    steps = tuple(k for k in measure.plan(config) if k not in ("blend", "residual"))
    measure.Chain(det, np.zeros(SHAPE, np.float32), s["sources"], config, **kw).run(steps, stats)
    assert "find_peaks" not in det.calls and "peaks_ms" not in stats


def test_chain_scene_on_the_references():
    """The scene of the chain-level GPU test (tests/test_gpu_peaks.py) with the numpy references in place of the detector: the
    references alone satisfy both of its statements at this seed."""
    img, sources = CR.scene()
    stats = {}
    chain = measure.Chain(CR.RefDetector(), img, sources, CR.CONFIG).run(measure.plan(CR.CONFIG), stats)
    CR.check(chain.peak_list, sources)
    assert stats["peaks_found"] >= stats["peaks_kept"] == len(chain.peak_list) >= 1 and chain.hole_list is None
    assert sources[0]["ncomponents"] == 1 and sources[0]["components"][0]["fit_status"] == 0
