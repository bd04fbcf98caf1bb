"""measure.Chain and measure.plan on the CPU, against tests/golden/measure_chain.npz.

The fixture was recorded before the seven *_and_annotate wrappers were folded into Chain, by driving them in the order of
Analyzer._finish (stats as SFinder._measure wrote them) with a detector backed by the numpy references of this folder (measure_ref,
bkg_ref, island_ref, deblend_ref, fit_ref, blend_ref, residual_ref; expand_background = measure.sample_mesh rounded to fp32), on one
96 x 96 synthetic image with five boxes: two overlapping boxes on one source (its peak is rendered once: a duplicate), a box on a
touching pair (a joint fit), a box without a seed and a box that leaves the image.  Scenario A: origin (0, 0), no mesh, no beam, no
WCS.  Scenario B: box_origin (37, 21), a non-zero wcs_origin, --bkg_map with 32-pixel cells, a beam and a WCS.  Per scenario it holds
what every detector call was given and what it returned (the residual map left out: no host step reads it), the final source dicts
and the count keys of the stats.

The replay detector below answers every call with the recorded output after checking that it was given exactly the recorded input,
so the driver must form the same boxes, thresholds, backgrounds, start values and masks in the pixel frame and write the same catalog
in the catalog frame: every key bit for bit, the *_err keys (through np.linalg.inv of a 6 x 6 matrix) to a relative 1e-12."""
import copy
import json
import os
import sys

import numpy as np
import pytest

from caesar_yolo_amd import lib as L
from caesar_yolo_amd import measure
from caesar_yolo_amd.wcs import WCS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "measure_chain.npz"))
SHAPE = tuple(int(v) for v in Z["shape"])
KERNEL_MS = 0.25
# what SFinder._measure wrote beside the counts, per step
TIME_KEYS = {"measure": ("measure_ms", "measure_kernel_ms"), "background": ("background_ms", "background_kernel_ms"),
             "islands": ("islands_ms", "islands_kernel_ms"), "deblend": ("deblend_ms", "deblend_kernel_ms"), "fit": ("fit_ms", "fit_kernel_ms"),
             "blend": ("blend_ms", "blend_kernel_ms"), "residual": ("residual_ms", "render_kernel_ms", "residual_kernel_ms")}
# scripts/run.py, the "implies" of its docstring
IMPLIED = {"measure_sources": ("measure",), "bkg_map": ("measure", "background"), "save_bkg_maps": ("measure", "background"),
           "measure_islands": ("measure", "islands"), "deblend_islands": ("measure", "islands", "deblend"),
           "fit_components": ("measure", "islands", "deblend", "fit"), "fit_blends": ("measure", "islands", "deblend", "fit", "blend"),
           "residual_map": ("measure", "islands", "deblend", "fit", "residual"),
           "save_residual_maps": ("measure", "islands", "deblend", "fit", "residual")}


def _stored(key):
    """An array of the fixture, or the list of masks that was stored as shapes and bytes."""
    if key + ".shapes" not in Z.files:
        return Z[key]
    shapes, flat = Z[key + ".shapes"], Z[key + ".bytes"]
    off = np.concatenate([[0], np.cumsum(shapes.prod(1))])
    return [flat[a:b].reshape(s) for a, b, s in zip(off, off[1:], shapes)]


def _same(got, want):
    if isinstance(want, list):
        return len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))
    got = np.asarray(got)
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


class Replay(object):
    """The measurement methods of HipDetector: each checks its arguments against the recorded ones and returns the recorded rows."""

    def __init__(self, scenario):
        self.scenario, self.calls = scenario, []

    def _call(self, name, nout, **args):
        self.calls.append(name)
        pre = "%s/%s/" % (self.scenario, name)
        for k, v in args.items():
            assert _same(v, _stored(pre + k)), "%s: argument %s is not the recorded one" % (name, k)
        out = tuple(_stored(pre + "out%d" % i) for i in range(nout))
        return out[0] if nout == 1 else out

    def __getattr__(self, name):
        if name.endswith("_kernel_ms"):
            return lambda: KERNEL_MS
        raise AttributeError(name)

    def measure_sources(self, img, boxes, ring=8):
        return self._call("measure_sources", 1, boxes=boxes, ring=ring)

    def measure_background(self, img, cell=128, k=3.0, niter=3):
        return self._call("measure_background", 1, cell=cell, k=k, niter=niter)

    def expand_background(self, mesh, cell, shape, want=("bkg", "rms")):
        self._call("expand_background", 0, mesh=mesh, cell=cell, shape=np.array(shape))
        return tuple(np.zeros(shape, np.float32) if n in want else None for n in ("bkg", "rms"))      # only the detector reads the maps

    def measure_islands(self, img, boxes, thr, conn=8):
        return self._call("measure_islands", 1, boxes=boxes, thr=thr, conn=conn)

    def deblend_islands(self, img, boxes, thr4, conn=8, radius=2, return_masks=False):
        return self._call("deblend_islands", 3, boxes=boxes, thr4=thr4, conn=conn, radius=radius)[:3 if return_masks else 2]

    def fit_components(self, img, boxes, bkg, ncomp, start, masks, max_iter=64):
        return self._call("fit_components", 1, boxes=boxes, bkg=bkg, ncomp=ncomp, start=start, masks=masks, max_iter=max_iter)

    def fit_blends(self, img, boxes, bkg, ncomp, start, masks, max_iter=64):
        return self._call("fit_blends", 1, boxes=boxes, bkg=bkg, ncomp=ncomp, start=start, masks=masks, max_iter=max_iter)

    def render_gaussians(self, img, comp, nsigma=5.0, bkg_dev=None):
        if not len(comp):                                     # no source: nothing recorded to compare with
            self.calls.append("render_gaussians")
            return np.zeros((0, L.CY_RND_FIELDS)), np.zeros(SHAPE, np.float32), np.zeros(SHAPE, np.float32)
        self.model = self._call("render_gaussians", 2, comp=comp, nsigma=nsigma, has_bkg=bkg_dev is not None)[1]
        return _stored("%s/render_gaussians/out0" % self.scenario), self.model, np.zeros(SHAPE, np.float32)

    def measure_residuals(self, img, model, boxes, bkg, masks):
        assert model is self.model
        return self._call("measure_residuals", 1, boxes=boxes, bkg=bkg, masks=masks)


def _setup(scenario):
    s = json.loads(str(Z[scenario + "/setup"]))
    wcs = WCS(json.loads(str(Z["wcs_header"]))) if s["wcs"] else None
    return s, dict(beam_area=s["beam"], wcs=wcs, box_origin=tuple(s["origin"]), wcs_origin=tuple(s["wcs_origin"]))


def _compare(got, want, path="catalog"):
    if isinstance(want, dict):
        assert set(got) == set(want), path
        for k in want:
            _compare(got[k], want[k], path + "." + k)
    elif isinstance(want, list):
        assert len(got) == len(want), path
        for i, (g, w) in enumerate(zip(got, want)):
            _compare(g, w, "%s[%d]" % (path, i))
    elif path.endswith("_err") and want is not None:
        assert got == pytest.approx(want, rel=1e-12, abs=0.0), path
    else:
        assert got == want and type(got) is type(want), (path, got, want)


def _stat_keys(steps, counts):
    return {k for s in steps for k in TIME_KEYS[s]} | set(counts)


@pytest.mark.parametrize("scenario", ["A", "B"])
def test_chain_reproduces_the_recorded_catalog(scenario):
    s, kw = _setup(scenario)
    det, src, stats = Replay(scenario), s["sources"], {}
    steps = measure.plan(s["config"])
    assert steps == tuple(k for k in measure.STEPS if k != "background" or scenario == "B")
    chain = measure.Chain(det, np.zeros(SHAPE, np.float32), src, s["config"], **kw).run(steps, stats)
    want = json.loads(str(Z[scenario + "/catalog"]))
    _compare(json.loads(json.dumps(src)), want)
    comps = [c for o in want for c in o["components"] or []]
    assert sum(c["blend_status"] == 0 and c["blend_size"] >= 2 for c in comps) >= 2           # the fixture is not empty
    counts = json.loads(str(Z[scenario + "/stats"]))
    assert counts["residual_duplicates"] >= 1 and counts["residual_rendered"] >= 1 and counts["blend_jobs"] >= 1
    assert set(stats) == _stat_keys(steps, counts) and {k: stats[k] for k in counts} == counts
    assert all(stats[k] == KERNEL_MS for k in stats if k.endswith("_kernel_ms")) and all(stats[k] >= 0 for k in stats if k.endswith("_ms"))
    recorded = {k.split("/")[1] for k in Z.files if k.startswith(scenario + "/") and k.count("/") == 2}
    assert sorted(det.calls) == sorted(recorded) and len(recorded) == (9 if scenario == "B" else 7)      # every recorded call, once
    assert chain.render_stats == {k[len("residual_"):]: v for k, v in counts.items() if k.startswith("residual_")}


def test_a_shorter_plan_stops_where_it_should():
    s, kw = _setup("A")
    config = {k: v for k, v in s["config"].items() if k not in ("fit_blends", "residual_map")}
    config["fit_components"] = True
    det, src, stats = Replay("A"), s["sources"], {}
    steps = measure.plan(config)
    measure.Chain(det, np.zeros(SHAPE, np.float32), src, config, **kw).run(steps, stats)
    assert steps == ("measure", "islands", "deblend", "fit")
    assert det.calls == ["measure_sources", "measure_islands", "deblend_islands", "fit_components"]
    counts = {k: v for k, v in json.loads(str(Z["A/stats"])).items() if k.startswith("fit_")}
    assert set(stats) == _stat_keys(steps, counts) and {k: stats[k] for k in counts} == counts
    want = json.loads(str(Z["A/catalog"]))
    for o in want:
        for k in measure.RESIDUAL_KEYS:
            del o[k]
        for c in o["components"] or []:
            for k in measure.BLEND_KEYS + measure.RENDER_ITEM_KEYS:
                del c[k]
    _compare(json.loads(json.dumps(src)), want)


@pytest.mark.parametrize("scenario", ["A", "B"])
def test_no_source(scenario):
    s, kw = _setup(scenario)
    det, src, stats = Replay(scenario), [], {}
    steps = measure.plan(s["config"])
    measure.Chain(det, np.zeros(SHAPE, np.float32), src, s["config"], **kw).run(steps, stats)
    assert src == []
    assert det.calls == (["measure_background", "expand_background"] if scenario == "B" else []) + ["render_gaussians"]
    counts = json.loads(str(Z[scenario + "/stats"]))
    assert set(stats) == _stat_keys(steps, counts) and all(stats[k] == 0 for k in counts)
    unguarded = ("background_kernel_ms", "render_kernel_ms")
    assert all(stats[k] == (KERNEL_MS if k in unguarded else 0.0) for k in stats if k.endswith("_kernel_ms"))


def test_plan_truth_table():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import run
    assert measure.plan({}) == () and measure.plan(run.measure_config(run.parse_args(["--weights=seeded:l:5"]))) == ()
    for flag, steps in IMPLIED.items():
        config = run.measure_config(run.parse_args(["--weights=seeded:l:5", "--" + flag]))
        assert config[flag] is True
        assert measure.plan(config) == steps, flag
        assert measure.plan({flag: True}) == steps, flag      # a hand-made config: the rule does not lean on run.py's implied flags
        assert copy.deepcopy(config) == run.measure_config(run.parse_args(["--weights=seeded:l:5"] + ["--" + f for f in config if config[f] is True]))
