"""cy_disc_residuals on the GPU against its numpy float64 restatement (tests/disc_residual_ref.py) on the inputs of
tests/disc_residual_cases.py, and the chain step --subtract_peaks on the real detector.

Status, npix, nexcluded, maxabs (one rounded subtraction) with its position, the reserved field, the window, clipped and nneigh are
exact integer or single IEEE operations on both sides: equal.  The three sums add the same float64 terms in another order, so
|gpu - ref| <= 2 npix 2^-53 sum|t_i| with sum|t_i| from the reference (disc_residual_ref.compare, the derived bound of
residual_ref.compare_stats).  No tolerance here is measured or chosen.

The chain-level test runs measure.Chain on the real detector over the scene of tests/test_disc_residual_cpu.py (the scene of
tests/peaks_chain_ref.py plus a planted pair 5 px apart); the same chain runs there on the numpy references, where the three
neighbourhood statements hold before the GPU is asked."""
import ctypes as C

import numpy as np
import pytest
import torch

import disc_residual_cases as DC
import disc_residual_ref as DR
import peaks_ref
import residual_ref as RR
from caesar_yolo_amd import lib as L
from caesar_yolo_amd import measure
from gpu_common import detector
from test_disc_residual_cpu import SUBTRACT_STATS, check_hole, check_pair, hole_scene, pair_config, pair_scene
from test_gpu_peaks import check_rows, upload

pytestmark = pytest.mark.gpu
GUARD = 8


@pytest.fixture(scope="module")
def det():
    return detector("fp32", max_batch=1, max_imgsz=160)


def raw_call(det, map_dev, model_dev, jobs, MH, MW):
    """The C entry with guard floats around h_out.  -> (rc, rows, whether the guards are untouched)."""
    jobs = np.ascontiguousarray(jobs, np.float64).reshape(-1, L.CY_PFIT_JOB_FIELDS)
    n = jobs.shape[0]
    buf = np.full(GUARD + n * L.CY_DRES_FIELDS + GUARD, -7.5, np.float64)
    out = buf[GUARD:GUARD + n * L.CY_DRES_FIELDS]
    dp = C.POINTER(C.c_double)
    rc = det.lib.cy_disc_residuals(det.ctx, det._p(map_dev), det._p(model_dev) if model_dev is not None else None, MH, MW,
                                   jobs.ctypes.data_as(dp) if n else None, n, out.ctypes.data_as(dp) if n else None, det._stream())
    torch.cuda.synchronize()
    return rc, out.reshape(n, L.CY_DRES_FIELDS).copy(), bool((buf[:GUARD] == -7.5).all() and (buf[GUARD + n * L.CY_DRES_FIELDS:] == -7.5).all())


@pytest.mark.parametrize("g", DC.groups(), ids=lambda g: g.name)
def test_case(det, g):
    ref, ab = DR.disc_residuals(g.map, g.model, g.jobs)
    MH, MW = g.map.shape
    dev = upload(det, g.map, g.offset)
    mdev = None if g.model is None else upload(det, g.model, g.offset)
    rc, got, guards = raw_call(det, dev, mdev, g.jobs, MH, MW)
    assert rc == 0 and guards, g.name
    DR.compare(got, ref, ab, ["%s / %s" % (g.name, nm) for nm in g.names])
    # the wrapper gives the same bytes; the maps are only read (NaN and inf compare by their bytes); a repeat call: byte-equal
    again = det.disc_residuals(dev, mdev, g.jobs)
    assert again.shape == got.shape and again.tobytes() == got.tobytes(), "%s: a second call gave other bytes" % g.name
    assert dev.cpu().numpy().tobytes() == g.map.tobytes() and (mdev is None or mdev.cpu().numpy().tobytes() == g.model.tobytes())
    if len(g.names) and (ref[:, 0] == 0).any():
        assert det.disc_residual_kernel_ms() > 0.0
    turned = ref[:, 0] != 0
    assert np.array_equal(got[turned], ref[turned])           # statuses 1 and 5: the whole row


def test_model_null_changes_the_model_sum_alone(det):
    a, b = DC.by_name("main_64x96"), DC.by_name("main_no_model")
    dev, mdev = upload(det, a.map), upload(det, a.model)
    with_model, without = det.disc_residuals(dev, mdev, a.jobs), det.disc_residuals(dev, None, b.jobs)
    keep = [f for f in range(L.CY_DRES_FIELDS) if f != 8]
    assert with_model[:, keep].tobytes() == without[:, keep].tobytes() and not without[:, 8].any() and with_model[:, 8].any()


def test_unaligned_pointers_give_the_same_rows(det):
    a, b = DC.by_name("main_64x96"), DC.by_name("main_offset")
    r0 = det.disc_residuals(upload(det, a.map), upload(det, a.model), a.jobs)
    r1 = det.disc_residuals(upload(det, b.map, True), upload(det, b.model, True), b.jobs)
    assert r0.tobytes() == r1.tobytes()


def test_argument_errors_leave_the_rows_untouched(det):
    g = DC.by_name("main_64x96")
    dev, mdev = upload(det, g.map), upload(det, g.model)
    MH, MW = g.map.shape
    n = g.jobs.shape[0]
    jobs = np.ascontiguousarray(g.jobs)
    out = np.full((n, L.CY_DRES_FIELDS), -7.5, np.float64)
    dp = C.POINTER(C.c_double)
    good = dict(ctx=det.ctx, m=det._p(dev), md=det._p(mdev), MH=MH, MW=MW, j=jobs.ctypes.data_as(dp), n=n, o=out.ctypes.data_as(dp))

    def call(**kw):
        a = dict(good, **kw)
        return det.lib.cy_disc_residuals(a["ctx"], a["m"], a["md"], a["MH"], a["MW"], a["j"], a["n"], a["o"], det._stream())
    bad = [dict(ctx=None), dict(m=None), dict(j=None), dict(o=None), dict(MH=0), dict(MW=0), dict(MH=-3), dict(MW=-1), dict(MH=1 << 16, MW=1 << 15),
           dict(MH=(1 << 31) - 1, MW=(1 << 31) - 1), dict(n=-1), dict(n=L.CY_PFIT_JOBS_MAX + 1)]
    for kw in bad:
        assert call(**kw) == -1, kw                          # CY_ERR_ARG
        torch.cuda.synchronize()
        assert (out == -7.5).all(), kw
    for kw, text in ((dict(m=None), b"null argument"), (dict(j=None), b"null argument"), (dict(o=None), b"null argument"), (dict(MH=0), b"MH, MW > 0"),
                     (dict(MH=1 << 16, MW=1 << 15), b"2^31"), (dict(n=-1), b"n outside"),
                     # the order of the checks: shape, size, n, pointers
                     (dict(MH=0, MW=1 << 30, n=-1, m=None), b"MH, MW > 0"), (dict(MH=1 << 16, MW=1 << 15, n=-1, m=None), b"2^31"), (dict(n=-1, m=None), b"n outside")):
        assert call(**kw) == -1
        assert text in det.lib.cy_last_error(det.ctx), (kw, det.lib.cy_last_error(det.ctx))
    # n == 0 is no error and writes nothing, whatever the pointers; a null model is no error
    assert call(n=0) == 0 and call(n=0, m=None, j=None, o=None) == 0 and (out == -7.5).all()
    assert call(md=None) == 0 and out[:, 8].tolist() == [0.0] * n
    assert call() == 0
    assert out.tobytes() == det.disc_residuals(dev, mdev, g.jobs).tobytes()
    for badcall in (lambda: det.disc_residuals(dev.double(), mdev, g.jobs), lambda: det.disc_residuals(dev.cpu(), mdev, g.jobs),
                    lambda: det.disc_residuals(dev[:, :-1], mdev, g.jobs), lambda: det.disc_residuals(dev, mdev[:-1], g.jobs)):
        with pytest.raises(L.CyError):
            badcall()
    assert det.disc_residuals(dev, None, np.zeros((0, L.CY_PFIT_JOB_FIELDS))).shape == (0, L.CY_DRES_FIELDS)


def test_kernel_time_is_kept():
    from caesar_yolo_amd.model import HipDetector
    from gpu_common import seeded_weights
    fresh = HipDetector(seeded_weights("l", 5)[0], device=0, precision="fp32", max_batch=1, max_imgsz=160)      # a context of its own
    assert fresh.disc_residual_kernel_ms() == -1.0
    g = DC.by_name("main_64x96")
    dev = upload(fresh, g.map)
    fresh.disc_residuals(dev, None, np.zeros((0, L.CY_PFIT_JOB_FIELDS)))
    away = fresh.disc_residuals(dev, None, np.array([DC.job(5.0, 5.0, -1.0), DC.job(float("nan"), 5.0, 2.0)]))
    assert fresh.disc_residual_kernel_ms() == -1.0            # no job that is measured, no launch
    assert away[:, 0].tolist() == [1.0, 5.0] and (away[:, [6, 7, 10, 11, 12, 13]] == -1.0).all() and not away[:, [1, 2, 3, 4, 5, 8, 9, 14, 15]].any()
    fresh.disc_residuals(dev, None, g.jobs)
    ms = fresh.disc_residual_kernel_ms()
    assert ms > 0.0
    fresh.disc_residuals(dev, None, np.array([DC.job(5.0, 5.0, -1.0)]))
    assert fresh.disc_residual_kernel_ms() == ms              # a call that launches nothing keeps the value
    fresh.close()


# ---- the chain
@pytest.fixture(scope="module")
def runs(det):
    """The chain on the real detector over pair_scene(): without the switch, with it and the group fits, with it and the single fits alone."""
    out = {}
    for key, config in (("plain", dict(pair_config(True), subtract_peaks=False)), ("groups", pair_config(True)), ("single", pair_config(False))):
        img, sources = pair_scene()
        stats = {}
        chain = measure.Chain(det, upload(det, img), sources, config).run(measure.plan(config), stats)
        out[key] = (chain, stats, sources, config)
    return out


@pytest.mark.parametrize("key", ["groups", "single"])
def test_chain_second_residual_and_peak_model(det, runs, key):
    chain, stats, _, config = runs[key]
    resid = chain.resid.cpu().numpy()
    comp, index, counts = measure.peak_render_selection(chain)
    assert np.array_equal(comp, chain.subtract_comp) and index == chain.subtract_index and len(index) == 3
    # the GPU's own selected components, rendered by the reference on the GPU's first residual
    rows, model, resid2 = DR.render_signed(resid, comp, float(config["residual_nsigma"]), None)
    assert np.array_equal(chain.subtract_render_rows, rows) and (rows[:, 0] == 0).all()
    got_model, got_resid2 = chain.peak_model.cpu().numpy().astype(np.float64), chain.resid2.cpu().numpy().astype(np.float64)
    dm, dr = np.abs(got_model - model), np.abs(got_resid2 - resid2)
    print("%s: peak model off by at most %.3g of its bound, second residual by %.3g of its bound" % (
        key, float((dm / RR.model_bound(model)).max()), float((dr / RR.resid_bound(resid2, model)).max())))
    assert (dm <= RR.model_bound(model)).all() and (dr <= RR.resid_bound(resid2, model)).all()
    assert chain.resid.cpu().numpy().tobytes() == resid.tobytes()
    assert (stats["subtract_selected"], stats["subtract_rendered"], stats["subtract_wandered"], stats["subtract_duplicates"]) == (3, 3, 0, 0)
    assert stats["subtract_render_kernel_ms"] > 0.0 and stats["disc_residual_kernel_ms"] > 0.0 and stats["left_peaks_kernel_ms"] > 0.0 and stats["subtract_ms"] > 0.0


@pytest.mark.parametrize("key", ["groups", "single"])
def test_chain_disc_rows_and_left_lists(det, runs, key):
    chain, stats, sources, config = runs[key]
    resid2, model = chain.resid2.cpu().numpy(), chain.peak_model.cpu().numpy()
    rms_dev = det.expand_background(chain.mesh, chain.cell, resid2.shape, want=("rms",))[1]
    rms = rms_dev.cpu().numpy()
    lists = measure.peak_lists(chain)
    assert list(chain.disc_rows) == ["residual_peaks"] and list(lists) == ["residual_peaks", "residual_holes", "residual_peaks_left", "residual_holes_left"]
    # every row against the reference run on the GPU's second-residual bytes
    jobs = chain.peakfit_jobs["residual_peaks"]
    ref, ab = DR.disc_residuals(resid2, model, jobs)
    DR.compare(chain.disc_rows["residual_peaks"], ref, ab, ["%s / residual_peaks[%d]" % (key, i) for i in chain.peakfit_select["residual_peaks"]])
    picked = {i: (src, int(r[0])) for (nm, i), src, r in zip(chain.subtract_index, measure.peak_render_selection(chain)[2]["sources"], chain.subtract_render_rows)}
    entries = lists["residual_peaks"]
    want = measure.annotate_peak_residuals([{} for _ in entries], chain.disc_rows["residual_peaks"], chain.peakfit_rms["residual_peaks"], picked, 0, (0, 0),
                                           chain.peakfit_select["residual_peaks"])
    assert [{k: d[k] for k in measure.GRES_KEYS} for d in entries] == want
    # the left lists against the reference search of the same bytes
    for sign, name, cnt in ((1, "residual_peaks_left", "left_peaks"), (-1, "residual_holes_left", "left_holes")):
        want_rows, absum = peaks_ref.find_peaks(resid2, rms, chain.peak_sigma, chain.peak_radius, sign)
        check_rows("%s / %s" % (key, name), chain.left_rows[sign], len(want_rows), want_rows, absum)
        probe = [dict(s) for s in sources]
        want_list = measure.annotate_peaks(probe, chain.left_rows[sign], len(want_rows), chain.peak_min_above, 0, None, (0, 0), holes=sign < 0)
        assert lists[name] == want_list and stats[cnt] == len(want_list)
    assert stats["left_truncated"] == 0
    # the three neighbourhood statements of the CPU test
    check_pair(lists, key == "groups")
    print("%s: gres_ratio %s, left peaks %d, left holes %d" % (key, [round(d["gres_ratio"], 3) for d in entries], stats["left_peaks"], stats["left_holes"]))


def test_chain_without_the_new_keys_is_the_run_without_the_switch(runs):
    plain, stats0, sources0, _ = runs["plain"]
    chain, stats, sources, _ = runs["groups"]
    lists0, lists = measure.peak_lists(plain), measure.peak_lists(chain)
    assert plain.resid2 is None and list(lists0) == ["residual_peaks", "residual_holes"]
    for name, before in lists0.items():
        assert [{k: v for k, v in d.items() if k not in measure.GRES_KEYS} for d in lists[name]] == before
        assert all(tuple(d) == tuple(d0) + measure.GRES_KEYS for d, d0 in zip(lists[name], before))
    assert [{k: v for k, v in s.items() if k not in measure.SOURCE_LEFT_KEYS} for s in sources] == sources0
    timed = lambda k: k.endswith("_ms")
    assert {k: v for k, v in stats.items() if k not in SUBTRACT_STATS and not timed(k)} == {k: v for k, v in stats0.items() if not timed(k)}
    assert set(stats) == set(stats0) | SUBTRACT_STATS and not set(stats0) & SUBTRACT_STATS
    assert plain.resid.cpu().numpy().tobytes() == chain.resid.cpu().numpy().tobytes()


# ---- the signed render
def test_signed_render_against_its_reference_and_the_plain_entry_is_what_it_was(det):
    """cy_render_signed_gaussians on components of either sign against disc_residual_ref.render_signed within the bounds of
    residual_ref; cy_render_gaussians on the same components still turns the negative ones away (status 1) and renders the rest."""
    img = (np.random.default_rng(21).standard_normal((70, 75)) + 0.5).astype(np.float32)
    img[10, 12], img[40, 41] = 0.0, np.nan
    comp = np.array([[-12.0, 20.3, 30.6, 0.4, 0.05, 0.3], [9.0, 24.1, 33.5, 0.35, 0.0, 0.35], [0.0, 50.0, 50.0, 0.4, 0.0, 0.4], [-3.0, 73.5, 1.2, 0.2, 0.0, 0.25],
                     [5.0, 40.0, 41.0, 0.4, 0.0, 0.4], [-2.0, 500.0, 10.0, 0.4, 0.0, 0.4], [-1.0, 30.0, 30.0, -0.4, 0.0, 0.4], [float("nan"), 30.0, 30.0, 0.4, 0.0, 0.4]])
    dev = upload(det, img)
    rows, model, resid = DR.render_signed(img, comp, 5.0)
    assert rows[:, 0].tolist() == [0.0, 0.0, 1.0, 0.0, 0.0, 3.0, 1.0, 1.0]
    grows, gmodel, gresid = det.render_gaussians(dev, comp, 5.0, None, signed=True)
    assert np.array_equal(grows, rows) and det.render_kernel_ms() > 0.0
    gm, gr = gmodel.cpu().numpy().astype(np.float64), gresid.cpu().numpy().astype(np.float64)
    assert (np.abs(gm - model) <= RR.model_bound(model)).all() and (np.abs(gr - resid) <= RR.resid_bound(resid, model)).all()
    assert gm.min() < -10.0 and gm.max() > 4.0 and gr[10, 12] == 0.0 and gr[40, 41] == 0.0
    again = det.render_gaussians(dev, comp, 5.0, None, signed=True)
    assert again[1].cpu().numpy().tobytes() == gmodel.cpu().numpy().tobytes() and again[2].cpu().numpy().tobytes() == gresid.cpu().numpy().tobytes()
    prow, pmodel, presid = RR.render(img, comp, 5.0)
    qrows, qmodel, qresid = det.render_gaussians(dev, comp, 5.0, None)
    assert np.array_equal(qrows, prow) and prow[:, 0].tolist() == [1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0]
    assert (np.abs(qmodel.cpu().numpy() - pmodel) <= RR.model_bound(pmodel)).all() and float(qmodel.min()) == 0.0
    assert dev.cpu().numpy().tobytes() == img.tobytes()


# ---- the chain with a hole and the scale search: the hole path and the scale-list path of subtract()
def test_chain_subtracts_a_hole_and_walks_the_scale_list(det):
    img, sources = hole_scene()
    config, stats = dict(pair_config(True), residual_scales=3), {}
    chain = measure.Chain(det, upload(det, img), sources, config).run(measure.plan(config), stats)
    lists = measure.peak_lists(chain)
    assert list(lists) == ["residual_peaks", "residual_holes", "residual_scale_peaks", "residual_peaks_left", "residual_holes_left"]
    check_hole(lists)
    resid = chain.resid.cpu().numpy()
    comp, index, counts = measure.peak_render_selection(chain)
    assert np.array_equal(comp, chain.subtract_comp) and index == chain.subtract_index
    k = index.index(("residual_holes", 0))
    assert comp[k, 0] < 0 and chain.subtract_render_rows[k, 0] == 0 and (comp[[i for i in range(len(index)) if i != k], 0] > 0).all()
    rows, model, resid2 = DR.render_signed(resid, comp, float(config["residual_nsigma"]), None)
    assert np.array_equal(chain.subtract_render_rows, rows)
    got_model, got_resid2 = chain.peak_model.cpu().numpy().astype(np.float64), chain.resid2.cpu().numpy().astype(np.float64)
    assert (np.abs(got_model - model) <= RR.model_bound(model)).all() and (np.abs(got_resid2 - resid2) <= RR.resid_bound(resid2, model)).all()
    assert got_model.min() < -15.0
    # the scale list: fitted (its strongest entries), measured, and every selected scale entry clear of the pixel components; the
    # ones that sit on a pixel peak are counted as duplicates
    scale = lists["residual_scale_peaks"]
    fitted = chain.peakfit_select["residual_scale_peaks"]
    assert list(chain.disc_rows) == ["residual_peaks", "residual_holes", "residual_scale_peaks"] and len(fitted) >= 1
    nscale = sum(nm == "residual_scale_peaks" for nm, _ in index)
    assert counts["duplicates"] >= 1 and nscale + counts["duplicates"] <= len(fitted)
    assert stats["subtract_duplicates"] == counts["duplicates"] and stats["subtract_wandered"] == counts["wandered"] and stats["subtract_selected"] == len(index)
    for name in chain.disc_rows:
        ref, ab = DR.disc_residuals(chain.resid2.cpu().numpy(), chain.peak_model.cpu().numpy(), chain.peakfit_jobs[name])
        DR.compare(chain.disc_rows[name], ref, ab, ["%s[%d]" % (name, i) for i in chain.peakfit_select[name]])
    for i, d in enumerate(scale):
        assert (d["gres_npix"] is not None) == (i in fitted)
        if ("residual_scale_peaks", i) not in index:
            assert not d["gres_subtracted"]
    print("hole scene: %d components (%d of the scale list), %d duplicates, %d wandered; left: %d peaks, %d holes" % (
        len(index), nscale, counts["duplicates"], counts["wandered"], stats["left_peaks"], stats["left_holes"]))
