"""cy_forced_fit on the GPU against its numpy float64 restatement (tests/forced_ref.py) on the inputs of tests/forced_cases.py, and
the chain step --forced_fit on the real detector.

Status, npix, nexcluded, K, nneigh, crowded, ndup, the window and capped are integers decided the same way on both sides: equal.
syy, n00 and b0 are compared within C_SUM npix 2^-53 sum|t_i| (forced_ref's docstring derives C_SUM = 16 from the operation
count with the device's exp within 2 ulp); amp and bkg_off within twice the reference's first-order bound |inv(N)| (db + dN |x|)
plus K cond 2^-53 |x| for the solve; the variances and corr_max within the analogous bound |C| dN |C|; chi2 within its sum bound
plus the propagated solution bound (forced_ref.tolerances).  No tolerance is measured on the code under test, and no job is left
out of the value comparison except one whose reference pivot margin is below 2^-30.

The two jobs 1e-9 px apart (close_a, close_b) and their neighbour close_third: the reference's second pivot is t / N_jj of the
order 1e-16, far below the 2^-40 of the pivot rule, so they fall on the status-4 side on both sides and are compared as such (the
whole row: counts, sums and window, zeros for the solution); the margin rule of forced_ref.compare does not come into play for them."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import forced_cases as FC
import forced_ref as FR
from caesar_yolo_amd import lib as L
from gpu_common import detector
from test_gpu_peaks import upload

pytestmark = pytest.mark.gpu
GUARD = 8


@pytest.fixture(scope="module")
def det():
    return detector("fp32", max_batch=1, max_imgsz=160)


_refs = {}


def reference(g):
    if g.name not in _refs:
        _refs[g.name] = FR.forced_fit(g.map, g.rms, g.jobs, g.nsigma, g.fit_bkg)
    return _refs[g.name]


def guarded(det, a, offset=False):
    """The map between two rows of guard floats on the device.  -> (the map's view, the whole buffer)."""
    a = np.ascontiguousarray(a, np.float32)
    pad = 4 * GUARD + (1 if offset else 0)
    buf = torch.full((a.size + 2 * pad,), -7.5, dtype=torch.float32, device=det.tdev)
    dev = buf[pad:pad + a.size].view(a.shape)
    dev.copy_(torch.from_numpy(a.copy()))
    torch.cuda.synchronize()
    assert dev.is_contiguous() and (not offset or dev.data_ptr() % 16 == 4)
    return dev, buf, pad


def raw_call(det, map_dev, rms_dev, jobs, MH, MW, nsigma, fit_bkg):
    """The C entry with guard floats around h_out.  -> (rc, rows, whether the guards are untouched)."""
    jobs = np.ascontiguousarray(jobs, np.float64).reshape(-1, L.CY_FORCED_JOB_FIELDS)
    n = jobs.shape[0]
    buf = np.full(GUARD + n * L.CY_FORCED_FIELDS + GUARD, -7.5, np.float64)
    out = buf[GUARD:GUARD + n * L.CY_FORCED_FIELDS]
    dp = C.POINTER(C.c_double)
    rc = det.lib.cy_forced_fit(det.ctx, det._p(map_dev), det._p(rms_dev) if rms_dev is not None else None, MH, MW,
                               jobs.ctypes.data_as(dp) if n else None, n, float(nsigma), int(fit_bkg), out.ctypes.data_as(dp) if n else None, det._stream())
    torch.cuda.synchronize()
    return rc, out.reshape(n, L.CY_FORCED_FIELDS).copy(), bool((buf[:GUARD] == -7.5).all() and (buf[GUARD + n * L.CY_FORCED_FIELDS:] == -7.5).all())


@pytest.mark.parametrize("g", FC.groups(), ids=lambda g: g.name)
def test_case(det, g):
    ref, aux = reference(g)
    MH, MW = g.map.shape
    dev, buf, pad = guarded(det, g.map, g.offset)
    rdev, rbuf, _ = guarded(det, g.rms, g.offset) if g.rms is not None else (None, None, 0)
    rc, got, guards = raw_call(det, dev, rdev, g.jobs, MH, MW, g.nsigma, g.fit_bkg)
    assert rc == 0 and guards, g.name
    report = []
    FR.compare(got, ref, aux, ["%s / %s" % (g.name, nm) for nm in g.names], report)
    print("%s: worst |gpu - ref| / bound per field: %s" % (g.name, ", ".join("%s %.3g (%s)" % (f, r, nm) for nm, f, r in report)))
    # the wrapper gives the same bytes; the maps and the floats around them are only read; a repeat call: byte-equal
    again = det.forced_fit(dev, rdev, g.jobs, g.nsigma, bool(g.fit_bkg))
    assert again.shape == got.shape and again.tobytes() == got.tobytes(), "%s: a second call gave other bytes" % g.name
    for b, a in ((buf, g.map), (rbuf, g.rms)):
        if b is None:
            continue
        h = b.cpu().numpy()
        assert (h[:pad] == -7.5).all() and (h[pad + a.size:] == -7.5).all() and h[pad:pad + a.size].tobytes() == np.ascontiguousarray(a, np.float32).tobytes()
    if len(g.names) and np.isin(ref[:, 0], (0, 2, 4, 5)).any():
        assert det.forced_kernel_ms() > 0.0


def test_the_cases_reach_every_status_and_rule():
    ref, aux = reference(FC.by_name("main_64x96"))
    names = FC.by_name("main_64x96").names
    row = lambda nm: ref[names.index(nm)]
    assert set(ref[:, 0].astype(int)) == {0, 1, 3, 4, 5} and reference(FC.by_name("capped_520x515"))[0][0, 0] == 2
    assert [row(n)[0] for n in ("misses", "centre_1e300", "nan_x0", "negative_a", "bb_ge_ac", "inf_bkg")] == [3, 3, 1, 1, 1, 1]
    assert row("no_valid_pixel")[[0, 1]].tolist() == [5, 0] and row("npix_K_minus_1")[[0, 1, 3]].tolist() == [5, 1, 2]
    assert row("bad_pixels")[2] == 4 and row("isolated")[2] == 4 and row("isolated")[4] == 0
    assert row("dup2_0")[[4, 6]].tolist() == [0, 1] and row("dup3_0")[[4, 6]].tolist() == [1, 2] and row("dup3_neighbour")[[4, 6]].tolist() == [1, 2]
    assert [row(n)[0] for n in ("close_a", "close_b", "close_third")] == [4, 4, 4]
    crowd = [row("crowd_%d" % t) for t in range(10)]
    assert all(r[4] == 7 and r[5] == 1 and r[3] == 9 for r in crowd)
    plans = FR.plan(FC.by_name("main_64x96").jobs, 3.0, 64, 96)
    c0 = names.index("crowd_0")
    assert plans[c0]["neigh"][:2] == [c0 + 1, c0 + 2]             # +-2.5 px: equal distances, the lower index first
    cap = reference(FC.by_name("capped_520x515"))[0][0]
    assert cap[[17, 18, 19, 20, 21]].tolist() == [1, 514, 1, 514, 1] and cap[1] == 514 * 514
    assert reference(FC.by_name("map_1x1"))[0][:, 0].tolist() == [5, 3] and reference(FC.by_name("map_1x1_no_bkg"))[0][:, 0].tolist() == [0, 3]


def test_random_scene(det):
    img, rms, jobs, truth = FC.random_scene(1)
    assert 230 <= len(jobs) <= 245
    ref, aux = FR.forced_fit(img, rms, jobs, 3.0, 1)
    assert np.isin(ref[:, 0], (0, 2)).all()
    conds = np.array([a["cond"] for a in aux])
    print("random scene: %d jobs, scaled cond median %.3g, max %.3g; %d with neighbours, %d crowded" % (
        len(jobs), np.median(conds), conds.max(), int((ref[:, 4] > 0).sum()), int(ref[:, 5].sum())))
    assert conds.max() < 1e4
    dev, rdev = upload(det, img), upload(det, rms)
    got = det.forced_fit(dev, rdev, jobs, 3.0, True)
    report = []
    FR.compare(got, ref, aux, ["random[%d]" % i for i in range(len(jobs))], report)
    print("random scene: worst |gpu - ref| / bound per field: %s" % ", ".join("%s %.3g (%s)" % (f, r, nm) for nm, f, r in report))
    pull = (got[:, 7] - truth) / np.sqrt(got[:, 8])
    print("random scene: rms of (amp - truth) / sqrt(amp_var) on the GPU rows: %.3f" % np.sqrt((pull ** 2).mean()))
    assert 0.75 <= np.sqrt((pull ** 2).mean()) <= 1.35


def test_unaligned_pointers_give_the_same_rows(det):
    a, b = FC.by_name("main_64x96"), FC.by_name("main_offset")
    r0 = det.forced_fit(upload(det, a.map), upload(det, a.rms), a.jobs)
    r1 = det.forced_fit(upload(det, b.map, True), upload(det, b.rms, True), b.jobs)
    assert r0.tobytes() == r1.tobytes()


def test_argument_errors_leave_the_rows_untouched(det):
    g = FC.by_name("main_64x96")
    dev, rdev = upload(det, g.map), upload(det, g.rms)
    MH, MW = g.map.shape
    n = g.jobs.shape[0]
    jobs = np.ascontiguousarray(g.jobs)
    out = np.full((n, L.CY_FORCED_FIELDS), -7.5, np.float64)
    dp = C.POINTER(C.c_double)
    good = dict(ctx=det.ctx, m=det._p(dev), r=det._p(rdev), MH=MH, MW=MW, j=jobs.ctypes.data_as(dp), n=n, ns=3.0, fb=1, o=out.ctypes.data_as(dp))

    def call(**kw):
        a = dict(good, **kw)
        return det.lib.cy_forced_fit(a["ctx"], a["m"], a["r"], a["MH"], a["MW"], a["j"], a["n"], a["ns"], a["fb"], a["o"], det._stream())
    bad = [dict(ctx=None), dict(m=None), dict(j=None), dict(o=None), dict(MH=0), dict(MW=0), dict(MH=-3), dict(MW=-1), dict(MH=1 << 16, MW=1 << 15),
           dict(MH=(1 << 31) - 1, MW=(1 << 31) - 1), dict(n=-1), dict(n=L.CY_FORCED_JOBS_MAX + 1), dict(ns=0.999), dict(ns=8.001), dict(ns=float("nan")),
           dict(ns=float("inf")), dict(fb=2), dict(fb=-1), dict(m=None, n=0)]
    for kw in bad:
        assert call(**kw) == -1, kw                          # CY_ERR_ARG
        torch.cuda.synchronize()
        assert (out == -7.5).all(), kw
    for kw, text in ((dict(m=None), b"null argument"), (dict(j=None), b"null argument"), (dict(o=None), b"null argument"), (dict(MH=0), b"MH, MW > 0"),
                     (dict(MH=1 << 16, MW=1 << 15), b"2^31"), (dict(n=-1), b"n outside"), (dict(ns=9.0), b"nsigma"), (dict(fb=3), b"fit_bkg"),
                     # the order of the checks: map, shape, size, nsigma, fit_bkg, n, pointers
                     (dict(m=None, MH=0), b"null argument"), (dict(MH=0, MW=1 << 30, ns=0.0), b"MH, MW > 0"), (dict(MH=1 << 16, MW=1 << 15, ns=0.0), b"2^31"),
                     (dict(ns=0.0, fb=2, n=-1), b"nsigma"), (dict(fb=2, n=-1), b"fit_bkg"), (dict(n=-1, j=None), b"n outside")):
        assert call(**kw) == -1
        assert text in det.lib.cy_last_error(det.ctx), (kw, det.lib.cy_last_error(det.ctx))
    # n == 0 is no error and writes nothing, whatever the host pointers; a null rms map is no error
    assert call(n=0) == 0 and call(n=0, j=None, o=None) == 0 and (out == -7.5).all()
    assert call(r=None) == 0
    assert call() == 0
    assert out.tobytes() == det.forced_fit(dev, rdev, g.jobs).tobytes()
    for badcall in (lambda: det.forced_fit(dev.double(), rdev, g.jobs), lambda: det.forced_fit(dev.cpu(), rdev, g.jobs),
                    lambda: det.forced_fit(dev[:, :-1], rdev, g.jobs), lambda: det.forced_fit(dev, rdev[:-1], g.jobs)):
        with pytest.raises(L.CyError):
            badcall()
    assert det.forced_fit(dev, None, np.zeros((0, L.CY_FORCED_JOB_FIELDS))).shape == (0, L.CY_FORCED_FIELDS)


def test_kernel_time_is_kept():
    from caesar_yolo_amd.model import HipDetector
    from gpu_common import seeded_weights
    fresh = HipDetector(seeded_weights("l", 5)[0], device=0, precision="fp32", max_batch=1, max_imgsz=160)      # a context of its own
    assert fresh.forced_kernel_ms() == -1.0
    g = FC.by_name("main_64x96")
    dev = upload(fresh, g.map)
    fresh.forced_fit(dev, None, np.zeros((0, L.CY_FORCED_JOB_FIELDS)))
    away = fresh.forced_fit(dev, None, np.array([FC.job(float("nan"), 5.0), FC.job(-40.0, 5.0)]))
    assert fresh.forced_kernel_ms() == -1.0                   # no runnable job, no launch
    assert away[:, 0].tolist() == [1.0, 3.0] and (away[:, 17:21] == -1.0).all() and not away[:, 1:17].any() and not away[:, 21:].any()
    fresh.forced_fit(dev, None, g.jobs)
    ms = fresh.forced_kernel_ms()
    assert ms > 0.0
    fresh.forced_fit(dev, None, np.array([FC.job(float("nan"), 5.0)]))
    assert fresh.forced_kernel_ms() == ms                     # a call that launches nothing keeps the value
    fresh.close()


# ---- the chain
@pytest.fixture(scope="module")
def runs(det):
    """The chain on the real detector over forced_cases.chain_scene(): without the switch, and with it and the second map."""
    from caesar_yolo_amd import measure
    out = {}
    for key in ("plain", "forced"):
        img, second, sources = FC.chain_scene()
        config = dict(FC.CHAIN_CONFIG, forced_fit=key == "forced")
        others = [dict(tag="second", path="second.fits", freq=FC.CHAIN_NU[1], beam_area=12.0, upload=lambda d, a=second: upload(d, a))] if key == "forced" else None
        stats = {}
        chain = measure.Chain(det, upload(det, img), sources, config, beam_area=12.0, freq=FC.CHAIN_NU[0], forced_maps=others).run(measure.plan(config), stats)
        out[key] = (chain, stats, sources, img, second)
    return out


def test_chain_forced_dicts_against_the_reference(det, runs):
    """The rows of both maps against the reference run on the GPU's own components, maps and rms maps, then the dicts: the host
    arithmetic of annotate_forced on rows that passed."""
    from caesar_yolo_amd import measure
    chain, stats, sources, img, second = runs["forced"]
    comp, index = chain.forced_comp, chain.forced_index
    assert np.array_equal(comp, chain.render_comp)                # every selected component was rendered
    assert len(comp) == len(FC.CHAIN_PLANTED) and list(chain.forced_rows) == ["self", "second"]
    rms_self = det.expand_background(chain.mesh, chain.cell, img.shape, want=("rms",))[1].cpu().numpy()
    mesh2, ndef2 = measure.fill_mesh(det.measure_background(upload(det, second), cell=chain.cell, k=chain.clip_sigma, niter=chain.clip_iters), chain.min_pix)
    rms_second = det.expand_background(mesh2, chain.cell, img.shape, want=("rms",))[1].cpu().numpy()
    jobs = {"self": measure.forced_jobs(comp, index, sources, True), "second": measure.forced_jobs(comp, index, sources, mesh=mesh2, cell=chain.cell)}
    maps = []
    for tag, m, rms, beam, freq in (("self", img, rms_self, 12.0, FC.CHAIN_NU[0]), ("second", second, rms_second, 12.0, FC.CHAIN_NU[1])):
        assert np.array_equal(chain.forced_job_rows[tag], jobs[tag])
        ref, aux = FR.forced_fit(m, rms, jobs[tag], 3.0, 1)
        FR.compare(chain.forced_rows[tag], ref, aux, ["chain / %s[%d]" % (tag, i) for i in range(len(comp))])
        assert (ref[:, 0] == 0).all()
        maps.append(dict(tag=tag, rows=chain.forced_rows[tag], jobs=jobs[tag], beam_area=beam, freq=freq, err_scale=np.ones(len(comp))))
    probe = [dict(s, components=[{k: v for k, v in c.items() if not k.startswith("forced")} for c in s["components"]]) for s in sources]
    measure.annotate_forced(probe, index, maps)
    assert json.loads(json.dumps(probe)) == json.loads(json.dumps(sources))
    assert measure.peak_lists(chain)["forced_images"] == [
        dict(tag="self", path="scene.fits", freq=FC.CHAIN_NU[0], beam_area=12.0, mesh_ndef=chain.ndef),
        dict(tag="second", path="second.fits", freq=FC.CHAIN_NU[1], beam_area=12.0, mesh_ndef=ndef2)]
    assert (stats["forced_maps"], stats["forced_jobs"], stats["forced_fitted"], stats["forced_crowded"], stats["forced_singular"]) == (2, 8, 8, 0, 0)
    assert stats["forced_kernel_ms"] > 0.0 and stats["forced_ms"] > 0.0


def test_chain_self_peaks_agree_with_the_fits_and_alpha_is_recovered(runs):
    chain, stats, sources, img, second = runs["forced"]
    seen = 0
    for s in sources:
        for c in s["components"]:
            if c["forced"] is None:
                continue
            seen += 1
            f0, f1 = c["forced"]
            assert f0["status"] == 0 and f1["status"] == 0 and f0["nneigh"] == 0
            # the noise-weighted flux with a fitted local constant is the cross-check of the non-linear fit: within the two quoted errors
            assert abs(f0["peak"] - c["fit_peak"]) <= f0["peak_err"] + c["fit_peak_err"], (f0, c["fit_peak"], c["fit_peak_err"])
            assert abs(f0["flux"] - c["fit_flux"]) <= f0["flux_err"] + c["fit_flux_err"]
            # the second map is the first scaled by (nu2 / nu1)^-0.7: alpha within its own quoted 3 sigma of -0.7
            assert c["forced_alpha_n"] == 2 and abs(c["forced_alpha"] - FC.CHAIN_ALPHA) <= 3.0 * c["forced_alpha_err"], (c["forced_alpha"], c["forced_alpha_err"])
            print("component at (%.1f, %.1f): forced %.2f +- %.2f, fit %.2f +- %.2f, second %.3f +- %.4f, alpha %.3f +- %.3f" % (
                c["fit_x"], c["fit_y"], f0["peak"], f0["peak_err"], c["fit_peak"], c["fit_peak_err"], f1["peak"], f1["peak_err"], c["forced_alpha"],
                c["forced_alpha_err"]))
    assert seen == len(FC.CHAIN_PLANTED)


def test_chain_without_the_new_keys_is_the_run_without_the_switch(runs):
    from caesar_yolo_amd import measure
    plain, stats0, sources0, _, _ = runs["plain"]
    chain, stats, sources, _, _ = runs["forced"]
    assert plain.forced_rows is None and measure.peak_lists(plain) == {} and list(measure.peak_lists(chain)) == ["forced_images"]
    stripped = [dict(s, components=[{k: v for k, v in c.items() if not k.startswith("forced")} for c in s["components"]]) for s in sources]
    assert json.dumps(stripped) == json.dumps(sources0)
    timed = lambda k: k.endswith("_ms")
    assert {k: v for k, v in stats.items() if k not in measure.FORCED_STATS and not timed(k)} == {k: v for k, v in stats0.items() if not timed(k)}
    assert set(stats) == set(stats0) | set(measure.FORCED_STATS) and not set(stats0) & set(measure.FORCED_STATS)
    assert plain.resid.cpu().numpy().tobytes() == chain.resid.cpu().numpy().tobytes() and plain.model.cpu().numpy().tobytes() == chain.model.cpu().numpy().tobytes()
