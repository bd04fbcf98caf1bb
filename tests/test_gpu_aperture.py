"""cy_aperture_sums on the GPU against its float64 restatement (tests/aperture_ref.py) on the inputs of tests/aperture_cases.py.

No tolerance anywhere: the window and the ring of a pixel are single rounded operations in a fixed order, contraction is off in the
kernel, the three sums of a ring are added in the association the reference reproduces, counts and the two medians depend on no
order.  Every row is compared as uint64 bit patterns (no field is NaN).  Nothing here was tuned on the GPU.

The chain-level test runs measure.Chain on the 256 x 256 two-blob scene of tests/atrous_chain_ref.py with peak_apertures on: every
entry of the lists equals annotate_apertures over the reference applied to the chain's own residual and rms maps, and the keys the
entries had before equal those of a run without the switch."""
import ctypes as C

import numpy as np
import pytest
import torch

import aperture_cases as PC
import aperture_ref as PR
import atrous_chain_ref as ACR
from caesar_yolo_amd import lib as L
from caesar_yolo_amd import measure
from gpu_common import detector

pytestmark = pytest.mark.gpu
H, F = L.CY_APER_HEAD, L.CY_APER_RING_FIELDS


@pytest.fixture(scope="module")
def det():
    return detector("fp32", max_batch=1, max_imgsz=160)


def upload(det, a):
    dev = torch.from_numpy(np.ascontiguousarray(a, np.float32).copy()).to(det.tdev)
    torch.cuda.synchronize()
    return dev


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_rows(name, got, want):
    assert got.shape == want.shape, name
    g, w = bits(got), bits(want)
    if not np.array_equal(g, w):
        i, f = (int(v[0]) for v in np.nonzero(g != w))
        raise AssertionError("%s: %d of %d fields differ; first: job %d field %d: %r on the GPU, %r in the reference" % (
            name, int((g != w).sum()), g.size, i, f, got[i, f], want[i, f]))


@pytest.mark.parametrize("with_rms", [True, False], ids=["rms", "no_rms"])
@pytest.mark.parametrize("name", PC.NAMES)
def test_case(det, name, with_rms):
    c = PC.case(name)
    want = PC.rows(name, with_rms)
    assert not np.isnan(want).any()
    dmap, drms = upload(det, c.map), upload(det, c.rms) if with_rms else None
    got = det.aperture_sums(dmap, drms, c.jobs, c.factors)
    assert_rows(name, got, want)
    # both maps are read only; a second call gives the same bytes
    assert dmap.cpu().numpy().tobytes() == c.map.tobytes() and (drms is None or drms.cpu().numpy().tobytes() == c.rms.tobytes())
    assert det.aperture_sums(dmap, drms, c.jobs, c.factors).tobytes() == got.tobytes(), "%s: a second call gave other bytes" % name


def test_the_exact_scene_holds_to_its_integers(det):
    c = PC.case("exact_scene")
    row = det.aperture_sums(upload(det, c.map), upload(det, c.rms), c.jobs, c.factors)[0]
    disc, npix = 113, [13, 49, 113, 197, 317, 613]            # pixels within the radii 2, 4, 6, 8, 10, 14 of an integer centre
    assert row[:8].tolist() == [0, 26, 54, 26, 54, 0, 3.0, 0.0]
    ring = np.diff([0] + npix)
    assert row[H::F][:6].tolist() == ring.tolist() and row[H + 3::F][:6].tolist() == (4.0 * ring).tolist()
    assert row[H + 1::F][:6].tolist() == [5.0 * 13, 5.0 * 36, 5.0 * 64, 3.0 * 84, 3.0 * 120, 3.0 * 296]
    d = measure.annotate_apertures([{}], row[None], 5, 0)[0]
    assert d["ap_npix"] == npix[:5] and d["ap_nbkg"] == 296 and d["ap_bkg"] == 3.0 and d["ap_bkg_rms"] == 0.0
    assert d["ap_flux_sum"] == [2.0 * 13, 2.0 * 49, 2.0 * disc, 2.0 * disc, 2.0 * disc]


def test_argument_errors_leave_the_rows_untouched(det):
    c = PC.case("centres")
    dmap, drms = upload(det, c.map), upload(det, c.rms)
    MH, MW = c.map.shape
    n = c.jobs.shape[0]
    jobs, factors = np.ascontiguousarray(c.jobs), np.array(c.factors, np.float64)
    out = np.full((n, L.CY_APER_FIELDS), -7.5, np.float64)
    dp = C.POINTER(C.c_double)
    good = dict(ctx=det.ctx, m=det._p(dmap), r=det._p(drms), MH=MH, MW=MW, j=jobs.ctypes.data_as(dp), n=n, f=factors.ctypes.data_as(dp), K=len(factors),
                o=out.ctypes.data_as(dp))

    def call(**kw):
        a = dict(good, **kw)
        return det.lib.cy_aperture_sums(a["ctx"], a["m"], a["r"], a["MH"], a["MW"], a["j"], a["n"], a["f"], a["K"], a["o"], det._stream())
    keep = [np.array(v, np.float64) for v in ((0.0, 1.0), (-1.0, 1.0), (1.0, 1.0), (2.0, 1.0), (1.0, np.nan), (np.inf, 1.0), (1.0, np.inf), (1.0, 2.0, 2.0))]
    bad = [dict(ctx=None), dict(m=None), dict(j=None), dict(f=None), dict(o=None), dict(MH=0), dict(MW=0), dict(MH=-3), dict(MW=-1),
           dict(MH=1 << 16, MW=1 << 15), dict(MH=(1 << 31) - 1, MW=(1 << 31) - 1), dict(n=-1), dict(n=L.CY_APER_JOBS_MAX + 1),
           dict(K=0), dict(K=-1), dict(K=9)] + [dict(f=v.ctypes.data_as(dp), K=v.size) for v in keep]
    for kw in bad:
        assert call(**kw) == -1, kw                          # CY_ERR_ARG
        torch.cuda.synchronize()
        assert (out == -7.5).all(), kw
    for kw, text in ((dict(m=None), b"null argument"), (dict(MH=0), b"MH, MW > 0"), (dict(MH=1 << 16, MW=1 << 15), b"2^31"), (dict(n=-1), b"n outside"),
                     (dict(K=9), b"K outside"), (dict(f=keep[3].ctypes.data_as(dp), K=2), b"strictly increasing")):
        call(**kw)
        assert text in det.lib.cy_last_error(det.ctx), (kw, det.lib.cy_last_error(det.ctx))
    # n == 0 is no error and writes nothing, whatever the pointers; a null rms map is allowed
    assert call(n=0) == 0 and call(n=0, m=None, j=None, o=None) == 0 and (out == -7.5).all()
    assert call(r=None) == 0 and out[0, 0] == 0.0
    assert_rows("no rms", out, PC.rows("centres", False))
    assert call() == 0
    assert_rows("rms", out, PC.rows("centres", True))
    with pytest.raises(L.CyError):
        det.aperture_sums(dmap, drms, c.jobs, (2.0, 1.0))
    with pytest.raises(L.CyError):
        det.aperture_sums(dmap, drms[:, :-1], c.jobs, c.factors)
    with pytest.raises(L.CyError):
        det.aperture_sums(dmap.double(), None, c.jobs, c.factors)
    with pytest.raises(L.CyError):
        det.aperture_sums(dmap.cpu(), None, c.jobs, c.factors)
    assert det.aperture_sums(dmap, None, np.zeros((0, 3)), c.factors).shape == (0, L.CY_APER_FIELDS)


def test_kernel_time_is_kept():
    from caesar_yolo_amd.model import HipDetector
    from gpu_common import seeded_weights
    fresh = HipDetector(seeded_weights("l", 5)[0], device=0, precision="fp32", max_batch=1, max_imgsz=160)      # a context of its own
    assert fresh.aperture_kernel_ms() == -1.0
    c = PC.case("area_1025")
    fresh.aperture_sums(upload(fresh, c.map), None, np.zeros((0, 3)), c.factors)
    assert fresh.aperture_kernel_ms() == -1.0                 # no job, no launch
    fresh.aperture_sums(upload(fresh, c.map), None, c.jobs, c.factors)
    assert fresh.aperture_kernel_ms() > 0.0
    fresh.close()


# ---- the chain
def test_chain_measures_what_the_searches_list(det):
    img, sources = ACR.scene()
    config = dict(ACR.CONFIG, residual_holes=True, peak_apertures=True, aperture_unit=1.0, aperture_radii="1,2,3,4", aperture_annulus=6.0)
    plain, _ = ACR.run(det, upload(det, img), [dict(s) for s in sources], dict(config, peak_apertures=False))
    chain, stats = ACR.run(det, upload(det, img), sources, config)
    resid = chain.resid.cpu().numpy()
    rms = det.expand_background(chain.mesh, chain.cell, img.shape, want=("rms",))[1].cpu().numpy()
    lists, before = measure.peak_lists(chain), measure.peak_lists(plain)
    assert set(lists) == set(before) == {"residual_peaks", "residual_holes", "residual_scale_peaks"} and len(lists["residual_scale_peaks"]) >= 2
    table, jobs_total, measured, clipped = (1.0, 2.0, 3.0, 4.0, 6.0), 0, 0, 0
    assert list(chain.aperture_rows) == [k for k in ("residual_peaks", "residual_holes", "residual_scale_peaks") if lists[k]]
    for name, rows in chain.aperture_rows.items():
        entries = lists[name]
        unit = [float(d.get("step", 1)) for d in entries]
        jobs = np.array([[d["x"], d["y"], u] for d, u in zip(entries, unit)], np.float64)
        want_rows = PR.reference(resid, rms, jobs, table)
        assert_rows(name, rows, want_rows)
        want = measure.annotate_apertures([{} for _ in entries], want_rows, 4, 0, [[u * f for f in table[:4]] for u in unit])
        for d, w, d0 in zip(entries, want, before[name]):
            assert {k: d[k] for k in measure.APERTURE_KEYS} == w and {k: v for k, v in d.items() if k not in measure.APERTURE_KEYS} == d0
            assert tuple(d) == tuple(d0) + measure.APERTURE_KEYS
        jobs_total, measured, clipped = jobs_total + len(entries), measured + int((want_rows[:, 0] == 0).sum()), clipped + int(want_rows[:, 5].sum())
    assert (stats["apertures_jobs"], stats["apertures_measured"], stats["apertures_clipped"]) == (jobs_total, measured, clipped)
    assert stats["aperture_kernel_ms"] > 0.0 and stats["apertures_ms"] > 0.0 and measured >= 2
    # the two blobs: a strongest entry each, measured at its own scale with the annulus inside the map, a positive curve of growth
    for x0, y0 in ACR.BLOBS:
        near = [p for p in lists["residual_scale_peaks"] if p["strongest"] and np.hypot(p["x_peak"] - x0, p["y_peak"] - y0) <= 4.0]
        assert len(near) == 1 and near[0]["ap_status"] == 0 and near[0]["ap_radius"] == [near[0]["step"] * f for f in (1.0, 2.0, 3.0, 4.0)]
        print("blob at (%d, %d): scale %d, ap_flux_sum %s, bkg %.3g +- %.3g over %d px" % (
            x0, y0, near[0]["scale"], [round(v, 1) for v in near[0]["ap_flux_sum"]], near[0]["ap_bkg"], near[0]["ap_bkg_rms"], near[0]["ap_nbkg"]))
    assert plain.aperture_rows is None and not [k for lst in before.values() for d in lst for k in d if k.startswith("ap_")]
    assert sources == plain.sources
