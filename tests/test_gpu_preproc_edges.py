"""The preprocessing statistics kernel (pre_stats_kernel, csrc/cy_preproc.hip) on the constructed tiles of tests/preproc_cases.py,
against the numpy oracle (oracle/preprocessing_ref.py): the branches that natural tiles never take -- bracket miss and overflow with
their radix fallback, a collapsed sample bracket, the small-tile route, sets of 0..3 pixels, sd == 0, n == 0 after a clip, pixels on
the inclusive bounds, medians between two values, negative / sixty-decade / subnormal keys, zscale below, at and above the
1000-sample cap and below minpix, HISTEQ on quantised data, and a tile flush in the mosaic's bottom-right corner with tw % 4 != 0
next to tiles at origins that are not 4-aligned (preproc_cases.mosaic_layout).  The context's median_bracket_hits / _misses counters
are the witness that bimodal / ties took the fallback; tests/test_preproc_cases_cpu.py holds the cases' preconditions.

Tolerances are those of tests/test_gpu_preproc.py: clip bounds and zscale limits 1e-11 relative, sigma-clipped mean / std 1e-10,
float64 planes 1e-10 relative + 1e-13 with identical zero mask and identical NaN positions.  Status: 1 where the oracle returns None,
2 where its rows 0..2 fail the constant-row check, else 0.  One addition to that rule: a BkgSubtractor / SigmaClipShifter whose
sigma-clipped set ends empty makes the REFERENCE raise (min() of an empty array in its log call), which the
oracle does not restate; the kernel reports status 1 there and nothing else is compared for that tile and pipeline.

Left out of value parity (and only these):
* ZSCALE on a sample whose values are all equal.  The reference's np.polyfit returns a slope of rounding noise (the oracle gives
  vmin = 2.000000000000004, vmax = 1.999999999999996 for a tile of 2.0) and the sign of vmax - vmin decides between 0 and 0.5 for every
  pixel.  Asserted instead: both limits of the kernel equal the value to 1e-11 relative; the stages behind it are not compared.
* BkgSubtractor(use_mask_box=True, mask_fract=1.0): the reference produces an all-NaN image; not run."""
import warnings
import numpy as np
import pytest
import torch
from gpu_common import detector
from caesar_yolo_amd import preprocessing as PP
import preproc_cases as K
from oracle import preprocessing_ref as P

pytestmark = pytest.mark.gpu

CHAN3 = dict(sigma_clip_baseline=0, sigma_clip_low=10, sigma_clip_up=10, zscale_contrast=0.25)
PIPES = {   # name -> (device stages, oracle spec)
    "clip_1_1": (lambda M: [M.SigmaClipper(sigma_low=1, sigma_up=1)], [("clip", dict(sigma_low=1, sigma_up=1))]),
    "clip_10_10": (lambda M: [M.SigmaClipper(sigma_low=10, sigma_up=10)], [("clip", dict(sigma_low=10, sigma_up=10))]),
    "clip_half": (lambda M: [M.SigmaClipper(sigma_low=0.5, sigma_up=0.5)], [("clip", dict(sigma_low=0.5, sigma_up=0.5))]),
    "bkg_3": (lambda M: [M.BkgSubtractor(sigma=3)], [("bkg", dict(sigma=3))]),
    "shift_1": (lambda M: [M.SigmaClipShifter(sigma=1)], [("shift", dict(sigma=1))]),
    "bkg_clip": (lambda M: [M.BkgSubtractor(sigma=3), M.SigmaClipper(sigma_low=1, sigma_up=1)],
                 [("bkg", dict(sigma=3)), ("clip", dict(sigma_low=1, sigma_up=1))]),
    "minmax": (lambda M: [M.MinMaxNormalizer(norm_min=0, norm_max=255)], [("minmax", dict(norm_min=0, norm_max=255))]),
    "zscale": (lambda M: [M.ZScaleTransformer(contrasts=[0.25] * 3)], [("zscale", dict(contrasts=[0.25] * 3))]),
    "zscale_minmax": (lambda M: [M.ZScaleTransformer(contrasts=[0.25] * 3), M.MinMaxNormalizer(norm_min=0, norm_max=255)],
                      [("zscale", dict(contrasts=[0.25] * 3)), ("minmax", dict(norm_min=0, norm_max=255))]),
    "clip_zscale_minmax": (lambda M: [M.SigmaClipper(sigma_low=1, sigma_up=1), M.ZScaleTransformer(contrasts=[0.25] * 3),
                                      M.MinMaxNormalizer(norm_min=0, norm_max=255)],
                           [("clip", dict(sigma_low=1, sigma_up=1)), ("zscale", dict(contrasts=[0.25] * 3)),
                            ("minmax", dict(norm_min=0, norm_max=255))]),
    "chan3": (lambda M: [M.ChanResizer(nchans=3), M.Chan3Trasformer(**CHAN3)], [("chanresize", dict(nchans=3)), ("chan3", CHAN3)]),
    "chan3_minmax": (lambda M: [M.ChanResizer(nchans=3), M.Chan3Trasformer(**CHAN3), M.MinMaxNormalizer(norm_min=0, norm_max=255)],
                     [("chanresize", dict(nchans=3)), ("chan3", CHAN3), ("minmax", dict(norm_min=0, norm_max=255))]),
}
_REF = {}


def _zs_degenerate(ch):
    v = ch.ravel()
    v = v[np.isfinite(v)]
    s = v[::int(max(1.0, v.size / P.ZS_NSAMPLES))][:P.ZS_NSAMPLES]
    return (float(s[0]),) if s.size and s.min() == s.max() else None


def reference(group, name, pname):
    """The oracle, stage by stage, on one tile -> dict: params = [(stage index, values, rtol)] of channel program 0, out = the (H, W, 3)
    image or None, status, degenerate = (stage index, value) of a ZSCALE on an all-equal sample (nothing behind it is compared), or for a
    chan3 pipeline True.  Computed once per (tile, pipeline)."""
    key = (group, name, pname)
    if key in _REF:
        return _REF[key]
    tile = K.case(group, name)
    spec = PIPES[pname][1]
    r = dict(params=[], out=None, status=None, degenerate=None, raises=False)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        data = P.to_cube(tile.astype(np.float64))
        if pname.startswith("chan3"):
            for lo in (CHAN3["sigma_clip_baseline"], CHAN3["sigma_clip_low"]):
                clipped = P.SigmaClipper(lo, CHAN3["sigma_clip_up"])(data[:, :, :1])
                if _zs_degenerate(clipped[:, :, 0]) is not None:
                    r["degenerate"] = True
            data = P.build_pipeline(spec)(data)
        else:
            for k, (st, kw) in enumerate(spec):
                if data is None:
                    break
                ch = data[:, :, 0]
                cond = P.nonzero_finite(ch)
                if st in ("bkg", "shift"):
                    f, _, _ = P.sigma_clip_1d(ch[cond], None, None, sigma=kw["sigma"])
                    if f.size == 0:
                        r["raises"] = True
                        break
                    m, sd = float(np.mean(f)), float(np.std(f))
                    r["params"].append((k, [m], 1e-10) if st == "bkg" else (k, [m + kw["sigma"] * sd, m, sd], 1e-10))
                elif st == "clip":
                    _, lo, hi = P.sigma_clip_1d(ch[cond], kw["sigma_low"], kw["sigma_up"])
                    r["params"].append((k, [lo, hi], 1e-11))
                elif st == "zscale":
                    d = _zs_degenerate(ch)
                    if d is not None:
                        r["degenerate"] = (k, d[0])
                        break
                    r["params"].append((k, list(P.zscale_limits(ch, kw["contrasts"][0])), 1e-11))
                data = P.build_pipeline([(st, kw)])(data)
    if r["raises"]:
        r["status"] = 1
    elif r["degenerate"] is None:
        r["out"] = data
        r["status"] = 1 if data is None else (2 if P.rows_constant(data) else 0)
    elif r["degenerate"] is True and data is not None:
        r["out"] = data                                            # (the HISTEQ channel is still compared)
    _REF[key] = r
    return r


MAX_BATCH = 4                    # tiles per launch: the shared test context's max_batch (gpu_common.detector)


def _launch(det, group, pname, names=None):
    """All tiles of the group through one pipeline, MAX_BATCH tiles per launch, each launch on a mosaic of its own whose last tile sits
    flush in the bottom-right corner -> (names, planes [B, 3, th, tw], status [B], parameters [B, 3, stages, 4])"""
    tiles = [(n, t) for n, t, _ in K.GROUPS[group] if names is None or n in names]
    th, tw = tiles[0][1].shape
    cfg = PP.DataPreprocessor(PIPES[pname][0](PP)).program()
    planes, status, params = [], [], []
    for i in range(0, len(tiles), MAX_BATCH):
        m, xy = K.mosaic_layout([t for _, t in tiles[i:i + MAX_BATCH]])
        mosaic = det.mosaic_to_device(m.astype(">f4"))             # big-endian like a FITS payload; NaN -> 0 on ingest
        pl, st = det.preproc_planes(mosaic, xy, th, tw, cfg)
        torch.cuda.synchronize()
        planes.append(pl.cpu().numpy())
        status += st.cpu().tolist()
        params.append(det.preproc_params(len(xy)).copy())
    return [n for n, _ in tiles], np.concatenate(planes), status, np.concatenate(params)


@pytest.mark.parametrize("pname", sorted(PIPES))
@pytest.mark.parametrize("group", sorted(K.GROUPS))
def test_constructed_tiles_match_the_oracle(group, pname):
    det = detector("fp32", max_imgsz=640)
    names, planes, status, params = _launch(det, group, pname)
    problems = []
    for b, name in enumerate(names):
        r = reference(group, name, pname)
        what = "%s/%s/%s" % (group, name, pname)
        try:
            for k, want, rtol in r["params"]:
                got = params[b, 0, k, :len(want)]
                print("%s stage %d: kernel %r oracle %r" % (what, k, got.tolist(), want))
                assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN parameters differ"
                np.testing.assert_allclose(got, want, rtol=rtol, atol=0)
            if r["status"] is not None:
                assert status[b] == r["status"], "status %d, the oracle implies %d" % (status[b], r["status"])
            if isinstance(r["degenerate"], tuple):
                k, value = r["degenerate"]
                np.testing.assert_allclose(params[b, 0, k, :2], [value, value], rtol=1e-11, atol=0)
            if r["out"] is not None:
                got = planes[b].transpose(1, 2, 0)
                ref = r["out"]
                if r["degenerate"] is True:
                    got, ref = got[:, :, 2], ref[:, :, 2]
                assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaNs at different positions"
                ok = ~np.isnan(ref)
                assert np.array_equal(got[ok] == 0, ref[ok] == 0), "zero masks differ at %d pixels" % int(((got == 0) != (ref == 0))[ok].sum())
                np.testing.assert_allclose(got[ok], ref[ok], rtol=1e-10, atol=1e-13)
        except AssertionError as e:
            problems.append("%s: %s" % (what, str(e).strip().replace("\n", " | ")[:600]))
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("group,name", [("big", "bimodal"), ("big", "ties"), ("big_odd", "bimodal"), ("big_odd", "ties")])
def test_bracket_miss_takes_the_radix_fallback(group, name):
    """bimodal: the first clip moves the median out of its bracket; ties: every bracket overflows its capacity.  Both as the first stage
    (raw pixels, sample bracket) and behind a BKG stage (replayed values, no sample), each launch on its own."""
    det = detector("fp32", max_imgsz=640)
    det.counters(reset=True)
    _, _, _, par = _launch(det, group, "clip_1_1", [name])
    c = det.counters(reset=True)
    print(group, name, "clip_1_1", c)
    assert c["median_bracket_misses"] >= 1
    np.testing.assert_allclose(par[0, 0, 0, :2], reference(group, name, "clip_1_1")["params"][0][1], rtol=1e-11)
    _launch(det, group, "bkg_3", [name])
    c_bkg = det.counters(reset=True)
    _, _, _, par = _launch(det, group, "bkg_clip", [name])
    c = det.counters(reset=True)
    print(group, name, "bkg_3", c_bkg, "bkg_clip", c)
    assert c["median_bracket_misses"] - c_bkg["median_bracket_misses"] >= 1       # the CLIP stage behind the BKG stage missed
    np.testing.assert_allclose(par[0, 0, 1, :2], reference(group, name, "bkg_clip")["params"][1][1], rtol=1e-11)


def test_plain_noise_hits_its_brackets():
    det = detector("fp32", max_imgsz=640)
    det.counters(reset=True)
    _launch(det, "big", "clip_1_1", ["noise"])
    c = det.counters(reset=True)
    print("noise", c)
    assert c["median_bracket_hits"] >= 1 and c["median_bracket_misses"] == 0


@pytest.mark.parametrize("group,names", [("big", ["bimodal", "ties"]), ("big_odd", ["bimodal", "ties"]), ("small", ["two_valued"])])
def test_variants_agree_on_the_fallback_tiles(group, names, monkeypatch):
    det = detector("fp32", max_imgsz=640)
    for pname in ("clip_1_1", "bkg_clip"):
        monkeypatch.setenv("CY_PRE_VARIANT", "0")
        _, _, st0, par0 = _launch(det, group, pname, names)
        for variant in (2, 4, 8, 64):
            monkeypatch.setenv("CY_PRE_VARIANT", str(variant))
            _, _, st, par = _launch(det, group, pname, names)
            assert st == st0
            np.testing.assert_allclose(par, par0, rtol=1e-12, atol=0, err_msg="%s %s, variant %d" % (group, pname, variant))
