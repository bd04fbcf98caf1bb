"""The model / residual step on the CPU: the reference (tests/residual_ref.py) against the analytic Gaussian, the measured tolerance
TOL_M, the host side of the step (measure.render_selection, measure.annotate_residuals, the three flags of scripts/run.py) and the
exports and field counts of the binding."""
import math
import os
import re
import sys

import numpy as np
import pytest

import residual_cases as RC
import residual_ref as RR
from caesar_yolo_amd import lib as L
from caesar_yolo_amd import measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference
@pytest.mark.parametrize("sig", [(2.0, 2.0, 0.0), (2.5, 1.2, 30.0), (3.0, 0.9, -75.0)])
def test_reference_is_the_analytic_gaussian(sig):
    MH, MW = 70, 75
    p = RC.gauss_params(7.5, 30.3, 28.8, *sig)
    rows, model, resid = RR.render(np.full((MH, MW), 1.0, np.float32), [p], 5.0)
    t = math.radians(sig[2])
    y, x = np.mgrid[0:MH, 0:MW].astype(np.float64)
    dx, dy = x - 30.3, y - 28.8
    along, across = dx * math.cos(t) + dy * math.sin(t), -dx * math.sin(t) + dy * math.cos(t)
    want = 7.5 * np.exp(-0.5 * ((along / sig[0]) ** 2 + (across / sig[1]) ** 2))
    sx0, sx1, sy0, sy1 = (int(v) for v in rows[0, 1:5])
    inside = np.zeros((MH, MW), bool)
    inside[sy0:sy1 + 1, sx0:sx1 + 1] = True
    assert np.allclose(model[inside], want[inside], rtol=1e-12, atol=0) and not model[~inside].any()
    assert want[~inside].max() < 7.5 * math.exp(-0.5 * 25.0) * 1.0001         # outside the rectangle: beyond 5 marginal sigma
    assert np.array_equal(resid, 1.0 - model)
    # the rectangle: 5 marginal sigmas either side of floor(centre), floor(centre) + 1
    a, b, c = p[3:]
    det = a * c - b * b
    hx, hy = math.ceil(5.0 * math.sqrt(c / det)), math.ceil(5.0 * math.sqrt(a / det))
    assert rows[0].tolist() == [0.0, 30 - hx, 31 + hx, 28 - hy, 29 + hy, rows[0, 5], 0.0, 0.0]


def test_reference_statuses_and_pixels():
    ref = RC.reference()
    assert ref["not_admissible_A"][0][:, 0].tolist() == [1.0] * 8 + [0.0]
    assert ref["outside_A"][0][:, 0].tolist() == [3.0, 3.0, 3.0, 0.0] and (ref["outside_A"][0][:3, 1:5] == -1).all()
    assert ref["sigma1000"][0][:, 0].tolist() == [2.0, 2.0, 2.0]
    assert ref["sigma1000"][0][0, 1:5].tolist() == [0.0, 299.0, 0.0, 299.0]           # 150 +- 256 clipped to the image
    assert ref["reaching_in_A"][0][0, 1:3].tolist() == [0.0, 7.0]
    assert (ref["scene600"][0][:, 0] == 0.0).all()
    assert not ref["m0_A"][1].any()
    img, bkg = RC.images()["A"], RC.backgrounds()["A"]
    ok = RR.valid(img)
    assert (~ok).sum() == 4 and not ref["two_one_tile_A"][2][~ok].any()
    assert np.array_equal(ref["m0_A"][2][ok], img[ok].astype(np.float64) - bkg[ok].astype(np.float64))
    assert np.array_equal(ref["m0_no_bkg_A"][2][ok], img[ok].astype(np.float64))
    # nsigma only moves the rectangles: a wider one adds terms, it changes none
    r1, r8 = ref["nsigma1_A"], ref["nsigma8_A"]
    assert (r1[1] != 0).sum() < (r8[1] != 0).sum() and (r1[1] <= r8[1]).all()


def test_tolerance_measurement():
    """TOL_M = 16 x the largest relative difference of the float64 model between the exp variants, over every render case."""
    imgs = RC.images()
    worst = max(RR.model_spread(comp, nsigma, *imgs[key].shape) for _, key, comp, nsigma, _, _ in RC.render_cases())
    print("largest relative model difference between the exp variants: %.4g (recorded %.4g)" % (worst, RR.MEASURED))
    assert 0.9 * RR.MEASURED <= worst <= RR.MEASURED
    assert RR.TOL_M == 16 * RR.MEASURED == 16 * 8.46e-16


def test_reference_statistics():
    img = RC.images()["S"]
    boxes, bkg, masks, names = RC.stats_case()
    model = RC.reference()["scene600"][1].astype(np.float32)
    out, ab = RR.residual_stats(img, model, boxes, bkg, masks)
    k = names.index("max_twice")
    assert out[k, [1, 2, 7, 8, 9, 10]].tolist() == [441.0, 441.0, 49.75, 497.0, 33.0, 0.0]
    assert out[names.index("empty")].tolist() == out[names.index("blank")].tolist() == [0.0] * 8 + [-1.0, -1.0, 0.0, 0.0]
    assert out[names.index("px4096"), 1] == 4096 - 0 and out[names.index("px4097"), 1] == 4097
    assert out[names.index("nan_under"), 1] == 21 * 13 - 3            # two NaN and one zero pixel inside the box
    b = names.index("bytes")
    assert set(np.unique(masks[b])) == {0, 1, 2, 3, 16, 255} and out[b, 2] == (masks[b] != 0).sum()
    assert (out[:, 2] <= out[:, 1]).all() and (ab >= np.abs(out[:, [3, 4, 5, 6, 10]]) * (1 - 1e-12)).all()


# ---- the host side
def _source(peaks):
    return {"x1": 0.0, "y1": 0.0, "x2": 9.0, "y2": 9.0, "rms": 0.5, "rms_map": 0.25,
            "components": [{"x_peak": x, "y_peak": y} for x, y in peaks]}


def _rows(n):
    fit, blend = np.zeros((n, 16, 32)), np.zeros((n, 16, 36))
    fit[:, :, 0] = 3.0
    blend[:, :, 0] = 6.0
    return fit, blend


def test_render_selection():
    src = [_source([(5, 5), (7, 7), (9, 9), (11, 11), (13, 13), (15, 15)]), _source([(7, 7), (20, 20)]), {"components": None}, _source([])]
    fit, blend = _rows(4)
    P = lambda v: [v, v + 0.5, v + 0.25, 1.0, 0.0, 1.0]
    for k, st in enumerate((0.0, 2.0, 0.0, 0.0, 0.0, 4.0)):          # source 0: fits with status 0, 2, 0, 0, 0 and one that failed
        fit[0, k, 0], fit[0, k, 5:11] = st, P(10.0 + k)
    for k, st in enumerate((0.0, 2.0, 3.0, 4.0, 5.0, 0.0)):          # its blend rows: 0 and 2 win, 3 4 5 fall back to the fit
        blend[0, k, 0], blend[0, k, 8:14] = st, P(100.0 + k)
    fit[1, 0, 0], fit[1, 0, 5:11] = 0.0, P(30.0)                      # the peak pixel (7, 7) again: a duplicate
    fit[1, 1, 0], fit[1, 1, 5:11] = 1.0, P(31.0)                      # status 1: not rendered
    blend[1, 1, 0] = 1.0
    comp, index, ndup = measure.render_selection(src, fit, blend)
    assert index.tolist() == [[0, 0], [0, 1], [0, 2], [0, 3], [0, 4], [0, 5]] and ndup == 1
    assert comp[:, 0].tolist() == [100.0, 101.0, 12.0, 13.0, 14.0, 105.0]     # 5: the fit failed but the joint fit did not
    assert np.array_equal(comp[0], P(100.0)) and np.array_equal(comp[2], P(12.0))
    # without blend rows: the fits alone; the failed fit drops out, and the second source's duplicate stays out
    comp, index, ndup = measure.render_selection(src, fit)
    assert ndup == 1 and index.tolist() == [[0, 0], [0, 1], [0, 2], [0, 3], [0, 4]] and comp[:, 0].tolist() == [10.0, 11.0, 12.0, 13.0, 14.0]
    # the earlier component wins whatever it is: with source 0's component 1 not fitted, source 1 renders the shared peak
    fit[0, 1, 0] = 3.0
    comp, index, ndup = measure.render_selection(src, fit)
    assert ndup == 0 and index.tolist() == [[0, 0], [0, 2], [0, 3], [0, 4], [1, 0]] and comp[-1, 0] == 30.0
    comp, index, ndup = measure.render_selection([], np.zeros((0, 16, 32)))
    assert comp.shape == (0, 6) and index.shape == (0, 2) and ndup == 0


def test_annotate_residuals():
    src = [_source([(5, 5), (7, 7)]), _source([(7, 7)]), _source([(1, 1)]), {"components": None, "rms": 1.0}]
    raw = np.array([[0, 50, 20, 5.0, 9.0, 4.0, 8.0, 1.5, 6, 7, 30.0, 0],
                    [0, 10, 0, 1.0, 2.0, 0, 0, 0, -1, -1, 0, 0],
                    [1, 0, 0, 0, 0, 0, 0, 0, -1, -1, 0, 0],
                    [0, 0, 4, 0.0, 0.0, 2.0, 4.0, 1.0, 3, 3, 1.0, 0]], np.float64)
    index = np.array([[0, 0], [0, 1], [2, 0]])
    rrows = np.zeros((3, 8))
    rrows[:, 0] = [0.0, 2.0, 3.0]
    measure.annotate_residuals(src, raw, index, rrows, beam_area=4.0, origin=(100, 200), use_map=False)
    s = src[0]
    assert set(measure.RESIDUAL_KEYS) <= set(s)
    assert (s["res_npix"], s["res_mean"], s["res_rms"], s["res_rms_box"]) == (20, 0.2, math.sqrt(0.4), math.sqrt(9.0 / 50))
    assert (s["res_max"], s["res_x_max"], s["res_y_max"], s["res_flux"], s["res_model_flux"]) == (1.5, 106, 207, 1.0, 7.5)
    assert s["res_ratio"] == math.sqrt(0.4) / 0.5
    assert [(d["rendered"], d["render_status"]) for d in s["components"]] == [(True, 0), (True, 2)]
    assert src[1]["components"][0] == {"x_peak": 7, "y_peak": 7, "rendered": False, "render_status": None}
    assert src[2]["components"][0]["rendered"] is False and src[2]["components"][0]["render_status"] == 3
    for t in (src[1], src[2]):
        assert t["res_npix"] == 0 and all(t[k] is None for k in measure.RESIDUAL_KEYS[1:])
    assert src[3]["res_rms_box"] is None and src[3]["res_rms"] == 1.0 and src[3]["res_ratio"] == 1.0
    measure.annotate_residuals(src[:1], raw[:1], index[:2], rrows[:2], beam_area=0, use_map=True)
    assert src[0]["res_flux"] is None and src[0]["res_model_flux"] is None and src[0]["res_ratio"] == math.sqrt(0.4) / 0.25
    assert (src[0]["res_x_max"], src[0]["res_y_max"]) == (6, 7)


def test_flag_implications():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import run
    finally:
        sys.path.pop(0)
    a = run.parse_args(["--weights=seeded:l:5"])
    assert not (a.residual_map or a.save_residual_maps or a.fit_components) and a.residual_nsigma == 5.0
    a = run.parse_args(["--weights=seeded:l:5", "--residual_map"])
    assert a.residual_map and a.fit_components and a.deblend_islands and a.measure_islands and not a.fit_blends and not a.save_residual_maps
    a = run.parse_args(["--weights=seeded:l:5", "--save_residual_maps", "--residual_nsigma", "3"])
    assert a.residual_map and a.save_residual_maps and a.fit_components and a.residual_nsigma == 3.0
    a = run.parse_args(["--weights=seeded:l:5", "--residual_map", "--fit_blends"])
    assert a.residual_map and a.fit_blends and a.fit_components
    a = run.parse_args(["--weights=seeded:l:5", "--fit_blends"])
    assert not a.residual_map


def test_exports_and_field_counts():
    for name in ("cy_render_gaussians", "cy_render_kernel_ms", "cy_measure_residuals", "cy_residual_kernel_ms"):
        assert name in L.EXPORTS
    assert (L.CY_RND_FIELDS, L.CY_RND_HALF_MAX, L.CY_RES_FIELDS) == (8, 256, 12) == (RR.RND_FIELDS, RR.HALF_MAX, RR.RES_FIELDS)
    assert len(L.RND_NAMES) == L.CY_RND_FIELDS and len(L.RES_NAMES) == L.CY_RES_FIELDS
    hdr = open(os.path.join(ROOT, "include", "caesar_yolo_hip.h")).read()
    for macro, v in (("CY_RND_FIELDS", 8), ("CY_RND_HALF_MAX", 256), ("CY_RES_FIELDS", 12)):
        assert int(re.search(r"#define %s (\d+)" % macro, hdr).group(1)) == v
    lib = L.load()
    assert hasattr(lib, "cy_render_gaussians") and hasattr(lib, "cy_measure_residuals")
