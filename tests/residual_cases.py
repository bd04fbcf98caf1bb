"""Inputs of the model / residual tests, shared by the CPU tests (tests/test_residual_cpu.py, tests/test_render_plan_cpu.py) and the
GPU test (tests/test_gpu_residual.py), all on small images:
  A      70 rows x 75 columns: MW % 4 != 0 (the pixel-by-pixel path), partial tiles on both edges
  B      64 rows x 96 columns: the 16-byte path
  C      300 x 300, for the capped half-widths
  S      384 rows x 512 columns, the random scene of 600 admissible components; the statistics cases live on it
Every image is noise around 0.5 with a few NaN, +inf and zero pixels under the first components.  render_cases() lists the render
calls; reference() computes tests/residual_ref.py on each of them once and is shared, read-only."""
import functools
import math

import numpy as np

import residual_ref

NAN, INF = float("nan"), float("inf")


def gauss_params(A, x0, y0, smaj, smin, theta_deg):
    """{A, x0, y0, a, b, c} of a Gaussian with the given sigmas along its axes, the major axis theta from +x towards +y."""
    t = math.radians(theta_deg)
    cs, sn = math.cos(t), math.sin(t)
    ia, ib = 1.0 / (smaj * smaj), 1.0 / (smin * smin)
    return [A, x0, y0, cs * cs * ia + sn * sn * ib, cs * sn * (ia - ib), sn * sn * ia + cs * cs * ib]


def _image(MH, MW, seed):
    rng = np.random.default_rng(seed)
    img = (0.5 + 0.05 * rng.standard_normal((MH, MW))).astype(np.float32)
    img[12, 10] = NAN
    img[13, 11] = NAN
    img[14, 10] = 0.0
    img[15, 20] = INF
    img[16, 21] = -0.75                                       # valid: negative and non-zero
    return img


@functools.lru_cache(maxsize=None)
def images():
    return {"A": _image(70, 75, 1), "B": _image(64, 96, 2), "C": _image(300, 300, 3), "S": scene()[0]}


@functools.lru_cache(maxsize=None)
def backgrounds():
    """A smooth fp32 background map per image."""
    out = {}
    for k, img in images().items():
        MH, MW = img.shape
        y, x = np.mgrid[0:MH, 0:MW]
        out[k] = (0.45 + 0.0004 * x + 0.0003 * y).astype(np.float32)
    return out


def grid_components(n):
    """n small Gaussians whose rectangles (nsigma 5, sigma 1.5: half-width 8) all contain pixel (16, 16) of tile (0, 0)."""
    out = []
    for k in range(n):
        out.append(gauss_params(1.0 + 0.01 * k, 10.0 + (k % 12) * 1.05 + 0.013 * k, 10.0 + (k // 12) * 1.1, 1.5, 1.5, 0.0))
    return np.array(out, np.float64)


@functools.lru_cache(maxsize=None)
def scene():
    """-> (image S with the components drawn into it, comp [600, 6]).  Centres stay left of column 440, so that the columns from
    460 on carry no model at all."""
    rng = np.random.default_rng(77)
    MH, MW = 384, 512
    comp = np.array([gauss_params(rng.uniform(0.2, 30.0), rng.uniform(-4.0, 440.0), rng.uniform(-4.0, MH + 3.0), rng.uniform(1.2, 3.0),
                                  rng.uniform(0.8, 1.2), rng.uniform(-90.0, 90.0)) for _ in range(600)], np.float64)
    img = _image(MH, MW, 4).astype(np.float64)
    rows = residual_ref.rectangles(comp, 5.0, MH, MW)
    img = (img + residual_ref.model_map(comp, rows, MH, MW)).astype(np.float32)
    img[10:21, 462:476] = 0.0                                 # an all-blank window
    img[30:51, 480:501] = 0.5
    img[33, 497] = 50.0                                       # the largest |r| twice, where the model is 0: (497, 33) comes first
    img[41, 483] = 50.0
    return img, comp


def render_cases():
    """[(name, image key, comp [m, 6], nsigma, with bkg, want)]"""
    two = np.array([gauss_params(8.0, 10.3, 12.7, 2.0, 2.0, 0.0), gauss_params(5.0, 20.5, 15.2, 2.5, 1.2, 30.0)])
    bad = np.array([[NAN, 10, 10, 1, 0, 1], [3, INF, 10, 1, 0, 1], [0.0, 10, 10, 1, 0, 1], [-2.0, 10, 10, 1, 0, 1], [3, 10, 10, 1, 2, 1],
                    [3, 10, 10, 1, 1, 1], [3, 10, 10, -1, 0, -1], [3, 10, 10, 0, 0, 1], gauss_params(4.0, 40.2, 33.3, 1.5, 1.5, 0.0)], np.float64)
    out = []
    for key in ("A", "B"):
        out += [("two_one_tile_" + key, key, two, 5.0, True, ("model", "resid")),
                ("two_no_bkg_" + key, key, two, 5.0, False, ("model", "resid")),
                ("two_model_only_" + key, key, two, 5.0, True, ("model",)),
                ("two_resid_only_" + key, key, two, 5.0, False, ("resid",)),
                ("nsigma1_" + key, key, two, 1.0, True, ("model", "resid")),
                ("nsigma8_" + key, key, two, 8.0, True, ("model", "resid")),
                ("corner4_" + key, key, np.array([gauss_params(6.0, 31.5, 31.5, 2.2, 1.4, -50.0)]), 5.0, True, ("model", "resid")),
                ("reaching_in_" + key, key, np.array([gauss_params(6.0, -3.2, 20.0, 2.0, 2.0, 0.0), gauss_params(4.0, 30.0, -2.6, 1.5, 1.0, 20.0),
                                                      gauss_params(4.0, 200.0, 40.0, 50.0, 50.0, 0.0)]), 5.0, True, ("model", "resid")),
                ("outside_" + key, key, np.array([gauss_params(6.0, -50.0, 20.0, 2.0, 2.0, 0.0), gauss_params(6.0, 20.0, 1e300, 2.0, 2.0, 0.0),
                                                  gauss_params(6.0, -1e300, -1e300, 2.0, 2.0, 0.0), gauss_params(2.0, 50.0, 50.0, 2.0, 2.0, 0.0)]),
                 5.0, False, ("model", "resid")),
                ("not_admissible_" + key, key, bad, 5.0, True, ("model", "resid")),
                ("m0_" + key, key, np.zeros((0, 6)), 5.0, True, ("model", "resid")),
                ("m0_no_bkg_" + key, key, np.zeros((0, 6)), 5.0, False, ("model", "resid"))]
        for n in (64, 65, 130):
            out.append(("chunk%d_%s" % (n, key), key, grid_components(n), 5.0, True, ("model", "resid")))
    out.append(("sigma1000", "C", np.array([[2.0, 150.3, 149.6, 1e-6, 0.0, 1e-6], [1.0, 10.0, 290.0, 1e-160, 0.0, 1e-160],
                                            gauss_params(3.0, 100.0, 100.0, 1000.0, 2.0, 0.0)]), 5.0, True, ("model", "resid")))
    out.append(("scene600", "S", scene()[1], 5.0, True, ("model", "resid")))
    return out


@functools.lru_cache(maxsize=None)
def reference():
    """name -> (rows, model float64, resid float64) of residual_ref.render on every render case."""
    imgs, bkgs = images(), backgrounds()
    return {name: residual_ref.render(imgs[key], comp, nsigma, bkgs[key] if with_bkg else None)
            for name, key, comp, nsigma, with_bkg, _ in render_cases()}


def stats_case():
    """The statistics inputs on image S: (boxes [n, 4], bkg [n], masks, names)."""
    img = scene()[0]
    MH, MW = img.shape
    rng = np.random.default_rng(5)
    names = ["corner_top_left", "corner_bottom_right", "empty", "blank", "bytes", "max_twice", "px4096", "px4097", "nan_under"]
    boxes = np.array([[-5.0, -5.0, 10.5, 8.2], [MW - 12.5, MH - 9.0, MW + 30.0, MH + 30.0], [10.2, 5.0, 10.8, 30.0], [462.0, 10.0, 475.0, 20.0],
                      [100.0, 100.0, 140.0, 130.0], [480.0, 30.0, 500.0, 50.0], [20.0, 30.0, 83.0, 93.0], [40.0, 200.0, 280.0, 216.0],
                      [5.0, 8.0, 25.0, 20.0]], np.float64)
    bkg = np.array([0.5, 0.48, 0.5, 0.5, 0.51, 0.25, 0.5, 0.5, 0.5])
    masks = []
    from caesar_yolo_amd.measure import box_window
    for i, b in enumerate(boxes):
        _, _, h, w = box_window(b, MH, MW)
        if names[i] == "bytes":
            m = rng.choice(np.array([0, 1, 2, 3, 16, 255], np.uint8), (h, w))
        elif names[i] == "max_twice":
            m = np.ones((h, w), np.uint8)
        else:
            m = (rng.random((h, w)) < 0.6).astype(np.uint8) * (1 + i % 3)
        masks.append(m)
    assert masks[6].size == 4096 and masks[7].size == 4097
    return boxes, bkg, masks, names
