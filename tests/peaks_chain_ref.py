"""The chain-level scene of the residual-peak tests, and a stand-in for HipDetector made of the numpy references of tests/ (measure_ref,
bkg_ref, island_ref, deblend_ref, fit_ref, residual_ref, peaks_ref), so that measure.Chain runs the same scene on the CPU.

Scene: 160 x 160, unit Gaussian noise from a fixed seed and two well-separated circular Gaussians of amplitude 50 and sigma 2; the
hand-made source list boxes only the first."""
import numpy as np

import bkg_ref
import deblend_ref
import fit_ref
import island_ref
import measure_ref
import peaks_ref
import residual_ref
from caesar_yolo_amd import measure

SEED, AMP, SIGMA, SIDE = 11, 50.0, 2.0, 160
BOXED, UNBOXED = (40, 40), (115, 110)
CONFIG = {"bkg_map": True, "bkg_cell": 32, "residual_map": True, "residual_peaks": True}


def scene():
    """-> (image float32 [160, 160], the source list)."""
    yy, xx = np.mgrid[0:SIDE, 0:SIDE].astype(np.float64)
    img = np.random.default_rng(SEED).standard_normal((SIDE, SIDE))
    for x0, y0 in (BOXED, UNBOXED):
        img += AMP * np.exp(-((xx - x0) ** 2 + (yy - y0) ** 2) / (2 * SIGMA ** 2))
    sources = [{"name": "S1", "x1": BOXED[0] - 12.0, "y1": BOXED[1] - 12.0, "x2": BOXED[0] + 12.0, "y2": BOXED[1] + 12.0}]
    return img.astype(np.float32), sources


def check(peak_list, sources):
    """The two statements of the chain-level test."""
    near = [p for p in peak_list if abs(p["x_peak"] - UNBOXED[0]) <= 1 and abs(p["y_peak"] - UNBOXED[1]) <= 1]
    assert near and all(p["in_source"] is None for p in near), peak_list
    assert not [p for p in peak_list if np.hypot(p["x_peak"] - BOXED[0], p["y_peak"] - BOXED[1]) <= 6.0], peak_list
    assert sources[0]["res_npeaks"] == 0 and sources[0]["res_peak_snr"] is None


class RefDetector(object):
    """The measurement methods of HipDetector on host arrays, each by the numpy reference of its kernel."""

    def measure_sources(self, img, boxes, ring=8):
        return measure_ref.measure(img, boxes, ring)[0]

    def measure_background(self, img, cell=128, k=3.0, niter=3):
        return bkg_ref.background(img, cell, k, niter)

    def expand_background(self, mesh, cell, shape, want=("bkg", "rms")):
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
        maps = measure.sample_mesh(np.asarray(mesh, np.float64)[:, :, :2], cell, xx, yy).astype(np.float32)
        return tuple(np.ascontiguousarray(maps[:, :, i]) if n in want else None for i, n in enumerate(("bkg", "rms")))

    def measure_islands(self, img, boxes, thr, conn=8):
        return island_ref.islands(img, boxes, thr, conn)[0]

    def deblend_islands(self, img, boxes, thr4, conn=8, radius=2, return_masks=False):
        return deblend_ref.deblend(img, boxes, thr4, conn, radius)[:3 if return_masks else 2]

    def fit_components(self, img, boxes, bkg, ncomp, start, masks, max_iter=64):
        return fit_ref.fit_components(img, boxes, bkg, ncomp, start, masks, max_iter)

    def render_gaussians(self, img, comp, nsigma=5.0, bkg_dev=None):
        rows, model, resid = residual_ref.render(img, comp, nsigma, bkg_dev)
        return rows, model.astype(np.float32), resid.astype(np.float32)

    def measure_residuals(self, img, model, boxes, bkg, masks):
        return residual_ref.residual_stats(img, model, boxes, bkg, masks)[0]

    def find_peaks(self, map_dev, rms_dev, k_sigma=5.0, radius=2, sign=1, cap=65536):
        rows = peaks_ref.find_peaks(map_dev, rms_dev, k_sigma, radius, sign)[0]
        return rows[:cap].copy(), len(rows)

    def __getattr__(self, name):
        if name.endswith("_kernel_ms"):
            return lambda: 0.0
        raise AttributeError(name)
