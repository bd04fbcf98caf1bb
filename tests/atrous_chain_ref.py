"""The chain-level scene of the residual-scale tests, and the stand-in detector of tests/peaks_chain_ref.py extended by the numpy
restatement of cy_atrous_step (tests/atrous_ref.py), so that measure.Chain runs the same scene on the CPU.

Scene: 256 x 256, unit Gaussian noise from a fixed seed, stored fp32; one bright compact Gaussian (amplitude 50, sigma 2) with a box,
which keeps the detect-side chain non-empty; two unboxed blobs of peak 1.5 and sigma 9 px at (x, y) = (90, 100) and (180, 170): faint
per pixel (1.5 rms at most), many pixels wide."""
import numpy as np

import atrous_ref
import peaks_chain_ref as CR
import peaks_ref
from caesar_yolo_amd import measure

SEED, SIDE = 2, 256
COMPACT, AMP, SIGMA = (40, 200), 50.0, 2.0
BLOBS, BLOB_PEAK, BLOB_SIGMA = ((90, 100), (180, 170)), 1.5, 9.0
CONFIG = {"bkg_map": True, "bkg_cell": 32, "residual_map": True, "residual_peaks": True, "residual_peaks_sigma": 5.0,
          "residual_scales": 5, "residual_scale_first": 2, "residual_scales_sigma": 5.0, "save_scale_maps": True}


def scene():
    """-> (image float32 [256, 256], the source list)."""
    yy, xx = np.mgrid[0:SIDE, 0:SIDE].astype(np.float64)
    img = np.random.default_rng(SEED).standard_normal((SIDE, SIDE))
    img += AMP * np.exp(-((xx - COMPACT[0]) ** 2 + (yy - COMPACT[1]) ** 2) / (2 * SIGMA ** 2))
    for x0, y0 in BLOBS:
        img += BLOB_PEAK * np.exp(-((xx - x0) ** 2 + (yy - y0) ** 2) / (2 * BLOB_SIGMA ** 2))
    sources = [{"name": "S1", "x1": COMPACT[0] - 12.0, "y1": COMPACT[1] - 12.0, "x2": COMPACT[0] + 12.0, "y2": COMPACT[1] + 12.0}]
    return img.astype(np.float32), sources


def check(peak_list, scale_list):
    """The two statements of the chain-level tests."""
    for x0, y0 in BLOBS:
        # 1. the pixel search at 5 sigma lists nothing within 20 px of the blob
        assert not [p for p in peak_list if np.hypot(p["x_peak"] - x0, p["y_peak"] - y0) <= 20.0], peak_list
        # 2. exactly one strongest entry within 4 px of its centre, at scale 4 or 5, in no source
        near = [p for p in scale_list if p["strongest"] and np.hypot(p["x_peak"] - x0, p["y_peak"] - y0) <= 4.0]
        assert len(near) == 1 and near[0]["scale"] in (4, 5) and near[0]["in_source"] is None, (x0, y0, near)


class RefDetector(CR.RefDetector):
    """peaks_chain_ref.RefDetector plus atrous_step by its numpy restatement (new arrays: `out` is a place to write, not a promise)."""

    def atrous_step(self, in_dev, step, want=("smooth", "detail"), out=(None, None)):
        smooth, detail = atrous_ref.atrous_step(in_dev, step)
        return (smooth if "smooth" in want else None), (detail if "detail" in want else None)

    def find_peaks(self, map_dev, rms_dev, k_sigma=5.0, radius=2, sign=1, cap=65536):
        rows, absum = peaks_ref.find_peaks(map_dev, rms_dev, k_sigma, radius, sign)
        self.absums = getattr(self, "absums", []) + [absum]    # per call: sum |t| of the four sums of every row (peaks_ref.sum_bound)
        return rows[:cap].copy(), len(rows)


def run(det, img, sources, config=CONFIG):
    """The chain of the scene on `det` -> (chain, stats)."""
    stats = {}
    return measure.Chain(det, img, sources, config).run(measure.plan(config), stats), stats
