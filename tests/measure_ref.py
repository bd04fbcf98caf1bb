"""Reference for the catalog source measurement (cy_measure_sources), plain numpy float64, written from the definitions
(DESIGN.md "Source measurement"), not from the kernel.

img: 2-D float32 image as cy_mosaic_prepare leaves it (blank = 0).  A pixel is valid when it is != 0 and finite.
Box (x1, y1, x2, y2), float64, 0-based pixels with a pixel's centre at its index:
  box window  ix in [max(0, ceil(x1)), min(MW - 1, floor(x2))], iy likewise with MH; may be empty
  ring        box window grown by `ring` pixels on each side, clipped to the image, minus the box window; an empty box window
              has no pixels to grow from, so no ring
Row: npix nring bkg rms peak x_peak y_peak sum sw swx swy reserved (FIELDS).  measure() also returns, per row, the sums of the
absolute values of the terms of sum / sw / swx / swy (the scale of the summation-order bound of the GPU tests)."""
import math

import numpy as np

FIELDS = ("npix", "nring", "bkg", "rms", "peak", "x_peak", "y_peak", "sum", "sw", "swx", "swy", "reserved")


def window(lo, hi, n):
    """Inclusive integer range [first, last] of one box side; first > last when it is empty."""
    return max(0, math.ceil(lo)), min(n - 1, math.floor(hi))


def measure_one(img, box, ring):
    MH, MW = img.shape
    x1, y1, x2, y2 = (float(v) for v in box)
    bx0, bx1 = window(x1, x2, MW)
    by0, by1 = window(y1, y2, MH)
    row = np.zeros(len(FIELDS), np.float64)
    row[5] = row[6] = -1.0
    mags = np.zeros(4, np.float64)
    if bx1 < bx0 or by1 < by0:
        return row, mags
    gx0, gx1 = max(0, bx0 - ring), min(MW - 1, bx1 + ring)
    gy0, gy1 = max(0, by0 - ring), min(MH - 1, by1 + ring)
    grown = img[gy0:gy1 + 1, gx0:gx1 + 1]
    in_ring = np.ones(grown.shape, bool)
    in_ring[by0 - gy0:by1 - gy0 + 1, bx0 - gx0:bx1 - gx0 + 1] = False
    with np.errstate(invalid="ignore"):
        rv = grown[in_ring & (grown != 0) & np.isfinite(grown)].astype(np.float64)
    bkg = rms = 0.0
    if rv.size:
        bkg = float(np.median(rv))
        rms = 1.4826 * float(np.median(np.abs(rv - bkg)))
    row[1], row[2], row[3] = rv.size, bkg, rms
    win = img[by0:by1 + 1, bx0:bx1 + 1]
    with np.errstate(invalid="ignore"):
        valid = (win != 0) & np.isfinite(win)
    row[0] = int(valid.sum())
    if row[0] == 0:
        return row, mags
    k = int(np.argmax(np.where(valid, win, -np.inf)))            # first occurrence in row-major order
    py, px = divmod(k, win.shape[1])
    row[4], row[5], row[6] = float(win[py, px]), bx0 + px, by0 + py
    iy, ix = np.nonzero(valid)
    d = win[iy, ix].astype(np.float64) - bkg
    w = np.where(d > 0, d, 0.0)
    tx, ty = w * (ix + bx0).astype(np.float64), w * (iy + by0).astype(np.float64)
    row[7], row[8], row[9], row[10] = d.sum(), w.sum(), tx.sum(), ty.sum()
    mags[:] = np.abs(d).sum(), w.sum(), np.abs(tx).sum(), np.abs(ty).sum()
    return row, mags


def measure(img, boxes, ring=8):
    """-> (rows [n, 12] float64, mags [n, 4] float64 = sum |term| of sum / sw / swx / swy)."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    rows = np.zeros((boxes.shape[0], len(FIELDS)), np.float64)
    mags = np.zeros((boxes.shape[0], 4), np.float64)
    for i, b in enumerate(boxes):
        rows[i], mags[i] = measure_one(img, b, int(ring))
    return rows, mags
