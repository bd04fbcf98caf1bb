"""Reference for the source islands (cy_measure_islands), plain numpy float64 and a queue flood fill, written from the definitions
(DESIGN.md "Source islands"), not from the kernel.

img, validity of a pixel and the box window: as tests/measure_ref.py.  Per source three float64 numbers seed_thr, merge_thr, bkg:
  candidate   valid pixel of the box window with float64(v) >= merge_thr; seed: a candidate with float64(v) >= seed_thr (a NaN
              threshold compares false: no candidate / no seed)
  component   maximal set of candidates connected through conn = 8 or 4 neighbours inside the box window
  island set  the components that hold a seed; main island: the component of the window's peak pixel (largest valid pixel,
              first in row-major order) when there is a seed
Row (FIELDS): status nseed nislands npix npix_main nborder xmin xmax ymin ymax S Sx Sy Sxx Syy Sxy S_main reserved x 3, with
dx = ix - wx0, dy = iy - wy0, w = float64(v) - bkg and the terms w, w * dx, w * dy, w * (dx * dx), w * (dy * dy), w * (dx * dy).
islands() also returns the masks (uint8, shaped like the windows: 0 / 1 island set / 2 main island) and, per row, the sums of
the absolute values of the terms of S Sx Sy Sxx Syy Sxy S_main (the scale of the summation-order bound of the GPU tests)."""
from collections import deque

import numpy as np

from measure_ref import window

FIELDS = ("status", "nseed", "nislands", "npix", "npix_main", "nborder", "xmin", "xmax", "ymin", "ymax", "S", "Sx", "Sy", "Sxx", "Syy",
          "Sxy", "S_main", "reserved0", "reserved1", "reserved2")
SUMS = (10, 11, 12, 13, 14, 15, 16)
MAX_AREA = 1 << 24                       # a window with more pixels gets status 1
NB8 = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
NB4 = ((-1, 0), (0, -1), (0, 1), (1, 0))


def box_side(lo, hi, n):
    """measure_ref.window for edges that may be infinite: an edge beyond the image is clipped to just outside it first, which
    leaves the window what it was."""
    clip = lambda v: min(max(float(v), -1.0), float(n))
    return window(clip(lo), clip(hi), n)


def label(cand, conn=8):
    """int32 labels 1, 2, ... of the connected components of the boolean array `cand` (0 elsewhere), numbered in row-major order
    of their first pixel; -> (labels, number of components)."""
    assert conn in (4, 8)
    nb = NB8 if conn == 8 else NB4
    h, w = cand.shape
    lab = np.zeros((h, w), np.int32)
    n = 0
    ys, xs = np.nonzero(cand)
    for y0, x0 in zip(ys.tolist(), xs.tolist()):
        if lab[y0, x0]:
            continue
        n += 1
        lab[y0, x0] = n
        q = deque([(y0, x0)])
        while q:
            y, x = q.popleft()
            for ddy, ddx in nb:
                yy, xx = y + ddy, x + ddx
                if 0 <= yy < h and 0 <= xx < w and cand[yy, xx] and not lab[yy, xx]:
                    lab[yy, xx] = n
                    q.append((yy, xx))
    return lab, n


def islands_one(img, box, thr, conn=8):
    MH, MW = img.shape
    x1, y1, x2, y2 = (float(v) for v in box)
    seed_thr, merge_thr, bkg = (float(v) for v in thr)
    bx0, bx1 = box_side(x1, x2, MW)
    by0, by1 = box_side(y1, y2, MH)
    row = np.zeros(len(FIELDS), np.float64)
    row[6:10] = -1.0
    mags = np.zeros(len(SUMS), np.float64)
    if bx1 < bx0 or by1 < by0:
        return row, np.zeros((0, 0), np.uint8), mags
    win = img[by0:by1 + 1, bx0:bx1 + 1]
    mask = np.zeros(win.shape, np.uint8)
    if win.size > MAX_AREA:
        row[0] = 1.0
        return row, mask, mags
    with np.errstate(invalid="ignore"):
        valid = (win != 0) & np.isfinite(win)
        v64 = win.astype(np.float64)
        cand = valid & (v64 >= merge_thr)
        seed = cand & (v64 >= seed_thr)
    row[1] = int(seed.sum())
    if row[1] == 0:
        return row, mask, mags
    lab, _ = label(cand, conn)
    seeded = np.unique(lab[seed])
    inset = np.isin(lab, seeded) & cand
    k = int(np.argmax(np.where(valid, win, -np.inf)))            # the peak pixel: first occurrence in row-major order
    py, px = divmod(k, win.shape[1])
    assert seed[py, px]
    main = lab == lab[py, px]
    mask[inset] = 1
    mask[main] = 2
    iy, ix = np.nonzero(inset)
    h, w = win.shape
    row[2], row[3], row[4] = seeded.size, iy.size, int(main.sum())
    row[5] = int(((ix == 0) | (iy == 0) | (ix == w - 1) | (iy == h - 1)).sum())
    row[6], row[7], row[8], row[9] = bx0 + ix.min(), bx0 + ix.max(), by0 + iy.min(), by0 + iy.max()
    wt = v64[iy, ix] - bkg
    dx, dy = ix.astype(np.float64), iy.astype(np.float64)
    terms = [wt, wt * dx, wt * dy, wt * (dx * dx), wt * (dy * dy), wt * (dx * dy), wt[main[iy, ix]]]
    for j, t in enumerate(terms):
        row[SUMS[j]] = t.sum()
        mags[j] = np.abs(t).sum()
    return row, mask, mags


def islands(img, boxes, thr, conn=8):
    """-> (rows [n, 20] float64, list of n uint8 masks, mags [n, 7] float64 = sum |term| of S Sx Sy Sxx Syy Sxy S_main)."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    thr = np.asarray(thr, np.float64).reshape(-1, 3)
    assert boxes.shape[0] == thr.shape[0]
    rows = np.zeros((boxes.shape[0], len(FIELDS)), np.float64)
    mags = np.zeros((boxes.shape[0], len(SUMS)), np.float64)
    masks = []
    for i in range(boxes.shape[0]):
        rows[i], m, mags[i] = islands_one(img, boxes[i], thr[i], conn)
        masks.append(m)
    return rows, masks, mags


def thresholds(meas_rows, k_seed=5.0, k_merge=2.5):
    """[n, 3] {bkg + k_seed * rms, bkg + k_merge * rms, bkg} from rows of measure_ref.measure."""
    bkg, rms = meas_rows[:, 2], meas_rows[:, 3]
    return np.stack([bkg + k_seed * rms, bkg + k_merge * rms, bkg], 1)
