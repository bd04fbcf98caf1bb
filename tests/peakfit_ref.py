"""Reference for cy_fit_peaks, the definition of include/caesar_yolo_hip.h restated in numpy float64 on top of fit_ref.fit_one.
  window()      the planner's status, window and clipped flag of one job with Python integers (math.ceil / math.floor are exact), as
                aperture_ref.window does it
  plan()        the planner's table of one call: statuses, windows, and the neighbour lists in (D2, job index) order
  members()     the pixel set of one job over its whole window: the disc test and the nearest-centre test against the kept neighbours
  fit_peaks()   the whole call on a host map -> [n, FIELDS] rows.  The job's list is every pixel of the window in increasing window
                index with ok = member & valid, so fit_ref's "tree" summation is the kernel's association
The summation variants and the exp nudge are those of fit_ref.VARIANTS.

TOL: over every job of tests/peakfit_cases.py (the drawn cases and the random scene) on which all variants end with status 0, the
largest per-parameter difference |dp_j| / (|p_j| + 1e-3) between any two variants was measured (MEASURED below;
tests/test_peakfit_cpu.py recomputes it and fails when it no longer matches).  The flat patch is not in it: there is no Gaussian in
it, its a, b, c run towards 0, the variants end 13 % apart, and it is compared on status and npix alone.  TOL is 16 times that, the project's margin for a
device exp that differs by more than the nudge and whose difference compounds over the iterations.  It is measured between the
variants of this reference, never against the kernel."""
import math

import numpy as np

import fit_ref as FR
from aperture_ref import side

JOB_FIELDS, FIELDS, RADIUS_MAX, NEIGH_MAX, JOBS_MAX, LDS_MAX = 11, 40, 256, 8, 1 << 20, 8192
JOB_NAMES = ("cx", "cy", "R", "bkg", "sign", "A", "x0", "y0", "a", "b", "c")
NAMES = FR.FIELDS + ("wx0", "wx1", "wy0", "wy1", "clipped", "nneigh", "crowded", "nexcluded")
VARIANTS = FR.VARIANTS
MEASURED = 1.65e-7      # measured 1.64e-7, on the random scene of seed 1 (the drawn jobs that are compared with TOL stay below 1e-12)
TOL = 16 * MEASURED


def window(cx, cy, R, bkg, sign, MH, MW):
    """(status, x0, x1, y0, y1, clipped) of one job by the planner's rules; the window is -1 when the job is not fitted."""
    cx, cy, R, bkg, sign = float(cx), float(cy), float(R), float(bkg), float(sign)
    if not (math.isfinite(R) and 0.0 < R <= RADIUS_MAX and sign in (1.0, -1.0) and math.isfinite(bkg)):
        return 1, -1, -1, -1, -1, 0
    sx = side(cx, R, MW) if math.isfinite(cx) and math.isfinite(cy) else None
    sy = side(cy, R, MH) if sx is not None else None
    if sx is None or sy is None:
        return 5, -1, -1, -1, -1, 0
    return 0, sx[0], sx[1], sy[0], sy[1], int(sx[2] or sy[2])


def neighbours(cx, cy, R, fitted, e):
    """(kept job indices in (D2, index) order, count) for job e: the other fitted jobs with D2 < 4 (R_e R_e).  cx, cy, R: float64
    arrays over the jobs; fitted: boolean."""
    with np.errstate(all="ignore"):
        dx, dy = cx - cx[e], cy - cy[e]
        D2 = dx * dx + dy * dy
        hit = fitted & (D2 < 4.0 * (R[e] * R[e]))
    hit[e] = False
    idx = np.nonzero(hit)[0]
    idx = idx[np.lexsort((idx, D2[idx]))]
    return [int(i) for i in idx[:NEIGH_MAX]], int(idx.size)


def plan(jobs, MH, MW, only=None):
    """-> (win [n, 6] int64 {status, x0, x1, y0, y1, clipped}, neigh: list of kept index lists, count [n]).  only: the jobs whose
    neighbours are wanted (None: all); the others get an empty list and count -1."""
    jobs = np.asarray(jobs, np.float64).reshape(-1, JOB_FIELDS)
    n = jobs.shape[0]
    win = np.array([window(j[0], j[1], j[2], j[3], j[4], MH, MW) for j in jobs], np.int64).reshape(n, 6)
    fitted = win[:, 0] == 0
    cx, cy, R = jobs[:, 0].copy(), jobs[:, 1].copy(), jobs[:, 2].copy()
    neigh, count = [[] for _ in range(n)], np.full(n, -1, np.int64)
    for e in (range(n) if only is None else only):
        count[e] = 0
        if fitted[e]:
            neigh[e], count[e] = neighbours(cx, cy, R, fitted, e)
    return win, neigh, count


def members(job, w, centres):
    """(member, in_disc, qx - x0, qy - y0) over the window w = (x0, x1, y0, y1) in increasing window index; centres: the kept
    neighbours' (cx, cy)."""
    x0, x1, y0, y1 = (int(v) for v in w)
    qy, qx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    qx, qy = qx.ravel().astype(np.float64), qy.ravel().astype(np.float64)
    ex, ey = qx - float(job[0]), qy - float(job[1])
    d2 = ex * ex + ey * ey
    R = float(job[2])
    inside = d2 <= R * R
    mine = inside.copy()
    for fx, fy in centres:
        gx, gy = qx - float(fx), qy - float(fy)
        mine &= gx * gx + gy * gy >= d2
    return mine, inside, qx - float(x0), qy - float(y0)


def fit_peaks(amap, jobs, max_iter=64, summ="tree", nudge=None, only=None):
    """The whole call on a host map (float32; a pixel is valid when it is non-zero and finite).  -> [n, FIELDS] float64.  only: the
    jobs to compute (the others' rows stay 0); the neighbours are those of the whole table either way."""
    amap = np.ascontiguousarray(amap, np.float32)
    jobs = np.asarray(jobs, np.float64).reshape(-1, JOB_FIELDS)
    MH, MW = amap.shape
    n = jobs.shape[0]
    win, neigh, count = plan(jobs, MH, MW, only)
    out = np.zeros((n, FIELDS), np.float64)
    for e in (range(n) if only is None else only):
        st, x0, x1, y0, y1, clipped = (int(v) for v in win[e])
        job = jobs[e]
        if st:
            out[e, 0], out[e, 32:36] = st, -1.0
            continue
        mine, inside, dx, dy = members(job, (x0, x1, y0, y1), [(jobs[f, 0], jobs[f, 1]) for f in neigh[e]])
        v = amap[y0:y1 + 1, x0:x1 + 1].ravel()
        valid = (v != 0) & np.isfinite(v)
        ok = mine & valid
        y = float(job[4]) * (np.where(valid, v.astype(np.float64), 0.0) - float(job[3]))
        p0 = job[5:11].copy()
        p0[1] -= float(x0)
        p0[2] -= float(y0)
        s, it, npix, F, lam, p, H = FR.fit_one(p0, dx, dy, y, ok, max_iter, summ, None if nudge is None else nudge + e)
        p = list(job[5:11]) if s in (3, 4) else [p[0], p[1] + float(x0), p[2] + float(y0)] + list(p[3:])
        out[e] = [s, it, npix, F, lam] + p + list(H) + [x0, x1, y0, y1, clipped, len(neigh[e]), int(count[e] > NEIGH_MAX), int((inside & ~mine & valid).sum())]
    return out


def fit_variants(amap, jobs, max_iter=64, only=None):
    """The call under every entry of VARIANTS: list of [n, FIELDS] arrays."""
    return [fit_peaks(amap, jobs, max_iter, s, g, only) for s, g in VARIANTS]


def spread(results, rows=None):
    """(largest |dp_j| / (|p_j| + 1e-3) between any two results over the jobs on which all have status 0, boolean [n] of those
    jobs, boolean [n] of the jobs on which the results disagree on status).  rows: the jobs that count (None: all)."""
    n = results[0].shape[0]
    use = np.ones(n, bool) if rows is None else np.isin(np.arange(n), rows)
    all0, differ = use.copy(), np.zeros(n, bool)
    for r in results:
        all0 &= r[:, 0] == 0
        differ |= use & (r[:, 0] != results[0][:, 0])
    worst = 0.0
    for a in range(len(results)):
        for b in range(a + 1, len(results)):
            pa, pb = results[a][all0, 5:11], results[b][all0, 5:11]
            if pa.size:
                worst = max(worst, float(np.max(np.abs(pa - pb) / (np.abs(pa) + 1e-3))))
    return worst, all0, differ


def cond_H(row):
    return FR.cond_H(row[:32])
