"""Reference for cy_disc_residuals, the definition of include/caesar_yolo_hip.h restated in numpy float64, twice:
  disc_residuals()        on whole index arrays, with the planner (peakfit_ref.plan) and the pixel set (peakfit_ref.members) of the
                          peak fits: the pixel set of a job is the one its single fit uses
  disc_residuals_loops()  the same definition as nested Python loops over the jobs, their neighbours and the pixels of the window,
                          with nothing shared with the first but the planner's window (peakfit_ref.window)
Both return (rows [n, FIELDS], ab [n, 3]): ab holds, per sum (sum r, sum r * r, model_sum), the sum of |terms| that the bound of the
GPU test needs.  Sums are plain sequential sums in window-index order; the kernel's association differs, and compare() allows for
it by the derived bound of residual_ref.compare_stats: both sides add the same float64 terms in some order.
  render_signed()         the reference of cy_render_signed_gaussians on top of residual_ref
"""
import math

import numpy as np

import peakfit_ref as PR
import residual_ref as RR

FIELDS = 16
NAMES = ("status", "npix", "nexcluded", "sum", "sumsq", "maxabs", "x_max", "y_max", "model_sum", "reserved", "wx0", "wx1", "wy0", "wy1",
         "clipped", "nneigh")
EXACT = [0, 1, 2, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15]       # status, the counts, maxabs (one rounded subtraction) with its position, the reserved field, the window, clipped, nneigh
SUMS = ((3, 0), (4, 1), (8, 2))                             # (field, column of ab)


def render_signed(img, comp, nsigma, bkg=None):
    """Reference for cy_render_signed_gaussians: residual_ref.render with amplitudes of either sign.  A component is admissible with
    A != 0 in place of A > 0, so its status and rectangle are those residual_ref.rectangles gives for |A| (A == 0: status 1); the
    model adds A * exp(..) with the sign in the same order.  -> (rows [m, 8], model float64, resid float64)."""
    img = np.asarray(img, np.float32)
    comp = np.asarray(comp, np.float64).reshape(-1, 6)
    MH, MW = img.shape
    mag = comp.copy()
    mag[:, 0] = np.abs(mag[:, 0])
    rows = RR.rectangles(mag, nsigma, MH, MW)
    model = RR.model_map(comp, rows, MH, MW)
    ok = RR.valid(img)
    b = np.zeros((MH, MW), np.float64) if bkg is None else np.asarray(bkg, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        resid = np.where(ok, (np.where(ok, img, 0).astype(np.float64) - b) - model, 0.0)
    return rows, model, resid


def _turned_away(status):
    row = np.zeros(FIELDS, np.float64)
    row[0] = status
    row[[6, 7, 10, 11, 12, 13]] = -1.0
    return row


def disc_residuals(amap, model, jobs):
    """The whole call on host maps (float32; model may be None).  -> (rows [n, FIELDS], ab [n, 3])."""
    amap = np.ascontiguousarray(amap, np.float32)
    jobs = np.asarray(jobs, np.float64).reshape(-1, PR.JOB_FIELDS)
    MH, MW = amap.shape
    n = jobs.shape[0]
    win, neigh, _ = PR.plan(jobs, MH, MW)
    out, ab = np.zeros((n, FIELDS), np.float64), np.zeros((n, 3), np.float64)
    for e in range(n):
        st, x0, x1, y0, y1, clipped = (int(v) for v in win[e])
        if st:
            out[e] = _turned_away(st)
            continue
        mine, inside, dx, _ = PR.members(jobs[e], (x0, x1, y0, y1), [(jobs[f, 0], jobs[f, 1]) for f in neigh[e]])
        v = amap[y0:y1 + 1, x0:x1 + 1].ravel()
        valid = (v != 0) & np.isfinite(v)
        ok = mine & valid
        with np.errstate(all="ignore"):
            r = np.where(ok, v, 0).astype(np.float64) - float(jobs[e, 3])
        r = r[ok]
        md = np.zeros(0) if model is None else np.asarray(model, np.float32)[y0:y1 + 1, x0:x1 + 1].ravel()[ok].astype(np.float64)
        row = np.zeros(FIELDS, np.float64)
        row[1], row[2] = ok.sum(), (inside & ~mine & valid).sum()
        row[3], row[4], row[8] = np.sum(r), np.sum(r * r), np.sum(md)
        row[6:8] = -1.0
        if r.size:
            j = int(np.argmax(np.abs(r)))                     # the first maximum in window-index order
            q = int(np.nonzero(ok)[0][j])
            W = x1 - x0 + 1
            row[5], row[6], row[7] = abs(r[j]), x0 + q % W, y0 + q // W
        row[10:16] = [x0, x1, y0, y1, clipped, len(neigh[e])]
        out[e] = row
        ab[e] = [np.sum(np.abs(r)), np.sum(r * r), np.sum(np.abs(md))]
    return out, ab


def disc_residuals_loops(amap, model, jobs):
    """The same call, pixel by pixel.  -> (rows [n, FIELDS], ab [n, 3])."""
    amap = np.ascontiguousarray(amap, np.float32)
    model = None if model is None else np.ascontiguousarray(model, np.float32)
    jobs = np.asarray(jobs, np.float64).reshape(-1, PR.JOB_FIELDS)
    MH, MW = amap.shape
    n = jobs.shape[0]
    wins = [PR.window(j[0], j[1], j[2], j[3], j[4], MH, MW) for j in jobs]
    out, ab = np.zeros((n, FIELDS), np.float64), np.zeros((n, 3), np.float64)
    for e in range(n):
        st, x0, x1, y0, y1, clipped = wins[e]
        if st:
            out[e] = _turned_away(st)
            continue
        cx, cy, R, bkg = (float(v) for v in jobs[e, :4])
        cand = []
        for f in range(n):
            if f == e or wins[f][0]:
                continue
            ddx, ddy = float(jobs[f, 0]) - cx, float(jobs[f, 1]) - cy
            D2 = ddx * ddx + ddy * ddy
            if D2 < 4.0 * (R * R):
                cand.append((D2, f))
        cand.sort()
        kept = [f for _, f in cand[:PR.NEIGH_MAX]]
        npix = nex = 0
        s = ss = ms = a0 = a2 = 0.0
        best, bx, by = 0.0, -1, -1
        for qy in range(y0, y1 + 1):
            for qx in range(x0, x1 + 1):
                ex, ey = float(qx) - cx, float(qy) - cy
                d2 = ex * ex + ey * ey
                if not d2 <= R * R:
                    continue
                v = amap[qy, qx]
                if v == 0 or not math.isfinite(float(v)):
                    continue
                mine = True
                for f in kept:
                    fx, fy = float(qx) - float(jobs[f, 0]), float(qy) - float(jobs[f, 1])
                    if not fx * fx + fy * fy >= d2:
                        mine = False
                if not mine:
                    nex += 1
                    continue
                r = float(v) - bkg
                npix += 1
                s += r
                ss += r * r
                a0 += abs(r)
                if model is not None:
                    ms += float(model[qy, qx])
                    a2 += abs(float(model[qy, qx]))
                if bx < 0 or abs(r) > best:
                    best, bx, by = abs(r), qx, qy
        out[e] = [0, npix, nex, s, ss, best, bx, by, ms, 0, x0, x1, y0, y1, clipped, len(kept)]
        ab[e] = [a0, ss, a2]
    return out, ab


def compare(got, ref, ab, names=None):
    """The rule of the GPU tests for rows of cy_disc_residuals against disc_residuals(): the fields of EXACT equal; the three sums
    within 2 npix 2^-53 sum|t_i| of the reference (both sides add the same float64 terms in some order)."""
    got, ref = np.asarray(got, np.float64).reshape(-1, FIELDS), np.asarray(ref, np.float64).reshape(-1, FIELDS)
    assert got.shape == ref.shape
    for i in range(ref.shape[0]):
        nm = names[i] if names is not None else "job %d" % i
        g, r = got[i], ref[i]
        assert np.array_equal(g[EXACT], r[EXACT]), "%s: %s, reference %s" % (nm, g, r)
        for f, t in SUMS:
            bound = 2.0 * r[1] * 2.0 ** -53 * ab[i, t]
            print("%s: field %d got %r reference %r bound %g" % (nm, f, g[f], r[f], bound))
            assert abs(g[f] - r[f]) <= bound, "%s: field %d %r, reference %r, bound %g" % (nm, f, g[f], r[f], bound)
