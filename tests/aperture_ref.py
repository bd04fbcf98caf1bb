"""Reference for cy_aperture_sums, the definition of include/caesar_yolo_hip.h restated twice in float64:
  reference()        whole index arrays per job, with the association of the kernel's sums reproduced: window pixel i on thread
                     i mod 256, sequential per thread in increasing i, a tree with offsets 32 .. 1 over the 64 lanes of a wave, the
                     four waves in order
  reference_loops()  nested Python loops over the pixels with plain float adds in the same order
Both return [n, FIELDS] float64 rows that the device has to equal bit for bit.  The window and the status are decided as
plan_apertures decides them (window()); the median and the MAD restate the rule of cy_select.h (median_rule()): the element of rank
(n - 1) / 2 of the sorted members, and for an even n the float64 mean of it and the next one.  Identical jobs of one call are
computed once."""
import math

import numpy as np

from reduce_ref import tree_sum      # the kernel's association (caesar_yolo_amd/csrc/cy_reduce.h)

RINGS_MAX, RADIUS_MAX, HEAD, RING_FIELDS, JOBS_MAX = 8, 256, 8, 4, 1 << 20
FIELDS = HEAD + RING_FIELDS * RINGS_MAX
T, LANES = 256, 64


def side(c, r, N):
    """One side of the window: (first, last, clipped) with [ceil(c - r), floor(c + r)] clipped to [0, N - 1], or None when it holds
    no pixel of the image.  c and r are finite."""
    lo, hi = math.ceil(c - r), math.floor(c + r)            # Python integers: exact
    if hi < 0 or lo > N - 1 or lo > hi:
        return None
    return max(lo, 0), min(hi, N - 1), int(lo < 0 or hi > N - 1)


def window(cx, cy, unit, factors, MH, MW):
    """(status, x0, x1, y0, y1, clipped, r2) of one job; the window is -1 and r2 empty when it is not measured."""
    cx, cy, unit = float(cx), float(cy), float(unit)
    rK = float(factors[-1]) * unit
    if not (math.isfinite(unit) and unit > 0.0 and math.isfinite(rK) and rK <= RADIUS_MAX):
        return 1, -1, -1, -1, -1, 0, []
    sx = side(cx, rK, MW) if math.isfinite(cx) and math.isfinite(cy) else None
    sy = side(cy, rK, MH) if sx is not None else None
    if sx is None or sy is None:
        return 2, -1, -1, -1, -1, 0, []
    r = [float(f) * unit for f in factors]
    return 0, sx[0], sx[1], sy[0], sy[1], int(sx[2] or sy[2]), [x * x for x in r]


def median_rule(values):
    """Exact median of a sequence of float64 by the rule of cy_select.h; 0.0 for an empty one."""
    v = sorted(float(x) for x in values)
    n = len(v)
    if n == 0:
        return 0.0
    a = v[(n - 1) // 2]
    return a if n % 2 else (a + v[n // 2]) / 2.0


def _head(row, st, x0, x1, y0, y1, clipped):
    row[0], row[1:5], row[5] = float(st), (x0, x1, y0, y1), float(clipped)


def job_arrays(amap, rms, job, factors):
    """One row, on whole index arrays."""
    MH, MW = amap.shape
    K = len(factors)
    row = np.zeros(FIELDS, np.float64)
    st, x0, x1, y0, y1, clipped, r2 = window(job[0], job[1], job[2], factors, MH, MW)
    _head(row, st, x0, x1, y0, y1, clipped)
    if st:
        return row
    cx, cy = float(job[0]), float(job[1])
    qy, qx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    dx, dy = qx.ravel().astype(np.float64) - cx, qy.ravel().astype(np.float64) - cy
    d2 = dx * dx + dy * dy
    ring = (d2[:, None] > np.array(r2, np.float64)[None, :]).sum(axis=1)
    v32 = amap[y0:y1 + 1, x0:x1 + 1].ravel()
    valid = (v32 != 0) & np.isfinite(v32)
    with np.errstate(all="ignore"):
        v = v32.astype(np.float64)
        vv = v * v
        if rms is not None:
            r32 = rms[y0:y1 + 1, x0:x1 + 1].ravel()
            r = r32.astype(np.float64)
            var = np.where(np.isfinite(r32) & (r32 > 0), r * r, 0.0)
        else:
            var = np.zeros_like(v)
        terms = []
        for k in range(K):
            sel = valid & (ring == k)
            terms += [np.where(sel, v, 0.0), np.where(sel, vv, 0.0), np.where(sel, var, 0.0)]
            row[HEAD + RING_FIELDS * k] = float(sel.sum())
    sums = tree_sum(np.stack(terms))
    for k in range(K):
        row[HEAD + RING_FIELDS * k + 1:HEAD + RING_FIELDS * k + 4] = sums[3 * k:3 * k + 3]
    ann = v[valid & (ring == K - 1)]
    row[6] = median_rule(ann)
    row[7] = median_rule(np.abs(ann - row[6]))
    return row


def job_loops(amap, rms, job, factors):
    """One row, pixel by pixel."""
    MH, MW = amap.shape
    K = len(factors)
    row = np.zeros(FIELDS, np.float64)
    st, x0, x1, y0, y1, clipped, r2 = window(job[0], job[1], job[2], factors, MH, MW)
    _head(row, st, x0, x1, y0, y1, clipped)
    if st:
        return row
    cx, cy = float(job[0]), float(job[1])
    W = x1 - x0 + 1
    acc = [[[0.0, 0.0, 0.0] for _ in range(K)] for _ in range(T)]
    cnt = [0] * K
    ann = []
    vals = amap[y0:y1 + 1, x0:x1 + 1].tolist()
    noise = rms[y0:y1 + 1, x0:x1 + 1].tolist() if rms is not None else None
    for wy in range(y1 - y0 + 1):
        dy = float(y0 + wy) - cy
        yy = dy * dy
        for wx in range(W):
            dx = float(x0 + wx) - cx
            d2 = dx * dx + yy
            k = 0
            while k < K and d2 > r2[k]:
                k += 1
            v = vals[wy][wx]                                  # a float32 value as a Python float: exact
            if k == K or v == 0.0 or not math.isfinite(v):
                continue
            a = acc[(wy * W + wx) % T][k]
            a[0] = a[0] + v
            a[1] = a[1] + v * v
            if noise is not None:
                r = noise[wy][wx]
                if math.isfinite(r) and r > 0.0:
                    a[2] = a[2] + r * r
            cnt[k] += 1
            if k == K - 1:
                ann.append(v)
    for k in range(K):
        f = HEAD + RING_FIELDS * k
        row[f] = float(cnt[k])
        for j in range(3):
            total = None
            for w in range(T // LANES):
                lanes = [acc[w * LANES + l][k][j] for l in range(LANES)]
                for o in (32, 16, 8, 4, 2, 1):
                    for l in range(o):
                        lanes[l] = lanes[l] + lanes[l + o]
                total = lanes[0] if total is None else total + lanes[0]
            row[f + 1 + j] = total
    med = median_rule(ann)
    row[6], row[7] = med, median_rule([abs(v - med) for v in ann])
    return row


def _rows(one, amap, rms, jobs, factors):
    amap = np.ascontiguousarray(amap, np.float32)
    rms = None if rms is None else np.ascontiguousarray(rms, np.float32)
    jobs = np.asarray(jobs, np.float64).reshape(-1, 3)
    factors = [float(f) for f in factors]
    assert 1 <= len(factors) <= RINGS_MAX and amap.ndim == 2 and (rms is None or rms.shape == amap.shape)
    out, seen = np.zeros((jobs.shape[0], FIELDS), np.float64), {}
    for i, job in enumerate(jobs):
        key = job.tobytes()
        if key not in seen:
            seen[key] = one(amap, rms, job, factors)
        out[i] = seen[key]
    return out


def reference(amap, rms, jobs, factors):
    return _rows(job_arrays, amap, rms, jobs, factors)


def reference_loops(amap, rms, jobs, factors):
    return _rows(job_loops, amap, rms, jobs, factors)
