"""Reference for the component fits (cy_fit_components), the algorithm of include/caesar_yolo_hip.h restated in numpy float64: the
same model, the same expressions and roundings per pixel, the same Cholesky (row by row, inner sums subtracted term by term), the
same accept / reject rules and constants.  Two parts are switchable, because the device differs from any host restatement in
exactly these two:
  summ    how the 28 sums of a sweep are added: "np" (np.sum, pairwise), "fsum" (math.fsum, exactly rounded) or "tree" (the
          kernel's association: list entry q on thread q mod 256, sequential per thread, shuffle tree per wave of 64, the four
          waves in order)
  nudge   None, or a seed: every exp result is moved by a random -2 .. +2 ulp (the device's exp is not the host's)
VARIANTS lists the four combinations the tolerance is measured with.

TOL: over every job of the GPU test cases (tests/fit_cases.py) that is compared with it and on which all variants end with status 0, the largest per-parameter
difference |dp_j| / (|p_j| + 1e-3) between any two variants was measured (MEASURED below; tests/test_fit_cpu.py recomputes it
and fails when it exceeds TOL / 16).  TOL is 16 times that: the device adds one more summation order and one more exp, which the
variants only sample."""
import math

import numpy as np

from caesar_yolo_amd.measure import box_window
from reduce_ref import tree_sum      # the kernel's association (caesar_yolo_amd/csrc/cy_reduce.h)

FIELDS = ("status", "niter", "npix", "F", "lambda", "A", "x0", "y0", "a", "b", "c") + tuple(
    "H%d%d" % (i, j) for i in range(6) for j in range(i, 6))
MAX_COMP, NFIELDS, MIN_PIX, LDS_MAX = 16, 32, 7, 4096
LAMBDA0, LAMBDA_MAX, LAMBDA_MIN, SMALL_REL, SMALL_ABS, F_REL = 1e-3, 1e12, 1e-12, 1e-10, 1e-6, 1e-14
VARIANTS = (("tree", None), ("np", None), ("fsum", None), ("np", 12345))
MEASURED = 2.13e-7      # measured 2.121e-7, on the random scene (the drawn jobs compared with TOL stay below 1e-8)
TOL = 16 * MEASURED
IU = [(i, j) for i in range(6) for j in range(i, 6)]


def admissible(p):
    return bool(all(math.isfinite(v) for v in p) and p[0] > 0 and p[3] > 0 and p[5] > 0 and p[3] * p[5] - p[4] * p[4] > 0)


def sweep(p, dx, dy, y, ok, summ, rng):
    """The 28 sums at p over the list (dx, dy, y, ok: per list entry; an entry that is not ok contributes 0)."""
    A, x0, y0, a, b, c = (float(v) for v in p)
    u, v = dx - x0, dy - y0
    with np.errstate(all="ignore"):
        e = np.exp(-0.5 * ((a * u) * u + ((2.0 * b) * u) * v + (c * v) * v))
        if rng is not None:
            k = rng.integers(-2, 3, e.shape)
            for s in (1, 2):
                e = np.where(k >= s, np.nextafter(e, np.inf), e)
                e = np.where(k <= -s, np.nextafter(e, -np.inf), e)
        m = A * e
        r = y - m
        J = [e, m * (a * u + b * v), m * (b * u + c * v), ((-0.5 * m) * u) * u, ((-m) * u) * v, ((-0.5 * m) * v) * v]
        t = np.stack([r * r] + [J[i] * r for i in range(6)] + [J[i] * J[j] for i, j in IU])
    t = np.where(ok[None, :], t, 0.0)
    if summ == "tree":
        return tree_sum(t)
    if summ == "fsum":
        return np.array([math.fsum(row[ok]) if np.isfinite(row[ok]).all() else float(np.sum(row[ok])) for row in t])
    return np.array([np.sum(row[ok]) for row in t])


def solve(S, lam):
    """d of (H + lam diag(H)) d = g from the 28 sums, or None when a pivot is not positive and finite."""
    H = [[0.0] * 6 for _ in range(6)]
    for k, (i, j) in enumerate(IU):
        H[i][j] = H[j][i] = float(S[7 + k])
    g = [float(v) for v in S[1:7]]
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        t = H[j][j] + lam * H[j][j]
        for k in range(j):
            t -= L[j][k] * L[j][k]
        if not (t > 0.0) or not math.isfinite(t):
            return None
        L[j][j] = math.sqrt(t)
        for i in range(j + 1, 6):
            q = H[j][i]
            for k in range(j):
                q -= L[i][k] * L[j][k]
            L[i][j] = q / L[j][j]
    z, d = [0.0] * 6, [0.0] * 6
    for i in range(6):
        q = g[i]
        for k in range(i):
            q -= L[i][k] * z[k]
        z[i] = q / L[i][i]
    for i in range(5, -1, -1):
        q = z[i]
        for k in range(i + 1, 6):
            q -= L[k][i] * d[k]
        d[i] = q / L[i][i]
    return d


def fit_one(p0, dx, dy, y, ok, max_iter=64, summ="tree", nudge=None):
    """One job.  p0 relative to the window.  -> (status, niter, npix, F, lambda, p [6], H upper [21])."""
    npix = int(ok.sum())
    p = [float(v) for v in p0]
    zero = [0.0] * 21
    if not admissible(p):
        return 4, 0, npix, 0.0, 0.0, p, zero
    if npix < MIN_PIX:
        return 3, 0, npix, 0.0, 0.0, p, zero
    rng = None if nudge is None else np.random.default_rng(nudge)
    S = sweep(p, dx, dy, y, ok, summ, rng)
    lam = LAMBDA0
    with np.errstate(all="ignore"):
        for it in range(1, max_iter + 1):
            d = solve(S, lam)
            small = False
            if d is not None:
                small = all(abs(d[k]) <= SMALL_REL * (abs(p[k]) + SMALL_ABS) for k in range(6))
                pn = [p[k] + d[k] for k in range(6)]
                if admissible(pn):
                    Sn = sweep(pn, dx, dy, y, ok, summ, rng)
                    if Sn[0] < S[0]:
                        conv = small or S[0] - Sn[0] <= F_REL * S[0]
                        p, S, lam = pn, Sn, max(lam / 10.0, LAMBDA_MIN)
                        if conv:
                            return 0, it, npix, float(S[0]), lam, p, [float(v) for v in S[7:]]
                        continue
            if small:
                return 0, it, npix, float(S[0]), lam, p, [float(v) for v in S[7:]]
            lam *= 10.0
            if lam > LAMBDA_MAX:
                return 2, it, npix, float(S[0]), lam, p, [float(v) for v in S[7:]]
    return 2, max_iter, npix, float(S[0]), lam, p, [float(v) for v in S[7:]]


def fit_components(img, boxes, bkg, ncomp, start, masks, max_iter=64, summ="tree", nudge=None):
    """The whole call on a host image (float32; a pixel is valid when it is non-zero and finite).  -> [n, 16, 32] float64."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    n = boxes.shape[0]
    start = np.asarray(start, np.float64).reshape(n, MAX_COMP, 6)
    out = np.zeros((n, MAX_COMP, NFIELDS), np.float64)
    MH, MW = img.shape
    for i in range(n):
        x0, y0, h, w = box_window(boxes[i], MH, MW)
        if h * w > 1 << 24:
            out[i, :int(ncomp[i]), 0] = 1.0
            continue
        win = img[y0:y0 + h, x0:x0 + w]
        m = np.asarray(masks[i], np.uint8).reshape(h, w)
        for k in range(int(ncomp[i])):
            yy, xx = np.nonzero(m == k + 1)                # row-major: increasing window index
            v = win[yy, xx]
            ok = (v != 0) & np.isfinite(v)
            y = np.where(ok, v.astype(np.float64), 0.0) - float(bkg[i])
            p0 = start[i, k].copy()
            p0[1] -= float(x0)
            p0[2] -= float(y0)
            st, it, npix, F, lam, p, H = fit_one(p0, xx.astype(np.float64), yy.astype(np.float64), y, ok, max_iter, summ,
                                                 None if nudge is None else nudge + 1000 * i + k)
            if st in (3, 4):
                p = list(start[i, k])
            else:
                p = [p[0], p[1] + float(x0), p[2] + float(y0)] + list(p[3:])
            out[i, k] = [st, it, npix, F, lam] + list(p) + list(H)
    return out


def fit_variants(img, boxes, bkg, ncomp, start, masks, max_iter=64):
    """The call under every entry of VARIANTS: list of [n, 16, 32] arrays."""
    return [fit_components(img, boxes, bkg, ncomp, start, masks, max_iter, s, g) for s, g in VARIANTS]


def spread(results, ncomp):
    """(largest |dp_j| / (|p_j| + 1e-3) between any two results over the jobs on which all have status 0, number of such jobs,
    boolean [n, 16] of the jobs on which the results disagree on status)."""
    r0 = results[0]
    jobs = np.arange(MAX_COMP)[None, :] < np.asarray(ncomp).reshape(-1, 1)
    all0 = jobs.copy()
    differ = np.zeros_like(jobs)
    for r in results:
        all0 &= r[:, :, 0] == 0
        differ |= jobs & (r[:, :, 0] != r0[:, :, 0])
    worst = 0.0
    for a in range(len(results)):
        for b in range(a + 1, len(results)):
            pa, pb = results[a][:, :, 5:11][all0], results[b][:, :, 5:11][all0]
            if pa.size:
                worst = max(worst, float(np.max(np.abs(pa - pb) / (np.abs(pa) + 1e-3))))
    return worst, int(all0.sum()), differ


def cond_H(row):
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = row[11:32]
    H = H + np.triu(H, 1).T
    return float(np.linalg.cond(H)) if np.isfinite(H).all() and H.any() else float("inf")
