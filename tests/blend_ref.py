"""Reference for the joint fits of blends (cy_fit_blends), the algorithm of include/caesar_yolo_hip.h restated in numpy float64 on
top of tests/fit_ref.py: the same grouping, the same expressions and roundings per pixel, the same Cholesky, accept / reject rules
and constants, the same inverse.  Two parts are switchable, because the device differs from any host restatement in these two:
  summ    how the sums of a sweep are added: "seq" (the kernel's association: one plain sequential sum per entry over the list in
          increasing list position; np.cumsum adds exactly so), "np" (np.sum, pairwise) or "fsum" (math.fsum, exactly rounded)
  nudge   None, or a seed: every exp result is moved by a random -2 .. +2 ulp (the device's exp is not the host's)
VARIANTS lists the four combinations the tolerance is measured with.

TOL: over every job of the GPU test cases (tests/blend_cases.py) that is compared on parameters (status 0 in all variants), the
largest |dp_j| / (|p_j| + 1e-3) between any two variants was measured (MEASURED; tests/test_blend_cpu.py recomputes it and fails
when it exceeds the recorded value).  TOL is 16 times that.  The entries of the members' blocks of C = inv(H) are compared
relative to sqrt(C_ii C_jj); their spread was measured separately (MEASURED_C) and is smaller than the parameters', so TOL_C = TOL."""
import math

import numpy as np

import fit_ref
from fit_ref import F_REL, LAMBDA0, LAMBDA_MAX, LAMBDA_MIN, SMALL_ABS, SMALL_REL, admissible
from caesar_yolo_amd import measure
from caesar_yolo_amd.measure import box_window

FIELDS = ("status", "niter", "npix", "F", "lambda", "group", "nmembers", "slot", "A", "x0", "y0", "a", "b", "c", "cov_ok") + tuple(
    "C%d%d" % (i, j) for i in range(6) for j in range(i, 6))
MAX_COMP, NFIELDS, MAX_MEMBERS, LDS_MAX, CHUNK = 16, 36, 4, 4096, 128
VARIANTS = (("seq", None), ("np", None), ("fsum", None), ("np", 12345))
MEASURED = 3.88e-7      # measured 3.879e-7, on the random scene (the drawn rows stay below 1e-10)
MEASURED_C = 2.70e-8    # measured 2.693e-8, on the random scene: not larger than the parameters', so C is compared with TOL
TOL = 16 * MEASURED
TOL_C = TOL
IU = fit_ref.IU


def nsum(P):
    return (P + 1) * (P + 2) // 2


def sweep(p, dx, dy, y, ok, summ, rng):
    """The (P + 1)(P + 2) / 2 sums at p [M, 6] over the list: the upper triangle of w^T w, w = (r, J_0 .. J_{P-1}), row-major."""
    M = len(p)
    rows, mt = [None], None
    with np.errstate(all="ignore"):
        for s in range(M):
            A, x0, y0, a, b, c = (float(v) for v in p[s])
            u, v = dx - x0, dy - y0
            e = np.exp(-0.5 * ((a * u) * u + ((2.0 * b) * u) * v + (c * v) * v))
            if rng is not None:
                k = rng.integers(-2, 3, e.shape)
                for t in (1, 2):
                    e = np.where(k >= t, np.nextafter(e, np.inf), e)
                    e = np.where(k <= -t, np.nextafter(e, -np.inf), e)
            m = A * e
            rows += [e, m * (a * u + b * v), m * (b * u + c * v), ((-0.5 * m) * u) * u, ((-m) * u) * v, ((-0.5 * m) * v) * v]
            mt = m if s == 0 else mt + m
        rows[0] = y - mt
        w = np.stack(rows)
        ia, ib = np.triu_indices(6 * M + 1)
        t = w[ia] * w[ib]
    t = np.where(ok[None, :], t, 0.0)
    if summ == "seq":
        return np.cumsum(t, axis=1)[:, -1] if t.shape[1] else np.zeros(t.shape[0])
    if summ == "fsum":
        return np.array([math.fsum(row[ok]) if np.isfinite(row[ok]).all() else float(np.sum(row[ok])) for row in t])
    return np.array([np.sum(row[ok]) for row in t])


def unpack(S, P):
    """(g [P], H [P, P] symmetric) from the sums."""
    H = np.zeros((P, P))
    H[np.triu_indices(P)] = S[1 + P:]
    return np.array(S[1:1 + P], np.float64), H + np.triu(H, 1).T


def factor(H, lam):
    """L of H + lam diag(H) (every inner sum subtracted term by term in increasing k), or None on a pivot not positive and finite."""
    P = H.shape[0]
    L = np.zeros((P, P))
    with np.errstate(all="ignore"):
        for j in range(P):
            t = H[j, j] + lam * H[j, j]
            for k in range(j):
                t -= L[j, k] * L[j, k]
            if not (t > 0.0) or not math.isfinite(t):
                return None
            L[j, j] = math.sqrt(t)
            q = H[j, j + 1:].copy()
            for k in range(j):
                q -= L[j + 1:, k] * L[j, k]
            L[j + 1:, j] = q / L[j, j]
    return L


def solve(S, P, lam):
    g, H = unpack(S, P)
    L = factor(H, lam)
    if L is None:
        return None
    z, d = [0.0] * P, [0.0] * P
    for i in range(P):
        q = float(g[i])
        for k in range(i):
            q -= float(L[i, k]) * z[k]
        z[i] = q / float(L[i, i])
    for i in range(P - 1, -1, -1):
        q = z[i]
        for k in range(i + 1, P):
            q -= float(L[k, i]) * d[k]
        d[i] = q / float(L[i, i])
    return d


def covariance_blocks(S, P):
    """(cov_ok, [M, 21]): the upper triangles of the members' 6 x 6 diagonal blocks of inv(H), by the header's recipe."""
    M = P // 6
    _, H = unpack(S, P)
    L = factor(H, 0.0)
    out = np.zeros((M, 21))
    if L is None:
        return 0, out
    X = np.zeros((P, P))
    with np.errstate(all="ignore"):
        for c in range(P):
            X[c, c] = 1.0 / L[c, c]
            for i in range(c + 1, P):
                q = 0.0
                for k in range(c, i):
                    q -= L[i, k] * X[k, c]
                X[i, c] = q / L[i, i]
        for s in range(M):
            for t, (i, j) in enumerate(IU):
                out[s, t] = np.cumsum(X[6 * s + j:, 6 * s + i] * X[6 * s + j:, 6 * s + j])[-1]
    return 1, out


def fit_job(p0, dx, dy, y, ok, max_iter=64, summ="seq", nudge=None):
    """One job.  p0 [M, 6] relative to the window.  -> (status, niter, npix, F, lambda, p [M, 6], S or None)."""
    M = len(p0)
    P = 6 * M
    npix = int(ok.sum())
    p = [[float(v) for v in row] for row in p0]
    if not all(admissible(q) for q in p):
        return 4, 0, npix, 0.0, 0.0, p, None
    if npix < P + 1:
        return 3, 0, npix, 0.0, 0.0, p, None
    rng = None if nudge is None else np.random.default_rng(nudge)
    S = sweep(p, dx, dy, y, ok, summ, rng)
    lam = LAMBDA0
    flat = lambda q: [v for row in q for v in row]
    with np.errstate(all="ignore"):
        for it in range(1, max_iter + 1):
            d = solve(S, P, lam)
            small = False
            if d is not None:
                pf = flat(p)
                small = all(abs(d[k]) <= SMALL_REL * (abs(pf[k]) + SMALL_ABS) for k in range(P))
                pn = [[pf[6 * s + k] + d[6 * s + k] for k in range(6)] for s in range(M)]
                if all(admissible(q) for q in pn):
                    Sn = sweep(pn, dx, dy, y, ok, summ, rng)
                    if Sn[0] < S[0]:
                        conv = small or S[0] - Sn[0] <= F_REL * S[0]
                        p, S, lam = pn, Sn, max(lam / 10.0, LAMBDA_MIN)
                        if conv:
                            return 0, it, npix, float(S[0]), lam, p, S
                        continue
            if small:
                return 0, it, npix, float(S[0]), lam, p, S
            lam *= 10.0
            if lam > LAMBDA_MAX:
                return 2, it, npix, float(S[0]), lam, p, S
    return 2, max_iter, npix, float(S[0]), lam, p, S


def cond_H(S, P):
    if S is None:
        return float("inf")
    _, H = unpack(S, P)
    return float(np.linalg.cond(H)) if np.isfinite(H).all() and H.any() else float("inf")


def fit_blends(img, boxes, bkg, ncomp, start, masks, max_iter=64, summ="seq", nudge=None, return_cond=False):
    """The whole call on a host image.  -> [n, 16, 36] float64 (with return_cond also cond(H) of the job on every member's row,
    [n, 16], inf where there is none)."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    n = boxes.shape[0]
    start = np.asarray(start, np.float64).reshape(n, MAX_COMP, 6)
    out = np.zeros((n, MAX_COMP, NFIELDS), np.float64)
    cond = np.full((n, MAX_COMP), np.inf)
    MH, MW = img.shape
    for i in range(n):
        x0, y0, h, w = box_window(boxes[i], MH, MW)
        nc = int(ncomp[i])
        if h * w > 1 << 24:
            out[i, :nc, 0] = 1.0
            continue
        win = img[y0:y0 + h, x0:x0 + w]
        m = np.asarray(masks[i], np.uint8).reshape(h, w)
        grp = measure.blend_groups(m, h, w, nc)
        for k in range(nc):
            g, M, slot = (int(v) for v in grp[k])
            out[i, k, 5:8] = [g, M, slot]
            if M == 1:
                out[i, k, 0] = 6.0
            elif M > MAX_MEMBERS:
                out[i, k, 0] = 5.0
                out[i, k, 8:14] = start[i, k]
        for g in range(nc):
            members = [k for k in range(nc) if grp[k][0] == g]
            if not 2 <= len(members) <= MAX_MEMBERS or members[0] != g:
                continue
            yy, xx = np.nonzero(np.isin(m, [k + 1 for k in members]))                # row-major: increasing window index
            v = win[yy, xx]
            ok = (v != 0) & np.isfinite(v)
            y = np.where(ok, v.astype(np.float64), 0.0) - float(bkg[i])
            p0 = start[i, members].copy()
            p0[:, 1] -= float(x0)
            p0[:, 2] -= float(y0)
            st, it, npix, F, lam, p, S = fit_job(p0, xx.astype(np.float64), yy.astype(np.float64), y, ok, max_iter, summ,
                                                 None if nudge is None else nudge + 1000 * i + g)
            cov_ok, C = (0, np.zeros((len(members), 21))) if st in (3, 4) else covariance_blocks(S, 6 * len(members))
            for s, k in enumerate(members):
                q = list(start[i, k]) if st in (3, 4) else [p[s][0], p[s][1] + float(x0), p[s][2] + float(y0)] + list(p[s][3:])
                out[i, k] = [st, it, npix, F, lam, g, len(members), s] + q + [cov_ok] + list(C[s])
                cond[i, k] = cond_H(S, 6 * len(members))
    return (out, cond) if return_cond else out


def fit_variants(img, boxes, bkg, ncomp, start, masks, max_iter=64):
    """The call under every entry of VARIANTS: (list of [n, 16, 36] arrays, cond [n, 16] of the first)."""
    first, cond = fit_blends(img, boxes, bkg, ncomp, start, masks, max_iter, *VARIANTS[0], return_cond=True)
    return [first] + [fit_blends(img, boxes, bkg, ncomp, start, masks, max_iter, s, g) for s, g in VARIANTS[1:]], cond


def spread(results, ncomp, keep=None):
    """(largest |dp_j| / (|p_j| + 1e-3) between any two results over the member rows on which all have status 0, the same for
    the entries of C relative to sqrt(C_ii C_jj) on the rows with cov_ok everywhere, number of such rows, boolean [n, 16] of
    the rows on which the results disagree on status).  keep: boolean [n, 16], rows to measure on (default: all below ncomp)."""
    r0 = results[0]
    rows = np.arange(MAX_COMP)[None, :] < np.asarray(ncomp).reshape(-1, 1)
    all0 = rows.copy() if keep is None else rows & keep
    differ = np.zeros_like(rows)
    for r in results:
        all0 &= r[:, :, 0] == 0
        differ |= rows & (r[:, :, 0] != r0[:, :, 0])
    worst = worst_c = 0.0
    for a in range(len(results)):
        for b in range(a + 1, len(results)):
            pa, pb = results[a][:, :, 8:14][all0], results[b][:, :, 8:14][all0]
            if pa.size:
                worst = max(worst, float(np.max(np.abs(pa - pb) / (np.abs(pa) + 1e-3))))
            for ra, rb in zip(results[a][all0], results[b][all0]):
                if ra[14] and rb[14]:
                    d = np.sqrt(np.abs(ra[[15, 21, 26, 30, 33, 35]]))
                    sc = np.array([max(d[i] * d[j], 1e-300) for i, j in IU])
                    worst_c = max(worst_c, float(np.max(np.abs(ra[15:] - rb[15:]) / sc)))
    return worst, worst_c, int(all0.sum()), differ
