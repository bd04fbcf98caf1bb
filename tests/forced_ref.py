"""Reference for forced photometry (cy_forced_fit): the definition of include/caesar_yolo_hip.h restated in numpy float64, twice.
  plan()            status, support rectangle (residual_ref.rectangles, the planner's own), neighbours in (D2, index) order with
                    the duplicate rule, crowded, ndup
  forced_fit()      rows [n, 24] and per job what the bounds need.  loops=False: whole arrays over the window, np.sum per sum;
                    loops=True: nested loops over the window's pixels, every sum sequential in window order.  Both keep the sum of
                    |terms| per sum.  `nudge` moves every exp result by that many ulp (the device's exp is not the host's)
  solve()           Cholesky row by row with the pivot rule t > N_jj 2^-40 and finite, x = inv(N) b, C = inv(N), in Python floats:
                    every operation rounded on its own, in the order the header states
  solution_bound()  the first-order componentwise bound |inv(N)| (db + dN |x|) on the solution from per-sum bounds
  compare()         GPU (or loops) rows against the reference rows within bounds derived from the operation count

The bound of a sum.  A term is a product of two entries of w; an entry is (v - bkg) s or exp(-q / 2) s.  Both sides do the same
float64 operations on the same inputs except exp: the device's is taken as within 2 ulp of the true value and numpy's as within 1,
so an entry differs by at most 3 ulp = 6 2^-53 relative and a term by 12 2^-53 (+ second order).  The two sides add the npix terms
in different orders: each order is off from the exact sum by at most (npix - 1) 2^-53 sum|t|, together 2 npix 2^-53 sum|t|.  With
npix >= 1: |gpu - ref| <= (2 npix + 12 + slack) 2^-53 sum|t| <= C_SUM npix 2^-53 sum|t|, C_SUM = 16.  Derived, not measured."""
import math

import numpy as np

import residual_ref as RR

FIELDS, JOB_FIELDS, NEIGH_MAX, JOBS_MAX = 24, 6, 7, 1 << 20
NAMES = ("status", "npix", "nexcluded", "K", "nneigh", "crowded", "ndup", "amp", "amp_var", "bkg_off", "bkg_var", "cov_amp_bkg", "chi2", "syy", "n00",
         "b0", "corr_max", "wx0", "wx1", "wy0", "wy1", "capped", "reserved0", "reserved1")
EXACT = [0, 1, 2, 3, 4, 5, 6, 17, 18, 19, 20, 21, 22, 23]
U = 2.0 ** -53
C_SUM = 16.0
PIVOT = 2.0 ** -40
MARGIN_LIMIT = 2.0 ** -30         # a reference pivot margin below this: the job is compared on its exact fields alone


def plan(jobs, nsigma, MH, MW):
    """-> list of dicts {status, rect (x0, x1, y0, y1), neigh, crowded, ndup} per job."""
    jobs = np.asarray(jobs, np.float64).reshape(-1, JOB_FIELDS)
    n = jobs.shape[0]
    comp = np.concatenate([np.ones((n, 1)), jobs[:, :5]], axis=1)
    rows = RR.rectangles(comp, nsigma, MH, MW)
    out = []
    for k in range(n):
        st = int(rows[k, 0]) if math.isfinite(jobs[k, 5]) else 1
        rect = tuple(int(v) for v in rows[k, 1:5]) if st in (0, 2) else (-1, -1, -1, -1)
        out.append(dict(status=st, rect=rect, neigh=[], crowded=0, ndup=0))
    run = [k for k in range(n) if out[k]["status"] in (0, 2)]
    rects = np.array([out[k]["rect"] for k in run], np.int64).reshape(-1, 4)
    runa = np.array(run, np.int64)
    for t, k in enumerate(run):
        x0, x1, y0, y1 = out[k]["rect"]
        hit = (rects[:, 0] <= x1) & (x0 <= rects[:, 1]) & (rects[:, 2] <= y1) & (y0 <= rects[:, 3])
        hit[t] = False
        cand = []
        for f in runa[hit]:
            dx, dy = float(jobs[f, 0]) - float(jobs[k, 0]), float(jobs[f, 1]) - float(jobs[k, 1])
            cand.append((dx * dx + dy * dy, int(f)))
        cand.sort()
        o = out[k]
        for _, f in cand:
            same = lambda g: all(float(jobs[f, t]) == float(jobs[g, t]) for t in range(5))
            if same(k) or any(same(g) for g in o["neigh"]):
                o["ndup"] += 1
            elif len(o["neigh"]) < NEIGH_MAX:
                o["neigh"].append(f)
            else:
                o["crowded"] = 1
    return out


def _q(p, px, py):
    u, v = px - p[0], py - p[1]
    return ((p[2] * u) * u + ((2.0 * p[3]) * u) * v) + (p[4] * v) * v


def _nudged(e, nudge):
    for _ in range(abs(nudge)):
        e = np.nextafter(e, np.inf if nudge > 0 else -np.inf)
    return e


def design_arrays(img, rms, jobs, k, pl, nsigma, fit_bkg, nudge=0):
    """-> (W [npix, K + 1] in window order, nexcluded): the vectors w of the pixel set of job k."""
    x0, x1, y0, y1 = pl["rect"]
    px = np.arange(x0, x1 + 1, dtype=np.float64)[None, :]
    py = np.arange(y0, y1 + 1, dtype=np.float64)[:, None]
    v = np.asarray(img, np.float32)[y0:y1 + 1, x0:x1 + 1]
    with np.errstate(all="ignore"):
        ok = (v != 0) & np.isfinite(v)
        if rms is not None:
            r = np.asarray(rms, np.float32)[y0:y1 + 1, x0:x1 + 1]
            ok &= (r > 0) & np.isfinite(r)
        inside = _q(jobs[k], px, py) <= nsigma * nsigma
        mem = inside & ok
        s = 1.0 / r[mem].astype(np.float64) if rms is not None else np.ones(int(mem.sum()))
        cols = [(v[mem].astype(np.float64) - float(jobs[k, 5])) * s]
        for f in [k] + pl["neigh"]:
            cols.append(_nudged(np.exp(-0.5 * _q(jobs[f], px + 0 * py, py + 0 * px)[mem]), nudge) * s)
        if fit_bkg:
            cols.append(s)
    return np.stack(cols, axis=1).reshape(-1, len(cols)), int((inside & ~ok).sum())


def design_loops(img, rms, jobs, k, pl, nsigma, fit_bkg, nudge=0):
    x0, x1, y0, y1 = pl["rect"]
    ns2, rows, nex = nsigma * nsigma, [], 0
    img = np.asarray(img, np.float32)
    for iy in range(y0, y1 + 1):
        for ix in range(x0, x1 + 1):
            p = [float(t) for t in jobs[k]]
            if not _q(p, float(ix), float(iy)) <= ns2:
                continue
            v = float(img[iy, ix])
            ok = v != 0.0 and math.isfinite(v)
            r = 1.0
            if rms is not None:
                r = float(np.float32(rms[iy, ix]))
                ok = ok and r > 0.0 and math.isfinite(r)
            if not ok:
                nex += 1
                continue
            with np.errstate(all="ignore"):
                s = float(np.float64(1.0) / np.float64(r)) if rms is not None else 1.0
                w = [(v - p[5]) * s]
                for f in [k] + pl["neigh"]:
                    g = [float(t) for t in jobs[f]]
                    w.append(float(_nudged(np.exp(np.float64(-0.5 * _q(g, float(ix), float(iy)))), nudge)) * s)
            if fit_bkg:
                w.append(s)
            rows.append(w)
    K1 = 2 + len(pl["neigh"]) + int(fit_bkg)
    return np.array(rows, np.float64).reshape(-1, K1), nex


def sums(W, loops):
    """-> (S, AB): the (K + 1) x (K + 1) sums of w^T w (upper triangle mirrored) and the sums of |terms|."""
    m = W.shape[1]
    S, AB = np.zeros((m, m)), np.zeros((m, m))
    with np.errstate(all="ignore"):
        for i in range(m):
            for j in range(i, m):
                if loops:
                    acc = ab = 0.0
                    for p in range(W.shape[0]):
                        t = float(W[p, i]) * float(W[p, j])
                        acc += t
                        ab += abs(t)
                else:
                    t = W[:, i] * W[:, j]
                    acc, ab = float(t.sum()), float(np.abs(t).sum())
                S[i, j] = S[j, i] = acc
                AB[i, j] = AB[j, i] = ab
    return S, AB


def solve(S):
    """S: the sums, row / column 0 the datum.  -> None when a pivot fails, else (x, C, margin): margin = the smallest t / N_jj."""
    K = S.shape[0] - 1
    N = [[float(S[1 + i, 1 + j]) for j in range(K)] for i in range(K)]
    b = [float(S[0, 1 + i]) for i in range(K)]
    L = [[0.0] * K for _ in range(K)]
    margin = math.inf
    for j in range(K):
        t = N[j][j]
        for k in range(j):
            t -= L[j][k] * L[j][k]
        if not t > N[j][j] * PIVOT or not math.isfinite(t):
            return None
        margin = min(margin, t / N[j][j])
        L[j][j] = math.sqrt(t)
        for i in range(j + 1, K):
            q = N[j][i]
            for k in range(j):
                q -= L[i][k] * L[j][k]
            L[i][j] = q / L[j][j]
    z, x = [0.0] * K, [0.0] * K
    for i in range(K):
        q = b[i]
        for k in range(i):
            q -= L[i][k] * z[k]
        z[i] = q / L[i][i]
    for i in range(K - 1, -1, -1):
        q = z[i]
        for k in range(i + 1, K):
            q -= L[k][i] * x[k]
        x[i] = q / L[i][i]
    X = [[0.0] * K for _ in range(K)]
    for c in range(K):
        X[c][c] = 1.0 / L[c][c]
        for i in range(c + 1, K):
            q = 0.0
            for k in range(c, i):
                q -= L[i][k] * X[k][c]
            X[i][c] = q / L[i][i]
    C = np.zeros((K, K))
    for i in range(K):
        for j in range(i, K):
            c = 0.0
            for k in range(j, K):
                c += X[k][i] * X[k][j]
            C[i, j] = C[j, i] = c
    return np.array(x), C, margin


def scaled_cond(S):
    N = S[1:, 1:]
    d = 1.0 / np.sqrt(np.diag(N))
    return float(np.linalg.cond(N * d[:, None] * d[None, :]))


def solution_bound(N, x, dN, db):
    """The first-order componentwise bound |inv(N)| (db + dN |x|)."""
    return np.abs(np.linalg.inv(N)) @ (db + dN @ np.abs(x))


def forced_fit(img, rms, jobs, nsigma, fit_bkg, nudge=0, loops=False):
    """-> (rows [n, 24], aux): aux[k] is None for a job that is not run, else a dict with W, S, AB and, when solved, x, C, margin,
    cond (of N scaled to a unit diagonal)."""
    jobs = np.asarray(jobs, np.float64).reshape(-1, JOB_FIELDS)
    MH, MW = np.asarray(img).shape
    fit_bkg = int(bool(fit_bkg))
    plans = plan(jobs, nsigma, MH, MW)
    rows, aux = np.zeros((jobs.shape[0], FIELDS)), []
    for k, pl in enumerate(plans):
        r = rows[k]
        r[0] = pl["status"]
        r[17:21] = pl["rect"]
        if pl["status"] in (1, 3):
            aux.append(None)
            continue
        W, nex = (design_loops if loops else design_arrays)(img, rms, jobs, k, pl, nsigma, fit_bkg, nudge)
        S, AB = sums(W, loops)
        nn = len(pl["neigh"])
        K = 1 + nn + fit_bkg
        a = dict(W=W, S=S, AB=AB, K=K, nn=nn, solved=False, margin=None)
        r[1:7] = [W.shape[0], nex, K, nn, pl["crowded"], pl["ndup"]]
        r[13:16] = [S[0, 0], S[1, 1], S[0, 1]]
        r[21] = 1.0 if pl["status"] == 2 else 0.0
        with np.errstate(all="ignore"):
            got = None if W.shape[0] < K else solve(S)
        if W.shape[0] < K:
            r[0] = 5.0
        elif got is None:
            r[0] = 4.0
        else:
            x, C, margin = got
            a.update(solved=True, x=x, C=C, margin=margin, cond=scaled_cond(S))
            r[7], r[8] = x[0], C[0, 0]
            if fit_bkg:
                r[9], r[10], r[11] = x[K - 1], C[K - 1, K - 1], C[0, K - 1]
            corr = 0.0
            for i in range(1, nn + 1):
                c = abs(C[0, i]) / math.sqrt(C[0, 0] * C[i, i])
                if c > corr:
                    corr = c
            r[16] = corr
            if loops:
                chi = 0.0
                for w in W:
                    m = x[0] * w[1]
                    for i in range(1, K):
                        m += x[i] * w[1 + i]
                    chi += (w[0] - m) * (w[0] - m)
            else:
                m = x[0] * W[:, 1]
                for i in range(1, K):
                    m = m + x[i] * W[:, 1 + i]
                chi = float(((W[:, 0] - m) * (W[:, 0] - m)).sum())
            r[12] = chi
        aux.append(a)
    return rows, aux


def tolerances(a):
    """The bounds of one solved job from its reference aux: dict of amp, bkg_off (same bound rule, per unknown: dx [K]), var [K, K],
    corr, chi2 and sums [K + 1, K + 1]."""
    W, S, AB, K, nn = a["W"], a["S"], a["AB"], a["K"], a["nn"]
    npix = W.shape[0]
    dS = C_SUM * npix * U * AB
    out = dict(sums=dS)
    if not a["solved"]:
        return out
    x, C = a["x"], a["C"]
    N, dN, db = S[1:, 1:], dS[1:, 1:], dS[0, 1:]
    # the solve: K cond 2^-53 |x_i| per unknown with the cond of N scaled to a unit diagonal, which is what governs a Cholesky
    # solve (its error does not depend on the scaling of the unknowns); an entry of C is held to the same factor of its scale
    # sqrt(C_ii C_jj)
    solve_term = K * a["cond"] * U
    dx = 2.0 * solution_bound(N, x, dN, db) + solve_term * np.abs(x)
    aC = np.abs(C)
    sC = np.sqrt(np.diag(C))
    dC = 2.0 * (aC @ dN @ aC) + solve_term * sC[:, None] * sC[None, :]
    out.update(dx=dx, dC=dC)
    dcorr = 0.0
    for i in range(1, nn + 1):
        den = math.sqrt(C[0, 0] * C[i, i])
        r = abs(C[0, i]) / den
        dcorr = max(dcorr, dC[0, i] / den + r * 0.5 * (dC[0, 0] / C[0, 0] + dC[i, i] / C[i, i]) + 8 * U * r)
    out["corr"] = dcorr
    aW = np.abs(W[:, 1:])
    resid = W[:, 0] - W[:, 1:] @ x
    d = C_SUM * U * (np.abs(W[:, 0]) + aW @ np.abs(x)) + aW @ dx
    out["chi2"] = float((2.0 * np.abs(resid) * d + d * d).sum() + 2.0 * npix * U * (resid * resid).sum())
    return out


def compare(got, ref, aux, names, report=None):
    """Every job: the exact fields equal; the others within the derived bounds (module docstring).  A job whose reference pivot
    margin is below MARGIN_LIMIT is compared on its exact fields alone unless it is status 4 on both sides (then zeros: equal).
    report: a list that receives (name, field, |diff| / bound) of the worst ratio per field."""
    worst = {}
    assert got.shape == ref.shape
    for k, nm in enumerate(names):
        g, r, a = got[k], ref[k], aux[k]
        if a is not None and a["solved"] and a["margin"] < MARGIN_LIMIT:
            assert g[0] in (r[0], 4.0) and np.array_equal(g[EXACT[1:]], r[EXACT[1:]]), (nm, g, r)
            continue
        assert np.array_equal(g[EXACT], r[EXACT]), (nm, [(NAMES[f], g[f], r[f]) for f in EXACT if g[f] != r[f]])
        if a is None:
            assert np.array_equal(g, r), nm
            continue
        tol = tolerances(a)
        checks = [(13, tol["sums"][0, 0]), (14, tol["sums"][1, 1]), (15, tol["sums"][0, 1])]
        if a["solved"]:
            K = a["K"]
            checks += [(7, tol["dx"][0]), (8, tol["dC"][0, 0]), (16, tol["corr"]), (12, tol["chi2"])]
            if r[3] == 2 + r[4]:
                checks += [(9, tol["dx"][K - 1]), (10, tol["dC"][K - 1, K - 1]), (11, tol["dC"][0, K - 1])]
            else:
                assert g[9] == 0 and g[10] == 0 and g[11] == 0, nm
        else:
            assert not g[[7, 8, 9, 10, 11, 12, 16]].any(), nm
        for f, bound in checks:
            diff = abs(g[f] - r[f])
            assert diff <= bound, "%s: %s gpu %r ref %r differ by %.3g, bound %.3g" % (nm, NAMES[f], g[f], r[f], diff, bound)
            ratio = diff / bound if bound > 0 else 0.0
            if ratio >= worst.get(f, (0.0, ""))[0]:
                worst[f] = (ratio, nm)
    if report is not None:
        report.extend((nm, NAMES[f], ratio) for f, (ratio, nm) in sorted(worst.items()))
