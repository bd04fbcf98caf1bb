"""Reference for cy_fit_peak_groups, the definition of include/caesar_yolo_hip.h restated in numpy float64 on top of peakfit_ref (the
planner's statuses, windows and kept neighbours; the position-addressed membership) and blend_ref (the multi-Gaussian sums, solve,
iteration and covariance blocks: blend_ref.fit_job with ok = member & valid).
  plan()             links (strict, symmetric, equal sign), groups by union-find, slots, nlinked and the status the host decides
  group_members()    the pixel set of one group job over its window, and the pixels of the discs
  fit_peak_groups()  the whole call on a host map -> [n, FIELDS] rows.  The job's list is every pixel of the group window in increasing
                     window index, so blend_ref's "seq" summation is the kernel's association
The summation variants and the exp nudge are those of blend_ref.VARIANTS.

TOL: over every job of tests/peakgroup_cases.py (the drawn cases and the three filtered random scenes) that is compared on parameters
(status 0 in all variants, not left out), the largest |dp_j| / (|p_j| + 1e-3) between any two variants was measured (MEASURED;
tests/test_peakgroup_cpu.py recomputes it and fails when it no longer matches).  TOL is 16 times that, the project's margin.  The
entries of the members' blocks of C = inv(H), relative to sqrt(C_ii C_jj), are treated the same way (MEASURED_C, TOL_C).  Both are
measured between the variants of this reference, never against the kernel."""
import numpy as np

import blend_ref as BR
import peakfit_ref as PR

FIELDS, MAX_MEMBERS, LDS_MAX, LINK_MAX = 44, BR.MAX_MEMBERS, 8192, 2.0
NAMES = BR.FIELDS + ("wx0", "wx1", "wy0", "wy1", "clipped", "nexcluded", "nlinked", "reserved")
VARIANTS = BR.VARIANTS
MEASURED = 2.39e-7      # measured 2.380e-7, on the filtered random scene of seed 3 (the drawn jobs stay below 5e-9)
MEASURED_C = 2.86e-8    # measured 2.854e-8, on the filtered random scene of seed 1
TOL = 16 * MEASURED
TOL_C = 16 * MEASURED_C
IU = BR.IU


def plan(jobs, MH, MW, link, only=None):
    """-> dict: win [n, 6] and neigh as peakfit_ref.plan (only: the jobs whose neighbour lists are wanted, None: all); links: list of
    sets; group, size, slot, nlinked, status [n] (status: 1 / 5 the planner's, 6 alone, 7 above MAX_MEMBERS, 0 member of a group job).
    Every job tests the fitted jobs of its own and the eight surrounding cells of a grid as wide as the longest link."""
    jobs = np.asarray(jobs, np.float64).reshape(-1, PR.JOB_FIELDS)
    n = jobs.shape[0]
    win, neigh, _ = PR.plan(jobs, MH, MW, only)
    fitted = win[:, 0] == 0
    cx, cy, R, sign = jobs[:, 0], jobs[:, 1], jobs[:, 2], jobs[:, 4]
    links = [set() for _ in range(n)]
    root = list(range(n))

    def find(k):
        while root[k] != k:
            root[k] = root[root[k]]
            k = root[k]
        return k
    link = float(link)
    idx = np.nonzero(fitted)[0]
    cell = max(link * float(R[idx].max()) * (1.0 + 1e-9), 1.0) if idx.size else 1.0
    kx, ky = np.floor(cx[idx] / cell).astype(np.int64), np.floor(cy[idx] / cell).astype(np.int64)
    grid = {}
    for e, a, b in zip(idx.tolist(), kx.tolist(), ky.tolist()):
        grid.setdefault((a, b), []).append(e)
    for e, a, b in zip(idx.tolist(), kx.tolist(), ky.tolist()):
        cand = np.array(sorted(f for u in (-1, 0, 1) for v in (-1, 0, 1) for f in grid.get((a + u, b + v), ()) if f != e), np.int64)
        if not cand.size:
            continue
        with np.errstate(all="ignore"):
            dx, dy = cx[cand] - cx[e], cy[cand] - cy[e]
            D2 = dx * dx + dy * dy
            Lm = link * np.maximum(R[cand], R[e])
            hit = (sign[cand] == sign[e]) & (D2 < Lm * Lm)
        for f in cand[hit].tolist():
            links[e].add(f)
            a2, b2 = find(e), find(f)
            if a2 != b2:
                root[max(a2, b2)] = min(a2, b2)
    group = np.array([find(k) for k in range(n)], np.int64)
    count = np.bincount(group, minlength=n) if n else np.zeros(0, np.int64)
    size = count[group].astype(np.int64) if n else np.zeros(0, np.int64)
    seen, slot = {}, np.zeros(n, np.int64)
    for k in range(n):
        slot[k] = seen.get(int(group[k]), 0)
        seen[int(group[k])] = int(slot[k]) + 1
    status = np.where(~fitted, win[:, 0], np.where(size == 1, 6, np.where(size > MAX_MEMBERS, 7, 0)))
    assert all((e in links[f]) == (f in links[e]) for e in range(n) for f in links[e])
    return dict(win=win, neigh=neigh, links=links, group=group, size=size, slot=slot, nlinked=np.array([len(s) for s in links], np.int64), status=status)


def group_window(win, members):
    w = win[members]
    return int(w[:, 1].min()), int(w[:, 2].max()), int(w[:, 3].min()), int(w[:, 4].max()), int(w[:, 5].max())


def group_members(jobs, members, neigh, w):
    """(in some member's share, inside some member's disc, dx, dy) over the group window w = (x0, x1, y0, y1)."""
    mine = inside = None
    for e in members:
        outside = [(jobs[f, 0], jobs[f, 1]) for f in neigh[e] if f not in members]
        m, i, dx, dy = PR.members(jobs[e], w, outside)
        mine, inside = (m, i) if mine is None else (mine | m, inside | i)
    return mine, inside, dx, dy


def fit_peak_groups(amap, jobs, link=1.5, max_iter=64, summ="seq", nudge=None, return_cond=False):
    """The whole call on a host map -> [n, FIELDS] float64 (with return_cond also cond(H) of the job on every member's row, inf
    where there is none)."""
    amap = np.ascontiguousarray(amap, np.float32)
    jobs = np.asarray(jobs, np.float64).reshape(-1, PR.JOB_FIELDS)
    MH, MW = amap.shape
    n = jobs.shape[0]
    P = plan(jobs, MH, MW, link)
    win, group, size, slot, status = P["win"], P["group"], P["size"], P["slot"], P["status"]
    out = np.zeros((n, FIELDS), np.float64)
    cond = np.full(n, np.inf)
    for e in range(n):
        st = int(status[e])
        out[e, 0] = st
        if st in (1, 5):
            out[e, 36:40] = -1.0
            continue
        members = [int(k) for k in np.nonzero(group == group[e])[0]]
        out[e, 5:8] = [group[e], size[e], slot[e]]
        out[e, 36:41] = group_window(win, members)
        out[e, 42] = P["nlinked"][e]
        if st == 7:
            out[e, 8:14] = jobs[e, 5:11]
    for g in range(n):
        if status[g] != 0 or group[g] != g:
            continue
        members = [int(k) for k in np.nonzero(group == g)[0]]
        x0, x1, y0, y1, _ = group_window(win, members)
        mine, inside, dx, dy = group_members(jobs, members, P["neigh"], (x0, x1, y0, y1))
        v = amap[y0:y1 + 1, x0:x1 + 1].ravel()
        valid = (v != 0) & np.isfinite(v)
        ok = mine & valid
        y = float(jobs[g, 4]) * (np.where(valid, v.astype(np.float64), 0.0) - float(jobs[g, 3]))
        p0 = jobs[members, 5:11].copy()
        p0[:, 1] -= float(x0)
        p0[:, 2] -= float(y0)
        M = len(members)
        st, it, npix, F, lam, p, S = BR.fit_job(p0, dx, dy, y, ok, max_iter, summ, None if nudge is None else nudge + g)
        cov_ok, C = (0, np.zeros((M, 21))) if st in (3, 4) else BR.covariance_blocks(S, 6 * M)
        nex = int((inside & ~mine & valid).sum())
        for s, k in enumerate(members):
            q = list(jobs[k, 5:11]) if st in (3, 4) else [p[s][0], p[s][1] + float(x0), p[s][2] + float(y0)] + list(p[s][3:])
            out[k, :36] = [st, it, npix, F, lam, g, M, s] + q + [cov_ok] + list(C[s])
            out[k, 41] = nex
            cond[k] = BR.cond_H(S, 6 * M)
    return (out, cond) if return_cond else out


def fit_variants(amap, jobs, link=1.5, max_iter=64):
    """The call under every entry of VARIANTS: (list of [n, FIELDS] arrays, cond [n] of the first)."""
    first, cond = fit_peak_groups(amap, jobs, link, max_iter, *VARIANTS[0], return_cond=True)
    return [first] + [fit_peak_groups(amap, jobs, link, max_iter, s, g) for s, g in VARIANTS[1:]], cond


def excluded(res, cond):
    """Boolean [n]: the jobs a parameter comparison may leave out: the variants disagree on status, one of them stopped at a limit
    (status 2), or cond(H) of the first variant exceeds 1e10.  Only rows of group jobs can be."""
    out = np.zeros(res[0].shape[0], bool)
    for e in range(out.size):
        sts = {float(r[e, 0]) for r in res}
        if not sts <= {0.0, 2.0}:
            out[e] = len(sts) > 1
        else:
            out[e] = len(sts) > 1 or 2.0 in sts or cond[e] > 1e10
    return out


def spread(results, keep=None):
    """(largest |dp_j| / (|p_j| + 1e-3) between any two results over the rows on which all have status 0, the same for the entries
    of C relative to sqrt(C_ii C_jj) on the rows with cov_ok everywhere, number of such rows).  keep: boolean [n], rows to measure on."""
    n = results[0].shape[0]
    all0 = np.ones(n, bool) if keep is None else keep.copy()
    for r in results:
        all0 &= r[:, 0] == 0
    worst = worst_c = 0.0
    for a in range(len(results)):
        for b in range(a + 1, len(results)):
            pa, pb = results[a][all0, 8:14], results[b][all0, 8:14]
            if pa.size:
                worst = max(worst, float(np.max(np.abs(pa - pb) / (np.abs(pa) + 1e-3))))
            for ra, rb in zip(results[a][all0], results[b][all0]):
                if ra[14] and rb[14]:
                    d = np.sqrt(np.abs(ra[[15, 21, 26, 30, 33, 35]]))
                    sc = np.array([max(d[i] * d[j], 1e-300) for i, j in IU])
                    worst_c = max(worst_c, float(np.max(np.abs(ra[15:36] - rb[15:36]) / sc)))
    return worst, worst_c, int(all0.sum())
