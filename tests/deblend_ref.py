"""Reference for the source components (cy_deblend_islands), plain numpy float64 and an explicit uphill walk, written from the
definitions (DESIGN.md "Source components"), not from the kernel.

img, box window, candidate, seed, component (conn = 8 or 4), island set and main island: tests/island_ref.py, which supplies the
island set.  Per source four float64 numbers seed_thr, merge_thr, bkg, peak_thr.  Inside a window, pixel index i = dy * W + dx:
  rank    p outranks q when v(p) > v(q), or v(p) == v(q) and i(p) < i(q)
  up(p)   the highest-ranked of an island-set pixel p and its conn neighbours that are candidates;  summit: up(p) == p
  basin   the pixels whose walk p -> up(p) -> ... ends at one summit
  peak    a summit that outranks every island-set pixel of its own component within |dx|, |dy| <= radius, and either has
          float64(v) >= peak_thr or is the top-ranked pixel of its component
  kept    the first MAX_COMP peaks in rank order, components 0 .. ncomp - 1; any other summit's basin goes to the kept peak of the
          same island with the smallest integer squared distance (ties: lower component); none: unassigned
Row (FIELDS): status nsummits npeaks ncomp npix npix_unassigned reserved x 2.  Component row (COMP_FIELDS): npix peak x_peak
y_peak S Sx Sy Sxx Syy Sxy main nsummits, terms as in island_ref.  Mask: 0 / k + 1 / 255 unassigned.
deblend() also returns, per component, the sums of the absolute values of the terms of S Sx Sy Sxx Syy Sxy."""
import numpy as np

import island_ref

FIELDS = ("status", "nsummits", "npeaks", "ncomp", "npix", "npix_unassigned", "reserved0", "reserved1")
COMP_FIELDS = ("npix", "peak", "x_peak", "y_peak", "S", "Sx", "Sy", "Sxx", "Syy", "Sxy", "main", "nsummits")
SUMS = (4, 5, 6, 7, 8, 9)
MAX_COMP = 16
UNASSIGNED = 255


def _shifted(a, ddy, ddx, fill):
    """b[y, x] = a[y + ddy, x + ddx] where that lies inside a, else fill."""
    h, w = a.shape
    b = np.full(a.shape, fill, a.dtype)
    if abs(ddy) >= h or abs(ddx) >= w:
        return b
    ys, yd = (slice(ddy, h), slice(0, h - ddy)) if ddy >= 0 else (slice(0, h + ddy), slice(-ddy, h))
    xs, xd = (slice(ddx, w), slice(0, w - ddx)) if ddx >= 0 else (slice(0, w + ddx), slice(-ddx, w))
    b[yd, xd] = a[ys, xs]
    return b


def uphill(win, cand, inset, conn):
    """up [h, w] int64: flat index of up(p) for the island-set pixels, -1 elsewhere."""
    h, w = win.shape
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    v = np.where(cand, win, -np.inf).astype(np.float64)        # float32 values are exact in float64: the same order
    bv, bi = v.copy(), idx.copy()
    for ddy, ddx in (island_ref.NB8 if conn == 8 else island_ref.NB4):
        nv, ni = _shifted(v, ddy, ddx, -np.inf), _shifted(idx, ddy, ddx, -1)
        better = (ni >= 0) & ((nv > bv) | ((nv == bv) & (ni < bi)))
        bv, bi = np.where(better, nv, bv), np.where(better, ni, bi)
    return np.where(inset, bi, -1)


def walk(up):
    """summit [h * w] int64 of every island-set pixel (-1 elsewhere) by following up step by step; a resolved pixel ends the walk
    of every pixel that reaches it."""
    nxt = up.ravel().tolist()
    top = [-1] * len(nxt)
    for p in np.flatnonzero(up.ravel() >= 0).tolist():
        path = []
        q = p
        while top[q] < 0 and nxt[q] != q:
            path.append(q)
            q = nxt[q]
        s = q if top[q] < 0 else top[q]
        top[q] = s
        for r in path:
            top[r] = s
    return np.array(top, np.int64)


def deblend_one(img, box, thr4, conn=8, radius=2, full=False):
    MH, MW = img.shape
    assert 1 <= radius <= 8
    x1, y1, x2, y2 = (float(t) for t in box)
    seed_thr, merge_thr, bkg, peak_thr = (float(t) for t in thr4)
    irow, imask, _ = island_ref.islands_one(img, box, (seed_thr, merge_thr, bkg), conn)
    row = np.zeros(len(FIELDS), np.float64)
    comp = np.zeros((MAX_COMP, len(COMP_FIELDS)), np.float64)
    mags = np.zeros((MAX_COMP, len(SUMS)), np.float64)
    mask = np.zeros(imask.shape, np.uint8)
    extra = dict(summit=np.zeros(0, np.int64), peaks=[])
    ret = lambda: (row, comp, mask, mags, extra) if full else (row, comp, mask, mags)
    if irow[0] == 1:
        row[0] = 1.0
        return ret()
    if irow[1] == 0:
        return ret()
    bx0, bx1 = island_ref.box_side(x1, x2, MW)
    by0, by1 = island_ref.box_side(y1, y2, MH)
    win = img[by0:by1 + 1, bx0:bx1 + 1]
    h, w = win.shape
    with np.errstate(invalid="ignore"):
        v64 = win.astype(np.float64)
        cand = (win != 0) & np.isfinite(win) & (v64 >= merge_thr)
    lab, _ = island_ref.label(cand, conn)
    inset = imask > 0
    up = uphill(win, cand, inset, conn)
    summit = walk(up)
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    is_summit = inset & (up == idx)
    # radius test, at the summits only: no island-set pixel of the same component within the square outranks the summit
    vs = np.where(inset, v64, -np.inf)
    ls = np.where(inset, lab, 0)
    summits = np.flatnonzero(is_summit.ravel())
    sy, sx = np.divmod(summits, w)
    sv, sl = vs[sy, sx], lab[sy, sx]
    keep = np.ones(summits.size, bool)
    for ddy in range(-radius, radius + 1):
        for ddx in range(-radius, radius + 1):
            if ddy == 0 and ddx == 0:
                continue
            yy, xx = sy + ddy, sx + ddx
            inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            yc, xc = np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)
            nv, ni = vs[yc, xc], yc * w + xc
            keep &= ~(inside & (ls[yc, xc] == sl) & ((nv > sv) | ((nv == sv) & (ni < summits))))
    local = np.zeros(h * w, bool)
    local[summits[keep]] = True
    # the top-ranked pixel of every island
    flat_v, flat_l = v64.ravel(), lab.ravel()
    ins = np.flatnonzero(inset.ravel())
    order = ins[np.lexsort((ins, -flat_v[ins]))]
    _, first = np.unique(flat_l[order], return_index=True)
    tops = set(order[first].tolist())
    cands = np.flatnonzero(local.ravel())
    with np.errstate(invalid="ignore"):
        peaks = [int(p) for p in cands if flat_v[p] >= peak_thr or int(p) in tops]
    peaks.sort(key=lambda p: (-flat_v[p], p))
    kept = peaks[:MAX_COMP]
    # component of every summit
    comp_of = np.full(h * w, -2, np.int64)                    # -2: no summit, -1: unassigned
    best_k, best_d = np.full(summits.size, -1, np.int64), np.full(summits.size, np.iinfo(np.int64).max, np.int64)
    for k, t in enumerate(kept):
        ty, tx = divmod(t, w)
        d = (sx - tx) ** 2 + (sy - ty) ** 2
        take = (flat_l[summits] == flat_l[t]) & (d < best_d)
        best_k, best_d = np.where(take, k, best_k), np.where(take, d, best_d)
    comp_of[summits] = best_k
    for k, t in enumerate(kept):
        comp_of[t] = k
    pix_comp = np.where(summit >= 0, comp_of[np.maximum(summit, 0)], -2)
    assert (pix_comp[ins] >= -1).all() and (pix_comp[~inset.ravel()] == -2).all()
    m = np.zeros(h * w, np.uint8)
    m[pix_comp >= 0] = (pix_comp[pix_comp >= 0] + 1).astype(np.uint8)
    m[pix_comp == -1] = UNASSIGNED
    mask = m.reshape(h, w)
    row[0] = 2.0 if len(peaks) > MAX_COMP else 0.0
    row[1], row[2], row[3], row[4], row[5] = summits.size, len(peaks), len(kept), ins.size, int((pix_comp == -1).sum())
    py, px = divmod(int(np.argmax(np.where((win != 0) & np.isfinite(win), win, -np.inf))), w)
    main_lab = lab[py, px]
    for k, t in enumerate(kept):
        sel = np.flatnonzero(pix_comp == k)                   # increasing pixel index
        iy, ix = np.divmod(sel, w)
        wt = flat_v[sel] - bkg
        dx, dy = ix.astype(np.float64), iy.astype(np.float64)
        terms = [wt, wt * dx, wt * dy, wt * (dx * dx), wt * (dy * dy), wt * (dx * dy)]
        ty, tx = divmod(t, w)
        comp[k, 0], comp[k, 1], comp[k, 2], comp[k, 3] = sel.size, flat_v[t], bx0 + tx, by0 + ty
        for j, tm in enumerate(terms):
            comp[k, SUMS[j]] = tm.sum()
            mags[k, j] = np.abs(tm).sum()
        comp[k, 10] = 1.0 if flat_l[t] == main_lab else 0.0
        comp[k, 11] = int((comp_of[summits] == k).sum())
    extra = dict(summit=summit, peaks=peaks)
    return ret()


def deblend(img, boxes, thr4, conn=8, radius=2):
    """-> (rows [n, 8], component rows [n, 16, 12], list of n uint8 masks, mags [n, 16, 6] = sum |term| of S Sx Sy Sxx Syy Sxy)."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    thr4 = np.asarray(thr4, np.float64).reshape(-1, 4)
    assert boxes.shape[0] == thr4.shape[0]
    n = boxes.shape[0]
    rows = np.zeros((n, len(FIELDS)), np.float64)
    comps = np.zeros((n, MAX_COMP, len(COMP_FIELDS)), np.float64)
    mags = np.zeros((n, MAX_COMP, len(SUMS)), np.float64)
    masks = []
    for i in range(n):
        rows[i], comps[i], m, mags[i] = deblend_one(img, boxes[i], thr4[i], conn, radius)
        masks.append(m)
    return rows, comps, masks, mags


def thresholds(meas_rows, k_seed=5.0, k_merge=2.5, k_peak=5.0):
    """[n, 4] {bkg + k_seed * rms, bkg + k_merge * rms, bkg, bkg + k_peak * rms} from rows of measure_ref.measure."""
    bkg, rms = meas_rows[:, 2], meas_rows[:, 3]
    return np.stack([bkg + k_seed * rms, bkg + k_merge * rms, bkg, bkg + k_peak * rms], 1)
