"""Reference of cy_measure_background in plain numpy float64 ("Background mesh"): per cell a sort, the
clip loop exactly as defined (all `niter` clips, no early exit), no radix selection.

  valid pixel   != 0 and finite
  med(V)        middle element of the sorted float32 values as float64; even count: the two middle ones promoted, added, halved
  sig(V)        1.4826 * median of |(double)v - med(V)|
  clip          d = k * sig, lo = med - d, hi = med + d, L = max(L, lo), H = min(H, hi), V = {v in V_0 : L <= (double)v <= H}
  an empty V is not clipped again; its med and sig are 0
Row (FIELDS): n0 n bkg rms L H rounds reserved."""
import numpy as np

FIELDS = ("n0", "n", "bkg", "rms", "L", "H", "rounds", "reserved")


def median(v):
    """Exact median of a 1-D float64 array (0 for an empty one): (a + b) / 2 of the two middle elements for an even count."""
    n = v.size
    if n == 0:
        return 0.0
    s = np.sort(v)
    return float(s[n // 2]) if n % 2 else float((s[n // 2 - 1] + s[n // 2]) / 2.0)


def med_sig(v):
    m = median(v)
    return m, (float(np.float64(1.4826) * median(np.abs(v - m))) if v.size else 0.0)


def cell_stats(px, k, niter):
    """Row of one cell; px: its pixels (any shape, float32)."""
    px = np.asarray(px, np.float32).ravel()
    v0 = px[(px != 0) & np.isfinite(px)].astype(np.float64)
    L, H, rounds = -np.inf, np.inf, 0
    v = v0
    med, sig = med_sig(v)
    for _ in range(int(niter)):
        if v.size == 0:
            break
        d = float(k) * sig
        lo, hi = med - d, med + d
        L, H = max(L, lo), min(H, hi)
        nv = v0[(v0 >= L) & (v0 <= H)]
        if nv.size != v.size:
            rounds += 1
        v = nv
        med, sig = med_sig(v)
    return np.array([v0.size, v.size, med, sig, L, H, rounds, 0.0], np.float64)


def background(img, cell, k, niter):
    """[ncy, ncx, 8] float64 rows of every cell of `img` (2-D float32, blank = 0 or non-finite)."""
    img = np.asarray(img, np.float32)
    MH, MW = img.shape
    cell = int(cell)
    ncy, ncx = -(-MH // cell), -(-MW // cell)
    out = np.zeros((ncy, ncx, len(FIELDS)), np.float64)
    for cy in range(ncy):
        for cx in range(ncx):
            out[cy, cx] = cell_stats(img[cy * cell:min(MH, (cy + 1) * cell), cx * cell:min(MW, (cx + 1) * cell)], k, niter)
    return out
