"""Reference for the model and residual maps (cy_render_gaussians) and the per-source residuals (cy_measure_residuals): the
definitions of include/caesar_yolo_hip.h restated in numpy float64.
  rectangles()      status, support rectangle and tile count of every component, the host's float64 arithmetic
  tile_table()      the CSR table over the 32 x 32 tiles the runtime builds from them
  render()          model = one plain sequential float64 sum per pixel over the contributing components in increasing index (term
                    after term added to the running sum inside the component's rectangle: the running sums np.cumsum would give over
                    the stacked terms, without storing the stack), residual = ((double)v - bkg) - model on valid pixels.  `nudge`
                    moves every exp result by that many ulp (the device's exp is not the host's)
  residual_stats()  counts, sums (plain np.sum), largest |r| with its first position, model sum; and per sum the sum of |terms| that
                    the GPU test's bound needs

TOL_M: over every render case of tests/residual_cases.py, the largest relative difference of the float64 model between the variants
nudge = -2, 0, +2 on the pixels whose model is at least 2^-149 (the smallest fp32 number; below it the absolute term of the GPU
bounds covers any float64 value), times 16, the factor of the fit and blend tests.  tests/test_residual_cpu.py recomputes MEASURED
and asserts it."""
import math

import numpy as np

from caesar_yolo_amd.measure import box_window

RND_FIELDS, HALF_MAX, TILE, RES_FIELDS = 8, 256, 32, 12
MAX_COMP, MAX_LIST, MAX_AREA = 1 << 20, 1 << 27, 1 << 24
NUDGES = (-2, 0, 2)
MEASURED = 8.46e-16      # measured 8.456e-16, on the 130 components of one tile (a single component gives 5.6e-16)
TOL_M = 16 * MEASURED
F32_MIN = 2.0 ** -149


def admissible(p):
    return bool(all(math.isfinite(v) for v in p) and p[0] > 0 and p[3] > 0 and p[5] > 0 and p[3] * p[5] - p[4] * p[4] > 0)


def _side(c0, h, N):
    f = math.floor(c0)
    lo, hi = f - h, (f + 1.0) + h
    if hi < 0.0 or lo > float(N - 1):
        return None
    return (int(lo) if lo > 0.0 else 0), (int(hi) if hi < float(N - 1) else N - 1)


def rectangles(comp, nsigma, MH, MW):
    """-> rows float64 [m, 8] {status, sx0, sx1, sy0, sy1, ntiles, 0, 0}."""
    comp = np.asarray(comp, np.float64).reshape(-1, 6)
    rows = np.zeros((comp.shape[0], RND_FIELDS), np.float64)
    rows[:, 1:5] = -1.0
    for k, p in enumerate(comp):
        p = [float(v) for v in p]
        if not admissible(p):
            rows[k, 0] = 1.0
            continue
        a, b, c = p[3:]
        det = a * c - b * b
        half, capped = [], False
        for num in (c, a):
            h = math.ceil(nsigma * math.sqrt(num / det)) if math.isfinite(nsigma * math.sqrt(num / det)) else math.inf
            if not h <= HALF_MAX:
                h, capped = HALF_MAX, True
            half.append(float(h))
        sx, sy = _side(p[1], half[0], MW), _side(p[2], half[1], MH)
        if sx is None or sy is None:
            rows[k, 0] = 3.0
            continue
        rows[k, 0] = 2.0 if capped else 0.0
        rows[k, 1:5] = [sx[0], sx[1], sy[0], sy[1]]
        rows[k, 5] = (sx[1] // TILE - sx[0] // TILE + 1) * (sy[1] // TILE - sy[0] // TILE + 1)
    return rows


def size_limit(comp_count, rows):
    """The message cy_render_gaussians' planner gives for a size limit, or None."""
    if comp_count < 0 or comp_count > MAX_COMP:
        return "m outside 0 .. 2^20"
    if len(rows) and np.cumsum(rows[:, 5]).max() > MAX_LIST:
        return "tile table above 2^27 entries"
    return None


def tile_table(rows, MH, MW):
    """-> (tile_off int64 [ntiles + 1], tile_list int64): per tile (row-major) the rendered components meeting it, increasing."""
    ntx, nty = -(-MW // TILE), -(-MH // TILE)
    lists = [[] for _ in range(ntx * nty)]
    for k, r in enumerate(np.asarray(rows)):
        if r[0] in (1.0, 3.0):
            continue
        sx0, sx1, sy0, sy1 = (int(v) for v in r[1:5])
        for ty in range(sy0 // TILE, sy1 // TILE + 1):
            for tx in range(sx0 // TILE, sx1 // TILE + 1):
                lists[ty * ntx + tx].append(k)
    off = np.zeros(ntx * nty + 1, np.int64)
    np.cumsum([len(l) for l in lists], out=off[1:])
    return off, np.array([k for l in lists for k in l], np.int64)


def valid(img):
    img = np.asarray(img, np.float32)
    return (img != 0) & np.isfinite(img)


def model_map(comp, rows, MH, MW, nudge=0, origin=(0, 0)):
    """The float64 model [MH, MW].  origin = (y0, x0): the map is the crop [y0, y0 + MH) x [x0, x0 + MW) of the image that comp and
    rows (rectangles() on the whole image) speak of; every pixel is computed from its true coordinates, so the crop of the full
    model and the model of the crop are the same numbers."""
    comp = np.asarray(comp, np.float64).reshape(-1, 6)
    model = np.zeros((MH, MW), np.float64)
    oy, ox = int(origin[0]), int(origin[1])
    for p, r in zip(comp, rows):
        if r[0] in (1.0, 3.0):
            continue
        sx0, sx1, sy0, sy1 = (int(v) for v in r[1:5])
        sx0, sx1, sy0, sy1 = max(sx0, ox), min(sx1, ox + MW - 1), max(sy0, oy), min(sy1, oy + MH - 1)
        if sx1 < sx0 or sy1 < sy0:
            continue
        A, x0, y0, a, b, c = (float(v) for v in p)
        u = np.arange(sx0, sx1 + 1, dtype=np.float64)[None, :] - x0
        v = np.arange(sy0, sy1 + 1, dtype=np.float64)[:, None] - y0
        with np.errstate(all="ignore"):
            e = np.exp(-0.5 * (((a * u) * u + ((2.0 * b) * u) * v) + (c * v) * v))
            for _ in range(abs(nudge)):
                e = np.nextafter(e, np.inf if nudge > 0 else -np.inf)
            model[sy0 - oy:sy1 + 1 - oy, sx0 - ox:sx1 + 1 - ox] += A * e
    return model


def render(img, comp, nsigma, bkg=None, nudge=0, origin=(0, 0), full=None):
    """-> (rows [m, 8], model float64 [MH, MW], resid float64 [MH, MW]); what the device stores is their fp32 rounding.
    origin, full: img (and bkg) is the crop at origin = (y0, x0) of an image of shape full = (MH, MW); comp and rows stay in that
    image's coordinates (model_map)."""
    img = np.asarray(img, np.float32)
    MH, MW = img.shape
    rows = rectangles(comp, nsigma, *(full or (MH, MW)))
    model = model_map(comp, rows, MH, MW, nudge, origin)
    ok = valid(img)
    b = np.zeros((MH, MW), np.float64) if bkg is None else np.asarray(bkg, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        resid = np.where(ok, (np.where(ok, img, 0).astype(np.float64) - b) - model, 0.0)
    return rows, model, resid


def model_spread(comp, nsigma, MH, MW):
    """Largest relative difference of the model between the NUDGES variants over the pixels with model >= 2^-149."""
    rows = rectangles(comp, nsigma, MH, MW)
    ms = [model_map(comp, rows, MH, MW, k) for k in NUDGES]
    big = ms[1] >= F32_MIN
    if not big.any():
        return 0.0
    return max(float(np.max(np.abs(ms[i] - ms[1])[big] / ms[1][big])) for i in (0, 2))


def model_bound(x):
    """|model_gpu - x| allowed, x the float64 reference."""
    x = np.abs(x)
    return 2.0 ** -24 * x * (1.0 + TOL_M) + TOL_M * x + F32_MIN


def resid_bound(x, model):
    """|resid_gpu - x| allowed, x the float64 reference residual and model the float64 reference model."""
    return 2.0 ** -24 * (np.abs(x) + TOL_M * np.abs(model)) + TOL_M * np.abs(model) + F32_MIN


def residual_stats(img, model, boxes, bkg, masks):
    """img, model: float32 [MH, MW].  -> (rows float64 [n, 12], abs float64 [n, 5]: the sums of |terms| of sum_win, sumsq_win,
    sum_isl, sumsq_isl, model_isl)."""
    img, model = np.asarray(img, np.float32), np.asarray(model, np.float32)
    MH, MW = img.shape
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    out = np.zeros((len(boxes), RES_FIELDS), np.float64)
    ab = np.zeros((len(boxes), 5), np.float64)
    out[:, 8:10] = -1.0
    for i, box in enumerate(boxes):
        x0, y0, h, w = box_window(box, MH, MW)
        if h * w > MAX_AREA:
            out[i, 0] = 1.0
            continue
        if h * w == 0:
            continue
        v = img[y0:y0 + h, x0:x0 + w]
        ok = valid(v)
        md = model[y0:y0 + h, x0:x0 + w].astype(np.float64)
        with np.errstate(all="ignore"):
            r = (np.where(ok, v, 0).astype(np.float64) - float(bkg[i])) - md
        isl = ok & (np.asarray(masks[i], np.uint8).reshape(h, w) != 0)
        out[i, 1], out[i, 2] = ok.sum(), isl.sum()
        out[i, 3], out[i, 4] = np.sum(r[ok]), np.sum(r[ok] * r[ok])
        out[i, 5], out[i, 6], out[i, 10] = np.sum(r[isl]), np.sum(r[isl] * r[isl]), np.sum(md[isl])
        ab[i] = [np.sum(np.abs(r[ok])), np.sum(r[ok] * r[ok]), np.sum(np.abs(r[isl])), np.sum(r[isl] * r[isl]), np.sum(np.abs(md[isl]))]
        if isl.any():
            ar = np.where(isl, np.abs(r), -1.0)
            j = int(np.argmax(ar))                            # the first maximum in row-major order
            out[i, 7], out[i, 8], out[i, 9] = ar.flat[j], x0 + j % w, y0 + j // w
    return out, ab


def compare_stats(got, ref, ab, names):
    """The rule of the GPU tests for rows of cy_measure_residuals against residual_stats(): status, the two counts, the largest
    |residual| with its position and the reserved field equal; the five sums within 2 m 2^-53 sum|t_i| of the reference, m the
    number of their terms (both sides add the same float64 terms in some order)."""
    assert got.shape == ref.shape
    for i, nm in enumerate(names):
        g, r = got[i], ref[i]
        assert np.array_equal(g[[0, 1, 2, 7, 8, 9, 11]], r[[0, 1, 2, 7, 8, 9, 11]]), "%s: %s, reference %s" % (nm, g, r)
        for f, t, cnt in ((3, 0, r[1]), (4, 1, r[1]), (5, 2, r[2]), (6, 3, r[2]), (10, 4, r[2])):
            bound = 2.0 * cnt * 2.0 ** -53 * ab[i, t]
            assert abs(g[f] - r[f]) <= bound, "%s: field %d %r, reference %r, bound %g" % (nm, f, g[f], r[f], bound)
