"""Inputs of the component-fit tests, shared by tests/test_fit_cpu.py (which measures the tolerance on them with the reference's
variants) and tests/test_gpu_fit.py (which runs them on the GPU).  drawn(): constructed stamps, masks and starts on one
400 x 403 image (MW % 4 != 0).  random_scene(): a 512 x 512 synth image with blended pairs and 300 random boxes; its masks, rows
and starts come from the component step (the GPU's in the GPU test, tests/deblend_ref.py's here: they are equal, bytes and rows
up to the sums' rounding, by tests/test_gpu_deblend.py)."""
import numpy as np

import deblend_ref
import measure_ref
from caesar_yolo_amd import measure
from caesar_yolo_amd.measure import box_window

MH, MW = 400, 403
BASE = np.float32(0.001)
_CACHE = {}


def gauss(shape, amp, cx, cy, smaj, smin, pa_deg):
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    t = np.radians(pa_deg)
    u = (xx - cx) * np.cos(t) + (yy - cy) * np.sin(t)
    v = -(xx - cx) * np.sin(t) + (yy - cy) * np.cos(t)
    return amp * np.exp(-0.5 * ((u / smaj) ** 2 + (v / smin) ** 2))


def truth_params(amp, cx, cy, smaj, smin, pa_deg):
    t = np.radians(pa_deg)
    R = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    P = np.linalg.inv(R @ np.diag([smaj ** 2, smin ** 2]) @ R.T)
    return np.array([amp, cx, cy, P[0, 0], P[0, 1], P[1, 1]])


def moment_start(win, mask, k, bkg, x0, y0):
    """fit_start() on the component row a numpy float64 pass over the mask gives (peak, peak position and the six sums)."""
    yy, xx = np.nonzero(mask == k + 1)
    v = win[yy, xx]
    ok = (v != 0) & np.isfinite(v)
    yy, xx, v = yy[ok], xx[ok], v[ok].astype(np.float64)
    row = np.zeros(12)
    if v.size:
        j = int(np.argmax(v))
        w = v - bkg
        row[:] = [v.size, v[j], x0 + xx[j], y0 + yy[j], w.sum(), (w * xx).sum(), (w * yy).sum(), (w * xx * xx).sum(), (w * yy * yy).sum(),
                  (w * xx * yy).sum(), 1, 1]
    return measure.fit_start(row, bkg, (x0, y0))


class Cases:
    def __init__(self):
        self.names, self.boxes, self.bkg, self.ncomp, self.start, self.masks, self.truth = [], [], [], [], [], [], {}

    def add(self, name, box, bkg, ncomp, start, mask):
        s = np.zeros((16, 6))
        if ncomp:
            s[:ncomp] = np.asarray(start, np.float64).reshape(ncomp, 6)
        self.names.append(name); self.boxes.append([float(v) for v in box]); self.bkg.append(float(bkg)); self.ncomp.append(int(ncomp))
        self.start.append(s); self.masks.append(np.ascontiguousarray(mask, np.uint8))
        return len(self.names) - 1

    def arrays(self, sel=None):
        idx = range(len(self.names)) if sel is None else sel
        return (np.array([self.boxes[i] for i in idx], np.float64).reshape(-1, 4), np.array([self.bkg[i] for i in idx], np.float64),
                np.array([self.ncomp[i] for i in idx], np.int32), np.array([self.start[i] for i in idx], np.float64).reshape(-1, 16, 6),
                [self.masks[i] for i in idx])


def drawn():
    """-> (image [400, 403] float32 with NaN and 0 pixels, Cases).  Every window lies where nothing else was drawn."""
    if "drawn" in _CACHE:
        return _CACHE["drawn"]
    rng = np.random.default_rng(2024)
    img = np.full((MH, MW), BASE, np.float32)
    c = Cases()

    def put(y, x, a):
        img[y:y + a.shape[0], x:x + a.shape[1]] = a.astype(np.float32)
        return [x, y, x + a.shape[1] - 1, y + a.shape[0] - 1]

    def full_box(name, y, x, a, mask=None, bkg=0.0, start=None):
        box = put(y, x, a)
        mask = np.ones(a.shape, np.uint8) if mask is None else mask
        win = img[y:y + a.shape[0], x:x + a.shape[1]]
        return c.add(name, box, bkg, 1, moment_start(win, mask, 0, bkg, x, y) if start is None else start, mask)

    # 1. circular and rotated ellipses with sub-pixel centres, noiseless and with seeded unit noise under a 3-sigma mask
    shapes = [("circ", 2.0, 2.0, 0.0), ("pa0", 3.0, 1.6, 0.0), ("pa30", 3.0, 1.6, 30.0), ("pa90", 3.0, 1.6, 90.0), ("pa135", 3.0, 1.6, 135.0)]
    for t, (nm, smaj, smin, pa) in enumerate(shapes):
        cx, cy = 10.0 + rng.uniform(-0.5, 0.5), 10.0 + rng.uniform(-0.5, 0.5)
        g = gauss((21, 21), 40.0, cx, cy, smaj, smin, pa)
        i = full_box("clean_" + nm, 0, 25 * t, g)
        c.truth[i] = truth_params(40.0, 25 * t + cx, cy, smaj, smin, pa)
        noisy = (g + rng.normal(0.0, 1.0, g.shape)).astype(np.float32)
        full_box("noisy_" + nm, 25, 25 * t, noisy, (noisy > 3.0).astype(np.uint8))
    # NaN and zero pixels inside a mask
    g = gauss((21, 21), 30.0, 10.3, 9.8, 2.5, 1.8, 60.0).astype(np.float32)
    g[9, 9] = g[12, 11] = g[5, 5] = np.nan
    g[10, 12] = g[8, 8] = 0.0
    full_box("invalid_inside", 50, 0, g)
    # 2. two blended Gaussians, basins from the component reference; 16 components in one box; a source without components
    g = gauss((21, 31), 50.0, 10.2, 10.1, 2.0, 2.0, 0.0) + gauss((21, 31), 35.0, 17.6, 11.3, 2.2, 1.7, 20.0)
    g = g + rng.normal(0.0, 0.05, g.shape)
    box = put(75, 0, g)
    row, comp, mask, _ = deblend_ref.deblend_one(img, box, [0.5, 0.25, 0.0, 0.5], 8, 2)
    assert row[3] == 2
    c.add("blend2", box, 0.0, 2, measure.fit_start(comp[:2], 0.0, (0, 75)), mask)
    g, mask = np.zeros((44, 44)), np.zeros((44, 44), np.uint8)
    for k in range(16):
        ky, kx = divmod(k, 4)
        g += gauss((44, 44), 20.0 + k, 6.0 + 10 * kx + 0.1 * k, 6.5 + 10 * ky - 0.05 * k, 1.6, 1.3, 11.0 * k)
        mask[2 + 10 * ky:12 + 10 * ky, 2 + 10 * kx:12 + 10 * kx] = k + 1
    mask[0, :] = 255                                            # unassigned pixels belong to no job
    box = put(100, 0, g)
    c.add("sixteen", box, 0.0, 16, [moment_start(img[100:144, 0:44], mask, k, 0.0, 0, 100) for k in range(16)], mask)
    c.add("ncomp0", [50, 100, 60, 110], 0.0, 0, None, np.zeros((11, 11), np.uint8))
    # 3. 6 and 7 pixels; four inadmissible starts; a flat patch
    g = gauss((9, 9), 25.0, 4.2, 3.9, 1.5, 1.5, 0.0)
    for npx, x in ((6, 70), (7, 85)):
        mask = np.zeros((9, 9), np.uint8)
        order = np.argsort(-g.ravel(), kind="stable")[:npx]
        mask.ravel()[order] = 1
        full_box("pix%d" % npx, 100, x, g, mask)
    g = gauss((21, 21), 30.0, 10.0, 10.0, 2.0, 2.0, 0.0)
    mask = np.zeros((21, 21), np.uint8)
    mask[:10, :10], mask[:10, 10:], mask[10:, :10], mask[10:, 10:] = 1, 2, 3, 4
    good = [30.0, 110.0, 110.0, 0.25, 0.0, 0.25]
    bad = [list(good) for _ in range(4)]
    bad[0][0] = np.nan
    bad[1][0] = -1.0
    bad[2][4] = 0.25
    bad[3][1] = np.inf
    c.add("inadmissible", put(100, 100, g), 0.0, 4, bad, mask)
    full_box("flat", 100, 130, np.full((15, 15), 5.0), start=[5.0, 137.0, 107.0, 1.0 / 9.0, 0.0, 1.0 / 9.0])
    # 4. a box that leaves the image at its last corner; an empty window
    g = gauss((18, 20), 30.0, 9.4, 8.7, 2.0, 1.5, 45.0)
    put(MH - 18, MW - 20, g)
    mask = np.ones((18, 20), np.uint8)
    c.add("corner", [MW - 20.5, MH - 18.5, MW + 6.0, MH + 4.0], 0.0, 1, moment_start(img[MH - 18:, MW - 20:], mask, 0, 0.0, MW - 20, MH - 18), mask)
    c.add("empty", [MW + 5, 10, MW + 20, 30], 0.0, 1, [[10.0, MW + 10.0, 20.0, 0.25, 0.0, 0.25]], np.zeros((0, 0), np.uint8))
    # 5. the LDS boundary: 4096 and 4097 pixels of one wide Gaussian, and all of its 80 x 80 = 6400
    g = gauss((80, 80), 60.0, 39.7, 40.2, 14.0, 11.0, 25.0)
    box = put(150, 0, g)
    yy, xx = np.mgrid[0:80, 0:80]
    order = np.argsort(((yy - 40) ** 2 + (xx - 40) ** 2).ravel(), kind="stable")
    win = img[150:230, 0:80]
    for npx in (4096, 4097, 6400):
        mask = np.zeros(6400, np.uint8)
        mask[order[:npx]] = 1
        mask = mask.reshape(80, 80)
        c.add("wide%d" % npx, box, 0.0, 1, moment_start(win, mask, 0, 0.0, 0, 150), mask)
    _CACHE["drawn"] = (img, c)
    return img, c


STATUS_ONLY = ("flat",)           # no Gaussian in it: a, b, c run towards 0 and cond(H) = 3e33; compared on status, npix and niter
ONE_ITER = ("clean_circ", "clean_pa30", "noisy_pa90", "blend2", "wide4097")      # also run with max_iter = 1


N_RANDOM, SEED_RANDOM = 300, 5
MIN_STATUS0, MIN_MULTI = 200, 40         # floors on the reference's status-0 jobs and multi-component sources


def random_image():
    """512 x 512 synth image (noise only: no sources of its own, no NaN strip, no zero block) with 121 blended pairs drawn in."""
    if "rimg" in _CACHE:
        return _CACHE["rimg"]
    from caesar_yolo_amd import synth
    img = synth.make_mosaic(n=512, seed=SEED_RANDOM, nsrc=0, next_=0, nan_strip=0, zero_block=0)
    q = img.astype(np.float64)
    noise = 1.4826 * np.median(np.abs(q - np.median(q)))
    rng = np.random.default_rng(SEED_RANDOM)
    centres = []
    for t in range(121):                                  # one pair per cell of an 11 x 11 grid: pairs do not overlap each other
        cy, cx = 36.0 + 44.0 * (t // 11) + rng.uniform(-6, 6), 36.0 + 44.0 * (t % 11) + rng.uniform(-6, 6)
        ang, sep = rng.uniform(0, np.pi), rng.uniform(4, 8)
        for (py, px) in ((cy, cx), (cy + sep * np.sin(ang), cx + sep * np.cos(ang))):
            amp, smaj, smin, pa = rng.uniform(15, 60) * noise, rng.uniform(1.2, 2.5), rng.uniform(1.0, 1.2), rng.uniform(0, 180)
            y0, x0 = int(py) - 10, int(px) - 10
            img[y0:y0 + 21, x0:x0 + 21] += gauss((21, 21), amp, px - x0, py - y0, smaj, smin, pa).astype(np.float32)
        centres.append((cy + 0.5 * sep * np.sin(ang), cx + 0.5 * sep * np.cos(ang)))
    # flux unit: a typical source has an amplitude of order 1 (noise = 1 / 32), so that cond(H), which mixes the amplitude's
    # column with the shape's, measures the geometry of a job and not the unit of the image
    img = (img.astype(np.float64) / (32.0 * noise)).astype(np.float32)
    boxes = []
    for t in range(N_RANDOM):
        cy, cx = centres[t % len(centres)]
        hw, hh = rng.uniform(8, 14, 2)
        boxes.append([cx - hw + rng.uniform(-2, 2), cy - hh + rng.uniform(-2, 2), cx + hw, cy + hh])
    _CACHE["rimg"] = (img, np.array(boxes, np.float64))
    return _CACHE["rimg"]


def random_thresholds(img, boxes):
    """[n, 4] thresholds bkg + 10 rms / bkg + 2.5 rms / bkg / bkg + 10 rms from the reference's measurement rows (ring 8)."""
    if "rthr" not in _CACHE:
        _CACHE["rthr"] = deblend_ref.thresholds(measure_ref.measure(img, boxes, 8)[0], 10.0, 2.5, 10.0)
    return _CACHE["rthr"]


def random_inputs(img, boxes, thr4, rows, comp):
    """(bkg, ncomp, start) of the fit from the component step's rows, as measure.Chain.fit forms them."""
    win0 = np.array([box_window(b, img.shape[0], img.shape[1])[:2] for b in boxes], np.float64).reshape(-1, 2)
    return thr4[:, 2].copy(), rows[:, 3].astype(np.int32), measure.fit_start(comp, thr4[:, 2], win0)


def random_reference():
    """The random scene with the component reference's masks and the fit reference's variants, computed once:
    (img, boxes, thr4, (bkg, ncomp, start, masks), results per variant)."""
    if "rref" not in _CACHE:
        import fit_ref
        img, boxes = random_image()
        thr4 = random_thresholds(img, boxes)
        rows, comp, masks, _ = deblend_ref.deblend(img, boxes, thr4, 8, 2)
        bkg, ncomp, start = random_inputs(img, boxes, thr4, rows, comp)
        _CACHE["rref"] = (img, boxes, thr4, (bkg, ncomp, start, masks), fit_ref.fit_variants(img, boxes, bkg, ncomp, start, masks))
    return _CACHE["rref"]


def drawn_reference():
    """(img, cases, results per variant at max_iter 64, indices of ONE_ITER, their results per variant at max_iter 1)."""
    if "dref" not in _CACHE:
        import fit_ref
        img, c = drawn()
        one = [c.names.index(nm) for nm in ONE_ITER]
        _CACHE["dref"] = (img, c, fit_ref.fit_variants(img, *c.arrays()), one, fit_ref.fit_variants(img, *c.arrays(one), max_iter=1))
    return _CACHE["dref"]


def excluded(results, ncomp):
    """Boolean [n, 16]: the jobs the random comparison may leave out: the variants disagree on status, or cond(H) of the first
    variant's row exceeds 1e10."""
    import fit_ref
    _, _, differ = fit_ref.spread(results, ncomp)
    out = differ.copy()
    for i in range(out.shape[0]):
        for k in range(int(ncomp[i])):
            if results[0][i, k, 0] in (0.0, 2.0) and fit_ref.cond_H(results[0][i, k]) > 1e10:
                out[i, k] = True
    return out
