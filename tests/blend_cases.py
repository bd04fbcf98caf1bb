"""Inputs of the joint-fit tests, shared by tests/test_blend_cpu.py (which measures the tolerance on them with the reference's
variants) and tests/test_gpu_blend.py (which runs them on the GPU).  drawn(): constructed blends, masks and starts on one
400 x 403 image (MW % 4 != 0); the starts are what measure.blend_start() would give: the single fit of tests/fit_ref.py where its
status is 0 or 2, else the moment start.  random_reference(): the 300 boxes of fit_cases.random_image() with the component
reference's masks and starts from the fit reference."""
import numpy as np

import fit_cases
import fit_ref
from fit_cases import BASE, MH, MW, Cases, gauss, moment_start, truth_params
from caesar_yolo_amd import measure

_CACHE = {}


def basins(shape, comps, g, thr, npx=None):
    """Mask of a drawn blend: the pixels with g > thr (or the npx brightest), each given to the member that contributes most."""
    parts = np.stack([gauss(shape, *c) for c in comps])
    owner = np.argmax(parts, 0) + 1
    if npx is None:
        return np.where(g > thr, owner, 0).astype(np.uint8)
    mask = np.zeros(g.size, np.uint8)
    order = np.argsort(-g.ravel(), kind="stable")[:npx]
    mask[order] = owner.ravel()[order]
    return mask.reshape(shape)


def single_starts(img, box, bkg, ncomp, mask, max_iter=64):
    """(start [ncomp, 6], single-fit rows [16, 32]): per component the single fit's parameters when its status is 0 or 2, else the
    moment start."""
    x0, y0, h, w = measure.box_window(box, *img.shape)
    win = img[y0:y0 + h, x0:x0 + w]
    s = np.zeros((16, 6))
    for k in range(ncomp):
        s[k] = moment_start(win, mask.reshape(h, w), k, bkg, x0, y0)
    rows = fit_ref.fit_components(img, [box], [bkg], [ncomp], s[None], [mask], max_iter)[0]
    use = np.isin(rows[:ncomp, 0], (0.0, 2.0))
    out = s[:ncomp].copy()
    out[use] = rows[:ncomp, 5:11][use]
    return out, rows


def drawn():
    """-> (image [400, 403] float32, Cases with .truth {case: [M, 6]}, .single {case: rows [16, 32]}, .noisy {case, ..})."""
    if "drawn" in _CACHE:
        return _CACHE["drawn"]
    rng = np.random.default_rng(77)
    img = np.full((MH, MW), BASE, np.float32)
    c = Cases()
    c.single, c.noisy = {}, set()
    shelf = {"x": 0, "y": 0, "h": 0}

    def place(h, w):
        if shelf["x"] + w > MW:
            shelf["x"], shelf["y"], shelf["h"] = 0, shelf["y"] + shelf["h"] + 1, 0
        y, x = shelf["y"], shelf["x"]
        shelf["x"], shelf["h"] = x + w + 1, max(shelf["h"], h)
        assert y + h <= MH - 24, "the last rows belong to the corner case"
        return y, x

    def put(y, x, a):
        img[y:y + a.shape[0], x:x + a.shape[1]] = a.astype(np.float32)
        return [x, y, x + a.shape[1] - 1, y + a.shape[0] - 1]

    def blend(name, shape, comps, noise=0.0, thr=0.5, npx=None, truth=True, edit=None, at=None, box=None, ncomp=None, mask=None):
        y, x = place(*shape) if at is None else at
        g = sum(gauss(shape, *cc) for cc in comps)
        if noise:
            g = g + rng.normal(0.0, noise, g.shape)
        g = g.astype(np.float32)
        if edit is not None:
            edit(g)
        b = put(y, x, g)
        box = b if box is None else box
        mask = basins(shape, comps, g, thr, npx) if mask is None else mask
        ncomp = len(comps) if ncomp is None else ncomp
        start, rows = single_starts(img, box, 0.0, ncomp, mask)
        i = c.add(name, box, 0.0, ncomp, start, mask)
        c.single[i] = rows
        if truth and not noise:
            c.truth[i] = np.array([truth_params(cc[0], x + cc[1], y + cc[2], *cc[3:]) for cc in comps])
        if noise:
            c.truth[i] = np.array([truth_params(cc[0], x + cc[1], y + cc[2], *cc[3:]) for cc in comps])
            c.noisy.add(i)
        return i

    # 1. a pair at three separations, clean and with noise; a pair of ellipses at different angles
    pairs = {"resolved": [(40.0, 10.3, 11.8, 2.0, 2.0, 0.0), (30.0, 18.1, 12.4, 2.0, 2.0, 0.0)],
             "overlap": [(40.0, 11.2, 12.1, 2.0, 2.0, 0.0), (32.0, 16.3, 11.6, 2.0, 2.0, 0.0)],
             "unequal": [(50.0, 10.8, 12.2, 2.0, 2.0, 0.0), (8.0, 17.4, 11.7, 2.0, 2.0, 0.0)],
             "ellipses": [(40.0, 10.6, 12.3, 3.0, 1.6, 30.0), (35.0, 18.2, 11.5, 2.6, 1.5, 120.0)]}
    for nm, comps in pairs.items():
        blend("pair_" + nm, (24, 29), comps)
        if nm != "ellipses":
            blend("noisy_" + nm, (24, 29), comps, noise=0.3, thr=1.0)
    # 2. chains of 3, 4 and 5 (the last one: status 5 on all five); two disjoint pairs; a pair and a lone component
    chain = [(40.0 - 3 * k, 8.4 + 5.6 * k, 11.7 + 0.4 * (k % 2), 2.0, 1.7, 20.0 * k) for k in range(5)]
    blend("chain3", (24, 30), chain[:3])
    blend("chain4", (24, 36), chain[:4])
    blend("chain5", (24, 42), chain, truth=False)
    two = [(40.0, 6.3, 7.2, 1.6, 1.6, 0.0), (30.0, 11.1, 7.7, 1.6, 1.6, 0.0), (35.0, 27.2, 15.8, 1.6, 1.6, 0.0), (28.0, 32.3, 15.1, 1.6, 1.6, 0.0)]
    blend("two_pairs", (24, 40), two, thr=1.0, truth=False)
    blend("pair_lone", (24, 40), two[:3], thr=1.0, truth=False)
    # 3. constructed masks on a smooth blend: touching only diagonally (one group); separated by one row of byte 0 (two singles);
    #    a component whose only neighbours are byte 255 (single)
    comps = [(30.0, 6.2, 6.1, 2.0, 2.0, 0.0), (30.0, 13.8, 13.9, 2.0, 2.0, 0.0)]
    m = np.zeros((20, 20), np.uint8)
    m[2:10, 2:10], m[10:18, 10:18] = 1, 2
    blend("diagonal", (20, 20), comps, mask=m, truth=False)
    comps = [(30.0, 10.0, 5.0, 2.0, 2.0, 0.0), (30.0, 10.0, 14.0, 2.0, 2.0, 0.0)]
    m = np.zeros((20, 20), np.uint8)
    m[1:9, 3:17], m[10:18, 3:17] = 1, 2
    blend("row_gap", (20, 20), comps, mask=m, truth=False)
    m = np.zeros((20, 20), np.uint8)
    m[1:9, 3:17], m[9, 3:17], m[10:18, 3:17] = 1, 255, 2
    blend("only_255", (20, 20), comps, mask=m, truth=False)

    # 4. NaN and zero pixels inside a member's basin
    def holes(g):
        g[12, 10] = g[11, 17] = g[9, 9] = np.nan
        g[12, 12] = g[13, 18] = 0.0
    blend("invalid_inside", (24, 29), pairs["resolved"], edit=holes, truth=False)
    # 5. exactly 12 and 13 valid pixels in the pair (status 3 / fitted); a member with fewer than 7 pixels, whose single fit has
    #    status 3 and whose start is the moment start
    tight = [(40.0, 6.2, 6.8, 1.3, 1.3, 0.0), (34.0, 9.9, 7.3, 1.3, 1.3, 0.0)]
    blend("pix12", (14, 16), tight, npx=12, truth=False)
    blend("pix13", (14, 16), tight, npx=13, truth=False)
    m = basins((24, 29), pairs["unequal"], sum(gauss((24, 29), *cc) for cc in pairs["unequal"]), 0.5)
    yy, xx = np.mgrid[0:24, 0:29]                           # the five pixels of the second basin that lie nearest to the first member
    keep = np.argsort(np.where(m == 2, (xx - 10.8) ** 2 + (yy - 12.2) ** 2, np.inf).ravel(), kind="stable")[:5]
    m2 = np.where(m == 2, 0, m).astype(np.uint8)
    m2.ravel()[keep] = 2
    i = blend("single_status3", (24, 29), pairs["unequal"], mask=m2, truth=False)
    assert c.single[i][1, 0] == 3.0
    # 6. one member's start inadmissible (status 4: the starts come back bit for bit)
    i = blend("inadmissible", (24, 29), pairs["resolved"], truth=False)
    c.start[i][1, 3] = -0.25
    # 7. list lengths around the chunk of 128 entries and around the LDS-resident 4096
    wide = [(60.0, 30.2, 40.3, 11.0, 9.0, 25.0), (45.0, 52.7, 38.8, 9.0, 8.0, 100.0)]
    for npx in (128, 129, 300):
        blend("chunk%d" % npx, (24, 29), pairs["resolved"], npx=npx, truth=False)
    at = place(80, 80)
    for npx in (4096, 4097, 6400):
        blend("wide%d" % npx, (80, 80), wide, npx=npx, truth=False, at=at)
    # 8. sixteen components in one box: one group of 5, three pairs and five singles
    g16 = []
    cells = {0: (5, 5), 1: (9, 5), 2: (13, 5), 3: (17, 5), 4: (21, 5),            # a chain of 5
             5: (5, 15), 6: (9, 15), 7: (17, 15), 8: (21, 15), 9: (29, 15), 10: (33, 15),      # three pairs
             11: (31, 4), 12: (40, 4), 13: (5, 25), 14: (15, 25), 15: (25, 25)}                   # five singles
    m = np.zeros((31, 46), np.uint8)
    for k, (cx, cy) in cells.items():
        g16.append((20.0 + k, cx + 0.1 * k, cy - 0.05 * k, 1.5, 1.3, 11.0 * k))
        m[cy - 3:cy + 4, cx - 2:cx + 2] = k + 1
    blend("sixteen", (31, 46), g16, mask=m, truth=False)
    # 9. no components; an empty window; a window clipped at the image's last corner
    c.add("ncomp0", [50, 100, 60, 110], 0.0, 0, None, np.zeros((11, 11), np.uint8))
    c.add("empty", [MW + 5, 10, MW + 20, 30], 0.0, 2, [[10.0, MW + 10.0, 20.0, 0.25, 0.0, 0.25]] * 2, np.zeros((0, 0), np.uint8))
    blend("corner", (20, 26), [(40.0, 8.3, 9.1, 2.0, 2.0, 0.0), (30.0, 15.6, 10.2, 2.0, 2.0, 0.0)], at=(MH - 20, MW - 26),
          box=[MW - 26.5, MH - 20.5, MW + 6.0, MH + 4.0], truth=False)
    _CACHE["drawn"] = (img, c)
    return img, c


ONE_ITER = ("pair_resolved", "noisy_overlap", "chain4", "wide4097")      # also run with max_iter = 1
# what the member rows of a drawn case must report
STATUS = {"chain5": [5] * 5, "pair_lone": [0, 0, 6], "row_gap": [6, 6], "only_255": [6, 6], "pix12": [3, 3], "inadmissible": [4, 4],
          "empty": [6, 6], "sixteen": [5] * 5 + [None] * 6 + [6] * 5,
          "single_status3": [None, None]}           # None: fitted, whatever status the reference ends with
GROUPS = {"two_pairs": [0, 0, 2, 2], "diagonal": [0, 0], "sixteen": [0] * 5 + [5, 5, 7, 7, 9, 9, 11, 12, 13, 14, 15]}


def drawn_reference():
    """(img, cases, (results per variant, cond) at max_iter 64, indices of ONE_ITER, the same at max_iter 1)."""
    if "dref" not in _CACHE:
        import blend_ref
        img, c = drawn()
        one = [c.names.index(nm) for nm in ONE_ITER]
        _CACHE["dref"] = (img, c, blend_ref.fit_variants(img, *c.arrays()), one, blend_ref.fit_variants(img, *c.arrays(one), max_iter=1))
    return _CACHE["dref"]


def random_starts(fit_rows, start):
    """measure.blend_start() given fit rows and the moment starts they began from."""
    out = np.array(start, np.float64)
    use = np.isin(fit_rows[:, :, 0], (0.0, 2.0))
    out[use] = fit_rows[:, :, 5:11][use]
    return out


def random_reference():
    """The random scene of the fit tests with the joint reference's variants, computed once:
    (img, boxes, thr4, (bkg, ncomp, blend starts, masks), (results per variant, cond))."""
    if "rref" not in _CACHE:
        import blend_ref
        img, boxes, thr4, (bkg, ncomp, start, masks), rr = fit_cases.random_reference()
        bstart = random_starts(rr[0], start)
        _CACHE["rref"] = (img, boxes, thr4, (bkg, ncomp, bstart, masks), blend_ref.fit_variants(img, boxes, bkg, ncomp, bstart, masks))
    return _CACHE["rref"]


def excluded(results, cond, ncomp):
    """Boolean [n, 16]: the member rows the random comparison may leave out: the variants disagree on the status, or cond(H) of
    the first variant's job exceeds 1e10."""
    import blend_ref
    differ = blend_ref.spread(results, ncomp)[3]
    rows = np.arange(16)[None, :] < np.asarray(ncomp).reshape(-1, 1)
    fitted = rows & np.isin(results[0][:, :, 0], (0.0, 2.0))
    return differ | (fitted & (cond > 1e10))
