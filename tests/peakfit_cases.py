"""Inputs of the peak-fit tests, shared by tests/test_peakfit_cpu.py (which measures the tolerance on them with the reference's
variants), tests/test_peakfit_plan_cpu.py (the planner alone) and tests/test_gpu_peakfit.py (which runs them on the GPU).  A group
is one cy_fit_peaks call: a map, a job table and max_iter; the jobs of one call see each other as neighbours, so jobs that are
meant to be alone lie more than 2 R apart.  No map is larger than 600 x 600.
  drawn      200 x 403 (MW % 4 != 0), one job per 24-pixel cell: ellipses at four angles, clean and noisy; a hole and its negated
             peak; centres of every kind; the radii around the 7-pixel limit; bad radii, signs and backgrounds; invalid pixels; an
             all-zero disc; inadmissible starts; a flat patch
  one_iter   five jobs of `drawn` with max_iter = 1
  r44, r46   the two sides of the staging switch (89 x 89 = 7921 and 93 x 93 = 8649 window pixels) on the same wide blob, with a
             neighbour each
  r256       the largest radius, 513 x 513 window pixels in 600 x 600
  neigh      what two jobs can be to each other: 5 px apart, a pixel equidistant from both, coincident, at exactly 2 R and one ulp
             inside, twelve at one distance (crowded, the 8 kept by index), and neighbours the planner turned away
  random(seed)  the crowded scene the definition was tried on: 512 x 512, noise 0.05, one blob per cell of a jittered 11 x 11 grid,
             half of them with a companion at 4 - 9 px"""
import math
from types import SimpleNamespace

import numpy as np

import peakfit_ref as PR
from fit_cases import gauss, truth_params

INF, NAN = float("inf"), float("nan")
CELL = 24
_CACHE = {}


def start_of(amp, cx, cy, sigma=1.5):
    a = 1.0 / (sigma * sigma)
    return [amp, cx, cy, a, 0.0, a]


def job(cx, cy, R, start, bkg=0.0, sign=1.0):
    return [cx, cy, R, bkg, sign] + list(start)


def radius_for(cx, cy, npix):
    """A radius whose disc around (cx, cy) holds exactly npix pixel centres (half way between two distinct distances)."""
    d2 = sorted((x - cx) ** 2 + (y - cy) ** 2 for x in range(int(cx) - 4, int(cx) + 6) for y in range(int(cy) - 4, int(cy) + 6))
    assert d2[npix - 1] < d2[npix]
    return math.sqrt(0.5 * (d2[npix - 1] + d2[npix]))


def drawn():
    """-> group: map [200, 403] float32 (0 where nothing is drawn: not valid), jobs, names, truth {job index: the six parameters}."""
    if "drawn" in _CACHE:
        return _CACHE["drawn"]
    rng = np.random.default_rng(2026)
    MH, MW = 200, 403
    amap = np.zeros((MH, MW), np.float32)
    names, jobs, truth = [], [], {}
    slot = [0]

    def cell():
        t = slot[0]
        slot[0] += 1
        assert t < (MH // CELL) * (MW // CELL)
        return CELL * (t % (MW // CELL)), CELL * (t // (MW // CELL))          # x, y of the cell's first pixel

    def stamp(x, y, a):
        amap[y:y + a.shape[0], x:x + a.shape[1]] = a.astype(np.float32)

    def add(name, j, tr=None):
        names.append(name)
        jobs.append([float(v) for v in j])
        if tr is not None:
            truth[len(jobs) - 1] = np.asarray(tr, np.float64)

    # 1. ellipses at four angles with sub-pixel centres, noiseless and with seeded noise; the centre of the job is the brightest pixel
    for nm, smaj, smin, pa in (("pa0", 2.4, 1.5, 0.0), ("pa30", 2.4, 1.5, 30.0), ("pa90", 2.4, 1.5, 90.0), ("pa135", 2.4, 1.5, 135.0)):
        for kind in ("clean", "noisy"):
            x, y = cell()
            cx, cy = 11.0 + rng.uniform(-0.5, 0.5), 11.0 + rng.uniform(-0.5, 0.5)
            g = gauss((CELL, CELL), 30.0, cx, cy, smaj, smin, pa) + 0.25
            if kind == "noisy":
                g = g + rng.normal(0.0, 0.3, g.shape)
            stamp(x, y, g)
            add("%s_%s" % (kind, nm), job(x + 11.0, y + 11.0, 8.0, start_of(28.0, x + 11.0, y + 11.0), bkg=0.25),
                truth_params(30.0, x + cx, y + cy, smaj, smin, pa) if kind == "clean" else None)
    # 2. a peak and the hole that is its negative, at the same place of their cells
    g = gauss((CELL, CELL), 20.0, 11.3, 10.8, 2.0, 1.4, 50.0) + rng.normal(0.0, 0.2, (CELL, CELL))
    for nm, sg in (("peak_of_hole", 1.0), ("hole", -1.0)):
        x, y = cell()
        stamp(x, y, sg * g.astype(np.float32).astype(np.float64))
        add(nm, job(x + 11.0, y + 11.0, 7.0, start_of(18.0, x + 11.0, y + 11.0), sign=sg))
    # 3. centres: integer, half-integer, irrational, and NaN / inf / far away
    for nm, ox, oy in (("centre_int", 11.0, 11.0), ("centre_half", 11.5, 10.5), ("centre_irr", 11.0 + math.pi / 10.0, 11.0 - math.sqrt(2.0) / 3.0)):
        x, y = cell()
        stamp(x, y, gauss((CELL, CELL), 12.0, 11.2, 11.1, 1.8, 1.8, 0.0))
        add(nm, job(x + ox, y + oy, 6.0, start_of(11.0, x + ox, y + oy)), truth_params(12.0, x + 11.2, y + 11.1, 1.8, 1.8, 0.0))
    for nm, cx, cy in (("centre_1e300", 1e300, 20.0), ("centre_nan", NAN, 20.0), ("centre_nan_y", 20.0, NAN), ("centre_inf", INF, 20.0), ("centre_minf", 20.0, -INF)):
        add(nm, job(cx, cy, 6.0, start_of(5.0, 20.0, 20.0)))
    # 4. radii: 5, 6 and 7 pixels; zero, negative, NaN, above the limit; signs and backgrounds the planner turns away
    x, y = cell()
    stamp(x, y, gauss((CELL, CELL), 25.0, 11.3, 11.2, 0.8, 0.7, 20.0))
    add("r1", job(x + 11.0, y + 11.0, 1.0, start_of(25.0, x + 11.0, y + 11.0, 0.8)))
    for npx in (6, 7):
        x, y = cell()
        stamp(x, y, gauss((CELL, CELL), 25.0, 11.3, 11.2, 0.8, 0.7, 20.0))
        add("pix%d" % npx, job(x + 11.3, y + 11.2, radius_for(11.3, 11.2, npx), start_of(25.0, x + 11.3, y + 11.2, 0.8)))
    x, y = cell()
    stamp(x, y, gauss((CELL, CELL), 9.0, 11.0, 11.0, 2.0, 2.0, 0.0))
    for nm, R in (("r0", 0.0), ("r_neg", -3.0), ("r_nan", NAN), ("r_inf", INF), ("r_above", math.nextafter(256.0, INF))):
        add(nm, job(x + 11.0, y + 11.0, R, start_of(9.0, x + 11.0, y + 11.0)))
    for nm, sg in (("sign0", 0.0), ("sign2", 2.0), ("sign_nan", NAN)):
        add(nm, job(x + 11.0, y + 11.0, 6.0, start_of(9.0, x + 11.0, y + 11.0), sign=sg))
    for nm, b in (("bkg_nan", NAN), ("bkg_inf", INF)):
        add(nm, job(x + 11.0, y + 11.0, 6.0, start_of(9.0, x + 11.0, y + 11.0), bkg=b))
    add("r0_centre_nan", job(NAN, y + 11.0, 0.0, start_of(9.0, x + 11.0, y + 11.0)))      # status 1 is decided before status 5
    # 5. NaN, 0 and +-inf pixels inside a disc; an all-zero disc
    x, y = cell()
    g = gauss((CELL, CELL), 30.0, 11.3, 10.8, 2.2, 1.7, 60.0).astype(np.float32)
    g[10, 10] = g[13, 12] = np.nan
    g[11, 13] = g[9, 9] = 0.0
    g[12, 9], g[8, 12] = np.inf, -np.inf
    stamp(x, y, g)
    add("invalid_inside", job(x + 11.0, y + 11.0, 7.0, start_of(28.0, x + 11.0, y + 11.0)))
    x, y = cell()
    add("all_zero", job(x + 11.0, y + 11.0, 6.0, start_of(5.0, x + 11.0, y + 11.0)))
    # 6. inadmissible starts, one of them on fewer than 7 pixels; a flat patch
    for t in range(4):
        x, y = cell()
        stamp(x, y, gauss((CELL, CELL), 30.0, 11.0, 11.0, 2.0, 2.0, 0.0))
        bad = start_of(30.0, x + 11.0, y + 11.0, 2.0)
        if t == 0:
            bad[0] = NAN
        elif t == 1:
            bad[0] = -1.0
        elif t == 2:
            bad[4] = bad[3]
        else:
            bad[1] = INF
        add("inadmissible%d" % t, job(x + 11.0, y + 11.0, 1.0 if t == 1 else 6.0, bad))
    x, y = cell()
    stamp(x, y, np.full((CELL, CELL), 5.0))
    add("flat", job(x + 11.0, y + 11.0, 7.0, start_of(5.0, x + 11.0, y + 11.0, 3.0)))
    # 7. at a corner, on an edge, and one pixel outside with the disc reaching in
    stamp(MW - CELL, MH - CELL, gauss((CELL, CELL), 30.0, CELL - 1.2, CELL - 0.9, 2.0, 1.5, 45.0))
    add("corner", job(MW - 1.0, MH - 1.0, 6.0, start_of(28.0, MW - 1.0, MH - 1.0)), truth_params(30.0, MW - 1.2, MH - 0.9, 2.0, 1.5, 45.0))
    stamp(MW - CELL, 96, gauss((CELL, CELL), 30.0, CELL - 1.4, 11.3, 2.0, 1.5, 120.0))
    add("edge", job(MW - 1.0, 96 + 11.0, 6.0, start_of(28.0, MW - 1.0, 96 + 11.0)), truth_params(30.0, MW - 1.4, 96 + 11.3, 2.0, 1.5, 120.0))
    stamp(MW - CELL, 48, gauss((CELL, CELL), 30.0, CELL - 0.2, 11.3, 2.0, 1.6, 70.0))
    add("outside", job(float(MW), 48 + 11.0, 6.0, start_of(28.0, float(MW), 48 + 11.0)), truth_params(30.0, MW - 0.2, 48 + 11.3, 2.0, 1.6, 70.0))
    add("outside_far", job(MW + 6.5, 48 + 11.0, 6.0, start_of(28.0, MW + 6.5, 48 + 11.0)))
    _CACHE["drawn"] = SimpleNamespace(name="drawn", map=amap, jobs=np.array(jobs, np.float64), names=names, truth=truth, max_iter=64)
    return _CACHE["drawn"]


ONE_ITER = ("clean_pa0", "noisy_pa30", "hole", "centre_irr", "corner")
STATUS_ONLY = ("flat",)           # no Gaussian in it: a, b, c run towards 0; compared on status and npix only


def one_iter():
    g = drawn()
    sel = [g.names.index(nm) for nm in ONE_ITER]
    return SimpleNamespace(name="one_iter", map=g.map, jobs=g.jobs[sel].copy(), names=list(ONE_ITER), truth={}, max_iter=1)


def _wide_map():
    if "wide" not in _CACHE:
        rng = np.random.default_rng(44)
        m = gauss((110, 210), 40.0, 54.7, 55.2, 14.0, 11.0, 25.0) + gauss((110, 210), 25.0, 120.4, 54.1, 9.0, 12.0, 100.0)
        _CACHE["wide"] = (m + rng.normal(0.0, 0.05, m.shape)).astype(np.float32)
    return _CACHE["wide"]


def staging(R):
    """R = 44: 89 x 89 window pixels, staged in LDS; R = 46: 93 x 93, membership evaluated in every sweep.  Two jobs that share."""
    jobs = [job(55.0, 55.0, float(R), start_of(38.0, 55.0, 55.0, 10.0)), job(120.0, 54.0, float(R), start_of(24.0, 120.0, 54.0, 10.0))]
    return SimpleNamespace(name="r%d" % R, map=_wide_map(), jobs=np.array(jobs, np.float64), names=["wide_a", "wide_b"], truth={}, max_iter=64)


def r256():
    if "r256" not in _CACHE:
        rng = np.random.default_rng(256)
        m = gauss((600, 600), 10.0, 300.3, 299.6, 60.0, 45.0, 35.0) + rng.normal(0.0, 0.05, (600, 600))
        p = truth_params(9.5, 300.0, 300.0, 58.0, 46.0, 33.0)
        _CACHE["r256"] = SimpleNamespace(name="r256", map=m.astype(np.float32), jobs=np.array([job(300.0, 300.0, 256.0, p)], np.float64), names=["r256"],
                                         truth={}, max_iter=64)
    return _CACHE["r256"]


def neigh():
    """-> group on a 130 x 170 map; .expect {job name: (nneigh, crowded)} for the jobs the case is about."""
    if "neigh" in _CACHE:
        return _CACHE["neigh"]
    rng = np.random.default_rng(8)
    MH, MW = 130, 170
    m = rng.normal(0.0, 0.05, (MH, MW))
    names, jobs, expect = [], [], {}

    def blob(nm, cx, cy, R=6.0, amp=8.0, sig=1.6, draw=True, **kw):
        nonlocal m
        if draw:
            m = m + gauss((MH, MW), amp, cx + 0.2, cy - 0.1, sig, sig * 0.8, 30.0)
        names.append(nm)
        jobs.append(job(cx, cy, R, start_of(amp, cx, cy), **kw))

    blob("pair5_a", 50.0, 20.3); blob("pair5_b", 54.0, 23.3, amp=5.0)             # 3-4-5: 5 px apart
    expect["pair5_a"] = expect["pair5_b"] = (1, 0)
    blob("tie_a", 20.0, 20.0); blob("tie_b", 26.0, 20.0)                          # the pixels of column 23 are equidistant
    expect["tie_a"] = expect["tie_b"] = (1, 0)
    blob("same_a", 85.0, 20.0); blob("same_b", 85.0, 20.0, draw=False)            # coincident: every pixel ties
    expect["same_a"] = expect["same_b"] = (1, 0)
    blob("at2r", 20.0, 60.0); blob("at2r_x", 32.0, 60.0); blob("at2r_y", 20.0, math.nextafter(72.0, 0.0))
    expect["at2r"], expect["at2r_x"], expect["at2r_y"] = (1, 0), (0, 0), (1, 0)    # exactly 2 R: not listed; one ulp inside: listed
    blob("crowd", 100.0, 60.0, R=8.0, amp=10.0, sig=3.0)
    for t, (ox, oy) in enumerate(((6, 8), (-6, 8), (6, -8), (-6, -8), (8, 6), (-8, 6), (8, -6), (-8, -6), (10, 0), (-10, 0), (0, 10), (0, -10))):
        blob("ring%d" % t, 100.0 + ox, 60.0 + oy, R=1.0, draw=False)    # five pixels each: status 3, but fitted jobs to the planner
    expect["crowd"] = (8, 1)
    blob("turned_away", 20.0, 100.0)
    blob("status1", 22.0, 100.0, R=-1.0, draw=False); blob("status5", 21.5, 100.5, R=0.1, draw=False)
    blob("status1_sign", 20.0, 101.0, draw=False, sign=0.0)
    expect["turned_away"] = (0, 0)
    blob("alone", 60.0, 100.0)
    expect["alone"] = (0, 0)
    _CACHE["neigh"] = SimpleNamespace(name="neigh", map=m.astype(np.float32), jobs=np.array(jobs, np.float64), names=names, truth={}, max_iter=64,
                                      expect=expect)
    return _CACHE["neigh"]


def groups():
    return [drawn(), one_iter(), staging(44), staging(46), r256(), neigh()]


SEEDS = (1, 2, 3)
GPU_SEED = 1
LEFT_OUT_MAX = 0.02          # of a random scene's jobs


def random(seed):
    """The random scene: map, jobs (R = 6, circular start of sigma 1.5 at the brightest pixel within 2 px of a blob's truth)."""
    key = "random%d" % seed
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(seed)
    N = 512
    m = rng.normal(0.0, 0.05, (N, N))
    centres = []
    for t in range(121):
        cy, cx = 36.0 + 44.0 * (t // 11) + rng.uniform(-8, 8), 36.0 + 44.0 * (t % 11) + rng.uniform(-8, 8)
        spots = [(cx, cy)]
        if rng.uniform() < 0.5:
            ang, sep = rng.uniform(0, 2 * np.pi), rng.uniform(4, 9)
            spots.append((cx + sep * np.cos(ang), cy + sep * np.sin(ang)))
        for px, py in spots:
            amp, sig, ratio, pa = rng.uniform(0.4, 3.0), rng.uniform(1.0, 2.2), rng.uniform(0.6, 1.0), rng.uniform(0, 180)
            x0, y0 = int(px) - 12, int(py) - 12
            m[y0:y0 + 25, x0:x0 + 25] += gauss((25, 25), amp, px - x0, py - y0, sig, sig * ratio, pa)
            centres.append((px, py))
    m = m.astype(np.float32)
    jobs, seen = [], set()
    for px, py in centres:
        ix, iy = int(round(px)), int(round(py))
        w = m[iy - 2:iy + 3, ix - 2:ix + 3]
        dy, dx = np.unravel_index(int(np.argmax(w)), w.shape)
        c = (ix - 2 + int(dx), iy - 2 + int(dy))
        if c in seen:                                     # two blobs with one brightest pixel are one peak
            continue
        seen.add(c)
        jobs.append(job(float(c[0]), float(c[1]), 6.0, start_of(float(m[c[1], c[0]]), float(c[0]), float(c[1]))))
    _CACHE[key] = SimpleNamespace(name=key, map=m, jobs=np.array(jobs, np.float64), names=["j%d" % i for i in range(len(jobs))], truth={}, max_iter=64)
    return _CACHE[key]


def reference(g):
    """The reference's variants on a group, computed once: list of [n, FIELDS] arrays, the kernel's association first."""
    key = "ref_" + g.name
    if key not in _CACHE:
        _CACHE[key] = PR.fit_variants(g.map, g.jobs, g.max_iter)
    return _CACHE[key]


def excluded(g):
    """Boolean [n]: the jobs a parameter comparison may leave out: the variants disagree on status, one of them stopped at a limit
    (status 2), or cond(H) of the first variant's row exceeds 1e10."""
    res = reference(g)
    _, _, differ = PR.spread(res)
    out = differ.copy()
    for e in range(out.size):
        if any(r[e, 0] == 2.0 for r in res):
            out[e] = True
        if res[0][e, 0] in (0.0, 2.0) and PR.cond_H(res[0][e]) > 1e10:
            out[e] = True
    return out
