"""Inputs of the forced-photometry tests (tests/test_forced_cpu.py, tests/test_forced_plan_cpu.py, tests/test_gpu_forced.py): small maps with
jobs that reach every status and every rule of cy_forced_fit, and the random scene of planted Gaussians."""
import math
from collections import namedtuple

import numpy as np

import forced_ref as FR

Group = namedtuple("Group", "name map rms jobs nsigma fit_bkg offset names big")
NAN, INF = float("nan"), float("inf")


def shape(smaj, smin, theta):
    """a, b, c of exp(-q / 2), q = a u^2 + 2 b u v + c v^2, for sigmas smaj, smin and the position angle theta of the major axis."""
    co, si = math.cos(theta), math.sin(theta)
    ia, ib = 1.0 / (smaj * smaj), 1.0 / (smin * smin)
    return co * co * ia + si * si * ib, si * co * (ia - ib), si * si * ia + co * co * ib


def job(x0, y0, smaj=1.5, smin=1.5, theta=0.0, bkg=0.0):
    return [x0, y0, *shape(smaj, smin, theta), bkg]


def plant(img, jb, amp):
    MH, MW = img.shape
    px, py = np.arange(MW, dtype=np.float64)[None, :], np.arange(MH, dtype=np.float64)[:, None]
    img += (amp * np.exp(-0.5 * FR._q([float(v) for v in jb], px, py))).astype(img.dtype)


def ellipse(jb, nsigma, MH, MW):
    px, py = np.arange(MW, dtype=np.float64)[None, :], np.arange(MH, dtype=np.float64)[:, None]
    return FR._q([float(v) for v in jb], px, py) <= nsigma * nsigma


def main_scene():
    """-> (img float32 [64, 96], rms float32, jobs, names)."""
    MH, MW = 64, 96
    rng = np.random.default_rng(7)
    img = rng.standard_normal((MH, MW)) + 0.3
    jobs, names = [], []

    def add(name, jb, amp=None):
        jobs.append(jb)
        names.append(name)
        if amp is not None:
            plant(img, jb, amp)
    add("isolated", job(20.3, 15.6, 2.0, 1.4, 0.5, 0.3), 25.0)
    add("pair_a", job(50.2, 14.1, 1.8, 1.2, 1.0, 0.3), 20.0)
    add("pair_b", job(53.2, 14.4, 1.3, 1.3, 0.0, 0.3), 12.0)
    add("corner", job(0.4, 0.3, 1.5, 1.5, 0.0, 0.3), 15.0)
    add("misses", job(-40.0, 20.0))
    add("centre_1e300", job(1e300, 20.0))
    add("nan_x0", job(NAN, 20.0))
    add("negative_a", [30.0, 20.0, -0.4, 0.0, 0.4, 0.0])
    add("bb_ge_ac", [30.0, 20.0, 0.4, 0.4, 0.4, 0.0])
    add("inf_bkg", job(30.0, 20.0, bkg=INF))
    add("bad_pixels", job(75.5, 16.2, 2.0, 2.0, 0.0, 0.3), 18.0)
    add("no_valid_pixel", job(10.0, 40.0, 0.7, 0.7))
    add("npix_K_minus_1", job(25.0, 40.0, 0.7, 0.7))
    for t in range(2):
        add("dup2_%d" % t, job(40.5, 40.2, 1.5, 1.2, 0.3, 0.3), 10.0 if t == 0 else None)
    for t in range(3):
        add("dup3_%d" % t, job(55.5, 40.5, 1.4, 1.4, 0.0, 0.3), 14.0 if t == 0 else None)
    add("dup3_neighbour", job(58.0, 41.0, 1.2, 1.2, 0.0, 0.3), 9.0)
    add("close_a", job(80.0, 42.0, 1.5, 1.5, 0.0, 0.3), 16.0)
    add("close_b", job(80.0 + 1e-9, 42.0, 1.5, 1.5, 0.0, 0.3))
    add("close_third", job(83.0, 42.5, 1.3, 1.3, 0.0, 0.3), 11.0)
    # ten components inside one another's rectangles: a centre and a ring; +-2.5 px in x tie in distance from the centre
    ring = [(0.0, 0.0), (2.5, 0.0), (-2.5, 0.0), (0.0, 3.0), (0.0, -3.5), (3.0, 3.0), (-3.0, 3.2), (3.2, -3.0), (-3.4, -3.1), (5.0, 0.5)]
    for t, (dx, dy) in enumerate(ring):
        add("crowd_%d" % t, job(30.0 + dx, 54.0 + dy, 1.1, 1.0, 0.2 * t, 0.3), 8.0 + t)
    img = img.astype(np.float32)
    rms = (1.0 + 0.2 * rng.random((MH, MW))).astype(np.float32)
    img[16, 75], img[17, 76], img[15, 75], img[16, 77] = NAN, INF, -INF, 0.0
    img[ellipse(jobs[names.index("no_valid_pixel")], 8.0, MH, MW)] = 0.0
    e = ellipse(jobs[names.index("npix_K_minus_1")], 8.0, MH, MW)
    keep = img[40, 25]
    img[e] = 0.0
    img[40, 25] = keep if keep != 0 else 1.0
    rms[15, 20], rms[16, 21], rms[15, 21], rms[16, 19] = 0.0, NAN, -1.0, INF
    return img, rms, np.array(jobs, np.float64), names


def random_scene(seed=1):
    """The scene of the issue: 512 x 512, unit noise plus 0.3, one to three components per cell of a jittered 11 x 11 grid.
    -> (img float32, rms float32 (ones), jobs [n, 6] with bkg 0, truth [n])."""
    rng = np.random.default_rng(seed)
    MH = MW = 512
    img = rng.standard_normal((MH, MW)) + 0.3
    jobs, truth = [], []
    for gy in range(11):
        for gx in range(11):
            cx, cy = 26.0 + 46.0 * gx + rng.uniform(-6, 6), 26.0 + 46.0 * gy + rng.uniform(-6, 6)
            for t in range(int(rng.integers(1, 4))):
                x, y = (cx, cy) if t == 0 else (cx + rng.uniform(-7, 7), cy + rng.uniform(-7, 7))
                smaj = rng.uniform(1.2, 3.0)
                jb = job(x, y, smaj, rng.uniform(1.0, smaj), rng.uniform(0, math.pi), 0.0)
                amp = rng.uniform(5, 50)
                plant(img, jb, amp)
                jobs.append(jb)
                truth.append(amp)
    return img.astype(np.float32), np.ones((MH, MW), np.float32), np.array(jobs, np.float64), np.array(truth)


def capped_scene():
    rng = np.random.default_rng(11)
    img = (rng.standard_normal((520, 515)) + 0.3).astype(np.float32)
    jb = job(257.5, 257.0, 200.0, 200.0, 0.0, 0.3)
    small = job(300.2, 250.7, 2.0, 1.5, 0.4, 0.3)
    img64 = img.astype(np.float64)
    plant(img64, jb, 6.0)
    plant(img64, small, 20.0)
    return img64.astype(np.float32), np.array([jb, small], np.float64), ["sigma_200", "inside_it"]


CHAIN_SIDE, CHAIN_NU, CHAIN_ALPHA = 160, (1.0e9, 2.5e9), -0.7
CHAIN_PLANTED = ((60.0, 40.3, 40.6, 2.0), (45.0, 115.2, 42.1, 2.2), (80.0, 42.4, 112.7, 1.8), (55.0, 112.0, 114.5, 2.1))     # amplitude, x, y, sigma


def chain_scene():
    """-> (image float32 [160, 160], second map float32, the source list).  The image: unit noise from a fixed seed and four clean,
    isolated circular Gaussians, each in a hand-made box.  The second map holds the same sources scaled by (nu2 / nu1)^-0.7 on
    noise of sigma 0.02 from another seed: as good as noise-free, but not free of it, because a pixel that is exactly 0 counts as
    blank and a map of exact zeros away from its sources would have no background mesh."""
    yy, xx = np.mgrid[0:CHAIN_SIDE, 0:CHAIN_SIDE].astype(np.float64)
    img = np.random.default_rng(31).standard_normal((CHAIN_SIDE, CHAIN_SIDE))
    second = 0.02 * np.random.default_rng(32).standard_normal((CHAIN_SIDE, CHAIN_SIDE))
    scale = (CHAIN_NU[1] / CHAIN_NU[0]) ** CHAIN_ALPHA
    sources = []
    for i, (amp, x0, y0, sig) in enumerate(CHAIN_PLANTED):
        g = np.exp(-((xx - x0) ** 2 + (yy - y0) ** 2) / (2 * sig ** 2))
        img += amp * g
        second += scale * amp * g
        sources.append({"name": "S%d" % (i + 1), "x1": round(x0) - 12.0, "y1": round(y0) - 12.0, "x2": round(x0) + 12.0, "y2": round(y0) + 12.0})
    return img.astype(np.float32), second.astype(np.float32), sources


CHAIN_CONFIG = {"bkg_map": True, "bkg_cell": 32, "residual_map": True, "forced_fit": True, "image_path": "scene.fits"}

_groups = None


def groups():
    global _groups
    if _groups is not None:
        return _groups
    img, rms, jobs, names = main_scene()
    g = [Group("main_64x96", img, rms, jobs, 3.0, 1, False, names, False),
         Group("main_offset", img, rms, jobs, 3.0, 1, True, names, False),
         Group("main_no_rms", img, None, jobs, 3.0, 1, False, names, False),
         Group("main_no_bkg", img, rms, jobs, 3.0, 0, False, names, False),
         Group("main_nsigma_1", img, rms, jobs, 1.0, 1, False, names, False),
         Group("main_nsigma_8", img, None, jobs, 8.0, 0, False, names, False)]
    one = np.array([[3.0]], np.float32)
    tiny = [job(0.2, 0.1, 1.5, 1.5), job(50.0, 0.0, 1.5, 1.5)]
    g.append(Group("map_1x1", one, None, np.array(tiny), 3.0, 1, False, ["status5", "misses"], False))
    g.append(Group("map_1x1_no_bkg", one, np.array([[2.0]], np.float32), np.array(tiny), 3.0, 0, False, ["fitted", "misses"], False))
    row = np.array([[1.0, 2.0, 5.0, 9.0, 5.5, 2.0, 1.5]], np.float32)
    g.append(Group("map_1x7", row, None, np.array([job(3.1, 0.0, 1.2, 1.2), job(6.4, 0.3, 0.8, 0.8)]), 3.0, 1, False, ["mid", "end"], False))
    cimg, cjobs, cnames = capped_scene()
    g.append(Group("capped_520x515", cimg, None, cjobs, 3.0, 1, False, cnames, True))
    g.append(Group("n0", img, rms, np.zeros((0, 6)), 3.0, 1, False, [], False))
    _groups = g
    return g


def by_name(name):
    return next(g for g in groups() if g.name == name)
