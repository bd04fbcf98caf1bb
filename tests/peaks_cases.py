"""Inputs of the residual-peak tests (tests/test_peaks_cpu.py, tests/test_gpu_peaks.py): the smallest maps at which cy_find_peaks can
still go wrong.  cases() -> a tuple of Case; reference() -> {name: peaks_ref.find_peaks(...)}, computed once and shared."""
import functools
from collections import namedtuple

import numpy as np

import peaks_ref as PR

SEG = 1024                              # PEAK_SEG of csrc/cy_measure_jobs.h
GRID_MAX = 1 << 16                      # PK_GRID_MAX of csrc/cy_peaks.hip: an image of more segments is walked with the grid's stride
# offset: the device maps start one float behind a 16-byte boundary (the pixel-by-pixel loads with MW % 4 == 0)
Case = namedtuple("Case", "name map rms k_sigma radius sign offset")


def _noise(seed, shape, sigma=1.0):
    return (sigma * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def _flat(shape, v=1.0):
    return np.full(shape, v, np.float32)


def _spiky(seed, shape, nspike, amp=(6.0, 40.0)):
    """Unit noise with nspike positive and nspike negative spikes at random pixels."""
    rng = np.random.default_rng(seed)
    m = _noise(seed + 1000, shape)
    for s in (1.0, -1.0):
        ys, xs = rng.integers(0, shape[0], nspike), rng.integers(0, shape[1], nspike)
        m[ys, xs] = (s * rng.uniform(amp[0], amp[1], nspike)).astype(np.float32)
    return m


def _dirty(seed, shape):
    """_spiky with NaN, +-inf and 0 in the map, and 0, negative, NaN and inf in an uneven rms map."""
    rng = np.random.default_rng(seed + 7)
    m = _spiky(seed, shape, max(shape[0] * shape[1] // 60, 2))
    rms = (1.0 + 0.3 * np.sin(np.arange(shape[1]) / 9.0)[None, :] * np.cos(np.arange(shape[0]) / 7.0)[:, None]).astype(np.float32)
    n = max(shape[0] * shape[1] // 40, 1)
    for bad in (np.nan, np.inf, -np.inf, 0.0):
        m[rng.integers(0, shape[0], n), rng.integers(0, shape[1], n)] = bad
    for bad in (0.0, -1.0, np.nan, np.inf):
        rms[rng.integers(0, shape[0], n), rng.integers(0, shape[1], n)] = bad
    return m, rms


def _boundaries(nseg):
    """12 rows, nseg segments and one pixel: a peak on the last pixel of a segment (row 0) and one on the first pixel of the next
    (row 4), and two equal values on both sides of the boundary (row 8), at every boundary."""
    m = _noise(31 + nseg, (12, nseg * SEG + 1), 0.1)
    for b in range(1, nseg + 1):
        m[0, b * SEG - 1] = 10.0 + b
        m[4, b * SEG] = 20.0 + b
        m[8, b * SEG - 1] = m[8, b * SEG] = 30.0 + b
    return m


def _ties():
    """A 5 x 5 plateau (its first pixel is the one peak); two equal maxima radius + 1 = 3 apart (both peaks) and radius = 2 apart
    (the first only), along a row and along a column."""
    m = _flat((40, 40), 0.5)
    m[3:8, 4:9] = 10.0
    m[12, 5] = m[12, 8] = 9.0
    m[18, 5] = m[18, 7] = 8.0
    m[22, 20] = m[25, 20] = 7.0
    m[30, 20] = m[32, 20] = 6.0
    return m


def _edges():
    m = _noise(5, (30, 41), 0.2)
    for y in (0, 15, 29):
        for x in (0, 20, 40):
            m[y, x] = 10.0 + y + 0.25 * x
    return m


def _validity():
    """Spikes 10 apart on a flat map, k_sigma = 5.
      row 5    u == k_sigma * rms exactly (7.5 = 5 * 1.5: a peak), one fp32 ulp below (not); the fp32 neighbours of 5 * 1.3f, whose
               product is not an fp32 value, one on each side of it
      row 15   rms 0, negative, NaN, inf under a spike: never a peak
      row 25   a spike beside a larger value whose rms is NaN: the larger one still outranks it and neither is a peak; a spike beside a
               smaller value above the threshold whose rms is 0: a peak, and the neighbour is not counted in nabove
      row 35   NaN, +inf, -inf and 0 in the map beside a spike: invalid, neither ranked nor counted"""
    m, rms = _flat((45, 60), 0.25), _flat((45, 60), 1.0)
    rms[5, 5] = rms[5, 15] = 1.5
    m[5, 5], m[5, 15] = 7.5, np.nextafter(np.float32(7.5), np.float32(0))
    r = np.float32(1.3)
    t = 5.0 * float(r)                                                # float64, not an fp32 value
    up = np.float32(t)
    up = up if float(up) >= t else np.nextafter(up, np.float32(np.inf))
    assert float(up) > t > float(np.nextafter(up, np.float32(0)))
    rms[5, 25] = rms[5, 35] = r
    m[5, 25], m[5, 35] = up, np.nextafter(up, np.float32(0))
    for x, bad in zip((5, 15, 25, 35), (0.0, -1.0, np.nan, np.inf)):
        m[15, x], rms[15, x] = 9.0, bad
    m[25, 5], m[25, 6], rms[25, 6] = 10.0, 12.0, np.nan
    m[25, 25], m[25, 26], rms[25, 26] = 10.0, 8.0, 0.0
    for x, bad in zip((5, 15, 25, 35), (np.nan, np.inf, -np.inf, 0.0)):
        m[35, x], m[35, x + 1], m[34, x] = 9.0, bad, bad
    return m, rms


def _tall(width):
    """GRID_MAX + 104 rows of one short segment each: the workgroups of rows 0 .. 103 take a second segment, GRID_MAX rows further
    down.  Spikes on rows 3 and 50 and on the rows GRID_MAX below them, so that one workgroup counts and fills peaks in both of its
    iterations, beside random ones."""
    m = _spiky(40 + width, (GRID_MAX + 104, width), 80)
    for y in (3, 50, GRID_MAX + 3, GRID_MAX + 50):
        m[y - 2:y + 3, :] = np.float32(0.5)
        m[y, 1] = np.float32(60.0 + y % 7)
    return m


def _lattice():
    """96 x 96, radius 1: a peak on every second pixel in both directions, 2304 of them, all different."""
    m = _flat((96, 96), 1.0)
    yy, xx = np.mgrid[0:96:2, 0:96:2]
    m[::2, ::2] = (10.0 + ((yy * 37 + xx * 11) % 101) / 8.0).astype(np.float32)
    return m


def _scene():
    """384 x 512: 600 circular Gaussians plus seeded unit noise scaled by a smooth rms map."""
    rng = np.random.default_rng(2024)
    H, W = 384, 512
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    rms = 1.0 + 0.5 * np.sin(xx / 80.0) * np.cos(yy / 60.0)
    m = rng.standard_normal((H, W)) * rms
    for _ in range(600):
        x0, y0, s, A = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(1.0, 3.0), rng.uniform(4.0, 60.0)
        x1, x2, y1, y2 = int(max(x0 - 6 * s, 0)), int(min(x0 + 6 * s + 1, W)), int(max(y0 - 6 * s, 0)), int(min(y0 + 6 * s + 1, H))
        m[y1:y2, x1:x2] += A * np.exp(-((xx[y1:y2, x1:x2] - x0) ** 2 + (yy[y1:y2, x1:x2] - y0) ** 2) / (2 * s * s))
    return m.astype(np.float32), rms.astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    d7075, r7075 = _dirty(1, (70, 75))
    d6496, r6496 = _dirty(2, (64, 96))
    vm, vr = _validity()
    sm, sr = _scene()
    out = [
        Case("1x1", np.array([[7.0]], np.float32), _flat((1, 1)), 5.0, 1, 1, False),
        Case("1x1_below", np.array([[4.0]], np.float32), _flat((1, 1)), 5.0, 2, 1, False),
        Case("1x37", _spiky(3, (1, 37), 4), _flat((1, 37)), 4.0, 2, 1, False),
        Case("37x1", _spiky(4, (37, 1), 4), _flat((37, 1)), 4.0, 2, 1, False),
        Case("70x75", d7075, r7075, 3.0, 2, 1, False),
        Case("70x75_r1", d7075, r7075, 3.0, 1, 1, False),
        Case("70x75_r8", d7075, r7075, 3.0, 8, 1, False),
        Case("70x75_holes", d7075, r7075, 3.0, 2, -1, False),
        Case("64x96", d6496, r6496, 3.0, 2, 1, False),
        Case("64x96_offset", d6496, r6496, 3.0, 2, 1, True),
        Case("one_segment_and_1", _boundaries(1), _flat((12, SEG + 1)), 5.0, 2, 1, False),
        Case("two_segments_and_1", _boundaries(2), _flat((12, 2 * SEG + 1)), 5.0, 2, 1, False),
        Case("ties", _ties(), _flat((40, 40)), 5.0, 2, 1, False),
        Case("edges_r2", _edges(), _flat((30, 41)), 5.0, 2, 1, False),
        Case("edges_r8", _edges(), _flat((30, 41)), 5.0, 8, 1, False),
        Case("validity", vm, vr, 5.0, 2, 1, False),
        Case("none", _noise(9, (33, 47)), _flat((33, 47)), 50.0, 2, 1, False),
        Case("lattice", _lattice(), _flat((96, 96)), 5.0, 1, 1, False),
        Case("tall_8", _tall(8), _flat((GRID_MAX + 104, 8)), 4.0, 2, 1, False),
        Case("tall_5", _tall(5), _flat((GRID_MAX + 104, 5)), 4.0, 2, 1, False),
        Case("scene", sm, sr, 5.0, 2, 1, False),
    ]
    for c in out:
        c.map.setflags(write=False)
        c.rms.setflags(write=False)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def reference():
    """{name: (rows, abs_terms)} of peaks_ref.find_peaks on every case; read-only."""
    out = {}
    for c in cases():
        rows, absum = PR.find_peaks(c.map, c.rms, c.k_sigma, c.radius, c.sign)
        rows.setflags(write=False)
        absum.setflags(write=False)
        out[c.name] = (rows, absum)
    return out


BRUTE_FORCE = ("1x1", "1x1_below", "1x37", "37x1", "70x75", "70x75_r1", "70x75_r8", "70x75_holes", "64x96", "ties", "edges_r2", "edges_r8",
               "validity", "none", "lattice", "tall_5")
