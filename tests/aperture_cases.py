"""Constructed cases of cy_aperture_sums, small on purpose: shared by tests/test_aperture_cpu.py (the two references against each
other), tests/test_aperture_plan_cpu.py (windows and statuses) and tests/test_gpu_aperture.py (the device against the reference).
A case is a map, an rms map, jobs [n, 3] (cx, cy, unit) and a factor table; case(name) builds it once, rows(name, with_rms)
computes the reference rows once."""
import functools
import math
from types import SimpleNamespace

import numpy as np

import aperture_ref as AR

FLT_MAX, FLT_TINY = float(np.finfo(np.float32).max), float(np.finfo(np.float32).smallest_subnormal)
INF, NAN = float("inf"), float("nan")


def noise_map(shape, seed, holes=True):
    """A random fp32 map with a few masked (0), NaN and infinite pixels; the rms map to it with a few that do not count."""
    rng = np.random.default_rng(seed)
    m = rng.normal(0.5, 2.0, shape).astype(np.float32)
    r = (0.5 + rng.random(shape)).astype(np.float32)
    if holes and m.size >= 16:
        idx = rng.choice(m.size, size=max(m.size // 16, 4), replace=False)
        m.ravel()[idx[0::4]] = 0.0
        m.ravel()[idx[1::4]] = NAN
        m.ravel()[idx[2::4]] = INF
        r.ravel()[idx[3::4]] = 0.0
    return m, r


def _case(amap, rms, jobs, factors):
    return SimpleNamespace(map=np.ascontiguousarray(amap, np.float32), rms=np.ascontiguousarray(rms, np.float32),
                           jobs=np.array(jobs, np.float64).reshape(-1, 3), factors=tuple(float(f) for f in factors))


def _annulus(values):
    """15 x 15 zeros with `values` on the first pixels (row-major) of the annulus 1 < d <= 3 around (7, 7); one job."""
    m = np.zeros((15, 15), np.float32)
    ring = [(y, x) for y in range(15) for x in range(15) if 1 < (x - 7) ** 2 + (y - 7) ** 2 <= 9]
    assert len(ring) == 24 and len(values) <= 24
    for (y, x), v in zip(ring, values):
        m[y, x] = v
    m[7, 7] = 5.0
    return _case(m, np.ones_like(m), [[7.0, 7.0, 1.0]], (1.0, 3.0))


def _one_window(shape, cx, cy, r, area):
    m, rms = noise_map(shape, area)
    c = _case(m, rms, [[cx, cy, r]], (0.5, 1.0))
    st, x0, x1, y0, y1 = AR.window(cx, cy, r, c.factors, *shape)[:5]
    assert st == 0 and (x1 - x0 + 1) * (y1 - y0 + 1) == area
    return c


CENTRES = [(0.0, 0.0), (30.0, 23.0), (0.0, 12.0), (14.0, 23.0), (10.0, 11.0), (10.5, 7.5), (7.0 * math.sqrt(2.0), 3.0 * math.pi),
           (-1.0, 5.0), (31.0, 5.0), (5.0, 24.0), (5.0, -1.0), (-1.0, -1.0), (1e300, 5.0), (5.0, -1e300), (NAN, 5.0), (5.0, NAN),
           (INF, 5.0), (5.0, -INF), (-INF, INF), (-6.0, 5.0), (5.0, 28.25), (-5.25, 5.0)]


def _build(name):
    if name == "image_1x1":
        return _case([[2.5]], [[0.5]], [[0.0, 0.0, 1.0], [0.5, 0.5, 1.0], [1.0, 0.0, 1.0], [-1.0, -1.0, 1.0], [0.5, 0.5, 0.1], [0.0, 3.0, 1.0]], (1.0, 2.0))
    if name == "image_1x7":
        m, r = noise_map((1, 7), 17, holes=False)
        return _case(m, r, [[x, y, 1.0] for x in (0.0, 3.0, 6.0, 7.0, 2.5) for y in (0.0, 0.5, -1.0)], (1.0, 2.0, 3.0))
    if name in ("centres", "rings_1", "rings_8"):
        m, r = noise_map((24, 31), 31)
        factors = {"centres": (1.0, 2.0, 3.5), "rings_1": (3.0,), "rings_8": (0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0)}[name]
        return _case(m, r, [[x, y, 1.5] for x, y in CENTRES], factors)
    if name in ("boundary5", "boundary5_below"):
        # (+-3, +-4), (+-4, +-3), (+-5, 0), (0, +-5) sit exactly on r_2 = 5: inside ring 2; one ulp below, they fall to ring 3
        m, r = noise_map((25, 25), 5, holes=False)
        five = 5.0 if name == "boundary5" else math.nextafter(5.0, 0.0)
        return _case(m, r, [[12.0, 12.0, 1.0]], (3.0, five, 6.0))
    if name == "radius_limits":
        m, r = noise_map((40, 40), 40)
        units = [0.0, -0.0, -1.0, NAN, INF, -INF, 128.0, math.nextafter(128.0, INF), 1e-320, 1e308, 0.25]
        return _case(m, r, [[20.0, 19.0, u] for u in units] + [[NAN, 19.0, 0.0]], (1.0, 2.0))
    if name == "area_255":
        return _one_window((15, 40), 20.0, 7.0, 8.0, 255)
    if name == "area_256":
        return _one_window((16, 40), 20.5, 7.5, 7.5, 256)
    if name == "area_257":
        return _one_window((1, 300), 150.0, 0.0, 128.0, 257)
    if name == "area_1025":
        return _one_window((25, 64), 30.0, 12.0, 20.0, 1025)
    if name == "largest":
        m, r = noise_map((600, 600), 600)
        return _case(m, r, [[300.0, 299.5, 256.0]], (0.25, 0.5, 1.0))
    if name == "pixel_values":
        vals = [NAN, INF, -INF, 0.0, -0.0, FLT_TINY, -FLT_TINY, 3 * FLT_TINY, FLT_MAX, -FLT_MAX, FLT_MAX, 1.0, -1.0, 1e-38, -1e-38, 1e38]
        m = np.array(vals * 4, np.float32).reshape(8, 8)
        rms = np.array(([1.0, FLT_MAX, FLT_TINY, 2.0] * 16), np.float32).reshape(8, 8)
        return _case(m, rms, [[3.5, 3.5, 1.0], [2.0, 3.0, 1.0], [0.0, 0.0, 2.0]], (1.5, 3.0, 5.0))
    if name.startswith("annulus_"):
        rng = np.random.default_rng(24)
        values = {"0": [], "1": [4.0], "2": [4.0, -1.5], "even": list(rng.normal(0, 1, 24)), "odd": list(rng.normal(0, 1, 23)),
                  "equal": [7.0] * 24, "ties": [1.0, 2.0, 2.0, 3.0, 2.0, 1.0, 3.0, 2.0, 2.0, 1.0] * 2,
                  "split": [1.0] * 12 + [3.0] * 12, "ties_odd": [2.0, 1.0, 2.0, 3.0, 2.0, 2.0, 5.0]}[name[len("annulus_"):]]
        return _annulus(values)
    if name == "rms_values":
        m, _ = noise_map((12, 12), 12, holes=False)
        rms = np.array([0.0, -1.0, NAN, INF, -INF, 1.0, FLT_TINY, FLT_MAX, -0.0, 2.0, 0.5, 3.0] * 12, np.float32).reshape(12, 12)
        return _case(m, rms, [[5.0, 6.0, 1.0], [0.0, 0.0, 1.0], [11.0, 5.5, 1.0]], (1.0, 2.5, 4.0))
    if name == "many_jobs":
        m, r = noise_map((64, 64), 64)
        i = np.arange(70000)
        jobs = np.stack([(i % 67).astype(np.float64) - 1.0, ((i // 67) % 66).astype(np.float64) - 1.0, np.ones(i.size)], axis=1)
        return _case(m, r, jobs, (1.0,))
    if name == "exact_scene":
        y, x = np.mgrid[0:96, 0:96]
        m = np.where((x - 40) ** 2 + (y - 40) ** 2 <= 36, 5.0, 3.0).astype(np.float32)
        return _case(m, np.full_like(m, 2.0), [[40.0, 40.0, 1.0]], (2.0, 4.0, 6.0, 8.0, 10.0, 14.0))
    raise KeyError(name)


NAMES = ("image_1x1", "image_1x7", "centres", "rings_1", "rings_8", "boundary5", "boundary5_below", "radius_limits", "area_255", "area_256",
         "area_257", "area_1025", "largest", "pixel_values", "annulus_0", "annulus_1", "annulus_2", "annulus_even", "annulus_odd",
         "annulus_equal", "annulus_ties", "annulus_split", "annulus_ties_odd", "rms_values", "many_jobs", "exact_scene")


@functools.lru_cache(maxsize=None)
def case(name):
    return _build(name)


@functools.lru_cache(maxsize=None)
def rows(name, with_rms=True):
    """The reference rows of a case, computed once; callers must not write into them."""
    c = case(name)
    out = AR.reference(c.map, c.rms if with_rms else None, c.jobs, c.factors)
    out.setflags(write=False)
    return out
