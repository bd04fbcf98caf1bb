"""Inputs of the disc-residual tests, shared by tests/test_disc_residual_cpu.py (the two statements of the reference against each
other), tests/test_disc_residual_plan_cpu.py and tests/test_gpu_disc_residual.py (the kernel against the reference).  A group is one
cy_disc_residuals call: a map, a model map (or None), a job table; the jobs of one call see each other as neighbours, so jobs
that are meant to be alone lie more than 2 R apart.  `offset` says that the GPU test hands the maps over through a pointer one
float behind the start of a larger buffer.  No map is larger than 520 x 515.
  tiny        1 x 1 and 1 x 7
  odd         70 x 75 (MW % 4 != 0): R = 1 at an integer and a half-integer centre; R = 6 inside, at a corner (clipped), one pixel
              outside the image and at 1e300 (status 5); bad job fields (R NaN, 0, 257; sign 0; bkg inf: status 1)
  main        64 x 96, with and without a model, and through the offset pointer: two discs 4 px apart on integer centres (tie pixels
              belong to both), coincident centres, R 6 beside R 12, a hole job, NaN / +-inf / 0 pixels inside a disc, a disc with
              no valid pixel, two equal largest |r| in one disc
  crowded     ten discs within one radius
  r256        one 520 x 515 map holding an R = 256 job: the 513 x 513 window
  empty       n = 0"""
from types import SimpleNamespace

import numpy as np

INF, NAN = float("inf"), float("nan")
_CACHE = {}


def job(cx, cy, R, bkg=0.0, sign=1.0, start=(1.0, 0.0, 0.0, 1.0, 0.0, 1.0)):
    """One row of the job table; the start is ignored by the entry (the default is not even near the disc)."""
    return [float(cx), float(cy), float(R), float(bkg), float(sign)] + [float(v) for v in start]


def _noise(shape, seed, scale=1.0):
    return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def _group(name, amap, model, named_jobs, offset=False):
    names = [n for n, _ in named_jobs]
    jobs = np.array([j for _, j in named_jobs], np.float64).reshape(-1, 11)
    return SimpleNamespace(name=name, map=np.ascontiguousarray(amap, np.float32), model=None if model is None else np.ascontiguousarray(model, np.float32),
                           jobs=jobs, names=names, offset=offset)


def _main_map():
    amap = _noise((64, 96), 5) + np.float32(0.75)
    # NaN, +-inf and 0 inside the disc at (20, 44), R = 6
    amap[44, 20], amap[43, 22] = np.nan, np.inf
    amap[46, 19], amap[45, 21] = -np.inf, 0.0
    # a disc with no valid pixel at (80, 50), R = 3: zeros and NaN
    amap[46:55, 76:85] = 0.0
    amap[50, 80] = np.nan
    # two equal largest |r| in the disc at (60, 20), R = 5, bkg 0.25: +9.25 - 0.25 = 9 at (62, 19) and -8.75 - 0.25 = -9 at (58, 21); the first in
    # window order (row 19) wins
    amap[19, 62], amap[21, 58] = 9.25, -8.75
    return amap


def _main_jobs():
    return [("pair_a", job(10.0, 10.0, 6.0, 0.5)), ("pair_b", job(14.0, 10.0, 6.0, -0.25)),             # 4 px apart on integer centres: column 12 ties
            ("coincident_a", job(40.0, 12.0, 5.0, 0.1)), ("coincident_b", job(40.0, 12.0, 5.0, 0.2)),
            ("r6_beside_r12", job(70.3, 40.6, 6.0, 0.0)), ("r12", job(80.2, 30.1, 12.0, 1.5)),
            ("hole", job(30.5, 50.25, 6.0, 0.75, -1.0)),
            ("invalid_inside", job(20.0, 44.0, 6.0, 0.3)),
            ("no_valid_pixel", job(80.0, 50.0, 3.0, 0.0)),
            ("equal_maxima", job(60.0, 20.0, 5.0, 0.25))]


def groups():
    """-> the list of groups (cached; nobody writes into them)."""
    if "groups" in _CACHE:
        return _CACHE["groups"]
    out = []
    out.append(_group("tiny_1x1", np.array([[2.5]], np.float32), np.array([[0.5]], np.float32),
                      [("on_it", job(0.0, 0.0, 1.0, 0.5)), ("beside", job(0.4, -0.3, 2.0, -1.0, -1.0)), ("off", job(3.0, 0.0, 1.0))]))
    out.append(_group("tiny_1x7", np.array([[1.0, -2.0, 0.0, 4.0, NAN, 3.0, -7.0]], np.float32), None,
                      [("left", job(1.0, 0.0, 2.0, 0.25)), ("right", job(5.5, 0.0, 1.5, 0.0)), ("all", job(3.0, 0.2, 4.0, 1.0))]))
    odd = _noise((70, 75), 3, 2.0)
    out.append(_group("odd_70x75", odd, _noise((70, 75), 4, 0.5), [
        ("r1_int", job(20.0, 20.0, 1.0, 0.1)), ("r1_half", job(30.5, 20.5, 1.0, 0.1)),
        ("r6_inside", job(40.25, 40.75, 6.0, -0.5)), ("r6_corner", job(73.0, 68.5, 6.0, 0.0)), ("r6_corner0", job(0.0, 0.0, 6.0, 0.0)),
        ("r6_outside", job(-1.0, 40.0, 6.0, 0.0)), ("r6_below", job(20.0, 76.5, 6.0, 0.0)), ("r6_far", job(1e300, 20.0, 6.0)),
        ("r6_nan_centre", job(NAN, 20.0, 6.0)),
        ("r_nan", job(50.0, 20.0, NAN)), ("r_zero", job(50.0, 20.0, 0.0)), ("r_257", job(50.0, 20.0, 257.0)),
        ("sign_zero", job(50.0, 20.0, 6.0, 0.0, 0.0)), ("bkg_inf", job(50.0, 20.0, 6.0, INF)),
        ("start_nan", job(60.0, 55.0, 4.0, 0.5, 1.0, (NAN, INF, -INF, NAN, NAN, NAN)))]))
    amap = _main_map()
    model = _noise((64, 96), 6, 0.25)
    out.append(_group("main_64x96", amap, model, _main_jobs()))
    out.append(_group("main_no_model", amap, None, _main_jobs()))
    out.append(_group("main_offset", amap, model, _main_jobs(), offset=True))
    rng = np.random.default_rng(8)
    out.append(_group("crowded", _noise((64, 96), 9) + np.float32(0.5), _noise((64, 96), 10),
                      [("crowd%d" % k, job(48.0 + rng.uniform(-3.0, 3.0), 32.0 + rng.uniform(-3.0, 3.0), 6.0, 0.05 * k)) for k in range(10)]))
    out.append(_group("r256_520x515", _noise((520, 515), 12), _noise((520, 515), 13, 0.1),
                      [("r256", job(257.0, 258.0, 256.0, 0.125)), ("r256_neighbour", job(500.0, 505.0, 5.0, 0.0))]))
    out.append(_group("empty", _noise((8, 9), 14), None, []))
    _CACHE["groups"] = out
    return out


def by_name(name):
    return next(g for g in groups() if g.name == name)
