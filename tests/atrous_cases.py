"""Inputs of the a trous tests (tests/test_atrous_cpu.py, tests/test_gpu_atrous.py): the smallest maps at which cy_atrous_step can go
wrong, each with its step.  reference() holds atrous_ref.atrous_step of every case, computed once and left unchanged.

COLS, CHUNK and GRID_MAX restate the kernel's geometry (cy_measure_jobs.h: ATR_COLS, ATR_CHUNK, ATR_GRID_MAX): a work item is a block of
COLS columns, one residue class y mod step and CHUNK consecutive rows of that class; at most GRID_MAX workgroups walk the items."""
import functools
from types import SimpleNamespace

import numpy as np

import atrous_ref as AR

COLS, CHUNK, GRID_MAX = 256, 64, 1 << 13
FLT_MAX = float(np.finfo(np.float32).max)
TINY = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5)]
TINY_STEPS, STEPS = (1, 4, 64), (1, 2, 3, 8, 64)
IMPULSES = {"corner": (0, 0), "edge": (0, 9), "interior": (8, 9)}          # (y, x) in a 17 x 19 map


def _noise(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def special_map():
    """20 x 23 of noise with every kind of value the definition names: NaN, +inf, -inf, 0, subnormals, and values near FLT_MAX of
    both signs next to each other (a smooth value stays finite: a convex combination; a detail value may overflow to +-inf, on both
    sides alike)."""
    m = _noise((20, 23), 5)
    m[0, 0], m[3, 4], m[19, 22], m[10, 0] = np.nan, np.inf, -np.inf, np.nan
    m[5, 5:9] = 0.0
    m[7, 1], m[7, 2], m[7, 3] = 1e-45, -1e-45, 1.1754942e-38        # the smallest subnormal of both signs, the largest subnormal
    m[12, 10], m[12, 11], m[13, 10], m[13, 11] = FLT_MAX, -FLT_MAX, -3.0e38, 3.3e38
    m[0, 22], m[19, 0] = FLT_MAX, -FLT_MAX
    m[14:19, 14:19], m[16, 16] = -FLT_MAX, FLT_MAX             # at step 1 the detail of the centre is about 1.7 FLT_MAX: +inf in fp32
    return m


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, m, step, offset=False):
        out.append(SimpleNamespace(name=name, map=np.ascontiguousarray(m, np.float32), step=int(step), offset=offset))
    for i, (h, w) in enumerate(TINY):
        for s in TINY_STEPS:                                   # 2 step >= the side: the fold wraps several times
            add("%dx%d_s%d" % (h, w, s), _noise((h, w), 10 + i), s)
    for s in STEPS:
        add("70x75_s%d" % s, _noise((70, 75), 21), s)          # MW % 4 != 0
        add("64x96_s%d" % s, _noise((64, 96), 22), s)
        add("64x96_offset_s%d" % s, _noise((64, 96), 22), s, offset=True)     # pointers one float behind a 16-byte boundary
    for s in (1, 3):
        add("special_s%d" % s, special_map(), s)
    for name, (y, x) in IMPULSES.items():
        for s in (1, 2):
            m = np.zeros((17, 19), np.float32)
            m[y, x] = 1.0
            add("impulse_%s_s%d" % (name, s), m, s)
    add("constant_s1", np.full((33, 40), np.float32(0.1)), 1)
    add("constant_s8", np.full((33, 40), np.float32(-1234.567)), 8)
    # one pixel beyond one and beyond two column blocks and row chunks (a class of step 2 has CHUNK + 1 rows at MH = 2 CHUNK + 1)
    add("cols_and_1", _noise((9, COLS + 1), 31), 1)
    add("two_cols_and_1", _noise((9, 2 * COLS + 1), 32), 3)
    add("chunk_and_1", _noise((CHUNK + 1, 31), 33), 1)
    add("two_chunks_and_1", _noise((2 * CHUNK + 1, 31), 34), 1)
    add("chunk_and_1_s2", _noise((2 * CHUNK + 1, 31), 35), 2)
    add("two_chunks_and_1_s2", _noise((4 * CHUNK + 2, 31), 36), 2)
    # more work items than the grid has workgroups: the first workgroups walk a second item
    add("tall_s1", _noise((GRID_MAX * CHUNK + 1, 3), 37), 1)
    add("tall_s3", _noise((600001, 2), 38), 3)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def items(MH, MW, step):
    """Work items of a shape, as plan_atrous counts them."""
    return -(-MW // COLS) * min(step, MH) * -(-(-(-MH // step)) // CHUNK)


@functools.lru_cache(maxsize=None)
def reference():
    """{name: (smooth, detail)} of every case."""
    return {c.name: AR.atrous_step(c.map, c.step) for c in cases()}


LOOPS = tuple(c.name for c in cases() if c.map.size <= 70 * 75 and not c.offset)      # the cases the pixel loop is run on
