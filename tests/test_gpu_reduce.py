"""The block reduction of the measurement kernels (caesar_yolo_amd/csrc/cy_reduce.h) on its own, through cy_debug_reduce, against
its numpy restatement (tests/reduce_ref.py).  No tolerance: every output word is compared as an integer, for both finishing styles
(thread 0 continues after the barrier / every thread reads the slots, taken from the last thread).

Random rows: 16 per length, values standard_normal * 10 ** randint(-6, 7), so that float64 addition is far from associative on them.
Before anything runs on the GPU the inputs are shown to tell the kernel's association from four others (waves reversed, waves
pairwise, an up-sweep inside the wave, the plain sequential sum) at every length from 255 on; below that one wave holds everything
and only the in-wave variant can differ.  The tie and empty rows of the first maximum are constructed."""
import ctypes as C

import numpy as np
import pytest
import torch

import reduce_ref as RR
from caesar_yolo_amd import lib as L

ROWS, LENGTHS, SEED = 16, (0, 1, 63, 64, 65, 255, 256, 257, 1000), 7
WORDS = ("sum", "count", "key", "index", "imin", "imax", "index64", "umin")


def random_rows(n):
    rng = np.random.default_rng([SEED, n])
    val = rng.standard_normal((ROWS, n)) * 10.0 ** rng.integers(-6, 7, (ROWS, n))
    key = (rng.standard_normal((ROWS, n)) * 10.0 ** rng.integers(-6, 7, (ROWS, n))).astype(np.float32)
    key[rng.random((ROWS, n)) < 0.25] = 0.0                  # blank entries: not valid, never a candidate
    return val, key


def constructed_rows():
    """name -> (key row of 600 entries, expected (key, index) or None)."""
    n = 600
    base = np.linspace(-3.0, 2.0, n).astype(np.float32)
    base[base == 0] = 0.5
    ties = base.copy()
    ties[[70, 200, 70 + 256]] = 9.0                           # thread 70 twice (the lane keeps its first), thread 200 in wave 3
    corner = base.copy()
    corner[255] = 9.0                                         # lane 63 of wave 3 only
    blank = np.zeros(n, np.float32)
    blank[5], blank[300] = np.nan, np.inf                     # not valid either
    one = blank.copy()
    one[511] = -2.5                                           # a single valid key, negative, in the second round of thread 255
    return {"ties": (ties, (9.0, 70)), "corner": (corner, (9.0, 255)), "blank": (blank, None), "one": (one, (-2.5, 511))}


def run(val, key):
    lib = L.load()
    rows, n = val.shape
    dv, dk = torch.from_numpy(np.ascontiguousarray(val)).cuda(), torch.from_numpy(np.ascontiguousarray(key)).cuda()
    out = torch.zeros((rows, 2, 8), dtype=torch.int64, device="cuda")
    rc = lib.cy_debug_reduce(C.c_void_p(dv.data_ptr() if n else None), C.c_void_p(dk.data_ptr() if n else None), rows, n,
                             C.c_void_p(out.data_ptr()))
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


def assert_words(what, got, want):
    for style, name in enumerate(("thread 0", "every thread")):
        g = got[:, style]
        if not np.array_equal(g, want):
            r, f = (int(v[0]) for v in np.nonzero(g != want))
            raise AssertionError("%s, %s: %d words differ; first: row %d %s: %#x on the GPU, %#x in the reference" % (
                what, name, int((g != want).sum()), r, WORDS[f], int(g[r, f]), int(want[r, f])))


def assert_told_apart(n, val):
    if n < 255:
        return
    want = RR.tree_sum(val).view(np.uint64)
    for name, other in RR.other_associations(val).items():
        assert (other.view(np.uint64) != want).any(), "length %d: '%s' gives the kernel's bits on all %d rows" % (n, name, ROWS)


def test_the_inputs_tell_associations_apart():
    for n in LENGTHS:
        assert_told_apart(n, random_rows(n)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_random_rows(n):
    val, key = random_rows(n)
    assert_told_apart(n, val)                                 # on the CPU, before anything runs on the GPU
    assert_words("length %d" % n, run(val, key), RR.probe_rows(val, key))


@pytest.mark.gpu
def test_ties_and_empty_rows():
    cases = constructed_rows()
    key = np.stack([k for k, _ in cases.values()])
    val = np.ones(key.shape, np.float64)
    want = RR.probe_rows(val, key)
    none_key = int(np.array([-np.inf], np.float32).view(np.uint32)[0])
    for r, (name, (_, exp)) in enumerate(cases.items()):        # the reference itself gives what the case was built for
        k, i = (none_key, RR.NONE32) if exp is None else (int(np.array([exp[0]], np.float32).view(np.uint32)[0]), exp[1])
        assert (int(want[r, 2]), int(want[r, 3])) == (k, i), name
        assert int(want[r, 6]) == (RR.NONE64 if exp is None else i), name
    assert_words("constructed rows", run(val, key), want)
