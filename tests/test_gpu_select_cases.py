"""The exact median selection of csrc/cy_select.h on constructed sets, through both of its entry points: cy_measure_background (the
cell, in its LDS form and in its L2 form) and cy_measure_sources (the ring), against the numpy references tests/bkg_ref.py and
tests/measure_ref.py: a sort.  The other tests compare the medians bit for bit too, but on noise, which rarely reaches the corner
branches of the selection; the sets here are built to reach them:

  counts     0, 1, 2, 3, 4, 255, 256, 257, 511, 512, 513, 1024 valid pixels (and the full ring) around the 256 bins, the 256 / 512
             threads and the 1024-pixel stride of a walk
  values     all equal (an even count needs no extra pass, rms is 0); two values in equal shares (the upper middle element
             differs: the extra pass runs and the median is the float64 mean of two floats, no float itself); values that differ
             only in the lowest mantissa byte (the first three passes fall in one bin); mixed signs from -FLT_MAX to FLT_MAX with
             FLT_MIN among them, no denormals; deviations that tie in pairs; deviations that differ only in the two lowest bytes of
             the float64 (the first six passes fall in one bin)
  clips      niter 0 and 3 at k = 3 and k = 0.5: sets a clip leaves whole (the selection returns after its counting pass), sets a
             clip cuts down to one survivor, and sets a clip empties

Every set lies in an otherwise blank (0) cell or ring.  Every case first asserts on the reference side that it is what its name
says.  Comparison: all eight fields of every cell, and the fields of a source that tests/test_gpu_measure.py treats as exact, equal
the reference bit for bit; the four sums of a source have one term each here (a one-pixel box) and keep that test's bound,
2 m 2^-53 sum|t_i| with m = 1.  No case is skipped."""
import numpy as np
import pytest
import torch

import bkg_ref
import measure_ref
from gpu_common import detector

pytestmark = pytest.mark.gpu

F32 = np.float32
FMAX, FMIN = np.finfo(F32).max, np.finfo(F32).tiny
COUNTS = (0, 1, 2, 3, 4, 255, 256, 257, 511, 512, 513, 1024)
LDS_SHAPE, LDS_CELL = (64, 96), 32                  # 2 x 3 cells of 1024 pixels: copied into LDS
L2_SHAPE, L2_CELL = (129, 258), 129                 # 1 x 2 cells of 16641 pixels: above BKG_LDS_MAX = 16384, re-read from the image
RINGS = {1: 8, 12: 624, 16: 1088}                   # ring -> pixels of the ring of a one-pixel box
PITCH = 40                                          # distance of the ring sites: a grown window is at most 33 pixels wide
CENTRE = F32(7.0)                                   # the box pixel of a ring site: in no set


# ---- the sets: n -> float32 values, or None where the pattern has no set of that size

def all_equal(n):
    return np.full(n, 0.375, F32) if n >= 1 else None


def two_values(n):
    if n < 2 or n % 2:
        return None
    return np.repeat(np.array([1.0, np.nextafter(F32(1.0), F32(2.0))], F32), n // 2)


def low_mantissa_byte(n):
    if n < 2:
        return None
    return (np.uint32(0x3F800000) + (np.arange(n, dtype=np.uint32) * np.uint32(37)) % np.uint32(256)).view(F32)


def extremes(n):
    if n < 3:
        return None
    rng = np.random.default_rng(1000 + n)
    rest = np.ldexp(rng.uniform(1.0, 2.0, n - 3), rng.integers(-126, 127, n - 3)) * rng.choice([-1.0, 1.0], n - 3)
    return np.concatenate([[-FMAX, FMAX, FMIN], rest.astype(F32)]).astype(F32)


def tied_deviations(n):
    if n < 2:
        return None
    m = n // 2
    j = np.arange(-m, m + 1)
    return (2.0 + j[(j != 0) | bool(n % 2)] * 2.0 ** -10).astype(F32)


def low_deviation_bytes(n):
    """k tiny values i 2^-50, one (odd n) or two (even n) 1.0, k 2.0: the median is 1.0 and the deviations are k ones, the zeros and
    the k values 1 - i 2^-50, which share their six upper bytes; the median of the deviations is among those."""
    if n < 3:
        return None
    k = (n - 1) // 2
    return np.concatenate([np.arange(1, k + 1) * 2.0 ** -50, np.ones(n - 2 * k), np.full(k, 2.0)]).astype(F32)


PATTERNS = (all_equal, two_values, low_mantissa_byte, extremes, tied_deviations, low_deviation_bytes)


def check_set(pattern, n, v):
    """The set is what its name says (values and the reference's median / rms of the whole set)."""
    assert v.dtype == F32 and v.shape == (n,) and np.all(v != 0) and np.all(np.abs(v) >= FMIN) and np.all(np.isfinite(v)), (pattern.__name__, n)
    d = v.astype(np.float64)
    med, sig = bkg_ref.med_sig(d)
    dev = np.abs(d - med)
    if pattern is all_equal:
        assert med == 0.375 and sig == 0.0
    elif pattern is two_values:
        lo, hi = float(v.min()), float(v.max())
        assert (v == v.min()).sum() == (v == v.max()).sum() == n // 2 and med == (lo + hi) / 2.0 and lo < med < hi and float(F32(med)) != med
    elif pattern is low_mantissa_byte:
        assert np.unique(v.view(np.uint32) >> 8).size == 1 and np.unique(v).size == min(n, 256)
    elif pattern is extremes:
        assert v.min() == -FMAX and v.max() == FMAX and (v == FMIN).any() and (v < 0).sum() >= 1 and (v > 0).sum() >= 2
    elif pattern is tied_deviations:
        assert med == 2.0 and np.unique(dev).size == n // 2 + n % 2 and np.unique(v).size == n
    else:
        k = (n - 1) // 2
        near = dev[(dev > 0) & (dev < 1)]
        assert med == 1.0 and near.size == k and np.unique(near).size == k and np.unique(near.view(np.uint64) >> 16).size == 1
        assert n == 4 or near.min() <= bkg_ref.median(dev) <= near.max()      # the median of the deviations is among them


def all_cases(capacity):
    """[(pattern or None, n, values)] for every count a site of `capacity` pixels holds (and the full site), every pattern."""
    out = [(None, 0, np.zeros(0, F32))]
    for n in sorted(set(c for c in COUNTS + (capacity,) if 0 < c <= capacity)):
        for p in PATTERNS:
            v = p(n)
            if v is not None:
                check_set(p, n, v)
                out.append((p, n, v))
    return out


def scatter(flat_site, values, seed):
    """The values at random places of the blank site (a writable 1-D view)."""
    assert not flat_site.any() and values.size <= flat_site.size
    flat_site[np.random.default_rng(seed).permutation(flat_site.size)[:values.size]] = values


def cell_images(shape, cell):
    """The cases of a cell form, one set per cell -> [(image, [case per cell in row-major cell order])]."""
    ncy, ncx = -(-shape[0] // cell), -(-shape[1] // cell)
    cases = all_cases(min(1024, cell * cell))
    out = []
    for first in range(0, len(cases), ncy * ncx):
        img, group = np.zeros(shape, F32), cases[first:first + ncy * ncx]
        for slot, (p, n, v) in enumerate(group):
            cy, cx = divmod(slot, ncx)
            site = np.zeros(img[cy * cell:(cy + 1) * cell, cx * cell:(cx + 1) * cell].shape, F32)
            scatter(site.reshape(-1), v, 7 * first + slot)
            img[cy * cell:(cy + 1) * cell, cx * cell:(cx + 1) * cell] = site
        out.append((img, group))
    return out


def ring_image(ring):
    """Every case the ring of `ring` pixels around a one-pixel box holds, one site each -> image, boxes [n, 4], cases."""
    cases = all_cases(RINGS[ring])
    side = int(np.ceil(np.sqrt(len(cases))))
    img = np.zeros((side * PITCH, side * PITCH), F32)
    boxes = np.zeros((len(cases), 4), np.float64)
    for slot, (p, n, v) in enumerate(cases):
        cy, cx = (slot // side) * PITCH + PITCH // 2, (slot % side) * PITCH + PITCH // 2
        grown = np.zeros((2 * ring + 1) ** 2, F32)
        members = np.delete(np.arange(grown.size), grown.size // 2)        # every pixel of the grown window but the box pixel
        site = np.zeros(members.size, F32)
        scatter(site, v, 31 * ring + slot)
        grown[members] = site
        grown[grown.size // 2] = CENTRE
        img[cy - ring:cy + ring + 1, cx - ring:cx + ring + 1] = grown.reshape(2 * ring + 1, 2 * ring + 1)
        boxes[slot] = (cx, cy, cx, cy)
    return img, boxes, cases


def cell_reference(images, cell, niter, k):
    """Reference rows of every image, and the assertions that the clips do to the sets what the docstring says."""
    refs = [bkg_ref.background(img, cell, k, niter) for img, _ in images]
    seen = set()
    for ref, (img, group) in zip(refs, images):
        rows = ref.reshape(-1, 8)
        for (p, n, v), row in zip(group, rows):
            r = dict(zip(bkg_ref.FIELDS, row))
            assert r["n0"] == n and r["n"] <= n and r["rounds"] <= niter, (p, n, r)
            if niter == 0 or n == 0:
                assert r["n"] == n and r["rounds"] == 0 and r["L"] == -np.inf and r["H"] == np.inf
                assert (r["bkg"], r["rms"]) == bkg_ref.med_sig(v.astype(np.float64))
            elif p is all_equal:                             # the clip at [bkg, bkg] removes nothing
                assert r["n"] == n and r["rounds"] == 0 and r["L"] == r["H"] == r["bkg"] == 0.375 and r["rms"] == 0.0
                seen.add("whole")
            elif p is two_values and k < 1.0:                # both values lie one MAD from the median: 0.74 MAD removes them
                assert r["n"] == 0 and r["rounds"] == 1 and r["bkg"] == 0.0 and r["rms"] == 0.0
                seen.add("emptied")
            elif p is low_deviation_bytes and k < 1.0:      # [1 - 0.74, 1 + 0.74] keeps the 1.0s: one of them for an odd count
                assert r["n"] == 2 - n % 2 and r["rounds"] == 1 and r["bkg"] == 1.0 and r["rms"] == 0.0
                seen.add("single" if n % 2 else "pair")
            elif p is low_deviation_bytes:                   # k = 3: [1 - 4.4, 1 + 4.4] holds them all
                assert r["n"] == n and r["rounds"] == 0
                seen.add("whole")
        for row in rows[len(group):]:                        # cells of the last image that hold no case: blank
            assert row[0] == 0
    if niter:
        assert "whole" in seen and (k >= 1.0 or {"single", "emptied"} <= seen), seen
    return refs


@pytest.fixture(scope="module")
def det():
    return detector("fp32", max_batch=1, max_imgsz=160)


def upload(det, img):
    dev = det.mosaic_to_device(img)
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), img.view(np.uint32))      # finite values arrive as they are
    return dev


_CELLS = {}


def cell_scene(det, form):
    if form not in _CELLS:
        shape, cell = (LDS_SHAPE, LDS_CELL) if form == "lds" else (L2_SHAPE, L2_CELL)
        images = cell_images(shape, cell)
        _CELLS[form] = (cell, images, [upload(det, img) for img, _ in images])
    return _CELLS[form]


@pytest.mark.parametrize("niter,k", [(0, 3.0), (3, 3.0), (3, 0.5)])
@pytest.mark.parametrize("form", ["lds", "l2"])
def test_cell_sets(det, form, niter, k):
    cell, images, devs = cell_scene(det, form)
    assert (cell * cell <= 16384) == (form == "lds")
    refs = cell_reference(images, cell, niter, k)
    ncases = 0
    for i, (ref, (img, group), dev) in enumerate(zip(refs, images, devs)):
        got = det.measure_background(dev, cell=cell, k=k, niter=niter)
        assert got.shape == ref.shape and got.dtype == np.float64
        bad = got.view(np.uint64).reshape(-1, 8) != ref.view(np.uint64).reshape(-1, 8)
        for slot in np.nonzero(bad.any(1))[0]:
            p, n, _ = group[slot] if slot < len(group) else (None, 0, None)
            raise AssertionError("%s form, niter %d, k %g, image %d cell %d (%s, %d values): GPU row %s, reference row %s" % (
                form, niter, k, i, slot, p.__name__ if p else "blank", n, got.reshape(-1, 8)[slot], ref.reshape(-1, 8)[slot]))
        ncases += len(group)
    print("%s form, niter %d, k %g: %d sets in %d images equal bit for bit" % (form, niter, k, ncases, len(images)))


@pytest.mark.parametrize("ring", sorted(RINGS))
def test_ring_sets(det, ring):
    img, boxes, cases = ring_image(ring)
    ref, mags = measure_ref.measure(img, boxes, ring)
    for (p, n, v), row in zip(cases, ref):
        r = dict(zip(measure_ref.FIELDS, row))
        assert r["nring"] == n and r["npix"] == 1 and r["peak"] == float(CENTRE), (p, n, r)
        assert (r["bkg"], r["rms"]) == bkg_ref.med_sig(v.astype(np.float64)), (p, n, r)      # the two references agree on the rule
    assert max(n for _, n, _ in cases) == RINGS[ring]
    got = det.measure_sources(upload(det, img), boxes, ring=ring)
    assert got.shape == ref.shape and got.dtype == np.float64
    for i, (p, n, _) in enumerate(cases):
        what = "ring %d, site %d (%s, %d values)" % (ring, i, p.__name__ if p else "blank", n)
        for f in (0, 1, 2, 3, 4, 5, 6, 11):                  # npix nring bkg rms peak x_peak y_peak reserved: exact
            assert got[i, f:f + 1].view(np.uint64) == ref[i, f:f + 1].view(np.uint64), "%s: %s = %r on the GPU, %r in the reference" % (
                what, measure_ref.FIELDS[f], got[i, f], ref[i, f])
        for f, mag in zip((7, 8, 9, 10), mags[i]):           # sum sw swx swy: one term each
            assert abs(got[i, f] - ref[i, f]) <= 2.0 * 2.0 ** -53 * mag, "%s: %s = %r on the GPU, %r in the reference" % (
                what, measure_ref.FIELDS[f], got[i, f], ref[i, f])
    print("ring %d: %d sets equal" % (ring, len(cases)))
