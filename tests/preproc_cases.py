"""Constructed tiles for the preprocessing statistics kernel (pre_stats_kernel, csrc/cy_preproc.hip): small fp32 images built so
that a sigma-clip, zscale or equalisation run takes a branch that natural radio tiles never reach -- a median bracket that misses
or overflows, a sample bracket that collapses on ties, sets of 0..3 pixels, pixels exactly on an inclusive clip bound, medians
between two distinct values, keys of both signs over sixty decades and fp32 subnormals, zscale samples below / at / above the
1000-sample cap, equalisation of quantised data whose pixels lie on bin edges.

Every constructor is deterministic (fixed seed) and returns (name, fp32 tile, what it is meant to reach).  GROUPS batches the tiles
by shape: one launch handles all tiles of a shape.  tests/test_preproc_cases_cpu.py checks on the numpy oracle that every case has
the property it is built for; tests/test_gpu_preproc_edges.py runs them through the kernel.  numpy only.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

NCAND = 24576                # capacity of the kernel's median bracket (csrc/cy_preproc.hip)
HALF_RANKS = 8192            # half-width of the first clip's bracket, in ranks
SAMPLE_MIN = 4096            # row-sample size below which a raw stage takes the histogram route for its first median

BIG = (256, 256)             # smallest size at which a bracket of +-8192 ranks can be missed; rows are whole 4-pixel groups
BIG_ODD = (250, 258)         # the same cases with tw % 4 != 0: the general loop instead of moments_plain
SMALL = (64, 64)             # 2048 sampled pixels: the `ns < 4096` route


def _rng(seed):
    return np.random.default_rng(seed)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# --------------------------------------------------------------------------- 256-class tiles
def noise(shape=BIG, seed=11):
    """plain Gaussian noise: the control -- every bracket holds its median"""
    return "noise", _f32(_rng(seed).standard_normal(shape)), "control: sample bracket and every later bracket hit"


def bimodal(shape=BIG, seed=12):
    """U(-2, 2) everywhere, +20 added to 45 % of the pixels.  Under a (1, 1) clip the first clip removes the upper cluster (all from
    above), the median moves ~14 700 ranks from ~1.64 to ~0 through a population of CONSTANT density, so a bracket of +-8192 ranks
    about the old median ends ~0.9 above the new one: a miss, whether the density came from the sample bracket (raw stage) or
    from the +-sd/32 window (stage behind another).  The survivors of a (1, 1) clip of a uniform set keep shrinking: five iterations.
    (With a Gaussian lower cluster the density rises towards the new median, the bracket of 8192 / density(old median) in VALUE is
    wider than the move, and the bracket hits although the rank shift exceeds 8192 -- hence the uniform cluster.)"""
    r = _rng(seed)
    t = r.uniform(-2.0, 2.0, shape)
    t[r.random(shape) < 0.45] += 20.0
    return "bimodal", _f32(t), "first clip moves the median > 8192 ranks at constant density: bracket miss -> radix fallback; 5 iterations"


def ties(shape=BIG, seed=13):
    """N(1.3, 0.5) with 60 % of the pixels exactly 1.0: the 0.48 / 0.52 sample quantiles are both 1.0 (the sample bracket collapses),
    and every later bracket holds the ~39 000 pixels equal to the median: more than NCAND, on each of the five trips.  (The rest is
    centred off the tied value so that the mean a BKG stage subtracts stays ~0.1 away from it: bounds of a clip behind that stage are
    then not a difference of nearly equal numbers, and 1e-11 relative stays a test of the kernel, not of the mean's last bit.)"""
    r = _rng(seed)
    t = r.normal(1.3, 0.5, shape)
    t[r.random(shape) < 0.60] = 1.0
    return "ties", _f32(t), "sample bracket collapses (hf == lf); every clip's bracket overflows NCAND -> radix fallback"


def constant_big(shape=BIG):
    return "constant_big", np.full(shape, np.float32(0.1)), "sampled route with sd == 0: collapsed sample bracket, no bracket at all"


# --------------------------------------------------------------------------- small tiles
def two_valued(shape=SMALL):
    """+-1 in alternating columns: median 0 between two distinct values, std exactly 1, (1, 1) bounds exactly (-1, 1) with every
    pixel ON a bound (inclusive: all survive); a (0.5, 0.5) clip removes every pixel (n == 0 after a clip)"""
    t = np.ones(shape)
    t[:, 1::2] = -1.0
    return "two_valued", _f32(t), "even-n median between two values; pixels exactly on inclusive bounds; n == 0 after a (0.5, 0.5) clip"


def two_valued_odd(shape=SMALL):
    """the same with one -1 pixel turned into +1 (and one pixel zeroed: an odd count): the median is +1, a tie straddling the middle"""
    _, t, _ = two_valued(shape)
    t = t.copy()
    t[5, 1] = 1.0
    t[7, 2] = 0.0
    return "two_valued_odd", t, "odd-n median inside a run of ties; the lower cluster is clipped, then sd == 0"


def constant(value, shape=SMALL):
    return "constant_%s" % str(value).replace(".", "p"), np.full(shape, np.float32(value)), "sd == 0 on the first trip; zscale sample all equal"


def sparse(k, shape=SMALL):
    """all zeros except k pixels (away from rows 0..2 and from the zscale sample stride)"""
    t = np.zeros(shape, np.float32)
    for (y, x), v in list(zip([(9, 13), (30, 7), (51, 62)], [2.5, -0.75, 7.0]))[:k]:
        t[y, x] = v
    return "sparse_%d" % k, t, "a set of %d pixel(s)" % k


def all_zero(shape=SMALL):
    return "all_zero", np.zeros(shape, np.float32), "empty initial set"


def all_negative(shape=SMALL, seed=14):
    t = -np.abs(_rng(seed).normal(3.0, 1.0, shape)) - 0.01
    return "all_negative", _f32(t), "fkey ordering of negative keys only (complemented bits)"


def decades(shape=SMALL, seed=15):
    r = _rng(seed)
    t = r.choice([-1.0, 1.0], shape) * 10.0 ** r.uniform(-30.0, 30.0, shape)
    return "decades", _f32(t), "fkey ordering over mixed signs and sixty decades of magnitude"


def subnormal(shape=SMALL, seed=16):
    """noise of sigma 1e-38 (most of its pixels are fp32 subnormals) with a block of pure subnormals and a block of zeros:
    the reference counts a subnormal as non-zero"""
    r = _rng(seed)
    t = _f32(r.normal(0.0, 1e-38, shape))
    t[8:24, 8:40] = (r.integers(1, 1 << 22, (16, 32)).astype(np.uint32) | (r.integers(0, 2, (16, 32)).astype(np.uint32) << 31)).view(np.float32)
    t[40:56, 20:60] = 0.0
    return "subnormal", t, "fp32 subnormals are non-zero set members and order correctly"


def converges_early(shape=SMALL, seed=17):
    return "converges_early", _f32(_rng(seed).normal(5.0, 2.0, shape)), "a (10, 10) clip removes nothing: stops at c >= 1 && n == nprev"


# --------------------------------------------------------------------------- zscale tiles
def _sources(t, r, frac=0.04):
    """a few bright pixels: the fitted line, not the sample's maximum, then decides the upper limit"""
    m = r.random(t.shape) < frac
    t[m] += 10.0 ** r.uniform(1.0, 3.0, t.shape)[m]
    return t


def zs_block(shape, seed=18):
    """noise and sources with a block of zeros (zeros are part of the zscale sample)"""
    h, w = shape
    r = _rng(seed + h)
    t = _sources(r.normal(10.0, 1.0, shape), r)
    t[h // 2:h // 2 + h // 4, w // 4:w // 4 + w // 2] = 0.0
    return "zs_block", _f32(t), "zscale on %d pixels: stride %d" % (h * w, max(1, h * w // 1000))


def zs_mostly_zero(shape, seed=19):
    h, w = shape
    r = _rng(seed + h)
    t = _sources(r.normal(10.0, 1.0, shape), r, 0.1)
    t[r.random(shape) < 0.8] = 0.0
    t[:3] = r.normal(10.0, 1.0, (3, w))
    return "zs_mostly_zero", _f32(t), "zscale samples that are mostly zeros"


def zs_outliers(shape, seed=20):
    """noise with 30 % outliers of either sign over three decades: the rejection loop rejects in several iterations and grows the
    rejected runs.  (It cannot end below minpix on a sample of this size: see zs_tiny.)"""
    r = _rng(seed + shape[0])
    t = r.normal(0.0, 1.0, shape)
    m = r.random(shape) < 0.3
    t[m] = (r.choice([-1.0, 1.0], shape) * 10.0 ** r.uniform(1.0, 4.0, shape))[m]
    return "zs_outliers", _f32(t), "zscale rejection over several iterations"


def zs_tiny():
    """4 x 1: four samples are fewer than minpix = 5, so the limits are the raw minimum and maximum.  An iteration of the rejection loop
    removes what lies beyond 2.5 sigma of the line's residuals -- less than 1 / 6.25 of the sample by Chebyshev's inequality, about a tenth
    once the line's tilt towards the tails (the sample is sorted) is counted -- so five iterations never reject half of a sample of
    >= 10 pixels: `ngood < minpix` is reached through the floor of 5 only."""
    return "zs_tiny", _f32([[3.0], [-1.5], [0.25], [8.0]]), "ngood < minpix: raw min / max"


def zs_equal(shape):
    return "zs_equal", np.full(shape, np.float32(2.0)), "zscale sample all equal (limits only: the reference's slope is rounding noise)"


# --------------------------------------------------------------------------- equalisation tiles (64 x 256: the lean histogram pass)
HEQ = (64, 256)


def quantised(levels, shape=HEQ, seed=21):
    """integers 0 .. levels - 1.  levels = 257: the bin width is exactly 1 and every pixel lies ON a bin edge; 513: width 2, the even
    pixels on edges and the odd ones on bin centres"""
    t = _rng(seed + levels).integers(0, levels, shape)
    t[0, :2] = [0, levels - 1]
    return "quantised_%d" % levels, _f32(t), "HISTEQ thresholds on quantised data" + (" (pixels on bin edges)" if levels in (257, 513) else "")


def two_valued_wide(shape=HEQ):
    _, t, _ = two_valued(shape)
    return "two_valued_wide", t, "HISTEQ of a two-valued tile: bins 0 and 255 only"


GROUPS = {
    "big": [noise(), bimodal(), ties(), constant_big()],
    "big_odd": [noise(BIG_ODD), bimodal(BIG_ODD), ties(BIG_ODD)],
    "small": [two_valued(), two_valued_odd(), constant(0.1), constant(3.5), sparse(1), sparse(2), sparse(3), all_zero(), all_negative(),
              decades(), subnormal(), converges_early()],
    "zs24": [zs_block((24, 24)), zs_mostly_zero((24, 24)), zs_outliers((24, 24)), zs_equal((24, 24))],
    "zs37x31": [zs_block((37, 31)), zs_mostly_zero((37, 31)), zs_outliers((37, 31))],
    "zs45": [zs_block((45, 45)), zs_mostly_zero((45, 45)), zs_outliers((45, 45))],
    "zs_tiny": [zs_tiny()],
    "heq": [quantised(256), quantised(512), quantised(257), quantised(513), two_valued_wide()],
}


def case(group, name):
    for n, t, _ in GROUPS[group]:
        if n == name:
            return t
    raise KeyError((group, name))


def mosaic_layout(tiles):
    """-> (mosaic fp32 [MH, MW] with NaN between the tiles, [(x0, y0)]): the LAST tile sits flush in the bottom-right corner (its
    last 16-byte group load of a row with tw % 4 != 0 reaches past the end of the mosaic), the others at origins with x0 % 4 in
    {1, 2, 3} and y0 in {0, 1, 2}."""
    th, tw = tiles[0].shape
    assert all(t.shape == (th, tw) for t in tiles)
    xy, x = [], 0
    for i in range(len(tiles) - 1):
        want = 1 + i % 3
        x += (want - x) % 4
        xy.append((x, i % 3))
        x += tw + 1
    mw, mh = max(x, 3) + tw, th + 3
    xy.append((mw - tw, mh - th))
    m = np.full((mh, mw), np.nan, np.float32)
    for t, (x0, y0) in zip(tiles, xy):
        m[y0:y0 + th, x0:x0 + tw] = t
    return m, xy
