"""The constructed preprocessing tiles (tests/preproc_cases.py) have the properties they are built for, measured on the numpy oracle
(oracle/preprocessing_ref.py) alone, so that a failure of tests/test_gpu_preproc_edges.py cannot be a broken case -- and so that a
change of the kernel's bracket heuristics (HALF_RANKS, NCAND, the sample size) or of a case shows up here, without a GPU."""
import warnings
import numpy as np
import pytest
import preproc_cases as K
from oracle import preprocessing_ref as P


def trace_clip(tile, lo_s, up_s):
    """The oracle's sigma-clip loop (sigma_clip_1d) on the tile's non-zero finite pixels, iteration by iteration:
    -> list of (n, median, std, lo, hi) per iteration, and the survivors.  Checked against sigma_clip_1d itself."""
    f = tile[P.nonzero_finite(tile)].astype(np.float64)
    want = P.sigma_clip_1d(f, lo_s, up_s)
    rows, nchanged = [], 1
    while nchanged != 0 and len(rows) < 5:
        med, sd = np.median(f), np.std(f)
        lo, hi = med - sd * lo_s, med + sd * up_s
        rows.append((f.size, med, sd, lo, hi))
        g = f[(f >= lo) & (f <= hi)]
        nchanged, f = f.size - g.size, g
    assert np.array_equal(f, want[0]) and np.array_equal(rows[-1][3:], want[1:], equal_nan=True)
    return rows, f


def local_density(f, centre, half):
    return np.count_nonzero(np.abs(f - centre) <= half) / (2.0 * half)


@pytest.mark.parametrize("group", ["big", "big_odd"])
def test_bimodal_first_clip_moves_the_median_out_of_the_bracket(group):
    t = K.case(group, "bimodal")
    rows, _ = trace_clip(t, 1.0, 1.0)
    assert len(rows) == 5                                            # runs to maxiters
    (n0, med0, sd0, lo0, hi0), (n1, med1, _, _, _) = rows[0], rows[1]
    f = t.ravel().astype(np.float64)
    assert np.count_nonzero(f < lo0) == 0 and n0 - n1 > 28000        # the first clip removes ~29 000 pixels, all from above
    kept = np.sort(f[f <= hi0])
    shift = np.searchsorted(kept, med0) - np.searchsorted(kept, med1)
    assert shift > K.HALF_RANKS + 4096                               # rank shift of the median (~14 700)
    # the bracket is +-HALF_RANKS / density about the old median, the density measured (a) by the sample bracket (the central ~6 % of
    # the initial set's ranks: the raw stage) or (b) inside +-sd / 32 (a stage behind another): either way it ends far above the new median
    srt = np.sort(f)
    qa, qb = srt[int(0.47 * f.size)], srt[int(0.53 * f.size)]
    rho_a = np.count_nonzero((f >= qa) & (f <= qb)) / (qb - qa)
    rho_b = local_density(f, med0, sd0 / 32.0)
    for rho in (rho_a, rho_b):
        assert med0 - med1 > 1.5 * K.HALF_RANKS / rho
    # and the sample bracket itself is sound: the raw stage's FIRST median is a hit (sample of >= 4096 pixels)
    assert f.size // 26 >= K.SAMPLE_MIN // 2


@pytest.mark.parametrize("group", ["big", "big_odd"])
def test_ties_overflow_the_bracket_on_every_trip(group):
    t = K.case(group, "ties")
    rows, last = trace_clip(t, 1.0, 1.0)
    assert len(rows) == 5
    f = t.ravel().astype(np.float64)
    for n, med, sd, lo, hi in rows:
        assert med == 1.0 and np.count_nonzero(f == med) > K.NCAND and sd > 0.0
    # the 0.48 and 0.52 quantiles of any row sample are the tied value: 60 % of the pixels
    srt = np.sort(f)
    assert srt[int(0.40 * f.size)] == 1.0 == srt[int(0.60 * f.size)]


def test_noise_control_stays_inside_its_brackets():
    t = K.case("big", "noise")
    rows, _ = trace_clip(t, 1.0, 1.0)
    f = np.sort(t.ravel().astype(np.float64))
    for (n0, m0, _, _, _), (n1, m1, _, lo, hi) in zip(rows, rows[1:]):
        assert abs(np.searchsorted(f, m0) - np.searchsorted(f, m1)) < 1024


def test_two_valued_sits_on_its_bounds():
    t = K.case("small", "two_valued")
    rows, last = trace_clip(t, 1.0, 1.0)
    assert rows == [(4096, 0.0, 1.0, -1.0, 1.0)]                      # one iteration: nothing removed, every pixel ON a bound
    assert last.size == 4096 and set(np.unique(t)) == {-1.0, 1.0}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rows, last = trace_clip(t, 0.5, 0.5)                          # bounds (-0.5, 0.5): every pixel removed, then NaN bounds
    assert [r[0] for r in rows] == [4096, 0] and last.size == 0 and np.isnan(rows[1][3]) and np.isnan(rows[1][4])
    t = K.case("small", "two_valued_odd")
    rows, last = trace_clip(t, 1.0, 1.0)
    assert [r[0] for r in rows] == [4095, 2048] and rows[0][1] == 1.0 and rows[1][2] == 0.0
    assert np.count_nonzero(t == 1.0) == 2048 and np.count_nonzero(t == -1.0) == 2047


ITERATIONS = {   # (case, clip) -> set sizes at the iterations of the oracle (it stops after the first one that removes nothing)
    ("constant_0p1", (1, 1)): [4096], ("constant_3p5", (1, 1)): [4096],
    ("sparse_1", (1, 1)): [1], ("sparse_2", (1, 1)): [2], ("sparse_3", (1, 1)): [3, 1],
    ("converges_early", (10, 10)): [4096], ("converges_early", (1, 1)): [4096, 2812, 1702, 991, 582],
}


@pytest.mark.parametrize("key", sorted(ITERATIONS))
def test_iteration_counts(key):
    name, (lo_s, up_s) = key
    rows, _ = trace_clip(K.case("small", name), float(lo_s), float(up_s))
    assert [r[0] for r in rows] == ITERATIONS[key]
    assert all(np.isfinite(r[1:]).all() for r in rows)
    if name.startswith("constant"):
        assert rows[0][2] == 0.0 and rows[0][3] == rows[0][4] == float(np.float32(float(name[9:].replace("p", "."))))
    if name == "sparse_2":                                           # both pixels exactly ON the (1, 1) bounds
        assert (rows[0][3], rows[0][4]) == (-0.75, 2.5)


def test_small_cases_are_what_they_say():
    g = dict((n, t) for n, t, _ in K.GROUPS["small"])
    assert not g["all_zero"].any()
    assert (g["all_negative"] < 0).all()
    d = g["decades"]
    assert (d > 0).sum() > 1000 and (d < 0).sum() > 1000 and np.abs(d).min() < 1e-29 and np.abs(d).max() > 1e29 and np.isfinite(d).all()
    s = g["subnormal"]
    tiny = np.finfo(np.float32).tiny
    sub = (s != 0) & (np.abs(s) < tiny)
    assert sub.sum() > 1000 and ((s != 0) & ~sub).sum() > 200 and (s == 0).sum() >= 640
    assert (s[8:24, 8:40] != 0).all() and (np.abs(s[8:24, 8:40]) < tiny).all()
    for name in ("all_negative", "decades", "subnormal", "converges_early"):
        rows, last = trace_clip(g[name], 1.0, 1.0)
        assert all(np.isfinite(r[1:]).all() for r in rows) and last.size > 0
    # medians between two distinct values (even n) occur in the traces
    rows, _ = trace_clip(g["decades"], 1.0, 1.0)
    v = np.sort(g["decades"].ravel().astype(np.float64))
    assert rows[0][0] % 2 == 0 and v[2047] != v[2048] and rows[0][1] == 0.5 * (v[2047] + v[2048])
    # every group shares one shape; the big tiles are sampled, the small ones are not
    for name, tiles in K.GROUPS.items():
        assert len({t.shape for _, t, _ in tiles}) == 1 and all(t.dtype == np.float32 for _, t, _ in tiles)
    assert K.BIG_ODD[1] % 4 != 0 and K.BIG[1] % 4 == 0


def _zs_sample(tile):
    v = tile.ravel().astype(np.float64)
    stride = int(max(1.0, v.size / P.ZS_NSAMPLES))
    return np.sort(v[::stride][:P.ZS_NSAMPLES]), stride


@pytest.mark.parametrize("group,npix,stride,ns", [("zs24", 576, 1, 576), ("zs37x31", 1147, 1, 1000), ("zs45", 2025, 2, 1000)])   # 2025 / 2 -> 1013 samples, capped
def test_zscale_cases(group, npix, stride, ns):
    for name, t, _ in K.GROUPS[group]:
        s, st = _zs_sample(t)
        assert t.size == npix and st == stride and s.size == ns
        vmin, vmax = P.zscale_limits(t.astype(np.float64), 0.25)
        assert np.isfinite([vmin, vmax]).all()
        if name == "zs_equal":
            assert s[0] == s[-1] == 2.0
            np.testing.assert_allclose([vmin, vmax], 2.0, rtol=1e-11)
        else:
            assert vmin > s[0] or vmax < s[-1]                       # the fitted line decided at least one limit
            if name != "zs_outliers":
                assert (s == 0).sum() > (0.6 * ns if name == "zs_mostly_zero" else 50)


def _zs_ngood(s):
    """the rejection loop of zscale_limits, replayed on a sorted sample: ngood after every iteration, and minpix"""
    npix = s.size
    minpix = max(P.ZS_MIN_NPIX, int(npix * P.ZS_MAX_REJECT))
    x = np.arange(npix)
    bad = np.zeros(npix, bool)
    ngood, last, out = npix, npix + 1, []
    kernel = np.ones(max(1, int(npix * 0.01)), bool)
    for _ in range(P.ZS_MAX_ITER):
        if ngood >= last or ngood < minpix:
            break
        fit = np.polyfit(x, s, 1, w=(~bad).astype(int))
        flat = s - np.poly1d(fit)(x)
        thr = P.ZS_KREJ * flat[~bad].std()
        bad[(flat < -thr) | (flat > thr)] = True
        bad = np.convolve(bad, kernel, mode="same")
        last, ngood = ngood, int(np.sum(~bad))
        out.append(ngood)
    return out, minpix


def test_zscale_rejection_iterations_and_the_minpix_floor():
    for group in ("zs24", "zs37x31", "zs45"):
        ng, minpix = _zs_ngood(_zs_sample(K.case(group, "zs_outliers"))[0])
        assert len(ng) == 5 and all(a > b for a, b in zip(ng, ng[1:])) and ng[0] - ng[-1] > 80 and ng[-1] >= minpix
    t = K.case("zs_tiny", "zs_tiny")
    s, _ = _zs_sample(t)
    ng, minpix = _zs_ngood(s)
    assert s.size == 4 < minpix == 5 and ng == []                    # ngood < minpix before the first fit
    assert P.zscale_limits(t.astype(np.float64), 0.25) == (-1.5, 8.0)


def test_quantised_pixels_lie_on_bin_edges():
    for levels, on_edge in ((257, 1.0), (513, 0.45)):
        t = K.case("heq", "quantised_%d" % levels)
        edges = np.histogram_bin_edges(t.ravel().astype(np.float64), 256)
        assert t.min() == 0 and t.max() == levels - 1
        assert np.isin(t.ravel().astype(np.float64), edges).mean() >= on_edge
    for levels in (256, 512):
        t = K.case("heq", "quantised_%d" % levels)
        assert t.min() == 0 and t.max() == levels - 1 and len(np.unique(t)) == levels
    h = K.HEQ
    assert h[1] % 4 == 0 and (h[0] * (h[1] // 4)) % 4096 == 0          # the lean histogram pass takes it


def test_mosaic_layout_puts_a_tile_flush_in_the_corner():
    for group, tiles in K.GROUPS.items():
        ts = [t for _, t, _ in tiles]
        m, xy = K.mosaic_layout(ts)
        th, tw = ts[0].shape
        assert xy[-1] == (m.shape[1] - tw, m.shape[0] - th)
        assert all(x % 4 in (1, 2, 3) for x, _ in xy[:-1])
        for t, (x, y) in zip(ts, xy):
            assert np.array_equal(m[y:y + th, x:x + tw], t)
        cover = np.zeros(m.shape, int)
        for x, y in xy:
            cover[y:y + th, x:x + tw] += 1
        assert cover.max() == 1 and np.isnan(m[cover == 0]).all()
