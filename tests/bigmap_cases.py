"""One map of 46341 x 46339 pixels (88 049 below 2^31, just under 8 GiB of fp32, odd width) that is blank (0) but for a few 128 x 128
patches placed where an index or byte offset of the wrong width goes wrong, shared by tests/test_bigmap_cases_cpu.py (which shows
on the reference side that the construction is what it claims) and the tests/test_gpu_bigmap_*.py modules (which run every
mosaic-reading entry on it).  No GPU import at module level.

The two twins hold the same pixels: host() is np.zeros plus the patches (the allocation is lazy: only the pages of the patches are
ever touched, so never run a whole-array operation on it), device() is torch.zeros plus the same patches copied one by one.

Patches (PLACES: name -> row, column of the first pixel; placed with divmod, nothing typed in):
  low      rows around 1000: the control
  s31      pixel index 2^29 at its (64, 64): a signed 32-bit byte offset goes wrong from there
  u32      pixel index 2^30 at its (8, 0): an unsigned 32-bit byte offset wraps from there.  2^30 cannot lie further inside: the
           pixels behind it wrap to the pixels from index 0 on, and only with 2^30 in the patch's first column is that wrapped part
           a rectangle with the same columns side by side; eight rows of the patch lie before it
  hi       pixel index 3 * 2^29 at its (64, 64): both again
  end      the last 128 rows x the last 128 columns, pixel MH * MW - 1 included
  edge_r   touches the right edge mid-image;  edge_b  touches the bottom edge mid-row
Decoys (DECOY_OF: patch -> decoy): a patch of another seed whose first pixel lies exactly 2^30 pixels before the patch's first
pixel, so that a kernel whose byte offset wrapped finds data there, and other data.  The decoy of `hi` is `s31`: both have to
hold pixel 2^29, so they are one patch.  The decoy of `u32` would begin eight rows above the image; its rows 8 .. 127 are rows
0 .. 119 of the image, which is what the pixels of `u32` from 2^30 on wrap to.

A patch holds noise of sigma 0.05, an isolated elliptical Gaussian, a blended pair 5 px apart, a hole (negative Gaussian), a
linked pair 4 and 3 px from its last row and column (so that at `end` boxes and discs around it leave the image), a 3 x 3
plateau of equal pixels on top of a broad Gaussian and three blank pixels; amplitudes, sub-pixel positions and noise follow the patch's seed.

Jobs: boxes(), aperture_jobs(), peak_jobs() give the job tables of one patch in image coordinates, all_*() those of every patch
and decoy in one table.  shift() is the step from a patch to its decoy.

Crops (crop()): the patch grown by a blank halo of at least the operation's reach and aligned outwards to a grid, cut at the image.
On a side that is a real image edge the crop ends at that edge, so edge handling there is the image's.  On any other side the
operation's fold, mirror or clamp at the crop's edge stays inside the halo (asserted: halo >= reach) and reads blank pixels, as
does the same operation on the full image, which reads blank pixels beyond: the reference on the crop equals the reference on the
full image there.  tests/test_bigmap_cases_cpu.py checks that bit for bit on a small stand-in."""
import numpy as np

from fit_cases import gauss, truth_params
from peakfit_cases import job, start_of

MH, MW = 46341, 46339
P = 128
WRAP = 1 << 30
NOISE = 0.05
SIG, RATIO, PA = 1.6, 0.8, 30.0
RADIUS, LINK = 6.0, 1.5
FACTORS = (1.0, 2.0, 3.0, 5.0)
_CACHE = {}

assert MH * MW == (1 << 31) - 88049


def rc(index):
    return divmod(int(index), MW)


def _before(y, x, pixels=WRAP):
    """(row, column) of the pixel `pixels` before (y, x); the row is negative when there is none."""
    return divmod(y * MW + x - pixels, MW)


def _places():
    y29, x29 = rc(1 << 29)
    y30, x30 = rc(1 << 30)
    y3, x3 = rc(3 << 29)
    p = {"low": (936, 5000), "s31": (y29 - 64, x29 - 64), "u32": (y30 - 8, x30), "hi": (y3 - 64, x3 - 64), "end": (MH - P, MW - P),
         "edge_r": (30000, MW - P), "edge_b": (MH - P, 20000)}
    p["u32_decoy"] = _before(*p["u32"])
    p["end_decoy"] = _before(*p["end"])
    assert _before(*p["hi"]) == p["s31"]
    return p


PLACES = _places()
SEEDS = {nm: 100 + i for i, nm in enumerate(PLACES)}
DECOY_OF = {"u32": "u32_decoy", "hi": "s31", "end": "end_decoy"}
THRESHOLD_PIXEL = {"s31": 1 << 29, "u32": 1 << 30, "hi": 3 << 29, "end": MH * MW - 1}


def top(name):
    """First row of the patch that lies inside the image (8 for u32_decoy, else 0)."""
    return max(0, -PLACES[name][0])


# ---- what a patch holds (positions relative to its first pixel: x, y)
BLANKS = ((25, 15), (100, 60), (101, 61))           # (x, y)
PLATEAU = (40, 100)                                  # first (x, y) of the 3 x 3 plateau
PLATEAU_VALUE = 2.5                                  # + seed / 64: above the broad Gaussian (amplitude 2) it is set into: nine equal peak pixels, other ones on every patch
BLOBS = (("iso", 30.0, 30.0, 8.0, 1.0), ("pair_a", 70.0, 30.0, 8.0, 1.0), ("pair_b", 75.0, 30.0, 5.0, 1.0), ("hole", 30.0, 70.0, 6.0, -1.0),
         ("corner_a", 124.0, 124.0, 8.0, 1.0), ("corner_b", 120.0, 121.0, 5.0, 1.0))


def patch(name):
    """-> (pixels float32 [128, 128], model float32 [128, 128]: the drawn Gaussians alone, truth {blob: the six parameters, patch frame})."""
    key = "patch_" + name
    if key not in _CACHE:
        rng = np.random.default_rng(SEEDS[name])
        model = np.zeros((P, P), np.float64)
        truth = {}
        for nm, cx, cy, amp, sign in BLOBS:
            cx, cy, amp = cx + rng.uniform(-0.4, 0.4), cy + rng.uniform(-0.4, 0.4), amp * rng.uniform(0.8, 1.25)
            model += sign * gauss((P, P), amp, cx, cy, SIG, SIG * RATIO, PA)
            truth[nm] = truth_params(amp, cx, cy, SIG, SIG * RATIO, PA)
        px = model + gauss((P, P), 2.0, PLATEAU[0] + 1.0, PLATEAU[1] + 1.0, 2.5, 2.5, 0.0)      # under the plateau; not part of the model map
        px = (px + rng.normal(0.0, NOISE, (P, P))).astype(np.float32)
        px[px == 0] = np.float32(NOISE)                       # no accidental blank
        px[PLATEAU[1]:PLATEAU[1] + 3, PLATEAU[0]:PLATEAU[0] + 3] = np.float32(PLATEAU_VALUE + (SEEDS[name] - 100) / 64.0)
        for x, y in BLANKS:
            px[y, x] = 0.0
        _CACHE[key] = (px, model.astype(np.float32), truth)
    return _CACHE[key]


def rms_patch(name):
    """The patch of the rms map: about NOISE, seeded, with one non-positive and one NaN pixel (they add no variance)."""
    rng = np.random.default_rng(1000 + SEEDS[name])
    r = (NOISE * rng.uniform(0.8, 1.2, (P, P))).astype(np.float32)
    r[31, 29], r[30, 72] = 0.0, np.nan
    return r


def _fill_host(of):
    a = np.zeros((MH, MW), np.float32)
    for nm, (y0, x0) in PLACES.items():
        t = top(nm)
        a[y0 + t:y0 + P, x0:x0 + P] = of(nm)[t:]
    return a


def host():
    if "host" not in _CACHE:
        _CACHE["host"] = _fill_host(lambda nm: patch(nm)[0])
    return _CACHE["host"]


def host_model():
    if "host_model" not in _CACHE:
        _CACHE["host_model"] = _fill_host(lambda nm: patch(nm)[1])
    return _CACHE["host_model"]


def host_rms():
    if "host_rms" not in _CACHE:
        _CACHE["host_rms"] = _fill_host(rms_patch)
    return _CACHE["host_rms"]


def device(tdev, of=None):
    """The device twin: torch.zeros plus the patches, never an upload of the host twin.  of: name -> [128, 128] float32 (default: the
    pixels)."""
    import torch
    of = of or (lambda nm: patch(nm)[0])
    d = torch.zeros((MH, MW), dtype=torch.float32, device=tdev)
    for nm, (y0, x0) in PLACES.items():
        t = top(nm)
        d[y0 + t:y0 + P, x0:x0 + P] = torch.from_numpy(np.ascontiguousarray(of(nm)[t:])).to(tdev)
    torch.cuda.synchronize()
    return d


def disjoint():
    """No two patches share a pixel."""
    r = [(nm, y0 + top(nm), y0 + P, x0, x0 + P) for nm, (y0, x0) in PLACES.items()]
    return all(a[2] <= b[1] or b[2] <= a[1] or a[4] <= b[3] or b[4] <= a[3] for i, a in enumerate(r) for b in r[i + 1:])


# ---- jobs of one patch, in image coordinates
BOX_NAMES = ("iso", "pair", "plateau", "hole", "corner", "iso and pair")
_BOXES = np.array([[20.0, 20.0, 40.0, 40.0], [58.0, 18.0, 88.0, 42.0], [34.0, 94.0, 48.0, 108.0], [20.0, 60.0, 40.0, 80.0],
                   [108.5, 108.5, 140.0, 140.0], [18.0, 16.0, 90.0, 44.0]], np.float64)


def boxes(name):
    """[6, 4] {x1, y1, x2, y2}; `corner` reaches 12 px beyond the patch's last row and column: at `end`, beyond the image."""
    y0, x0 = PLACES[name]
    return _BOXES + np.array([x0, y0, x0, y0], np.float64)


def aperture_jobs(name):
    """[n, 3] {cx, cy, unit} with FACTORS: the outermost radius is 5 units; the last job's disc leaves the patch by 6 px."""
    y0, x0 = PLACES[name]
    j = np.array([[30.0, 30.0, 2.0], [72.3, 30.4, 2.0], [30.0, 70.0, 1.5], [41.0, 101.0, 1.0], [124.0, 124.0, 2.0]], np.float64)
    return j + np.array([x0, y0, 0.0], np.float64)


PEAK_NAMES = tuple(b[0] for b in BLOBS)


def peak_jobs(name):
    """[6, 11] peak-fit jobs (peakfit_ref.JOB_NAMES) on the blobs of BLOBS, centres on the drawn integer positions, R = 6: the
    discs of corner_a and corner_b leave the patch (at `end`: the image) on two sides."""
    y0, x0 = PLACES[name]
    return np.array([job(cx + x0, cy + y0, RADIUS, start_of(amp, cx + x0, cy + y0, SIG), bkg=0.0, sign=sign) for _, cx, cy, amp, sign in BLOBS], np.float64)


def names(with_decoys=True):
    return [nm for nm in PLACES if with_decoys or not nm.endswith("_decoy")]


def job_names(per_patch):
    return ["%s/%s" % (nm, j) for nm in names() for j in per_patch]


def all_boxes():
    return np.concatenate([boxes(nm) for nm in names()])


def all_aperture_jobs():
    return np.concatenate([aperture_jobs(nm) for nm in names()])


def all_peak_jobs():
    return np.concatenate([peak_jobs(nm) for nm in names()])


def rows_of(name, per_patch):
    """The slice of an all_*() table that holds the jobs of one patch."""
    i = names().index(name)
    return slice(i * per_patch, (i + 1) * per_patch)


def shift(name):
    """(dy, dx) from a patch to its decoy."""
    (y0, x0), (y1, x1) = PLACES[name], PLACES[DECOY_OF[name]]
    assert (y0 * MW + x0) - (y1 * MW + x1) == WRAP
    return y1 - y0, x1 - x0


# ---- crops for the entries that walk the whole map
# Halo per operation.  find_peaks reads 2 pixels around a pixel and neither folds nor clamps.  render_gaussians writes up to
# ceil(5 sigma) + 1 = 10 pixels from a centre, 7 beyond a patch.  atrous_step reads 2 * step pixels away and mirrors at the image's
# edge: a crop's own edge mirrors reads of up to 2 * step pixels back into the crop, so the halo has to be wider than 2 * step for
# them to find blank pixels, which is what the full image holds beyond the crop.  The background mesh reads its own cell only: the
# crop is aligned to the cell grid and needs no halo.
RADIUS_PEAKS, NSIGMA = 2, 5.0
HALO_PEAKS, HALO_RENDER = 4, 16
assert HALO_PEAKS >= RADIUS_PEAKS and HALO_RENDER >= 7


def halo_atrous(step):
    return 2 * step + 1


def crop_at(py, px, first, halo, grid, MH_, MW_):
    """(y0, y1, x0, x1), half-open: rows first .. 127 of the patch at (py, px) grown by `halo` on every side, then outwards to
    multiples of `grid`, cut at the image of MH_ x MW_."""
    y0, y1, x0, x1 = py + first - halo, py + P + halo, px - halo, px + P + halo
    y0, x0 = (y0 // grid) * grid, (x0 // grid) * grid
    y1, x1 = -(-y1 // grid) * grid, -(-x1 // grid) * grid
    return max(y0, 0), min(y1, MH_), max(x0, 0), min(x1, MW_)


def crop(name, halo, grid=1):
    return crop_at(*PLACES[name], top(name), halo, grid, MH, MW)


def crops(halo, grid=1):
    """name -> crop, with the claims of the module's header asserted: the crops are disjoint, and what lies between a patch and
    its crop's side is blank and at least `halo` wide unless that side is the image's edge."""
    out = {nm: crop(nm, halo, grid) for nm in PLACES}
    c = list(out.values())
    assert all(a[1] <= b[0] or b[1] <= a[0] or a[3] <= b[2] or b[3] <= a[2] for i, a in enumerate(c) for b in c[i + 1:]), "crops overlap"
    for nm, (y0, y1, x0, x1) in out.items():
        py, px = PLACES[nm]
        assert (py + top(nm) - y0 >= halo or y0 == 0) and (y1 - (py + P) >= halo or y1 == MH), nm
        assert (px - x0 >= halo or x0 == 0) and (x1 - (px + P) >= halo or x1 == MW), nm
    return out


def cut(a, c):
    return a[c[0]:c[1], c[2]:c[3]]


def peaks_on_crop(img, rms, c, k_sigma, sign):
    """peaks_ref.find_peaks on the crop c of img and rms -> (rows with x, y in image pixels, sums of |terms|)."""
    import peaks_ref
    rows, absum = peaks_ref.find_peaks(cut(img, c), cut(rms, c), k_sigma, RADIUS_PEAKS, sign)
    rows[:, 0] += c[2]
    rows[:, 1] += c[0]
    return rows, absum


def merged_peaks(img, rms, crop_table, k_sigma, sign):
    """The peaks of every crop merged in increasing (y, x), as cy_find_peaks lists those of the whole image."""
    parts = [peaks_on_crop(img, rms, c, k_sigma, sign) for c in crop_table.values()]
    rows, absum = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    order = np.lexsort((rows[:, 0], rows[:, 1]))
    return rows[order], absum[order]


def atrous_on_crop(img, c, step):
    import atrous_ref
    return atrous_ref.atrous_step(cut(img, c), step)


def background_on_crop(img, c, cell, k, niter):
    """bkg_ref.background on a crop aligned to the cell grid -> (rows [ny, nx, 8], index of its first cell (cy0, cx0))."""
    import bkg_ref
    assert c[0] % cell == 0 and c[2] % cell == 0
    return bkg_ref.background(cut(img, c), cell, k, niter), (c[0] // cell, c[2] // cell)


def render_components(place_table=None):
    """[m, 6] {A, x0, y0, a, b, c} in image pixels: the positive blobs of every patch and decoy as they were drawn."""
    out = []
    for nm, (py, px) in (place_table or PLACES).items():
        for blob, _, _, _, sign in BLOBS:
            if sign > 0:
                p = patch(nm)[2][blob].copy()
                p[1], p[2] = p[1] + px, p[2] + py
                out.append(p)
    return np.array(out, np.float64)


def render_on_crop(img, comp, c, full):
    """residual_ref.render on the crop c with the true coordinates -> (rows of the whole image, model, resid of the crop)."""
    import residual_ref
    return residual_ref.render(cut(img, c), comp, NSIGMA, origin=(c[0], c[2]), full=full)


def outside_ranges(crop_table):
    """The complement of the crops as row ranges: a list of (y0, y1, [(x0, x1), ...]) that covers every pixel outside the crops
    exactly once: rows cut at every crop's first and last row, and in each band the columns between the crops that meet it."""
    cuts = sorted({0, MH} | {v for c in crop_table.values() for v in c[:2]})
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        spans = sorted((c[2], c[3]) for c in crop_table.values() if c[0] <= a and b <= c[1])
        cols, x = [], 0
        for s0, s1 in spans:
            if s0 > x:
                cols.append((x, s0))
            x = s1
        if x < MW:
            cols.append((x, MW))
        out.append((a, b, cols))
    return out


# ---- the references of the job-type entries on the host twin, each computed once
def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def measure_reference(ring):
    import measure_ref
    return _once("meas%d" % ring, lambda: measure_ref.measure(host(), all_boxes(), ring))


def thresholds():
    """[n, 4] {bkg + 5 rms, bkg + 2.5 rms, bkg, bkg + 5 rms} from the reference's measurement rows (ring 8), as the existing tests form them."""
    import deblend_ref
    return _once("thr4", lambda: deblend_ref.thresholds(measure_reference(8)[0], 5.0, 2.5, 5.0))


def island_reference():
    import island_ref
    return _once("isl", lambda: island_ref.islands(host(), all_boxes(), thresholds()[:, :3], 8))


def deblend_reference():
    import deblend_ref
    return _once("dbl", lambda: deblend_ref.deblend(host(), all_boxes(), thresholds(), 8, 2))


def fit_inputs():
    """(bkg, ncomp, start, masks) of cy_fit_components from the component reference, as fit_cases.random_reference forms them."""
    import fit_cases
    rows, comp, masks, _ = deblend_reference()
    return _once("fit_in", lambda: fit_cases.random_inputs(host(), all_boxes(), thresholds(), rows, comp) + (masks,))


def fit_reference():
    """The variants of fit_ref on the twin, the kernel's association first."""
    import fit_ref
    return _once("fit", lambda: fit_ref.fit_variants(host(), all_boxes(), *fit_inputs()))


def blend_inputs():
    import blend_cases
    bkg, ncomp, start, masks = fit_inputs()
    return bkg, ncomp, _once("blend_start", lambda: blend_cases.random_starts(fit_reference()[0], start)), masks


def blend_reference():
    """(variants, cond) of blend_ref on the twin."""
    import blend_ref
    return _once("blend", lambda: blend_ref.fit_variants(host(), all_boxes(), *blend_inputs()))


def residual_reference():
    """(rows, sums of |terms|) of residual_ref.residual_stats with the drawn Gaussians as the model and the island masks."""
    import residual_ref
    return _once("res", lambda: residual_ref.residual_stats(host(), host_model(), all_boxes(), thresholds()[:, 2], island_reference()[1]))


def aperture_reference(with_rms):
    import aperture_ref
    return _once("aper%d" % with_rms, lambda: aperture_ref.reference(host(), host_rms() if with_rms else None, all_aperture_jobs(), FACTORS))


def peakfit_reference():
    import peakfit_ref
    return _once("pfit", lambda: peakfit_ref.fit_variants(host(), all_peak_jobs()))


def group_jobs():
    """all_peak_jobs() with the reference's single fits as starts, as the chain hands them over."""
    jobs = all_peak_jobs()
    first = peakfit_reference()[0]
    hit = np.isin(first[:, 0], (0.0, 2.0))
    jobs[hit, 5:11] = first[hit, 5:11]
    return jobs


def peakgroup_reference():
    """(variants, cond) of peakgroup_ref on the twin."""
    import peakgroup_ref
    return _once("pgrp", lambda: peakgroup_ref.fit_variants(host(), group_jobs(), LINK))
