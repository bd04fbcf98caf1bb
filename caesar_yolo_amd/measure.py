"""Catalog source measurement, host side: from the raw rows of `cy_measure_sources` (HipDetector.measure_sources) to the keys a
catalog source carries with --measure_sources.  The reference's catalog stops at boxes; this is an addition.

Raw row (lib.MEAS_NAMES): npix nring bkg rms peak x_peak y_peak sum sw swx swy reserved -- counts of valid pixels (non-zero and
finite) in the box window and in the background ring, the ring's median and 1.4826 x its median absolute deviation, the largest
valid pixel of the box and where it first occurs, the sum of (v - bkg) and the moments of the weights max(v - bkg, 0).  All positions
are 0-based pixel indices of the measured image with a pixel's centre at its index.

--measure_islands adds a second step: `cy_measure_islands` (HipDetector.measure_islands) on the same boxes with thresholds formed
from the first step's bkg and rms, raw rows lib.ISL_NAMES, keys ISLAND_KEYS (annotate_islands).

--bkg_map adds a global background and noise mesh between the two: `cy_measure_background` (HipDetector.measure_background) gives
the clipped median and MAD of every cell (raw rows lib.BKG_NAMES), fill_mesh() fills the cells without data, sample_mesh()
interpolates bilinearly between the cell centres, keys BKG_KEYS (annotate_background); the island step then takes its thresholds
from bkg_map / rms_map.

--deblend_islands adds a fourth step: `cy_deblend_islands` (HipDetector.deblend_islands) splits the island set of every box into
components by local peaks and steepest-ascent basins, raw rows lib.DBL_NAMES / lib.DBL_COMP_NAMES, keys COMPONENT_KEYS
(annotate_components).

--fit_components adds a fifth step: `cy_fit_components` (HipDetector.fit_components) fits one elliptical Gaussian to every component
by Levenberg-Marquardt from the start values fit_start() forms out of the component rows, raw rows lib.FIT_NAMES, keys FIT_KEYS on
every component dict (annotate_fits).

--fit_blends adds a sixth step: `cy_fit_blends` (HipDetector.fit_blends) fits the sum of the Gaussians of every group of touching
components (blend_groups) jointly to the union of their basins, from the single fits as starts (blend_start), raw rows
lib.BLEND_NAMES, keys BLEND_KEYS on every component dict (annotate_blends).

--residual_map adds a seventh step: `cy_render_gaussians` (HipDetector.render_gaussians) renders the sum of the fitted components
(render_selection: the joint fit where there is one, else the single fit, every peak pixel once) over the whole image into a model
map and forms the residual map; `cy_measure_residuals` (HipDetector.measure_residuals) measures the residual inside every source's
box and island set, raw rows lib.RND_NAMES / lib.RES_NAMES, keys RESIDUAL_KEYS on every source and RENDER_ITEM_KEYS on every
component dict (annotate_residuals).

--residual_peaks searches the residual map for what the fitted model does not explain: `cy_find_peaks` (HipDetector.find_peaks)
lists the local maxima of the residual at or above residual_peaks_sigma times the expanded rms map of the mesh, raw rows
lib.PEAK_NAMES, a list of dicts with PEAK_KEYS beside the catalog and SOURCE_PEAK_KEYS on every source (annotate_peaks);
--residual_holes does the same for the negated residual (SOURCE_HOLE_KEYS).  It is not one of STEPS: Chain.run() calls Chain.peaks()
after them.

--residual_scales J searches the residual map scale by scale: `cy_atrous_step` (HipDetector.atrous_step) splits it into J a trous
wavelet planes, every searched plane gets a noise mesh of its own (`cy_measure_background` with a cell that grows with the scale)
and one `cy_find_peaks` call; a list of dicts with SCALE_PEAK_KEYS beside the catalog and SOURCE_SCALE_KEYS on every source
(annotate_scale_peaks).  Not one of STEPS either: Chain.run() calls Chain.scale_peaks() after Chain.peaks().

--peak_apertures measures what the searches list: `cy_aperture_sums` (HipDetector.aperture_sums) takes concentric circular
apertures and a background annulus on the residual map around every entry of the peak lists, raw rows lib.APER_NAMES /
lib.APER_RING_NAMES, keys APERTURE_KEYS on every entry (annotate_apertures).  Chain.run() calls Chain.apertures() after the searches.

--fit_peaks gives the entries of those lists a shape: `cy_fit_peaks` (HipDetector.fit_peaks) fits one elliptical Gaussian to the
residual map on a disc around every entry (of the scale peaks: the strongest ones), a disc it shares with neighbouring entries by
a nearest-centre rule; a hole is fitted with sign -1.  Raw rows lib.PFIT_NAMES, keys GFIT_KEYS on every entry
(annotate_peak_fits).  Chain.run() calls Chain.peak_fits() after the apertures, so that their local background is there when they ran.

--fit_peak_groups (which implies --fit_peaks) then fits the entries of a list that lie closer than fit_peaks_link times their disc
radius together: `cy_fit_peak_groups` (HipDetector.fit_peak_groups) fits the sum of two to four Gaussians on the union of their
discs, started from the single fits.  Raw rows lib.PGRP_NAMES, keys GBLEND_KEYS on every entry (annotate_peak_groups).
Chain.run() calls Chain.peak_groups() after the single fits.

--subtract_peaks (which implies --fit_peaks) renders the fitted peaks into a second residual: peak_render_selection() picks per
fitted entry the group fit where there is one, else the single fit, `cy_render_signed_gaussians` subtracts them from the residual map,
`cy_disc_residuals` (HipDetector.disc_residuals) measures that second residual on the pixels every fit used, raw rows
lib.DRES_NAMES, keys GRES_KEYS on every entry (annotate_peak_residuals), and `cy_find_peaks` searches it in both signs: the lists
"residual_peaks_left" / "residual_holes_left" and SOURCE_LEFT_KEYS on every source.  Chain.run() calls Chain.subtract() last.

--forced_fit measures every rendered component again with its position and shape FIXED: forced_jobs() turns the selection of the
residual step into jobs, `cy_forced_fit` (HipDetector.forced_fit) solves per job the amplitudes of the component and its
overlapping neighbours and a local constant by weighted linear least squares, raw rows lib.FORCED_NAMES, on the detection image
and on every co-registered map of --forced_images; annotate_forced() writes the key "forced" (one dict per map, FORCED_KEYS) and,
when two maps carry a frequency, the spectral index keys FORCED_ALPHA_KEYS on every component.  Chain.run() calls Chain.forced()
after the residual step's own followers.

Everything below is float64 arithmetic on those rows: given the rows, the keys are deterministic.

plan() names the steps a config asks for and Chain runs them on one image: the one place that knows their order, what each hands to
the next and the three frames (pixels of the measured image, catalog coordinates, the frame of the WCS)."""
import math
import os
import time
from types import SimpleNamespace

import numpy as np

from . import lib as L


def _fields(names):
    """The column of every named field of a raw row: _fields(L.MEAS_NAMES).bkg == 2."""
    return SimpleNamespace(**{n: i for i, n in enumerate(names)})


MEAS, ISL, DBL, COMP, FIT, BLEND = (_fields(t) for t in (L.MEAS_NAMES, L.ISL_NAMES, L.DBL_NAMES, L.DBL_COMP_NAMES, L.FIT_NAMES, L.BLEND_NAMES))
RND, RES, BKG, PEAK = _fields(L.RND_NAMES), _fields(L.RES_NAMES), _fields(L.BKG_NAMES), _fields(L.PEAK_NAMES)
APER, APER_RING = _fields(L.APER_NAMES), _fields(L.APER_RING_NAMES)
PFIT, PFIT_JOB, PGRP, DRES = _fields(L.PFIT_NAMES), _fields(L.PFIT_JOB_NAMES), _fields(L.PGRP_NAMES), _fields(L.DRES_NAMES)
FORCED = _fields(L.FORCED_NAMES)
_PFIT_JOB_PARAMS = [getattr(PFIT_JOB, k) for k in "A x0 y0 a b c".split()]
_PFIT_PARAMS = [getattr(PFIT, k) for k in "A x0 y0 a b c".split()]
_MEAS_USED = [getattr(MEAS, k) for k in "npix bkg rms peak x_peak y_peak sum sw swx swy".split()]
_MOMENTS = ("S", "Sx", "Sy", "Sxx", "Syy", "Sxy")
_COMP_MOMENTS = [getattr(COMP, k) for k in _MOMENTS]
_ISL_MOMENTS = [getattr(ISL, k) for k in _MOMENTS + ("S_main",)]
_ISL_BOX = [ISL.xmin, ISL.xmax, ISL.ymin, ISL.ymax]
_FIT_PARAMS = [getattr(FIT, k) for k in "A x0 y0 a b c".split()]
_BLEND_PARAMS = [getattr(BLEND, k) for k in "A x0 y0 a b c".split()]
_FITTED = (0.0, 2.0)               # status of a fit or blend row that holds a result: converged, or stopped at the iteration limit

KEYS = ("npix", "bkg", "rms", "peak", "snr", "x_peak", "y_peak", "x0", "y0", "flux_sum", "flux", "ra", "dec")
ISLAND_KEYS = ("island_count", "island_npix", "island_npix_main", "island_border", "island_x1", "island_x2", "island_y1", "island_y2",
               "island_flux_sum", "island_flux", "island_flux_main", "x_isl", "y_isl", "ra_isl", "dec_isl", "major", "minor", "pa")
BKG_KEYS = ("bkg_map", "rms_map", "snr_map")
COMPONENT_KEYS = ("npeaks", "ncomponents", "components_truncated", "components_unassigned_npix", "components")
COMPONENT_ITEM_KEYS = ("x", "y", "ra", "dec", "peak", "x_peak", "y_peak", "npix", "flux_sum", "flux", "major", "minor", "pa", "main", "nsummits")
FIT_KEYS = ("fit_status", "fit_niter", "fit_npix", "fit_chi2", "fit_peak", "fit_x", "fit_y", "fit_ra", "fit_dec", "fit_major", "fit_minor",
            "fit_pa", "fit_flux", "fit_peak_err", "fit_x_err", "fit_y_err", "fit_flux_err")
BLEND_KEYS = ("blend_group", "blend_size", "blend_status", "blend_niter", "blend_npix", "blend_chi2", "blend_peak", "blend_x", "blend_y",
              "blend_ra", "blend_dec", "blend_major", "blend_minor", "blend_pa", "blend_flux", "blend_peak_err", "blend_x_err", "blend_y_err",
              "blend_flux_err")
RESIDUAL_KEYS = ("res_npix", "res_mean", "res_rms", "res_rms_box", "res_max", "res_x_max", "res_y_max", "res_flux", "res_model_flux", "res_ratio")
RENDER_ITEM_KEYS = ("rendered", "render_status")
PEAK_KEYS = ("x_peak", "y_peak", "x", "y", "ra", "dec", "peak", "rms", "snr", "npix", "nabove", "flux_sum", "flux", "in_source")
SOURCE_PEAK_KEYS, SOURCE_HOLE_KEYS = ("res_npeaks", "res_peak_snr"), ("res_nholes", "res_hole_snr")
SCALE_PEAK_KEYS = PEAK_KEYS + ("scale", "step", "strongest")
SOURCE_SCALE_KEYS = ("res_nscale_peaks", "res_scale_peak_snr")
APERTURE_KEYS = ("ap_status", "ap_clipped", "ap_radius", "ap_npix", "ap_sum", "ap_bkg", "ap_bkg_rms", "ap_nbkg", "ap_flux_sum", "ap_flux",
                 "ap_flux_err", "ap_snr", "ap_best")
GFIT_KEYS = ("gfit_status", "gfit_niter", "gfit_npix", "gfit_nexcluded", "gfit_nneigh", "gfit_crowded", "gfit_clipped", "gfit_radius", "gfit_bkg",
             "gfit_chi2", "gfit_peak", "gfit_x", "gfit_y", "gfit_ra", "gfit_dec", "gfit_major", "gfit_minor", "gfit_pa", "gfit_flux", "gfit_peak_err",
             "gfit_x_err", "gfit_y_err", "gfit_flux_err")
GBLEND_KEYS = ("gblend_group", "gblend_size", "gblend_slot", "gblend_status", "gblend_niter", "gblend_npix", "gblend_nexcluded", "gblend_chi2",
               "gblend_peak", "gblend_x", "gblend_y", "gblend_ra", "gblend_dec", "gblend_major", "gblend_minor", "gblend_pa", "gblend_flux",
               "gblend_peak_err", "gblend_x_err", "gblend_y_err", "gblend_flux_err")
GRES_KEYS = ("gres_subtracted", "gres_source", "gres_render_status", "gres_npix", "gres_mean", "gres_rms", "gres_max", "gres_x_max", "gres_y_max",
             "gres_ratio", "gres_chi2", "gres_model_flux")
SOURCE_LEFT_KEYS = ("res_npeaks_left", "res_nholes_left")
FORCED_KEYS = ("image", "status", "npix", "nneigh", "crowded", "peak", "peak_err", "bkg", "chi2", "corr_max", "flux", "flux_err")
FORCED_ALPHA_KEYS = ("forced_alpha", "forced_alpha_err", "forced_alpha_n")
FORCED_STATS = ("forced_ms", "forced_kernel_ms", "forced_maps", "forced_jobs", "forced_fitted", "forced_crowded", "forced_singular")
PEAK_LIST_NAMES = ("residual_peaks", "residual_holes", "residual_scale_peaks")     # the order the fitted lists are walked in
MAD_TO_SIGMA = 1.482602218505602   # 1 / Phi^-1(3/4): the standard deviation of a normal distribution in units of its MAD
SCALES_MAX = 6                     # most scales of --residual_scales: step 2^5 = 32 on the last
FIT_SIGMA2_MIN = 0.25              # px^2: floor of the eigenvalues of a start covariance
FWHM = 2.3548200450309493          # 2 sqrt(2 ln 2): FWHM of a Gaussian in units of its sigma


def boxes_of(sources):
    """[n, 4] float64 {x1, y1, x2, y2} of catalog source dicts."""
    return np.array([[s["x1"], s["y1"], s["x2"], s["y2"]] for s in sources], np.float64).reshape(-1, 4)


def _sky(wcs, x, y, ox, oy):
    """(ra, dec) of catalog position (x, y), (ox, oy) being catalog coordinate (0, 0) in the frame of the WCS; (None, None)
    without a WCS."""
    if wcs is None:
        return None, None
    a, d = wcs.wcs_pix2world(x + ox, y + oy, 0)
    return float(a), float(d)


def _rms_of(s, use_map):
    """The noise a source's thresholds were formed with (rms, or rms_map with use_map) as a float; 0.0 when missing."""
    rms = s.get("rms_map" if use_map else "rms")
    return float(rms) if rms else 0.0


def annotate(sources, raw, beam_area, wcs, origin=(0, 0)):
    """Adds KEYS to every source dict (in place; returns the list).  raw: [n, CY_MEAS_FIELDS] rows measured on the boxes (x1, y1,
    x2, y2) of `sources`, in the pixel frame of the measured image.
      x0, y0    centroid swx / sw, swy / sw; the centre of the box when no pixel lies above the background (sw == 0)
      snr       (peak - bkg) / rms, 0 when rms == 0
      flux_sum  sum of (v - bkg) over the box; flux = flux_sum / beam_area (pixels per beam) when beam_area > 0, else None
      ra, dec   wcs.wcs_pix2world(x0 + ox, y0 + oy, 0) when a WCS is given, else None; origin = (ox, oy) is the position of the
                measured image inside the frame the WCS describes (the serial run's --xmin / --ymin crop)."""
    if not sources:
        return sources
    raw = np.asarray(raw, np.float64).reshape(len(sources), -1)
    ox, oy = float(origin[0]), float(origin[1])
    ba = float(beam_area) if beam_area else 0.0
    for s, r in zip(sources, raw):
        npix, bkg, rms, peak, xp, yp, total, sw, swx, swy = (float(r[k]) for k in _MEAS_USED)
        if sw == 0.0:
            x0, y0 = (float(s["x1"]) + float(s["x2"])) / 2.0, (float(s["y1"]) + float(s["y2"])) / 2.0
        else:
            x0, y0 = swx / sw, swy / sw
        s["npix"] = int(npix)
        s["bkg"], s["rms"], s["peak"] = bkg, rms, peak
        s["snr"] = (peak - bkg) / rms if rms != 0.0 else 0.0
        s["x_peak"], s["y_peak"] = int(xp), int(yp)
        s["x0"], s["y0"] = x0, y0
        s["flux_sum"] = total
        s["flux"] = total / ba if ba > 0.0 else None
        s["ra"], s["dec"] = _sky(wcs, x0, y0, ox, oy)
    return sources


def box_window(box, MH, MW):
    """(wx0, wy0, h, w) of the box window of cy_measure_sources / cy_measure_islands: ix in [max(0, ceil(x1)), min(MW - 1,
    floor(x2))], iy likewise with MH; (0, 0, 0, 0) when it is empty (a NaN edge makes it empty)."""
    x1, y1, x2, y2 = (float(v) for v in box)
    if any(math.isnan(v) for v in (x1, y1, x2, y2)) or x1 > MW - 1 or y1 > MH - 1 or x2 < 0 or y2 < 0:
        return 0, 0, 0, 0
    # clipped before the conversion to int: an infinite edge is an ordinary edge beyond the image, as in the library
    fx, fy = math.ceil(x1) if x1 > 0 else 0, math.ceil(y1) if y1 > 0 else 0
    lx, ly = math.floor(x2) if x2 < MW - 1 else MW - 1, math.floor(y2) if y2 < MH - 1 else MH - 1
    if lx < fx or ly < fy:
        return 0, 0, 0, 0
    return fx, fy, ly - fy + 1, lx - fx + 1


def island_shape(S, Sx, Sy, Sxx, Syy, Sxy):
    """(major, minor, pa) from the moments of the weights about the window's first pixel: central second moments cxx = Sxx / S -
    (Sx / S)^2 etc., their eigenvalues l1 >= l2 (a negative one, from rounding, counts as 0), major / minor = FWHM * sqrt(l) in
    pixels, pa = angle of the major axis from +x towards +y in degrees, in (-90, 90], 0 when l1 == l2."""
    mx, my = Sx / S, Sy / S
    return _axes(Sxx / S - mx * mx, Syy / S - my * my, Sxy / S - mx * my)


def _axes(cxx, cyy, cxy):
    """(major, minor, pa) of the covariance [[cxx, cxy], [cxy, cyy]]: the tail of island_shape() and gaussian_shape()."""
    half, d = (cxx + cyy) / 2.0, math.hypot((cxx - cyy) / 2.0, cxy)
    l1, l2 = max(half + d, 0.0), max(half - d, 0.0)
    pa = 0.0
    if l1 != l2:
        pa = 0.5 * math.degrees(math.atan2(2.0 * cxy + 0.0, cxx - cyy))
        if pa <= -90.0:
            pa += 180.0
    return FWHM * math.sqrt(l1), FWHM * math.sqrt(l2), pa


def annotate_islands(sources, raw, win0, beam_area, wcs, origin=(0, 0)):
    """Adds ISLAND_KEYS to every source dict (in place; returns the list).  raw: [n, CY_ISL_FIELDS] rows of cy_measure_islands on
    the boxes of `sources`; win0: [n, 2] first column / row (wx0, wy0) of every box window (box_window), in the frame the catalog's
    positions are wanted in, as is the bounding box in raw.
      island_count, island_npix, island_npix_main   nislands, npix, npix_main;  island_border  nborder > 0
      island_x1 / x2 / y1 / y2   bounding box of the island set (pixel indices)
      island_flux_sum  S;  island_flux, island_flux_main = S / beam_area, S_main / beam_area when beam_area > 0, else None
      x_isl, y_isl  wx0 + Sx / S, wy0 + Sy / S;  ra_isl, dec_isl  wcs.wcs_pix2world(x_isl + ox, y_isl + oy, 0), None without a WCS
      major, minor, pa   island_shape()
    No seed: the three counts are 0, island_border False and every other key None.  status == 1 (window above the supported
    maximum): every key None.  S == 0: position and shape keys None."""
    if not sources:
        return sources
    raw = np.asarray(raw, np.float64).reshape(len(sources), -1)
    win0 = np.asarray(win0, np.float64).reshape(len(sources), 2)
    ox, oy = float(origin[0]), float(origin[1])
    ba = float(beam_area) if beam_area else 0.0
    for s, r, (wx0, wy0) in zip(sources, raw, win0):
        for k in ISLAND_KEYS:
            s[k] = None
        if r[ISL.status] != 0.0:
            continue
        s["island_count"], s["island_npix"], s["island_npix_main"] = int(r[ISL.nislands]), int(r[ISL.npix]), int(r[ISL.npix_main])
        s["island_border"] = bool(r[ISL.nborder] > 0)
        if r[ISL.nseed] == 0.0:
            continue
        s["island_x1"], s["island_x2"], s["island_y1"], s["island_y2"] = (int(v) for v in r[_ISL_BOX])
        S, Sx, Sy, Sxx, Syy, Sxy, Sm = (float(v) for v in r[_ISL_MOMENTS])
        s["island_flux_sum"] = S
        if ba > 0.0:
            s["island_flux"], s["island_flux_main"] = S / ba, Sm / ba
        if S == 0.0:
            continue
        s["x_isl"], s["y_isl"] = float(wx0) + Sx / S, float(wy0) + Sy / S
        s["major"], s["minor"], s["pa"] = island_shape(S, Sx, Sy, Sxx, Syy, Sxy)
        s["ra_isl"], s["dec_isl"] = _sky(wcs, s["x_isl"], s["y_isl"], ox, oy)
    return sources


def _bkg_of(sources, use_map):
    """[n] float64: the background a source's thresholds are formed with: bkg of annotate(), or with use_map bkg_map of the mesh."""
    return np.array([s["bkg_map" if use_map else "bkg"] for s in sources], np.float64)


def _thresholds(sources, ks, use_map):
    """(bkg [n], [bkg + k * rms for k in ks]) from bkg and rms of annotate(), or with use_map bkg_map and rms_map."""
    bkg = _bkg_of(sources, use_map)
    rms = np.array([s["rms_map" if use_map else "rms"] for s in sources], np.float64)
    return bkg, [bkg + float(k) * rms for k in ks]


def island_thresholds(sources, k_seed, k_merge, use_map=False):
    """[n, 3] float64 {seed_thr, merge_thr, bkg} from the bkg and rms the first step (annotate) left on the sources; use_map: from
    the bkg_map and rms_map of the background mesh (annotate_background) instead."""
    bkg, t = _thresholds(sources, (k_seed, k_merge), use_map)
    return np.stack(t + [bkg], 1)


# ---- source components (--deblend_islands)
def deblend_thresholds(sources, k_seed, k_merge, k_peak, use_map=False):
    """[n, 4] float64 {seed_thr, merge_thr, bkg, peak_thr}: island_thresholds() plus bkg + k_peak * rms."""
    bkg, t = _thresholds(sources, (k_seed, k_merge, k_peak), use_map)
    return np.stack(t[:2] + [bkg, t[2]], 1)


def annotate_components(sources, raw, comp, win0, beam_area, wcs, origin=(0, 0)):
    """Adds COMPONENT_KEYS to every source dict (in place; returns the list).  raw: [n, CY_DBL_FIELDS] rows and comp:
    [n, CY_DBL_MAX_COMP, CY_DBL_COMP_FIELDS] component rows of cy_deblend_islands on the boxes of `sources`; win0: [n, 2] first
    column / row (wx0, wy0) of every box window (box_window), in the frame the catalog's positions are wanted in, as are the peak
    positions in comp.
      npeaks, ncomponents   npeaks, ncomp;  components_truncated  status == 2 (more than CY_DBL_MAX_COMP peaks)
      components_unassigned_npix   npix_unassigned
      components   a list of ncomp dicts in component order (COMPONENT_ITEM_KEYS): x, y = wx0 + Sx / S, wy0 + Sy / S;  ra, dec =
                   wcs.wcs_pix2world(x + ox, y + oy, 0), None without a WCS;  peak, x_peak, y_peak;  npix;  flux_sum = S;  flux =
                   S / beam_area when beam_area > 0, else None;  major, minor, pa  island_shape();  main (bool);  nsummits
    No seed: the counts are 0 and components is an empty list.  status == 1 (window above the supported maximum): every key
    None.  S == 0: position and shape keys of that component None."""
    if not sources:
        return sources
    n = len(sources)
    raw = np.asarray(raw, np.float64).reshape(n, -1)
    comp = np.asarray(comp, np.float64).reshape(n, -1, L.CY_DBL_COMP_FIELDS)
    win0 = np.asarray(win0, np.float64).reshape(n, 2)
    ox, oy = float(origin[0]), float(origin[1])
    ba = float(beam_area) if beam_area else 0.0
    for s, r, cr, (wx0, wy0) in zip(sources, raw, comp, win0):
        for k in COMPONENT_KEYS:
            s[k] = None
        if r[DBL.status] == 1.0:
            continue
        s["npeaks"], s["ncomponents"], s["components_truncated"] = int(r[DBL.npeaks]), int(r[DBL.ncomp]), bool(r[DBL.status] == 2.0)
        s["components_unassigned_npix"] = int(r[DBL.npix_unassigned])
        items = []
        for c in cr[:int(r[DBL.ncomp])]:
            S, Sx, Sy, Sxx, Syy, Sxy = (float(v) for v in c[_COMP_MOMENTS])
            d = dict.fromkeys(COMPONENT_ITEM_KEYS)
            d["peak"], d["x_peak"], d["y_peak"], d["npix"] = float(c[COMP.peak]), int(c[COMP.x_peak]), int(c[COMP.y_peak]), int(c[COMP.npix])
            d["flux_sum"], d["main"], d["nsummits"] = S, bool(c[COMP.main] != 0.0), int(c[COMP.nsummits])
            if ba > 0.0:
                d["flux"] = S / ba
            if S != 0.0:
                d["x"], d["y"] = float(wx0) + Sx / S, float(wy0) + Sy / S
                d["major"], d["minor"], d["pa"] = island_shape(S, Sx, Sy, Sxx, Syy, Sxy)
                d["ra"], d["dec"] = _sky(wcs, d["x"], d["y"], ox, oy)
            items.append(d)
        s["components"] = items
    return sources


# ---- component fits (--fit_components)
def fit_start(comp_rows, bkg, win0):
    """Start values {A, x0, y0, a, b, c} of the fit from component rows (lib.DBL_COMP_NAMES): comp_rows [..., CY_DBL_COMP_FIELDS], bkg [...] and
    win0 [..., 2] (first column / row of the box window) broadcast against the leading axes; x0, y0 in the frame of win0 and of the
    rows' peak positions.  -> float64 [..., 6].
      A        peak - bkg
      centre   the moment centroid win0 + (Sx / S, Sy / S)
      a, b, c  the inverse of the central-moment covariance (cxx = Sxx / S - (Sx / S)^2 ...) with its eigenvalues floored at
               FIT_SIGMA2_MIN = 0.25 px^2 (the eigenvectors stay)
      S <= 0, or a moment, the centroid or the covariance not finite: the peak position and a circular sigma of 1 px (a = c = 1,
      b = 0)."""
    r = np.asarray(comp_rows, np.float64)
    lead = r.shape[:-1]
    bkg = np.broadcast_to(np.asarray(bkg, np.float64).reshape(np.shape(bkg) + (1,) * (len(lead) - np.ndim(bkg))), lead)
    w0 = np.asarray(win0, np.float64)
    w0 = np.broadcast_to(w0.reshape(w0.shape[:-1] + (1,) * (len(lead) - (w0.ndim - 1)) + (2,)), lead + (2,))
    S, Sx, Sy, Sxx, Syy, Sxy = (r[..., k] for k in _COMP_MOMENTS)
    with np.errstate(all="ignore"):
        mx, my = Sx / S, Sy / S
        cxx, cyy, cxy = Sxx / S - mx * mx, Syy / S - my * my, Sxy / S - mx * my
        half, d = (cxx + cyy) / 2.0, np.hypot((cxx - cyy) / 2.0, cxy)
        l1, l2 = np.maximum(half + d, FIT_SIGMA2_MIN), np.maximum(half - d, FIT_SIGMA2_MIN)
        th = 0.5 * np.arctan2(2.0 * cxy, cxx - cyy)
        cs, sn = np.cos(th), np.sin(th)
        vxx, vyy, vxy = l1 * cs * cs + l2 * sn * sn, l1 * sn * sn + l2 * cs * cs, (l1 - l2) * sn * cs
        det = l1 * l2
        a, b, c = vyy / det, -vxy / det, vxx / det
        good = (S > 0.0) & np.isfinite(S) & np.isfinite(mx) & np.isfinite(my) & np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
    out = np.empty(lead + (6,), np.float64)
    out[..., 0] = r[..., COMP.peak] - bkg
    out[..., 1] = np.where(good, w0[..., 0] + mx, r[..., COMP.x_peak])
    out[..., 2] = np.where(good, w0[..., 1] + my, r[..., COMP.y_peak])
    out[..., 3] = np.where(good, a, 1.0)
    out[..., 4] = np.where(good, b, 0.0)
    out[..., 5] = np.where(good, c, 1.0)
    return out


def gaussian_shape(a, b, c):
    """(major, minor, pa) of a fitted Gaussian with inverse covariance [[a, b], [b, c]]: FWHM * sqrt of the eigenvalues of the
    covariance, in pixels; pa as island_shape(): angle of the major axis from +x towards +y in degrees, in (-90, 90], 0 for a
    circle."""
    det = a * c - b * b
    return _axes(c / det, a / det, -b / det)


def fit_flux(p, beam_area):
    """Integrated flux of the model p = (A, x0, y0, a, b, c): 2 pi A / sqrt(a c - b^2) pixel-sums, over the beam area."""
    return 2.0 * math.pi * p[0] / math.sqrt(p[3] * p[5] - p[4] * p[4]) / beam_area


def fit_flux_grad(p, beam_area):
    """Gradient of fit_flux() with respect to the six parameters (the centre does not enter)."""
    f, D = fit_flux(p, beam_area), p[3] * p[5] - p[4] * p[4]
    return np.array([f / p[0], 0.0, 0.0, -0.5 * f * p[5] / D, f * p[4] / D, -0.5 * f * p[3] / D], np.float64)


def fit_covariance(row, rms):
    """rms^2 * inv(H) from a fit row (lib.FIT_NAMES), the covariance of the six parameters for uncorrelated noise of that rms; None
    when H is singular or not finite."""
    H = np.zeros((6, 6), np.float64)
    H[np.triu_indices(6)] = np.asarray(row, np.float64)[FIT.H00:FIT.H55 + 1]
    H = H + np.triu(H, 1).T
    if not np.isfinite(H).all():
        return None
    try:
        cov = np.linalg.inv(H) * (float(rms) * float(rms))
    except np.linalg.LinAlgError:
        return None
    return cov if np.isfinite(cov).all() and (np.diag(cov) >= 0.0).all() else None


def annotate_fits(sources, fit, beam_area, wcs, origin=(0, 0), use_map=False):
    """Adds FIT_KEYS to every component dict of every source (in place; returns the list), after annotate_components().  fit:
    [n, CY_DBL_MAX_COMP, CY_FIT_FIELDS] rows of cy_fit_components with x0, y0 in the frame the catalog's positions are wanted in.
      fit_status, fit_niter, fit_npix   as in the row
      fit_chi2   F / rms^2 with the source's rms (rms_map with use_map); None when that is missing or 0
      fit_peak = A, fit_x, fit_y; fit_ra, fit_dec  wcs.wcs_pix2world(fit_x + ox, fit_y + oy, 0), None without a WCS
      fit_major, fit_minor, fit_pa   gaussian_shape(a, b, c)
      fit_flux   fit_flux(): 2 pi A / sqrt(a c - b^2) / beam_area, None without a beam
      fit_peak_err, fit_x_err, fit_y_err   square roots of the diagonal of fit_covariance() = rms^2 inv(H); fit_flux_err =
                 sqrt(g^T cov g) with g = fit_flux_grad(): first-order propagation.  None without rms or with a singular H
    With status 1, 3 or 4 every key but fit_status, fit_niter and fit_npix is None.  A source whose components are None (window above
    the supported maximum) is left alone."""
    if not sources:
        return sources
    fit = np.asarray(fit, np.float64).reshape(len(sources), -1, L.CY_FIT_FIELDS)
    ox, oy = float(origin[0]), float(origin[1])
    ba = float(beam_area) if beam_area else 0.0
    for s, fr in zip(sources, fit):
        rms = _rms_of(s, use_map)
        for d, r in zip(s.get("components") or [], fr):
            for k in FIT_KEYS:
                d[k] = None
            st = int(r[FIT.status])
            d["fit_status"], d["fit_niter"], d["fit_npix"] = st, int(r[FIT.niter]), int(r[FIT.npix])
            if st in (0, 2):
                _gaussian_keys(d, "fit_", r, FIT.F, _FIT_PARAMS, fit_covariance, rms, ba, wcs, ox, oy)
    return sources


def _gaussian_keys(d, pre, r, F, params, covariance, rms, ba, wcs, ox, oy):
    """The value and error keys <pre>chi2 .. <pre>flux_err of component dict d from its fitted row r of cy_fit_components (pre
    "fit_") or cy_fit_blends ("blend_"): F, params are the row's columns of the sum of squares and of the six parameters,
    covariance(r, rms) gives their covariance or None."""
    p = [float(v) for v in r[params]]
    d[pre + "chi2"] = float(r[F]) / (rms * rms) if rms > 0.0 else None
    d[pre + "peak"], d[pre + "x"], d[pre + "y"] = p[0], p[1], p[2]
    d[pre + "major"], d[pre + "minor"], d[pre + "pa"] = gaussian_shape(p[3], p[4], p[5])
    d[pre + "ra"], d[pre + "dec"] = _sky(wcs, p[1], p[2], ox, oy)
    if ba > 0.0:
        d[pre + "flux"] = fit_flux(p, ba)
    cov = covariance(r, rms) if rms > 0.0 else None
    if cov is not None:
        d[pre + "peak_err"], d[pre + "x_err"], d[pre + "y_err"] = (math.sqrt(cov[k, k]) for k in range(3))
        if ba > 0.0:
            g = fit_flux_grad(p, ba)
            d[pre + "flux_err"] = math.sqrt(max(float(g @ cov @ g), 0.0))


def fit_iterations(fit):
    """(jobs, mean niter, largest niter) over the fitted rows (status 0 or 2) of cy_fit_components; (0, 0.0, 0) without one."""
    fit = np.asarray(fit, np.float64).reshape(-1, L.CY_FIT_FIELDS)
    it = fit[(fit[:, FIT.niter] > 0) & np.isin(fit[:, FIT.status], _FITTED), FIT.niter]
    return (int(it.size), float(it.mean()), int(it.max())) if it.size else (0, 0.0, 0)


# ---- joint fits of blends (--fit_blends)
def blend_groups(mask, h, w, ncomp):
    """The grouping of cy_fit_blends on one mask (h x w bytes as cy_deblend_islands writes them): components k and l (< ncomp) are
    adjacent when a pixel with byte k + 1 has a pixel with byte l + 1 among its 8 neighbours inside the window; a group is a
    connected set of that graph.  -> int64 [ncomp, 3] {group id (lowest member), members M, slot (position among the members in
    increasing index)}."""
    ncomp = int(ncomp)
    m = np.asarray(mask, np.uint8).reshape(int(h), int(w)).astype(np.int64)
    adj = np.eye(ncomp, dtype=bool)
    if ncomp and m.size:
        for a, b in ((m[:, :-1], m[:, 1:]), (m[:-1, :], m[1:, :]), (m[:-1, :-1], m[1:, 1:]), (m[:-1, 1:], m[1:, :-1])):
            ok = (a >= 1) & (a <= ncomp) & (b >= 1) & (b <= ncomp) & (a != b)
            adj[a[ok] - 1, b[ok] - 1] = True
            adj[b[ok] - 1, a[ok] - 1] = True
    group = np.arange(ncomp)
    for _ in range(ncomp):                                   # lowest index reachable: ncomp rounds reach every member of a chain
        for k in range(ncomp):
            group[k] = group[adj[k]].min()
    out = np.zeros((ncomp, 3), np.int64)
    for k in range(ncomp):
        members = np.nonzero(group == group[k])[0]
        out[k] = [group[k], members.size, int(np.searchsorted(members, k))]
    return out


def blend_start(fit_rows, comp_rows, bkg, win0):
    """One start {A, x0, y0, a, b, c} per component for cy_fit_blends: the parameters of its cy_fit_components row (fit_rows
    [..., CY_FIT_FIELDS]) when that row's status is 0 or 2, else fit_start(comp_rows, bkg, win0).  Both in the same pixel frame.
    -> float64 [..., 6]."""
    fit_rows = np.asarray(fit_rows, np.float64)
    out = fit_start(comp_rows, bkg, win0)
    use = np.isin(fit_rows[..., FIT.status], _FITTED) & (fit_rows[..., FIT.niter] > 0.0)     # niter 0: a row beyond ncomp
    out[use] = fit_rows[..., _FIT_PARAMS][use]
    return out


def blend_covariance(row, rms):
    """rms^2 times the member's 6 x 6 block of inv(H) from a blend row (lib.BLEND_NAMES); None when cov_ok is 0 or it is not finite."""
    row = np.asarray(row, np.float64)
    if row[BLEND.cov_ok] == 0.0:
        return None
    C = np.zeros((6, 6), np.float64)
    C[np.triu_indices(6)] = row[BLEND.C00:BLEND.C55 + 1]
    C = (C + np.triu(C, 1).T) * (float(rms) * float(rms))
    return C if np.isfinite(C).all() and (np.diag(C) >= 0.0).all() else None


def annotate_blends(sources, rows, beam_area, wcs, origin=(0, 0), use_map=False):
    """Adds BLEND_KEYS to every component dict of every source (in place; returns the list), after annotate_fits().  rows:
    [n, CY_DBL_MAX_COMP, CY_BLEND_FIELDS] rows of cy_fit_blends with x0, y0 in the frame the catalog's positions are wanted in.
      blend_group, blend_size, blend_status, blend_niter, blend_npix   group, nmembers, status, niter, npix of the row
      blend_chi2   F / rms^2 of the job with the source's rms (rms_map with use_map); None when that is missing or 0
      blend_peak = A, blend_x, blend_y; blend_ra, blend_dec; blend_major, blend_minor, blend_pa (gaussian_shape); blend_flux
      (fit_flux): as their fit_ namesakes, from the member's parameters of the joint fit
      blend_peak_err, blend_x_err, blend_y_err, blend_flux_err   from rms^2 times the member's block of C (blend_covariance),
                 the flux by fit_flux_grad(); None without rms or with cov_ok == 0
    Status 6 (the component is alone): blend_chi2 and the value and error keys repeat the component's fit_ values, so that one set
    of columns describes every component.  Status 1, 3, 4 or 5: they are None.  A source whose components are None is left alone."""
    if not sources:
        return sources
    rows = np.asarray(rows, np.float64).reshape(len(sources), -1, L.CY_BLEND_FIELDS)
    ox, oy = float(origin[0]), float(origin[1])
    ba = float(beam_area) if beam_area else 0.0
    for s, br in zip(sources, rows):
        rms = _rms_of(s, use_map)
        for d, r in zip(s.get("components") or [], br):
            for k in BLEND_KEYS:
                d[k] = None
            st = int(r[BLEND.status])
            d["blend_group"], d["blend_size"], d["blend_status"] = int(r[BLEND.group]), int(r[BLEND.nmembers]), st
            d["blend_niter"], d["blend_npix"] = int(r[BLEND.niter]), int(r[BLEND.npix])
            if st == 6:
                for k in BLEND_KEYS[BLEND_KEYS.index("blend_chi2"):]:
                    d[k] = d.get("fit_" + k[len("blend_"):])
            elif st in (0, 2):
                _gaussian_keys(d, "blend_", r, BLEND.F, _BLEND_PARAMS, blend_covariance, rms, ba, wcs, ox, oy)
    return sources


def blend_stats(rows):
    """(jobs, mean niter, largest niter, groups above CY_BLEND_MAX_MEMBERS) over the rows of cy_fit_blends: a fitted job (status 0
    or 2) is counted once, on its slot-0 row, as is a group above the limit (status 5); (0, 0.0, 0, 0) without any."""
    rows = np.asarray(rows, np.float64).reshape(-1, L.CY_BLEND_FIELDS)
    first = rows[:, BLEND.slot] == 0.0
    it = rows[first & (rows[:, BLEND.niter] > 0) & np.isin(rows[:, BLEND.status], _FITTED), BLEND.niter]
    over = int((first & (rows[:, BLEND.status] == 5.0)).sum())
    return (int(it.size), float(it.mean()), int(it.max()), over) if it.size else (0, 0.0, 0, over)


# ---- model and residual maps (--residual_map)
def _fitted_params(fit_row, blend_row):
    """The six parameters a component is rendered with: those of its blend row when that row's status is 0 or 2, else those of its
    fit row when that row's status is 0 or 2, else None."""
    if blend_row is not None and blend_row[BLEND.status] in _FITTED:
        return blend_row[_BLEND_PARAMS]
    if fit_row[FIT.status] in _FITTED:
        return fit_row[_FIT_PARAMS]
    return None


def render_selection(sources, fit_rows, blend_rows=None):
    """The components cy_render_gaussians is given, after annotate_components() on `sources`.  fit_rows [n, CY_DBL_MAX_COMP, CY_FIT_FIELDS] /
    blend_rows [n, CY_DBL_MAX_COMP, CY_BLEND_FIELDS] (or None): the rows of cy_fit_components / cy_fit_blends with their centres in the pixel frame
    of the image that is rendered.  Per component of every source, in source order, then component order:
      parameters   the blend row's when its status is 0 or 2, else the fit row's when its status is 0 or 2, else it is not rendered
      duplicates   overlapping boxes share islands, so the same peak can be a component of two sources; a component whose kept peak
                   pixel (x_peak, y_peak) was already taken by an earlier rendered component is not rendered: the model counts a
                   peak once
    -> (comp float64 [m, 6] {A, x0, y0, a, b, c}, index int64 [m, 2] {source, component}, the number of duplicates left out)."""
    n = len(sources)
    fit_rows = np.asarray(fit_rows, np.float64).reshape(n, L.CY_DBL_MAX_COMP, L.CY_FIT_FIELDS)
    blend_rows = None if blend_rows is None else np.asarray(blend_rows, np.float64).reshape(n, L.CY_DBL_MAX_COMP, L.CY_BLEND_FIELDS)
    comp, index, taken, ndup = [], [], set(), 0
    for i, s in enumerate(sources):
        for k, d in enumerate(s.get("components") or []):
            p = _fitted_params(fit_rows[i, k], None if blend_rows is None else blend_rows[i, k])
            peak = (int(d["x_peak"]), int(d["y_peak"]))
            if p is None:
                continue
            if peak in taken:
                ndup += 1
                continue
            taken.add(peak)
            comp.append(p)
            index.append((i, k))
    return np.array(comp, np.float64).reshape(-1, 6), np.array(index, np.int64).reshape(-1, 2), ndup


def annotate_residuals(sources, raw, index, render_rows, beam_area, origin=(0, 0), use_map=False):
    """Adds RESIDUAL_KEYS to every source dict and RENDER_ITEM_KEYS to every component dict (in place; returns the list).  raw:
    [n, CY_RES_FIELDS] rows of cy_measure_residuals; index, render_rows: what render_selection() and cy_render_gaussians returned.
      rendered, render_status   whether the component is part of the model, and the status of its render row (0, 2: rendered; 1, 3:
                   skipped by the library); None for a component that was not selected
      res_npix     valid pixels of the island set; res_mean = sum_isl / npix_isl, res_rms = sqrt(sumsq_isl / npix_isl)
      res_rms_box  sqrt(sumsq_win / npix_win), None when the window has no valid pixel
      res_max      largest |residual| of the island set, res_x_max, res_y_max its position (+ origin)
      res_flux     sum_isl / beam_area, res_model_flux = model_isl / beam_area; None without a beam
      res_ratio    res_rms / rms (rms_map with use_map); None when that is missing or 0
    Status 1 (window above the supported maximum) or npix_isl == 0: every value but res_npix (0) is None."""
    if not sources:
        return sources
    raw = np.asarray(raw, np.float64).reshape(len(sources), -1)
    ox, oy = int(origin[0]), int(origin[1])
    ba = float(beam_area) if beam_area else 0.0
    render_rows = np.asarray(render_rows).reshape(-1, L.CY_RND_FIELDS)
    status = {(int(i), int(k)): int(r[RND.status]) for (i, k), r in zip(np.asarray(index).reshape(-1, 2), render_rows)}
    for i, (s, r) in enumerate(zip(sources, raw)):
        for k, d in enumerate(s.get("components") or []):
            st = status.get((i, k))
            d["rendered"], d["render_status"] = st in (0, 2), st
        for key in RESIDUAL_KEYS:
            s[key] = None
        n_isl = int(r[RES.npix_isl]) if r[RES.status] == 0.0 else 0
        s["res_npix"] = n_isl
        if n_isl == 0:
            continue
        rms = _rms_of(s, use_map)
        s["res_mean"], s["res_rms"] = float(r[RES.sum_isl]) / n_isl, math.sqrt(float(r[RES.sumsq_isl]) / n_isl)
        s["res_rms_box"] = math.sqrt(float(r[RES.sumsq_win]) / float(r[RES.npix_win])) if r[RES.npix_win] > 0 else None
        s["res_max"], s["res_x_max"], s["res_y_max"] = float(r[RES.maxabs_isl]), int(r[RES.x_max]) + ox, int(r[RES.y_max]) + oy
        if ba > 0.0:
            s["res_flux"], s["res_model_flux"] = float(r[RES.sum_isl]) / ba, float(r[RES.model_isl]) / ba
        s["res_ratio"] = s["res_rms"] / rms if rms > 0.0 else None
    return sources


# ---- forced photometry (--forced_fit, --forced_images)
def forced_config(config):
    """(nsigma, fit_bkg, the list of map paths) of --forced_fit from a config dictionary; forced_images is a list or a
    comma-separated string."""
    images = config.get('forced_images') or []
    if isinstance(images, str):
        images = [p for p in (q.strip() for q in images.split(',')) if p]
    return float(config.get('forced_nsigma', 3.0)), bool(int(config.get('forced_fit_bkg', 1))), list(images)


def wants_forced(config):
    """Whether Chain.forced() runs: forced_fit, or a map named in forced_images."""
    return bool(config.get('forced_fit', False)) or bool(forced_config(config)[2])


def header_beam_area(h):
    """The beam area in pixels from a FITS header as SFinder._beam_info forms it: pi BMAJ BMIN / (4 ln 2) / |CDELT1 CDELT2|; 0 when
    one of CDELT1, CDELT2, BMAJ, BMIN, BPA is missing or there is no header."""
    if h is None or any(k not in h for k in ("CDELT1", "CDELT2", "BMAJ", "BMIN", "BPA")):
        return 0
    return float(np.pi * h["BMAJ"] * h["BMIN"] / (4 * np.log(2)) / np.abs(h["CDELT1"] * h["CDELT2"]))


def header_frequency(h):
    """The frequency of a map from its FITS header: the first of RESTFRQ, RESTFREQ, FREQ, or CRVAL3 / CRVAL4 whose CTYPE starts with
    FREQ, that holds a positive finite number (a continuum map's RESTFRQ = 0 is passed over); None without one."""
    if h is None:
        return None
    cand = [h[k] for k in ("RESTFRQ", "RESTFREQ", "FREQ") if k in h]
    cand += [h["CRVAL%d" % ax] for ax in (3, 4) if str(h["CTYPE%d" % ax] if "CTYPE%d" % ax in h else "").strip().upper().startswith("FREQ") and "CRVAL%d" % ax in h]
    for v in cand:
        try:
            v = float(v)
        except (TypeError, ValueError):
            continue
        if math.isfinite(v) and v > 0.0:
            return v
    return None


def forced_jobs(comp, index, sources, use_map=False, mesh=None, cell=0):
    """The jobs of cy_forced_fit ([m, CY_FORCED_JOB_FIELDS] {x0, y0, a, b, c, bkg}) for the components render_selection() chose: comp
    [m, 6] {A, x0, y0, a, b, c} in the pixel frame of the map, index [m, 2] {source, component}.  bkg without a mesh: the background
    of the job's source (bkg_map with use_map, else bkg), the detection image's own; with `mesh` ([ncy, ncx, 2] of another map, cell
    wide): sample_mesh() of its bkg plane at the component's centre; mesh == 0 (a scalar): 0."""
    comp = np.asarray(comp, np.float64).reshape(-1, 6)
    index = np.asarray(index, np.int64).reshape(-1, 2)
    jobs = np.zeros((comp.shape[0], L.CY_FORCED_JOB_FIELDS), np.float64)
    jobs[:, :5] = comp[:, 1:]
    if comp.shape[0] == 0:
        return jobs
    if mesh is None:
        jobs[:, 5] = _bkg_of(sources, use_map)[index[:, 0]]
    elif np.ndim(mesh) > 0:
        jobs[:, 5] = sample_mesh(np.asarray(mesh, np.float64)[:, :, 0], cell, comp[:, 1], comp[:, 2])
    return jobs


def forced_alpha(points):
    """The spectral index of one component.  points: (nu, S, sigma_S) per map; those with S > 0 and a finite sigma_S > 0 enter a
    weighted least-squares line of ln S on ln nu with weights (S / sigma_S)^2 (the inverse variance of ln S to first order).
    -> (alpha, alpha_err, n): with x = ln nu about its weighted mean, the slope sum w x y / sum w x^2, its error 1 / sqrt(sum w x^2),
    and the number of points; (None, None, None) with fewer than two points or fewer than two different frequencies."""
    pts = [(math.log(nu), math.log(S), (S / e) ** 2) for nu, S, e in points
           if nu and S is not None and e is not None and S > 0.0 and e > 0.0 and math.isfinite(S) and math.isfinite(e)]
    if len(pts) < 2 or len({x for x, _, _ in pts}) < 2:
        return None, None, None
    sw = sum(w for _, _, w in pts)
    xm = sum(w * x for x, _, w in pts) / sw
    sxx, sxy = sum(w * (x - xm) * (x - xm) for x, _, w in pts), sum(w * (x - xm) * y for x, y, w in pts)
    if not sxx > 0.0:
        return None, None, None
    return sxy / sxx, 1.0 / math.sqrt(sxx), len(pts)


def annotate_forced(sources, index, maps):
    """Adds "forced" to every component dict of every source (in place; returns the list), and FORCED_ALPHA_KEYS when at least two
    maps carry a frequency.  index: [m, 2] {source, component} of render_selection(); maps: one dict per measured map, in the order
    they were measured: tag, rows ([m, CY_FORCED_FIELDS] of cy_forced_fit), jobs ([m, CY_FORCED_JOB_FIELDS]), beam_area (0: none),
    freq (None: none) and err_scale ([m] what sqrt(amp_var) is multiplied with: 1 for a weighted fit, the source's rms for an
    unweighted one; None, or an entry that is not > 0: the errors are None).  Per rendered component "forced" is a list with one dict of FORCED_KEYS per map:
      image = tag; status, npix, nneigh, crowded as in the row
      peak = amp, peak_err = sqrt(amp_var) * err_scale, bkg = the job's bkg + bkg_off, chi2, corr_max as in the row
      flux = peak * 2 pi / sqrt(a c - b^2) / beam_area of that map, flux_err likewise from peak_err; None without a beam
    The value keys (peak .. flux_err) are None for a status other than 0 and 2.  A component that was not rendered gets None.
    forced_alpha, forced_alpha_err, forced_alpha_n: forced_alpha() over the maps with a frequency and status 0 or 2, S the flux when
    every map with a frequency has a beam, else the peak."""
    index = np.asarray(index, np.int64).reshape(-1, 2)
    with_freq = [m for m in maps if m.get("freq")]
    use_flux = bool(with_freq) and all(m.get("beam_area") for m in with_freq)
    for s in sources:
        for d in s.get("components") or []:
            d["forced"] = None
    for t, (i, k) in enumerate(index):
        d = sources[int(i)]["components"][int(k)]
        out, points = [], []
        for m in maps:
            r, j = np.asarray(m["rows"], np.float64)[t], np.asarray(m["jobs"], np.float64)[t]
            e = {key: None for key in FORCED_KEYS}
            st = int(r[FORCED.status])
            e.update(image=m["tag"], status=st, npix=int(r[FORCED.npix]), nneigh=int(r[FORCED.nneigh]), crowded=int(r[FORCED.crowded]))
            if st in (0, 2):
                scale = None if m.get("err_scale") is None else float(np.asarray(m["err_scale"], np.float64)[t])
                if scale is not None and not scale > 0.0:      # an unweighted fit of a source without a noise: no error
                    scale = None
                e["peak"], e["bkg"] = float(r[FORCED.amp]), float(j[5]) + float(r[FORCED.bkg_off])
                e["chi2"], e["corr_max"] = float(r[FORCED.chi2]), float(r[FORCED.corr_max])
                e["peak_err"] = None if scale is None else math.sqrt(max(float(r[FORCED.amp_var]), 0.0)) * scale
                ba = float(m["beam_area"]) if m.get("beam_area") else 0.0
                if ba > 0.0:
                    f = 2.0 * math.pi / math.sqrt(j[2] * j[4] - j[3] * j[3]) / ba
                    e["flux"], e["flux_err"] = e["peak"] * f, None if e["peak_err"] is None else e["peak_err"] * f
                if m.get("freq"):
                    points.append((float(m["freq"]), e["flux"] if use_flux else e["peak"], e["flux_err"] if use_flux else e["peak_err"]))
            out.append(e)
        d["forced"] = out
        if len(with_freq) >= 2:
            d["forced_alpha"], d["forced_alpha_err"], d["forced_alpha_n"] = forced_alpha(points)
    return sources


# ---- residual peaks (--residual_peaks, --residual_holes)
def annotate_peaks(sources, rows, total, min_above, beam_area, wcs, origin=(0, 0), holes=False, keys=None):
    """The peak list of a residual map, and the peak keys of every source.  rows: [n, CY_PEAK_FIELDS] rows of cy_find_peaks with x, y
    in catalog coordinates, in the library's order; total: the number of peaks it counted (rows holds the first n of them).  A row
    is kept when nabove >= min_above.  -> a list of dicts (PEAK_KEYS) in decreasing snr, equal snr in row order:
      x_peak, y_peak   the pixel (ints);  x, y = x_peak + swx / sw, y_peak + swy / sw (sw > 0 at a peak)
      ra, dec          wcs.wcs_pix2world(x + ox, y + oy, 0), None without a WCS; origin = (ox, oy) as in annotate()
      peak             the signed value of the residual map;  rms, snr, npix, nabove as in the row
      flux_sum         the signed sum over the neighbourhood (holes: minus the row's sum, which is taken of the negated map);
                       flux = flux_sum / beam_area when beam_area > 0, else None
      in_source        index of the first source whose box contains the peak pixel (x1 <= x_peak <= x2 and y1 <= y_peak <= y2), else None
    Every source dict gets SOURCE_PEAK_KEYS (holes: SOURCE_HOLE_KEYS): the number of kept peaks inside its box (a peak counts for every
    box that contains it) and the largest snr among them, None without one.  keys: other names for those two (count key, snr key);
    a key that is None is not written (the search of the second residual writes a count only, under a name of its own)."""
    rows = np.asarray(rows, np.float64).reshape(-1, L.CY_PEAK_FIELDS)
    assert int(total) >= rows.shape[0]
    ox, oy = float(origin[0]), float(origin[1])
    ba = float(beam_area) if beam_area else 0.0
    sign = -1.0 if holes else 1.0
    kept = rows[rows[:, PEAK.nabove] >= float(min_above)]
    kept = kept[np.argsort(-kept[:, PEAK.snr], kind="stable")]
    first = _peaks_in_boxes(sources, kept, keys if keys is not None else SOURCE_HOLE_KEYS if holes else SOURCE_PEAK_KEYS)
    return [_peak_entry(PEAK_KEYS, r, f, sign, ba, wcs, ox, oy) for r, f in zip(kept, first)]


def _peaks_in_boxes(sources, kept, keys):
    """Which of the peak rows `kept` lie in which box: the peaks sorted by column once, then per box a binary search for its columns
    and a test of the rows of those few.  Every source gets keys = (count key, snr key): the number of peaks whose pixel lies in its
    box and the largest snr among them (None without one).  -> per peak the index of the first such source, -1 without one."""
    nkey, skey = keys
    boxes, n = boxes_of(sources), kept.shape[0]
    xp, yp, snr = kept[:, PEAK.x], kept[:, PEAK.y], kept[:, PEAK.snr]
    by_x = np.argsort(xp, kind="stable")
    xs = xp[by_x]
    first, count = np.full(n, -1, np.int64), np.zeros(len(sources), np.int64)
    best = np.full(len(sources), -np.inf, np.float64)
    for i, (x1, y1, x2, y2) in enumerate(boxes):
        idx = by_x[np.searchsorted(xs, x1, "left"):np.searchsorted(xs, x2, "right")]
        idx = idx[(y1 <= yp[idx]) & (yp[idx] <= y2)]
        if idx.size:
            count[i], best[i] = idx.size, snr[idx].max()
            first[idx[first[idx] < 0]] = i                    # boxes come in source order: the first one stays
    for s, c, m in zip(sources, count, best):
        if nkey is not None:
            s[nkey] = int(c)
        if skey is not None:
            s[skey] = float(m) if c else None
    return first


def _peak_entry(keys, r, f, sign, ba, wcs, ox, oy):
    """The dict (its first keys PEAK_KEYS) of one raw peak row r whose first containing source is f (-1: none)."""
    xp_, yp_, sw = int(r[PEAK.x]), int(r[PEAK.y]), float(r[PEAK.sw])
    d = dict.fromkeys(keys)
    d["x_peak"], d["y_peak"] = xp_, yp_
    d["x"], d["y"] = xp_ + float(r[PEAK.swx]) / sw, yp_ + float(r[PEAK.swy]) / sw
    d["ra"], d["dec"] = _sky(wcs, d["x"], d["y"], ox, oy)
    d["peak"], d["rms"], d["snr"] = float(r[PEAK.v]), float(r[PEAK.rms]), float(r[PEAK.snr])
    d["npix"], d["nabove"] = int(r[PEAK.npix]), int(r[PEAK.nabove])
    d["flux_sum"] = sign * float(r[PEAK.sum])
    if ba > 0.0:
        d["flux"] = d["flux_sum"] / ba
    d["in_source"] = int(f) if f >= 0 else None
    return d


# ---- residual scales (--residual_scales)
def annotate_scale_peaks(sources, levels, min_above, beam_area, wcs, origin=(0, 0)):
    """The peak list of the wavelet planes of a residual map, and the scale keys of every source.  levels: per searched scale
    (scale, step, rows, total), rows [n, CY_PEAK_FIELDS] of cy_find_peaks on that plane with x, y in catalog coordinates.  A row is
    kept when nabove >= min_above.  -> a list of dicts (SCALE_PEAK_KEYS) merged over the scales in decreasing snr, equal snr in
    (scale, y_peak, x_peak) order: PEAK_KEYS as annotate_peaks gives them (peak, rms, flux_sum are of the wavelet plane), then
      scale, step    the plane j and its tap distance 2^(j - 1)
      strongest      False exactly when another kept entry f outranks this entry e (it comes before e in the order above) and lies
                     within 2 max(step_e, step_f) of it in both |dx| and |dy| of the peak pixels; f may be of any scale, e's own
                     included, and need not be strongest itself
    Every source dict gets SOURCE_SCALE_KEYS: the number of kept entries (of all scales) whose peak pixel lies in its box and the
    largest snr among them, None without one."""
    ox, oy = float(origin[0]), float(origin[1])
    ba = float(beam_area) if beam_area else 0.0
    parts, scale, step = [], [], []
    for j, st, rows, total in levels:
        rows = np.asarray(rows, np.float64).reshape(-1, L.CY_PEAK_FIELDS)
        assert int(total) >= rows.shape[0]
        rows = rows[rows[:, PEAK.nabove] >= float(min_above)]
        parts.append(rows)
        scale.append(np.full(rows.shape[0], int(j), np.int64))
        step.append(np.full(rows.shape[0], int(st), np.int64))
    kept = np.concatenate(parts) if parts else np.zeros((0, L.CY_PEAK_FIELDS), np.float64)
    scale = np.concatenate(scale) if scale else np.zeros(0, np.int64)
    step = np.concatenate(step) if step else np.zeros(0, np.int64)
    order = np.lexsort((kept[:, PEAK.x], kept[:, PEAK.y], scale, -kept[:, PEAK.snr]))
    kept, scale, step = kept[order], scale[order], step[order]
    first = _peaks_in_boxes(sources, kept, SOURCE_SCALE_KEYS)
    # strongest: per step value the entries of that step sorted by column; for an entry e and a step S the columns within
    # 2 max(step_e, S) by binary search, then the rows and the rank (the position in `kept`) of those few
    n = kept.shape[0]
    xp, yp = kept[:, PEAK.x], kept[:, PEAK.y]
    strongest = np.ones(n, bool)
    by_step = []
    for S in np.unique(step):
        idx = np.nonzero(step == S)[0]
        idx = idx[np.argsort(xp[idx], kind="stable")]
        by_step.append((int(S), idx, xp[idx]))
    for S, idx, xs in by_step:
        d = 2.0 * np.maximum(step, S).astype(np.float64)
        lo, hi = np.searchsorted(xs, xp - d, "left"), np.searchsorted(xs, xp + d, "right")
        ends = np.cumsum(hi - lo)
        e0 = 0
        while e0 < n:                                         # entries e0 .. e1 - 1 against their column ranges, at most about 2^22 pairs at a time
            e1 = max(int(np.searchsorted(ends, (ends[e0 - 1] if e0 else 0) + (1 << 22), "right")), e0 + 1)
            cnt = (hi - lo)[e0:e1]
            e = np.repeat(np.arange(e0, e1), cnt)
            f = idx[np.repeat(lo[e0:e1], cnt) + (np.arange(e.size) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
            hit = (f < e) & (np.abs(yp[f] - yp[e]) <= d[e])
            strongest[e[hit]] = False
            e0 = e1
    out = []
    for r, f, j, st, top in zip(kept, first, scale, step, strongest):
        d = _peak_entry(SCALE_PEAK_KEYS, r, f, 1.0, ba, wcs, ox, oy)
        d["scale"], d["step"], d["strongest"] = int(j), int(st), bool(top)
        out.append(d)
    return out


def scales_config(config):
    """(J, first, k_sigma) of --residual_scales from a config dictionary: the number of scales (0: no search), the first scale that
    is searched and the threshold in units of the plane's rms map."""
    return int(config.get('residual_scales', 0) or 0), int(config.get('residual_scale_first', 2)), float(config.get('residual_scales_sigma', 5.0))


def wants_scales(config):
    """Whether a config asks for the multi-scale search of the residual map (residual_scales > 0)."""
    return scales_config(config)[0] > 0


def scale_cell(bkg_cell, step):
    """Cell of the noise mesh of the wavelet plane with tap distance `step`: the noise of a coarse plane is correlated over about
    4 step pixels, and a cell has to hold many such patches."""
    return min(4096, max(int(bkg_cell), 16 * int(step)))


def scale_radius(peaks_radius, step):
    """Neighbourhood radius of the peak search on the wavelet plane with tap distance `step` (cy_find_peaks takes at most 8)."""
    return min(L.CY_PEAK_RADIUS_MAX, max(int(peaks_radius), int(step)))


# ---- peak apertures (--peak_apertures)
def aperture_config(config):
    """(unit, factors, annulus) of --peak_apertures from a config dictionary: the pixel size of one radius unit at step 1, the
    aperture radii in that unit (a tuple; `aperture_radii` is a comma-separated string or a sequence) and the outer edge of the
    background annulus.  ValueError for a unit or an annulus that is not finite and positive, for an empty list, more than
    CY_APER_RINGS_MAX - 1 radii, radii that are not finite, positive and strictly increasing, or an annulus that is not greater
    than the last radius."""
    unit, annulus = float(config.get('aperture_unit', 1.0)), float(config.get('aperture_annulus', 6.0))
    radii = config.get('aperture_radii', "1,2,3,4")
    if isinstance(radii, str):
        parts = [t.strip() for t in radii.split(",")]
        if not all(parts):
            raise ValueError("aperture_radii: an empty entry in %r" % radii)
        radii = parts
    try:
        factors = tuple(float(t) for t in radii)
    except (TypeError, ValueError):
        raise ValueError("aperture_radii: not a list of numbers: %r" % (radii,))
    if not 1 <= len(factors) <= L.CY_APER_RINGS_MAX - 1:
        raise ValueError("aperture_radii: 1 to %d radii required" % (L.CY_APER_RINGS_MAX - 1))
    if not all(math.isfinite(f) and f > 0.0 for f in factors) or any(b <= a for a, b in zip(factors, factors[1:])):
        raise ValueError("aperture_radii: the radii must be finite, positive and strictly increasing")
    if not (math.isfinite(unit) and unit > 0.0):
        raise ValueError("aperture_unit must be finite and > 0")
    if not (math.isfinite(annulus) and annulus > factors[-1]):
        raise ValueError("aperture_annulus must be finite and greater than the last radius")
    return unit, factors, annulus


def wants_apertures(config):
    """Whether a config asks for apertures on the entries of its peak lists (peak_apertures)."""
    return bool(config.get('peak_apertures', False))


def annotate_apertures(entries, rows, nap, beam_area, radii=None):
    """APERTURE_KEYS on every dict of `entries` from rows [n, CY_APER_FIELDS] of cy_aperture_sums, entry i from row i, whose first
    `nap` rings are the apertures and whose ring nap + 1 is the background annulus.  radii: [n, nap] the radii in pixels (None:
    ap_radius stays None).  With m = 0 .. nap - 1 and cum(x)[m] = x_1 + .. + x_(m+1) over the rings, a plain sequential float64
    sum in increasing ring:
      ap_status, ap_clipped   as in the row (ints)
      ap_radius               the radii in pixels
      ap_npix, ap_sum         cum(npix) (ints), cum(sum)
      ap_bkg, ap_bkg_rms      bkg_med; MAD_TO_SIGMA * bkg_mad;  ap_nbkg  npix of ring nap + 1
      ap_flux_sum             ap_sum[m] - ap_npix[m] * ap_bkg
      ap_flux                 ap_flux_sum[m] / beam_area; None (not a list) unless beam_area > 0
      ap_flux_err             sqrt(cum(svar)[m] / beam_area), likewise: the noise is correlated over one beam, so the variance of
                              the sum over an aperture is beam_area * sum(rms^2) and the error of sum / beam_area the root of
                              sum(rms^2) / beam_area.  The error of the background is not in it
      ap_snr                  ap_flux[m] / ap_flux_err[m] where the error is > 0, else None; None (not a list) without a beam
      ap_best                 the index of the largest ap_snr, the first of equal ones; None without one
    For a status other than 0 the lists and ap_best are None.  -> entries."""
    rows = np.asarray(rows, np.float64).reshape(-1, L.CY_APER_FIELDS)
    assert rows.shape[0] == len(entries) and 1 <= nap < L.CY_APER_RINGS_MAX
    ba = float(beam_area) if beam_area else 0.0
    H, F = L.CY_APER_HEAD, L.CY_APER_RING_FIELDS
    for i, (d, r) in enumerate(zip(entries, rows)):
        d.update(dict.fromkeys(APERTURE_KEYS))
        d["ap_status"], d["ap_clipped"] = int(r[APER.status]), int(r[APER.clipped])
        d["ap_bkg"], d["ap_bkg_rms"] = float(r[APER.bkg_med]), MAD_TO_SIGMA * float(r[APER.bkg_mad])
        d["ap_nbkg"] = int(r[H + F * nap + APER_RING.npix])
        if d["ap_status"] != 0:
            continue
        npix, tot, var = [], [], []
        n, s, v = 0, 0.0, 0.0
        for k in range(nap):
            n += int(r[H + F * k + APER_RING.npix])
            s = s + float(r[H + F * k + APER_RING.sum])
            v = v + float(r[H + F * k + APER_RING.svar])
            npix.append(n); tot.append(s); var.append(v)
        d["ap_radius"] = [float(x) for x in radii[i]] if radii is not None else None
        d["ap_npix"], d["ap_sum"] = npix, tot
        d["ap_flux_sum"] = [s - n * d["ap_bkg"] for s, n in zip(tot, npix)]
        if ba > 0.0:
            d["ap_flux"] = [f / ba for f in d["ap_flux_sum"]]
            d["ap_flux_err"] = [math.sqrt(v / ba) for v in var]
            d["ap_snr"] = [f / e if e > 0.0 else None for f, e in zip(d["ap_flux"], d["ap_flux_err"])]
            best = None
            for m, q in enumerate(d["ap_snr"]):
                if q is not None and (best is None or q > d["ap_snr"][best]):
                    best = m
            d["ap_best"] = best
    return entries


# ---- peak fits (--fit_peaks)
def peakfit_config(config):
    """(radius, sigma0, max_iter) of --fit_peaks from a config dictionary: the radius of the fitted disc and the sigma of the
    circular start, both in pixels at step 1, and the iteration limit.  ValueError for a radius or a sigma that is not finite and
    positive, or a max_iter outside 1 .. 256."""
    radius, sigma0 = float(config.get('fit_peaks_radius', 6.0)), float(config.get('fit_peaks_sigma', 1.5))
    max_iter = config.get('fit_peaks_max_iter', 64)
    if not (math.isfinite(radius) and radius > 0.0):
        raise ValueError("fit_peaks_radius must be finite and > 0")
    if not (math.isfinite(sigma0) and sigma0 > 0.0):
        raise ValueError("fit_peaks_sigma must be finite and > 0")
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or not 1 <= int(max_iter) <= 256:
        raise ValueError("fit_peaks_max_iter must be an integer in [1, 256]")
    return radius, sigma0, int(max_iter)


def wants_peak_fits(config):
    """Whether a config asks for a Gaussian fit of the entries of its peak lists (fit_peaks)."""
    return bool(config.get('fit_peaks', False))


def peak_fit_jobs(entries, sign, radius, sigma0, at_peak, origin=(0, 0)):
    """[n, CY_PFIT_JOB_FIELDS] float64 (lib.PFIT_JOB_NAMES), one job of cy_fit_peaks per entry of a peak list, in the pixel frame
    (catalog coordinates - origin).  at_peak: [n] the map's value at every entry's peak pixel.
      centre   the entry's x, y;  R = radius * step (step 1 for the entries of the pixel searches)
      bkg      the entry's ap_bkg when the apertures ran and it is not None, else 0.0;  sign as given (-1 for holes)
      start    A = sign * (at_peak - bkg), |entry["peak"]| when that is not > 0;  x0, y0 the centre;  a = c = 1 / (sigma0 * step)^2,
               b = 0"""
    bx, by = float(origin[0]), float(origin[1])
    n = len(entries)
    jobs = np.zeros((n, L.CY_PFIT_JOB_FIELDS), np.float64)
    at_peak = np.asarray(at_peak, np.float64).reshape(n)
    for i, d in enumerate(entries):
        step = float(d.get("step", 1))
        bkg = d.get("ap_bkg")
        bkg = float(bkg) if bkg is not None else 0.0
        A = float(sign) * (float(at_peak[i]) - bkg)
        if not A > 0.0:
            A = abs(float(d["peak"]))
        a = 1.0 / ((float(sigma0) * step) * (float(sigma0) * step))
        cx, cy = float(d["x"]) - bx, float(d["y"]) - by
        jobs[i] = [cx, cy, float(radius) * step, bkg, float(sign), A, cx, cy, a, 0.0, a]
    return jobs


def annotate_peak_fits(entries, rows, jobs, rms, sign, beam_area, wcs, origin=(0, 0), select=None):
    """GFIT_KEYS on every dict of `entries`.  rows: [m, CY_PFIT_FIELDS] rows of cy_fit_peaks with x0, y0 in catalog coordinates,
    jobs: [m, CY_PFIT_JOB_FIELDS] what was asked for, rms: [m] the noise at the peak pixels; row t belongs to entries[select[t]]
    (select None: entry t).  An entry without a row (a scale peak that is not the strongest of its place) gets every key None.
      gfit_status, gfit_niter, gfit_npix, gfit_nexcluded, gfit_nneigh, gfit_crowded, gfit_clipped   as in the row (ints)
      gfit_radius, gfit_bkg    R and bkg of the job
      gfit_chi2 .. gfit_flux_err   as the fit_ keys of annotate_fits() (_gaussian_keys) with that rms; gfit_peak and gfit_flux carry
                               the sign: negative for a hole
    With status 1, 3, 4 or 5 the keys from gfit_chi2 on are None.  -> entries."""
    rows = np.asarray(rows, np.float64).reshape(-1, L.CY_PFIT_FIELDS)
    jobs = np.asarray(jobs, np.float64).reshape(-1, L.CY_PFIT_JOB_FIELDS)
    rms = np.asarray(rms, np.float64).reshape(-1)
    select = list(range(len(entries))) if select is None else [int(i) for i in select]
    assert rows.shape[0] == jobs.shape[0] == rms.shape[0] == len(select)
    ox, oy = float(origin[0]), float(origin[1])
    ba = float(beam_area) if beam_area else 0.0
    for d in entries:
        d.update(dict.fromkeys(GFIT_KEYS))
    for i, r, job, noise in zip(select, rows, jobs, rms):
        d = entries[i]
        st = int(r[PFIT.status])
        d["gfit_status"], d["gfit_niter"], d["gfit_npix"], d["gfit_nexcluded"] = st, int(r[PFIT.niter]), int(r[PFIT.npix]), int(r[PFIT.nexcluded])
        d["gfit_nneigh"], d["gfit_crowded"], d["gfit_clipped"] = int(r[PFIT.nneigh]), int(r[PFIT.crowded]), int(r[PFIT.clipped])
        d["gfit_radius"], d["gfit_bkg"] = float(job[PFIT_JOB.R]), float(job[PFIT_JOB.bkg])
        if st in (0, 2):
            noise = float(noise) if math.isfinite(noise) and noise > 0.0 else 0.0
            _gaussian_keys(d, "gfit_", r, PFIT.F, _PFIT_PARAMS, fit_covariance, noise, ba, wcs, ox, oy)
            if sign < 0:
                d["gfit_peak"] = -d["gfit_peak"]
                if d["gfit_flux"] is not None:
                    d["gfit_flux"] = -d["gfit_flux"]
    return entries


def peak_fit_stats(rows):
    """(jobs, converged, mean niter, largest niter, crowded) over rows [n, CY_PFIT_FIELDS] of cy_fit_peaks; the iterations over the
    fitted rows (status 0 or 2)."""
    rows = np.asarray(rows, np.float64).reshape(-1, L.CY_PFIT_FIELDS)
    it = rows[np.isin(rows[:, PFIT.status], _FITTED), PFIT.niter]
    return (int(rows.shape[0]), int((rows[:, PFIT.status] == 0.0).sum()), float(it.mean()) if it.size else 0.0, int(it.max()) if it.size else 0,
            int((rows[:, PFIT.crowded] == 1.0).sum()))


# ---- joint fits of neighbouring peaks (--fit_peak_groups)
def peakgroup_config(config):
    """link of --fit_peak_groups from a config dictionary (fit_peaks_link, default 1.5): two entries of a list are fitted together
    when their centres are closer than link times the larger of their disc radii.  The default rests on the bias of the single
    fits measured on clean pairs (R = 6, sigma 1.6): 0.85 px at 4 px apart, 0.31 px at 5, 0.04 px at 7, negligible at 9; with R = 6
    it links entries closer than 9 px.  ValueError outside (0, 2]."""
    link = float(config.get('fit_peaks_link', 1.5))
    if not (math.isfinite(link) and 0.0 < link <= 2.0):
        raise ValueError("fit_peaks_link must be in (0, 2]")
    return link


def wants_peak_groups(config):
    """Whether a config asks for the joint fit of neighbouring entries of its peak lists (fit_peak_groups)."""
    return bool(config.get('fit_peak_groups', False))


def peak_group_jobs(jobs, rows):
    """The jobs of cy_fit_peak_groups for one list: those of cy_fit_peaks (jobs, [n, CY_PFIT_JOB_FIELDS]) with the start of every job
    whose cy_fit_peaks row (rows, [n, CY_PFIT_FIELDS]) has status 0 or 2 replaced by that row's parameters.  Both in the same pixel
    frame, as blend_start() does for components."""
    jobs = np.array(jobs, np.float64).reshape(-1, L.CY_PFIT_JOB_FIELDS)
    rows = np.asarray(rows, np.float64).reshape(-1, L.CY_PFIT_FIELDS)
    use = np.isin(rows[:, PFIT.status], _FITTED)
    jobs[np.ix_(use, _PFIT_JOB_PARAMS)] = rows[np.ix_(use, _PFIT_PARAMS)]
    return jobs


def annotate_peak_groups(entries, rows, rms, sign, beam_area, wcs, origin=(0, 0), select=None):
    """GBLEND_KEYS on every dict of `entries`, after annotate_peak_fits().  rows: [m, CY_PGRP_FIELDS] rows of cy_fit_peak_groups with
    x0, y0 in catalog coordinates, rms: [m] the noise at the peak pixels; row t belongs to entries[select[t]] (select None: entry
    t).  An entry without a row (a scale peak that is not the strongest of its place) gets every key None.
      gblend_group   the index in `entries` of the group's first member (the entry's own when it is alone); gblend_size, gblend_slot,
                     gblend_status, gblend_niter, gblend_npix, gblend_nexcluded   as in the row (ints); group, size and slot are None
                     with status 1 or 5, which have no group
      gblend_chi2 .. gblend_flux_err   as their gfit_ namesakes, from the member's parameters of the joint fit (_gaussian_keys), the
                     errors from rms^2 times the member's block of C (blend_covariance); gblend_peak and gblend_flux carry the sign
    Status 6 (the entry is alone): the keys from gblend_chi2 on repeat the entry's gfit_ values.  Status 1, 3, 4, 5 or 7: they are
    None.  -> entries."""
    rows = np.asarray(rows, np.float64).reshape(-1, L.CY_PGRP_FIELDS)
    rms = np.asarray(rms, np.float64).reshape(-1)
    select = list(range(len(entries))) if select is None else [int(i) for i in select]
    assert rows.shape[0] == rms.shape[0] == len(select)
    ox, oy = float(origin[0]), float(origin[1])
    ba = float(beam_area) if beam_area else 0.0
    values = GBLEND_KEYS[GBLEND_KEYS.index("gblend_chi2"):]
    for d in entries:
        d.update(dict.fromkeys(GBLEND_KEYS))
    for i, r, noise in zip(select, rows, rms):
        d = entries[i]
        st = int(r[PGRP.status])
        d["gblend_status"], d["gblend_niter"], d["gblend_npix"], d["gblend_nexcluded"] = st, int(r[PGRP.niter]), int(r[PGRP.npix]), int(r[PGRP.nexcluded])
        if st not in (1, 5):
            d["gblend_group"], d["gblend_size"], d["gblend_slot"] = select[int(r[PGRP.group])], int(r[PGRP.nmembers]), int(r[PGRP.slot])
        if st == 6:
            for k in values:
                d[k] = d.get("gfit_" + k[len("gblend_"):])
        elif st in (0, 2):
            noise = float(noise) if math.isfinite(noise) and noise > 0.0 else 0.0
            _gaussian_keys(d, "gblend_", r, PGRP.F, _BLEND_PARAMS, blend_covariance, noise, ba, wcs, ox, oy)
            if sign < 0:
                d["gblend_peak"] = -d["gblend_peak"]
                if d["gblend_flux"] is not None:
                    d["gblend_flux"] = -d["gblend_flux"]
    return entries


def peak_group_stats(rows):
    """(jobs, members, converged, mean niter, largest niter, groups above CY_BLEND_MAX_MEMBERS) over rows [n, CY_PGRP_FIELDS] of
    cy_fit_peak_groups: a group job (status 0, 2, 3 or 4) is counted once, on its slot-0 row, as is a group above the limit (status
    7); members: the rows of the group jobs; the iterations over the fitted jobs (status 0 or 2)."""
    rows = np.asarray(rows, np.float64).reshape(-1, L.CY_PGRP_FIELDS)
    job = np.isin(rows[:, PGRP.status], (0.0, 2.0, 3.0, 4.0))
    first = rows[:, PGRP.slot] == 0.0
    it = rows[first & np.isin(rows[:, PGRP.status], _FITTED), PGRP.niter]
    return (int((job & first).sum()), int(job.sum()), int((first & (rows[:, PGRP.status] == 0.0)).sum()), float(it.mean()) if it.size else 0.0,
            int(it.max()) if it.size else 0, int((first & (rows[:, PGRP.status] == 7.0)).sum()))


# ---- the second residual (--subtract_peaks)
def wants_subtract(config):
    """Whether a config asks for the second residual: the fitted peaks subtracted from the residual map (subtract_peaks)."""
    return bool(config.get('subtract_peaks', False))


def peak_render_selection(chain):
    """The Gaussians the second residual subtracts, after Chain.peak_fits() (and Chain.peak_groups() when it ran): the fitted
    entries of the lists in the order residual_peaks, residual_holes, residual_scale_peaks (PEAK_LIST_NAMES), inside a list in the
    order of its jobs.  Everything in the pixel frame of chain.img, as the library answered (.peakfit_rows, .peakgroup_rows,
    .peakfit_jobs).  Per fitted entry, tested in this order:
      parameters   its cy_fit_peak_groups row's when the groups ran and that row's status is 0 or 2, else its cy_fit_peaks row's when
                   that status is 0 or 2, else the entry is not selected (the rule of _fitted_params; a status 6 row carries no
                   parameters of its own, so the single fit is used)
      wandered     left out when the fitted centre lies farther than the job's R from the job's centre: dx * dx + dy * dy > R * R
      duplicates   a scale entry is left out when a component already selected from the two pixel lists has its centre within
                   that scale entry's R of its job centre (dx * dx + dy * dy <= R * R): the same emission is subtracted once
      sign         A is multiplied by the list's sign: holes are rendered negative (cy_render_signed_gaussians admits them)
    -> (comp float64 [m, 6] {A, x0, y0, a, b, c}, index: m tuples (list name, entry index), counts {"wandered", "duplicates",
    "sources": per component "group" or "single", the fit its parameters came from})."""
    comp, index, counts = [], [], {"wandered": 0, "duplicates": 0, "sources": []}
    pixel_centres, by_x = [], None                            # the selected centres of the two pixel lists; sorted by column for the scale list
    fits, groups = chain.peakfit_rows or {}, chain.peakgroup_rows or {}
    for name in PEAK_LIST_NAMES:
        if name not in fits:
            continue
        sign = -1.0 if name == "residual_holes" else 1.0
        single = np.asarray(fits[name], np.float64).reshape(-1, L.CY_PFIT_FIELDS)
        joint = np.asarray(groups[name], np.float64).reshape(-1, L.CY_PGRP_FIELDS) if name in groups else None
        jobs = np.asarray(chain.peakfit_jobs[name], np.float64).reshape(-1, L.CY_PFIT_JOB_FIELDS)
        for t, i in enumerate(chain.peakfit_select[name]):
            if joint is not None and joint[t, PGRP.status] in _FITTED:
                p, source = joint[t, _BLEND_PARAMS].copy(), "group"
            elif single[t, PFIT.status] in _FITTED:
                p, source = single[t, _PFIT_PARAMS].copy(), "single"
            else:
                continue
            cx, cy, R = (float(jobs[t, k]) for k in (PFIT_JOB.cx, PFIT_JOB.cy, PFIT_JOB.R))
            dx, dy = float(p[1]) - cx, float(p[2]) - cy
            if not dx * dx + dy * dy <= R * R:
                counts["wandered"] += 1
                continue
            if name == "residual_scale_peaks":
                if by_x is None:
                    by_x = np.array(sorted(pixel_centres), np.float64).reshape(-1, 2)
                # the stretch of columns within R (one more on either side: the test below decides, this only narrows it)
                near = by_x[np.searchsorted(by_x[:, 0], cx - R - 1.0, "left"):np.searchsorted(by_x[:, 0], cx + R + 1.0, "right")]
                qx, qy = near[:, 0] - cx, near[:, 1] - cy
                if (qx * qx + qy * qy <= R * R).any():
                    counts["duplicates"] += 1
                    continue
            else:
                pixel_centres.append((float(p[1]), float(p[2])))
            p[0] *= sign
            comp.append(p)
            index.append((name, int(i)))
            counts["sources"].append(source)
    return np.array(comp, np.float64).reshape(-1, 6), index, counts


def annotate_peak_residuals(entries, rows, rms, picked, beam_area, origin=(0, 0), select=None):
    """GRES_KEYS on every dict of `entries`, after annotate_peak_fits().  rows: [m, CY_DRES_FIELDS] rows of cy_disc_residuals on the
    second residual, in the pixels of the measured image; rms: [m] the noise at the peak pixels; row t belongs to
    entries[select[t]] (select None: entry t).  picked: {entry index: (source, render status)} for the entries
    peak_render_selection() chose, with the status of their cy_render_gaussians rows.  An entry without a row (one that was never
    fitted) gets every key None.
      gres_subtracted      whether the entry's Gaussian is part of the peak model (chosen, and render status 0 or 2)
      gres_source          "group" or "single": the fit it was rendered from; None when it was not chosen
      gres_render_status   the status of its render row (0, 2: rendered; 1, 3: skipped by the library); None when it was not chosen
      gres_npix            valid pixels of the entry's share of its disc: the pixels its single fit used (0 with status 1 or 5)
      gres_mean = sum / npix, gres_rms = sqrt(sumsq / npix) of r = v - bkg on the second residual over those pixels
      gres_max             the largest |r|; gres_x_max, gres_y_max its position (+ origin)
      gres_ratio = gres_rms / rms, gres_chi2 = sumsq / rms^2; None when that rms is not finite and > 0
      gres_model_flux = model_sum / beam_area, what the peak model holds on those pixels; None without a beam
    With npix == 0 the keys from gres_mean on are None.  -> entries."""
    rows = np.asarray(rows, np.float64).reshape(-1, L.CY_DRES_FIELDS)
    rms = np.asarray(rms, np.float64).reshape(-1)
    select = list(range(len(entries))) if select is None else [int(i) for i in select]
    assert rows.shape[0] == rms.shape[0] == len(select)
    ox, oy = int(origin[0]), int(origin[1])
    ba = float(beam_area) if beam_area else 0.0
    for d in entries:
        d.update(dict.fromkeys(GRES_KEYS))
    for i, r, noise in zip(select, rows, rms):
        d = entries[i]
        source, st = picked.get(i, (None, None))
        d["gres_subtracted"], d["gres_source"], d["gres_render_status"] = st in (0, 2), source, st
        npix = int(r[DRES.npix]) if r[DRES.status] == 0.0 else 0
        d["gres_npix"] = npix
        if npix == 0:
            continue
        sumsq = float(r[DRES.sumsq])
        d["gres_mean"], d["gres_rms"] = float(r[DRES.sum]) / npix, math.sqrt(sumsq / npix)
        d["gres_max"], d["gres_x_max"], d["gres_y_max"] = float(r[DRES.maxabs]), int(r[DRES.x_max]) + ox, int(r[DRES.y_max]) + oy
        noise = float(noise)
        if math.isfinite(noise) and noise > 0.0:
            d["gres_ratio"], d["gres_chi2"] = d["gres_rms"] / noise, sumsq / (noise * noise)
        if ba > 0.0:
            d["gres_model_flux"] = float(r[DRES.model_sum]) / ba
    return entries


def _read_at(m, iy, ix):
    """m[iy, ix] of a device map (or a host array) as numpy float64: one indexed read."""
    if hasattr(m, "is_cuda"):
        import torch
        return m[torch.as_tensor(iy, device=m.device), torch.as_tensor(ix, device=m.device)].cpu().numpy().astype(np.float64)
    return np.asarray(m)[iy, ix].astype(np.float64)


def peaks_config(config):
    """(k_sigma, radius, min_above, cap) of --residual_peaks from a config dictionary."""
    return (float(config.get('residual_peaks_sigma', 5.0)), int(config.get('residual_peaks_radius', 2)),
            int(config.get('residual_peaks_min_above', 3)), int(config.get('residual_peaks_max', 65536)))


def wants_peaks(config):
    """Whether a config asks for the search of the residual map (residual_peaks or residual_holes)."""
    return bool(config.get('residual_peaks', False) or config.get('residual_holes', False))


def peak_lists(chain):
    """What a catalog file carries beside its sources after Chain.run(): {"residual_peaks": [...]} and, when holes were searched,
    "residual_holes", and "residual_scale_peaks" when the scales were, and "residual_peaks_left" / "residual_holes_left" when the
    fitted peaks were subtracted, and "forced_images" (tag, path, freq, beam_area, mesh_ndef per measured map) after the forced
    fits; empty when the chain (or None) did none of these."""
    out = {}
    if chain is not None and chain.peak_list is not None:
        out["residual_peaks"] = chain.peak_list
    if chain is not None and chain.hole_list is not None:
        out["residual_holes"] = chain.hole_list
    if chain is not None and chain.scale_list is not None:
        out["residual_scale_peaks"] = chain.scale_list
    if chain is not None and chain.left_peak_list is not None:
        out["residual_peaks_left"], out["residual_holes_left"] = chain.left_peak_list, chain.left_hole_list
    if chain is not None and chain.forced_images is not None:
        out["forced_images"] = chain.forced_images
    return out


def _save_maps(tags, maps, catalog_path):
    """Two device maps written as fp32 FITS images <tag><name>.fits beside the catalog file, <name> = the catalog's file name
    without its extension.  -> the two paths."""
    from . import utils
    d, name = os.path.split(catalog_path)
    name = os.path.splitext(name)[0]
    paths = tuple(os.path.join(d, tag + name + ".fits") for tag in tags)
    for path, m in zip(paths, maps):
        utils.write_fits_image(path, m.cpu().numpy())
    return paths


def save_scale_maps(planes, catalog_path):
    """--save_scale_maps: wav<j>_<name>.fits beside the catalog file for every searched plane {j: device map} (_save_maps).  -> the paths."""
    scales = sorted(planes)
    return _save_maps(tuple("wav%d_" % j for j in scales), tuple(planes[j] for j in scales), catalog_path)


def save_residual_maps(model, resid, catalog_path):
    """--save_residual_maps: model_<name>.fits / resid_<name>.fits beside the catalog file (_save_maps).  -> the two paths."""
    return _save_maps(("model_", "resid_"), (model, resid), catalog_path)


def save_second_residual_maps(peak_model, resid2, catalog_path):
    """--save_residual_maps with --subtract_peaks: peakmodel_<name>.fits / resid2_<name>.fits beside the catalog file (_save_maps).
    -> the two paths."""
    return _save_maps(("peakmodel_", "resid2_"), (peak_model, resid2), catalog_path)


def deblend_config(config):
    """(k_peak, radius) of --deblend_islands from a config dictionary; the peak threshold defaults to the island seed threshold."""
    k = config.get('deblend_peak_sigma')
    return (float(config.get('island_seed_sigma', 5.0)) if k is None else float(k)), int(config.get('deblend_radius', 2))


# ---- background and noise mesh (--bkg_map)
def fill_mesh(raw, min_pix=64):
    """raw: [ncy, ncx, CY_BKG_FIELDS] rows of cy_measure_background.  -> (mesh [ncy, ncx, 2] float64 {bkg, rms}, number of defined
    cells).  A cell is defined when n >= min_pix; an undefined cell takes bkg and rms of the defined cell with the smallest squared
    index distance dcy^2 + dcx^2, ties to the smallest row-major index.  No defined cell: the mesh is 0 and the count 0."""
    raw = np.asarray(raw, np.float64)
    ncy, ncx = raw.shape[:2]
    mesh = np.zeros((ncy, ncx, 2), np.float64)
    ok = raw[:, :, BKG.n] >= float(min_pix)
    dy, dx = np.nonzero(ok)                                  # row-major order: the first minimum is the smallest index
    if dy.size == 0:
        return mesh, 0
    mesh[ok] = raw[:, :, [BKG.bkg, BKG.rms]][ok]
    uy, ux = np.nonzero(~ok)
    for i in range(0, uy.size, 256):
        d = (uy[i:i + 256, None] - dy[None, :]) ** 2 + (ux[i:i + 256, None] - dx[None, :]) ** 2
        j = np.argmin(d, 1)
        mesh[uy[i:i + 256], ux[i:i + 256]] = mesh[dy[j], dx[j]]
    return mesh, int(dy.size)


def _mesh_coord(p, cell, nc):
    p = np.asarray(p, np.float64)
    if nc == 1:
        return np.zeros(p.shape, np.int64), np.zeros(p.shape, np.float64)
    t = (p - (cell - 1) / 2.0) / float(cell)
    t = np.where(t < 0.0, 0.0, t)
    t = np.where(t > float(nc - 1), float(nc - 1), t)
    i0 = np.minimum(np.floor(t).astype(np.int64), nc - 2)
    return i0, t - i0


def sample_mesh(mesh, cell, x, y):
    """Bilinear interpolation of mesh [ncy, ncx] (or [ncy, ncx, C]: every plane) between the cell centres cx * cell + (cell - 1) / 2
    at the pixel positions x, y (scalars or arrays of one shape); constant outside the outermost centres.  float64, the
    expression and association of background_expand_kernel: (m00 (1 - fx) + m01 fx) (1 - fy) + (m10 (1 - fx) + m11 fx) fy."""
    mesh = np.asarray(mesh, np.float64)
    cell = int(cell)
    ncy, ncx = mesh.shape[:2]
    x0, fx = _mesh_coord(x, cell, ncx)
    y0, fy = _mesh_coord(y, cell, ncy)
    x1, y1 = np.minimum(x0 + 1, ncx - 1), np.minimum(y0 + 1, ncy - 1)
    if mesh.ndim == 3:
        fx, fy = fx[..., None], fy[..., None]
    gx, gy = 1.0 - fx, 1.0 - fy
    return (mesh[y0, x0] * gx + mesh[y0, x1] * fx) * gy + (mesh[y1, x0] * gx + mesh[y1, x1] * fx) * fy


def annotate_background(sources, mesh, cell, origin=(0, 0)):
    """Adds BKG_KEYS to every source dict (in place; returns the list), after annotate(): bkg_map, rms_map = sample_mesh at
    (x_peak, y_peak), at the centre of the box when npix == 0; snr_map = (peak - bkg_map) / rms_map, 0 when rms_map == 0.
    origin: catalog coordinates of pixel [0, 0] of the image the mesh was measured on."""
    if not sources:
        return sources
    ox, oy = float(origin[0]), float(origin[1])
    x = np.array([float(s["x_peak"]) if s["npix"] > 0 else (float(s["x1"]) + float(s["x2"])) / 2.0 for s in sources], np.float64) - ox
    y = np.array([float(s["y_peak"]) if s["npix"] > 0 else (float(s["y1"]) + float(s["y2"])) / 2.0 for s in sources], np.float64) - oy
    v = sample_mesh(np.asarray(mesh, np.float64)[:, :, :2], cell, x, y)
    for s, (b, r) in zip(sources, v):
        b, r = float(b), float(r)
        s["bkg_map"], s["rms_map"] = b, r
        s["snr_map"] = (float(s["peak"]) - b) / r if r != 0.0 else 0.0
    return sources


def save_background_maps(det, mesh, cell, shape, catalog_path):
    """--save_bkg_maps: the mesh expanded on the GPU (HipDetector.expand_background) and written as bkg_<name>.fits /
    rms_<name>.fits beside the catalog file (_save_maps).  -> the two paths."""
    return _save_maps(("bkg_", "rms_"), det.expand_background(mesh, cell, shape), catalog_path)


def background_config(config):
    """(cell, k, niter, min_pix) of --bkg_map from a config dictionary."""
    return (int(config.get('bkg_cell', 128)), float(config.get('bkg_clip_sigma', 3.0)), int(config.get('bkg_clip_iters', 3)),
            int(config.get('bkg_min_pix', 64)))


# ---- the chain of steps
STEPS = ("measure", "background", "islands", "deblend", "fit", "blend", "residual")


def plan(config):
    """The steps a config dictionary (or the parsed arguments of scripts/run.py as a dictionary) asks for, a tuple of names out of
    STEPS in the order they run.  Every later step implies the ones it builds on: save_residual_maps the residual step, residual
    and blend the fits, the fits the components, the components the islands, the islands the first measurement; bkg_map or
    save_bkg_maps the mesh, which implies the first measurement too.  residual_peaks and residual_holes (Chain.peaks, which is no
    step of STEPS) imply the residual step, whose map they search, and the mesh, whose rms map is their noise; residual_scales > 0
    (Chain.scale_peaks, no step either) implies exactly the same, and so do peak_apertures (Chain.apertures), fit_peaks
    (Chain.peak_fits), fit_peak_groups (Chain.peak_groups, which implies fit_peaks) and subtract_peaks (Chain.subtract, which
    implies fit_peaks too), which measure on the residual map with the rms map of the mesh but turn no search on.  forced_fit or
    forced_images (Chain.forced, no step either) imply the residual step like save_residual_maps, and nothing else."""
    on = {k for k in ("measure_sources", "bkg_map", "save_bkg_maps", "measure_islands", "deblend_islands", "fit_components", "fit_blends",
                      "residual_map", "save_residual_maps", "residual_peaks", "residual_holes") if config.get(k, False)}
    peaks = bool(on & {"residual_peaks", "residual_holes"}) or wants_scales(config) or wants_apertures(config) or wants_peak_fits(config) or wants_peak_groups(config) or wants_subtract(config)
    residual = peaks or bool(on & {"residual_map", "save_residual_maps"}) or wants_forced(config)
    fit = residual or bool(on & {"fit_components", "fit_blends"})
    deblend = fit or "deblend_islands" in on
    islands = deblend or "measure_islands" in on
    background = peaks or bool(on & {"bkg_map", "save_bkg_maps"})
    want = (islands or background or "measure_sources" in on, background, islands, deblend, fit, "fit_blends" in on, residual)
    return tuple(s for s, w in zip(STEPS, want) if w)


class Chain(object):
    """The measurement steps on one device image img_dev over the catalog dicts `sources`, which they annotate in place.  One
    method per step of STEPS; a step reads what the earlier ones left on the sources and on this object, so a caller that starts
    mid-chain (from a catalog that already carries bkg / rms, say) sets what it skipped and calls the later methods only.

    Three frames: the detector is given boxes and start values in the pixels of img_dev and answers in them (boxes, win0, raw,
    comp, masks, fit_pixel_rows, blend_pixel_rows, model, resid); the catalog's boxes and every position written into it are
    those pixels + box_origin, the catalog coordinates of pixel [0, 0] of img_dev (fit_rows, blend_rows); sky positions are taken
    at catalog coordinates + wcs_origin, the position of catalog coordinate (0, 0) in the frame of the WCS."""

    def __init__(self, det, img_dev, sources, config, beam_area=0, wcs=None, box_origin=(0, 0), wcs_origin=(0, 0), freq=None, forced_maps=None):
        c = config
        # --forced_fit: freq is the detection image's frequency; forced_maps the other maps, one dict each: tag, path, freq, beam_area
        # and upload, a callable (det) -> the map on the device, of img_dev's shape
        self.want_forced = wants_forced(c)
        self.forced_nsigma, self.forced_fit_bkg, _ = forced_config(c)
        self.freq, self.forced_maps, self.image_path = freq, list(forced_maps or []), c.get('image_path')
        self.render_comp = self.render_index = self.render_rows = None
        self.forced_rows = self.forced_job_rows = self.forced_images = self.forced_stats = self.forced_comp = self.forced_index = None
        self.det, self.img, self.sources, self.beam_area, self.wcs = det, img_dev, sources, beam_area, wcs
        self.box_origin, self.wcs_origin = box_origin, wcs_origin
        self.ring = int(c.get('measure_ring', 8))
        self.cell, self.clip_sigma, self.clip_iters, self.min_pix = background_config(c)
        self.k_seed, self.k_merge, self.conn = c.get('island_seed_sigma', 5.0), c.get('island_merge_sigma', 2.5), int(c.get('island_conn', 8))
        self.k_peak, self.radius = deblend_config(c)
        self.max_iter, self.nsigma = int(c.get('fit_max_iter', 64)), float(c.get('residual_nsigma', 5.0))
        self.save_bkg, self.save_residual = bool(c.get('save_bkg_maps', False)), bool(c.get('save_residual_maps', False))
        self.want_peaks, self.want_holes = wants_peaks(c), bool(c.get('residual_holes', False))
        self.peak_sigma, self.peak_radius, self.peak_min_above, self.peak_cap = peaks_config(c)
        self.nscales, self.scale_first, self.scale_sigma = scales_config(c)
        self.save_scales = bool(c.get('save_scale_maps', False))
        self.want_apertures = wants_apertures(c)
        self.ap_unit, self.ap_factors, self.ap_annulus = aperture_config(c) if self.want_apertures else (1.0, (), 0.0)
        self.want_peak_groups = wants_peak_groups(c)
        self.pg_link = peakgroup_config(c) if self.want_peak_groups else 1.5
        self.want_subtract = wants_subtract(c)
        self.want_peak_fits = wants_peak_fits(c) or self.want_peak_groups or self.want_subtract
        self.pf_radius, self.pf_sigma, self.pf_max_iter = peakfit_config(c) if self.want_peak_fits else (6.0, 1.5, 64)
        self.use_map = "background" in plan(c)               # thresholds, fit backgrounds and chi2 from bkg_map / rms_map
        self.bx, self.by = float(box_origin[0]), float(box_origin[1])
        self.MH, self.MW = int(img_dev.shape[0]), int(img_dev.shape[1])
        self.boxes = boxes_of(sources) - np.array([self.bx, self.by, self.bx, self.by], np.float64)
        self.win0 = np.array([box_window(b, self.MH, self.MW)[:2] for b in self.boxes], np.float64).reshape(-1, 2)
        self.mesh, self.ndef, self.keep_masks = None, None, True
        self.raw, self.masks = np.zeros((0, L.CY_DBL_FIELDS)), []
        self.comp = np.zeros((0, L.CY_DBL_MAX_COMP, L.CY_DBL_COMP_FIELDS))
        self.fit_rows = self.fit_pixel_rows = np.zeros((0, L.CY_DBL_MAX_COMP, L.CY_FIT_FIELDS), np.float64)
        self.blend_rows = self.blend_pixel_rows = None
        self.model = self.resid = self.render_stats = None
        self.peak_list = self.hole_list = self.peak_stats = None
        self.scale_list = self.scale_stats = self.scale_levels = self.scale_planes = self.scale_rows = None
        self.aperture_rows = self.aperture_stats = None
        self.peakfit_rows = self.peakfit_jobs = self.peakfit_select = self.peakfit_stats = self.peakfit_rms = None
        self.peakgroup_rows = self.peakgroup_jobs = self.peakgroup_stats = None
        self.peak_model = self.resid2 = self.subtract_comp = self.subtract_index = self.subtract_render_rows = None
        self.disc_rows = self.left_rows = self.left_peak_list = self.left_hole_list = self.subtract_stats = None

    def _moved(self, rows, has, xcols, ycols):
        """rows with the columns xcols / ycols of the rows `has` moved from the pixels of img_dev to catalog coordinates; rows
        itself when the two frames are one."""
        if not (self.bx or self.by):
            return rows
        rows = rows.copy()
        for cols, d in ((xcols, self.bx), (ycols, self.by)):
            for k in cols:
                rows[..., k][has] += d
        return rows

    def _ncomp(self):
        raw = np.asarray(self.raw, np.float64).reshape(len(self.sources), -1)
        return np.where(raw[:, DBL.status] == 1.0, 0, raw[:, DBL.ncomp]).astype(np.int32)

    def measure(self):
        """One cy_measure_sources call, then annotate()."""
        if not self.sources:
            return
        raw = self.det.measure_sources(self.img, self.boxes, ring=self.ring)
        raw = self._moved(raw, raw[:, MEAS.npix] > 0, (MEAS.x_peak,), (MEAS.y_peak,))
        if self.bx or self.by:
            raw[:, MEAS.swx] += self.bx * raw[:, MEAS.sw]
            raw[:, MEAS.swy] += self.by * raw[:, MEAS.sw]
        annotate(self.sources, raw, self.beam_area, self.wcs, self.wcs_origin)

    def background(self):
        """One cy_measure_background call, fill_mesh(), annotate_background(); leaves the filled mesh and the number of defined
        cells in .mesh / .ndef."""
        raw = self.det.measure_background(self.img, cell=self.cell, k=self.clip_sigma, niter=self.clip_iters)
        self.mesh, self.ndef = fill_mesh(raw, self.min_pix)
        annotate_background(self.sources, self.mesh, self.cell, self.box_origin)

    def islands(self):
        """Thresholds bkg + k * rms in numpy float64, one cy_measure_islands call, then annotate_islands()."""
        if not self.sources:
            return
        raw = self.det.measure_islands(self.img, self.boxes, island_thresholds(self.sources, self.k_seed, self.k_merge, self.use_map), conn=self.conn)
        raw = self._moved(raw, raw[:, ISL.npix] > 0, (ISL.xmin, ISL.xmax), (ISL.ymin, ISL.ymax))
        annotate_islands(self.sources, raw, self.win0 + np.array([self.bx, self.by]), self.beam_area, self.wcs, self.wcs_origin)

    def deblend(self):
        """One cy_deblend_islands call, then annotate_components(); leaves .raw, .comp and .masks (None unless .keep_masks) as the
        library gave them."""
        if not self.sources:
            return
        thr4 = deblend_thresholds(self.sources, self.k_seed, self.k_merge, self.k_peak, self.use_map)
        out = self.det.deblend_islands(self.img, self.boxes, thr4, conn=self.conn, radius=self.radius, return_masks=self.keep_masks)
        self.raw, self.comp, self.masks = out if self.keep_masks else out + (None,)
        has = np.arange(self.comp.shape[1])[None, :] < self.raw[:, DBL.ncomp].astype(np.int64)[:, None]
        annotate_components(self.sources, self.raw, self._moved(self.comp, has, (COMP.x_peak,), (COMP.y_peak,)),
                            self.win0 + np.array([self.bx, self.by]), self.beam_area, self.wcs, self.wcs_origin)

    def _fit_call(self, entry, start):
        """cy_fit_components / cy_fit_blends on the component step's masks with the background the thresholds were formed with."""
        n = len(self.sources)
        comp = np.asarray(self.comp, np.float64).reshape(n, -1, L.CY_DBL_COMP_FIELDS)
        bkg, ncomp = _bkg_of(self.sources, self.use_map), self._ncomp()
        rows = entry(self.img, self.boxes, bkg, ncomp, start(comp, bkg, self.win0), self.masks, max_iter=self.max_iter)
        return rows, np.arange(rows.shape[1])[None, :] < ncomp[:, None]

    def fit(self):
        """fit_start(), one cy_fit_components call, then annotate_fits(); leaves .fit_pixel_rows and .fit_rows."""
        if not self.sources:
            return
        rows, below = self._fit_call(self.det.fit_components, fit_start)
        self.fit_pixel_rows = rows
        self.fit_rows = self._moved(rows, below & (rows[:, :, FIT.status] != 1.0), (FIT.x0,), (FIT.y0,))
        annotate_fits(self.sources, self.fit_rows, self.beam_area, self.wcs, self.wcs_origin, self.use_map)

    def blend(self):
        """blend_start() from .fit_pixel_rows, one cy_fit_blends call, then annotate_blends(); leaves .blend_pixel_rows and
        .blend_rows."""
        self.blend_rows = self.blend_pixel_rows = np.zeros((0, L.CY_DBL_MAX_COMP, L.CY_BLEND_FIELDS), np.float64)
        if not self.sources:
            return
        fit_rows = np.asarray(self.fit_pixel_rows, np.float64).reshape(len(self.sources), -1, L.CY_FIT_FIELDS)
        rows, below = self._fit_call(self.det.fit_blends, lambda comp, bkg, win0: blend_start(fit_rows, comp, bkg, win0))
        self.blend_pixel_rows = rows
        self.blend_rows = self._moved(rows, below & np.isin(rows[:, :, BLEND.status], (0.0, 2.0, 3.0, 4.0, 5.0)), (BLEND.x0,), (BLEND.y0,))
        annotate_blends(self.sources, self.blend_rows, self.beam_area, self.wcs, self.wcs_origin, self.use_map)

    def residual(self):
        """render_selection() on the pixel rows, one cy_render_gaussians call over the whole image (minus the expanded mesh when
        there is one: else the residual keeps the background), one cy_measure_residuals call, then annotate_residuals(); leaves
        the device maps .model / .resid and .render_stats {"rendered", "duplicates", "capped"}."""
        src = self.sources
        comp, index, ndup = np.zeros((0, 6)), np.zeros((0, 2), np.int64), 0
        if src:
            comp, index, ndup = render_selection(src, self.fit_pixel_rows, self.blend_pixel_rows)
        bkg_dev = self.det.expand_background(self.mesh, self.cell, self.img.shape, want=("bkg",))[0] if self.use_map else None
        rows, self.model, self.resid = self.det.render_gaussians(self.img, comp, self.nsigma, bkg_dev)
        self.render_comp, self.render_index, self.render_rows = comp, index, rows
        if src:
            raw = self.det.measure_residuals(self.img, self.model, self.boxes, _bkg_of(src, self.use_map), self.masks)
            annotate_residuals(src, raw, index, rows, self.beam_area, self.box_origin, self.use_map)
        st = rows[:, RND.status]
        self.render_stats = {"rendered": int(np.isin(st, _FITTED).sum()), "duplicates": ndup, "capped": int((st == 2.0).sum())}

    def peaks(self):
        """After residual(): the rms map of the mesh expanded by a call of its own, one cy_find_peaks call on .resid (a second one with
        sign -1 when holes are wanted), the rows moved to catalog coordinates, then annotate_peaks(); leaves .peak_list, .hole_list
        (None unless holes are wanted) and .peak_stats {"peaks_ms", "peaks_kernel_ms", "peaks_found", "peaks_kept", "peaks_truncated"}
        (and their holes_ counterparts; peaks_ms is wall time and includes the expansion of the rms map)."""
        t1 = time.time()
        rms_dev = self.det.expand_background(self.mesh, self.cell, self.img.shape, want=("rms",))[1]
        self.peak_stats = {}
        for pre, sign in (("peaks_", 1), ("holes_", -1))[:2 if self.want_holes else 1]:
            rows, total = self.det.find_peaks(self.resid, rms_dev, k_sigma=self.peak_sigma, radius=self.peak_radius, sign=sign, cap=self.peak_cap)
            kernel_ms = self.det.peaks_kernel_ms()
            rows = self._moved(rows, np.ones(rows.shape[0], bool), (PEAK.x,), (PEAK.y,))
            found = annotate_peaks(self.sources, rows, total, self.peak_min_above, self.beam_area, self.wcs, self.wcs_origin, holes=sign < 0)
            if sign > 0:
                self.peak_list = found
            else:
                self.hole_list = found
            self.peak_stats.update({pre + "ms": 1e3 * (time.time() - t1), pre + "kernel_ms": kernel_ms, pre + "found": int(total), pre + "kept": len(found),
                                    pre + "truncated": int(total > rows.shape[0])})
            t1 = time.time()

    def scale_peaks(self):
        """After residual() (and peaks()): the a trous planes of .resid, c_0 = .resid, one cy_atrous_step call per scale j = 1 .. J
        with step 2^(j - 1) -> c_j, w_j (two smooth maps taken in turn, one detail map written again by every scale unless the planes
        are to be saved).  Every scale from .scale_first on is searched: a noise mesh of w_j alone (cy_measure_background with the
        cell scale_cell(), fill_mesh, the rms map expanded), then one cy_find_peaks call on w_j with the radius scale_radius(), sign
        +1 only (a wavelet plane has zero mean: every positive blob carries a negative ring).  The rows move to catalog coordinates,
        then annotate_scale_peaks(); leaves .scale_list, .scale_levels (per scale: step, cell, radius, searched, the kernel times,
        found), .scale_rows ({j: the rows of cy_find_peaks as the library gave them}), .scale_planes ({j: w_j} with save_scale_maps,
        else {}) and .scale_stats."""
        t1 = time.time()
        det, shape = self.det, self.img.shape
        smooth, detail, c = [None, None], None, self.resid
        levels, self.scale_levels, self.scale_planes, self.scale_rows = [], [], {}, {}
        st = {"atrous_kernel_ms": 0.0, "scales_background_kernel_ms": 0.0, "scales_peaks_kernel_ms": 0.0, "scales_found": 0, "scales_truncated": 0}
        for j in range(1, self.nscales + 1):
            step, k = 1 << (j - 1), j & 1
            smooth[k], w = det.atrous_step(c, step, want=("smooth", "detail"), out=(smooth[k], None if self.save_scales else detail))
            c = smooth[k]
            if not self.save_scales:
                detail = w
            lv = {"scale": j, "step": step, "searched": j >= self.scale_first, "atrous_kernel_ms": det.atrous_kernel_ms()}
            st["atrous_kernel_ms"] += lv["atrous_kernel_ms"]
            self.scale_levels.append(lv)
            if j < self.scale_first:
                continue
            cell, radius = scale_cell(self.cell, step), scale_radius(self.peak_radius, step)
            mesh, _ = fill_mesh(det.measure_background(w, cell=cell, k=self.clip_sigma, niter=self.clip_iters), self.min_pix)
            lv["background_kernel_ms"] = det.background_kernel_ms()
            rms_dev = det.expand_background(mesh, cell, shape, want=("rms",))[1]
            rows, total = det.find_peaks(w, rms_dev, k_sigma=self.scale_sigma, radius=radius, sign=1, cap=self.peak_cap)
            lv["peaks_kernel_ms"] = det.peaks_kernel_ms()
            lv.update(cell=cell, radius=radius, found=int(total))
            st["scales_background_kernel_ms"] += lv["background_kernel_ms"]
            st["scales_peaks_kernel_ms"] += lv["peaks_kernel_ms"]
            st["scales_found"] += int(total)
            st["scales_truncated"] += int(total > rows.shape[0])
            self.scale_rows[j] = rows
            levels.append((j, step, self._moved(rows, np.ones(rows.shape[0], bool), (PEAK.x,), (PEAK.y,)), total))
            if self.save_scales:
                self.scale_planes[j] = w
        self.scale_list = annotate_scale_peaks(self.sources, levels, self.peak_min_above, self.beam_area, self.wcs, self.wcs_origin)
        st["scales_kept"], st["scales_strongest"] = len(self.scale_list), sum(1 for d in self.scale_list if d["strongest"])
        st["scales_ms"] = 1e3 * (time.time() - t1)
        self.scale_stats = st

    def apertures(self):
        """After residual() and the searches: the rms map of the mesh expanded once, then per non-empty list (residual_peaks,
        residual_holes, residual_scale_peaks) one cy_aperture_sums call on .resid with the factor table ap_factors + (ap_annulus,):
        the centre of an entry is its x, y moved back to the pixels of img_dev, its unit ap_unit times its step (1 for the entries
        of the pixel searches); then annotate_apertures().  Leaves .aperture_rows ({list name: rows}) and .aperture_stats
        {"apertures_ms", "aperture_kernel_ms" (summed over the calls), "apertures_jobs", "apertures_measured", "apertures_clipped"}."""
        t1 = time.time()
        table = tuple(self.ap_factors) + (self.ap_annulus,)
        nap = len(self.ap_factors)
        self.aperture_rows = {}
        st = {"aperture_kernel_ms": 0.0, "apertures_jobs": 0, "apertures_measured": 0, "apertures_clipped": 0}
        lists = [(k, v) for k, v in (("residual_peaks", self.peak_list), ("residual_holes", self.hole_list),
                                     ("residual_scale_peaks", self.scale_list)) if v]
        rms_dev = self.det.expand_background(self.mesh, self.cell, self.img.shape, want=("rms",))[1] if lists else None
        for name, entries in lists:
            unit = np.array([self.ap_unit * float(d.get("step", 1)) for d in entries], np.float64)
            jobs = np.stack([np.array([d["x"] for d in entries], np.float64) - self.bx,
                             np.array([d["y"] for d in entries], np.float64) - self.by, unit], axis=1)
            rows = self.det.aperture_sums(self.resid, rms_dev, jobs, table)
            st["aperture_kernel_ms"] += max(self.det.aperture_kernel_ms(), 0.0)
            radii = unit[:, None] * np.array(self.ap_factors, np.float64)[None, :]
            annotate_apertures(entries, rows, nap, self.beam_area, radii)
            self.aperture_rows[name] = rows
            st["apertures_jobs"] += rows.shape[0]
            st["apertures_measured"] += int((rows[:, APER.status] == 0.0).sum())
            st["apertures_clipped"] += int((rows[:, APER.clipped] == 1.0).sum())
        st["apertures_ms"] = 1e3 * (time.time() - t1)
        self.aperture_stats = st

    def peak_fits(self):
        """After residual(), the searches and apertures(): the rms map of the mesh expanded once, then per non-empty list
        (residual_peaks, residual_holes with sign -1, residual_scale_peaks: its strongest entries only) one indexed read of .resid
        and one of the rms map at the entries' peak pixels, peak_fit_jobs(), one cy_fit_peaks call on .resid, the rows moved to
        catalog coordinates, then annotate_peak_fits().  Leaves .peakfit_rows, .peakfit_jobs (both as the library saw them, in the
        pixels of img_dev) and .peakfit_select ({list name: ...}; select: the entries that were fitted) and .peakfit_stats
        {"peakfit_ms", "peakfit_kernel_ms" (summed over the calls), "peakfit_jobs", "peakfit_converged", "peakfit_niter_mean",
        "peakfit_niter_max", "peakfit_crowded"}."""
        t1 = time.time()
        self.peakfit_rows, self.peakfit_jobs, self.peakfit_select, self.peakfit_rms = {}, {}, {}, {}
        st = {"peakfit_kernel_ms": 0.0}
        lists = [(k, v, sg) for k, v, sg in (("residual_peaks", self.peak_list, 1.0), ("residual_holes", self.hole_list, -1.0),
                                             ("residual_scale_peaks", self.scale_list, 1.0)) if v]
        rms_dev = self.det.expand_background(self.mesh, self.cell, self.img.shape, want=("rms",))[1] if lists else None
        every = []
        for name, entries, sign in lists:
            select = [i for i, d in enumerate(entries) if d.get("strongest", True)]
            chosen = [entries[i] for i in select]
            ix = np.clip(np.array([int(round(d["x_peak"] - self.bx)) for d in chosen], np.int64), 0, self.MW - 1)
            iy = np.clip(np.array([int(round(d["y_peak"] - self.by)) for d in chosen], np.int64), 0, self.MH - 1)
            at_peak, rms = _read_at(self.resid, iy, ix), _read_at(rms_dev, iy, ix)
            jobs = peak_fit_jobs(chosen, sign, self.pf_radius, self.pf_sigma, at_peak, self.box_origin)
            rows = np.zeros((0, L.CY_PFIT_FIELDS), np.float64)
            if select:                                        # a scale list may hold no strongest entry: no call, no kernel time
                rows = self.det.fit_peaks(self.resid, jobs, max_iter=self.pf_max_iter)
                st["peakfit_kernel_ms"] += max(self.det.peakfit_kernel_ms(), 0.0)
            has = ~np.isin(rows[:, PFIT.status], (1.0, 5.0))
            moved = self._moved(rows, has, (PFIT.x0, PFIT.wx0, PFIT.wx1), (PFIT.y0, PFIT.wy0, PFIT.wy1))
            annotate_peak_fits(entries, moved, jobs, rms, sign, self.beam_area, self.wcs, self.wcs_origin, select)
            self.peakfit_rows[name], self.peakfit_jobs[name], self.peakfit_select[name], self.peakfit_rms[name] = rows, jobs, select, rms
            every.append(rows)
        every = np.concatenate(every) if every else np.zeros((0, L.CY_PFIT_FIELDS), np.float64)
        (st["peakfit_jobs"], st["peakfit_converged"], st["peakfit_niter_mean"], st["peakfit_niter_max"], st["peakfit_crowded"]) = peak_fit_stats(every)
        st["peakfit_ms"] = 1e3 * (time.time() - t1)
        self.peakfit_stats = st

    def peak_groups(self):
        """After peak_fits(): per non-empty list peak_group_jobs() (the jobs of peak_fits() started from its rows), one
        cy_fit_peak_groups call on .resid, the rows moved to catalog coordinates, then annotate_peak_groups().  Leaves .peakgroup_rows
        and .peakgroup_jobs (as the library saw them, in the pixels of img_dev) and .peakgroup_stats {"peakgroup_ms",
        "peakgroup_kernel_ms" (summed over the calls that launched), "peakgroup_jobs", "peakgroup_members", "peakgroup_converged",
        "peakgroup_niter_mean", "peakgroup_niter_max", "peakgroup_over_limit"}."""
        t1 = time.time()
        self.peakgroup_rows, self.peakgroup_jobs = {}, {}
        st = {"peakgroup_kernel_ms": 0.0}
        lists = {"residual_peaks": (self.peak_list, 1.0), "residual_holes": (self.hole_list, -1.0), "residual_scale_peaks": (self.scale_list, 1.0)}
        every = []
        for name, single in self.peakfit_rows.items():
            entries, sign = lists[name]
            select = self.peakfit_select[name]
            jobs = peak_group_jobs(self.peakfit_jobs[name], single)
            rows = np.zeros((0, L.CY_PGRP_FIELDS), np.float64)
            if select:
                rows = self.det.fit_peak_groups(self.resid, jobs, link=self.pg_link, max_iter=self.pf_max_iter)
                if np.isin(rows[:, PGRP.status], (0.0, 2.0, 3.0, 4.0)).any():       # a call without a group job launches nothing
                    st["peakgroup_kernel_ms"] += max(self.det.peakgroup_kernel_ms(), 0.0)
            has = ~np.isin(rows[:, PGRP.status], (1.0, 5.0))
            moved = self._moved(rows, has, (PGRP.x0, PGRP.wx0, PGRP.wx1), (PGRP.y0, PGRP.wy0, PGRP.wy1))
            annotate_peak_groups(entries, moved, self.peakfit_rms[name], sign, self.beam_area, self.wcs, self.wcs_origin, select)
            self.peakgroup_rows[name], self.peakgroup_jobs[name] = rows, jobs
            every.append(rows)
        every = np.concatenate(every) if every else np.zeros((0, L.CY_PGRP_FIELDS), np.float64)
        (st["peakgroup_jobs"], st["peakgroup_members"], st["peakgroup_converged"], st["peakgroup_niter_mean"], st["peakgroup_niter_max"],
         st["peakgroup_over_limit"]) = peak_group_stats(every)
        st["peakgroup_ms"] = 1e3 * (time.time() - t1)
        self.peakgroup_stats = st

    def subtract(self):
        """After peak_fits() (and peak_groups()): peak_render_selection(), one cy_render_signed_gaussians call (holes carry a negative amplitude)
        with .resid as the image, no background and the nsigma of the residual step (made with no component too: the second residual is then the first), then
        per fitted list one cy_disc_residuals call on the second residual and the peak model with that list's jobs and
        annotate_peak_residuals().  Then the rms map of the mesh expanded once and cy_find_peaks on the second residual with the
        threshold, radius and cap of the pixel search, always in both signs (an over-subtraction only shows as a hole): the rows
        moved to catalog coordinates and annotate_peaks() with count keys of their own (SOURCE_LEFT_KEYS).  The apertures, the fits
        and the groups measured on the first residual, which stays as it is.  Leaves the device maps .peak_model / .resid2,
        .subtract_comp / .subtract_index / .subtract_render_rows (what was rendered), .disc_rows ({list name: rows} as the library
        gave them), .left_rows ({sign: the rows of cy_find_peaks}), .left_peak_list / .left_hole_list and .subtract_stats
        {"subtract_ms", "subtract_render_kernel_ms", "disc_residual_kernel_ms" (summed over the calls that launched),
        "subtract_selected", "subtract_rendered", "subtract_wandered", "subtract_duplicates", "left_peaks_kernel_ms" (both signs),
        "left_peaks", "left_holes" (kept entries), "left_truncated"}."""
        t1 = time.time()
        det = self.det
        comp, index, counts = peak_render_selection(self)
        rows, self.peak_model, self.resid2 = det.render_gaussians(self.resid, comp, self.nsigma, None, signed=True)
        self.subtract_comp, self.subtract_index, self.subtract_render_rows = comp, index, rows
        st = {"subtract_render_kernel_ms": det.render_kernel_ms(), "disc_residual_kernel_ms": 0.0, "subtract_selected": len(index),
              "subtract_rendered": int(np.isin(rows[:, RND.status], _FITTED).sum()), "subtract_wandered": counts["wandered"],
              "subtract_duplicates": counts["duplicates"]}
        lists = {"residual_peaks": self.peak_list, "residual_holes": self.hole_list, "residual_scale_peaks": self.scale_list}
        self.disc_rows = {}
        for name, jobs in self.peakfit_jobs.items():
            entries, select = lists[name], self.peakfit_select[name]
            raw = np.zeros((0, L.CY_DRES_FIELDS), np.float64)
            if select:
                raw = det.disc_residuals(self.resid2, self.peak_model, jobs)
                if (raw[:, DRES.status] == 0.0).any():                # a call without a measured job launches nothing
                    st["disc_residual_kernel_ms"] += max(det.disc_residual_kernel_ms(), 0.0)
            picked = {i: (source, int(r[RND.status])) for (nm, i), source, r in zip(index, counts["sources"], rows) if nm == name}
            annotate_peak_residuals(entries, raw, self.peakfit_rms[name], picked, self.beam_area, self.box_origin, select)
            self.disc_rows[name] = raw
        rms_dev = det.expand_background(self.mesh, self.cell, self.img.shape, want=("rms",))[1]
        self.left_rows, found, st["left_peaks_kernel_ms"], st["left_truncated"] = {}, {}, 0.0, 0
        for sign, key in ((1, SOURCE_LEFT_KEYS[0]), (-1, SOURCE_LEFT_KEYS[1])):
            raw, total = det.find_peaks(self.resid2, rms_dev, k_sigma=self.peak_sigma, radius=self.peak_radius, sign=sign, cap=self.peak_cap)
            st["left_peaks_kernel_ms"] += max(det.peaks_kernel_ms(), 0.0)
            st["left_truncated"] += int(total > raw.shape[0])
            self.left_rows[sign] = raw
            moved = self._moved(raw, np.ones(raw.shape[0], bool), (PEAK.x,), (PEAK.y,))
            found[sign] = annotate_peaks(self.sources, moved, total, self.peak_min_above, self.beam_area, self.wcs, self.wcs_origin, holes=sign < 0,
                                         keys=(key, None))
        self.left_peak_list, self.left_hole_list = found[1], found[-1]
        st["left_peaks"], st["left_holes"] = len(found[1]), len(found[-1])
        st["subtract_ms"] = 1e3 * (time.time() - t1)
        self.subtract_stats = st

    def forced(self):
        """After residual(): forced_jobs() for the components it rendered (.render_comp / .render_index with a render status of 0 or 2;
        kept in .forced_comp / .forced_index), then one cy_forced_fit
        call per map, with the nsigma and fit_bkg of forced_config(), and annotate_forced().
          self         the detection image; bkg of a job = its source's background, d_rms = the expanded rms map of the mesh when the
                       background step ran (weighted: the errors are sqrt(C_00)), else none (the errors are sqrt(C_00) times
                       the source's rms, as annotate_fits scales its own)
          other maps   in the order of forced_maps: uploaded (upload(det)), its own mesh by cy_measure_background / fill_mesh with
                       this chain's parameters, bkg of a job = sample_mesh at the component's centre, d_rms = its expanded rms
                       map; with no defined cell it is measured unweighted with bkg 0 and its errors are None.  The device copy
                       is dropped after its call
        Leaves .forced_rows / .forced_job_rows ({tag: rows} as the library gave / took them), .forced_images (what the catalog
        lists) and .forced_stats (FORCED_STATS; the kernel time summed over the calls that launched)."""
        t1 = time.time()
        det, src = self.det, self.sources
        # what the model map holds: a selected component that the render call turned away (status 1 or 3) is not forced either
        shown = np.isin(np.asarray(self.render_rows, np.float64).reshape(-1, L.CY_RND_FIELDS)[:, RND.status], _FITTED)
        comp, index = self.render_comp[shown], np.asarray(self.render_index, np.int64).reshape(-1, 2)[shown]
        maps, listed = [], []
        self.forced_rows, self.forced_job_rows = {}, {}
        self.forced_comp, self.forced_index = comp, index
        st = dict.fromkeys(FORCED_STATS, 0)
        st["forced_kernel_ms"] = 0.0

        def call(tag, dev, rms_dev, jobs, beam_area, freq, err_scale):
            rows = det.forced_fit(dev, rms_dev, jobs, self.forced_nsigma, self.forced_fit_bkg)
            if np.isin(rows[:, FORCED.status], (0.0, 2.0, 4.0, 5.0)).any():      # a call without a runnable job launches nothing
                st["forced_kernel_ms"] += max(det.forced_kernel_ms(), 0.0)
            self.forced_rows[tag], self.forced_job_rows[tag] = rows, jobs
            maps.append({"tag": tag, "rows": rows, "jobs": jobs, "beam_area": beam_area, "freq": freq, "err_scale": err_scale})
            status = rows[:, FORCED.status]
            st["forced_maps"] += 1
            st["forced_jobs"] += int(rows.shape[0])
            st["forced_fitted"] += int(np.isin(status, _FITTED).sum())
            st["forced_crowded"] += int((rows[:, FORCED.crowded] > 0).sum())
            st["forced_singular"] += int((status == 4.0).sum())

        m = comp.shape[0]
        rms_dev = det.expand_background(self.mesh, self.cell, self.img.shape, want=("rms",))[1] if self.use_map else None
        scale = np.ones(m) if self.use_map else np.array([_rms_of(src[int(i)], False) for i in index[:, 0]], np.float64).reshape(m)
        call("self", self.img, rms_dev, forced_jobs(comp, index, src, self.use_map), self.beam_area, self.freq, scale)
        listed.append({"tag": "self", "path": self.image_path, "freq": self.freq, "beam_area": float(self.beam_area) if self.beam_area else 0.0,
                       "mesh_ndef": self.ndef if self.use_map else None})
        del rms_dev
        for fm in self.forced_maps:
            dev = fm["upload"](det)
            if tuple(int(v) for v in dev.shape) != (self.MH, self.MW):
                raise L.CyError("forced_fit: map %s has shape %s, the image %s" % (fm["path"], tuple(dev.shape), (self.MH, self.MW)))
            mesh, ndef = fill_mesh(det.measure_background(dev, cell=self.cell, k=self.clip_sigma, niter=self.clip_iters), self.min_pix)
            rms_dev = det.expand_background(mesh, self.cell, dev.shape, want=("rms",))[1] if ndef > 0 else None
            jobs = forced_jobs(comp, index, src, mesh=mesh if ndef > 0 else 0.0, cell=self.cell)
            call(fm["tag"], dev, rms_dev, jobs, fm.get("beam_area") or 0, fm.get("freq"), np.ones(m) if ndef > 0 else None)
            listed.append({"tag": fm["tag"], "path": fm["path"], "freq": fm.get("freq"), "beam_area": float(fm.get("beam_area") or 0.0), "mesh_ndef": int(ndef)})
            del dev, rms_dev
        annotate_forced(src, index, maps)
        self.forced_images = listed
        st["forced_ms"] = 1e3 * (time.time() - t1)
        self.forced_stats = st

    def run(self, steps, stats=None, t0=None):
        """The steps named in `steps` (plan()) in the order of STEPS, then peaks(), scale_peaks(), apertures(), peak_fits(), peak_groups(), subtract() and forced(), each when the
        config asks for it and the residual step ran.  stats: a dictionary that takes, per step that ran, <step>_ms
        (wall time), the kernel times and the counts; t0: when the first step's clock started, if before this call."""
        det, src = self.det, self.sources
        self.keep_masks = "fit" in steps                     # the component step hands its masks on only when a step reads them
        for step in STEPS:
            if step not in steps:
                continue
            t1 = t0 if (step == "measure" and t0 is not None) else time.time()
            getattr(self, step)()
            if stats is None:
                continue
            stats[step + "_ms"] = 1e3 * (time.time() - t1)
            if step == "background":
                stats["background_kernel_ms"] = det.background_kernel_ms()
            elif step == "fit":
                stats["fit_kernel_ms"] = max(det.fit_kernel_ms(), 0.0) if src else 0.0
                stats["fit_jobs"], stats["fit_niter_mean"], stats["fit_niter_max"] = fit_iterations(self.fit_rows)
            elif step == "blend":
                stats["blend_kernel_ms"] = max(det.blend_kernel_ms(), 0.0) if src else 0.0
                stats["blend_jobs"], stats["blend_niter_mean"], stats["blend_niter_max"], stats["blend_over_limit"] = blend_stats(self.blend_rows)
            elif step == "residual":
                stats["render_kernel_ms"] = det.render_kernel_ms()
                stats["residual_kernel_ms"] = det.residual_kernel_ms() if src else 0.0
                for k, v in self.render_stats.items():
                    stats["residual_" + k] = v
            else:
                stats[step + "_kernel_ms"] = getattr(det, step + "_kernel_ms")() if src else 0.0
        if self.want_peaks and "residual" in steps:
            self.peaks()
            if stats is not None:
                stats.update(self.peak_stats)
        if self.nscales > 0 and "residual" in steps:
            self.scale_peaks()
            if stats is not None:
                stats.update(self.scale_stats)
        if self.want_apertures and "residual" in steps:
            self.apertures()
            if stats is not None:
                stats.update(self.aperture_stats)
        if self.want_peak_fits and "residual" in steps:
            self.peak_fits()
            if stats is not None:
                stats.update(self.peakfit_stats)
        if self.want_peak_groups and "residual" in steps:
            self.peak_groups()
            if stats is not None:
                stats.update(self.peakgroup_stats)
        if self.want_subtract and "residual" in steps:
            self.subtract()
            if stats is not None:
                stats.update(self.subtract_stats)
        if self.want_forced and "residual" in steps:
            self.forced()
            if stats is not None:
                stats.update(self.forced_stats)
        return self

    def save_maps(self, catalog_path):
        """--save_bkg_maps / --save_residual_maps, after run(): the maps of the mesh and of the residual step (and, when the fitted peaks were
        subtracted, the peak model and the second residual) beside the catalog."""
        if self.save_bkg:
            save_background_maps(self.det, self.mesh, self.cell, self.img.shape, catalog_path)
        if self.save_residual:
            save_residual_maps(self.model, self.resid, catalog_path)
            if self.resid2 is not None:
                save_second_residual_maps(self.peak_model, self.resid2, catalog_path)
        if self.save_scales and self.scale_planes:
            save_scale_maps(self.scale_planes, catalog_path)
