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

Everything below is float64 arithmetic on those rows: given the rows, the keys are deterministic."""
import math

import numpy as np

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
FIT_SIGMA2_MIN = 0.25              # px^2: floor of the eigenvalues of a start covariance
FWHM = 2.3548200450309493          # 2 sqrt(2 ln 2): FWHM of a Gaussian in units of its sigma


def boxes_of(sources):
    """[n, 4] float64 {x1, y1, x2, y2} of catalog source dicts."""
    return np.array([[s["x1"], s["y1"], s["x2"], s["y2"]] for s in sources], np.float64).reshape(-1, 4)


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
        npix, _, bkg, rms, peak, xp, yp, total, sw, swx, swy = (float(v) for v in r[:11])
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
        if wcs is not None:
            a, d = wcs.wcs_pix2world(x0 + ox, y0 + oy, 0)
            s["ra"], s["dec"] = float(a), float(d)
        else:
            s["ra"], s["dec"] = None, None
    return sources


def measure_and_annotate(det, img_dev, sources, ring, beam_area, wcs, box_origin=(0, 0), wcs_origin=(0, 0)):
    """One cy_measure_sources call over `sources` on the device image, then annotate().  box_origin: the catalog boxes'
    coordinates of pixel [0, 0] of img_dev (subtracted before measuring; x_peak, y_peak, x0, y0 come back in catalog
    coordinates).  wcs_origin: position of catalog coordinate (0, 0) in the frame of the WCS."""
    if not sources:
        return sources
    bx, by = float(box_origin[0]), float(box_origin[1])
    boxes = boxes_of(sources) - np.array([bx, by, bx, by], np.float64)
    raw = det.measure_sources(img_dev, boxes, ring=ring)
    if bx or by:
        raw = raw.copy()
        has = raw[:, 0] > 0
        raw[has, 5] += bx
        raw[has, 6] += by
        raw[:, 9] += bx * raw[:, 8]
        raw[:, 10] += by * raw[:, 8]
    return annotate(sources, raw, beam_area, wcs, wcs_origin)


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
    cxx, cyy, cxy = Sxx / S - mx * mx, Syy / S - my * my, Sxy / S - mx * my
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
        if r[0] != 0.0:
            continue
        s["island_count"], s["island_npix"], s["island_npix_main"], s["island_border"] = int(r[2]), int(r[3]), int(r[4]), bool(r[5] > 0)
        if r[1] == 0.0:
            continue
        s["island_x1"], s["island_x2"], s["island_y1"], s["island_y2"] = (int(v) for v in r[6:10])
        S, Sx, Sy, Sxx, Syy, Sxy, Sm = (float(v) for v in r[10:17])
        s["island_flux_sum"] = S
        if ba > 0.0:
            s["island_flux"], s["island_flux_main"] = S / ba, Sm / ba
        if S == 0.0:
            continue
        s["x_isl"], s["y_isl"] = float(wx0) + Sx / S, float(wy0) + Sy / S
        s["major"], s["minor"], s["pa"] = island_shape(S, Sx, Sy, Sxx, Syy, Sxy)
        if wcs is not None:
            a, d = wcs.wcs_pix2world(s["x_isl"] + ox, s["y_isl"] + oy, 0)
            s["ra_isl"], s["dec_isl"] = float(a), float(d)
    return sources


def island_thresholds(sources, k_seed, k_merge, use_map=False):
    """[n, 3] float64 {seed_thr, merge_thr, bkg} from the bkg and rms the first step (annotate) left on the sources; use_map: from
    the bkg_map and rms_map of the background mesh (annotate_background) instead."""
    kb, kr = ("bkg_map", "rms_map") if use_map else ("bkg", "rms")
    bkg = np.array([s[kb] for s in sources], np.float64)
    rms = np.array([s[kr] for s in sources], np.float64)
    return np.stack([bkg + float(k_seed) * rms, bkg + float(k_merge) * rms, bkg], 1)


def islands_and_annotate(det, img_dev, sources, k_seed, k_merge, conn, beam_area, wcs, box_origin=(0, 0), wcs_origin=(0, 0), use_map=False):
    """The island step, after measure_and_annotate on the same sources and image: thresholds bkg + k * rms in numpy float64, one
    cy_measure_islands call, then annotate_islands().  box_origin / wcs_origin as in measure_and_annotate: positions come back in
    catalog coordinates.  use_map: thresholds (and the bkg of the sums) from bkg_map / rms_map, after background_and_annotate."""
    if not sources:
        return sources
    bx, by = float(box_origin[0]), float(box_origin[1])
    boxes = boxes_of(sources) - np.array([bx, by, bx, by], np.float64)
    raw = det.measure_islands(img_dev, boxes, island_thresholds(sources, k_seed, k_merge, use_map), conn=conn)
    MH, MW = int(img_dev.shape[0]), int(img_dev.shape[1])
    win0 = np.array([box_window(b, MH, MW)[:2] for b in boxes], np.float64).reshape(-1, 2) + np.array([bx, by])
    if bx or by:
        raw = raw.copy()
        has = raw[:, 3] > 0
        raw[has, 6:8] += bx
        raw[has, 8:10] += by
    return annotate_islands(sources, raw, win0, beam_area, wcs, wcs_origin)


# ---- source components (--deblend_islands)
def deblend_thresholds(sources, k_seed, k_merge, k_peak, use_map=False):
    """[n, 4] float64 {seed_thr, merge_thr, bkg, peak_thr}: island_thresholds() plus bkg + k_peak * rms."""
    t = island_thresholds(sources, k_seed, k_merge, use_map)
    kb, kr = ("bkg_map", "rms_map") if use_map else ("bkg", "rms")
    bkg = np.array([s[kb] for s in sources], np.float64)
    rms = np.array([s[kr] for s in sources], np.float64)
    return np.concatenate([t.reshape(-1, 3), (bkg + float(k_peak) * rms).reshape(-1, 1)], 1)


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
    comp = np.asarray(comp, np.float64).reshape(n, -1, 12)                # CY_DBL_COMP_FIELDS
    win0 = np.asarray(win0, np.float64).reshape(n, 2)
    ox, oy = float(origin[0]), float(origin[1])
    ba = float(beam_area) if beam_area else 0.0
    for s, r, cr, (wx0, wy0) in zip(sources, raw, comp, win0):
        for k in COMPONENT_KEYS:
            s[k] = None
        if r[0] == 1.0:
            continue
        s["npeaks"], s["ncomponents"], s["components_truncated"], s["components_unassigned_npix"] = int(r[2]), int(r[3]), bool(r[0] == 2.0), int(r[5])
        items = []
        for c in cr[:int(r[3])]:
            S, Sx, Sy, Sxx, Syy, Sxy = (float(v) for v in c[4:10])
            d = dict.fromkeys(COMPONENT_ITEM_KEYS)
            d["peak"], d["x_peak"], d["y_peak"], d["npix"] = float(c[1]), int(c[2]), int(c[3]), int(c[0])
            d["flux_sum"], d["main"], d["nsummits"] = S, bool(c[10] != 0.0), int(c[11])
            if ba > 0.0:
                d["flux"] = S / ba
            if S != 0.0:
                d["x"], d["y"] = float(wx0) + Sx / S, float(wy0) + Sy / S
                d["major"], d["minor"], d["pa"] = island_shape(S, Sx, Sy, Sxx, Syy, Sxy)
                if wcs is not None:
                    a, dd = wcs.wcs_pix2world(d["x"] + ox, d["y"] + oy, 0)
                    d["ra"], d["dec"] = float(a), float(dd)
            items.append(d)
        s["components"] = items
    return sources


def deblend_and_annotate(det, img_dev, sources, k_seed, k_merge, k_peak, conn, radius, beam_area, wcs, box_origin=(0, 0), wcs_origin=(0, 0),
                         use_map=False, return_raw=False):
    """The component step, after islands_and_annotate on the same sources and image: thresholds in numpy float64, one
    cy_deblend_islands call, then annotate_components().  box_origin / wcs_origin / use_map as in islands_and_annotate: positions
    come back in catalog coordinates.  return_raw: -> (sources, raw rows, component rows, masks) as HipDetector.deblend_islands
    returns them with return_masks, in the pixel frame of img_dev: what fit_and_annotate() takes, so that the kernel runs once."""
    if not sources:
        return (sources, np.zeros((0, 8)), np.zeros((0, 16, 12)), []) if return_raw else sources
    bx, by = float(box_origin[0]), float(box_origin[1])
    boxes = boxes_of(sources) - np.array([bx, by, bx, by], np.float64)
    thr4 = deblend_thresholds(sources, k_seed, k_merge, k_peak, use_map)
    if return_raw:
        raw, comp, masks = det.deblend_islands(img_dev, boxes, thr4, conn=conn, radius=radius, return_masks=True)
        keep = (sources, raw, comp, masks)
    else:
        raw, comp = det.deblend_islands(img_dev, boxes, thr4, conn=conn, radius=radius)
    MH, MW = int(img_dev.shape[0]), int(img_dev.shape[1])
    win0 = np.array([box_window(b, MH, MW)[:2] for b in boxes], np.float64).reshape(-1, 2) + np.array([bx, by])
    annotate_components(sources, raw, _shift_comp(raw, comp, bx, by), win0, beam_area, wcs, wcs_origin)
    return keep if return_raw else sources


def _shift_comp(raw, comp, bx, by):
    """Component rows with the peak positions of the rows below ncomp moved by (bx, by); a copy when anything moves."""
    if not (bx or by):
        return comp
    comp = comp.copy()
    has = np.arange(comp.shape[1])[None, :] < raw[:, 3].astype(np.int64)[:, None]
    comp[:, :, 2][has] += bx
    comp[:, :, 3][has] += by
    return comp


# ---- component fits (--fit_components)
def fit_start(comp_rows, bkg, win0):
    """Start values {A, x0, y0, a, b, c} of the fit from component rows (lib.DBL_COMP_NAMES): comp_rows [..., 12], bkg [...] and
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
    S, Sx, Sy, Sxx, Syy, Sxy = (r[..., k] for k in range(4, 10))
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
    out[..., 0] = r[..., 1] - bkg
    out[..., 1] = np.where(good, w0[..., 0] + mx, r[..., 2])
    out[..., 2] = np.where(good, w0[..., 1] + my, r[..., 3])
    out[..., 3] = np.where(good, a, 1.0)
    out[..., 4] = np.where(good, b, 0.0)
    out[..., 5] = np.where(good, c, 1.0)
    return out


def gaussian_shape(a, b, c):
    """(major, minor, pa) of a fitted Gaussian with inverse covariance [[a, b], [b, c]]: FWHM * sqrt of the eigenvalues of the
    covariance, in pixels; pa as island_shape(): angle of the major axis from +x towards +y in degrees, in (-90, 90], 0 for a
    circle."""
    det = a * c - b * b
    cxx, cyy, cxy = c / det, a / det, -b / det
    half, d = (cxx + cyy) / 2.0, math.hypot((cxx - cyy) / 2.0, cxy)
    l1, l2 = max(half + d, 0.0), max(half - d, 0.0)
    pa = 0.0
    if l1 != l2:
        pa = 0.5 * math.degrees(math.atan2(2.0 * cxy + 0.0, cxx - cyy))
        if pa <= -90.0:
            pa += 180.0
    return FWHM * math.sqrt(l1), FWHM * math.sqrt(l2), pa


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
    H[np.triu_indices(6)] = np.asarray(row, np.float64)[11:32]
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
    fit = np.asarray(fit, np.float64).reshape(len(sources), -1, 32)       # CY_FIT_FIELDS
    ox, oy = float(origin[0]), float(origin[1])
    ba = float(beam_area) if beam_area else 0.0
    for s, fr in zip(sources, fit):
        rms = s.get("rms_map" if use_map else "rms")
        rms = float(rms) if rms else 0.0
        for d, r in zip(s.get("components") or [], fr):
            for k in FIT_KEYS:
                d[k] = None
            st = int(r[0])
            d["fit_status"], d["fit_niter"], d["fit_npix"] = st, int(r[1]), int(r[2])
            if st not in (0, 2):
                continue
            p = [float(v) for v in r[5:11]]
            d["fit_chi2"] = float(r[3]) / (rms * rms) if rms > 0.0 else None
            d["fit_peak"], d["fit_x"], d["fit_y"] = p[0], p[1], p[2]
            d["fit_major"], d["fit_minor"], d["fit_pa"] = gaussian_shape(p[3], p[4], p[5])
            if wcs is not None:
                a, dd = wcs.wcs_pix2world(p[1] + ox, p[2] + oy, 0)
                d["fit_ra"], d["fit_dec"] = float(a), float(dd)
            if ba > 0.0:
                d["fit_flux"] = fit_flux(p, ba)
            cov = fit_covariance(r, rms) if rms > 0.0 else None
            if cov is not None:
                d["fit_peak_err"], d["fit_x_err"], d["fit_y_err"] = (math.sqrt(cov[k, k]) for k in range(3))
                if ba > 0.0:
                    g = fit_flux_grad(p, ba)
                    d["fit_flux_err"] = math.sqrt(max(float(g @ cov @ g), 0.0))
    return sources


def fit_and_annotate(det, img_dev, sources, raw, comp, masks, beam_area, wcs, box_origin=(0, 0), wcs_origin=(0, 0), use_map=False,
                     max_iter=64, return_pixel_rows=False):
    """The fit step, after deblend_and_annotate(..., return_raw=True) on the same sources and image, whose raw rows, component rows
    and masks it takes (pixel frame of img_dev): fit_start(), one cy_fit_components call, then annotate_fits().  The background of
    a source is the one its thresholds were formed with (bkg, or bkg_map with use_map).  -> the fit rows, centres in catalog
    coordinates; with return_pixel_rows -> (those rows, the rows as the library gave them, in the pixel frame of img_dev: what
    blends_and_annotate() takes)."""
    n = len(sources)
    if not n:
        return (np.zeros((0, 16, 32), np.float64),) * 2 if return_pixel_rows else np.zeros((0, 16, 32), np.float64)
    bx, by = float(box_origin[0]), float(box_origin[1])
    boxes = boxes_of(sources) - np.array([bx, by, bx, by], np.float64)
    MH, MW = int(img_dev.shape[0]), int(img_dev.shape[1])
    win0 = np.array([box_window(b, MH, MW)[:2] for b in boxes], np.float64).reshape(-1, 2)
    bkg = np.array([s["bkg_map" if use_map else "bkg"] for s in sources], np.float64)
    raw = np.asarray(raw, np.float64).reshape(n, -1)
    ncomp = np.where(raw[:, 0] == 1.0, 0, raw[:, 3]).astype(np.int32)
    start = fit_start(np.asarray(comp, np.float64).reshape(n, -1, 12), bkg, win0)
    fit = det.fit_components(img_dev, boxes, bkg, ncomp, start, masks, max_iter=max_iter)
    pixel_rows = fit.copy() if return_pixel_rows else None
    if bx or by:
        has = (np.arange(fit.shape[1])[None, :] < ncomp[:, None]) & (fit[:, :, 0] != 1.0)
        fit[:, :, 6][has] += bx
        fit[:, :, 7][has] += by
    annotate_fits(sources, fit, beam_area, wcs, wcs_origin, use_map)
    return (fit, pixel_rows) if return_pixel_rows else fit


def fit_iterations(fit):
    """(jobs, mean niter, largest niter) over the fitted rows (status 0 or 2) of cy_fit_components; (0, 0.0, 0) without one."""
    fit = np.asarray(fit, np.float64).reshape(-1, 32)
    it = fit[(fit[:, 1] > 0) & ((fit[:, 0] == 0.0) | (fit[:, 0] == 2.0)), 1]
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
    [..., 32]) when that row's status is 0 or 2, else fit_start(comp_rows, bkg, win0).  Both in the same pixel frame.
    -> float64 [..., 6]."""
    fit_rows = np.asarray(fit_rows, np.float64)
    out = fit_start(comp_rows, bkg, win0)
    use = ((fit_rows[..., 0] == 0.0) | (fit_rows[..., 0] == 2.0)) & (fit_rows[..., 1] > 0.0)     # niter 0: a row beyond ncomp
    out[use] = fit_rows[..., 5:11][use]
    return out


def blend_covariance(row, rms):
    """rms^2 times the member's 6 x 6 block of inv(H) from a blend row (lib.BLEND_NAMES); None when cov_ok is 0 or it is not finite."""
    row = np.asarray(row, np.float64)
    if row[14] == 0.0:
        return None
    C = np.zeros((6, 6), np.float64)
    C[np.triu_indices(6)] = row[15:36]
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
    rows = np.asarray(rows, np.float64).reshape(len(sources), -1, 36)     # CY_BLEND_FIELDS
    ox, oy = float(origin[0]), float(origin[1])
    ba = float(beam_area) if beam_area else 0.0
    for s, br in zip(sources, rows):
        rms = s.get("rms_map" if use_map else "rms")
        rms = float(rms) if rms else 0.0
        for d, r in zip(s.get("components") or [], br):
            for k in BLEND_KEYS:
                d[k] = None
            st = int(r[0])
            d["blend_group"], d["blend_size"], d["blend_status"], d["blend_niter"], d["blend_npix"] = int(r[5]), int(r[6]), st, int(r[1]), int(r[2])
            if st == 6:
                for k in BLEND_KEYS[5:]:
                    d[k] = d.get("fit_" + k[6:])
                continue
            if st not in (0, 2):
                continue
            p = [float(v) for v in r[8:14]]
            d["blend_chi2"] = float(r[3]) / (rms * rms) if rms > 0.0 else None
            d["blend_peak"], d["blend_x"], d["blend_y"] = p[0], p[1], p[2]
            d["blend_major"], d["blend_minor"], d["blend_pa"] = gaussian_shape(p[3], p[4], p[5])
            if wcs is not None:
                a, dd = wcs.wcs_pix2world(p[1] + ox, p[2] + oy, 0)
                d["blend_ra"], d["blend_dec"] = float(a), float(dd)
            if ba > 0.0:
                d["blend_flux"] = fit_flux(p, ba)
            cov = blend_covariance(r, rms) if rms > 0.0 else None
            if cov is not None:
                d["blend_peak_err"], d["blend_x_err"], d["blend_y_err"] = (math.sqrt(cov[k, k]) for k in range(3))
                if ba > 0.0:
                    g = fit_flux_grad(p, ba)
                    d["blend_flux_err"] = math.sqrt(max(float(g @ cov @ g), 0.0))
    return sources


def blends_and_annotate(det, img_dev, sources, raw, comp, masks, fit_rows, beam_area, wcs, box_origin=(0, 0), wcs_origin=(0, 0),
                        use_map=False, max_iter=64, return_pixel_rows=False):
    """The joint-fit step, after fit_and_annotate(..., return_pixel_rows=True) on the same sources, image, raw rows, component
    rows and masks, whose fit rows in the pixel frame of img_dev it takes: blend_start(), one cy_fit_blends call, then
    annotate_blends().  -> the blend rows, centres in catalog coordinates; with return_pixel_rows -> (those rows, the rows as the
    library gave them, in the pixel frame of img_dev: what residuals_and_annotate() takes)."""
    n = len(sources)
    if not n:
        return (np.zeros((0, 16, 36), np.float64),) * 2 if return_pixel_rows else np.zeros((0, 16, 36), np.float64)
    bx, by = float(box_origin[0]), float(box_origin[1])
    boxes = boxes_of(sources) - np.array([bx, by, bx, by], np.float64)
    MH, MW = int(img_dev.shape[0]), int(img_dev.shape[1])
    win0 = np.array([box_window(b, MH, MW)[:2] for b in boxes], np.float64).reshape(-1, 2)
    bkg = np.array([s["bkg_map" if use_map else "bkg"] for s in sources], np.float64)
    raw = np.asarray(raw, np.float64).reshape(n, -1)
    ncomp = np.where(raw[:, 0] == 1.0, 0, raw[:, 3]).astype(np.int32)
    fit_rows = np.asarray(fit_rows, np.float64).reshape(n, -1, 32)
    start = blend_start(fit_rows, np.asarray(comp, np.float64).reshape(n, -1, 12), bkg, win0)
    rows = det.fit_blends(img_dev, boxes, bkg, ncomp, start, masks, max_iter=max_iter)
    pixel_rows = rows.copy() if return_pixel_rows else None
    if bx or by:
        has = (np.arange(rows.shape[1])[None, :] < ncomp[:, None]) & np.isin(rows[:, :, 0], (0.0, 2.0, 3.0, 4.0, 5.0))
        rows[:, :, 9][has] += bx
        rows[:, :, 10][has] += by
    annotate_blends(sources, rows, beam_area, wcs, wcs_origin, use_map)
    return (rows, pixel_rows) if return_pixel_rows else rows


def blend_stats(rows):
    """(jobs, mean niter, largest niter, groups above CY_BLEND_MAX_MEMBERS) over the rows of cy_fit_blends: a fitted job (status 0
    or 2) is counted once, on its slot-0 row, as is a group above the limit (status 5); (0, 0.0, 0, 0) without any."""
    rows = np.asarray(rows, np.float64).reshape(-1, 36)
    first = rows[:, 7] == 0.0
    it = rows[first & (rows[:, 1] > 0) & ((rows[:, 0] == 0.0) | (rows[:, 0] == 2.0)), 1]
    over = int((first & (rows[:, 0] == 5.0)).sum())
    return (int(it.size), float(it.mean()), int(it.max()), over) if it.size else (0, 0.0, 0, over)


# ---- model and residual maps (--residual_map)
def _fitted_params(fit_row, blend_row):
    """The six parameters a component is rendered with: those of its blend row when that row's status is 0 or 2, else those of its
    fit row when that row's status is 0 or 2, else None."""
    if blend_row is not None and blend_row[0] in (0.0, 2.0):
        return blend_row[8:14]
    if fit_row[0] in (0.0, 2.0):
        return fit_row[5:11]
    return None


def render_selection(sources, fit_rows, blend_rows=None):
    """The components cy_render_gaussians is given, after annotate_components() on `sources`.  fit_rows [n, 16, CY_FIT_FIELDS] /
    blend_rows [n, 16, CY_BLEND_FIELDS] (or None): the rows of cy_fit_components / cy_fit_blends with their centres in the pixel frame
    of the image that is rendered.  Per component of every source, in source order, then component order:
      parameters   the blend row's when its status is 0 or 2, else the fit row's when its status is 0 or 2, else it is not rendered
      duplicates   overlapping boxes share islands, so the same peak can be a component of two sources; a component whose kept peak
                   pixel (x_peak, y_peak) was already taken by an earlier rendered component is not rendered: the model counts a
                   peak once
    -> (comp float64 [m, 6] {A, x0, y0, a, b, c}, index int64 [m, 2] {source, component}, the number of duplicates left out)."""
    n = len(sources)
    fit_rows = np.asarray(fit_rows, np.float64).reshape(n, 16, 32)        # CY_DBL_MAX_COMP, CY_FIT_FIELDS
    blend_rows = None if blend_rows is None else np.asarray(blend_rows, np.float64).reshape(n, 16, 36)     # CY_BLEND_FIELDS
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
    status = {(int(i), int(k)): int(r[0]) for (i, k), r in zip(np.asarray(index).reshape(-1, 2), np.asarray(render_rows).reshape(-1, 8))}     # CY_RND_FIELDS
    for i, (s, r) in enumerate(zip(sources, raw)):
        for k, d in enumerate(s.get("components") or []):
            st = status.get((i, k))
            d["rendered"], d["render_status"] = st in (0, 2), st
        for key in RESIDUAL_KEYS:
            s[key] = None
        n_isl = int(r[2]) if r[0] == 0.0 else 0
        s["res_npix"] = n_isl
        if n_isl == 0:
            continue
        rms = s.get("rms_map" if use_map else "rms")
        rms = float(rms) if rms else 0.0
        s["res_mean"], s["res_rms"] = float(r[5]) / n_isl, math.sqrt(float(r[6]) / n_isl)
        s["res_rms_box"] = math.sqrt(float(r[4]) / float(r[1])) if r[1] > 0 else None
        s["res_max"], s["res_x_max"], s["res_y_max"] = float(r[7]), int(r[8]) + ox, int(r[9]) + oy
        if ba > 0.0:
            s["res_flux"], s["res_model_flux"] = float(r[5]) / ba, float(r[10]) / ba
        s["res_ratio"] = s["res_rms"] / rms if rms > 0.0 else None
    return sources


def residuals_and_annotate(det, img_dev, sources, masks, fit_rows, blend_rows=None, nsigma=5.0, bkg_dev=None, beam_area=0, box_origin=(0, 0),
                           use_map=False):
    """The residual step, after fit_and_annotate(..., return_pixel_rows=True) (and blends_and_annotate) on the same sources and
    image: render_selection() on their rows in the pixel frame of img_dev (return_pixel_rows), one cy_render_gaussians call over the
    whole image (bkg_dev: the expanded background map, or None: the residual keeps the background), one cy_measure_residuals
    call on the boxes with the masks of deblend_and_annotate and the background the fits used, then annotate_residuals().
    -> (model, resid device maps, {"rendered", "duplicates", "capped"})."""
    n = len(sources)
    bx, by = float(box_origin[0]), float(box_origin[1])
    comp, index, ndup = render_selection(sources, fit_rows, blend_rows) if n else (np.zeros((0, 6)), np.zeros((0, 2), np.int64), 0)
    rows, model, resid = det.render_gaussians(img_dev, comp, nsigma, bkg_dev)
    if n:
        boxes = boxes_of(sources) - np.array([bx, by, bx, by], np.float64)
        bkg = np.array([s["bkg_map" if use_map else "bkg"] for s in sources], np.float64)
        raw = det.measure_residuals(img_dev, model, boxes, bkg, masks)
        annotate_residuals(sources, raw, index, rows, beam_area, box_origin, use_map)
    stats = {"rendered": int(np.isin(rows[:, 0], (0.0, 2.0)).sum()), "duplicates": ndup, "capped": int((rows[:, 0] == 2.0).sum())}
    return model, resid, stats


def save_residual_maps(model, resid, catalog_path):
    """--save_residual_maps: the two device maps written as fp32 FITS images model_<name>.fits / resid_<name>.fits beside the
    catalog file, <name> = the catalog's file name without its extension.  -> the two paths."""
    import os
    from . import utils
    d, name = os.path.split(catalog_path)
    name = os.path.splitext(name)[0]
    paths = []
    for tag, m in zip(("model_", "resid_"), (model, resid)):
        paths.append(os.path.join(d, tag + name + ".fits"))
        utils.write_fits_image(paths[-1], m.cpu().numpy())
    return tuple(paths)


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
    ok = raw[:, :, 1] >= float(min_pix)
    dy, dx = np.nonzero(ok)                                  # row-major order: the first minimum is the smallest index
    if dy.size == 0:
        return mesh, 0
    mesh[ok] = raw[:, :, 2:4][ok]
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


def background_and_annotate(det, img_dev, sources, cell=128, k=3.0, niter=3, min_pix=64, box_origin=(0, 0)):
    """The background step, after measure_and_annotate on the same sources and image: one cy_measure_background call, fill_mesh(),
    annotate_background().  -> (filled mesh [ncy, ncx, 2], number of defined cells); box_origin as in measure_and_annotate."""
    raw = det.measure_background(img_dev, cell=cell, k=k, niter=niter)
    mesh, ndef = fill_mesh(raw, min_pix)
    annotate_background(sources, mesh, cell, box_origin)
    return mesh, ndef


def save_background_maps(det, mesh, cell, shape, catalog_path):
    """--save_bkg_maps: the mesh expanded on the GPU (HipDetector.expand_background) and written as fp32 FITS images
    bkg_<name>.fits / rms_<name>.fits beside the catalog file, <name> = the catalog's file name without its extension.
    -> the two paths."""
    import os
    from . import utils
    d, name = os.path.split(catalog_path)
    name = os.path.splitext(name)[0]
    paths = []
    for tag, m in zip(("bkg_", "rms_"), det.expand_background(mesh, cell, shape)):
        paths.append(os.path.join(d, tag + name + ".fits"))
        utils.write_fits_image(paths[-1], m.cpu().numpy())
    return tuple(paths)


def background_config(config):
    """(cell, k, niter, min_pix) of --bkg_map from a config dictionary."""
    return (int(config.get('bkg_cell', 128)), float(config.get('bkg_clip_sigma', 3.0)), int(config.get('bkg_clip_iters', 3)),
            int(config.get('bkg_min_pix', 64)))
