"""Catalog source measurement, host side: from the raw rows of `cy_measure_sources` (HipDetector.measure_sources) to the keys a
catalog source carries with --measure_sources.  The reference's catalog stops at boxes; this is an addition.

Raw row (lib.MEAS_NAMES): npix nring bkg rms peak x_peak y_peak sum sw swx swy reserved -- counts of valid pixels (non-zero and
finite) in the box window and in the background ring, the ring's median and 1.4826 x its median absolute deviation, the largest
valid pixel of the box and where it first occurs, the sum of (v - bkg) and the moments of the weights max(v - bkg, 0).  All positions
are 0-based pixel indices of the measured image with a pixel's centre at its index.

Everything below is float64 arithmetic on those rows: given the rows, the keys are deterministic."""
import numpy as np

KEYS = ("npix", "bkg", "rms", "peak", "snr", "x_peak", "y_peak", "x0", "y0", "flux_sum", "flux", "ra", "dec")


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
