"""--measure_islands end to end through scripts/run.py on the 2048 x 2048 synthetic FITS mosaic of tests/test_gpu_measure_cli.py
(same recipe): without the switch, and with --measure_sources alone, the catalog is what it was; with it every source carries
measure.ISLAND_KEYS beside the others, and they are what the reference (tests/island_ref.py on the host image, thresholds from the
catalog's own bkg and rms) and measure.annotate_islands give.

Comparison rules (tests/test_gpu_islands.py): counts, flags and the bounding box equal; island_flux_sum within 2 m 2^-53 sum|t_i| of
the reference; x_isl = wx0 + Sx / S within (B_Sx + |Sx / S| B_S) / (|S| - B_S) plus the rounding of the division and the addition;
island_flux, island_flux_main, ra_isl, dec_isl are float64 functions of values the catalog itself holds and must equal them exactly
(island_flux_main: of the reference's S_main within its bound).

major, minor, pa against annotate_islands of the reference rows, with a bound carried from those of the sums (shape_bounds):
  a ratio r = X / S moves by at most e_r = (B_X + |r| B_S) / (|S| - B_S);
  a central moment cxx = Sxx / S - (Sx / S)^2 by at most dcxx = e_xx + 2 |mx| e_x + e_x^2, cyy alike, cxy = Sxy / S - mx my by
  e_xy + |mx| e_y + |my| e_x + e_x e_y; each plus 16 eps of the magnitudes subtracted, for the roundings of both sides;
  the eigenvalues of the symmetric 2 x 2 matrix by at most its Frobenius norm dl = sqrt(dcxx^2 + dcyy^2 + 2 dcxy^2) (Weyl), plus
  16 eps (|cxx| + |cyy| + |cxy|) for the roundings of the eigenvalue formula; the clamp at 0 does not widen that;
  major = FWHM sqrt(l1): |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(b), sqrt(|a - b|)), so a zero eigenvalue has a bound too;
  pa = half the angle of the vector (cxx - cyy, 2 cxy), whose length is l1 - l2; a vector moved by dv < its length turns by at most
  asin(dv / length) <= (pi / 2) dv / length.  Where dv >= l1 - l2 (a round island: l1 == l2 up to the error) the angle is not
  determined and only its range is checked.  pa is compared modulo 180 degrees (-90 and 90 are one axis).
Thresholds come from the reference's own formula (island_ref.thresholds) on the catalog's bkg and rms."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import island_ref
from gpu_common import ROOT

pytestmark = pytest.mark.gpu

N = 2048
OLD_KEYS = {"name", "x1", "x2", "y1", "y2", "class_id", "class_name", "score", "edge", "merged"}
WCS_CARDS = [("CTYPE1", "RA---SIN"), ("CTYPE2", "DEC--SIN"), ("CRVAL1", 254.5), ("CRVAL2", -41.25), ("CRPIX1", 1024.5), ("CRPIX2", 1020.0),
             ("CUNIT1", "deg"), ("CUNIT2", "deg")]
COMMON = ["--weights=seeded:l:5", "--preprocessing", "--zscale_stretch", "--normalize_minmax", "--norm_max=255", "--imgsize=256", "--devices=0"]
TILED = COMMON + ["--split_img_in_tiles", "--tile_xsize=256", "--tile_ysize=256", "--tile_xstep=1", "--tile_ystep=1", "--tile_batch=32"]
EPS = 2.0 ** -53


def _run(args, cwd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run.py")] + args, cwd=cwd, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]


@pytest.fixture(scope="module")
def mosaic(tmp_path_factory):
    from caesar_yolo_amd import synth, utils
    from caesar_yolo_amd.wcs import WCS
    d = tmp_path_factory.mktemp("islands_cli")
    img = synth.make_mosaic(n=N, seed=11)
    path = str(d / "sky.fits")
    utils.write_fits_image(path, img, synth.FITS_CARDS + WCS_CARDS)
    _, header = utils.read_fits_image(path)
    host = np.where(np.isfinite(img), img, np.float32(0)).astype(np.float32)
    c = dict(synth.FITS_CARDS)
    beam = np.pi * c["BMAJ"] * c["BMIN"] / (4 * np.log(2)) / np.abs(c["CDELT1"] * c["CDELT2"])       # SFinder._beam_info
    return d, path, host, beam, WCS(header)


@pytest.fixture(scope="module")
def tiled(mosaic):
    """The one-rank tiled run without a switch, with --measure_sources and with --measure_islands."""
    d, path = mosaic[0], mosaic[1]
    dirs = []
    for name, extra in (("off", []), ("on", ["--measure_sources"]), ("isl", ["--measure_islands"])):
        (d / name).mkdir()
        _run(["--image=" + path] + TILED + extra, str(d / name))
        dirs.append(d / name)
    return dirs


def _strip(sources, keys):
    return [{k: v for k, v in s.items() if k not in keys} for s in sources]


def shape_bounds(row, mag, w):
    """(bound on major, on minor, on pa in degrees or None when the axis is not determined) for a reference row, the sums of the
    absolute values of its terms and the keys `w` that annotate_islands derived from it; derivation in the module docstring."""
    from caesar_yolo_amd.measure import FWHM
    m = row[3]
    S, Sx, Sy, Sxx, Syy, Sxy = row[10:16]
    B = [2.0 * m * EPS * v for v in mag[:6]]
    den = abs(S) - B[0]
    e = lambda X, b: (b + abs(X / S) * B[0]) / den
    ex, ey, exx, eyy, exy = e(Sx, B[1]), e(Sy, B[2]), e(Sxx, B[3]), e(Syy, B[4]), e(Sxy, B[5])
    mx, my = abs(Sx / S), abs(Sy / S)
    dcxx = exx + 2 * mx * ex + ex * ex + 16 * EPS * (abs(Sxx / S) + mx * mx)
    dcyy = eyy + 2 * my * ey + ey * ey + 16 * EPS * (abs(Syy / S) + my * my)
    dcxy = exy + mx * ey + my * ex + ex * ey + 16 * EPS * (abs(Sxy / S) + mx * my)
    cxx, cyy, cxy = Sxx / S - (Sx / S) ** 2, Syy / S - (Sy / S) ** 2, Sxy / S - (Sx / S) * (Sy / S)
    dl = np.sqrt(dcxx ** 2 + dcyy ** 2 + 2 * dcxy ** 2) + 16 * EPS * (abs(cxx) + abs(cyy) + abs(cxy))
    out = []
    for k in ("major", "minor"):
        root = w[k] / FWHM                                   # sqrt of the reference's eigenvalue
        out.append(FWHM * (min(dl / root, np.sqrt(dl)) if root > 0 else np.sqrt(dl)) + 4 * EPS * w[k])
    length = (w["major"] / FWHM) ** 2 - (w["minor"] / FWHM) ** 2
    dv = np.hypot(dcxx + dcyy, 2 * dcxy) + 16 * EPS * (abs(cxx) + abs(cyy) + abs(cxy))
    out.append(np.degrees(0.5 * (np.pi / 2) * dv / length) + 4 * EPS * 90 if dv < length else None)
    return out


def _check(sources, host, beam, wcs, origin, k_seed=5.0, k_merge=2.5, conn=8):
    """Every source's island keys against the reference on `host` (the analysed image; origin = where it sits in the FITS frame)."""
    from caesar_yolo_amd import measure
    boxes = measure.boxes_of(sources)
    thr = island_ref.thresholds(np.array([[0.0, 0.0, s["bkg"], s["rms"]] for s in sources], np.float64).reshape(-1, 4), k_seed, k_merge)
    ref, _, mags = island_ref.islands(host, boxes, thr, conn)
    win0 = np.array([measure.box_window(b, host.shape[0], host.shape[1])[:2] for b in boxes], np.float64)
    want = measure.annotate_islands(copy.deepcopy(_strip(sources, measure.ISLAND_KEYS)), ref, win0, beam, wcs, origin)
    worst, shape = 0.0, {"worst": 0.0, "n": 0, "axes": 0}
    for i, (s, w) in enumerate(zip(sources, want)):
        assert set(s) == set(w), (sorted(s), sorted(w))
        for k in ("island_count", "island_npix", "island_npix_main", "island_border", "island_x1", "island_x2", "island_y1", "island_y2"):
            assert s[k] == w[k] and type(s[k]) is type(w[k]), "source %d %s: %r in the catalog, %r from the reference" % (i, k, s[k], w[k])
        if not w["island_count"]:
            assert all(s[k] is None for k in measure.ISLAND_KEYS[4:])
            continue
        m = ref[i, 3]
        b_S, b_Sx, b_Sy = (2.0 * m * EPS * v for v in mags[i, :3])
        assert abs(s["island_flux_sum"] - w["island_flux_sum"]) <= b_S, (i, s["island_flux_sum"], w["island_flux_sum"], b_S)
        assert s["island_flux"] == s["island_flux_sum"] / beam
        assert abs(s["island_flux_main"] * beam - ref[i, 16]) <= 2.0 * m * EPS * mags[i, 6] + 4 * EPS * abs(ref[i, 16])
        S = abs(ref[i, 10])
        if w["x_isl"] is None or S - b_S <= 0:              # S == 0 (or not told from it): no position, no shape
            assert ref[i, 10] == 0 and all(s[k] is None for k in ("x_isl", "y_isl", "ra_isl", "dec_isl", "major", "minor", "pa"))
            continue
        for k, b, w0, j in (("x_isl", b_Sx, win0[i, 0], 11), ("y_isl", b_Sy, win0[i, 1], 12)):
            q = abs(ref[i, j] / ref[i, 10])
            bound = (b + q * b_S) / (S - b_S) + 4 * EPS * (q + abs(w[k]))
            assert abs(s[k] - w[k]) <= bound, "source %d %s: %r in the catalog, %r from the reference, bound %g" % (i, k, s[k], w[k], bound)
            worst = max(worst, abs(s[k] - w[k]) / bound)
        assert s["island_x1"] - 0.5 <= s["x_isl"] <= s["island_x2"] + 0.5 and s["island_y1"] - 0.5 <= s["y_isl"] <= s["island_y2"] + 0.5
        a, d = wcs.wcs_pix2world(s["x_isl"] + origin[0], s["y_isl"] + origin[1], 0)
        assert s["ra_isl"] == float(a) and s["dec_isl"] == float(d)
        assert np.isfinite([s["major"], s["minor"], s["pa"]]).all() and s["major"] >= s["minor"] >= 0 and -90 < s["pa"] <= 90
        b_major, b_minor, b_pa = shape_bounds(ref[i], mags[i], w)
        for k, b in (("major", b_major), ("minor", b_minor)):
            assert abs(s[k] - w[k]) <= b, "source %d %s: %r in the catalog, %r from the reference, bound %g" % (i, k, s[k], w[k], b)
            shape["worst"] = max(shape["worst"], abs(s[k] - w[k]) / b)
        if b_pa is not None:
            turn = abs((s["pa"] - w["pa"] + 90.0) % 180.0 - 90.0)
            assert turn <= b_pa, "source %d pa: %r in the catalog, %r from the reference, bound %g" % (i, s["pa"], w["pa"], b_pa)
            shape["worst"] = max(shape["worst"], turn / b_pa)
            shape["axes"] += 1
        shape["n"] += 1
    print("shape: %d islands compared, %d with a determined axis, largest |diff| / bound %.3g" % (shape["n"], shape["axes"], shape["worst"]))
    assert shape["axes"] * 2 >= shape["n"]                   # most islands are not round to within the error: pa was compared
    return worst


def test_tiled_catalog_with_and_without_the_switches(mosaic, tiled):
    from caesar_yolo_amd import measure
    d, path, host, beam, wcs = mosaic
    off, on, isl = tiled
    raw_off, raw_on = open(off / "catalog_sky.json", "rb").read(), open(on / "catalog_sky.json", "rb").read()
    cat_off, cat_on, cat_isl = json.loads(raw_off), json.loads(raw_on), json.load(open(isl / "catalog_sky.json"))
    assert len(cat_off["sources"]) > 20
    assert all(set(s) == OLD_KEYS for s in cat_off["sources"])                                    # no switch: exactly the old keys
    assert all(set(s) == OLD_KEYS | set(measure.KEYS) for s in cat_on["sources"])                 # --measure_sources: exactly its 13 more
    assert all(set(s) == OLD_KEYS | set(measure.KEYS) | set(measure.ISLAND_KEYS) for s in cat_isl["sources"])
    assert not (OLD_KEYS | set(measure.KEYS)) & set(measure.ISLAND_KEYS)
    # the island keys deleted: the bytes of the --measure_sources catalog; its keys deleted too: the bytes of the plain one
    dump = lambda src: json.dumps({"sources": src}, indent=2, sort_keys=True).encode()
    assert dump(_strip(cat_isl["sources"], measure.ISLAND_KEYS)) == raw_on
    assert dump(_strip(cat_isl["sources"], measure.ISLAND_KEYS + measure.KEYS)) == raw_off
    assert open(isl / "ds9_sky.reg", "rb").read() == open(off / "ds9_sky.reg", "rb").read()
    worst = _check(cat_isl["sources"], host, beam, wcs, (0, 0))
    n_isl = sum(bool(s["island_count"]) for s in cat_isl["sources"])
    assert n_isl > 10 and any(s["island_flux"] for s in cat_isl["sources"])
    print("%d sources, %d with an island; counts equal, largest |x_isl - ref| / bound %.3g" % (len(cat_isl["sources"]), n_isl, worst))


def test_options_and_serial_crop(mosaic, tiled):
    from caesar_yolo_amd import measure
    d, path, host, beam, wcs = mosaic
    ser = d / "serial"
    ser.mkdir()
    # the crop = the 256 x 256 tile of the tiled run that holds the most sources with an island (a serial run of it sees the same pixels)
    per_tile = {}
    for s in json.load(open(tiled[2] / "catalog_sky.json"))["sources"]:
        t = (int(s["x1"]) // 256, int(s["y1"]) // 256)
        if s["island_count"] and not s["merged"] and not s["edge"] and t != (0, 0) and t == (int(s["x2"]) // 256, int(s["y2"]) // 256):
            per_tile[t] = per_tile.get(t, 0) + 1
    (tx, ty), _ = max(per_tile.items(), key=lambda kv: (kv[1], kv[0]))
    xmin, xmax, ymin, ymax = tx * 256, tx * 256 + 256, ty * 256, ty * 256 + 256
    _run(["--image=" + path] + COMMON + ["--xmin=%d" % xmin, "--xmax=%d" % xmax, "--ymin=%d" % ymin, "--ymax=%d" % ymax,
                                         "--measure_islands", "--island_seed_sigma=4", "--island_merge_sigma=2", "--island_conn=4"], str(ser))
    objs = json.load(open(ser / "out_sky.json"))["objs"]
    assert len(objs) > 0 and all(set(measure.KEYS) | set(measure.ISLAND_KEYS) <= set(o) for o in objs)
    # catalog coordinates are relative to the crop; the crop's origin enters the sky position only
    _check(objs, np.ascontiguousarray(host[ymin:ymax, xmin:xmax]), beam, wcs, (xmin, ymin), 4.0, 2.0, 4)
    have = [o for o in objs if o["island_count"]]
    assert have and all(0 <= o["x_isl"] <= xmax - xmin and 0 <= o["island_x1"] <= o["island_x2"] < xmax - xmin for o in have)
    a, dd = wcs.wcs_pix2world(have[0]["x_isl"], have[0]["y_isl"], 0)
    assert (float(a), float(dd)) != (have[0]["ra_isl"], have[0]["dec_isl"])       # the sky position is NOT the crop-relative pixel's
