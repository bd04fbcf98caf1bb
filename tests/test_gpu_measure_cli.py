"""--measure_sources end to end through scripts/run.py on a 2048 x 2048 synthetic FITS mosaic with beam and celestial WCS cards:
the switch changes nothing but the added keys, and the added keys are what the numpy reference (tests/measure_ref.py) and
measure.annotate give for the catalog's own boxes on the host image.

Comparison rules (tests/test_gpu_measure.py): npix, bkg, rms, peak, x_peak, y_peak -- and snr, which is float64 arithmetic on
them -- equal; flux_sum within 2 m 2^-53 sum|t_i| of the reference; x0 = swx / sw within the bound that follows from those of swx
and sw, (B_swx + |x0| B_sw) / (sw - B_sw) plus the division's rounding; flux, ra, dec are float64 functions of flux_sum, x0, y0
and must equal those functions of the catalog's own values exactly."""
import copy
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import measure_ref
from gpu_common import ROOT

pytestmark = pytest.mark.gpu

N = 2048
OLD_KEYS = {"name", "x1", "x2", "y1", "y2", "class_id", "class_name", "score", "edge", "merged"}
WCS_CARDS = [("CTYPE1", "RA---SIN"), ("CTYPE2", "DEC--SIN"), ("CRVAL1", 254.5), ("CRVAL2", -41.25), ("CRPIX1", 1024.5), ("CRPIX2", 1020.0),
             ("CUNIT1", "deg"), ("CUNIT2", "deg")]
TILED = ["--weights=seeded:l:5", "--preprocessing", "--zscale_stretch", "--normalize_minmax", "--norm_max=255", "--imgsize=256",
         "--split_img_in_tiles", "--tile_xsize=256", "--tile_ysize=256", "--tile_xstep=1", "--tile_ystep=1", "--devices=0", "--tile_batch=32"]
EPS = 2.0 ** -53


def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    return env


def _run(args, cwd):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run.py")] + args, cwd=cwd, env=_env(), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]


@pytest.fixture(scope="module")
def mosaic(tmp_path_factory):
    from caesar_yolo_amd import synth, utils
    from caesar_yolo_amd.wcs import WCS
    d = tmp_path_factory.mktemp("measure_cli")
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
    """The one-rank tiled run without and with the switch (directories `off` and `on` of the module's scratch directory)."""
    d, path = mosaic[0], mosaic[1]
    off, on = d / "off", d / "on"
    off.mkdir(); on.mkdir()
    _run(["--image=" + path] + TILED, str(off))
    _run(["--image=" + path] + TILED + ["--measure_sources"], str(on))
    return off, on


def _strip(sources):
    from caesar_yolo_amd import measure
    return [{k: v for k, v in s.items() if k not in measure.KEYS} for s in sources]


def _check(sources, host, ring, beam, wcs, origin):
    """Every source's measured keys against the reference on `host` (the analysed image; origin = where it sits in the FITS frame)."""
    from caesar_yolo_amd import measure
    boxes = measure.boxes_of(sources)
    ref, mags = measure_ref.measure(host, boxes, ring)
    want = measure.annotate(copy.deepcopy(_strip(sources)), ref, beam, wcs, origin)
    worst = 0.0
    for i, (s, w) in enumerate(zip(sources, want)):
        assert set(s) == set(w), (sorted(s), sorted(w))
        for k in ("npix", "bkg", "rms", "peak", "snr", "x_peak", "y_peak"):
            assert s[k] == w[k], "source %d %s: %r in the catalog, %r from the reference" % (i, k, s[k], w[k])
        m = ref[i, 0]
        b_sum, b_sw, b_swx, b_swy = (2.0 * m * EPS * v for v in mags[i])
        assert abs(s["flux_sum"] - w["flux_sum"]) <= b_sum, (i, s["flux_sum"], w["flux_sum"], b_sum)
        sw = ref[i, 8]
        if sw > 0 and sw - b_sw > 0:
            for k, b in (("x0", b_swx), ("y0", b_swy)):
                bound = (b + abs(w[k]) * b_sw) / (sw - b_sw) + 4 * EPS * abs(w[k])
                assert abs(s[k] - w[k]) <= bound, "source %d %s: %r in the catalog, %r from the reference, bound %g" % (i, k, s[k], w[k], bound)
                worst = max(worst, abs(s[k] - w[k]) / bound)
        else:
            assert s["x0"] == w["x0"] and s["y0"] == w["y0"]                     # the centre of the box
        assert s["flux"] == s["flux_sum"] / beam
        a, d = wcs.wcs_pix2world(s["x0"] + origin[0], s["y0"] + origin[1], 0)
        assert s["ra"] == float(a) and s["dec"] == float(d)
    return worst


def test_tiled_catalog_with_and_without_the_switch(mosaic, tiled):
    d, path, host, beam, wcs = mosaic
    off, on = tiled
    raw_off = open(off / "catalog_sky.json", "rb").read()
    cat_off, cat_on = json.loads(raw_off), json.load(open(on / "catalog_sky.json"))
    assert len(cat_off["sources"]) > 20
    assert all(set(s) == OLD_KEYS for s in cat_off["sources"])                   # the switch off: exactly today's keys
    from caesar_yolo_amd import measure
    assert all(set(s) == OLD_KEYS | set(measure.KEYS) for s in cat_on["sources"])
    # the new keys deleted: the same bytes (same boxes, classes, scores, flags and order)
    assert json.dumps({"sources": _strip(cat_on["sources"])}, indent=2, sort_keys=True).encode() == raw_off
    assert open(on / "ds9_sky.reg", "rb").read() == open(off / "ds9_sky.reg", "rb").read()
    worst = _check(cat_on["sources"], host, 8, beam, wcs, (0, 0))
    assert sum(s["npix"] > 0 for s in cat_on["sources"]) > 10 and any(s["flux"] for s in cat_on["sources"])
    print("%d sources measured; exact keys equal, largest |x0 - ref| / bound %.3g" % (len(cat_on["sources"]), worst))


def test_ring_option_and_serial_crop(mosaic, tiled):
    d, path, host, beam, wcs = mosaic
    ser = d / "serial"
    ser.mkdir()
    # the crop = the 256 x 256 tile of the tiled run that holds the most sources of its own (a serial run of it sees the same pixels)
    per_tile = {}
    for s in json.load(open(tiled[1] / "catalog_sky.json"))["sources"]:
        t = (int(s["x1"]) // 256, int(s["y1"]) // 256)
        if not s["merged"] and not s["edge"] and t != (0, 0) and t == (int(s["x2"]) // 256, int(s["y2"]) // 256):     # (0, 0): no origin to test
            per_tile[t] = per_tile.get(t, 0) + 1
    (tx, ty), _ = max(per_tile.items(), key=lambda kv: (kv[1], kv[0]))
    xmin, xmax, ymin, ymax = tx * 256, tx * 256 + 256, ty * 256, ty * 256 + 256
    _run(["--image=" + path, "--weights=seeded:l:5", "--preprocessing", "--zscale_stretch", "--normalize_minmax", "--norm_max=255",
          "--imgsize=256", "--devices=0", "--xmin=%d" % xmin, "--xmax=%d" % xmax, "--ymin=%d" % ymin, "--ymax=%d" % ymax,
          "--measure_sources", "--measure_ring=5"], str(ser))
    objs = json.load(open(ser / "out_sky.json"))["objs"]
    assert len(objs) > 0
    from caesar_yolo_amd import measure
    assert all(set(measure.KEYS) <= set(o) for o in objs)
    # catalog coordinates are relative to the crop; the crop's origin enters the sky position only
    _check(objs, np.ascontiguousarray(host[ymin:ymax, xmin:xmax]), 5, beam, wcs, (xmin, ymin))
    assert all(0 <= o["x0"] <= xmax - xmin and 0 <= o["y0"] <= ymax - ymin for o in objs)


def test_two_ranks_on_one_card_give_the_one_rank_catalog(mosaic, tiled):
    """Modelled on tests/test_gpu_multirank.py: two fresh rank processes through torch.distributed.run, both on GPU 0, the record
    gather over gloo; rank 0 measures the merged catalog on the whole image."""
    d, path, host, beam, wcs = mosaic
    one, two = tiled[1], d / "two"
    two.mkdir()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = _env()
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "measure_rank_worker.py"), "--image=" + path] + TILED + ["--measure_sources"]
    r = subprocess.run(cmd, cwd=str(two), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    a, b = open(one / "catalog_sky.json", "rb").read(), open(two / "catalog_sky.json", "rb").read()
    assert len(json.loads(a)["sources"]) > 20
    assert a == b
