"""--residual_map end to end through scripts/run.py on a 1024 x 1024 synthetic FITS mosaic (the recipe of
tests/test_gpu_islands_cli.py at half the side: the smallest on which the catalog has a joint fit and a duplicated peak; both counts
are asserted, so that nothing here passes emptily), tiled and serial, with --fit_blends and --bkg_map.
  - the --residual_map catalog with the new keys deleted equals the --fit_blends catalog byte for byte
  - the saved FITS maps and the new keys equal the deblend, fit, blend and residual steps of a measure.Chain started on the catalog's boxes
    (the kernels are deterministic and the host arithmetic is the same code, so equal means equal)
  - model + resid + bkg == image on valid pixels to within the two fp32 roundings: |sum - v| <= 2^-24 (|model| + |resid|) (1 + 2^-20)
    + 2^-148, the sum taken in float64
  - residual_ms and its companions are in the stats only with the switch."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_common import ROOT, detector
from test_gpu_islands_cli import COMMON, WCS_CARDS, _strip

pytestmark = pytest.mark.gpu

N = 1024
TILED = COMMON + ["--split_img_in_tiles", "--tile_xsize=256", "--tile_ysize=256", "--tile_xstep=1", "--tile_ystep=1", "--tile_batch=32"]
STAT_KEYS = ("residual_ms", "render_kernel_ms", "residual_kernel_ms", "residual_rendered", "residual_duplicates", "residual_capped")
_SPY = """
import json, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "scripts"))
import run
from caesar_yolo_amd.inference import SFinder
orig = SFinder.run_parallel
def spy(self):
    rc = orig(self)
    json.dump({k: v for k, v in self.stats.items() if isinstance(v, (int, float))}, open("stats.json", "w"))
    return rc
SFinder.run_parallel = spy
sys.exit(run.main(sys.argv[2:]))
"""


def _run(args, cwd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", _SPY, ROOT] + args, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]


@pytest.fixture(scope="module")
def mosaic(tmp_path_factory):
    from caesar_yolo_amd import synth, utils
    from caesar_yolo_amd.wcs import WCS
    d = tmp_path_factory.mktemp("residual_cli")
    img = synth.make_mosaic(n=N, seed=11)
    path = str(d / "sky.fits")
    utils.write_fits_image(path, img, synth.FITS_CARDS + WCS_CARDS)
    _, header = utils.read_fits_image(path)
    c = dict(synth.FITS_CARDS)
    beam = np.pi * c["BMAJ"] * c["BMIN"] / (4 * np.log(2)) / np.abs(c["CDELT1"] * c["CDELT2"])       # SFinder._beam_info
    return d, path, img, beam, WCS(header)


def _without(sources):
    from caesar_yolo_amd import measure
    out = copy.deepcopy(_strip(sources, measure.RESIDUAL_KEYS))
    for s in out:
        for c in s.get("components") or []:
            for k in measure.RENDER_ITEM_KEYS:
                del c[k]
    return out


def _direct(sources, img, beam, wcs, origin, cell):
    """Every step from the components on, called directly on the catalog's boxes and its own bkg_map / rms_map keys.  The boxes are
    in the pixels of `img` (a serial run's catalog is relative to its crop); origin: where `img` lies in the frame of the WCS."""
    from caesar_yolo_amd import measure
    det = detector("fp32", max_batch=1, max_imgsz=160)
    dev = det.mosaic_to_device(np.ascontiguousarray(img))
    torch.cuda.synchronize()
    want = _without(sources)
    chain = measure.Chain(det, dev, want, {"bkg_map": True, "bkg_cell": cell}, beam, wcs, wcs_origin=origin)
    chain.mesh, _ = measure.fill_mesh(det.measure_background(dev, cell=cell, k=3.0, niter=3), 64)      # the mesh alone: bkg_map / rms_map stay the catalog's
    bkg_dev = det.expand_background(chain.mesh, cell, dev.shape, want=("bkg",))[0]
    for step in ("deblend", "fit", "blend", "residual"):
        getattr(chain, step)()
    return want, chain.model.cpu().numpy(), chain.resid.cpu().numpy(), bkg_dev.cpu().numpy(), dev.cpu().numpy(), chain.render_stats


def _check(sources, d, name, img, beam, wcs, origin, cell):
    from caesar_yolo_amd import measure, utils
    want, model, resid, bkg, dev, stats = _direct(sources, img, beam, wcs, origin, cell)
    for s, w in zip(sources, want):
        assert set(measure.RESIDUAL_KEYS) <= set(s)
        for k in measure.RESIDUAL_KEYS:
            assert s[k] == w[k], (k, s[k], w[k])
        for c, e in zip(s["components"] or [], w["components"] or []):
            assert (c["rendered"], c["render_status"]) == (e["rendered"], e["render_status"])
    got_model, got_resid = utils.read_fits_image(str(d / ("model_" + name + ".fits")))[0], utils.read_fits_image(str(d / ("resid_" + name + ".fits")))[0]
    assert np.asarray(got_model, np.float32).tobytes() == model.tobytes() and np.asarray(got_resid, np.float32).tobytes() == resid.tobytes()
    ok = (dev != 0) & np.isfinite(dev)
    total = model.astype(np.float64) + resid.astype(np.float64) + bkg.astype(np.float64)
    bound = 2.0 ** -24 * (np.abs(model) + np.abs(resid)).astype(np.float64) * (1 + 2.0 ** -20) + 2.0 ** -148
    assert ok.any() and (np.abs(total - dev.astype(np.float64))[ok] <= bound[ok]).all() and not resid[~ok].any()
    assert model.max() > 0
    return stats


def _counts(sources):
    comps = [c for s in sources for c in s["components"] or []]
    joint = sum(c["blend_status"] in (0, 2) and c["blend_size"] >= 2 for c in comps)
    usable = [c for c in comps if c["blend_status"] in (0, 2) or c["fit_status"] in (0, 2)]
    return joint, sum(not c["rendered"] for c in usable), sum(c["rendered"] for c in comps)


@pytest.fixture(scope="module")
def tiled(mosaic):
    d, path = mosaic[0], mosaic[1]
    dirs = {}
    for name, extra in (("blend", ["--fit_blends", "--bkg_map"]), ("res", ["--fit_blends", "--bkg_map", "--save_residual_maps"])):
        (d / name).mkdir()
        _run(["--image=" + path] + TILED + extra, str(d / name))
        dirs[name] = d / name
    return dirs


def test_tiled(mosaic, tiled):
    d, path, img, beam, wcs = mosaic
    raw_blend = open(tiled["blend"] / "catalog_sky.json", "rb").read()
    cat = json.load(open(tiled["res"] / "catalog_sky.json"))["sources"]
    assert b"res_" not in raw_blend and b"render" not in raw_blend
    assert json.dumps({"sources": _without(cat)}, indent=2, sort_keys=True).encode() == raw_blend
    joint, dup, rendered = _counts(cat)
    print("tiled %d x %d: %d sources, %d jointly fitted components, %d duplicated peaks, %d rendered" % (N, N, len(cat), joint, dup, rendered))
    assert joint >= 1 and dup >= 1 and rendered >= 10
    stats = _check(cat, tiled["res"], "catalog_sky", img, beam, wcs, (0, 0), 128)
    seen = [json.load(open(tiled[k] / "stats.json")) for k in ("blend", "res")]
    assert not [k for k in seen[0] if k.startswith("residual_") or k.startswith("render_")] and "blend_ms" in seen[0]
    assert all(seen[1][k] >= 0 for k in STAT_KEYS)
    assert (seen[1]["residual_rendered"], seen[1]["residual_duplicates"]) == (rendered, dup) == (stats["rendered"], stats["duplicates"])


def test_serial_crop(mosaic, tiled):
    d, path, img, beam, wcs = mosaic
    ser = d / "serial"
    ser.mkdir()
    per_tile = {}                                             # the crop = the tile of the tiled run with the most rendered components
    for s in json.load(open(tiled["res"] / "catalog_sky.json"))["sources"]:
        t = (int(s["x1"]) // 256, int(s["y1"]) // 256)
        if s["ncomponents"] and t != (0, 0) and t == (int(s["x2"]) // 256, int(s["y2"]) // 256):
            per_tile[t] = per_tile.get(t, 0) + sum(c["rendered"] for c in s["components"])
    (tx, ty), _ = max(per_tile.items(), key=lambda kv: (kv[1], kv[0]))
    xmin, xmax, ymin, ymax = tx * 256, tx * 256 + 256, ty * 256, ty * 256 + 256
    args = ["--image=" + path] + COMMON + ["--xmin=%d" % xmin, "--xmax=%d" % xmax, "--ymin=%d" % ymin, "--ymax=%d" % ymax, "--bkg_map", "--bkg_cell=64"]
    _run(args + ["--fit_blends", "--save_residual_maps"], str(ser))
    objs = json.load(open(ser / "out_sky.json"))["objs"]
    (ser / "blend").mkdir()
    _run(args + ["--fit_blends"], str(ser / "blend"))
    plain = json.load(open(ser / "blend" / "out_sky.json"))["objs"]
    assert "res_" not in json.dumps(plain) and _without(objs) == plain
    crop = np.ascontiguousarray(img[ymin:ymax, xmin:xmax])
    _check(objs, ser, "out_sky", crop, beam, wcs, (xmin, ymin), 64)
    have = [o for o in objs if o["res_npix"]]
    assert have and sum(c["rendered"] for o in objs for c in o["components"] or []) >= 1
    assert all(o["x1"] <= o["res_x_max"] <= o["x2"] and o["y1"] <= o["res_y_max"] <= o["y2"] for o in have)       # the frame of the boxes
