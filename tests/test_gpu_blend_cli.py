"""--fit_blends end to end through scripts/run.py on the 2048 x 2048 synthetic FITS mosaic of tests/test_gpu_fit_cli.py (same
recipe), tiled and serial, each with and without --bkg_map.  Every component carries measure.BLEND_KEYS; their values equal a
the deblend, fit and blend steps of a measure.Chain started on the written catalog's boxes (the kernels
are deterministic and the host arithmetic is the same code, so equal means equal); a --fit_components run writes the catalog the
--fit_blends run writes with the blend_ keys deleted, byte for byte; and a run without the switch has no blend_ms in its stats."""
import copy
import json

import numpy as np
import pytest
import torch

from gpu_common import detector
from test_gpu_islands_cli import COMMON, N, TILED, WCS_CARDS, _run, _strip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mosaic(tmp_path_factory):
    from caesar_yolo_amd import synth, utils
    from caesar_yolo_amd.wcs import WCS
    d = tmp_path_factory.mktemp("blend_cli")
    img = synth.make_mosaic(n=N, seed=11)
    path = str(d / "sky.fits")
    utils.write_fits_image(path, img, synth.FITS_CARDS + WCS_CARDS)
    _, header = utils.read_fits_image(path)
    c = dict(synth.FITS_CARDS)
    beam = np.pi * c["BMAJ"] * c["BMIN"] / (4 * np.log(2)) / np.abs(c["CDELT1"] * c["CDELT2"])       # SFinder._beam_info
    return d, path, img, beam, WCS(header)


def _no_blend(sources):
    out = copy.deepcopy(sources)
    for s in out:
        for c in s.get("components") or []:
            for k in [k for k in c if k.startswith("blend_")]:
                del c[k]
    return out


def _direct(sources, img, beam, wcs, origin, use_map, k_seed=5.0, k_merge=2.5, k_peak=5.0, conn=8, radius=2, max_iter=64):
    """The component, fit and joint-fit steps called directly on the catalog's boxes, from its own bkg / rms keys."""
    from caesar_yolo_amd import measure
    det = detector("fp32", max_batch=1, max_imgsz=160)
    dev = det.mosaic_to_device(np.ascontiguousarray(img))
    torch.cuda.synchronize()
    want = copy.deepcopy(_strip(sources, measure.COMPONENT_KEYS))
    config = {"bkg_map": use_map, "island_seed_sigma": k_seed, "island_merge_sigma": k_merge, "deblend_peak_sigma": k_peak, "island_conn": conn,
              "deblend_radius": radius, "fit_max_iter": max_iter}
    chain = measure.Chain(det, dev, want, config, beam, wcs, wcs_origin=origin)
    chain.deblend()
    chain.fit()
    chain.blend()
    return want, chain.blend_rows


def _check(sources, want, brows):
    from caesar_yolo_amd import measure
    ncmp = njoint = 0
    for s, w in zip(sources, want):
        assert (s["components"] is None) == (w["components"] is None)
        for c, d in zip(s["components"] or [], w["components"] or []):
            assert set(measure.BLEND_KEYS) <= set(c) and set(measure.FIT_KEYS) <= set(c)
            assert c == d, (c, d)
            ncmp += 1
            njoint += c["blend_status"] in (0, 2)
            if c["blend_status"] == 6:
                assert c["blend_size"] == 1 and all(c[k] == c["fit_" + k[6:]] for k in measure.BLEND_KEYS[5:])
    assert measure.blend_stats(brows)[0] <= njoint
    return ncmp, njoint


@pytest.fixture(scope="module")
def tiled(mosaic):
    d, path = mosaic[0], mosaic[1]
    dirs = {}
    for name, extra in (("fit", ["--fit_components"]), ("blend", ["--fit_blends"]),
                        ("map", ["--fit_blends", "--bkg_map", "--deblend_peak_sigma=4", "--fit_max_iter=40"])):
        (d / name).mkdir()
        _run(["--image=" + path] + TILED + extra, str(d / name))
        dirs[name] = d / name
    return dirs


def test_tiled(mosaic, tiled):
    d, path, img, beam, wcs = mosaic
    raw_fit = open(tiled["fit"] / "catalog_sky.json", "rb").read()
    cat = json.load(open(tiled["blend"] / "catalog_sky.json"))["sources"]
    cat_map = json.load(open(tiled["map"] / "catalog_sky.json"))["sources"]
    assert b"blend_" not in raw_fit and len(cat) > 20
    # without the switch: the same command with --fit_components writes these bytes, every earlier key unchanged
    assert json.dumps({"sources": _no_blend(cat)}, indent=2, sort_keys=True).encode() == raw_fit
    ncmp, njoint = _check(cat, *_direct(cat, img, beam, wcs, (0, 0), False))
    ncmp2, njoint2 = _check(cat_map, *_direct(cat_map, img, beam, wcs, (0, 0), True, k_peak=4.0, max_iter=40))
    print("tiled: %d components, %d in joint fits; with --bkg_map %d, %d" % (ncmp, njoint, ncmp2, njoint2))
    assert ncmp > 20 and ncmp2 > 20 and njoint + njoint2 > 0
    joint = [c for s in cat + cat_map for c in s["components"] or [] if c["blend_status"] == 0]
    assert all(c["blend_flux"] is not None and c["blend_ra"] is not None and c["blend_major"] >= c["blend_minor"] > 0 and c["blend_size"] >= 2
               for c in joint)


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


def test_stats_only_with_the_switch(mosaic, tiled):
    """The stats of a run carry blend_ms only with the switch: SFinder.stats of the command line's own entry, in a process of its
    own (scripts/run.py fills the package's CONFIG in place)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d, path = mosaic[0], mosaic[1]
    env = dict(os.environ)
    env["PYTHONPATH"] = root
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    seen = []
    for name, extra in (("stats_fit", ["--fit_components"]), ("stats_blend", ["--fit_blends"])):
        (d / name).mkdir()
        r = subprocess.run([sys.executable, "-c", _SPY, root, "--image=" + path] + TILED + extra, cwd=str(d / name), env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
        seen.append(json.load(open(d / name / "stats.json")))
    assert "blend_ms" not in seen[0] and not [k for k in seen[0] if k.startswith("blend_")] and "fit_ms" in seen[0]
    assert seen[1]["blend_ms"] >= 0 and seen[1]["blend_kernel_ms"] >= 0 and seen[1]["blend_jobs"] >= 0 and "fit_ms" in seen[1]
    assert seen[1]["blend_niter_max"] <= 64 and seen[1]["blend_over_limit"] >= 0
    assert open(d / "stats_fit" / "catalog_sky.json", "rb").read() == open(tiled["fit"] / "catalog_sky.json", "rb").read()
    assert open(d / "stats_blend" / "catalog_sky.json", "rb").read() == open(tiled["blend"] / "catalog_sky.json", "rb").read()


@pytest.mark.parametrize("bkg_map", [False, True])
def test_serial_crop(mosaic, tiled, bkg_map):
    d, path, img, beam, wcs = mosaic
    ser = d / ("serial_map" if bkg_map else "serial")
    ser.mkdir()
    per_tile = {}                                             # the crop = the tile of the tiled run with the most jointly fitted components
    for s in json.load(open(tiled["blend"] / "catalog_sky.json"))["sources"]:
        t = (int(s["x1"]) // 256, int(s["y1"]) // 256)
        if s["ncomponents"] and not s["merged"] and not s["edge"] and t != (0, 0) and t == (int(s["x2"]) // 256, int(s["y2"]) // 256):
            per_tile[t] = per_tile.get(t, 0) + sum(c["blend_status"] in (0, 2) for c in s["components"]) + 1e-3 * len(s["components"])
    (tx, ty), _ = max(per_tile.items(), key=lambda kv: (kv[1], kv[0]))
    xmin, xmax, ymin, ymax = tx * 256, tx * 256 + 256, ty * 256, ty * 256 + 256
    args = ["--image=" + path] + COMMON + ["--xmin=%d" % xmin, "--xmax=%d" % xmax, "--ymin=%d" % ymin, "--ymax=%d" % ymax]
    extra = ["--island_seed_sigma=4", "--island_merge_sigma=2", "--island_conn=4", "--deblend_radius=1"] + (["--bkg_map", "--bkg_cell=64"] if bkg_map else [])
    _run(args + ["--fit_blends"] + extra, str(ser))
    objs = json.load(open(ser / "out_sky.json"))["objs"]
    (ser / "fit").mkdir()
    _run(args + ["--fit_components"] + extra, str(ser / "fit"))
    plain = json.load(open(ser / "fit" / "out_sky.json"))["objs"]
    assert "blend_" not in json.dumps(plain) and _no_blend(objs) == plain
    crop = np.ascontiguousarray(img[ymin:ymax, xmin:xmax])
    want, brows = _direct(objs, crop, beam, wcs, (xmin, ymin), bkg_map, 4.0, 2.0, 4.0, 4, 1)
    _check(objs, want, brows)
    have = [c for o in objs for c in (o["components"] or []) if c["blend_status"] in (0, 2)]
    near = [c for c in have if abs(c["blend_x"] - c["x_peak"]) <= 3 and abs(c["blend_y"] - c["y_peak"]) <= 3]       # crop-relative pixels, as the peaks
    assert len(near) >= len(have) // 2
