"""--bkg_map end to end through scripts/run.py on the 2048 x 2048 synthetic FITS mosaic of tests/test_gpu_measure_cli.py (same
recipe).  Without the switch the catalog holds exactly the old keys, with --measure_islands alone exactly its 13 + 18 more, and the
--bkg_map catalogs with the new keys deleted are the bytes of the catalogs without it.  With --bkg_map every source carries
measure.BKG_KEYS, and they are what the reference mesh (tests/bkg_ref.py on the host image), measure.fill_mesh and
measure.sample_mesh give: equal bit for bit, because the mesh is (tests/test_gpu_background.py) and everything after it is float64
arithmetic on the host.  With --measure_islands too, the island keys are those of tests/island_ref.py driven by thresholds formed
from bkg_map / rms_map (the comparison rules of tests/test_gpu_islands_cli.py, whose _check runs here on the map values)."""
import copy
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import bkg_ref
import test_gpu_islands_cli as ICLI
from gpu_common import ROOT

pytestmark = pytest.mark.gpu

N = 2048
OLD_KEYS, COMMON, TILED, _run, _strip = ICLI.OLD_KEYS, ICLI.COMMON, ICLI.TILED, ICLI._run, ICLI._strip


@pytest.fixture(scope="module")
def mosaic(tmp_path_factory):
    from caesar_yolo_amd import synth, utils
    from caesar_yolo_amd.wcs import WCS
    d = tmp_path_factory.mktemp("background_cli")
    img = synth.make_mosaic(n=N, seed=11)
    path = str(d / "sky.fits")
    utils.write_fits_image(path, img, synth.FITS_CARDS + ICLI.WCS_CARDS)
    _, header = utils.read_fits_image(path)
    host = np.where(np.isfinite(img), img, np.float32(0)).astype(np.float32)
    c = dict(synth.FITS_CARDS)
    beam = np.pi * c["BMAJ"] * c["BMIN"] / (4 * np.log(2)) / np.abs(c["CDELT1"] * c["CDELT2"])       # SFinder._beam_info
    return d, path, host, beam, WCS(header)


@pytest.fixture(scope="module")
def tiled(mosaic):
    """One-rank tiled runs: no switch, --measure_sources, --measure_islands, --bkg_map, --bkg_map --measure_islands --save_bkg_maps."""
    d, path = mosaic[0], mosaic[1]
    dirs = {}
    for name, extra in (("off", []), ("on", ["--measure_sources"]), ("isl", ["--measure_islands"]), ("bkg", ["--bkg_map"]),
                        ("both", ["--bkg_map", "--measure_islands", "--save_bkg_maps"])):
        (d / name).mkdir()
        _run(["--image=" + path] + TILED + extra, str(d / name))
        dirs[name] = d / name
    return dirs


def _mesh(host, cell=128, k=3.0, niter=3, min_pix=64):
    from caesar_yolo_amd import measure
    mesh, ndef = measure.fill_mesh(bkg_ref.background(host, cell, k, niter), min_pix)
    assert ndef > 0
    return mesh


def _check_map_keys(sources, mesh, cell):
    """bkg_map, rms_map, snr_map of every source against sample_mesh of the reference mesh at the source's peak pixel (the centre
    of its box when it has no valid pixel): equal."""
    from caesar_yolo_amd import measure
    n_centre = 0
    for i, s in enumerate(sources):
        if s["npix"] > 0:
            x, y = float(s["x_peak"]), float(s["y_peak"])
        else:
            x, y, n_centre = (s["x1"] + s["x2"]) / 2.0, (s["y1"] + s["y2"]) / 2.0, n_centre + 1
        b, r = (float(v) for v in measure.sample_mesh(mesh, cell, x, y))
        assert s["bkg_map"] == b and s["rms_map"] == r, "source %d: bkg_map, rms_map = %r, %r in the catalog, %r, %r from the reference" % (
            i, s["bkg_map"], s["rms_map"], b, r)
        assert s["snr_map"] == ((s["peak"] - b) / r if r != 0.0 else 0.0)
    return n_centre


def _as_ring(sources):
    """The sources with bkg / rms replaced by bkg_map / rms_map and the map keys deleted: what ICLI._check forms its thresholds from."""
    from caesar_yolo_amd import measure
    out = copy.deepcopy(_strip(sources, measure.BKG_KEYS))
    for o, s in zip(out, sources):
        o["bkg"], o["rms"] = s["bkg_map"], s["rms_map"]
    return out


def test_catalogs_without_the_switch_are_what_they_were(mosaic, tiled):
    from caesar_yolo_amd import measure
    d, path, host, beam, wcs = mosaic
    raw = {k: open(v / "catalog_sky.json", "rb").read() for k, v in tiled.items()}
    cat = {k: json.loads(v)["sources"] for k, v in raw.items()}
    assert len(cat["off"]) > 20
    assert len(measure.KEYS) == 13 and len(measure.ISLAND_KEYS) == 18
    assert all(set(s) == OLD_KEYS for s in cat["off"])                                            # no switch: exactly the old keys
    assert all(set(s) == OLD_KEYS | set(measure.KEYS) for s in cat["on"])
    assert all(set(s) == OLD_KEYS | set(measure.KEYS) | set(measure.ISLAND_KEYS) for s in cat["isl"])      # --measure_islands alone: 13 + 18
    assert all(set(s) == OLD_KEYS | set(measure.KEYS) | set(measure.BKG_KEYS) for s in cat["bkg"])         # --bkg_map implies --measure_sources
    assert all(set(s) == OLD_KEYS | set(measure.KEYS) | set(measure.ISLAND_KEYS) | set(measure.BKG_KEYS) for s in cat["both"])
    dump = lambda src: json.dumps({"sources": src}, indent=2, sort_keys=True).encode()
    assert dump(_strip(cat["isl"], measure.ISLAND_KEYS)) == raw["on"] and dump(_strip(cat["on"], measure.KEYS)) == raw["off"]
    # --measure_islands alone still takes its thresholds from the ring: the existing comparison against the reference holds
    ICLI._check(cat["isl"], host, beam, wcs, (0, 0))
    # the map keys deleted: the bytes of the run without --bkg_map (bkg, rms, snr keep their ring values)
    assert dump(_strip(cat["bkg"], measure.BKG_KEYS)) == raw["on"]
    assert dump(_strip(cat["both"], measure.BKG_KEYS + measure.ISLAND_KEYS)) == raw["on"]
    for k in ("isl", "bkg", "both"):
        assert open(tiled[k] / "ds9_sky.reg", "rb").read() == open(tiled["off"] / "ds9_sky.reg", "rb").read()
    assert not os.path.exists(tiled["bkg"] / "bkg_catalog_sky.fits") and not os.path.exists(tiled["isl"] / "bkg_catalog_sky.fits")


def test_map_keys_islands_from_the_map_and_saved_maps(mosaic, tiled):
    from caesar_yolo_amd import measure, utils
    d, path, host, beam, wcs = mosaic
    mesh = _mesh(host)
    bkg = json.load(open(tiled["bkg"] / "catalog_sky.json"))["sources"]
    both = json.load(open(tiled["both"] / "catalog_sky.json"))["sources"]
    _check_map_keys(bkg, mesh, 128)
    _check_map_keys(both, mesh, 128)
    assert any(s["bkg_map"] != s["bkg"] for s in bkg) and all(s["rms_map"] > 0 for s in bkg)
    # the island keys: the reference driven by the map thresholds
    worst = ICLI._check(_as_ring(both), host, beam, wcs, (0, 0))
    isl = json.load(open(tiled["isl"] / "catalog_sky.json"))["sources"]
    assert any(a["island_npix"] != b["island_npix"] for a, b in zip(isl, both))                  # the thresholds did change
    assert sum(bool(s["island_count"]) for s in both) > 10
    # --save_bkg_maps: the expansion of the same mesh, as fp32 FITS images beside the catalog and named after it
    x, y = np.meshgrid(np.arange(N, dtype=np.float64), np.arange(N, dtype=np.float64))
    want = measure.sample_mesh(mesh, 128, x, y).astype(np.float32)
    for plane, tag in enumerate(("bkg_", "rms_")):
        data, hdr = utils.read_fits_image(str(tiled["both"] / (tag + "catalog_sky.fits")))
        assert hdr["BITPIX"] == -32 and data.shape == (N, N)
        assert np.array_equal(np.asarray(data).astype(np.float32).view(np.uint32), np.ascontiguousarray(want[:, :, plane]).view(np.uint32))
    print("%d sources: map keys equal; island keys from the map thresholds, largest |x_isl - ref| / bound %.3g" % (len(both), worst))


def test_options_and_serial_crop(mosaic, tiled):
    from caesar_yolo_amd import measure, utils
    d, path, host, beam, wcs = mosaic
    ser = d / "serial"
    ser.mkdir()
    per_tile = {}
    for s in json.load(open(tiled["both"] / "catalog_sky.json"))["sources"]:
        t = (int(s["x1"]) // 256, int(s["y1"]) // 256)
        if s["island_count"] and not s["merged"] and not s["edge"] and t != (0, 0) and t == (int(s["x2"]) // 256, int(s["y2"]) // 256):
            per_tile[t] = per_tile.get(t, 0) + 1
    (tx, ty), _ = max(per_tile.items(), key=lambda kv: (kv[1], kv[0]))
    xmin, xmax, ymin, ymax = tx * 256, tx * 256 + 256, ty * 256, ty * 256 + 256
    _run(["--image=" + path] + COMMON + ["--xmin=%d" % xmin, "--xmax=%d" % xmax, "--ymin=%d" % ymin, "--ymax=%d" % ymax, "--measure_islands",
                                         "--save_bkg_maps", "--bkg_cell=50", "--bkg_clip_sigma=2.5", "--bkg_clip_iters=5", "--bkg_min_pix=100"], str(ser))
    objs = json.load(open(ser / "out_sky.json"))["objs"]
    assert len(objs) > 0 and all(set(measure.KEYS) | set(measure.ISLAND_KEYS) | set(measure.BKG_KEYS) <= set(o) for o in objs)
    crop = np.ascontiguousarray(host[ymin:ymax, xmin:xmax])
    mesh = _mesh(crop, 50, 2.5, 5, 100)                                    # 6 x 6 cells, the last row and column 6 pixels wide; the corner cell (36 pixels) is filled
    assert mesh.shape == (6, 6, 2)
    # catalog coordinates are relative to the crop, and so is the mesh: the crop's origin enters the sky position only
    _check_map_keys(objs, mesh, 50)
    ICLI._check(_as_ring(objs), crop, beam, wcs, (xmin, ymin))
    x, y = np.meshgrid(np.arange(256, dtype=np.float64), np.arange(256, dtype=np.float64))
    want = measure.sample_mesh(mesh, 50, x, y).astype(np.float32)
    for plane, tag in enumerate(("bkg_", "rms_")):
        data, _ = utils.read_fits_image(str(ser / (tag + "out_sky.fits")))
        assert np.array_equal(np.asarray(data).astype(np.float32).view(np.uint32), np.ascontiguousarray(want[:, :, plane]).view(np.uint32))


def test_two_ranks_on_one_card_give_the_one_rank_catalog(mosaic, tiled):
    """As tests/test_gpu_measure_cli.py: two fresh rank processes through torch.distributed.run, both on GPU 0, the record gather
    over gloo; rank 0 measures the merged catalog, the mesh and the islands on the whole image."""
    d, path, host, beam, wcs = mosaic
    two = d / "two"
    two.mkdir()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "measure_rank_worker.py"), "--image=" + path] + TILED + [
               "--bkg_map", "--measure_islands", "--save_bkg_maps"]
    r = subprocess.run(cmd, cwd=str(two), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    for name in ("catalog_sky.json", "bkg_catalog_sky.fits", "rms_catalog_sky.fits"):
        a, b = open(tiled["both"] / name, "rb").read(), open(two / name, "rb").read()
        assert len(a) > 1000 and a == b, name
