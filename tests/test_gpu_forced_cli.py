"""--forced_fit / --forced_images end to end through scripts/run.py on the 1024 x 1024 synthetic FITS mosaic of
tests/test_gpu_residual_cli.py, tiled and serial (the serial run on a crop), with --fit_blends --bkg_map --residual_map and two FITS
maps written here: the mosaic at 0.55 of its brightness with a frequency and a wider beam, and the mosaic at 0.3 with a frequency
and no beam keywords.
  - with "forced_images" removed and the "forced" / forced_alpha keys stripped from the components, the catalog equals the catalog
    written without the switch byte for byte
  - the "forced" dicts, the alpha keys and "forced_images" equal those of a measure.Chain started on the catalog's boxes with
    forced() called last on uploads of the same arrays (the kernels are deterministic and the host arithmetic is the same code, so
    equal means equal)
  - forced_ms and its companions are in the stats only with the switch
  - the maps are scaled copies, so a clean component's peak on them is that fraction of its peak on the image
  - the serial run crops the maps with the image's own ranges
  - a map of another shape ends the run with an error before anything is written."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_common import ROOT, detector
from test_gpu_islands_cli import COMMON, WCS_CARDS
from test_gpu_residual_cli import TILED, _run, _without, mosaic  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

PLAIN = ["--fit_blends", "--bkg_map", "--residual_map"]
SCALES = (0.55, 0.3)
FREQS = (2.8e9, 5.5e9)


@pytest.fixture(scope="module")
def maps(mosaic):  # noqa: F811
    from caesar_yolo_amd import measure, synth, utils
    d, path, img = mosaic[0], mosaic[1], mosaic[2]
    full = utils.read_fits_image(path)[0]
    full = np.asarray(full, np.float32)
    wide = [(k, v * 2 if k in ("BMAJ", "BMIN") else v) for k, v in synth.FITS_CARDS]
    bare = [(k, v) for k, v in synth.FITS_CARDS if k not in ("BMAJ", "BMIN", "BPA")]
    out = []
    for name, scale, cards, freq in (("hi", SCALES[0], wide, FREQS[0]), ("top", SCALES[1], bare, FREQS[1])):
        p = str(d / (name + ".fits"))
        arr = (full * np.float32(scale)).astype(np.float32)
        utils.write_fits_image(p, arr, cards + WCS_CARDS + [("FREQ", freq)])
        header = utils.read_fits_image(p)[1]
        out.append(dict(tag=name, path=p, host=arr, freq=measure.header_frequency(header), beam_area=measure.header_beam_area(header)))
    assert [m["freq"] for m in out] == list(FREQS) and out[0]["beam_area"] > 0 and out[1]["beam_area"] == 0
    small = str(d / "small.fits")
    utils.write_fits_image(small, np.ascontiguousarray(full[:-1]), synth.FITS_CARDS + WCS_CARDS)
    return out, small


def _direct(sources, img, beam, wcs, origin, cell, others, image_path):
    """The steps from the components on and then forced(), called directly on the catalog's boxes and its own bkg_map / rms_map keys."""
    from caesar_yolo_amd import measure
    det = detector("fp32", max_batch=1, max_imgsz=160)
    dev = det.mosaic_to_device(np.ascontiguousarray(img))
    torch.cuda.synchronize()
    want = _without(sources)
    for s in want:
        for c in s.get("components") or []:
            for k in ("forced",) + measure.FORCED_ALPHA_KEYS:
                c.pop(k, None)
    fm = [dict(tag=m["tag"], path=m["path"], freq=m["freq"], beam_area=m["beam_area"],
               upload=lambda det, a=m["crop"]: det.mosaic_to_device(np.ascontiguousarray(a))) for m in others]
    config = {"bkg_map": True, "bkg_cell": cell, "forced_fit": True, "image_path": image_path}
    chain = measure.Chain(det, dev, want, config, beam, wcs, wcs_origin=origin, forced_maps=fm)
    chain.mesh, chain.ndef = measure.fill_mesh(det.measure_background(dev, cell=cell, k=3.0, niter=3), 64)
    for step in ("deblend", "fit", "blend", "residual", "forced"):
        getattr(chain, step)()
    return chain


def _plain_of(doc, key):
    from caesar_yolo_amd import measure
    out = {k: v for k, v in doc.items() if k != "forced_images"}
    out[key] = [dict(s) for s in doc[key]]
    for s in out[key]:
        if s.get("components"):
            s["components"] = [{k: v for k, v in c.items() if k != "forced" and k not in measure.FORCED_ALPHA_KEYS} for c in s["components"]]
    return json.dumps(out, indent=2, sort_keys=True).encode()


def _check(doc, key, img, beam, wcs, origin, cell, others, image_path, at_least=(1, 0)):
    from caesar_yolo_amd import measure
    chain = _direct(doc[key], img, beam, wcs, origin, cell, others, image_path)
    assert doc["forced_images"] == json.loads(json.dumps(chain.forced_images))
    assert [m["tag"] for m in doc["forced_images"]] == ["self", "hi", "top"] and doc["forced_images"][0]["path"] == image_path
    assert all(m["mesh_ndef"] > 0 for m in doc["forced_images"])
    nforced = clean = 0
    for s, w in zip(doc[key], json.loads(json.dumps(chain.sources))):
        for c, e in zip(s["components"] or [], w["components"] or []):
            assert c["forced"] == e["forced"] and (c["forced"] is None) == (not c["rendered"])
            if c["forced"] is None:
                assert "forced_alpha" not in c
                continue
            nforced += 1
            assert [c[k] for k in measure.FORCED_ALPHA_KEYS] == [e[k] for k in measure.FORCED_ALPHA_KEYS]
            f = c["forced"]
            assert [t["image"] for t in f] == ["self", "hi", "top"] and all(tuple(sorted(t)) == tuple(sorted(measure.FORCED_KEYS)) for t in f)
            if all(t["status"] == 0 for t in f):
                assert f[0]["flux"] is not None and f[1]["flux"] is not None and f[2]["flux"] is None and f[2]["peak"] is not None
                assert f[1]["flux"] == pytest.approx(f[1]["peak"] / f[0]["peak"] * f[0]["flux"] / 4.0, rel=1e-9)      # twice the beam axes: four times the area
                # a scaled copy of the image is the same linear problem with every datum and every weight scaled, so the peak
                # scales with the map; what does not scale exactly are the fp32 roundings of the pixels and of the clipped
                # medians of the two meshes, which move the weights and the subtracted background by a small fraction: a
                # twentieth of the quoted error is far above that and far below what a wrong map, crop or weight would give
                if f[0]["nneigh"] == 0 and f[0]["peak"] > 20 * f[0]["peak_err"]:
                    clean += 1
                    for t, sc in zip(f[1:], SCALES):
                        assert abs(t["peak"] - sc * f[0]["peak"]) <= 0.05 * sc * f[0]["peak_err"], (f[0], t)
                        assert t["peak_err"] == pytest.approx(sc * f[0]["peak_err"], rel=0.02)
                    assert c["forced_alpha_n"] == 2       # the image has no frequency: the two maps carry the slope
    assert nforced >= at_least[0] and clean >= at_least[1], (nforced, clean)
    return chain, nforced, clean


@pytest.fixture(scope="module")
def tiled(mosaic, maps):  # noqa: F811
    d, path = mosaic[0], mosaic[1]
    dirs = {}
    for name, extra in (("plain3", PLAIN), ("forced", PLAIN + ["--forced_images=%s,%s" % (maps[0][0]["path"], maps[0][1]["path"])])):
        (d / name).mkdir()
        _run(["--image=" + path] + TILED + extra, str(d / name))
        dirs[name] = d / name
    return dirs


def test_tiled(mosaic, maps, tiled):  # noqa: F811
    from caesar_yolo_amd import measure
    d, path, img, beam, wcs = mosaic
    raw_plain = open(tiled["plain3"] / "catalog_sky.json", "rb").read()
    doc = json.load(open(tiled["forced"] / "catalog_sky.json"))
    assert set(doc) == {"sources", "forced_images"} and b"forced" not in raw_plain
    assert _plain_of(doc, "sources") == raw_plain
    from caesar_yolo_amd import utils
    others = [dict(m, crop=m["host"]) for m in maps[0]]
    full = np.asarray(utils.read_fits_image(path)[0], np.float32)
    chain, nforced, clean = _check(doc, "sources", full, beam, wcs, (0, 0), 128, others, path, at_least=(3, 1))
    seen = [json.load(open(tiled[k] / "stats.json")) for k in ("plain3", "forced")]
    assert not set(seen[0]) & set(measure.FORCED_STATS) and set(measure.FORCED_STATS) <= set(seen[1])
    assert set(seen[1]) - set(measure.FORCED_STATS) == set(seen[0])
    for k in measure.FORCED_STATS:
        assert seen[1][k] >= 0
        if not k.endswith("_ms"):
            assert seen[1][k] == chain.forced_stats[k], k
    assert seen[1]["forced_maps"] == 3 and seen[1]["forced_jobs"] == 3 * nforced and seen[1]["forced_kernel_ms"] > 0
    print("tiled: %d components forced on 3 maps (%d clean and isolated), %d fitted, %d crowded, %d singular, kernel %.3f ms" % (
        nforced, clean, seen[1]["forced_fitted"], seen[1]["forced_crowded"], seen[1]["forced_singular"], seen[1]["forced_kernel_ms"]))


def test_serial_crop(mosaic, maps, tiled):  # noqa: F811
    d, path, img, beam, wcs = mosaic
    per_tile = {}                                             # the crop = the tile of the tiled run with the most forced components (not the first)
    for s in json.load(open(tiled["forced"] / "catalog_sky.json"))["sources"]:
        for c in s["components"] or []:
            t = (int(c["x"]) // 256, int(c["y"]) // 256)
            if t != (0, 0) and c["forced"] is not None:
                per_tile[t] = per_tile.get(t, 0) + 1
    (tx, ty), _ = max(per_tile.items(), key=lambda kv: (kv[1], kv[0]))
    xmin, xmax, ymin, ymax = tx * 256, tx * 256 + 256, ty * 256, ty * 256 + 256
    args = ["--image=" + path] + COMMON + ["--xmin=%d" % xmin, "--xmax=%d" % xmax, "--ymin=%d" % ymin, "--ymax=%d" % ymax, "--bkg_cell=64"]
    docs = {}
    for name, extra in (("plain3", PLAIN), ("forced", PLAIN + ["--forced_images=%s,%s" % (maps[0][0]["path"], maps[0][1]["path"])])):
        (d / ("serial_" + name)).mkdir()
        _run(args + extra, str(d / ("serial_" + name)))
        docs[name] = open(d / ("serial_" + name) / "out_sky.json", "rb").read()
    doc = json.loads(docs["forced"])
    assert set(doc) == {"image_id", "objs", "forced_images"} and b"forced" not in docs["plain3"]
    assert _plain_of(doc, "objs") == docs["plain3"]
    from caesar_yolo_amd import utils
    full = np.asarray(utils.read_fits_image(path)[0], np.float32)
    others = [dict(m, crop=m["host"][ymin:ymax, xmin:xmax]) for m in maps[0]]
    _, nforced, clean = _check(doc, "objs", np.ascontiguousarray(full[ymin:ymax, xmin:xmax]), beam, wcs, (xmin, ymin), 64, others, path)
    print("serial crop x %d.. y %d..: %d components forced on 3 maps (%d clean and isolated)" % (xmin, ymin, nforced, clean))


def test_a_map_of_another_shape_ends_the_run(mosaic, maps):  # noqa: F811
    d, path = mosaic[0], mosaic[1]
    # the serial run crops a window that lies inside both the image and the shorter map: the whole shapes are what is compared
    for name, args in (("bad_tiled", TILED), ("bad_serial", COMMON), ("bad_crop", COMMON + ["--xmin=0", "--xmax=256", "--ymin=0", "--ymax=256"])):
        (d / name).mkdir()
        env = dict(os.environ, PYTHONPATH=ROOT)
        for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
            env.pop(k, None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run.py"), "--image=" + path] + args + PLAIN + ["--forced_images=" + maps[1]],
                           cwd=str(d / name), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        out = r.stdout.decode(errors="replace")
        assert r.returncode != 0 and "has shape" in out, out[-2000:]
        assert not [f for f in os.listdir(str(d / name)) if f.endswith(".json")]
