"""Test-time augmentation (`model(img, augment=True)`, ultralytics DetectionModel._predict_augment) on the HIP path against the
torch-CPU restatement of tests/augment_ref.py: the view kernel against torch's own resize / pad, the augmented decode + NMS on
the oracle's raw head outputs, the model call end to end, the tiled path and its pipeline, and the CLI flag."""
import ctypes as C
import json
import os
import numpy as np
import pytest
import torch
from gpu_common import detector, oracle_model, netin_from_chw, assert_same_detections, seeded_weights, ROOT
import augment_ref as AR

pytestmark = pytest.mark.gpu
TOL = 1e-4
CONF, IOU, SOFT, HARD = 0.3, 0.5, 0.3, 0.8


def _prep(name, h=None, w=None):
    from oracle import preprocessing_ref as P
    g = np.load(os.path.join(ROOT, "tests/golden/preproc.npz"))
    img = g["in/" + name]
    if h:
        img = img[:h, :w]
    dp = P.build_pipeline([("zscale", dict(contrasts=[0.25] * 3)), ("minmax", dict(norm_min=0, norm_max=255))])
    return dp(P.to_cube(img))


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= TOL * np.maximum(1.0, np.abs(b)))


@pytest.mark.parametrize("prec", ["fp32", "fp16x3", "fp16"])
@pytest.mark.parametrize("h0,w0,imgsz", [(512, 512, 512), (200, 230, 256), (360, 640, 640)])
def test_view_kernel_matches_torch(prec, h0, w0, imgsz):
    """cy_augment_pack on the letterboxed batch against F.interpolate(bilinear) + F.pad(0.447) of torch (CPU): within 2 fp32 ulp of the
    unit range (the values are in [0, 1]; torch's CPU build rounds its weights differently by up to an ulp), fp16 within one fp16
    rounding; the 4th channel 0; view 0 of the fp16 context = fp16 of the fp32 source."""
    from oracle import yolov8_ref as Y
    det = detector(prec, max_batch=2, max_imgsz=640)
    rng = np.random.default_rng(h0)
    big = _prep("big512")                                                # a real frame, resampled to h0 x w0 (nearest)
    imgs = [rng.uniform(0, 255, (h0, w0, 3)), big[np.arange(h0) * big.shape[0] // h0][:, np.arange(w0) * big.shape[1] // w0]]
    x = torch.cat([Y.preprocess(im, imgsz)[0] for im in imgs])          # [2,3,H,W] fp32, letterboxed
    src = netin_from_chw(x, torch.float32)
    outs = det.augment_pack(src)
    torch.cuda.synchronize()
    ref = AR.views(x)
    for k, (o, r) in enumerate(zip(outs, ref)):
        o = o.float().cpu()
        assert tuple(o.shape) == (2, r.shape[2], r.shape[3], 4), (k, o.shape, r.shape)
        assert torch.all(o[..., 3] == 0)
        r = r.permute(0, 2, 3, 1)
        if prec == "fp16":                                 # one fp16 rounding of a value within 2 fp32 ulp of torch's
            err = (o[..., :3] - r).abs()
            assert torch.all(err <= 2.0 ** -11 * r.abs().clamp(min=2.0 ** -14) + 2 * 2.0 ** -23), (k, float(err.max()))
        else:
            err = (o[..., :3] - r).abs()
            assert float(err.max()) <= 2 * 2.0 ** -23, (k, float(err.max()))
        print("view %d %s %dx%d: max |err| vs torch %.3e" % (k, prec, h0, w0, float(err.max())))
        ch, cw, Hp, Wp = AR.view_geometry(x.shape[2], x.shape[3], AR.SCALES[k])
        pad = float(torch.tensor(0.447, dtype=det.dtype))
        assert torch.all(o[:, ch:, :, :3] == pad) and torch.all(o[:, :, cw:, :3] == pad)


def test_augmented_calls_need_the_context_enabled():
    from caesar_yolo_amd.model import HipDetector
    det = HipDetector(seeded_weights()[0], device=0, precision="fp32", max_batch=1, max_imgsz=64)
    src = torch.zeros((1, 64, 64, 4), dtype=torch.float32, device="cuda")
    v1 = torch.zeros((1, 64, 64, 4), dtype=torch.float32, device="cuda")
    rc = det.lib.cy_augment_pack(det.ctx, det._p(src), 1, 64, 64, None, det._p(v1), det._p(v1), det._stream())
    assert rc == -4                                                        # CY_ERR_STATE
    det.enable_augment()
    det.augment_pack(src)
    torch.cuda.synchronize()
    det.close()


@pytest.mark.parametrize("name,imgsz,conf,iou", [("big512", 512, 0.5, 0.5), ("rag", 256, 0.25, 0.7), ("galaxy", 640, 0.7, 0.5),
                                                 # conf ~ 0 at 640: ~15000 candidates (> 8192: the global-memory sort of nms_kernel)
                                                 ("galaxy", 640, 0.001, 0.7),
                                                 ("big512", 1024, 0.6, 0.5),
                                                 # conf ~ 0 at 1024: more than max_nms = 30000 candidates over the three views (the
                                                 # default capacity holds them all; NMS keeps the top 30000 by score)
                                                 ("big512", 1024, 0.001, 0.7)])
def test_decode_nms_augmented_on_oracle_logits(name, imgsz, conf, iou):
    """cy_decode_nms_augmented on the oracle's raw head outputs of the three views: kept concatenated-index list identical (order
    included), boxes and scores within 1e-4 relative, classes equal."""
    det = detector("fp32", max_imgsz=max(640, imgsz))
    m = oracle_model()
    img = _prep(name)
    d_ref, a_ref, raws, pred = AR.predict_augment(m.net, img, imgsz, conf, iou)
    from oracle import yolov8_ref as Y
    _, (H, W) = Y.preprocess(img, imgsz)
    preds = [r.permute(0, 2, 1).contiguous().cuda() for r in raws]
    d, anch, cnt = det.decode_nms_augmented(preds, H, W, img.shape[0], img.shape[1], conf, iou)
    torch.cuda.synchronize()
    n = int(cnt[0])
    ncand = int((pred[0, 4:].amax(0) > conf).sum())
    if conf < 0.01:
        assert ncand > 8192, ncand
    assert n == d_ref.shape[0]
    assert anch[0, :n].cpu().tolist() == a_ref.tolist()
    assert _close(d[0, :n, :4].cpu().numpy(), d_ref[:, :4].numpy())
    assert _close(d[0, :n, 4].cpu().numpy(), d_ref[:, 4].numpy())
    assert np.array_equal(d[0, :n, 5].cpu().numpy(), d_ref[:, 5].numpy())
    assert det.counters()["cand_overflow_tiles"] == 0


E2E_BOX_PX, E2E_SCORE = 5e-3, 2e-5


def _e2e(y, net, img, imgsz, conf, iou, what):
    from oracle import yolov8_ref as Y
    # move the threshold off any candidate within 1e-5 of it (as test_model_call_end_to_end_fp32)
    for dconf in (0.0, 0.003, -0.003, 0.006, -0.006):
        d_ref, _, _, pred = AR.predict_augment(net, img, imgsz, conf + dconf, iou)
        if int(np.sum(np.abs(pred[0, 4:].amax(0).numpy() - (conf + dconf)) < 1e-5)) == 0:
            conf = conf + dconf
            break
    near = int(np.sum(np.abs(pred[0, 4:].amax(0).numpy() - conf) < 1e-5))
    if near:
        pytest.skip("%d candidates within 1e-5 of the confidence threshold" % near)
    # the feature is visible: the augmented result is not the plain one
    x, hw = Y.preprocess(img, imgsz)
    d_plain = Y.non_max_suppression(Y.decode(net.forward(x), net.level_shapes, net.nc), conf, iou, net.nc)[0][0]
    assert d_plain.shape[0] != d_ref.shape[0] or not torch.equal(Y.scale_boxes(d_plain[:, :4], hw, img.shape[:2]), d_ref[:, :4])
    r = y(img, device="cuda:0", imgsz=imgsz, conf=conf, iou=iou, augment=True)[0]
    xyxy, cf, cl = r.boxes.xyxy.cpu().numpy(), r.boxes.conf.cpu().numpy(), r.boxes.cls.cpu().numpy()
    btol = E2E_BOX_PX * max(1.0, imgsz / 640.0)
    moved = assert_same_detections(xyxy, cf, cl, d_ref[:, :4].numpy(), d_ref[:, 4].numpy(), d_ref[:, 5].numpy(), btol, E2E_SCORE, what)
    berr = float(np.abs(xyxy - d_ref[:, :4].numpy()).max()) if len(cf) and not moved else 0.0
    print("augmented end-to-end %s: %d boxes (plain: %d), max |dbox| = %.3e px, %d moved inside score ties"
          % (what, len(cf), d_plain.shape[0], berr, moved))
    assert len(cf) > 0


@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
@pytest.mark.parametrize("name,imgsz,conf", [("big512", 512, 0.7), ("syn192", 192, 0.7), ("galaxy", 640, 0.7)])
def test_model_call_augmented_end_to_end(name, imgsz, conf, prec):
    from caesar_yolo_amd.model import YOLO
    y = YOLO(seeded_weights()[0], precision=prec, max_batch=2, max_imgsz=640, device=0)
    _e2e(y, oracle_model().net, _prep(name), imgsz, conf, 0.5, "%s %s@%d" % (prec, name, imgsz))


def test_model_call_augmented_yolo11(tmp_path):
    from caesar_yolo_amd import weights as W
    from caesar_yolo_amd.model import YOLO
    from oracle import yolo11_ref as O
    from yolo11_common import seeded_folded
    nc, names = 3, {0: "a", 1: "b", 2: "c"}
    g, wd = seeded_folded("n", nc, cls_bias=-1.5)
    path = str(tmp_path / "y11n.cyw")
    W.write_cyw2(path, g, [(cs, wd[cs.name][0], wd[cs.name][1]) for cs in g.convs], names)
    y = YOLO(path, precision="fp32", max_batch=1, max_imgsz=256, device=0)
    img = np.random.default_rng(3).uniform(0, 255, (200, 230, 3))
    _e2e(y, O.Net11(wd, "n", nc), img, 256, 0.3, 0.5, "yolo11n fp32 200x230@256")


def _mosaic():
    img = np.load(os.path.join(ROOT, "tests/golden/mosaic_c.npz"))["img"].astype(np.float32)
    return img


def _cfg():
    from caesar_yolo_amd import preprocessing as PP
    return PP.DataPreprocessor([PP.ZScaleTransformer([0.25] * 3), PP.MinMaxNormalizer(0, 255)]).program()


def test_predict_tiles_augmented_equals_per_tile_model_call():
    """predict_tiles(augment=True) on a full-size and a ragged shape class = per tile: the device-preprocessed cube through
    YOLO(...)(cube, augment=True), then the IoU merge."""
    from caesar_yolo_amd.model import YOLO
    y = YOLO(seeded_weights()[0], precision="fp32", max_batch=4, max_imgsz=256, device=0)
    det = y.engine()
    img = _mosaic()
    mosaic = det.mosaic_to_device(img)
    cfg = _cfg()
    groups = [[(0, 256, 0, 256), (256, 512, 0, 256), (128, 384, 128, 384)],
              [(644, 900, 0, 132), (0, 256, 568, 700)]]           # 256 x 132 tiles: a ragged class (letterboxed to 256 x 160)
    total, differ = 0, 0
    for coords in groups:
        res = y.predict_tiles(mosaic, coords, cfg, imgsz=256, conf=CONF, iou=IOU, merge_overlap_iou_thr_soft=SOFT,
                              merge_overlap_iou_thr_hard=HARD, augment=True)
        plain = y.predict_tiles(mosaic, coords, cfg, imgsz=256, conf=CONF, iou=IOU, merge_overlap_iou_thr_soft=SOFT,
                                merge_overlap_iou_thr_hard=HARD)
        for (x0, x1, y0, y1), r, p in zip(coords, res, plain):
            planes, st = det.preproc_planes(mosaic, [(x0, y0)], y1 - y0, x1 - x0, cfg)
            assert int(st[0]) == 0 and r is not None
            cube = planes[0].cpu().numpy().transpose(1, 2, 0)
            one = y(cube, imgsz=256, conf=CONF, iou=IOU, augment=True)[0]
            n = len(one.boxes.conf)
            d = torch.zeros((1, 300, 6), dtype=torch.float32, device="cuda")
            if n:
                d[0, :n, :4], d[0, :n, 4], d[0, :n, 5] = one.boxes.xyxy, one.boxes.conf, one.boxes.cls
            out, ocnt, _ = det.iou_merge(d, torch.tensor([n], dtype=torch.int32, device="cuda"), CONF, SOFT, HARD)
            m = int(ocnt[0])
            o = out[0, :m].cpu().numpy()
            assert_same_detections(r.boxes.xyxy.cpu().numpy(), r.boxes.conf.cpu().numpy(), r.boxes.cls.cpu().numpy(),
                                   o[:, :4], o[:, 4], o[:, 5], 5e-3, 2e-5, "tile (%d, %d)" % (x0, y0))
            total += m
            differ += int(len(p.boxes.conf) != m or not torch.equal(p.boxes.xyxy.cpu(), r.boxes.xyxy.cpu()))
    print("predict_tiles(augment=True): %d merged detections; %d tiles differ from the plain call" % (total, differ))
    assert total >= 4


def test_fp16x3_augmented_results_do_not_depend_on_the_batch():
    from caesar_yolo_amd.model import YOLO
    y = YOLO(seeded_weights()[0], precision="fp16x3", max_batch=4, max_imgsz=256, device=0)
    mosaic = y.engine().mosaic_to_device(_mosaic())
    coords = [(0, 256, 0, 256), (256, 512, 0, 256), (128, 384, 128, 384), (600, 856, 400, 656)]
    kw = dict(imgsz=256, conf=CONF, iou=IOU, merge_overlap_iou_thr_soft=SOFT, merge_overlap_iou_thr_hard=HARD, augment=True)
    together = y.predict_tiles(mosaic, coords, _cfg(), **kw)
    n = 0
    for c, t in zip(coords, together):
        a = y.predict_tiles(mosaic, [c], _cfg(), **kw)[0]
        assert torch.equal(a.boxes.xyxy, t.boxes.xyxy) and torch.equal(a.boxes.conf, t.boxes.conf) and torch.equal(a.boxes.cls, t.boxes.cls)
        n += len(t.boxes.conf)
    assert n >= 4


@pytest.mark.parametrize("prec", ["fp16x3", "fp16"])
def test_unflushed_augmented_and_plain_calls(prec):
    """Three unflushed calls -- augmented, plain, augmented -- each equal their flushed standalone results (bit for bit); and
    augment = 0 through cy_detect_tiles_augmented is cy_detect_tiles."""
    from caesar_yolo_amd.model import HipDetector
    det = HipDetector(seeded_weights()[0], device=0, precision=prec, max_batch=8, max_imgsz=256)
    mosaic = det.mosaic_to_device(_mosaic())
    cfg = _cfg()
    seq = [([(64 * i, 40 * (i % 3)) for i in range(5)], True), ([(600, 400), (300, 200), (128, 128)], False),
           ([(10 * i, 300 + 20 * i) for i in range(4)], True)]
    args = (256, 256, 256, cfg, CONF, IOU, SOFT, HARD)

    def alloc(B):
        return (torch.full((B, 300, 6), 7.0, device="cuda"), torch.full((B,), 77, dtype=torch.int32, device="cuda"),
                torch.full((B,), 7, dtype=torch.int32, device="cuda"))
    alone = []
    for xy, aug in seq:
        d, c, s = det.detect_tiles(mosaic, xy, *args, augment=aug)
        torch.cuda.synchronize()
        alone.append((d.cpu().numpy(), c.cpu().numpy(), s.cpu().numpy()))
    outs = [alloc(len(xy)) for xy, _ in seq]
    torch.cuda.synchronize()
    for (xy, aug), o in zip(seq, outs):
        det.detect_tiles(mosaic, xy, *args, out=o, flush=False, augment=aug)
    det.flush()
    torch.cuda.synchronize()
    ndet = 0
    for (d0, c0, s0), (d1, c1, s1) in zip(alone, [(d.cpu().numpy(), c.cpu().numpy(), s.cpu().numpy()) for d, c, s in outs]):
        np.testing.assert_array_equal(c0, c1)
        np.testing.assert_array_equal(s0, s1)
        for b in range(len(c0)):
            np.testing.assert_array_equal(d0[b, :c0[b]], d1[b, :c0[b]])
        ndet += int(c0.sum())
    assert ndet >= 4
    # augment = 0 through the new entry point
    xy = seq[0][0]
    o = alloc(len(xy))
    t = (C.c_int * (2 * len(xy)))(*[int(v) for p in xy for v in p])
    rc = det.lib.cy_detect_tiles_augmented(det.ctx, det._p(mosaic), mosaic.shape[0], mosaic.shape[1], t, len(xy), 256, 256, 256,
                                           C.byref(cfg), CONF, IOU, SOFT, HARD, 0, det._p(o[0]), det._p(o[1]), det._p(o[2]),
                                           det._stream())
    assert rc == 0
    det.flush()
    d, c, s = det.detect_tiles(mosaic, xy, *args)
    torch.cuda.synchronize()
    assert torch.equal(c, o[1]) and torch.equal(s, o[2])
    for b in range(len(xy)):
        assert torch.equal(d[b, :int(c[b])], o[0][b, :int(c[b])])
    det.close()


def test_cli_augment_equals_sfinder(tmp_path, monkeypatch):
    """scripts/run.py --augment on a small tiled run writes the catalog SFinder.run_parallel gives with CONFIG['augment'] = True."""
    import subprocess
    import sys
    from caesar_yolo_amd import utils
    from caesar_yolo_amd.config import CONFIG
    from caesar_yolo_amd.inference import SFinder
    from caesar_yolo_amd.model import YOLO
    from caesar_yolo_amd import preprocessing as PP
    img = np.load(os.path.join(ROOT, "tests/golden/mosaic_b.npz"))["img"][:512, :512]
    path = str(tmp_path / "mosaic_b.fits")
    utils.write_fits_image(path, img)
    (tmp_path / "cli").mkdir()
    (tmp_path / "api").mkdir()
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run.py"), "--image=" + path, "--weights=seeded:l:5",
                        "--preprocessing", "--zscale_stretch", "--normalize_minmax", "--norm_max=255", "--imgsize=256",
                        "--split_img_in_tiles", "--tile_xsize=256", "--tile_ysize=256", "--tile_xstep=0.5", "--tile_ystep=0.5",
                        "--devices=0", "--tile_batch=16", "--scoreThr=0.3", "--augment"], cwd=str(tmp_path / "cli"), env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
    got = json.load(open(tmp_path / "cli" / "catalog_mosaic_b.json"))["sources"]
    monkeypatch.chdir(tmp_path / "api")
    c = dict(CONFIG)
    c.update(image_path=path, preprocess_fcn=PP.DataPreprocessor([PP.ZScaleTransformer([0.25] * 3), PP.MinMaxNormalizer(0, 255)]),
             img_size=256, split_image_in_tiles=True, tile_xsize=256, tile_ysize=256, tile_xstep=0.5, tile_ystep=0.5,
             devices=["0"], tile_batch=16, score_thr=0.3, save_region=True, augment=True)
    sf = SFinder(YOLO("seeded:l:5", precision="fp16x3", max_batch=16, max_imgsz=256), c)
    assert sf.run_parallel() == 0
    ref = json.load(open(tmp_path / "api" / "catalog_mosaic_b.json"))["sources"]
    assert len(got) > 0 and got == ref
    c.update(augment=False)
    sf = SFinder(YOLO("seeded:l:5", precision="fp16x3", max_batch=16, max_imgsz=256), c)
    assert sf.run_parallel() == 0
    plain = json.load(open(tmp_path / "api" / "catalog_mosaic_b.json"))["sources"]
    assert plain != ref
