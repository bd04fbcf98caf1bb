"""Test-time augmentation restated in torch-CPU fp32: ultralytics 8.x DetectionModel._predict_augment (YOLOv8 and YOLO11 detection)
on the oracle's network, decode, non_max_suppression and scale_boxes (oracle/yolov8_ref.py; any net with the same head layout,
e.g. oracle/yolo11_ref.Net11).  The resize and the pad are torch's own F.interpolate / F.pad: torch is the oracle of the view
kernel.  TEST INFRASTRUCTURE ONLY."""
import math
import torch
import torch.nn.functional as F
from oracle import yolov8_ref as Y

SCALES = (1, 0.83, 0.67)
FLIPS = (None, 3, None)            # 3: left-right
GS = 32                            # max stride
PAD = 0.447


def view_geometry(H, W, s):
    """-> (content h, content w, padded h, padded w) of the view at scale s of an H x W input, in Python float arithmetic."""
    if s == 1:
        return H, W, H, W
    return int(H * s), int(W * s), math.ceil(H * s / GS) * GS, math.ceil(W * s / GS) * GS


def clip_ranges(anchors):
    """_clip_augmented on the three views' anchor counts -> [(lo, hi)] kept per view (g = 1 + 4 + 16)."""
    g = sum(4 ** x for x in range(3))
    a0, a1, a2 = anchors
    return [(0, a0 - (a0 // g)), (0, a1), ((a2 // g) * 16, a2)]


def scale_img(x, s):
    """ultralytics torch_utils.scale_img(img, ratio=s, same_shape=False, gs=32)."""
    if s == 1:
        return x
    h, w = x.shape[2:]
    ch, cw, Hp, Wp = view_geometry(h, w, s)
    x = F.interpolate(x, size=(ch, cw), mode="bilinear", align_corners=False)
    return F.pad(x, [0, Wp - cw, 0, Hp - ch], value=PAD)


def views(x, scales=SCALES, flips=FLIPS):
    """x: letterboxed [B,3,H,W] fp32 -> the network inputs of the views."""
    return [scale_img(x.flip(3) if f else x, s) for s, f in zip(scales, flips)]


@torch.no_grad()
def predict_augment_raw(net, x, scales=SCALES, flips=FLIPS):
    """-> (concatenated decoded prediction [B, 4+nc, A'], raw head outputs of the views [B, 64+nc, A_k]).  With the three standard
    views the stride-32 anchors of view 0 and the stride-8 anchors of view 2 are dropped (_clip_augmented); a single view is
    the plain prediction."""
    raws, shapes = [], []
    for xi in views(x, scales, flips):
        raws.append(net.forward(xi))
        shapes.append(net.level_shapes)
    return decode_views(raws, shapes, net.nc, x.shape[-1], scales, flips), raws


def decode_views(raws, level_shapes, nc, W, scales=SCALES, flips=FLIPS):
    """The views' raw head outputs [B, 64+nc, A_k] (level shapes of each view) -> the concatenated decoded prediction; W: width of
    view 0 (the mirror of the flipped view)."""
    ys = []
    for raw, shp, s, f in zip(raws, level_shapes, scales, flips):
        yi = Y.decode(raw, shp, nc)
        yi[:, :4] /= s                                    # divided by s itself, not by the integer size ratio
        if f == 3:
            yi[:, 0] = W - yi[:, 0]
        ys.append(yi)
    if len(ys) == 3:
        rng = clip_ranges([y.shape[-1] for y in ys])
        ys = [y[..., lo:hi] for y, (lo, hi) in zip(ys, rng)]
    return torch.cat(ys, -1)


@torch.no_grad()
def predict_augment(net, image_hwc, imgsz=640, conf=0.25, iou=0.7, scales=SCALES, flips=FLIPS):
    """The model call `model(image, imgsz=, conf=, iou=, augment=True)`: -> (det [n,6] in image pixels, concatenated index [n],
    raw head outputs of the views, concatenated prediction)."""
    x, hw = Y.preprocess(image_hwc, imgsz)
    pred, raws = predict_augment_raw(net, x, scales, flips)
    det, aidx = Y.non_max_suppression(pred, conf, iou, net.nc)[0]
    det = det.clone()
    det[:, :4] = Y.scale_boxes(det[:, :4], hw, image_hwc.shape[:2])
    return det, aidx, raws, pred
