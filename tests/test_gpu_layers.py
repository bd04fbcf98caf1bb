"""Layer-exact forward check: every convolution of cy_forward against the teacher-forced float64 walk of tests/layer_ref.py.

One forward on a random input (uniform in [0, 1], independent per channel, pixel and image), then the walk: the float64
reference of each layer is computed from the device's own input to that layer (`read_conv`, or the prediction rows for the
nine head outputs) and the device's output must lie within the bound derived in layer_ref's docstring, element by element.
A failure names the layer, the kernel variant that ran it, the position, the value, the reference and the bound.
Layers that ran fused (refused by read_conv) are covered through their reader, as the walk describes."""
import numpy as np
import pytest
import torch
import layer_ref as LR
from gpu_common import detector, seeded_weights, netin_from_chw

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 32),        # 16 / 8 / 4 / 2 / 1-pixel maps
          (2, 32, 64),        # a 1 x 2 top map; the stem tile a quarter full
          (3, 96, 160),       # model.1 map 24 x 40: ragged tile columns, three tile rows; 12 x 20, 6 x 10, 3 x 5 below; odd batch
          (2, 64, 416),       # the 104-pixel-wide map of the 16k mosaic's edge tiles
          (1, 256, 256)]      # the patch kernels that need full 16 x 32 patches
MID, BIG = SHAPES[2], SHAPES[4]
SWITCHES = [{"CY_BATCH_INVARIANT": "0"}, {"CY_DIRECT_MIN_BLOCKS": "1"}, {"CY_DIRECT_MIN_BLOCKS": "-1"}, {"CY_STEM_FUSE": "0"},
            {"CY_STEM_FUSE": "2"}, {"CY_STEM_FUSE": "2", "CY_STEM_V": "2"}, {"CY_FUSE_PW": "0"}, {"CY_BNECK_FUSE": "1"},
            {"CY_HEAD_DIRECT": "0"}, {"CY_HEAD_PAIR": "0"}, {"CY_STRIP": "2"}, {"CY_WIDE_PERSIST": "0"}, {"CY_WIDE_PERSIST": "2"}]


def _input(shape, dtype):
    """-> (device NHWC4 input, the same values as float64 [B, 3, H, W]); non-zero on every border, fourth channel zero."""
    B, H, W = shape
    x = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(20260104 + 1000 * B + H + W))
    netin = netin_from_chw(x, dtype)
    seen = netin.cpu().double()
    assert float(seen[..., 3].abs().max()) == 0.0
    xd = seen[..., :3].permute(0, 3, 1, 2).contiguous()
    for edge in (xd[:, :, 0], xd[:, :, -1], xd[:, :, :, 0], xd[:, :, :, -1]):
        assert float(edge.min()) > 0.0
    return netin, xd


def _check(det, wd, prec, shape, passes=2, what=""):
    from caesar_yolo_amd.lib import CyError
    B, H, W = shape
    netin, xd = _input(shape, det.dtype)
    det.profile(1)
    pred = det.forward(netin)
    torch.cuda.synchronize()
    variant = {name: det.layer_variant(name) for name in wd}
    det.profile(0)
    rows = LR.pred_rows(pred.cpu().double(), B, H, W, det.nc)

    def provider(name, ref):
        if name in rows:
            return rows[name]
        try:
            return torch.from_numpy(det.read_conv(name, ref.numel())).double()
        except CyError as e:
            if "not materialised" in str(e) or "ran fused" in str(e):
                return None
            raise
    rep = LR.walk(wd, xd, provider, prec, passes)
    done = {n: v for n, v in rep.items() if v["materialised"]}
    fused = sorted(n for n, v in rep.items() if not v["materialised"])
    r, name = max((v["ratio"], n) for n, v in done.items())
    print("LAYERS %s %s %s: worst ratio %.3f at %s [%s] %s; covered through their reader: %s; variants: %s" % (
        prec, shape, what, r, name, variant[name] or "in its neighbour's launch", done[name]["pos"], "%d layers" % len(fused),
        "|".join(sorted(set(v for v in variant.values() if v)))))
    for n, v in done.items():
        assert v["ratio"] <= 1.0, "%s [%s] at (b, c, row, col) = %s: got %.9g, reference %.9g, bound %.3g (ratio %.3f, K = %d)" % (
            n, variant[n] or "in its neighbour's launch", v["pos"], v["got"], v["ref"], v["bound"], v["ratio"], v["K"])
    return rep


@pytest.mark.parametrize("shape", SHAPES)
def test_fp16_default(shape):
    _check(detector("fp16"), seeded_weights()[3], "fp16", shape)


@pytest.mark.parametrize("shape", [MID, BIG])
@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: ",".join("%s=%s" % kv for kv in sorted(e.items())))
def test_fp16_switches(env, shape, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rep = _check(detector("fp16"), seeded_weights()[3], "fp16", shape, what=str(env))
    if env.get("CY_STEM_FUSE") == "0":
        assert rep["model.0"]["materialised"]
    if env.get("CY_STEM_FUSE") == "2":
        assert not rep["model.0"]["materialised"]
    if "CY_BNECK_FUSE" in env:
        assert not rep["model.2.m.1.cv1"]["materialised"]
    if "CY_FUSE_PW" in env:
        assert rep["model.3"]["materialised"]


@pytest.mark.parametrize("prec,shape,env", [("fp32", MID, {}), ("fp32", SHAPES[0], {}), ("fp32", MID, {"CY_STEM_QUAD": "0"}),
                                            ("fp16x3", MID, {}), ("fp16x3", SHAPES[0], {}), ("fp16x3", BIG, {"CY_STEM_QUAD": "0"})])
def test_fp32_and_fp16x3(prec, shape, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    det = detector(prec)
    passes = 2
    if prec == "fp16x3":
        assert det.weight_passes()[1] == 0           # the seeded filters are fp16 values times a factor: the two-pass form
    _check(det, seeded_weights()[3], prec, shape, passes, what=str(env))


def test_fp16x3_three_pass_form(monkeypatch):
    from caesar_yolo_amd.model import HipDetector
    monkeypatch.setenv("CY_X3_PASSES", "3")
    det = HipDetector(seeded_weights()[0], device=0, precision="fp16x3", max_batch=4, max_imgsz=256)
    try:
        assert det.weight_passes()[0] == 0
        _check(det, seeded_weights()[3], "fp16x3", MID, 3, what="CY_X3_PASSES=3")
    finally:
        det.close()


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("scale", ["n", "s"])
def test_other_scales(scale, prec):
    """yolov8n / yolov8s: channel counts that are no multiples of 64 (16 .. 512), the fp32-filter stem of the fp16 context."""
    _check(detector(prec, scale=scale), seeded_weights(scale)[3], prec, MID, what="yolov8" + scale)


@pytest.mark.parametrize("prec", ["fp16", "fp32", "fp16x3"])
def test_forward_is_repeatable(prec):
    det = detector(prec)
    netin, _ = _input(MID, det.dtype)
    a = det.forward(netin).cpu().numpy().tobytes()
    b = det.forward(netin).cpu().numpy().tobytes()
    assert a == b, "%s: two forward passes over the same input differ" % prec
    assert np.isfinite(np.frombuffer(a, np.float32)).all()
