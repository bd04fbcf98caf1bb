"""The float64 layer walk (tests/layer_ref.py) on the CPU: its topology against the oracle, its bound against a device
emulated in torch (which must stay inside it), and its sensitivity (ten seeded kernel faults, each caught at its own layer)."""
import re
import pytest
import torch
import torch.nn.functional as F
import layer_ref as LR
from gpu_common import seeded_weights

SHAPES = [(1, 32, 32), (2, 32, 64), (3, 96, 160), (2, 64, 416), (1, 256, 256)]      # the shapes of tests/test_gpu_layers.py


def _input(shape, prec, seed=7):
    B, H, W = shape
    x = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(seed + 1000 * B + H + W))
    return x.half().float() if prec == "fp16" else x


@pytest.mark.parametrize("scale", ["l", "n", "s"])
def test_walk_reproduces_the_oracle_graph(scale):
    """Provider = the reference itself: the walk is then a float64 forward pass, and must be the oracle's Net.forward (run on
    float64 copies of the same folded weights) at every tap and at the head output."""
    from oracle import yolov8_ref as Y
    _, sc, names, wd = seeded_weights(scale, 5)
    net = Y.Net(wd, sc, len(names))
    net.w = {k: (w.double(), b.double()) for k, (w, b) in net.w.items()}
    net.taps = {}
    x = _input((2, 64, 96), "fp32").double()
    with torch.no_grad():
        raw = net.forward(x)
    seen = {}

    def provider(name, ref):
        seen[name] = ref
        return ref
    rep = LR.walk(wd, x, provider, "fp32")
    assert set(seen) == set(net.taps) == set(wd) == set(rep)
    for name, ref in net.taps.items():
        got = seen[name]
        m = re.match(r"model\.([2468])\.m\.(\d+)\.cv2$", name)
        if m:             # a shortcut bottleneck: the layer's output is the sum the kernel stores, the oracle's tap the conv alone
            i, j = int(m.group(1)), int(m.group(2))
            prev = seen["model.%d.m.%d.cv2" % (i, j - 1)] if j else seen["model.%d.cv1" % i].chunk(2, 1)[1]
            assert torch.allclose(got - prev, ref, rtol=1e-12, atol=1e-12), name
        else:
            assert torch.equal(got.float(), ref.float()), name
        assert rep[name]["ratio"] == 0.0
    rows = torch.cat([torch.cat((seen["model.22.cv2.%d.2" % l], seen["model.22.cv3.%d.2" % l]), 1).flatten(2) for l in range(3)], 2)
    assert torch.equal(rows.float(), raw.float())
    pr = LR.pred_rows(raw.permute(0, 2, 1).contiguous(), 2, 64, 96, len(names))
    assert torch.equal(pr["model.22.cv3.1.2"], seen["model.22.cv3.1.2"])


def _worst(rep):
    return max((v["ratio"], k) for k, v in rep.items() if v["materialised"])


@pytest.mark.parametrize("prec,fused", [("fp16", ()), ("fp16", ("model.0", "model.3", "model.2.m.0.cv1", "model.2.m.1.cv1", "model.2.m.2.cv1")),
                                        ("fp32", ()), ("fp32", ("model.2.m.0.cv1", "model.4.m.4.cv1", "model.21.m.1.cv1"))])
@pytest.mark.parametrize("shape", SHAPES)
def test_emulated_device_stays_inside_the_bound(shape, prec, fused):
    """A correct device (torch fp32 arithmetic on the context's operands, one rounding to the storage type; with and without the
    layers the fp16 context can run fused) is within the bound at every layer: the bound is not too tight."""
    wd = seeded_weights("l", 5)[3]
    x = _input(shape, prec)
    em = LR.Emulator(wd, prec, fused=fused).run(x)
    rep = LR.walk(wd, x.double(), em.provider, prec)
    r, name = _worst(rep)
    print("emulated %s %s fused %d: worst ratio %.3f at %s %s" % (prec, shape, len(fused), r, name, rep[name]["pos"]))
    assert all(not rep[n]["materialised"] for n in fused)
    for n, v in rep.items():
        assert not v["materialised"] or v["ratio"] <= 1.0, (n, v)


@pytest.mark.parametrize("scale", ["n", "s"])
@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_emulated_device_other_scales(scale, prec):
    wd = seeded_weights(scale, 5)[3]
    x = _input((3, 96, 160), prec)
    em = LR.Emulator(wd, prec).run(x)
    rep = LR.walk(wd, x.double(), em.provider, prec)
    print("emulated %s yolov8%s: worst ratio %.3f at %s" % ((prec, scale) + _worst(rep)))
    for n, v in rep.items():
        assert v["ratio"] <= 1.0, (n, v)


# ---- seeded faults: (layer whose ratio must rise, layers run fused, hook)
def _drop_tap(kh, kw, row=None, col=None):
    def f(stage, t, w, b, s, y):
        w2 = w.clone()
        w2[:, :, kh, kw] = 0
        y2 = F.conv2d(t, w2, b, stride=s, padding=1)
        y = y.clone()
        if row is not None:
            y[:, :, row] = y2[:, :, row]
        else:
            y[..., col] = y2[..., col]
        return y
    return f


def _zero_tail(stage, ts):
    t = ts[1].clone()
    t[:, -8:] = 0
    return [ts[0], t] + list(ts[2:])


def _no_res_last_image(stage, y, res):
    out = y + res
    out[-1] = y[-1]
    return out


def _no_last_bias(stage, t, w, b):
    b = b.clone()
    b[-1] = 0
    return t, w, b


def _unwritten_pixel(stage, y):
    y = y.clone()
    assert y.shape[-1] == 40                           # the second 32-pixel tile of the row holds 8 pixels
    y[1, :, 23, 39] = 0
    return y


def _neighbour_anchor(stage, y):
    y = y.clone()
    y[0, :, 2, 3] = y[0, :, 2, 4]
    return y


FAULTS = {
    "stem input channels 0 and 2 swapped": ("model.0", (), ("model.0", "operands"), lambda st, t, w, b: (t[:, [2, 1, 0]], w, b)),
    "one tap dropped on the last column": ("model.2.m.0.cv1", (), ("model.2.m.0.cv1", "taps"), _drop_tap(1, 0, col=-1)),
    "one tap dropped on the first row": ("model.16", (), ("model.16", "taps"), _drop_tap(2, 1, row=0)),
    "last 8 channels of a concat's second input zeroed": ("model.12.cv1", (), ("model.12.cv1", "cat"), _zero_tail),
    "upsampled input shifted by one pixel": ("model.15.cv1", (), ("model.15.cv1", "up"), lambda st, u: torch.roll(u, 1, 3)),
    "residual omitted for the last image": ("model.4.m.1.cv2", (), ("model.4.m.1.cv2", "res"), _no_res_last_image),
    "bias of the last output channel omitted": ("model.9.cv2", (), ("model.9.cv2", "operands"), _no_last_bias),
    "one output pixel unwritten at the ragged edge of a 32-pixel tile": ("model.1", (), ("model.1", "out"), _unwritten_pixel),
    "fp16 intermediate of a fused pair not rounded": ("model.1", ("model.0",), ("model.0", "keep32"), lambda st: True),
    "head class row taken from the neighbouring anchor": ("model.22.cv3.1.2", (), ("model.22.cv3.1.2", "out"), _neighbour_anchor),
}


@pytest.mark.parametrize("what", list(FAULTS))
def test_seeded_fault_is_caught_at_its_layer_only(what):
    """yolov8n, fp16 emulation, (3, 96, 160): model.1's map is 24 x 40 (a ragged second tile), three images.  The fault pushes its
    layer above 1; teacher forcing keeps every other layer at or below 1."""
    layer, fused, (at, stage), hook = FAULTS[what]
    wd = seeded_weights("n", 5)[3]
    x = _input((3, 96, 160), "fp16")
    hit = []

    def fault(name, st, *args):
        if name == at and st == stage:
            hit.append(1)
            return hook(st, *args)
        return None
    em = LR.Emulator(wd, "fp16", fused=fused, fault=fault).run(x)
    assert hit, "the fault hook never ran"
    rep = LR.walk(wd, x.double(), em.provider, "fp16")
    print("%s: %s ratio %.3g at %s; worst other layer %.3f" % (what, layer, rep[layer]["ratio"], rep[layer]["pos"],
                                                              max(v["ratio"] for n, v in rep.items() if n != layer and v["materialised"])))
    assert rep[layer]["ratio"] > 1.0, "%s not seen: ratio %.3f" % (what, rep[layer]["ratio"])
    for n, v in rep.items():
        if n != layer and v["materialised"]:
            assert v["ratio"] <= 1.0, "%s also raised %s to %.3f" % (what, n, v["ratio"])
