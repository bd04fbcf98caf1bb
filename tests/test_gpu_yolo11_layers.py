"""Op-exact check of the YOLO11 forward pass: every op of the plan that cy_forward interprets (stem, convolutions with their
up0 / in1 / res_coff / out_coff slices, depth-wise convolutions with the attn.pe gather, attention, the in-place pools) against
the teacher-forced float64 walk of tests/plan_ref.py.

The device is the HIP context itself: cy_debug_stop_after ends the pass after n plan ops, cy_debug_read_tensor reads the slices
an op is about to read and the slice it has just written, the prediction buffer is filled with NaN before every pass.  A value is
compared only when the stopped pass ran the op on the launch the whole pass uses (profile(1) / layer_variant on both).  A
failure names the op index, the convolution or op kind, the kernel variant, the position, the value, the reference, the bound
and their ratio.  Ops that ran inside their neighbour's launch are covered through that neighbour, as the walk describes."""
import os
import pytest
import torch
import plan_ref as PR
from test_gpu_layers import _input

pytestmark = pytest.mark.gpu

TINY, WIDE, MID, BIG = (1, 32, 32), (2, 32, 64), (3, 96, 160), (1, 256, 256)
T256, T320 = (1, 512, 512), (1, 640, 512)
SWITCHES = [{"CY_BATCH_INVARIANT": "0"}, {"CY_DIRECT_MIN_BLOCKS": "1"}, {"CY_DIRECT_MIN_BLOCKS": "-1"}, {"CY_STEM_FUSE": "0"},
            {"CY_STEM_FUSE": "2"}, {"CY_FUSE_PW": "0"}, {"CY_NARROW_DIRECT": "0"}, {"CY_HEAD_PAIR": "0"}, {"CY_HEAD_DIRECT": "0"},
            {"CY_STRIP": "2"}, {"CY_WIDE_PERSIST": "0"}, {"CY_WIDE_PERSIST": "2"}, {"CY_ATTN_SLOW": "1"}, {"CY_XCD_ORDER": "0"},
            {"CY_STEM_FUSE": "0", "CY_FUSE_PW": "0"}]
_CACHE = {}


def _model(scale, prec, kind="seeded11"):
    """(graph, folded weights, detector).  kind "seeded11": the benchmark's weights (fp16-valued: the two-pass fp16x3 form);
    "fp32": yolo11_common.seeded_folded (fp32-valued filters: the three-pass form)."""
    from caesar_yolo_amd import weights as W
    from caesar_yolo_amd.model import HipDetector
    wk = (kind, scale)
    if wk not in _CACHE:
        path = os.path.join("/tmp", "cy_test_y11_%s_%s_5.cyw" % (kind, scale))
        if kind == "seeded11":
            g, wd = W.seeded11_folded(scale, 5)
            W.make_seeded11_file(path, scale, 5)
        else:
            from yolo11_common import seeded_folded
            g, wd = seeded_folded(scale, 5)
            W.write_cyw2(path, g, [(cs, wd[cs.name][0], wd[cs.name][1]) for cs in g.convs], {i: "c%d" % i for i in range(5)})
        _CACHE[wk] = (g, wd, path)
    g, wd, path = _CACHE[wk]
    dk = (kind, scale, prec, os.environ.get("CY_X3_PASSES", ""))         # (the form of the fp16x3 filters is decided at load)
    if dk not in _CACHE:
        _CACHE[dk] = HipDetector(path, device=0, precision=prec, max_batch=3, max_imgsz=640)
    return g, wd, _CACHE[dk]


class _HipDevice(object):
    """The device of plan_ref.walk on a HipDetector."""

    def __init__(self, det, g, netin):
        self.det, self.g, self.netin, self.N = det, g, netin, len(g.ops)
        B, H, W, _ = netin.shape
        self.B, self.H, self.W = B, H, W
        self.p = torch.empty((B, det.lib.cy_num_anchors(H, W), 64 + det.nc), dtype=torch.float32, device=netin.device)
        self.log = []

    def run(self, n):
        self.p.fill_(float("nan"))
        self.det.stop_after(n if n < self.N else 0)
        self.det.profile(1)
        self.det.forward(self.netin, out=self.p)
        torch.cuda.synchronize()
        done = self.det.ops_done()
        self.log.append((n, done))
        return done

    def read(self, t, coff, C):
        lev = self.g.tensors[t][0]
        return torch.from_numpy(self.det.read_tensor(t, coff, C, self.B * C * (self.H >> lev) * (self.W >> lev))).double()

    def pred(self):
        return self.p.cpu().double().numpy()

    def variant(self, i):
        o = self.g.ops[i]
        return self.det.layer_variant(PR.op_name(self.g, o)) if o["conv"] >= 0 else PR.KIND[o["kind"]] + "_kernel"

    def close(self):
        self.det.stop_after(0)
        self.det.profile(0)


def _check(scale, prec, shape, kind="seeded11", passes=2, what=""):
    g, wd, det = _model(scale, prec, kind)
    if prec == "fp16x3":
        n2, n3 = det.weight_passes()
        assert (n3 == 0 and n2 > 0) if passes == 2 else (n2 == 0 and n3 > 0), (n2, n3)
    netin, xd = _input(shape, det.dtype)
    dev = _HipDevice(det, g, netin)
    try:
        rep = PR.walk(g, wd, xd, dev, prec, passes)
    finally:
        dev.close()
    N = len(g.ops)
    assert sorted(rep) == list(range(N))
    jumped = sorted(n - 1 for n, done in dev.log if n < N and done == n + 1)
    fused = sorted(i for i, v in rep.items() if not v["materialised"])
    assert fused == jumped, "unmaterialised ops %s, completed-op count jumped at %s" % (fused, jumped)
    r, i = PR.worst(rep)
    kinds = {}
    for v in rep.values():
        if v["materialised"]:
            kinds[v["kind"]] = max(kinds.get(v["kind"], 0.0), v["ratio"])
    print("PLAN yolo11%s %s %s %s: worst ratio %.3f at op %d %s [%s] %s; per kind: %s; covered through their reader: %s; variants: %s" % (
        scale, prec, shape, what, r, i, rep[i]["name"], rep[i]["variant"] or "in its neighbour's launch", rep[i]["pos"],
        " ".join("%s %.3f" % kv for kv in sorted(kinds.items())), [rep[j]["name"] for j in fused],
        "|".join(sorted(set(v["variant"] for v in rep.values() if v["variant"])))))
    bad = PR.failures(rep)
    assert not bad, "\n".join(bad)
    return g, rep


@pytest.mark.parametrize("shape", [TINY, WIDE, MID, BIG])
def test_yolo11l_fp16(shape):
    """(1, 32, 32): one-token attention, 1-pixel maps; MID: 15 tokens, ragged tiles, odd batch; (1, 256, 256): full 16 x 32 patches."""
    _check("l", "fp16", shape)


@pytest.mark.parametrize("scale", ["l", "n"])
@pytest.mark.parametrize("prec", ["fp32", "fp16x3"])
def test_mid_fp32_and_fp16x3(scale, prec):
    _check(scale, prec, MID)


def test_yolo11n_fp16():
    """8 -> 16, 16 -> 8 and 48 -> 64 channel convolutions; the fp32-filter stem; plain bottlenecks whose shortcut is a channel slice."""
    _check("n", "fp16", MID)


def test_yolo11l_fp16x3_full_patches():
    _check("l", "fp16x3", BIG)


def test_attention_256_tokens_fp32():
    """One query per thread of the fast attention kernel."""
    _check("n", "fp32", T256)


def test_attention_320_tokens_fp16():
    """The two-query loop of the fast attention kernel, ragged."""
    _check("n", "fp16", T320)


def test_yolo11m_fp16():
    """C3k blocks everywhere at depth 0.5; fp32-valued filters rounded to fp16 by the context."""
    _check("m", "fp16", MID, kind="fp32")


def test_fp16x3_three_pass_form(monkeypatch):
    monkeypatch.setenv("CY_X3_PASSES", "3")
    _check("l", "fp16x3", MID, kind="fp32", passes=3, what="CY_X3_PASSES=3")


@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: ",".join("%s=%s" % kv for kv in sorted(e.items())))
def test_fp16_switches(env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g, rep = _check("l", "fp16", MID, what=str(env))
    fused = [v["name"] for v in rep.values() if not v["materialised"]]
    if env.get("CY_STEM_FUSE") == "0":
        assert "model.0" not in fused
    if env.get("CY_STEM_FUSE") == "2":
        assert "model.0" in fused
    if "CY_FUSE_PW" in env:
        assert "model.3" not in fused
    if len(env) == 2:
        assert not fused                                  # every op checked directly
    if "CY_HEAD_PAIR" in env:
        assert all(v["variant"] for i, v in rep.items() if g.ops[i]["out"] < 0)


@pytest.mark.parametrize("name,field,value", [("model.10.m.0.ffn.1", "res_coff", 0),        # the shortcut taken from block a of psa, not b
                                              ("model.10.m.0.attn.pe", "p2", 32),          # goff: k | half of v in place of v
                                              ("pool", "in0_coff", 0)])                    # the last SPPF pool reading slice 0, not slice 2
def test_wrong_plan_on_the_device_is_caught_at_its_op_only(tmp_path, name, field, value):
    """The harness on the GPU is not vacuous: a context loaded with a plan that differs from the graph in one (valid) field of
    one op, walked against the unchanged graph, is reported at that op and at no other."""
    import copy
    from caesar_yolo_amd import weights as W
    from caesar_yolo_amd.model import HipDetector
    g, wd = W.seeded11_folded("n", 5)
    k = [i for i, o in enumerate(g.ops) if PR.op_name(g, o) == name][-1]
    bad = copy.deepcopy(g)
    assert bad.ops[k][field] != value
    bad.ops[k][field] = value
    path = str(tmp_path / "bad.cyw")
    W.write_cyw2(path, bad, [(cs, wd[cs.name][0], wd[cs.name][1], torch.ones(cs.cout).numpy()) for cs in g.convs], {i: "c%d" % i for i in range(5)})
    det = HipDetector(path, device=0, precision="fp16", max_batch=3, max_imgsz=160)
    netin, xd = _input(MID, det.dtype)
    dev = _HipDevice(det, g, netin)
    try:
        rep = PR.walk(g, wd, xd, dev, "fp16")
    finally:
        dev.close()
        det.close()
    others = max(v["ratio"] for i, v in rep.items() if i != k and v["materialised"])
    print("PLAN fault %s.%s = %d: op %d ratio %.3g; worst other op %.3f" % (name, field, value, k, rep[k]["ratio"], others))
    assert rep[k]["materialised"] and rep[k]["ratio"] > 1.0
    assert others <= 1.0
