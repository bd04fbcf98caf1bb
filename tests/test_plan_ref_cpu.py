"""The float64 plan walk (tests/plan_ref.py) on the CPU: its topology against the oracle (the reference itself as the device), its
bounds against a device emulated in torch on real buffers (which must stay inside them), and its sensitivity (twelve seeded
faults of the emulated device, each caught at its own op and at no other)."""
import pytest
import torch
import plan_ref as PR

SHAPES = [(1, 32, 32), (3, 96, 160), (1, 256, 256)]
_CACHE = {}


def _weights(scale):
    """(graph, folded weights): the benchmark's seeded YOLO11 weights for l and n (fp16-valued), calibrated fp32-valued ones for m."""
    if scale not in _CACHE:
        if scale == "m":
            from yolo11_common import seeded_folded
            _CACHE[scale] = seeded_folded("m", 5)
        else:
            from caesar_yolo_amd import weights as W
            _CACHE[scale] = W.seeded11_folded(scale, 5)
    return _CACHE[scale]


def _input(shape, prec, seed=7):
    B, H, W = shape
    x = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(seed + 1000 * B + H + W))
    return x.half().float() if prec == "fp16" else x


def _op(g, name, nth=0):
    """Index of the op of the named convolution, or of the nth op of a kind ("pool", "attention")."""
    hits = [i for i, o in enumerate(g.ops) if PR.op_name(g, o) == name]
    return hits[nth]


@pytest.mark.parametrize("scale", ["n", "m", "l"])
def test_walk_reproduces_the_oracle_graph(scale):
    """Device = the plan executed in float64 without rounding: the walk is then a float64 forward pass, and must be the oracle's
    Net11.forward (on float64 copies of the same folded weights) at every tap that file records and at the head output.  m has
    C3k blocks everywhere at depth 0.5; n has plain bottlenecks whose shortcut is a slice of the block's own buffer."""
    from oracle import yolo11_ref as O
    g, wd = _weights(scale)
    net = O.Net11(wd, scale, g.nc)
    net.w = {k: (w.double(), b.double()) for k, (w, b) in net.w.items()}
    net.taps = {}
    x = _input((2, 64, 96), "fp32").double()
    with torch.no_grad():
        raw = net.forward(x)
    seen = {}

    def tap(i, y, res):
        seen[PR.op_name(g, g.ops[i])] = y if res is None else y - res      # the oracle taps the convolution before the shortcut add
    dev = PR.PlanEmulator(g, wd, x, "ref")
    rep = PR.walk(g, wd, x, dev, "fp32", tap=tap)
    assert sorted(rep) == list(range(len(g.ops)))
    assert set(net.taps) == set(wd) == set(n for n in seen if n not in ("pool", "attention"))
    for name, ref in net.taps.items():
        assert tuple(seen[name].shape) == tuple(ref.shape), name
        assert torch.allclose(seen[name], ref, rtol=1e-11, atol=1e-11), "%s: %.3e" % (name, float((seen[name] - ref).abs().max()))
    for i, v in rep.items():
        assert v["materialised"] and v["ratio"] < 1e-6, (i, v)          # (the attention reference sums in another order than the emulator)
    pred = torch.from_numpy(dev.pred())
    assert torch.allclose(pred, raw.permute(0, 2, 1), rtol=1e-11, atol=1e-11)


def _fusable(g):
    """The ops the fp16 context can run inside one launch with the op behind them: the stem, and model.3 (a back-to-back pair
    with model.4.cv1 in yolo11l; emulated on yolo11n too)."""
    return (_op(g, "model.0"), _op(g, "model.3"))


@pytest.mark.parametrize("fused", [False, True], ids=["apart", "fused"])
@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("scale", ["n", "l"])
@pytest.mark.parametrize("shape", SHAPES)
def test_emulated_device_stays_inside_the_bound(shape, scale, prec, fused):
    """A correct device (torch fp32 arithmetic on the context's operands, one rounding to the storage type; with and without
    the fusable layers left unmaterialised and the box branches deferred for their head pair) is within the bound at every op:
    the bounds are not too tight."""
    g, wd = _weights(scale)
    x = _input(shape, prec)
    dev = PR.PlanEmulator(g, wd, x, prec, fused=_fusable(g) if fused else (), head_pair=fused)
    rep = PR.walk(g, wd, x.double(), dev, prec)
    r, i = PR.worst(rep)
    um = sorted(j for j, v in rep.items() if not v["materialised"])
    print("emulated yolo11%s %s %s fused %s: worst ratio %.3f at op %d %s %s" % (scale, prec, shape, um, r, i, rep[i]["name"], rep[i]["pos"]))
    assert um == (sorted(_fusable(g)) if fused else [])
    assert not PR.failures(rep), PR.failures(rep)
    assert r <= 1.0


# ---- seeded faults: name -> (graph -> (op index, fault))
def _pc(g):
    return g.tensors[g.ops[_op(g, "model.10.cv1")]["out"]][1] // 2


FAULTS = {
    "out_coff off by 8": lambda g: (_op(g, "model.6.cv1"), ("op", ("out_coff", 8))),
    "res_coff one block off": lambda g: (_op(g, "model.10.m.0.ffn.1"), ("op", ("res_coff", -_pc(g)))),
    "in0 and in1 swapped in an upsample-concat": lambda g: (_op(g, "model.13.cv1"), ("swap_inputs",)),
    "nearest upsample with the wrong parity": lambda g: (_op(g, "model.16.cv1"), ("up_parity",)),
    "wrong goff in attn.pe": lambda g: (_op(g, "model.10.m.1.attn.pe"), ("op", ("p2", -32))),
    "attention without the kd^-0.5 scale": lambda g: (_op(g, "attention", 0), ("no_scale",)),
    "attention reading k where v belongs": lambda g: (_op(g, "attention", 1), ("k_for_v",)),
    "a pool writing the neighbouring slice": lambda g: (_op(g, "pool", 1), ("op", ("out_coff", g.ops[_op(g, "pool", 1)]["c0"]))),
    "one 16x16 tile of one conv from the previous image": lambda g: (_op(g, "model.2.m.0.m.0.cv1"), ("tile_prev_image",)),
    "one output channel's bias dropped": lambda g: (_op(g, "model.9.cv2"), ("no_bias", -1)),
    "an fp16 store rounded twice": lambda g: (_op(g, "model.4.m.0.m.1.cv2"), ("round_twice",)),
    "the second PSA block reading the first block's qkv": lambda g: (_op(g, "attention", 1), ("stale_qkv", _op(g, "attention", 0))),
    "in0_coff off by 8": lambda g: (_op(g, "model.8.m.1.cv2"), ("op", ("in0_coff", -8))),
}


@pytest.mark.parametrize("what", list(FAULTS))
def test_seeded_fault_is_caught_at_its_op_only(what):
    """yolo11l, fp16 emulation, (3, 96, 160): 24 x 40 maps at stride 4, fifteen tokens, three images; the stem and model.3 fused
    into their readers, the box branches deferred.  The buffers start from a finite value (memory an earlier pass left behind).
    The fault pushes its own op above 1; teacher forcing keeps every other op at or below 1."""
    g, wd = _weights("l")
    at, fault = FAULTS[what](g)
    x = _input((3, 96, 160), "fp16")
    dev = PR.PlanEmulator(g, wd, x, "fp16", fused=_fusable(g), head_pair=True, faults={at: fault}, fill=0.5)
    rep = PR.walk(g, wd, x.double(), dev, "fp16")
    assert at in dev.hit, "the fault never ran"
    others = max(v["ratio"] for i, v in rep.items() if i != at and v["materialised"])
    print("%s: op %d %s ratio %.3g at %s; worst other op %.3f" % (what, at, rep[at]["name"], rep[at]["ratio"], rep[at]["pos"], others))
    assert rep[at]["materialised"] and rep[at]["ratio"] > 1.0, "%s not seen: ratio %.3f" % (what, rep[at]["ratio"])
    for i, v in rep.items():
        if i != at and v["materialised"]:
            assert v["ratio"] <= 1.0, "%s also raised op %d %s to %.3f" % (what, i, v["name"], v["ratio"])
