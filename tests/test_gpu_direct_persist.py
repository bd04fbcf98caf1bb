"""The persistent form of the pixels-direct kernel (conv1x1_direct_kernel<4,2,3,...,PERSIST>, CY_DIRECT_PERSIST) against its
one-tile form, byte for byte.

The persistent form walks several 256 px x 256 ch tiles per workgroup and keeps the request stream running across the tile
boundary; within a tile it does the one-tile form's arithmetic in the same order, so the outputs must be identical.  Agreement of
the one-tile form with float64 is asserted by the layer tests (tests/test_gpu_conv.py, tests/test_gpu_conv_slices.py), so equality
with it is the whole check here.  Every case runs with CY_DIRECT_MIN_BLOCKS=0 (the pixels-direct kernel whatever the launch size),
CY_DIRECT_PERSIST=2 against 0, and CY_DIRECT_PERSIST_GRID=3 unless the case says otherwise, so that every workgroup walks three or
four tiles: the ring phase at a tile's first chunk, the bias buffer and the rebased lane addresses all change from tile to tile."""
import numpy as np
import pytest
import torch
import conv_slices_ref as R
from gpu_common import detector

pytestmark = pytest.mark.gpu
DIRECT_256 = "conv1x1_direct_kernel<4,2>"


def _knobs(monkeypatch, persist, grid=3):
    monkeypatch.setenv("CY_DIRECT_MIN_BLOCKS", "0")
    monkeypatch.setenv("CY_DIRECT_PERSIST", str(persist))
    monkeypatch.setenv("CY_DIRECT_PERSIST_GRID", str(grid))


def _dense(monkeypatch, B, H, W, Cin, Cout, k=1, s=1, res=False, grid=3, seed=0, repeats=2):
    """conv_bn_silu (dense buffers) with the persistent form against the one-tile form."""
    det = detector("fp16", max_batch=4)
    g = torch.Generator().manual_seed(1000 + seed)
    xd = torch.randn((B, H, W, Cin), generator=g).half().cuda()
    Ho, Wo = R.out_hw(H, W, k, s)
    rd = torch.randn((B, Ho, Wo, Cout), generator=g).half().cuda() if res else None
    w = (torch.randn((Cout, Cin, k, k), generator=g) / (Cin * k * k) ** 0.5).numpy()
    b = (torch.randn((Cout,), generator=g) * 0.1).numpy()
    _knobs(monkeypatch, 0, grid)
    ref = det.conv_bn_silu(xd, w, b, k, s, True, rd).clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ref).all()) and float(ref.float().abs().max()) > 0.1
    _knobs(monkeypatch, 2, grid)
    for _ in range(repeats):                      # (the hand-over between tiles rests on counted waits: the same bits every time)
        got = det.conv_bn_silu(xd, w, b, k, s, True, rd)
        torch.cuda.synchronize()
        assert torch.equal(ref.view(torch.int16), got.view(torch.int16)), "%d elements differ" % int((ref != got).sum())


@pytest.mark.parametrize("Cout", [512, 256])
def test_base(Cout, monkeypatch):
    """B = 2 on a 24 x 24 map: M = 1152 = four full pixel tiles and one of 128 px; Cout 512 = two channel tiles per pixel block."""
    _dense(monkeypatch, 2, 24, 24, 256, Cout, seed=Cout)


@pytest.mark.parametrize("Cin", [64, 128, 192, 448, 640])
def test_cin_sweep(Cin, monkeypatch):
    """1, 2, 3, 7 and 10 K chunks: fewer than the request distance, equal to it, equal to the ring, no multiple of the ring (the next
    tile starts at another ring phase), and one of the network's own.  Below three chunks the dispatch keeps the one-tile form
    (tests/test_direct_persist_plan_cpu.py pins that), and the comparison holds trivially."""
    _dense(monkeypatch, 2, 24, 24, Cin, 512, seed=Cin)


@pytest.mark.parametrize("Cout", [200, 328])
def test_ragged_cout(Cout, monkeypatch):
    """Output channels that are no multiple of 64 (nor of 16): the scalar store path, and a second channel tile that is mostly
    empty (328: 72 of its 256 channels)."""
    _dense(monkeypatch, 2, 24, 24, 192, Cout, seed=Cout)


@pytest.mark.parametrize("hw", [(48, 48), (47, 45)])
def test_strided_3x3(hw, monkeypatch):
    """3x3 stride 2, 128 -> 256 channels (18 chunks): 48 x 48 -> 24 x 24 and 47 x 45 -> 24 x 23 (border taps on all four sides, odd
    sizes): the tap cursor and the tap masks are rebased with the lane addresses."""
    _dense(monkeypatch, 2, hw[0], hw[1], 128, 256, k=3, s=2, seed=hw[1])


@pytest.mark.parametrize("k", [1, 3])
def test_residual(k, monkeypatch):
    """The residual loads of the epilogue sit between the next tile's first requests and its later ones."""
    _dense(monkeypatch, 2, 24 * (2 if k == 3 else 1), 24 * (2 if k == 3 else 1), 192, 512 if k == 1 else 256, k=k, s=2 if k == 3 else 1, res=True, seed=7 + k)


@pytest.mark.parametrize("grid", [64, 1])
def test_single_tile_and_single_workgroup(grid, monkeypatch):
    """A grid of at least the tile count (every workgroup exactly one tile: prologue and tail of the one-tile form, the zero
    requests behind it) and a grid of one (one workgroup walks all ten tiles)."""
    _dense(monkeypatch, 2, 24, 24, 320, 512, grid=grid, seed=grid)


def _slices(monkeypatch, make, call):
    det = detector("fp16", max_batch=4)
    outs = []
    for persist in (0, 2, 2):
        _knobs(monkeypatch, persist)
        bufs = make()
        name = call(det, bufs)
        torch.cuda.synchronize()
        assert name.startswith(DIRECT_256), name
        outs.append(bufs["out"].cpu())
    for got in outs[1:]:
        assert torch.equal(outs[0].view(torch.int16), got.view(torch.int16))
    return outs[0]


def test_two_segments(monkeypatch):
    """Segment 0 through the nearest x2 upsample (128 channels stored on 12 x 12) plus 64 channels on 24 x 24, 256 output channels:
    the lane addresses change with the segment inside a tile and back at the tile boundary."""
    g = torch.Generator().manual_seed(12)
    x0 = torch.randn((2, 12, 12, 128), generator=g).half()
    x1 = torch.randn((2, 24, 24, 64), generator=g).half()
    w = (torch.randn((256, 192, 1, 1), generator=g) / 192 ** 0.5).numpy()
    b = (torch.randn((256,), generator=g) * 0.1).numpy()

    def make():
        return dict(in0=x0.cuda(), in1=x1.cuda(), out=torch.zeros((2, 24, 24, 256), dtype=torch.float16).cuda())

    def call(det, d):
        return det.conv_slices(w, b, 1, 1, True, d["in0"], 128, d["out"], up0=True, in1=d["in1"], c1=64)[0]

    out = _slices(monkeypatch, make, call)
    assert float(out.float().abs().max()) > 0.1


@pytest.mark.parametrize("layout", ["slices", "shared", "concat", "upcat"])
def test_channel_slices(layout, monkeypatch):
    """Input, residual and output channel slices inside wider buffers (tests/conv_slices_ref.py): NaN around the input slices, a
    pattern around the output slice that must come back untouched -- checked against the float64 reference and the guards once
    (the persistent form), and byte for byte against the one-tile form."""
    t = R.build("fp16", (2, 24, 24, 256, 512, 1, 1), True, layout, 31)

    def make():
        return {k: getattr(t, k).cuda() for k in ("in0", "in1", "res", "out") if getattr(t, k) is not None}

    def call(det, d):
        return det.conv_slices(t.w.numpy(), t.b.numpy(), 1, 1, t.act, d["in0"], t.c0, d["out"], in0_coff=t.in0_coff, up0=t.up0,
                               in1=d.get("in1"), in1_coff=t.in1_coff, c1=t.c1, res=d["out"] if t.shared else d.get("res"),
                               res_coff=t.res_coff, out_coff=t.out_coff)[0]

    out = _slices(monkeypatch, make, call)
    R.check(t, out, "persistent", 0)


def test_whole_network(monkeypatch):
    """cy_forward on two 64 x 64 tiles: every layer the dispatch gives to the pixels-direct 256-channel tile in its persistent form
    against the one-tile form, head outputs byte-equal."""
    det = detector("fp16", max_batch=4)
    x = torch.rand((2, 64, 64, 4), generator=torch.Generator().manual_seed(5)).half().cuda()
    monkeypatch.setenv("CY_DIRECT_MIN_BLOCKS", "0")
    monkeypatch.setenv("CY_DIRECT_PERSIST_GRID", "3")
    monkeypatch.setenv("CY_DIRECT_PERSIST", "0")
    ref = det.forward(x).clone()
    torch.cuda.synchronize()
    monkeypatch.setenv("CY_DIRECT_PERSIST", "2")
    got = det.forward(x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ref).all())
    assert torch.equal(ref.view(torch.int32), got.view(torch.int32))
