"""Kernel-level parity of the YOLO11 / SPPF operators outside the implicit-GEMM convolution: the depth-wise 3x3 kernel, both
attention kernels (LDS fast form, per-query form) and the 5x5 max pools, through the C-ABI test entries cy_dwconv3x3 /
cy_attention / cy_maxpool5 (the launch functions and argument structs of the forward), against plain torch in float64, in the
fp32, fp16 and fp16x3 contexts.

Every output tensor starts as a NaN sentinel: every element of the written slice must be finite afterwards, and every channel
outside it must still hold the sentinel (bit for bit; in fp16x3, where the caller tensor makes a split / merge round trip, still NaN).

Error model (u = 2^-24, the fp32 unit roundoff; E16 = 2^-11, the fp16 one):
  * fp32 context: the kernels compute in fp32 from the stored values.
  * fp16 context: the inputs are fp16 values (the reference gets the same fp16-rounded values); fp32 arithmetic, one rounding of
    the result to fp16 (<= E16 |y| + 2^-25 per element on top of the fp32-level error).
  * fp16x3 context: the fp32 caller values are split into x_hi + x_lo = x (1 + d), |d| <= 2^-22, absolute 2^-25 where x_lo is an
    fp16 subnormal; the kernels compute in fp32 on hi + lo, and the result is split the same way on the way out.
A max picks one of its inputs, so the pools are bit-exact in every context (fp16x3 inputs are drawn as exact hi + lo pairs)."""
import math
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from gpu_common import detector
from plan_ref import attn_ref as _attn_ref, attn_bound as _attn_bound, dw_bound     # (shared with the plan walk of tests/plan_ref.py)
from caesar_yolo_amd import lib as L

pytestmark = pytest.mark.gpu
PRECS = ["fp32", "fp16", "fp16x3"]
U32, E16 = 2.0 ** -24, 2.0 ** -11


def _dtype(prec):
    return torch.float16 if prec == "fp16" else torch.float32


def _stored(t, prec):
    """What the context holds of host values t: fp16-rounded in the fp16 context, fp32 otherwise (float64 result)."""
    return t.half().double() if prec == "fp16" else t.float().double()


def _sentinel(shape, prec):
    return torch.full(shape, float("nan"), dtype=_dtype(prec), device="cuda")


def _check_slice(got, lo, hi, prec, what):
    """got: the whole caller output tensor (host, [..., ct]); channels [lo, hi) were to be written."""
    inside = got[..., lo:hi]
    assert torch.isfinite(inside).all(), "%s: %d output elements unwritten or not finite" % (what, int((~torch.isfinite(inside)).sum()))
    keep = torch.ones(got.shape[-1], dtype=torch.bool)
    keep[lo:hi] = False
    rest = got[..., keep]
    if prec == "fp16x3":
        assert torch.isnan(rest).all(), "%s: a channel outside the written slice was overwritten" % what
    else:
        iv = torch.int16 if rest.dtype == torch.float16 else torch.int32
        ref = torch.full_like(rest, float("nan"))
        assert torch.equal(rest.view(iv), ref.view(iv)), "%s: a channel outside the written slice was overwritten" % what


def _to_dev(t_nhwc, prec):
    return t_nhwc.contiguous().to(_dtype(prec)).cuda()


# ------------------------------------------------------------------------------------------------ depth-wise 3x3
def _dw_case(prec, B, H, W, C, act, use_res, in_ct=None, in_coff=0, out_ct=None, out_coff=0, res_ct=None, res_coff=0, chmap=(0, 0, 0),
             seed=0, what=""):
    """One cy_dwconv3x3 call against F.conv2d(groups=C) (+SiLU)(+residual) in float64.
    Bound per output element, with A = |b| + sum_taps |x| |w| (+ |r|) and y the float64 result:
      fp32:   b + 9 fused multiply-adds, one rounding each of a partial sum below A: worst case 10 u A, but the roundings are
              independent and their sum stays below 5 u A (the worst element of every case reaches about half of that);
              SiLU (slope <= 1.1), expf, the division and the residual add: 3 u |y|.  Bound 5 u A + 3 u |y|;
      fp16x3: + the split of x and r (x (1 + d), |d| <= 4 u; absolute 2^-25 sum |w| + 2^-25) and of the result (4 u |y| + 2^-25),
              again as independent roundings: 7 u A + 5 u |y| + 2^-25 (sum |w| + 2);
      fp16:   fp32-level error with the hardware exp2 / rcp SiLU (5 u A + 5 u |y|), then one fp16 rounding: + E16 |y| + 2^-25.
    (plan_ref.dw_bound.)  The test asserts max(err / bound) <= 1 and prints it."""
    in_ct = in_ct or C
    out_ct = out_ct or C
    res_ct = res_ct or C
    det = detector(prec)
    g = torch.Generator().manual_seed(seed)
    xin = _stored(torch.randn((B, H, W, in_ct), generator=g), prec)
    w = torch.randn((C, 1, 3, 3), generator=g) / 3.0
    b = torch.randn((C,), generator=g) * 0.1
    blk, gstride, goff = chmap
    cidx = torch.arange(C)
    src = in_coff + ((cidx // blk) * gstride + goff + cidx % blk if blk else cidx)
    x = xin[..., src].permute(0, 3, 1, 2)
    y = F.conv2d(x, w.double(), b.double(), padding=1, groups=C)
    A = F.conv2d(x.abs(), w.double().abs(), b.double().abs(), padding=1, groups=C)
    if act:
        y = F.silu(y)
    res = rin = None
    if use_res:
        rin = _stored(torch.randn((B, H, W, res_ct), generator=g), prec)
        r = rin[..., res_coff:res_coff + C].permute(0, 3, 1, 2)
        y = y + r
        A = A + r.abs()
        res = _to_dev(rin, prec)
    out = _sentinel((B, H, W, out_ct), prec)
    det.dwconv3x3(_to_dev(xin, prec), C, w.numpy(), b.numpy(), out, in_coff=in_coff, out_coff=out_coff, act=act, res=res,
                  res_coff=res_coff, chmap=chmap)
    torch.cuda.synchronize()
    got_all = out.cpu()
    _check_slice(got_all, out_coff, out_coff + C, prec, what)
    got = got_all[..., out_coff:out_coff + C].double().permute(0, 3, 1, 2)
    bound = dw_bound(prec, A, y, w.double().abs().sum((1, 2, 3)).view(1, C, 1, 1))
    err = (got - y).abs()
    ratio = float((err / bound).max())
    print("dw %s %s: max abs err %.3e, max err / bound %.3f" % (prec, what, float(err.max()), ratio))
    assert ratio <= 1.0, "%s %s: max err / bound %.3f (max abs err %.3e)" % (prec, what, ratio, float(err.max()))
    return got_all


DW_MAPS = [(h, w) for h in (1, 2, 5, 16) for w in (1, 2, 3, 4, 5, 7, 8, 33, 64)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("hw", DW_MAPS, ids=["%dx%d" % m for m in DW_MAPS])
def test_dwconv_map_edges(prec, hw):
    """Widths around and below DW_PX = 4 (the pixels one thread owns), one-row maps, maps narrower than the 3x3 window: the
    clamped loads must never let a border tap into the sum.  Batch, channel count, SiLU and residual cycle over the maps."""
    H, W = hw
    i = DW_MAPS.index(hw)
    B, C = (1, 3)[i % 2], (8, 24, 64, 256)[(i // 2) % 4]
    act, use_res = bool(i % 3 != 1), bool((i // 3) % 2)
    _dw_case(prec, B, H, W, C, act, use_res, seed=100 + i, what="B%d %dx%d C%d act%d res%d" % (B, H, W, C, act, use_res))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("C", [8, 24, 64, 256])
@pytest.mark.parametrize("act,use_res", [(True, False), (False, True), (True, True), (False, False)])
def test_dwconv_channel_slices(prec, C, act, use_res):
    """Input, output and residual as channel slices of wider tensors (ct > C, coff != 0)."""
    _dw_case(prec, 3, 5, 7, C, act, use_res, in_ct=C + 16, in_coff=8, out_ct=C + 24, out_coff=16, res_ct=C + 8, res_coff=8,
             seed=C * 4 + 2 * act + use_res, what="slices C%d act%d res%d" % (C, act, use_res))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("heads,H,W", [(1, 8, 6), (2, 5, 7), (4, 16, 16)])
def test_dwconv_pe_channel_map(prec, heads, H, W):
    """The C2PSA positional-encoding conv as the plan runs it: v read in place out of the qkv tensor through blk = hd,
    gstride = 2 kd + hd, goff = 2 kd (kd 32, hd 64), no activation, the attention output as the residual."""
    kd, hd = 32, 64
    C = heads * hd
    _dw_case(prec, 2, H, W, C, False, True, in_ct=heads * (2 * kd + hd), out_ct=C, res_ct=C, chmap=(hd, 2 * kd + hd, 2 * kd),
             seed=heads * 7 + H, what="pe heads%d %dx%d" % (heads, H, W))


@pytest.mark.parametrize("prec", PRECS)
def test_dwconv_xcd_order_is_bit_identical(prec, monkeypatch):
    """CY_XCD_ORDER=0 / 1 (workgroups in launch order / XCD-contiguous order) give the same bits."""
    outs = []
    for v in ("0", "1"):
        monkeypatch.setenv("CY_XCD_ORDER", v)
        outs.append(_dw_case(prec, 3, 40, 37, 64, True, True, in_ct=80, in_coff=8, out_ct=72, out_coff=8, seed=7, what="xcd%s" % v))
    iv = torch.int16 if prec == "fp16" else torch.int32
    assert torch.equal(outs[0].view(iv), outs[1].view(iv))


# ------------------------------------------------------------------------------------------------ attention
def _attn_inputs(regime, B, N, heads, kd, hd, ct, coff, g):
    """qkv [B, N, ct] float64 with the per-head blocks [q | k | v] from channel coff on."""
    qkv = torch.randn((B, N, ct), generator=g, dtype=torch.float64)
    per = 2 * kd + hd
    for h in range(heads):
        o = coff + h * per
        if regime == "large":            # scores spanning about +-30: the running maximum moves and the sums rescale many times
            qkv[..., o:o + kd] *= 30.0 / 4.0
        elif regime == "rising":         # every query's scores rise along the keys, from 0 to 60..120: a new maximum at every step,
            u = torch.randn((kd,), generator=g, dtype=torch.float64)    # and exp(score) beyond the fp32 range (exp(88.7)) without it
            u /= u.norm()
            t = torch.arange(N, dtype=torch.float64) / max(N - 1, 1)
            qkv[..., o:o + kd] = u * (1.0 + torch.rand((B, N, 1), generator=g, dtype=torch.float64)) * 4.0
            qkv[..., o + kd:o + 2 * kd] = u * t.view(1, N, 1) * 15.0 * math.sqrt(kd)
        elif regime == "equal":          # every key the same: all scores equal, the output is the mean of v
            qkv[..., o + kd:o + 2 * kd] = qkv[:, :1, o + kd:o + 2 * kd]
    return qkv


def _attn_case(prec, B, N, heads, regime="random", kd=32, hd=64, coff=0, extra=0, out_coff=0, out_extra=0, slow=False, rows=None,
               seed=0, monkeypatch=None, what=""):
    """One cy_attention call (CY_ATTN_SLOW=1: the per-query kernel) against _attn_ref; rows: compare these query rows only."""
    monkeypatch.setenv("CY_ATTN_SLOW", "1" if slow else "0")
    det = detector(prec)
    g = torch.Generator().manual_seed(seed)
    ct = coff + heads * (2 * kd + hd) + extra
    qkv = _stored(_attn_inputs(regime, B, N, heads, kd, hd, ct, coff, g), prec)
    out_ct = out_coff + heads * hd + out_extra
    out = _sentinel((B, N, out_ct), prec)
    det.attention(qkv.to(_dtype(prec)).cuda(), heads, kd, hd, out, coff=coff, out_coff=out_coff)
    torch.cuda.synchronize()
    got_all = out.cpu()
    _check_slice(got_all, out_coff, out_coff + heads * hd, prec, what)
    y, smax, R = _attn_ref(qkv, heads, kd, hd, coff, rows)
    got = got_all[..., out_coff:out_coff + heads * hd].double()
    if rows is not None:
        got = got[:, rows]
    per = 2 * kd + hd
    vmax = max(float(qkv[..., coff + h * per + 2 * kd:coff + (h + 1) * per].abs().max()) for h in range(heads))
    bound = _attn_bound(prec, y, vmax, R)
    err = (got - y).abs()
    ratio = float((err / bound).max())
    fast = not slow and kd == 32 and hd == 64 and N * (kd + hd) * 4 <= 160 * 1024
    print("attn %s %s %s: max |score| %.1f, half spread %.1f, max abs err %.3e, max err / bound %.3f" % (
        prec, "fast" if fast else "per-query", what, smax, R, float(err.max()), ratio))
    assert ratio <= 1.0, "%s %s: max err / bound %.3f (max abs err %.3e)" % (prec, what, ratio, float(err.max()))
    return got_all


ATTN_N = [1, 2, 48, 63, 64, 65, 255, 256, 257, 320, 400, 426, 427, 1024]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", ATTN_N)
def test_attention_token_counts(prec, N, monkeypatch):
    """Both sides of the fast kernel's 256-query loop (one query per thread up to 256, two from 257: 400 = the 640-px tile) and of
    its 160 KiB LDS limit (426 tokens fast, 427 per-query); every case also through the per-query kernel (CY_ATTN_SLOW=1).  qkv
    and output are channel slices of wider tensors; heads and batch cycle over N."""
    i = ATTN_N.index(N)
    heads, B = (1, 2, 4)[i % 3], (1, 3)[(i // 3) % 2]
    if N >= 1024:
        B = 1
    for slow in (False, True):
        _attn_case(prec, B, N, heads, coff=8, extra=16, out_coff=8, out_extra=8, slow=slow, seed=N, monkeypatch=monkeypatch,
                   what="B%d N%d heads%d" % (B, N, heads))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("regime", ["large", "rising", "equal"])
@pytest.mark.parametrize("N", [48, 257, 400, 427])
def test_attention_score_regimes(prec, regime, N, monkeypatch):
    """Scores spanning about +-30 (the online softmax rescales many times), scores rising along the keys to 60..120 (a new maximum
    at every key; exp without the maximum subtracted overflows) and all-equal scores, through both kernels."""
    for slow in (False, True):
        _attn_case(prec, 2, N, 2, regime=regime, slow=slow, seed=N + len(regime), monkeypatch=monkeypatch,
                   what="%s N%d" % (regime, N))


@pytest.mark.parametrize("prec", PRECS)
def test_attention_generic_head_shape(prec, monkeypatch):
    """kd 64 / hd 128 (only the per-query kernel takes head shapes other than 32 / 64): two output channels per lane."""
    _attn_case(prec, 2, 100, 2, kd=64, hd=128, coff=8, extra=8, out_coff=8, seed=3, monkeypatch=monkeypatch, what="kd64 hd128")
    _attn_case(prec, 1, 70, 1, kd=16, hd=8, coff=0, extra=0, seed=4, monkeypatch=monkeypatch, what="kd16 hd8")


@pytest.mark.parametrize("prec", PRECS)
def test_attention_largest_map(prec, monkeypatch):
    """N = 10240, the largest map the per-query kernel accepts (its score rows fill the 160 KiB of LDS): a seeded sample of 256
    query rows against the reference over all keys."""
    rows = torch.from_numpy(np.sort(np.random.default_rng(10240).choice(10240, 256, replace=False)))
    _attn_case(prec, 1, 10240, 1, coff=8, extra=8, rows=rows, seed=10240, monkeypatch=monkeypatch, what="N10240")


@pytest.mark.parametrize("prec", PRECS)
def test_attention_map_too_large_is_refused(prec):
    """N = 10241 is refused with the forward's "too large" error; nothing is written."""
    det = detector(prec)
    qkv = torch.randn((1, 10241, 128), dtype=_dtype(prec), device="cuda")
    out = _sentinel((1, 10241, 64), prec)
    with pytest.raises(L.CyError, match="attention map too large"):
        det.attention(qkv, 1, 32, 64, out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


@pytest.mark.parametrize("slow,N", [(False, 400), (True, 400), (True, 1024)])
def test_attention_is_repeatable(slow, N, monkeypatch):
    """Race screen: the per-query kernel hands each wave's score row between lanes through LDS behind a fence and a wait count,
    the fast kernel stages K / V behind a barrier; twenty launches must give the same bits."""
    monkeypatch.setenv("CY_ATTN_SLOW", "1" if slow else "0")
    det = detector("fp32")
    g = torch.Generator().manual_seed(N)
    qkv = torch.randn((2, N, 256), generator=g).cuda()
    first = det.attention(qkv, 2, 32, 64, torch.empty((2, N, 128), device="cuda")).clone()
    for _ in range(20):
        assert torch.equal(first, det.attention(qkv, 2, 32, 64, torch.empty((2, N, 128), device="cuda")))


# ------------------------------------------------------------------------------------------------ 5x5 max pool
def _x3_exact(x):
    """fp32 values v that the fp16x3 split represents exactly: hi = fp16(v), lo = fp16(v - hi), hi + lo == v."""
    hi = x.half()
    lo = (x - hi.float()).half()
    v = hi.float() + lo.float()
    ok = (v.double() == hi.double() + lo.double()) & (v.half() == hi) & ((v - hi.float()).half() == lo)
    return torch.where(ok, v, hi.float())


def _pool_input(kind, shape, g, prec):
    x = torch.randn(shape, generator=g)
    if kind == "negative":              # all values negative: a zero pad would win at the borders
        x = -x.abs() - 0.5
    elif kind == "ties":                # a few levels: many equal values in every window
        x = torch.randint(-2, 3, shape, generator=g).float() * 0.75
    elif kind == "x3ties":              # high halves tie, low halves differ: the winner is decided on hi + lo
        hi = torch.randint(0, 4, shape, generator=g).float() * 0.25 + 2.25        # (half an fp16 ulp in [2, 4): 2^-10 > 500 2^-20)
        x = hi + torch.randint(-500, 500, shape, generator=g).float() * 2.0 ** -20
    if prec == "fp16":
        return x.half()
    return _x3_exact(x) if prec == "fp16x3" else x


def _pool_ref(x_nhwc):
    """F.max_pool2d(5, 1, 2) (-inf padding) in float64 on [B, H, W, C]."""
    return F.max_pool2d(x_nhwc.double().permute(0, 3, 1, 2), 5, 1, 2).permute(0, 2, 3, 1)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


POOL_MAPS = [(1, 1), (2, 3), (4, 4), (5, 7), (16, 16), (20, 20), (32, 32), (13, 9)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", ["random", "negative", "ties"])
@pytest.mark.parametrize("hw", POOL_MAPS, ids=["%dx%d" % m for m in POOL_MAPS])
def test_maxpool5_bit_exact(prec, kind, hw):
    """pool5_kernel (fp32, fp16) / pool5_x3_kernel (fp16x3) on maps down to 1x1 (smaller than the window: every window clamped),
    source and destination as slices of two wider tensors: bit-exact against F.max_pool2d."""
    H, W = hw
    det = detector(prec)
    g = torch.Generator().manual_seed(H * 100 + W + len(kind))
    B, C, ct = 2, 24, 48
    x = _pool_input(kind, (B, H, W, ct), g, prec)
    src = x.to(_dtype(prec)).cuda()
    dst = _sentinel((B, H, W, ct), prec)
    det.maxpool5(src, C, dst, src_coff=8, dst_coff=16)
    torch.cuda.synchronize()
    got = dst.cpu()
    _check_slice(got, 16, 16 + C, prec, "%s %dx%d" % (kind, H, W))
    ref = _pool_ref(x[..., 8:8 + C]).to(_dtype(prec))
    assert torch.equal(_bits(got[..., 16:16 + C]), _bits(ref)), "%s %dx%d: %d values differ" % (
        kind, H, W, int((got[..., 16:16 + C] != ref).sum()))


@pytest.mark.parametrize("hw", [(4, 4), (13, 9), (20, 20)])
def test_maxpool5_x3_decides_on_hi_plus_lo(hw):
    """fp16x3: windows whose high halves tie while the low halves differ; the stored halves must be those of the maximum of
    hi + lo (a comparison on hi alone keeps the first of the tied pixels)."""
    H, W = hw
    det = detector("fp16x3")
    g = torch.Generator().manual_seed(H * W)
    x = _pool_input("x3ties", (3, H, W, 16), g, "fp16x3")
    assert (x.half().float() != x).float().mean() > 0.9          # the low halves are there
    dst = _sentinel((3, H, W, 16), "fp16x3")
    det.maxpool5(x.cuda(), 8, dst, src_coff=0, dst_coff=8)
    got = dst.cpu()
    _check_slice(got, 8, 16, "fp16x3", "x3 ties")
    assert torch.equal(_bits(got[..., 8:]), _bits(_pool_ref(x[..., :8]).float()))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("hw", [(20, 20), (13, 9)])
def test_sppf_chain_in_place(prec, hw):
    """SPPF as the plan runs it: slice 0 -> 1 -> 2 -> 3 of one buffer, every pool reading and writing the same tensor."""
    H, W = hw
    det = detector(prec)
    g = torch.Generator().manual_seed(H + W)
    C = 32
    buf = _sentinel((2, H, W, 4 * C), prec)
    x = _pool_input("random", (2, H, W, C), g, prec)
    buf[..., :C] = x.to(_dtype(prec)).cuda()
    for j in range(3):
        det.maxpool5(buf, C, buf, src_coff=j * C, dst_coff=(j + 1) * C)
    got = buf.cpu()
    ref = x.double()
    for j in range(3):
        ref = _pool_ref(ref)
        part = got[..., (j + 1) * C:(j + 2) * C]
        assert torch.isfinite(part).all()
        assert torch.equal(_bits(part), _bits(ref.to(_dtype(prec)))), "slice %d" % (j + 1)
    assert torch.equal(_bits(got[..., :C]), _bits(x.to(_dtype(prec))))
