"""One convolution in the layout the forward pass gives it (cy_conv_slices): caller buffers with guard channels, the float64
reference with layer_ref.conv_bound's per-element bound, the checker, and a stand-in device in torch with seeded address faults.

Buffers (`build`).  Every tensor a kernel may touch is exactly as large as the entry is told; what lies outside the slices is
there to be noticed:
  * input and residual channels outside their slice are NaN -- a read past the slice poisons the sum even through a zero weight;
  * output elements outside the slice hold (flat index mod 2039) - 1000, integers that fp16 holds exactly (so they survive the
    fp16x3 split / merge of the whole buffer bit for bit) and that differ from their neighbours -- a store past the slice, a
    shifted slice or a dropped row offset changes one of them.  In rows mode the rows outside [out_ro, out_ro + Ho Wo) are guards too.
Slices hold seeded normal values as the context stores activations: fp16-rounded in the fp16 context (weights too: what the
context's packing would make of them), fp16 high + low halves in fp16x3.

Layouts (channel counts of the buffers; offsets are multiples of 8 as the kernels' 8-channel vectors need):
  dense    ct = C, offset 0 everywhere                                  (what cy_conv_bn_silu passes)
  slices   in0 at 16 of Cin + 24; out at 24 of Cout + 40; res at 8 of a third buffer of Cout + 16
  shared   as slices, but res at 8 and out at 8 + Cout of ONE buffer of 2 Cout + 24 (the C2f bottleneck: res slice j, out slice j + 1)
  concat   two segments: c0 = 64 channels at 16 of a buffer of 64 + 24, c1 = Cin - 64 at 8 of a buffer of c1 + 16; out / res as slices
  upcat    concat with segment 0 stored at half resolution and read through the nearest x2 upsample
  rows     in0 as slices; out = fp32 prediction rows [B][out_bs][out_ct] at (out_ro, out_coff); no residual, no activation

The check (`check`): every slice element within e + st of the float64 reference (conv_bound, unchanged: no tolerance is chosen
here), every guard element bit-identical to what `build` put there, no NaN anywhere in the output buffer."""
from types import SimpleNamespace
import numpy as np
import torch
import torch.nn.functional as F
import layer_ref as LR

LAYOUTS = ("dense", "slices", "shared", "concat", "upcat", "rows")
SEG0 = 64                                  # channels of segment 0 in the two-segment layouts: one K chunk of fp16, two of fp32


def out_hw(H, W, k, s):
    return (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1


def _pattern(shape, dtype):
    n = int(np.prod(shape))
    return ((torch.arange(n, dtype=torch.int64) % 2039) - 1000).to(dtype).reshape(shape)


def _embed(vals_nhwc, ct, coff, dtype, fill):
    """NHWC values into channels [coff, coff + C) of a buffer of ct channels whose other channels hold `fill` (None: the pattern)."""
    shape = tuple(vals_nhwc.shape[:-1]) + (ct,)
    buf = _pattern(shape, dtype) if fill is None else torch.full(shape, fill, dtype=dtype)
    buf[..., coff:coff + vals_nhwc.shape[-1]] = vals_nhwc.to(dtype)
    return buf.contiguous()


def build(prec, geom, act, layout, seed, rows=None, w16=False):
    """geom = (B, Hi, Wi, Cin, Cout, k, s); rows = dict(out_ct, out_coff, out_bs, out_ro) for layout "rows".
    w16: fp16-exact filter in the fp32 / fp16x3 contexts (the two-pass form of fp16x3)."""
    B, H, W, Cin, Cout, k, s = geom
    assert layout in LAYOUTS and (layout == "rows") == (rows is not None)
    dtype = torch.float16 if prec == "fp16" else torch.float32
    # activations as the context stores them (fp16x3: hi + lo, which the entry's split reproduces exactly -- conv_bound takes the
    # input as stored, and a residual inside the output buffer must come back from the split / merge bit for bit)
    rnd = (lambda v: v) if prec == "fp32" else (lambda v: LR.round_store(v.double(), prec).float())
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = out_hw(H, W, k, s)
    two = layout in ("concat", "upcat")
    up = layout == "upcat"
    assert not two or (k == 1 and s == 1 and Cin > SEG0), "two segments: 1x1 with more than %d channels" % SEG0
    assert not up or (H % 2 == 0 and W % 2 == 0)
    c0 = SEG0 if two else Cin
    c1 = Cin - c0
    x0 = rnd(torch.randn((B, H >> up, W >> up, c0), generator=g))
    x1 = rnd(torch.randn((B, H, W, c1), generator=g)) if two else None
    w = torch.randn((Cout, Cin, k, k), generator=g) / (Cin * k * k) ** 0.5
    w = w.half().float() if (prec == "fp16" or w16) else w
    b = torch.randn((Cout,), generator=g) * 0.1
    use_res = layout != "rows"
    r = rnd(torch.randn((B, Ho, Wo, Cout), generator=g)) if use_res else None
    nan = float("nan")
    t = SimpleNamespace(prec=prec, geom=geom, act=bool(act) and layout != "rows", layout=layout, rows=rows, w=w, b=b, c0=c0, c1=c1, up0=up,
                        Ho=Ho, Wo=Wo, in1=None, in1_coff=0, res=None, res_coff=0, shared=False)
    if layout == "dense":
        t.in0, t.in0_coff = _embed(x0, c0, 0, dtype, nan), 0
        t.out, t.out_coff = _pattern((B, Ho, Wo, Cout), dtype), 0
        t.res = _embed(r, Cout, 0, dtype, nan)
    else:
        t.in0, t.in0_coff = _embed(x0, c0 + 24, 16, dtype, nan), 16
        if two:
            t.in1, t.in1_coff = _embed(x1, c1 + 16, 8, dtype, nan), 8
        if layout == "rows":
            t.out = _pattern((B, rows["out_bs"], rows["out_ct"]), torch.float32)
            t.out_coff = rows["out_coff"]
        elif layout == "shared":
            t.out = _embed(r, 2 * Cout + 24, 8, dtype, None)
            t.out_coff, t.res_coff, t.shared = 8 + Cout, 8, True
        else:
            t.out, t.out_coff = _pattern((B, Ho, Wo, Cout + 40), dtype), 24
            t.res, t.res_coff = _embed(r, Cout + 16, 8, dtype, nan), 8
    # the logical operands of the reference, float64 NCHW
    xs = [x0.permute(0, 3, 1, 2).double()]
    if up:
        xs[0] = F.interpolate(xs[0], scale_factor=2, mode="nearest")
    if two:
        xs.append(x1.permute(0, 3, 1, 2).double())
    t.x = torch.cat(xs, 1)
    t.r = r.permute(0, 3, 1, 2).double() if use_res else None
    return t


def out_mask(t):
    """bool tensor of t.out's shape: True inside the output slice."""
    m = torch.zeros(tuple(t.out.shape), dtype=torch.bool)
    Cout = t.geom[4]
    if t.layout == "rows":
        ro = t.rows["out_ro"]
        m[:, ro:ro + t.Ho * t.Wo, t.out_coff:t.out_coff + Cout] = True
    else:
        m[..., t.out_coff:t.out_coff + Cout] = True
    return m


def out_slice(t, buf):
    """The output slice of a buffer shaped like t.out -> float64 [B, Cout, Ho, Wo]."""
    B, Cout = t.geom[0], t.geom[4]
    if t.layout == "rows":
        ro = t.rows["out_ro"]
        v = buf[:, ro:ro + t.Ho * t.Wo, t.out_coff:t.out_coff + Cout].reshape(B, t.Ho, t.Wo, Cout)
    else:
        v = buf[..., t.out_coff:t.out_coff + Cout]
    return v.permute(0, 3, 1, 2).double()


def reference(t, passes):
    """-> (y, bound) float64 [B, Cout, Ho, Wo]: layer_ref.conv_bound on cat(up(x0), x1)."""
    _, _, _, Cin, _, k, s = t.geom
    with torch.no_grad():
        y, e, st = LR.conv_bound("conv_slices", LR.Val(t.x), t.w.double(), t.b.double(), s, t.act, t.r, t.prec, passes, False,
                                 t.layout == "rows")
    return y, e + st


def check(t, got, variant="", passes=2, ref=None):
    """got: the output buffer after the call (CPU tensor shaped and typed like t.out).  Asserts the three properties of the module
    docstring; -> worst |got - ref| / bound over the slice.  ref: a (y, bound) computed before (shared between runs of one case)."""
    assert tuple(got.shape) == tuple(t.out.shape) and got.dtype == t.out.dtype
    what = "%s %s %s [%s]" % (t.prec, "x".join(map(str, t.geom)), t.layout, variant)
    y, bound = ref if ref is not None else reference(t, passes)
    K = t.geom[3] * t.geom[5] * t.geom[5]
    rep = LR.compare(out_slice(t, got), y, bound, K)
    assert rep["ratio"] <= 1.0, "%s at (b, c, row, col) = %s: got %.9g, reference %.9g, bound %.3g (ratio %.3f, K = %d)" % (
        what, rep["pos"], rep["got"], rep["ref"], rep["bound"], rep["ratio"], K)
    bits = torch.int16 if got.dtype == torch.float16 else torch.int32
    diff = (got.contiguous().view(bits) != t.out.contiguous().view(bits)) & ~out_mask(t)
    if bool(diff.any()):
        pos = tuple(int(v) for v in diff.nonzero()[0])
        raise AssertionError("%s: guard element %s of the output buffer (slice at channel %d, %d channels) changed from %r to %r; %d changed in all"
                             % (what, pos, t.out_coff, t.geom[4], float(t.out[pos]), float(got[pos]), int(diff.sum())))
    assert not bool(torch.isnan(got).any()), "%s: NaN in the output buffer" % what
    return rep["ratio"]


# ------------------------------------------------------------------------------------------------ a device in torch, on the CPU
MUTANTS = ("store_past_cout", "out_coff_plus8", "res_coff_ignored", "in0_ct_is_c0", "in1_at_in0_stride", "up_full_res", "out_ro_dropped",
           "tap_dropped", "double_rounding")


def _gather(buf, pix, ct, coff, c):
    """Channels [coff, coff + c) of pixel indices `pix` of a buffer read with pixel stride ct; an address past the buffer reads 0
    (the hardware range check of the kernels' buffer loads)."""
    flat = buf.flatten().float()
    idx = pix.unsqueeze(-1) * ct + coff + torch.arange(c)
    ok = idx < flat.numel()
    return torch.where(ok, flat[idx.clamp(max=flat.numel() - 1)], torch.zeros(()))


def emulate(t, mutant=None):
    """The entry as an fp16 / fp32 context computes it, from the buffers alone and by their addresses: fp32 convolution and
    epilogue, one rounding to the storage type, stores into a copy of t.out.  mutant: one of MUTANTS, a seeded address or
    arithmetic fault.  -> the output buffer."""
    assert t.prec in ("fp16", "fp32") and (mutant is None or mutant in MUTANTS)
    B, H, W, Cin, Cout, k, s = t.geom
    H0, W0 = H >> t.up0, W >> t.up0
    bb, hh, ww = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing="ij")
    if t.up0 and mutant != "up_full_res":
        p0 = (bb * H0 + (hh >> 1)) * W0 + (ww >> 1)
    else:
        p0 = (bb * H0 + hh) * W0 + ww if t.up0 else (bb * H + hh) * W + ww
    x = _gather(t.in0, p0, t.c0 if mutant == "in0_ct_is_c0" else t.in0.shape[-1], t.in0_coff, t.c0)
    if t.c1:
        p1 = (bb * H + hh) * W + ww
        x = torch.cat([x, _gather(t.in1, p1, t.in0.shape[-1] if mutant == "in1_at_in0_stride" else t.in1.shape[-1], t.in1_coff, t.c1)], -1)
    x = x.permute(0, 3, 1, 2)
    w = t.w.float()
    y = F.conv2d(x, w, t.b.float(), stride=s, padding=k // 2)
    if mutant == "tap_dropped":            # the centre-row left tap of output pixel (0, 1) of the last image
        kh, kw, ho, wo = k // 2, 0, 0, 1
        hi, wi = ho * s - k // 2 + kh, wo * s - k // 2 + kw
        assert 0 <= hi < H and 0 <= wi < W
        y[B - 1, :, ho, wo] -= (w[:, :, kh, kw] * x[B - 1, :, hi, wi]).sum(1)
    if t.act:
        y = F.silu(y)
    y = y.permute(0, 2, 3, 1)
    pix = torch.arange(B * t.Ho * t.Wo).reshape(B, t.Ho, t.Wo)
    res = t.out if t.shared else t.res
    if res is not None:
        y = y + _gather(res, pix, res.shape[-1], 0 if mutant == "res_coff_ignored" else t.res_coff, Cout)
    if mutant == "double_rounding":        # fp32 -> its upper 16 bits -> the storage type
        y = (y.contiguous().view(torch.int32) & -65536).view(torch.float32)
    y = y.to(t.out.dtype)
    n = Cout + (8 if mutant == "store_past_cout" else 0)
    vals = torch.zeros((B, t.Ho, t.Wo, n), dtype=t.out.dtype)
    vals[..., :Cout] = y
    coff = t.out_coff + (8 if mutant == "out_coff_plus8" else 0)
    if t.layout == "rows":
        img = torch.arange(B).reshape(B, 1, 1)
        pix = img * t.rows["out_bs"] + (0 if mutant == "out_ro_dropped" else t.rows["out_ro"]) + (pix - img * t.Ho * t.Wo)
    out = t.out.clone().flatten()
    idx = pix.unsqueeze(-1) * t.out.shape[-1] + coff + torch.arange(n)
    ok = idx < out.numel()
    out[idx[ok]] = vals[ok]
    return out.reshape(t.out.shape)


# ------------------------------------------------------------------------------------------------ the cases, and the variant each must select
# Read by tests/test_gpu_conv_slices.py (runs them) and tests/test_conv_plan_cpu.py (asks the dispatch alone, on the CPU).
G128, G64, HALO, PP, C64, BIG, WIDE, D256, D128, WIDE64, DUAL, STRIP, HEAD = (
    "conv_igemm_kernel<2,2,4>", "conv_igemm_kernel<4,1,2>", "conv3x3_halo2_kernel", "conv3x3_pp_kernel<2>", "conv3x3_c64_kernel<64|32>",
    "conv_igemm_kernel<4,2,4,3>", "conv3x3_wide_kernel", "conv1x1_direct_kernel<4,2>", "conv1x1_direct_kernel<2,2>",
    "conv3x3_wide_kernel<WN=1>", "conv3x3_wide_kernel<dual>", "conv3x3_widep_kernel<strip>", "head1x1_kernel")
DIRECT = {"CY_DIRECT_MIN_BLOCKS": "1"}
TWO = ("concat", "upcat")

# name: ((B, H, W, Cin, Cout, k, s), CY_BATCH_INVARIANT, further switches, variant, takes two segments / the upsample)
SHAPES = {
    "wide": ((2, 10, 30, 128, 200, 3, 1), "1", {}, WIDE, False),                  # ragged rows and columns of the 16 x 32 patch; Cout % 16 != 0: not persistent
    "wide-persist": ((2, 10, 30, 128, 208, 3, 1), "1", {"CY_WIDE_PERSIST": "2"}, WIDE, False),
    "dual": ((3, 9, 15, 128, 200, 3, 1), "1", {"CY_WIDE_DUAL": "2"}, DUAL, False),      # odd batch: the last pair has one image
    "halo2": ((2, 10, 20, 128, 200, 3, 1), "1", {}, HALO, False),                 # two taps per barrier (two 64-channel slabs)
    "halo": ((2, 10, 20, 64, 200, 3, 1), "1", {}, HALO, False),                   # conv3x3_halo_kernel<2, 2> (one slab)
    "wide64": ((2, 10, 32, 128, 40, 3, 1), "1", {}, WIDE64, False),
    "pp": ((2, 10, 18, 128, 40, 3, 1), "1", {}, PP, False),
    "c64": ((2, 20, 18, 64, 40, 3, 1), "1", {}, C64, False),
    "c64<32>": ((2, 20, 18, 32, 40, 3, 1), "1", {}, C64, False),
    "strip": ((2, 19, 21, 128, 208, 3, 1), "1", {"CY_STRIP": "2"}, STRIP, False),
    "direct256": ((2, 9, 11, 128, 200, 1, 1), "1", DIRECT, D256, True),
    "direct128": ((2, 9, 11, 128, 72, 1, 1), "1", DIRECT, D128, True),
    "direct256-3x3s2": ((2, 18, 22, 128, 200, 3, 2), "1", DIRECT, D256, False),
    "direct128-3x3s2": ((2, 18, 22, 128, 72, 3, 2), "1", DIRECT, D128, False),
    "head-inside": ((2, 9, 11, 128, 40, 1, 1), "1", {}, HEAD, False),             # head1x1_kernel inside the network: fp16 slice, SiLU, residual
    "generic-big": ((2, 9, 15, 72, 200, 1, 1), "1", {}, BIG, True),
    "generic64": ((2, 9, 11, 72, 40, 1, 1), "1", {}, G64, True),
    "generic128": ((2, 9, 11, 72, 200, 1, 1), "0", {}, G128, True),               # thresholds see the real batch
}
# fp16x3 selects by geometry alone: no CY_DIRECT_MIN_BLOCKS, no CY_STRIP=2; CY_X3_PERSIST=1 is the persistent launch of the wide kernel
X3 = {n: SHAPES[n] for n in ("wide", "dual", "wide64", "strip", "direct256", "direct128", "direct256-3x3s2", "direct128-3x3s2",
                             "head-inside", "generic128", "generic64")}
X3["wide-persist"] = (SHAPES["wide-persist"][0], "1", {"CY_X3_PERSIST": "1"}, WIDE, False)
F32 = {n: SHAPES[n] for n in ("generic128", "generic64")}

# the head's output convolutions: prediction rows [B][out_bs][64 + nc] with rows before and behind the level's block
ROW_CASES = []      # (id, prec, geom, head_direct, variant, rows, seed)
for prec in ("fp16", "fp16x3", "fp32"):
    for hd in (1, 0):
        for mi, (h, w) in enumerate(((3, 5), (8, 8), (13, 16))):
            for bi, (cin, cout, nc) in enumerate(((64, 64, 5), (128, 1, 1), (128, 5, 5), (128, 80, 80))):      # box branch, class branches
                coff = 0 if bi == 0 else 64
                direct = hd == 1 and prec != "fp32" and cout <= 64
                variant = HEAD if direct else (G64 if cout <= 64 else G128)
                rows = dict(out_ct=64 + nc, out_coff=coff, out_bs=h * w + 29, out_ro=17)
                ROW_CASES.append(("%s-hd%d-%dx%d-%s" % (prec, hd, h, w, "box" if bi == 0 else "nc%d" % nc), prec, (2, h, w, cin, cout, 1, 1), hd,
                                  variant, rows, 1000 + 10 * mi + bi))
