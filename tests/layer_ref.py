"""Teacher-forced float64 walk of the YOLOv8 detection graph: every convolution of one forward pass checked on its own.

The graph (`run_graph`) restates oracle/yolov8_ref.py `Net.forward`: stem, C2f with and without shortcut, SPPF, nearest
upsample, the concats and the three head levels, for any scale whose weights are given (n3 / n6 are read off the names).

`walk(weights, x, provider, prec)` computes, for every convolution, the float64 reference of THAT layer from the values that
entered it on the device, and continues from the device's output (`provider(name, ref)`, float64 [B, C, H, W]) -- never from
the reference -- so no error travels past one layer.  Chunk, concat, upsample and the 5 x 5 max pools are exact: they are
applied in torch to the provider's values, so a wrong device pool or gather shows at the convolution that reads it.

Weights are the ones the context holds (`context_weights`): fp16 context -- folded filters rounded to fp16 (the stem too when
it has 64 output channels: the matrix-core stem kernels; narrower stems keep the fp32 filter of stem_kernel); fp32 / fp16x3 --
the folded fp32 filters.  The bias is fp32 everywhere.

A layer the device never stored (provider returns None: it ran fused into its reader) gets the two-step definition of the
unfused path: its reference is rounded to the context's storage type and fed to the reader, and the interval within which the
device's intermediate may differ from that rounded reference is carried through the reader's |w| into the reader's bound.
The interval is (error before the store + one spacing of the storage type), and in the fp16 context 0 where the exact value
lies farther from a rounding tie of fp16 than the layer's own error before the store (device and reference then round to the
same number).  The same holds for a layer whose buffer a later layer reuses: the bottlenecks of one C2f share the buffer of
their cv1 outputs, so only the last one's survives the pass (read_conv refuses the others).

THE BOUND, per output element.  u = 2^-24 (fp32 unit roundoff), K = Cin k k, S = sum |x| |w| + |b| (one float64 convolution of
the absolute values), z the pre-activation, y the output before the store.
  accumulation   fp16 / fp32 contexts: (K + 1) u S -- K products and the bias added in fp32, any summation order (the products
                 of fp16 operands are exact in fp32; fp32 context: fused multiply-adds, one rounding each).
                 fp16x3 context: the input IS x_hi + x_lo as stored, so it carries no error.  Two-pass layers (filter = fp16
                 filter w16 times a per-channel factor, factor applied to the accumulator): 2K products against
                 S' = sum (|x_hi| + |x_lo|) |w| <= (1 + 2^-10) S, the factor and the bias two more roundings, and the folded
                 filter the reference uses is fl32(w16 * factor), one rounding away from the device's: (2K + 3) u (1 + 2^-10) S.
                 Three-pass layers (pack_weights_x3: w 2^e = w_hi + w_lo + r): 3K products and the bias, (3K + 1) u (1 + 2^-10) S;
                 |r| <= 2^-22 |w| while w_lo is a normal fp16 number, else <= 2^-25 in scaled units whose channel maximum is
                 >= 2^13, i.e. 2^-38 max|w_n|: 2^-22 S + 2^-38 max|w_n| sum|x|; the dropped x_lo w_lo product: 2^-22 S.
                 fp16x3 stem: an fp32 fmaf chain on the fp32 filter: (K + 1) u S.
                 An unmaterialised input adds conv(interval, |w|).
  activation     SiLU carries the pre-activation error with |silu'| <= 1.1.  silu_fast is z * rcp(1 + exp2(z * fl(-log2 e))):
                 the product and the constant are one fp32 rounding each, which moves the exponent by <= |z| log2(e) 2^-23, i.e.
                 exp2's value by |z| 2^-23 relative; exp2 is 1 ulp (2^-23), both enter 1 / (1 + e) with weight e / (1 + e) =
                 1 - sigmoid(z); the addition is 2^-24, rcp 1 ulp (2^-23), the last product 2^-24:
                 rel = 2^-23 ((1 + |z|) (1 - sigmoid(z)) + 1.5).  silu_exact (fp32 context: expf 1 ulp, add, correctly rounded
                 divide) lies inside the same expression.  CONDITION, asserted: rel < 2^-16, a thirty-second of the fp16
                 half-ulp, so this term can never decide.  Below z = -87 exp2 overflows and the device returns -0 where the
                 exact value is ~1e-36: the allowance there is |y| itself.
  residual add   one fp32 rounding of the sum: u (|y + r| + error so far).  (fp16x3: r_hi + r_lo is exact in fp32.)
  store          fp16: 2^-11 |out| + 2^-25 (half a spacing; 2^-25 in the subnormal range).  fp32: 2^-24 |out|.  fp16x3
                 (store_split16: hi = fp16(v), lo = fp16(v - hi)): |v - hi| <= 2^-11 |v| and lo rounds it to 2^-11 of that:
                 2^-22 |out|, or 2^-25 when lo is subnormal: 2^-22 |out| + 2^-25.  |out| is |ref| + the error so far.
                 The head's prediction rows are the fp32 epilogue values themselves in the fp16 / fp16x3 contexts: no store term.
  double rounding  none: every epilogue read for this bound (conv_igemm_kernel, the halo / wide / direct / head kernels, the stem
                 kernels) keeps SiLU's result and the residual sum in fp32 and rounds once at the store.
No term carries a free factor; none was adjusted to an observed output.
"""
import re
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24


class Val(object):
    """A tensor on its way through the graph: v float64 [B, C, H, W]; iv = interval of an unmaterialised value, else None."""

    def __init__(self, v, iv=None):
        self.v, self.iv = v, iv


def depths(weights):
    """(n3, n6) of the scale, from the bottleneck names present."""
    cnt = lambda i: 1 + max(int(m.group(1)) for m in (re.match(r"model\.%d\.m\.(\d+)\.cv1$" % i, k) for k in weights) if m)
    return cnt(2), cnt(4)


def run_graph(x, ops, n3, n6):
    """The yolov8 graph on `ops` (conv(name, t, s, act, res), chunk2, cat, up, pool): returns the nine head outputs
    {name: t} of the box / class branches; every conv output passes through ops.conv."""
    def c2f(i, t, n, shortcut):
        y = list(ops.chunk2(ops.conv("model.%d.cv1" % i, t)))
        for j in range(n):
            h = ops.conv("model.%d.m.%d.cv1" % (i, j), y[-1])
            y.append(ops.conv("model.%d.m.%d.cv2" % (i, j), h, res=y[-1] if shortcut else None))
        return ops.conv("model.%d.cv2" % i, ops.cat(y, "model.%d.cv2" % i))

    x0 = ops.conv("model.0", x, s=2)
    x1 = ops.conv("model.1", x0, s=2)
    x2 = c2f(2, x1, n3, True)
    x4 = c2f(4, ops.conv("model.3", x2, s=2), n6, True)
    x6 = c2f(6, ops.conv("model.5", x4, s=2), n6, True)
    x8 = c2f(8, ops.conv("model.7", x6, s=2), n3, True)
    a = ops.conv("model.9.cv1", x8)
    b = ops.pool(a)
    c = ops.pool(b)
    d = ops.pool(c)
    x9 = ops.conv("model.9.cv2", ops.cat((a, b, c, d), "model.9.cv2"))
    x12 = c2f(12, ops.cat((ops.up(x9, "model.12.cv1"), x6), "model.12.cv1"), n3, False)
    x15 = c2f(15, ops.cat((ops.up(x12, "model.15.cv1"), x4), "model.15.cv1"), n3, False)
    x18 = c2f(18, ops.cat((ops.conv("model.16", x15, s=2), x12), "model.18.cv1"), n3, False)
    x21 = c2f(21, ops.cat((ops.conv("model.19", x18, s=2), x9), "model.21.cv1"), n3, False)
    heads = {}
    for lvl, f in enumerate((x15, x18, x21)):
        for br in ("cv2", "cv3"):
            p = "model.22.%s.%d." % (br, lvl)
            heads[p + "2"] = ops.conv(p + "2", ops.conv(p + "1", ops.conv(p + "0", f)), act=False)
    return heads


def context_weights(weights, prec):
    """name -> (W, b) float64 as the context of precision `prec` holds them."""
    out = {}
    for k, (w, b) in weights.items():
        w, b = torch.tensor(np.asarray(w), dtype=torch.float32), torch.tensor(np.asarray(b), dtype=torch.float32)
        if prec == "fp16" and not (k == "model.0" and w.shape[0] != 64):
            w = w.half().float()
        out[k] = (w.double(), b.double())
    return out


def round_store(v, prec):
    """Round float64 values to the storage type of the context (fp16x3: hi + lo)."""
    if prec == "fp16":
        return v.float().half().double()
    if prec == "fp32":
        return v.float().double()
    hi = v.float().half().float()
    return hi.double() + (v.float() - hi).half().double()


def store_term(mag, prec):
    if prec == "fp16":
        return 2.0 ** -11 * mag + 2.0 ** -25
    if prec == "fp32":
        return U * mag
    return 2.0 ** -22 * mag + 2.0 ** -25


def fp16_tie_distance(y):
    """Distance of float64 y from the nearest value at which rounding to fp16 changes its result."""
    a = y.abs()
    r = a.float().half().double()
    e = torch.frexp(torch.clamp(r, min=2.0 ** -14))[1].double() - 1.0
    e = torch.clamp(e, min=-14.0)
    sp = torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 10.0)
    pow2 = (r == torch.pow(torch.tensor(2.0, dtype=torch.float64), e)) & (e > -14.0)
    below = torch.where(pow2, sp / 4, sp / 2)
    return torch.minimum(r + sp / 2 - a, a - (r - below))


def silu_allowance(z):
    """Relative allowance of silu_fast / silu_exact at pre-activation z (see the module docstring)."""
    return 2.0 ** -23 * ((1.0 + z.abs()) * (1.0 - torch.sigmoid(z)) + 1.5)


def acc_term(x, w, S, s, pad, prec, passes, stem):
    """Accumulation term of one convolution (module docstring); stem: the fp32 fmaf chain of the stem kernels."""
    K = w.shape[1] * w.shape[2] * w.shape[3]
    if prec != "fp16x3" or stem:
        return (K + 1) * U * S
    if passes == 2:
        return (2 * K + 3) * U * (1 + 2.0 ** -10) * S
    wmax = w.abs().amax(dim=(1, 2, 3)).view(1, -1, 1, 1)
    sx = F.conv2d(x.abs(), torch.ones((1,) + tuple(w.shape[1:]), dtype=torch.float64), None, stride=s, padding=pad)
    return (3 * K + 1) * U * (1 + 2.0 ** -10) * S + 2.0 ** -21 * S + 2.0 ** -38 * wmax * sx


def conv_bound(name, t, w, b, s, act, res, prec, passes, stem, head):
    """One convolution (+ bias, SiLU, residual) in float64 on the values that entered it.  t: Val (iv: the interval of an
    unmaterialised input); w, b float64; res: float64 residual or None; stem: the stem kernels' accumulation; head: the output is
    a block of prediction rows.  -> (y, e, st): the reference, the error bound before the store and the store term; the device's
    value must lie within e + st of y.  Shared by the YOLOv8 walk below and the plan walk of tests/plan_ref.py."""
    pad = w.shape[-1] // 2
    x = t.v
    z = F.conv2d(x, w, b, stride=s, padding=pad)
    S = F.conv2d(x.abs(), w.abs(), b.abs(), stride=s, padding=pad)
    ez = acc_term(x, w, S, s, pad, prec, passes, stem)
    if t.iv is not None:
        ez = ez + F.conv2d(t.iv, w.abs(), None, stride=s, padding=pad)
    if act:
        y = F.silu(z)
        rel = silu_allowance(z)
        used = torch.where(z < -87.0, torch.zeros_like(rel), rel)          # (below -87 the allowance is |y| itself, not rel |y|)
        assert float(used.max()) < 2.0 ** -16, "%s: SiLU allowance %.3e is not below 2^-16" % (name, float(used.max()))
        e = 1.1 * ez + torch.where(z < -87.0, y.abs(), rel * y.abs())
    else:
        y, e = z, ez
    if res is not None:
        y = y + res
        e = e + U * (y.abs() + e)
    st = torch.zeros_like(y) if (head and prec != "fp32") else store_term(y.abs() + e, prec)
    return y, e, st


def unmaterialised(y, e, st, prec):
    """The value a reader gets of a layer the device never stored: the reference rounded to the storage type, with the interval
    within which the device's intermediate may differ from it (module docstring)."""
    iv = e + 2.0 * st
    if prec == "fp16":
        iv = torch.where(fp16_tie_distance(y) > e, torch.zeros_like(e), iv)
    return Val(round_store(y, prec), iv)


def compare(got, y, bound, K):
    """-> the report entry of one materialised output: worst |got - y| / bound and where."""
    ratio = (got - y).abs() / bound
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    i = int(ratio.argmax())
    pos = tuple(int(v) for v in np.unravel_index(i, tuple(ratio.shape)))
    return dict(materialised=True, ratio=float(ratio.flatten()[i]), pos=pos, got=float(got[pos]), ref=float(y[pos]),
                bound=float(bound[pos]), K=K)


class _Walk(object):
    def __init__(self, weights, provider, prec, passes):
        self.w, self.provider, self.prec, self.passes = context_weights(weights, prec), provider, prec, passes
        self.report = {}

    def chunk2(self, t):
        assert t.iv is None
        return [Val(c) for c in t.v.chunk(2, 1)]

    def cat(self, ts, reader):
        assert all(t.iv is None for t in ts)
        return Val(torch.cat([t.v for t in ts], 1))

    def up(self, t, reader):
        assert t.iv is None
        return Val(F.interpolate(t.v, scale_factor=2, mode="nearest"))

    def pool(self, t):
        assert t.iv is None
        return Val(F.max_pool2d(t.v, 5, 1, 2))

    def conv(self, name, t, s=1, act=True, res=None):
        w, b = self.w[name]
        assert res is None or res.iv is None
        head = name.startswith("model.22.") and name.endswith(".2")
        y, e, st = conv_bound(name, t, w, b, s, act, None if res is None else res.v, self.prec, self.passes, name == "model.0", head)
        got = self.provider(name, y)
        if got is None:
            self.report[name] = dict(materialised=False, ratio=None)
            return unmaterialised(y, e, st, self.prec)
        got = torch.as_tensor(got, dtype=torch.float64)
        assert tuple(got.shape) == tuple(y.shape), "%s: device shape %s, reference %s" % (name, tuple(got.shape), tuple(y.shape))
        self.report[name] = compare(got, y, e + st, int(w.shape[1] * w.shape[2] * w.shape[3]))
        return Val(got)


def walk(weights, x, provider, prec, passes=2):
    """weights: name -> (W, b) folded fp32; x: the network input [B, 3, H, W] as the device read it (float64);
    provider(name, ref) -> the device's output of that convolution as [B, C, H, W] (the shortcut sum where the kernel adds the
    residual; the head's box / class rows taken from the prediction buffer), or None when the layer was never stored.
    prec: fp16 | fp32 | fp16x3; passes: 2 | 3, the form of the fp16x3 filters (cy_weight_passes).
    -> {name: dict(materialised, ratio = worst |got - ref| / bound, pos = (b, c, row, col), got, ref, bound, K)}."""
    n3, n6 = depths(weights)
    wk = _Walk(weights, provider, prec, passes)
    with torch.no_grad():
        run_graph(Val(torch.as_tensor(x, dtype=torch.float64)), wk, n3, n6)
    return wk.report


def pred_rows(pred, B, H, W, nc):
    """Head output [B, A, 64 + nc] -> {name: [B, C, h, w]} of the nine output convolutions' rows."""
    out, off = {}, 0
    for lvl, s in enumerate((8, 16, 32)):
        h, w = H // s, W // s
        rows = pred[:, off:off + h * w].reshape(B, h, w, 64 + nc).permute(0, 3, 1, 2)
        out["model.22.cv2.%d.2" % lvl] = rows[:, :64]
        out["model.22.cv3.%d.2" % lvl] = rows[:, 64:]
        off += h * w
    return out


# ------------------------------------------------------------------------------------------------ a device in torch, on the CPU
class Emulator(object):
    """The forward pass as a context of precision fp16 / fp32 runs it, in torch on the CPU: operands as the context holds
    them, fp32 conv2d, fp32 epilogue (bias, SiLU, residual), one rounding to the storage type.  `fused`: layers whose output
    is handed to their reader rounded but never stored.  `fault(name, stage, ...)`: hooks of the seeded faults (tests)."""

    def __init__(self, weights, prec, fused=(), fault=None):
        self.w = {k: (w.float(), b.float()) for k, (w, b) in context_weights(weights, prec).items()}
        self.prec, self.fused, self.fault, self.out = prec, set(fused), fault or (lambda *a, **k: None), {}

    def chunk2(self, t):
        return list(t.chunk(2, 1))

    def cat(self, ts, reader):
        ts = list(ts)
        r = self.fault(reader, "cat", ts)
        return torch.cat(r if r is not None else ts, 1)

    def up(self, t, reader):
        u = F.interpolate(t, scale_factor=2, mode="nearest")
        r = self.fault(reader, "up", u)
        return r if r is not None else u

    def pool(self, t):
        return F.max_pool2d(t, 5, 1, 2)

    def conv(self, name, t, s=1, act=True, res=None):
        w, b = self.w[name]
        r = self.fault(name, "operands", t, w, b)
        if r is not None:
            t, w, b = r
        y = F.conv2d(t, w, b, stride=s, padding=w.shape[-1] // 2)
        r = self.fault(name, "taps", t, w, b, s, y)
        if r is not None:
            y = r
        if act:
            y = F.silu(y)
        if res is not None:
            r = self.fault(name, "res", y, res)
            y = r if r is not None else y + res
        head = name.startswith("model.22.") and name.endswith(".2")
        if self.prec == "fp16" and not head and self.fault(name, "keep32") is None:
            y = y.half().float()
        r = self.fault(name, "out", y)
        if r is not None:
            y = r
        self.out[name] = y
        return y

    def run(self, x):
        n3, n6 = depths(self.w)
        with torch.no_grad():
            run_graph(torch.as_tensor(x, dtype=torch.float32), self, n3, n6)
        return self

    def provider(self, name, ref):
        return None if name in self.fused else self.out[name].double()
