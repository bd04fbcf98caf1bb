"""Teacher-forced float64 walk of an execution plan (caesar_yolo_amd/yolo11_graph.Graph: tensors, ops, convs): every op of one
forward pass checked on its own, whatever buffer it writes.

THE DEVICE is anything with
    run(n) -> done      one forward pass over the network input that stops after the first n plan ops (n = len(ops): the whole,
                        unstopped pass) into a prediction buffer filled with NaN beforehand; done = plan ops completed
    read(t, coff, C)    channels [coff, coff + C) of plan tensor t as that pass left them, float64 [B, C, h, w]
    pred()              the prediction buffer of that pass, float64 [B, A, 64 + nc] (NaN where nothing was written)
    variant(i)          the kernel variant that ran op i in that pass ('' when it had no launch of its own)
-- the HIP context through cy_debug_stop_after / cy_debug_ops_done / cy_debug_read_tensor (tests/test_gpu_yolo11_layers.py) or
the torch emulator below (tests/test_plan_ref_cpu.py).

THE WALK.  The inputs of op i (in0 through up0, in1, res, each a channel slice) are read after run(i), its output slice after
run(i + 1).  An in-place update (psa[pc:] += ...) therefore has its old value read before and its new value after, tensors that
several ops share (qkv / att / mix / ffn of the two PSA blocks, ta / tb / t1 of the C3k bottlenecks) are read while they hold what
the op saw, and no error travels past one op.  run(i + 1) may complete i + 2 ops: op i and op i + 1 ran as one launch (stem +
model.1, a back-to-back 1x1 pair) and op i's output was never stored.  Op i then gets layer_ref's two-step treatment: its
reference is rounded to the storage type and handed to op i + 1 with the interval within which the device's intermediate may
differ, carried through op i + 1's |w| (zero in the fp16 context away from rounding ties).  The box-branch output convolution of
a detect level that waits for its class branch (the head pair) writes nothing in the pass that stops behind it; its rows are
read from the pass that ends with the class branch, whose launch is the pair launch of the unstopped pass.

SAME LAUNCH.  The walk starts with the unstopped pass and records variant(i) of every op.  A value is compared only after the
stopped pass that produced it reports the same string for that op (and '' for an op that ran in its neighbour's launch).  At
the end the unstopped pass runs again and must reproduce the first one's prediction bytes.

BOUNDS.  Convolutions and the stem: layer_ref.conv_bound (the YOLOv8 walk's, term by term in layer_ref's docstring) on the
context's weights.  Depth-wise 3x3: dw_bound.  Attention: attn_ref / attn_bound.  5x5 max pool: bit-exact.  The last three are
the bounds of tests/test_gpu_yolo11_ops.py, which imports them from here.  No term carries a free factor; none was adjusted to
an observed output.
"""
import numpy as np
import torch
import torch.nn.functional as F
import layer_ref as LR

OPK_STEM, OPK_CONV, OPK_POOL, OPK_DWCONV, OPK_ATTN = 0, 1, 2, 3, 4
KIND = {OPK_STEM: "stem", OPK_CONV: "conv", OPK_POOL: "pool", OPK_DWCONV: "dwconv", OPK_ATTN: "attention"}
U32, E16 = 2.0 ** -24, 2.0 ** -11


# ------------------------------------------------------------------------------------------------ bounds of the non-GEMM operators
def dw_bound(prec, A, y, wsum):
    """Depth-wise 3x3 (+ SiLU)(+ residual).  A = |b| + sum_taps |x| |w| (+ |r|), y the float64 result, wsum = sum |w| per channel
    (broadcastable to y).
      fp32:   b + 9 fused multiply-adds, one rounding each of a partial sum below A: worst case 10 u A, but the roundings are
              independent and their sum stays below 5 u A; SiLU (slope <= 1.1), expf, the division and the residual add: 3 u |y|.
      fp16x3: + the split of x and r (x (1 + d), |d| <= 4 u; absolute 2^-25 sum |w| + 2^-25) and of the result (4 u |y| + 2^-25),
              again as independent roundings: 7 u A + 5 u |y| + 2^-25 (sum |w| + 2);
      fp16:   fp32-level error with the hardware exp2 / rcp SiLU (5 u A + 5 u |y|), then one fp16 rounding: + E16 |y| + 2^-25."""
    ay = y.abs()
    if prec == "fp32":
        return U32 * (5 * A + 3 * ay)
    if prec == "fp16x3":
        return U32 * (7 * A + 5 * ay) + 2.0 ** -25 * (wsum + 2)
    return U32 * (5 * A + 5 * ay) + E16 * ay + 2.0 ** -25


def dw_source_channels(C, blk, gstride, goff):
    """Input channel (relative to in0_coff) of each of the C output channels of a depth-wise op: blk = 0 the identity, else
    channel c reads (c // blk) * gstride + goff + c % blk (attn.pe: v in place inside the qkv tensor)."""
    c = torch.arange(C)
    return (c // blk) * gstride + goff + c % blk if blk else c


def attn_ref(qkv, heads, kd, hd, coff, rows=None):
    """softmax(q k^T kd^-0.5) v per head in float64, written out; rows: the query rows to compute (all keys).
    -> out [B, nrows, heads*hd], max |score|, R = the largest half spread (max_m s - min_m s) / 2 of a query's score row."""
    per = 2 * kd + hd
    outs, smax, spread = [], 0.0, 0.0
    for h in range(heads):
        o = coff + h * per
        q, k, v = qkv[..., o:o + kd], qkv[..., o + kd:o + 2 * kd], qkv[..., o + 2 * kd:o + per]
        if rows is not None:
            q = q[:, rows]
        s = torch.matmul(q, k.transpose(1, 2)) * kd ** -0.5
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        outs.append(torch.matmul(e, v) / e.sum(-1, keepdim=True))
        smax = max(smax, float(s.abs().max()))
        spread = max(spread, float((s.max(-1).values - s.min(-1).values).max()) / 2)
    return torch.cat(outs, -1), smax, spread


def attn_bound(prec, y, vmax, R):
    """Per-element bound of one attention output.  The softmax weights depend on score differences only; a computed score
    carries an error of a few u |s| (kd fused multiply-adds and the scale, or the pre-scaled q of the fast kernel), so against a
    row's centre the weights move by factors exp(+-c u R), R = half the score spread of the row, and expf, the running sums and
    the final division add a few u: the output, a convex combination of v, moves by <= u vmax (4 + 4 R).  (The worst-case form
    (kd + 2) u sum_d |q_d k_d| over N-term sums is 10-50x above every case here; the bound grows with the score range, which is
    what the rescaling of the online softmax has to survive.)  fp16x3 adds the split of q, k, v (relative 4 u: u vmax (2 + R))
    and of the output (4 u |y|); fp16 one rounding of the output (E16 |y| + 2^-25)."""
    if prec == "fp16x3":
        return U32 * vmax * (6 + 5 * R) + 4 * U32 * y.abs()
    b = torch.full_like(y, U32 * vmax * (4 + 4 * R))
    return b + E16 * y.abs() + 2.0 ** -25 if prec == "fp16" else b


# ------------------------------------------------------------------------------------------------ plan helpers
def plan_weights(g, weights, prec):
    """name -> (W, b) float64 as the context holds them: layer_ref.context_weights, except that depth-wise filters stay fp32 in
    every context (the depth-wise kernel reads an fp32 filter)."""
    cw = LR.context_weights(weights, prec)
    for cs in g.convs:
        if cs.groups != 1:
            w, b = weights[cs.name]
            cw[cs.name] = (torch.tensor(np.asarray(w), dtype=torch.float32).double(), torch.tensor(np.asarray(b), dtype=torch.float32).double())
    return cw


def op_name(g, o):
    return g.convs[o["conv"]].name if o["conv"] >= 0 else KIND[o["kind"]]


def out_channels(g, o):
    if o["kind"] == OPK_ATTN:
        return o["p0"] * o["p2"]
    return g.convs[o["conv"]].cout if o["conv"] >= 0 else o["c0"]


def level_offsets(H, W):
    """-> [(first anchor, h, w)] of the three prediction levels."""
    out, off = [], 0
    for s in (8, 16, 32):
        out.append((off, H // s, W // s))
        off += (H // s) * (W // s)
    return out


def pred_slice(pred, o, g, H, W):
    """The rows a head op (out < 0) writes: [B, A, 64 + nc] -> [B, C, h, w] (a view)."""
    off, h, w = level_offsets(H, W)[o["pred_level"]]
    C = g.convs[o["conv"]].cout
    return pred[:, off:off + h * w, o["pred_coff"]:o["pred_coff"] + C].reshape(pred.shape[0], h, w, C).permute(0, 3, 1, 2)


def conv_input(o, read):
    """The input of a convolution / stem op as the kernel assembles it: in0's slice (through a nearest x2 upsample when up0),
    then in1's slice behind it."""
    a = read(o["in0"], o["in0_coff"], o["c0"])
    if o["up0"]:
        a = F.interpolate(a, scale_factor=2, mode="nearest")
    if o["in1"] >= 0:
        a = torch.cat((a, read(o["in1"], o["in1_coff"], o["c1"])), 1)
    return a


def dw_input(o, C, read):
    src = dw_source_channels(C, o["p0"], o["p1"], o["p2"])
    return read(o["in0"], o["in0_coff"], int(src.max()) + 1)[:, src]


def attn_tokens(t):
    """[B, C, h, w] -> [B, N, C]"""
    return t.flatten(2).transpose(1, 2)


# ------------------------------------------------------------------------------------------------ the walk
class _PlanWalk(object):
    def __init__(self, g, weights, x, dev, prec, passes, tap):
        self.g, self.w, self.dev, self.prec, self.passes, self.tap = g, plan_weights(g, weights, prec), dev, prec, passes, tap
        self.x = torch.as_tensor(x, dtype=torch.float64)
        self.H, self.W = int(self.x.shape[2]), int(self.x.shape[3])
        self.report = {}

    def read(self, t, coff, C):
        if t == 0:
            return self.x[:, coff:coff + C]
        return torch.as_tensor(self.dev.read(t, coff, C), dtype=torch.float64)

    def inputs(self, i):
        """Everything op i reads, taken from the device now (before the op runs)."""
        o = self.g.ops[i]
        k = o["kind"]
        d = {}
        if k in (OPK_STEM, OPK_CONV):
            d["x"] = conv_input(o, self.read)
        elif k == OPK_DWCONV:
            d["x"] = dw_input(o, self.g.convs[o["conv"]].cout, self.read)
        elif k == OPK_ATTN:
            d["x"] = self.read(o["in0"], o["in0_coff"], o["p0"] * (2 * o["p1"] + o["p2"]))
        else:
            d["x"] = self.read(o["in0"], o["in0_coff"], o["c0"])
        if o["res"] >= 0:
            d["res"] = self.read(o["res"], o["res_coff"], out_channels(self.g, o))
        return d

    def reference(self, i, x, res, iv=None):
        """-> (y, e, st, K) of op i on input x (interval iv when x was never stored): reference, bound before the store, store term."""
        o = self.g.ops[i]
        k = o["kind"]
        if k in (OPK_STEM, OPK_CONV):
            cs = self.g.convs[o["conv"]]
            w, b = self.w[cs.name]
            assert x.shape[1] == cs.cin and cs.groups == 1 and tuple(w.shape) == (cs.cout, cs.cin, cs.k, cs.k), cs.name
            y, e, st = LR.conv_bound(cs.name, LR.Val(x, iv), w, b, cs.s, cs.act, res, self.prec, self.passes, k == OPK_STEM, o["out"] < 0)
            return y, e, st, cs.cin * cs.k * cs.k
        assert iv is None, "only a convolution may read an unmaterialised value"
        if k == OPK_DWCONV:
            cs = self.g.convs[o["conv"]]
            w, b = self.w[cs.name]
            assert cs.k == 3 and cs.s == 1 and cs.groups == cs.cout == x.shape[1]
            y = F.conv2d(x, w, b, padding=1, groups=cs.cout)
            A = F.conv2d(x.abs(), w.abs(), b.abs(), padding=1, groups=cs.cout)
            if cs.act:
                y = F.silu(y)
            if res is not None:
                y, A = y + res, A + res.abs()
            return y, dw_bound(self.prec, A, y, w.abs().sum((1, 2, 3)).view(1, -1, 1, 1)), torch.zeros_like(y), 9
        assert res is None
        if k == OPK_ATTN:
            heads, kd, hd = o["p0"], o["p1"], o["p2"]
            qkv = attn_tokens(x)
            y, _, R = attn_ref(qkv, heads, kd, hd, 0)
            per = 2 * kd + hd
            vmax = max(float(qkv[..., h * per + 2 * kd:(h + 1) * per].abs().max()) for h in range(heads))
            bound = attn_bound(self.prec, y, vmax, R)
            back = lambda t: t.transpose(1, 2).reshape(x.shape[0], heads * hd, x.shape[2], x.shape[3])
            return back(y), back(bound), torch.zeros_like(back(y)), kd
        assert k == OPK_POOL
        y = F.max_pool2d(x, 5, 1, 2)
        return y, torch.zeros_like(y), torch.zeros_like(y), 25

    def output(self, i):
        o = self.g.ops[i]
        if o["out"] < 0:
            return pred_slice(torch.as_tensor(self.dev.pred(), dtype=torch.float64), o, self.g, self.H, self.W)
        return self.read(o["out"], o["out_coff"], out_channels(self.g, o))

    def check(self, i, y, e, st, K, variant):
        got = self.output(i)
        assert tuple(got.shape) == tuple(y.shape), "op %d %s: device shape %s, reference %s" % (
            i, op_name(self.g, self.g.ops[i]), tuple(got.shape), tuple(y.shape))
        bound = e + st
        if self.g.ops[i]["kind"] == OPK_POOL:               # bit-exact: any difference is infinitely far outside
            r = LR.compare(got, y, torch.ones_like(y), K)
            r.update(ratio=0.0 if r["ratio"] == 0.0 else float("inf"), bound=0.0)
        else:
            r = LR.compare(got, y, bound, K)
        r.update(op=i, name=op_name(self.g, self.g.ops[i]), kind=KIND[self.g.ops[i]["kind"]], variant=variant)
        self.report[i] = r

    def same_launch(self, i, full):
        v = self.dev.variant(i)
        assert v == full[i], "op %d %s ran as [%s] in the stopped pass and as [%s] in the whole pass" % (
            i, op_name(self.g, self.g.ops[i]), v, full[i])
        return v

    def run(self):
        g, dev = self.g, self.dev
        N = len(g.ops)
        assert dev.run(N) == N
        full = [dev.variant(i) for i in range(N)]
        first = np.array(dev.pred(), copy=True)
        assert np.isfinite(first).all(), "the whole pass left prediction rows unwritten"
        waiting = {}                                         # pred_level -> (op, y, e, st, K) of a box branch deferred for its pair
        k, ins, iv = 0, self.inputs(0), None
        while k < N:
            o = g.ops[k]
            done = dev.run(k + 1)
            assert done in (k + 1, k + 2) and done <= N, "run(%d) completed %d ops" % (k + 1, done)
            y, e, st, K = self.reference(k, ins["x"], ins.get("res"), iv)
            if self.tap:
                self.tap(k, y, ins.get("res"))
            iv = None
            if done == k + 2:                                # op k and op k + 1 in one launch: op k was never stored
                n = g.ops[k + 1]
                assert o["kind"] in (OPK_STEM, OPK_CONV) and n["kind"] == OPK_CONV and o["out"] >= 1 and o["res"] < 0
                assert n["in0"] == o["out"] and n["in0_coff"] == o["out_coff"] and n["c0"] == out_channels(g, o)
                assert n["in1"] < 0 and n["res"] < 0 and not n["up0"]
                v = self.same_launch(k, full)
                assert v and full[k + 1] == "" and self.same_launch(k + 1, full) == ""
                self.report[k] = dict(materialised=False, ratio=None, op=k, name=op_name(g, o), kind=KIND[o["kind"]], variant=v)
                um = LR.unmaterialised(y, e, st, self.prec)
                y2, e2, st2, K2 = self.reference(k + 1, um.v, None, um.iv)
                if self.tap:
                    self.tap(k + 1, y2, None)
                self.check(k + 1, y2, e2, st2, K2, "")
            elif o["out"] < 0 and o["pred_coff"] == 0 and dev.variant(k) == "" and bool(torch.isnan(self.output(k)).all()):
                assert o["pred_level"] not in waiting
                waiting[o["pred_level"]] = (k, y, e, st, K)   # deferred for the head pair: nothing launched, nothing written
            else:
                v = self.same_launch(k, full)
                assert v, "op %d %s completed without a launch of its own" % (k, op_name(g, o))
                self.check(k, y, e, st, K, v)
                if o["out"] < 0 and o["pred_level"] in waiting:      # the class branch: the deferred box branch ran by now
                    j, yj, ej, stj, Kj = waiting.pop(o["pred_level"])
                    self.check(j, yj, ej, stj, Kj, self.same_launch(j, full))
            k = done
            if k < N:
                ins = self.inputs(k)
        assert not waiting, "box branches %s never ran" % sorted(waiting)
        assert sorted(self.report) == list(range(N)), "ops missing from the report: %s" % sorted(set(range(N)) - set(self.report))
        assert dev.run(N) == N
        again = np.array(dev.pred(), copy=True)
        assert first.tobytes() == again.tobytes(), "the whole pass after the stopped ones differs from the one before them"
        return self.report


def walk(g, weights, x, dev, prec, passes=2, tap=None):
    """g: yolo11_graph.Graph; weights: name -> (W, b) folded fp32; x: the network input [B, 3, H, W] as the device read it
    (float64); dev: the device (module docstring); prec: fp16 | fp32 | fp16x3; passes: 2 | 3, the form of the fp16x3 filters;
    tap(i, y, res): called with every op's float64 reference (and the residual it added).
    -> {op index: dict(op, name, kind, variant, materialised, ratio, pos = (b, c, row, col), got, ref, bound, K)}, one entry per
    plan op (asserted)."""
    with torch.no_grad():
        return _PlanWalk(g, weights, x, dev, prec, passes, tap).run()


def worst(rep):
    """-> (ratio, op index) of the worst materialised op."""
    return max((v["ratio"], i) for i, v in rep.items() if v["materialised"])


def failures(rep):
    return ["op %d %s [%s] at (b, c, row, col) = %s: got %.9g, reference %.9g, bound %.3g (ratio %.3f, K = %d)" % (
        i, v["name"], v["variant"] or "in its neighbour's launch", v["pos"], v["got"], v["ref"], v["bound"], v["ratio"], v["K"])
        for i, v in sorted(rep.items()) if v["materialised"] and not v["ratio"] <= 1.0]


# ------------------------------------------------------------------------------------------------ a device in torch, on the CPU
class PlanEmulator(object):
    """The plan as a context of precision fp16 / fp32 runs it, in torch on the CPU, on real buffers: one [B, C, h, w] array per
    plan tensor, ops reading and writing channel slices of them (the in-place ones and the shared ones included), operands as the
    context holds them, fp32 arithmetic, one rounding to the storage type.  prec "ref": float64 throughout, no rounding (the
    reference itself as the device).  Every pass starts from buffers full of `fill` (NaN; the fault tests use a finite value, as
    memory that an earlier pass left behind, so that a slice a faulty op failed to write does not poison its readers).  `fused`: indices of ops that run in one launch with the
    op behind them (their output goes to the reader rounded, and is never stored); `head_pair`: the box-branch output convolution
    writes its rows when the class branch of its level runs.  `faults`: {op index: (kind, ...)} seeded faults (tests)."""

    def __init__(self, g, weights, x, prec, fused=(), head_pair=False, faults=None, fill=float("nan")):
        self.g, self.prec = g, prec
        self.dt = torch.float64 if prec == "ref" else torch.float32
        cw = plan_weights(g, weights, "fp32" if prec == "ref" else prec)
        self.w = {k: (w.to(self.dt), b.to(self.dt)) for k, (w, b) in cw.items()}
        self.x = torch.as_tensor(x, dtype=self.dt)
        self.B, self.H, self.W = int(self.x.shape[0]), int(self.x.shape[2]), int(self.x.shape[3])
        self.fused, self.head_pair, self.faults = set(fused), head_pair, dict(faults or {})
        self.A = sum(h * w for _, h, w in level_offsets(self.H, self.W))
        self.hit, self.fill = set(), fill
        self.reset()

    def reset(self):
        self.t = [None] + [torch.full((self.B, C, self.H >> lev, self.W >> lev), self.fill, dtype=self.dt) for lev, C in self.g.tensors[1:]]
        self.p = torch.full((self.B, self.A, 64 + self.g.nc), float("nan"), dtype=self.dt)
        self.done, self.var, self.wait, self.snap = 0, {}, {}, {}

    # ---- the device interface
    def run(self, n):
        if n <= self.done:                                    # (a pass that stops later continues the one before: same values)
            self.reset()
        with torch.no_grad():
            while self.done < n:
                self.done += self.step(self.done)
            if n >= len(self.g.ops):
                for lvl in sorted(self.wait):
                    self.flush(lvl, solitary=True)
        return self.done

    def read(self, t, coff, C):
        assert t >= 1
        return self.t[t][:, coff:coff + C].double().clone()

    def pred(self):
        return self.p.double().clone().numpy()

    def variant(self, i):
        return self.var.get(i, "")

    # ---- execution
    def store(self, y, head=False):
        if self.prec == "fp16" and not head:
            return y.half().float()
        return y

    def src(self, t, coff, C):
        return self.x[:, coff:coff + C] if t == 0 else self.t[t][:, coff:coff + C]

    def flush(self, lvl, solitary):
        o, rows = self.wait.pop(lvl)
        pred_slice(self.p, o, self.g, self.H, self.W)[:] = rows
        if solitary:
            self.var[self.g.ops.index(o)] = "emulated head"

    def conv(self, i, o, x, res):
        cs = self.g.convs[o["conv"]]
        w, b = self.w[cs.name]
        f = self.faults.get(i, ("",))
        if f[0] == "no_bias":
            self.hit.add(i)
            b = b.clone()
            b[f[1]] = 0
        y = F.conv2d(x, w, b, stride=cs.s, padding=cs.k // 2)
        if f[0] == "tile_prev_image":                        # one 16 x 16 tile of image 1 computed from image 0's input
            self.hit.add(i)
            y = y.clone()
            y[1, :, :16, :16] = y[0, :, :16, :16]
        if cs.act:
            y = F.silu(y)
        if res is not None:
            if f[0] == "round_twice":                        # the convolution's result rounded before the residual add, and again after
                self.hit.add(i)
                y = y.half().float()
            y = y + res
        return self.store(y, o["out"] < 0)

    def step(self, i):
        g = self.g
        o = dict(g.ops[i])
        f = self.faults.get(i, ("",))
        if f[0] == "op":                                     # a wrong plan field: (field, delta) pairs
            self.hit.add(i)
            for field, delta in f[1:]:
                o[field] += delta
        if f[0] == "swap_inputs":
            self.hit.add(i)
            assert o["in1"] >= 0 and o["up0"]
        k = o["kind"]
        self.var[i] = "emulated " + KIND[k]
        if k in (OPK_STEM, OPK_CONV):
            a = self.src(o["in0"], o["in0_coff"], o["c0"])
            if o["up0"]:
                if f[0] == "up_parity":                      # source pixel (y + 1) // 2 in place of y // 2
                    self.hit.add(i)
                    idx = lambda n: torch.clamp((torch.arange(2 * n) + 1) // 2, max=n - 1)
                    a = a[:, :, idx(a.shape[2])][:, :, :, idx(a.shape[3])]
                else:
                    a = F.interpolate(a, scale_factor=2, mode="nearest")
            if o["in1"] >= 0:
                b = self.src(o["in1"], o["in1_coff"], o["c1"])
                a = torch.cat((b, a) if f[0] == "swap_inputs" else (a, b), 1)
            res = self.src(o["res"], o["res_coff"], out_channels(g, o)) if o["res"] >= 0 else None
            y = self.conv(i, o, a, res)
            if i in self.fused:
                n = g.ops[i + 1]
                y = self.conv(i + 1, n, y, None)
                self.t[n["out"]][:, n["out_coff"]:n["out_coff"] + y.shape[1]] = y
                self.var[i + 1] = ""
                return 2
            if o["out"] < 0:
                if self.head_pair and o["pred_coff"] == 0:
                    self.wait[o["pred_level"]] = (g.ops[i], y)
                    self.var[i] = ""
                    return 1
                pred_slice(self.p, o, g, self.H, self.W)[:] = y
                if o["pred_level"] in self.wait:
                    self.flush(o["pred_level"], solitary=False)
                return 1
        elif k == OPK_DWCONV:
            cs = g.convs[o["conv"]]
            w, b = self.w[cs.name]
            sc = dw_source_channels(cs.cout, o["p0"], o["p1"], o["p2"])
            a = self.src(o["in0"], o["in0_coff"], int(sc.max()) + 1)[:, sc]
            y = F.conv2d(a, w, b, padding=1, groups=cs.cout)
            if cs.act:
                y = F.silu(y)
            if o["res"] >= 0:
                y = y + self.src(o["res"], o["res_coff"], cs.cout)
            y = self.store(y)
        elif k == OPK_ATTN:
            heads, kd, hd = o["p0"], o["p1"], o["p2"]
            per = 2 * kd + hd
            a = self.src(o["in0"], o["in0_coff"], heads * per)
            self.snap[i] = a.clone()
            if f[0] == "stale_qkv":                          # the qkv an earlier attention op (f[1]) saw
                self.hit.add(i)
                a = self.snap[f[1]]
            qkv = attn_tokens(a)
            outs = []
            for h in range(heads):
                q, kk, v = qkv[..., h * per:h * per + kd], qkv[..., h * per + kd:h * per + 2 * kd], qkv[..., h * per + 2 * kd:(h + 1) * per]
                if f[0] == "k_for_v":                        # v read one block early: k's channels, then the first half of v's
                    self.hit.add(i)
                    v = qkv[..., h * per + kd:h * per + kd + hd]
                s = torch.matmul(q, kk.transpose(1, 2))
                if f[0] == "no_scale":
                    self.hit.add(i)
                else:
                    s = s * kd ** -0.5
                outs.append(torch.matmul(torch.softmax(s, -1), v))
            y = torch.cat(outs, -1).transpose(1, 2).reshape(a.shape[0], heads * hd, a.shape[2], a.shape[3])
            y = self.store(y)
        else:
            y = F.max_pool2d(self.src(o["in0"], o["in0_coff"], o["c0"]), 5, 1, 2)
        self.t[o["out"]][:, o["out_coff"]:o["out_coff"] + y.shape[1]] = y
        return 1
