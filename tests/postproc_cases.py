"""Constructed inputs for the post-processing kernels (decode, NMS, IoU merge): synthetic raw head outputs [B, 64+nc, A] of a
letterboxed H x W input, and detection lists for the merge, built so that threshold decisions land exactly where a case wants them.

* Exact boxes: every DFL side is one-hot with a margin of 120 logits.  exp(-120) underflows to 0 in fp32, so the softmax weights
  are exactly 0 and 1 (expf on the device, torch on the host) and the distances are whole grid units.  Box edges then lie on the
  lattice stride * (c + 0.5 - d), identical boxes come from different anchors, and IoUs are exact rationals computed the same
  way on both sides (class-offset coordinates stay far below 2^24).
* Exact scores: class logits are multiples of 1/16 in [-6, 6].  Two such sigmoids are either equal or some 1e-5 apart (far more
  than an fp32 ulp), in 1 / (1 + expf(-x)) and in torch.sigmoid alike; logit 0 gives 0.5 exactly.

The device takes the [B, A, 64+nc] layout (device_layout).  tests/test_postproc_cases_cpu.py checks on the oracle that every
case has the property it is built for; tests/test_gpu_postproc.py runs them through the kernels.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

MARGIN = 120.0               # DFL one-hot margin (>= 110: the other weights are exactly 0 in fp32)
LOW = -16.0                  # class logit of "no object" (sigmoid 1.1e-7: below every conf used here except 0)
STRIDES = (8, 16, 32)


def level_shapes(H, W):
    return [(H // s, W // s) for s in STRIDES]


def num_anchors(H, W):
    return sum(h * w for h, w in level_shapes(H, W))


def level_offset(H, W, lvl):
    return sum(h * w for h, w in level_shapes(H, W)[:lvl])


def anchor_index(H, W, lvl, cy, cx):
    gh, gw = level_shapes(H, W)[lvl]
    assert 0 <= cy < gh and 0 <= cx < gw
    return level_offset(H, W, lvl) + cy * gw + cx


def anchor_cell(H, W, a):
    """anchor index -> (level, cy, cx)"""
    for lvl, (gh, gw) in enumerate(level_shapes(H, W)):
        if a < gh * gw:
            return lvl, a // gw, a % gw
        a -= gh * gw
    raise IndexError(a)


def lattice_box(lvl, cy, cx, d):
    """letterboxed-pixel xyxy of the anchor (lvl, cy, cx) with whole distances d = (left, top, right, bottom)"""
    s = STRIDES[lvl]
    return (s * (cx + 0.5 - d[0]), s * (cy + 0.5 - d[1]), s * (cx + 0.5 + d[2]), s * (cy + 0.5 + d[3]))


def distances_for(lvl, cy, cx, box):
    """whole distances that make anchor (lvl, cy, cx) produce `box` exactly (asserts that it can)"""
    s = STRIDES[lvl]
    d = ((cx + 0.5) - box[0] / s, (cy + 0.5) - box[1] / s, box[2] / s - (cx + 0.5), box[3] / s - (cy + 0.5))
    for v in d:
        assert v == int(v) and 0 <= v <= 15, (lvl, cy, cx, box, d)
    return tuple(int(v) for v in d)


def coarse(logit):
    """a class logit on the 1/16 grid in [-6, 6] (or the 'no object' / saturated values)"""
    assert logit in (LOW, 100.0, -100.0) or (-6 <= logit <= 6 and logit * 16 == int(logit * 16)), logit
    return float(logit)


class Raw(object):
    """raw head output [B, 64+nc, A] fp32; every anchor starts as 'no object' with the box d = (1, 1, 1, 1)."""

    def __init__(self, B, H, W, nc):
        self.B, self.H, self.W, self.nc = B, H, W, nc
        self.A = num_anchors(H, W)
        self.raw = torch.zeros((B, 64 + nc, self.A), dtype=torch.float32)
        self.raw[:, 64:] = LOW
        self.set_dist(slice(None), slice(None), (1, 1, 1, 1))

    def set_dist(self, b, a, d):
        """whole distances of anchors a (index, slice or index array) of tile b: one-hot DFL logits"""
        for side in range(4):
            blk = self.raw[b, side * 16:(side + 1) * 16]
            blk[..., a] = 0.0
            self.raw[b, side * 16 + int(d[side]), a] = MARGIN

    def set_dists(self, b, idx, d4):
        """per-anchor distances: idx [n] anchors, d4 [n, 4] ints"""
        idx = torch.as_tensor(idx, dtype=torch.long)
        d4 = torch.as_tensor(d4, dtype=torch.long)
        for side in range(4):
            self.raw[b, side * 16:(side + 1) * 16, idx] = 0.0
            self.raw[b, side * 16 + d4[:, side], idx] = MARGIN

    def set_cls(self, b, a, cls, logit):
        """score of anchor(s) a: class `cls` at `logit`, every other class at LOW"""
        self.raw[b, 64:, a] = LOW
        self.raw[b, 64 + cls, a] = torch.as_tensor(logit, dtype=torch.float32) if not isinstance(logit, float) else coarse(logit)

    def put(self, b, lvl, cy, cx, box, cls, logit):
        """anchor (lvl, cy, cx) of tile b produces exactly `box` with class `cls` at `logit`; -> its index"""
        a = anchor_index(self.H, self.W, lvl, cy, cx)
        self.set_dist(b, a, distances_for(lvl, cy, cx, box))
        self.set_cls(b, a, cls, logit)
        return a


def device_layout(raw):
    """[B, 64+nc, A] -> [B, A, 64+nc] (cy_decode_nms' input)"""
    return raw.permute(0, 2, 1).contiguous()


# --------------------------------------------------------------------------- oracle
def oracle_decode_nms(raw, H, W, nc, conf, iou, h0=None, w0=None):
    """The oracle of cy_decode_nms: per tile (det [n,6] in original-image pixels, kept anchor indices [n], candidates)."""
    from oracle import yolov8_ref as Y
    pred = Y.decode(raw, level_shapes(H, W), nc)
    out = []
    for b, (d, a) in enumerate(Y.non_max_suppression(pred, conf, iou, nc)):
        d = d.clone()
        d[:, :4] = Y.scale_boxes(d[:, :4], (H, W), (h0 or H, w0 or W))
        out.append((d, a, int((pred[b, 4:].amax(0) > conf).sum())))
    return out


def oracle_candidates(raw, H, W, nc, conf):
    """-> per tile (class-offset xyxy [n,4] f32, scores [n], anchors [n]) of the candidates in NMS order (score desc, anchor asc),
    before the max_nms cut"""
    from oracle import yolov8_ref as Y
    pred = Y.decode(raw, level_shapes(H, W), nc)
    res = []
    for b in range(raw.shape[0]):
        p = pred[b].t()
        sc, cl = p[:, 4:].max(1)
        keep = torch.nonzero(sc > conf).flatten()
        xy, wh = p[keep, :2], p[keep, 2:4]
        box = torch.cat((xy - wh / 2, xy + wh / 2), 1) + cl[keep, None].float() * Y.MAX_WH
        o = torch.argsort(sc[keep], descending=True, stable=True)
        res.append((box[o], sc[keep][o], keep[o]))
    return res


def iou_f32(a, b):
    """torchvision-style IoU of two class-offset boxes in fp32, as nms_indices computes it"""
    a, b = torch.as_tensor(a, dtype=torch.float32), torch.as_tensor(b, dtype=torch.float32)
    xx1, yy1 = torch.maximum(a[0], b[0]), torch.maximum(a[1], b[1])
    xx2, yy2 = torch.minimum(a[2], b[2]), torch.minimum(a[3], b[3])
    inter = (xx2 - xx1).clamp(min=0) * (yy2 - yy1).clamp(min=0)
    aa = (a[2] - a[0]) * (a[3] - a[1])
    ab = (b[2] - b[0]) * (b[3] - b[1])
    return inter / (aa + ab - inter)


def blocks(n, k=16):
    """split n cells into ceil(n / k) runs of 2..k cells -> [(start, size)]"""
    m = -(-n // k)
    base, extra = divmod(n, m)
    out, s = [], 0
    for i in range(m):
        sz = base + (1 if i < extra else 0)
        assert 2 <= sz <= k
        out.append((s, sz))
        s += sz
    return out


def set_block_boxes(r, b, lvls=(0, 1, 2), k=16):
    """every anchor of the given levels gets the box shared by its block of k x k cells (edges on the block's outer cell centres
    +- 0.5: k x k anchors produce one identical box; neighbouring blocks' boxes are one cell apart).  -> {anchor: block id}"""
    H, W = r.H, r.W
    ids = 0
    idx_all, d_all, blk_all = [], [], []
    for lvl in lvls:
        gh, gw = level_shapes(H, W)[lvl]
        for y0, ny in blocks(gh, k):
            for x0, nx in blocks(gw, k):
                cy, cx = np.meshgrid(np.arange(y0, y0 + ny), np.arange(x0, x0 + nx), indexing="ij")
                cy, cx = cy.ravel(), cx.ravel()
                d = np.stack([cx - x0, cy - y0, x0 + nx - 1 - cx, y0 + ny - 1 - cy], 1)
                idx_all.append(level_offset(H, W, lvl) + cy * gw + cx)
                d_all.append(d)
                blk_all.append(np.full(len(cy), ids))
                ids += 1
    idx, d = np.concatenate(idx_all), np.concatenate(d_all)
    r.set_dists(b, idx, d)
    return dict(zip(idx.tolist(), np.concatenate(blk_all).tolist()))


# --------------------------------------------------------------------------- A: random logits, decode against float64
def random_decode_case(B, H, W, nc, seed, npos=None):
    """Random non-lattice logits over a wide range: DFL logits at scale 1, 10 or 1e4 per anchor side, class logits in [-100, 0] for
    the rejected anchors (some exactly 0: score 0.5 = conf), and for <= 300 accepted anchors a best logit in (0.25, 4] or +100
    (score 1.0 in fp32: exact ties); best logits on a 1/64 grid, so distinct scores are far apart, with some exact class ties inside one anchor.  conf = 0.5; iou = 1.0 suppresses nothing.
    -> (raw, conf, iou).  The accepted anchors' distinct scores are checked to be far apart in test_postproc_cases_cpu."""
    g = torch.Generator().manual_seed(seed)
    A = num_anchors(H, W)
    npos = min(A - 5, 300) if npos is None else npos
    raw = torch.empty((B, 64 + nc, A), dtype=torch.float32)
    scale = torch.tensor([1.0, 10.0, 1e4])[torch.randint(0, 3, (B, 4, 1, A), generator=g)]
    raw[:, :64] = (torch.randn((B, 4, 16, A), generator=g) * scale).view(B, 64, A)
    raw[:, 64:] = -100.0 * torch.rand((B, nc, A), generator=g)
    for b in range(B):
        perm = torch.randperm(A, generator=g)
        pos, neg = perm[:npos], perm[npos:]
        zero = neg[torch.rand(len(neg), generator=g) < 0.05].tolist() + [int(neg[0])]    # rejected on the threshold itself
        raw[b, 64 + torch.randint(0, nc, (len(zero),), generator=g), torch.tensor(zero)] = 0.0
        best = 0.25 + torch.randint(0, 241, (npos,), generator=g) / 64.0          # distinct scores >= 2.7e-4 apart
        sat = torch.rand(npos, generator=g) < 0.1
        sat[:2] = True
        best[sat] = 100.0
        cls = torch.randint(0, nc, (npos,), generator=g)
        raw[b, 64:, pos] = torch.minimum(raw[b, 64:, pos], best[None] - 0.5)    # every other class below the best
        raw[b, 64 + cls, pos] = best
        if nc > 1:                                                       # exact class tie inside the anchor: first maximum wins
            tie = torch.nonzero(torch.rand(npos, generator=g) < 0.2).flatten()
            tie = torch.cat([tie, torch.tensor([2])]) if 2 not in tie.tolist() else tie
            other = (cls[tie] + 1 + torch.randint(0, nc - 1, (len(tie),), generator=g)) % nc
            raw[b, 64 + other, pos[tie]] = best[tie]
    return raw, 0.5, 1.0


# --------------------------------------------------------------------------- B: NMS decisions
NMS_IOU = 0.5


def nms_decisions_case(B=2, H=256, W=256, nc=5, iou=NMS_IOU):
    """One tile of decisions, repeated with a shift of the scores per tile:
    * pairs at IoU exactly 0.5 (kept at iou = 0.5, the lower one suppressed at the next fp32 below 0.5),
    * the same geometry in two classes (never suppressed),
    * a tie group of equal scores on disjoint boxes (kept in ascending anchor order) and a tie group of identical boxes
      (only the lowest anchor is kept).
    -> (raw, info) with info['pairs'] [(higher-score anchor, lower-score anchor)], info['cross_class'], info['tie_disjoint'],
    info['tie_same']: anchors of tile 0"""
    r = Raw(B, H, W, nc)
    info = dict(pairs=[], cross_class=[], tie_disjoint=[], tie_same=[])
    for b in range(B):
        sh = b / 16.0
        # IoU 1/2: box P 2x2 cells, Q = P's left half (same x range, half the height), from the next cell
        for k in range(6):
            cy, cx = 2 + 3 * k, 2
            P = lattice_box(0, cy, cx, (1, 1, 1, 1))
            Q = (P[0], P[1], P[2], P[1] + 8.0)
            pa = r.put(b, 0, cy, cx, P, k % nc, 3.0 - k / 4.0 + sh)
            qa = r.put(b, 0, cy - 1 if k % 2 else cy, cx + 1, Q, k % nc, 2.0 - k / 4.0 + sh)
            if b == 0:
                info["pairs"].append((pa, qa))
        # IoU 1/2 the other way round: the lower anchor has the lower score
        for k in range(3):
            cy, cx = 4 + 4 * k, 8
            P = lattice_box(0, cy, cx, (2, 1, 2, 1))               # 4 x 2 cells
            Q = (P[0], P[1], P[0] + 16.0, P[3])                    # its left half
            pa = r.put(b, 0, cy, cx, P, 0, 1.5 + sh)
            qa = r.put(b, 0, cy - 1, cx - 1, Q, 0, 1.0 + sh)
            if b == 0:
                info["pairs"].append((pa, qa))
        # identical geometry, two classes
        for k in range(3):
            cy, cx = 2 + 5 * k, 14
            P = lattice_box(0, cy, cx, (1, 1, 1, 1))
            pa = r.put(b, 0, cy, cx, P, 1, 2.5 + sh)
            qa = r.put(b, 0, cy, cx + 1, P, 2, 2.0 + sh)
            if b == 0:
                info["cross_class"].append((pa, qa))
        # tie group on disjoint boxes (one cell each, touching) at the same score
        for k in range(20):
            a = r.put(b, 0, 20, 2 + k, lattice_box(0, 20, 2 + k, (0, 0, 1, 1)), 3, 0.5 + sh)
            if b == 0:
                info["tie_disjoint"].append(a)
        # tie group of identical boxes from different anchors (and levels): only the lowest anchor survives
        box = lattice_box(1, 12, 10, (2, 2, 2, 2))                 # 64 x 64 px, reachable from stride-16 rows 10..14, cols 8..12
        for (lvl, cy, cx) in [(1, 12, 10), (1, 10, 9), (1, 13, 11), (1, 11, 8), (1, 14, 12)]:
            a = r.put(b, lvl, cy, cx, box, 4, 1.25 + sh)
            if b == 0:
                info["tie_same"].append(a)
    return r.raw, info


def many_survivors_case(B=2, H=512, W=512, nc=5, n=400, seed=1, region=40):
    """n candidates on stride-8 cells of a region x region corner with random small boxes (d in 0..3, no zero-width box) and coarse scores: more than 300
    survive NMS at iou 0.5, so the 300th kept box falls inside a 64-candidate round of the scan."""
    g = np.random.default_rng(seed)
    r = Raw(B, H, W, nc)
    gh, gw = level_shapes(H, W)[0]
    for b in range(B):
        cells = g.choice(region * region, n, replace=False)
        cells = cells // region * gw + cells % region                  # dense: some boxes suppress others
        d = g.integers(0, 4, (n, 4))
        d[:, 2] = np.maximum(d[:, 2], 1 - d[:, 0])
        d[:, 3] = np.maximum(d[:, 3], 1 - d[:, 1])
        r.set_dists(b, cells, d)
        logit = g.integers(-16, 97, n) / 16.0                         # all above conf 0.25
        cls = g.integers(0, 2, n)
        for a, c, l in zip(cells.tolist(), cls.tolist(), logit.tolist()):
            r.set_cls(b, a, c, l)
    return r.raw


def count_mix_case(counts=(0, 1, 64, 65, 8192, 8193, 16000), H=1024, W=1024, nc=5, seed=2):
    """One batch whose tiles have exactly the given numbers of candidates (conf 0.01): LDS sort (<= 8192) and global-memory sort,
    per-tile key regions.  Random small boxes and coarse scores; tile b's candidates are a random anchor subset."""
    g = np.random.default_rng(seed)
    B = len(counts)
    r = Raw(B, H, W, nc)
    A = r.A
    # every anchor: random box d in 0..3 (no zero-width box)
    d = g.integers(0, 4, (B, A, 4))
    d[..., 2] = np.maximum(d[..., 2], 1 - d[..., 0])
    d[..., 3] = np.maximum(d[..., 3], 1 - d[..., 1])
    for b, n in enumerate(counts):
        r.set_dists(b, np.arange(A), d[b])
        sel = g.choice(A, n, replace=False)
        logit = torch.from_numpy(g.integers(-64, 97, n) / 16.0).float()
        cls = torch.from_numpy(g.integers(0, nc, n))
        r.raw[b, 64:, sel] = LOW
        r.raw[b, 64 + cls, sel] = logit
    return r.raw, 0.01


# --------------------------------------------------------------------------- C: more than max_nms = 30000 candidates
def big_case(B=2, H=1280, W=1280, nc=5, hi=(29900, 29950), group=200):
    """conf = 0: every anchor is a candidate (33600 at 1280^2).  Scores rise with the anchor index: an arrival-order cut at 30000
    would drop the best.  Class 0 anchors share one box per block of cells (set_block_boxes: one survivor per block at iou 0.5);
    a tie group of `group` class-1 anchors on disjoint one-cell boxes sits just below the `hi[b]` highest anchors, so it straddles
    rank 30000: its lower anchors are kept, the others are cut.  -> (raw, conf, iou, info) with info[b] = (group anchors kept,
    group anchors cut)."""
    r = Raw(B, H, W, nc)
    A = r.A
    info = []
    for b in range(B):
        set_block_boxes(r, b)
        lo = A - hi[b]                                             # the highest hi[b] anchors rank above the group
        ramp = -5.0 + np.floor(np.arange(A) * 160 / A) / 16.0          # rising, in ties of ~A/160 anchors, within [-5, 5)
        logit = torch.from_numpy(ramp).float()
        logit[lo - group:lo] = float(ramp[lo - group] - 1.0 / 16.0)    # the tie group: below every higher anchor
        logit[:lo - group] = -5.5                                  # everything below it
        r.raw[b, 64:] = LOW
        r.raw[b, 64, :] = logit
        g = np.arange(lo - group, lo)
        r.raw[b, 64, g] = LOW
        r.raw[b, 65, g] = float(ramp[lo - group] - 1.0 / 16.0)
        cells = [anchor_cell(H, W, a) for a in g]
        assert all(c[0] == 0 for c in cells)
        r.set_dists(b, g, np.array([(0, 0, 1, 1)] * group))
        n_in = 30000 - hi[b]
        info.append((g[:n_in].tolist(), g[n_in:].tolist()))
    return r.raw, 0.0, NMS_IOU, info


def aug_views_case(B=2, H=1024, W=1024, nc=5, seed=3):
    """Synthetic head outputs of the three test-time-augmentation views of an H x W input (view k's candidates all of class k, one
    box per block of cells, scores rising with the concatenated index, conf 0): more than 30000 candidates over the concatenation
    (38209 at 1024^2).  -> (raws [B, 64+nc, A_k] x 3, view level shapes, conf, iou)"""
    import augment_ref as AR
    shapes, raws = [], []
    geo = [AR.view_geometry(H, W, s) for s in AR.SCALES]
    A = [num_anchors(Hp, Wp) for _, _, Hp, Wp in geo]
    rng = AR.clip_ranges(A)
    off = np.cumsum([0] + [hi - lo for lo, hi in rng])
    tot = int(off[-1])
    for k, (_, _, Hp, Wp) in enumerate(geo):
        r = Raw(B, Hp, Wp, nc)
        lo, hi = rng[k]
        for b in range(B):
            set_block_boxes(r, b)
            conc = np.arange(r.A) - lo + off[k]                      # concatenated index (outside [lo, hi): clipped away)
            logit = -5.0 + np.floor(np.clip(conc, 0, tot - 1) * (160 - 8 * b) / tot) / 16.0
            r.raw[b, 64:] = LOW
            r.raw[b, 64 + k] = torch.from_numpy(logit).float()
        raws.append(r.raw)
        shapes.append(level_shapes(Hp, Wp))
    return raws, shapes, 0.0, NMS_IOU, tot


def oracle_augmented(raws, shapes, nc, W, conf, iou, h0, w0, H):
    """decode of the views + concatenation (augment_ref.decode_views) + non_max_suppression + scale_boxes -> per tile (det, idx)"""
    import augment_ref as AR
    from oracle import yolov8_ref as Y
    pred = AR.decode_views(raws, shapes, nc, W)
    out = []
    for d, a in Y.non_max_suppression(pred, conf, iou, nc):
        d = d.clone()
        d[:, :4] = Y.scale_boxes(d[:, :4], (H, W), (h0, w0))
        out.append((d, a))
    return out, pred


# --------------------------------------------------------------------------- D: IoU merge inputs
def merge_chain_case(n=300, seed=4):
    """n boxes in one class on a row, each overlapping the next at IoU 1/3 (soft 0.3 links them), broken into chains whose
    boundaries do not align with the 64-bit words; coarse scores with ties.  -> (xyxy [n,4], conf [n], cls [n])"""
    g = np.random.default_rng(seed)
    xyxy = np.zeros((n, 4), np.float32)
    breaks = {50, 130, 131, 200, 263}
    x = 0.0
    for i in range(n):
        if i in breaks:
            x += 64.0                                              # a gap: next chain
        xyxy[i] = (x, 0.0, x + 16.0, 16.0)
        x += 8.0                                                   # overlap 8 of 16: IoU 8*16 / (2*256 - 128) = 1/3
    conf = (g.integers(8, 16, n) / 16.0).astype(np.float32)
    cls = np.zeros(n, np.int32)
    return xyxy, conf, cls


def merge_preorder_case():
    """Components whose DFS preorder differs from index order, with tied maximum scores (soft 0.3, one class): the first maximum
    in PREORDER survives.  Component 1: edges 0-2, 0-3, 1-3 (IoU 1/2) -> preorder 0, 2, 3, 1 (0, 3, 1, 2 if the walk took the
    highest neighbour); maximum tied at 1 and 2.  Component 2: intervals in x order 4, 9, 5, 8, 6, 7 overlapping their
    neighbours at IoU 1/3 -> preorder 4, 9, 5, 8, 6, 7; maximum tied at 5 and 9.  -> (xyxy, conf, cls)"""
    xyxy = [(0, 0, 40, 40), (0, 0, 20, 20), (0, 20, 40, 40), (0, 0, 40, 20)]
    conf = [0.5, 0.875, 0.875, 0.625]
    pos = {4: 0, 9: 1, 5: 2, 8: 3, 6: 4, 7: 5}
    for v in range(4, 10):
        x = 1000.0 + 20.0 * pos[v]
        xyxy.append((x, 0, x + 40, 40))
    conf += [0.25, 0.75, 0.5, 0.5, 0.625, 0.75]
    return np.array(xyxy, np.float32), np.array(conf, np.float32), np.zeros(len(conf), np.int32)


def merge_threshold_case():
    """Pairs at IoU exactly 1/2 (same class: the soft test), exactly 3/4 (different classes: the hard test), touching boxes
    (IoU 0), and a score exactly equal to score_thr = 0.5.  -> (xyxy, conf, cls)"""
    xyxy = [(0, 0, 40, 40), (0, 0, 40, 20),              # same class, IoU 1/2
            (100, 0, 140, 40), (100, 0, 130, 40),        # classes 0 / 1, IoU 3/4
            (200, 0, 240, 40), (240, 0, 280, 40),        # touching (IoU 0), same class
            (300, 0, 340, 40), (400, 0, 440, 40)]        # the second alone, at score == score_thr
    conf = [0.75, 0.625, 0.75, 0.875, 0.625, 0.75, 0.5625, 0.5]
    cls = [0, 0, 0, 1, 2, 2, 3, 3]
    return np.array(xyxy, np.float32), np.array(conf, np.float32), np.array(cls, np.int32)


def merge_dense_case(n=300, seed=5):
    """n random overlapping boxes in three classes in a 200 px square, coarse scores with ties: dense adjacency, large
    components."""
    g = np.random.default_rng(seed)
    x1 = g.integers(0, 200, n).astype(np.float32)
    y1 = g.integers(0, 200, n).astype(np.float32)
    w = g.integers(4, 60, n).astype(np.float32)
    h = g.integers(4, 60, n).astype(np.float32)
    xyxy = np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32)
    conf = (g.integers(4, 16, n) / 16.0).astype(np.float32)
    cls = g.integers(0, 3, n).astype(np.int32)
    return xyxy, conf, cls
