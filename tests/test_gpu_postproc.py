"""decode_kernel, decode_augmented_kernel, nms_kernel and iou_merge_kernel on constructed edge cases (tests/postproc_cases.py, whose
properties test_postproc_cases_cpu.py checks on the oracle): exact score ties, IoUs exactly on the thresholds, scores exactly on
conf / score_thr, more than 300 survivors, mixed candidate counts in one batch, more than max_nms = 30000 candidates, DFS preorder
and word boundaries of the merge.  Kept index lists (order included) and classes must equal the oracle's exactly, boxes and
scores within 1e-4 * max(1, |x|) (decode / NMS) or bit for bit (IoU merge).  Outputs start as NaN / -7 sentinels: nothing may be
written past the count."""
import numpy as np
import pytest
import torch
from gpu_common import detector
import postproc_cases as P
from oracle import yolov8_ref as Y
from oracle import postproc_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-4
U = 2.0 ** -24                       # unit roundoff of fp32


def _det(nc=5):
    return detector("fp32", max_batch=16, max_imgsz=1280, scale="n", nc=nc)


def _sentinels(B, dev):
    return (torch.full((B, 300, 6), float("nan"), device=dev), torch.full((B, 300), -7, dtype=torch.int32, device=dev),
            torch.full((B,), -7, dtype=torch.int32, device=dev))


def _check_tail(d, a, n, b):
    assert 0 <= n <= 300
    assert torch.isnan(d[b, n:]).all(), "written past the count"
    assert bool((a[b, n:] == -7).all()), "written past the count"
    assert not torch.isnan(d[b, :n]).any()


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= TOL * np.maximum(1.0, np.abs(b)))


def _decode_nms(det, raw, H, W, conf, iou, h0=None, w0=None):
    B = raw.shape[0]
    out = _sentinels(B, det.tdev)
    det.decode_nms(P.device_layout(raw).to(det.tdev), H, W, h0 or H, w0 or W, conf, iou, out=out)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def _same_as_oracle(got, ref, what=""):
    d, a, cnt = got
    for b, (dr, ar) in enumerate(ref):
        n = int(cnt[b])
        _check_tail(d, a, n, b)
        assert n == dr.shape[0], (what, b, n, dr.shape[0])
        assert a[b, :n].tolist() == ar.tolist(), (what, b)                     # kept index set AND order
        assert np.array_equal(d[b, :n, 5].numpy(), dr[:, 5].numpy()), (what, b)
        assert _close(d[b, :n, :4].numpy(), dr[:, :4].numpy()), (what, b)
        assert _close(d[b, :n, 4].numpy(), dr[:, 4].numpy()), (what, b)


def _oracle(raw, H, W, nc, conf, iou, h0=None, w0=None):
    return [(d, a) for d, a, _ in P.oracle_decode_nms(raw, H, W, nc, conf, iou, h0, w0)]


# ------------------------------------------------------------------------------------------------ A: decode against float64
# Error bound of a decoded coordinate (derived from the fp32 operation count of decode_kernel, contraction off):
#  * a DFL side: e_k = expf(q_k - m) carries <= (|q_k - m| + 2) u relative error (the subtraction rounds at most |q_k - m| u,
#    expf within 1 ulp); since p_k = e_k / s <= exp(q_k - m), sum_k p_k |q_k - m| <= 16 / e.  The 16-term sum s adds <= 15 u,
#    the division u, and acc = sum p_k k (<= 15) another 16 * 15 u of summation:  E_d <= 15 (16/e + 3 + 15 + 1) u + 240 u < 600 u
#    grid units.
#  * the box: x1 = ax - d0, x2 = ax + d2, the centre, the width, the product by the stride and the final cx -+ w/2 are 7 roundings
#    of values <= |x| + 32 * 16 px:  |dx| <= stride * 2 E_d + 8 u (|x| + 512).
#  * a score 1 / (1 + expf(-x)): expf within 1 ulp, the sum and the division: <= 4 u relative.
E_D = 600 * U


@pytest.mark.parametrize("nc", [1, 5, 80])
@pytest.mark.parametrize("H,W", [(32, 32), (416, 512), (640, 640), (1280, 1280)])
def test_decode_matches_float64(H, W, nc):
    """Random non-lattice logits (DFL at scale 1 / 10 / 1e4, class logits down to -100 and +100), iou = 1 (nothing suppressed),
    conf = 0.5 with scores exactly 0.5 present (rejected) and exact class ties inside an anchor (first class wins): the output is
    every candidate in score order, equal to the fp32 oracle's list, boxes and scores within the derived bound of float64."""
    det = _det(nc)
    raw, conf, iou = P.random_decode_case(2, H, W, nc, seed=H + W + nc)
    got = _decode_nms(det, raw, H, W, conf, iou)
    ref = _oracle(raw, H, W, nc, conf, iou)
    d, a, cnt = got
    pred64 = Y.decode(raw.double(), P.level_shapes(H, W), nc)
    _, strides = Y.make_anchors(P.level_shapes(H, W))
    worst_b = worst_s = 0.0
    for b, (dr, ar) in enumerate(ref):
        n = int(cnt[b])
        _check_tail(d, a, n, b)
        assert n == dr.shape[0] and a[b, :n].tolist() == ar.tolist()
        assert np.array_equal(d[b, :n, 5].numpy(), dr[:, 5].numpy())
        idx = a[b, :n].long()
        p = pred64[b][:, idx]
        box = torch.stack([p[0] - p[2] / 2, p[1] - p[3] / 2, p[0] + p[2] / 2, p[1] + p[3] / 2], 1)
        box = Y.scale_boxes(box, (H, W), (H, W))
        st = strides[0, idx].double()[:, None]
        bound = st * 2 * E_D + 8 * U * (box.abs() + 512)
        err = (d[b, :n, :4].double() - box).abs()
        assert bool((err <= bound).all()), float((err / bound).max())
        sc = p[4:].amax(0)
        serr = (d[b, :n, 4].double() - sc).abs()
        sbound = 4 * U * sc
        assert bool((serr <= sbound).all()), float((serr / sbound).max())
        worst_b = max(worst_b, float((err / bound).max()))
        worst_s = max(worst_s, float((serr / sbound).max()))
    print("decode %dx%d nc=%d: %s candidates; worst box error %.3f of the bound, score %.3f" % (H, W, nc, cnt.tolist(), worst_b, worst_s))


# ------------------------------------------------------------------------------------------------ B: NMS decisions
def test_nms_threshold_ties_and_classes():
    """IoU exactly 0.5 at iou = 0.5: kept (strict >); at the next fp32 below 0.5: suppressed.  Identical geometry in two classes:
    never suppressed.  Equal scores: ascending anchor order; identical boxes at equal scores: only the lowest anchor survives."""
    det = _det()
    raw, info = P.nms_decisions_case()
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    for iou in (0.5, below):
        got = _decode_nms(det, raw, 256, 256, 0.25, iou)
        _same_as_oracle(got, _oracle(raw, 256, 256, 5, 0.25, iou), "iou %r" % iou)
        kept = got[1][0, :int(got[2][0])].tolist()
        for hi, lo in info["pairs"]:
            assert hi in kept and (lo in kept) == (iou == 0.5)
        for p, q in info["cross_class"]:
            assert p in kept and q in kept
        assert [x for x in kept if x in info["tie_disjoint"]] == sorted(info["tie_disjoint"])
        assert [x for x in kept if x in info["tie_same"]] == [min(info["tie_same"])]


def test_nms_more_than_300_survivors():
    """Over 300 boxes survive; the 300th kept sits inside a 64-candidate round of the scan: exactly the oracle's first 300."""
    det = _det()
    raw = P.many_survivors_case()
    got = _decode_nms(det, raw, 512, 512, 0.25, P.NMS_IOU)
    assert got[2].tolist() == [300, 300]
    _same_as_oracle(got, _oracle(raw, 512, 512, 5, 0.25, P.NMS_IOU))


def test_nms_mixed_candidate_counts_in_one_batch():
    """Tiles of 0, 1, 64, 65, 8192, 8193 and 16000 candidates in one launch: the LDS sort, the global-memory sort and the per-tile
    key regions of the latter."""
    det = _det()
    raw, conf = P.count_mix_case()
    got = _decode_nms(det, raw, 1024, 1024, conf, P.NMS_IOU)
    assert got[2].tolist()[:3] == [0, 1, 64]
    _same_as_oracle(got, _oracle(raw, 1024, 1024, 5, conf, P.NMS_IOU))
    assert det.counters()["cand_overflow_tiles"] == 0


def test_nms_global_sort_key_regions_of_16_tiles():
    """Sixteen tiles of 8193..8400 candidates (640^2): every tile sorts in its own global-memory key region, and tiles b and b + 8
    run side by side whichever way the workgroups are spread over the chip."""
    det = _det()
    counts = tuple(8400 - 13 * b for b in range(16))
    raw, conf = P.count_mix_case(counts=counts, H=640, W=640, seed=7)
    got = _decode_nms(det, raw, 640, 640, conf, P.NMS_IOU)
    _same_as_oracle(got, _oracle(raw, 640, 640, 5, conf, P.NMS_IOU))


@pytest.mark.parametrize("h0,w0", [(300, 517), (517, 300), (512, 512)])
def test_letterbox_undo_against_float64(h0, w0):
    """scale_boxes + clip_boxes for non-square originals, boxes running off the image: within 1e-4 of float64."""
    det = _det()
    raw = P.many_survivors_case()
    got = _decode_nms(det, raw, 512, 512, 0.25, P.NMS_IOU, h0, w0)
    ref = _oracle(raw, 512, 512, 5, 0.25, P.NMS_IOU, h0, w0)
    _same_as_oracle(got, ref)
    pred64 = Y.decode(raw.double(), P.level_shapes(512, 512), 5)
    d, a, cnt = got
    clipped = 0
    for b in range(raw.shape[0]):
        n = int(cnt[b])
        p = pred64[b][:, a[b, :n].long()]
        box = torch.stack([p[0] - p[2] / 2, p[1] - p[3] / 2, p[0] + p[2] / 2, p[1] + p[3] / 2], 1)
        clipped += int(((box < 0).any(1)).sum())
        box = Y.scale_boxes(box, (512, 512), (h0, w0))
        assert _close(d[b, :n, :4].numpy(), box.numpy())
    assert clipped > 0


# ------------------------------------------------------------------------------------------------ C: more than 30000 candidates
def test_more_than_max_nms_candidates_plain():
    """1280^2, conf 0: 33600 candidates per tile, scores rising with the anchor index, a tie group straddling rank 30000.  The
    default capacity holds them all; NMS keeps ultralytics' top 30000 by (score, anchor): no overflow, the oracle's list."""
    det = _det()
    raw, conf, iou, info = P.big_case()
    det.counters(reset=True)
    got = _decode_nms(det, raw, 1280, 1280, conf, iou)
    assert det.counters()["cand_overflow_tiles"] == 0
    _same_as_oracle(got, _oracle(raw, 1280, 1280, 5, conf, iou))
    for b, (kin, kout) in enumerate(info):
        kept = set(got[1][b, :int(got[2][b])].tolist())
        assert set(kin) <= kept and not set(kout) & kept


def test_more_than_max_nms_candidates_augmented():
    """Three synthetic views of a 1024^2 input (38209 concatenated candidates at conf 0, view k in class k) through
    decode_nms_augmented: clip ranges, concatenated index, the mirror with view 0's width, the division by s, and the top-30000 cut
    against augment_ref's restatement; no overflow."""
    det = _det()
    raws, shapes, conf, iou, tot = P.aug_views_case()
    det.counters(reset=True)
    B = raws[0].shape[0]
    out = _sentinels(B, det.tdev)
    det.decode_nms_augmented([P.device_layout(r).to(det.tdev) for r in raws], 1024, 1024, 1000, 1024, conf, iou, out=out)
    torch.cuda.synchronize()
    got = [t.cpu() for t in out]
    assert det.counters()["cand_overflow_tiles"] == 0
    ref, _ = P.oracle_augmented(raws, shapes, 5, 1024, conf, iou, 1000, 1024, 1024)
    _same_as_oracle(got, ref, "augmented")


# ------------------------------------------------------------------------------------------------ D: IoU merge, bit-exact
def _merge(det, tiles, score_thr, soft, hard):
    """tiles: list of (xyxy, conf, cls) -> per tile (out rows, source rows); NaN / -7 sentinels checked"""
    B = len(tiles)
    d = torch.full((B, 300, 6), float("nan"))
    cnt = torch.zeros((B,), dtype=torch.int32)
    for b, (x, c, k) in enumerate(tiles):
        n = len(c)
        d[b, :n, :4] = torch.from_numpy(np.asarray(x, np.float32))
        d[b, :n, 4] = torch.from_numpy(np.asarray(c, np.float32))
        d[b, :n, 5] = torch.from_numpy(np.asarray(k, np.float32))
        cnt[b] = n
    out = (torch.full((B, 300, 6), float("nan"), device=det.tdev), torch.full((B,), -7, dtype=torch.int32, device=det.tdev),
           torch.full((B, 300), -7, dtype=torch.int32, device=det.tdev))
    det.iou_merge(d.to(det.tdev), cnt.to(det.tdev), float(np.float32(score_thr)), float(soft), float(hard), out=out)
    torch.cuda.synchronize()
    o, oc, osrc = [t.cpu() for t in out]
    res = []
    for b in range(B):
        m = int(oc[b])
        assert 0 <= m <= 300 and torch.isnan(o[b, m:]).all() and bool((osrc[b, m:] == -7).all())
        res.append((o[b, :m].numpy(), osrc[b, :m].numpy()))
    return res


def _merge_same(got, tile, score_thr, soft, hard, what=""):
    x, c, k = tile
    rb, rs, rc, keep = R.process_detections(x, c, k, np.float32(score_thr), soft, hard)
    o, src = got
    assert src.tolist() == keep.tolist(), what
    assert np.array_equal(o[:, :4], rb) and np.array_equal(o[:, 4], rs) and np.array_equal(o[:, 5].astype(np.int32), rc), what


def test_merge_preorder_and_tied_maxima():
    det = _det()
    tile = P.merge_preorder_case()
    got = _merge(det, [tile], 0.25, 0.3, 0.9)[0]
    _merge_same(got, tile, 0.25, 0.3, 0.9)
    assert got[1].tolist() == [2, 9]


@pytest.mark.parametrize("soft,hard", [(0.5, 0.75), (float(np.nextafter(0.5, 1)), float(np.nextafter(0.75, 1))), (0.0, 0.75)])
def test_merge_thresholds_touching_and_score_thr(soft, hard):
    """IoU exactly soft (same class) and hard (two classes) merge (>=), one double step above does not; touching boxes have IoU 0
    (merged only at soft 0, where every same-class pair merges); a score exactly score_thr is kept."""
    det = _det()
    tile = P.merge_threshold_case()
    got = _merge(det, [tile], 0.5, soft, hard)[0]
    _merge_same(got, tile, 0.5, soft, hard)
    if soft > 0:
        assert 7 in got[1].tolist()                                        # alone at score == score_thr: kept


def test_merge_300_boxes_chains_across_words_and_batch_counts():
    """300 boxes in chains that cross the 64-bit adjacency words; a batch of tiles with 0, 1, 150 and 300 detections."""
    det = _det()
    chain = P.merge_chain_case()
    dense = P.merge_dense_case()
    tiles = [tuple(v[:0] for v in dense), tuple(v[:1] for v in dense), tuple(v[:150] for v in dense), chain]
    got = _merge(det, tiles, 0.25, 0.3, 0.9)
    for b, t in enumerate(tiles):
        _merge_same(got[b], t, 0.25, 0.3, 0.9, "tile %d" % b)
    assert len(got[3][1]) == 6 and len(got[0][1]) == 0 and len(got[1][1]) == 1


def test_merge_drops_and_counts_degenerate_boxes():
    """Degenerate boxes (x1 >= x2 or y1 >= y2) are dropped and counted (the reference would abort on them); the rest merges as the
    reference does on the list without them."""
    det = _det()
    x, c, k = P.merge_dense_case(120, seed=6)
    bad = [3, 50, 51, 119]
    x = x.copy()
    x[3, 2] = x[3, 0]                      # zero width
    x[50, 3] = x[50, 1] - 1                # negative height
    x[51, :] = 10                          # a point
    x[119, 0] = x[119, 2] + 5
    det.counters(reset=True)
    o, src = _merge(det, [(x, c, k)], 0.25, 0.3, 0.9)[0]
    assert det.counters()["degenerate_boxes"] == len(bad)
    good = np.array([i for i in range(len(c)) if i not in bad])
    rb, rs, rc, keep = R.process_detections(x[good], c[good], k[good], np.float32(0.25), 0.3, 0.9)
    assert src.tolist() == good[keep].tolist()
    assert np.array_equal(o[:, :4], rb) and np.array_equal(o[:, 4], rs)


# ------------------------------------------------------------------------------------------------ E: race screen
def test_repeated_runs_are_bit_identical():
    """A dense 300-box merge and a more-than-8192-candidate NMS, ten times each: the same bits every time."""
    det = _det()
    dense = P.merge_dense_case()
    first = _merge(det, [dense, P.merge_chain_case()], 0.25, 0.3, 0.9)
    _merge_same(first[0], dense, 0.25, 0.3, 0.9)
    raw, conf = P.count_mix_case(counts=(16000, 8193))
    nfirst = _decode_nms(det, raw, 1024, 1024, conf, P.NMS_IOU)
    for _ in range(9):
        again = _merge(det, [dense, P.merge_chain_case()], 0.25, 0.3, 0.9)
        for (o1, s1), (o2, s2) in zip(first, again):
            assert np.array_equal(o1.view(np.int32), o2.view(np.int32)) and np.array_equal(s1, s2)
        n2 = _decode_nms(det, raw, 1024, 1024, conf, P.NMS_IOU)
        for t1, t2 in zip(nfirst, n2):
            assert torch.equal(t1.view(torch.int32) if t1.dtype == torch.float32 else t1,
                               t2.view(torch.int32) if t2.dtype == torch.float32 else t2)
