"""The constructed post-processing cases (tests/postproc_cases.py) have the properties they are built for, checked on the CPU
oracle (oracle/yolov8_ref decode / non_max_suppression / scale_boxes, oracle/postproc_ref.process_detections), so that a failure
of tests/test_gpu_postproc.py cannot be a broken case.  Also: the context refuses inputs the NMS sort key cannot index."""
import ctypes as C
import numpy as np
import pytest
import torch
import postproc_cases as P
from oracle import yolov8_ref as Y
from oracle import postproc_ref as R


def test_one_hot_dfl_gives_exact_lattice_boxes():
    r = P.Raw(1, 64, 96, 3)
    a = r.put(0, 1, 2, 3, P.lattice_box(1, 2, 3, (3, 0, 15, 2)), 2, 0.0)
    pred = Y.decode(r.raw, P.level_shapes(64, 96), 3)[0, :, a]
    cx, cy, w, h = pred[:4].tolist()
    assert (cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2) == P.lattice_box(1, 2, 3, (3, 0, 15, 2))
    assert float(pred[4 + 2]) == 0.5                                  # logit 0: score exactly 0.5
    assert float(pred[4]) == float(torch.sigmoid(torch.tensor(P.LOW)))


def _kept_before_cut(raw, H, W, nc, conf, iou):
    """the oracle's NMS without its [:300] cut: kept anchors per tile"""
    out = []
    for box, sc, anc in P.oracle_candidates(raw, H, W, nc, conf):
        box, sc, anc = box[:Y.MAX_NMS], sc[:Y.MAX_NMS], anc[:Y.MAX_NMS]
        out.append(anc[Y.nms_indices(box, sc, iou)] if len(sc) else anc)
    return out


@pytest.mark.parametrize("H,W,nc", [(32, 32, 5), (416, 512, 80), (1280, 1280, 1)])
def test_random_decode_case(H, W, nc):
    raw, conf, iou = P.random_decode_case(2, H, W, nc, seed=H + nc)
    pred = Y.decode(raw, P.level_shapes(H, W), nc)
    sc = pred[:, 4:].amax(1)
    assert bool((sc == conf).any())                                   # a score exactly on the threshold (rejected)
    for b, (d, a, ncand) in enumerate(P.oracle_decode_nms(raw, H, W, nc, conf, iou)):
        assert 0 < ncand <= 300 and d.shape[0] == ncand               # iou = 1: every candidate is kept
        s = torch.unique(d[:, 4]).double()                           # distinct scores are far apart (order cannot flip)
        assert len(s) < 2 or float((s[1:] - s[:-1]).min()) > 1e-5
        assert bool((d[:, 4] == 1.0).sum() >= 2)                      # exact ties at 1.0
        if nc > 1:                                                    # exact class ties inside an anchor: the first class wins
            cl = pred[b, 4:, a]
            tie = (cl == cl.amax(0)).sum(0) > 1
            assert int(tie.sum()) > 0
            first = torch.argmax((cl == cl.amax(0)).int(), 0)
            assert torch.equal(d[:, 5].long(), first)


def test_nms_decisions_case():
    raw, info = P.nms_decisions_case()
    cands = P.oracle_candidates(raw, 256, 256, 5, 0.25)[0]
    pos = {int(a): i for i, a in enumerate(cands[2])}
    half = np.float32(P.NMS_IOU)
    for hi, lo in info["pairs"]:
        assert float(cands[1][pos[hi]]) > float(cands[1][pos[lo]])
        assert float(P.iou_f32(cands[0][pos[hi]], cands[0][pos[lo]])) == half        # exactly on the threshold
    for p, q in info["cross_class"]:
        assert torch.equal(cands[0][pos[p]] - 1 * Y.MAX_WH, cands[0][pos[q]] - 2 * Y.MAX_WH)
    below = float(np.nextafter(half, np.float32(0)))
    k_on = set(P.oracle_decode_nms(raw, 256, 256, 5, 0.25, float(half))[0][1].tolist())
    k_below = set(P.oracle_decode_nms(raw, 256, 256, 5, 0.25, below)[0][1].tolist())
    for hi, lo in info["pairs"]:
        assert hi in k_on and lo in k_on and hi in k_below and lo not in k_below
    for p, q in info["cross_class"]:
        assert {p, q} <= k_on and {p, q} <= k_below
    ties = info["tie_disjoint"]
    assert len({float(cands[1][pos[a]]) for a in ties}) == 1 and set(ties) <= k_on
    kept = P.oracle_decode_nms(raw, 256, 256, 5, 0.25, float(half))[0][1].tolist()
    assert [a for a in kept if a in ties] == sorted(ties)
    same = info["tie_same"]
    assert len({tuple(cands[0][pos[a]].tolist()) for a in same}) == 1
    assert [a for a in kept if a in same] == [min(same)]


def test_many_survivors_case():
    raw = P.many_survivors_case()
    for b, kept in enumerate(_kept_before_cut(raw, 512, 512, 5, 0.25, P.NMS_IOU)):
        assert 300 < len(kept) < 400                                 # some suppressed, more than max_det survive
        cands = P.oracle_candidates(raw, 512, 512, 5, 0.25)[b][2].tolist()
        r300 = cands.index(int(kept[299]))                           # rank of the 300th kept box in the scan order
        assert r300 % 64 not in (0, 63) and r300 > 300


def test_count_mix_case():
    raw, conf = P.count_mix_case()
    counts = [int((Y.decode(raw[b:b + 1], P.level_shapes(1024, 1024), 5)[0, 4:].amax(0) > conf).sum()) for b in range(raw.shape[0])]
    assert counts == [0, 1, 64, 65, 8192, 8193, 16000]
    raw, conf = P.count_mix_case(counts=tuple(8400 - 13 * b for b in range(16)), H=640, W=640, seed=7)
    assert min(int((Y.decode(raw[b:b + 1], P.level_shapes(640, 640), 5)[0, 4:].amax(0) > conf).sum()) for b in range(16)) > 8192


def test_big_case_straddles_max_nms():
    raw, conf, iou, info = P.big_case()
    A = P.num_anchors(1280, 1280)
    assert A == 33600 > Y.MAX_NMS
    res = P.oracle_decode_nms(raw, 1280, 1280, 5, conf, iou)
    cands = P.oracle_candidates(raw, 1280, 1280, 5, conf)
    for b, ((d, a, ncand), (kin, kout)) in enumerate(zip(res, info)):
        assert ncand == A
        sc = cands[b][1]
        assert float(sc[Y.MAX_NMS - 1]) == float(sc[Y.MAX_NMS])     # a tie group straddles rank 30000
        kept = a.tolist()
        assert 0 < len(kept) < Y.MAX_DET
        assert set(kin) <= set(kept) and not set(kout) & set(kept)
        assert float(d[0, 4]) == float(sc[0]) and float(sc[0]) > float(sc[-1])      # the best candidate first
        assert min(kept) >= min(kin)


def test_aug_views_case():
    import augment_ref as AR
    raws, shapes, conf, iou, tot = P.aug_views_case()
    assert tot == 38209
    res, pred = P.oracle_augmented(raws, shapes, 5, 1024, conf, iou, 1000, 1024, 1024)
    assert pred.shape[-1] == tot
    for b, (d, a) in enumerate(res):
        assert 0 < len(a) < Y.MAX_DET
        assert float(d[0, 4]) == float(pred[b, 4:].amax())
        assert set(d[:, 5].long().tolist()) == {0, 1, 2}              # all three views survive
        sc = torch.sort(pred[b, 4:].amax(0), descending=True)[0]
        assert float(sc[Y.MAX_NMS - 1]) > float(sc[-1])              # the cut at 30000 drops the lowest scores
    # the flipped view (class 1) is mirrored with view 0's width: its boxes lie inside the 1024 px frame only that way
    assert float(res[0][0][res[0][0][:, 5] == 1][:, 2].max()) > 864 / 0.83 * 0.9


def test_merge_cases_on_the_reference():
    xyxy, conf, cls = P.merge_preorder_case()
    _, _, _, keep = R.process_detections(xyxy, conf, cls, 0.25, 0.3, 0.9)
    assert keep.tolist() == [2, 9]                                    # first maximum in DFS preorder, not in index order
    cc = R.connected_components(10, [(0, 2), (0, 3), (1, 3), (4, 9), (5, 9), (5, 8), (6, 8), (6, 7)])
    assert cc == [[0, 2, 3, 1], [4, 9, 5, 8, 6, 7]]
    assert R.get_iou(xyxy[0], xyxy[2]) == 0.5 and R.get_iou(xyxy[1], xyxy[3]) == 0.5 and R.get_iou(xyxy[0], xyxy[1]) == 0.25
    xyxy, conf, cls = P.merge_threshold_case()
    assert R.get_iou(xyxy[0], xyxy[1]) == 0.5 and R.get_iou(xyxy[2], xyxy[3]) == 0.75 and R.get_iou(xyxy[4], xyxy[5]) == 0.0
    on = R.process_detections(xyxy, conf, cls, 0.5, 0.5, 0.75)[3].tolist()
    off = R.process_detections(xyxy, conf, cls, 0.5, float(np.nextafter(0.5, 1)), float(np.nextafter(0.75, 1)))[3].tolist()
    assert on == [0, 3, 4, 5, 6, 7] and off == [0, 1, 2, 3, 4, 5, 6, 7]
    assert R.process_detections(xyxy, conf, cls, 0.5, 0.0, 0.75)[3].tolist() == [3, 5, 6]          # soft 0: every same-class pair
    xyxy, conf, cls = P.merge_chain_case()
    keep = R.process_detections(xyxy, conf, cls, 0.25, 0.3, 0.9)[3]
    assert len(keep) == 6                                             # six chains, across the 64-bit words


def test_context_refuses_inputs_beyond_the_sort_key():
    """cy_create refuses max_h x max_w with more than CY_MAX_CAND = 65535 anchors (1792 x 1792: 65856) and max_cand above it,
    before it touches a device; the augmented geometry reaches the limit from 1376 x 1376 (cy_enable_augment refuses it,
    tests/test_gpu_boundary.py)."""
    from caesar_yolo_amd import lib as L
    lib = L.load()
    assert lib.cy_num_anchors(1760, 1760) == 63525 and lib.cy_num_anchors(1792, 1792) == 65856
    for (h, w, mc) in [(1792, 1792, 0), (1792, 1792, 1000), (64, 64000, 0), (640, 640, 65536)]:
        ctx = C.c_void_p()
        cfg = L.cy_config(L.F32, 1, h, w, mc)
        assert lib.cy_create(0, C.byref(cfg), C.byref(ctx)) == -1, (h, w, mc)        # CY_ERR_ARG
        msg = lib.cy_last_error(None).decode()
        assert "65535" in msg and "sort key" in msg, msg
    assert L.augment_geometry(1344, 1344)[1] == 65210 and L.augment_geometry(1376, 1376)[1] == 68401
