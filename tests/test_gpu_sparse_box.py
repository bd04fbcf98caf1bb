"""The box branch of the detect head at candidate anchors only (cy_sparse_box.hip; plain detect path of the fp16 context).

decode_kernel reads an anchor's 64 box logits only when its best class score passes `conf`, so cy_detect_tiles computes the
branch (model.22.cv2.l: 3x3, 3x3, 1x1) only there.  A candidate's logits must be the SAME BITS the dense kernels write, so no
detection can change: checked per level on the raw prediction rows (cy_debug_sparse_box into a NaN-filled buffer against
cy_forward) and on the detect path itself (CY_SPARSE_BOX=0 against =2)."""
import numpy as np
import pytest
import torch
from gpu_common import detector

pytestmark = pytest.mark.gpu
_CACHE = {}


def _sky():
    """2048 x 2048 px of the benchmark's synthetic sky (seeded)"""
    from caesar_yolo_amd import synth
    if "sky" not in _CACHE:
        _CACHE["sky"] = synth.make_mosaic(2048, seed=20260104, zero_block=0)
    return _CACHE["sky"]


def _cfg():
    from caesar_yolo_amd import preprocessing as PP
    return PP.DataPreprocessor([PP.ZScaleTransformer([0.25] * 3), PP.MinMaxNormalizer(0, 255)]).program()


def _best(dense):
    """best class score per anchor, float64 sigmoid of the dense class logits: [B, A]"""
    return (1.0 / (1.0 + np.exp(-dense[:, :, 64:].cpu().numpy().astype(np.float64)))).max(axis=2)


def _forward_tiles(det, mos, xy, size):
    """(network input, dense rows) of the tiles at xy, four at a time"""
    nets, rows = [], []
    for i in range(0, len(xy), 4):
        netin, status, lb = det.preproc(mos, xy[i:i + 4], size, size, size, _cfg())
        rows.append(det.forward(netin).clone())
        nets.append(netin)
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == 0).all() and (lb.H, lb.W) == (size, size)
    return torch.cat(nets), torch.cat(rows)


def _busy_tiles(det):
    """origins of the full 512-px tiles of the sky's grid (step 0.8), those with the most anchors whose best score clearly passes
    0.7 first: most tiles of this sky have a few dozen such anchors, some hundreds, some none"""
    key = (id(det), "busy")
    if key not in _CACHE:
        mos = det.mosaic_to_device(_sky())
        xy = [(x, y) for y in (0, 410, 820, 1230) for x in (0, 410, 820, 1230)]
        _, dense = _forward_tiles(det, mos, xy, 512)
        n = (_best(dense) > 0.7 + 1e-6).sum(axis=1)
        print("anchors above 0.7 on the 16 full tiles:", n.tolist())
        _CACHE[key] = [xy[k] for k in np.argsort(-n, kind="stable")]
    return _CACHE[key]


def _case(det, size, scale):
    """network input + dense rows of (1 x 512 x 512: the benchmark's geometry, maps 64 / 32 / 16) or (3 x 256 x 256: maps 32 / 16 / 8,
    lists that span images); computed once per context and left unchanged.  Scale l: the 512-px tile is the one with the most anchors
    above 0.7, the 256-px tiles are the three with the most such anchors among the 256-px windows (step 128) of the three busiest."""
    key = (id(det), size)
    if key not in _CACHE:
        mos = det.mosaic_to_device(_sky())
        busy = _busy_tiles(det)[:3] if scale == "l" else [(410, 410)]
        if size == 512:
            netin, dense = _forward_tiles(det, mos, busy[:1], 512)
        else:
            xy = [(x0 + dx, y0 + dy) for (x0, y0) in busy for dy in (0, 128, 256) for dx in (0, 128, 256)]
            netin, dense = _forward_tiles(det, mos, xy, 256)
            n = (_best(dense) > 0.7 + 1e-6).sum(axis=1)
            print("anchors above 0.7 on the 256-px windows:", n.tolist())
            pick = sorted(np.argsort(-n, kind="stable")[:3].tolist())
            netin, dense = netin[pick].contiguous(), dense[pick].contiguous()
            # the same three tiles as ONE batch give the same rows (batch-invariant kernel selection), and these are the rows compared
            dense = det.forward(netin).clone()
            torch.cuda.synchronize()
        _CACHE[key] = (netin, dense)
    return _CACHE[key]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("scale,size", [("l", 512), ("l", 256), ("n", 256)])
def test_candidate_rows_are_the_dense_bits(scale, size):
    """Per stride level, conf = 0.0 (every anchor a candidate: corners, borders, the full lists), 0.7 (the benchmark's threshold)
    and 2.0 (no candidate, empty lists): the class columns are bit-equal to cy_forward's at every anchor; the box columns are
    bit-equal at the candidates and still NaN elsewhere.  Which anchors the device took is read from the rows it wrote and must
    lie between the anchors whose best score (float64 sigmoid of the dense class logits) exceeds conf + 1e-6 and conf - 1e-6:
    the device compares a float32 sigmoid (a few 6e-8 at 0.7) and the two may disagree on an anchor only inside that band.
    A level whose dense kernels the sparse ones do not reproduce (the 8 x 8 map of 256-px inputs: strip kernel) is reported as
    dense and must then hold the dense rows everywhere.  The benchmark's geometry must be sparse on all three levels."""
    det = detector("fp16", scale=scale)
    netin, dense = _case(det, size, scale)
    B, A, R = dense.shape
    d = dense.cpu()
    assert torch.isfinite(d).all()
    best = _best(dense)
    hw = [(size >> (3 + l)) ** 2 for l in range(3)]
    lo = [0, hw[0], hw[0] + hw[1]]
    for conf in (0.0, 0.7, 2.0):
        out = torch.full_like(dense, float("nan"))
        out, sparse = det.forward_sparse_box(netin, conf, out)
        torch.cuda.synchronize()
        o = out.cpu()
        if size == 512:
            assert sparse == [1, 1, 1], "the benchmark's geometry keeps a dense level: %s" % sparse
        assert sparse[0] == 1 and sparse[1] == 1, sparse
        assert torch.equal(_bits(o[:, :, 64:]), _bits(d[:, :, 64:])), "class columns differ (conf %.2f)" % conf
        ncand = 0
        for l in range(3):
            ol, dl = o[:, lo[l]:lo[l] + hw[l], :64], d[:, lo[l]:lo[l] + hw[l], :64]
            if not sparse[l]:
                assert torch.equal(_bits(ol), _bits(dl)), "dense level %d differs" % l
                continue
            nan = torch.isnan(ol)
            written = ~nan.any(dim=2)
            assert bool((nan.all(dim=2) | written).all()), "level %d: a row is written in part" % l
            bl = best[:, lo[l]:lo[l] + hw[l]]
            must, may = torch.from_numpy(bl > conf + 1e-6), torch.from_numpy(bl > conf - 1e-6)
            assert bool((written | ~must).all()), "level %d conf %.2f: %d candidates without box logits" % (l, conf, int((must & ~written).sum()))
            assert bool((may | ~written).all()), "level %d conf %.2f: %d rows written that are no candidates" % (l, conf, int((written & ~may).sum()))
            assert torch.equal(_bits(ol[written]), _bits(dl[written])), "level %d conf %.2f: %d of %d candidate rows differ from the dense kernels' bits" % (
                l, conf, int((_bits(ol[written]) != _bits(dl[written])).any(dim=1).sum()), int(written.sum()))
            ncand += int(written.sum())
            if conf == 0.0:
                assert bool(written.all())
        print("%s %d px conf %.2f: sparse levels %s, %d candidate rows" % (scale, size, conf, sparse, ncand))
        if conf == 0.7 and scale == "l":               # (the second scale is an extra: its seeded scores need not reach 0.7)
            assert ncand >= 1, "no candidate at conf 0.7: the case checks nothing"
        if conf == 2.0:
            assert ncand == 0


def test_detect_path_is_byte_equal_with_and_without(monkeypatch):
    """cy_detect_tiles over the nine 512-px tiles (step 0.8) of an 1100 x 1100 px window of the sky (full, ragged and corner
    tiles: main lane and small-batch lane, the ragged maps on the ping-pong kernel's walk) with CY_SPARSE_BOX=0 and =2 (0.05 lies
    below the default's conf floor, so 2 it is) at conf 0.7 and 0.05: detections, counts, status and
    the context counters are byte-equal; the sparse pass run twice in a row in one context gives the same again (no slot map,
    list or count of the batch before is read)."""
    from caesar_yolo_amd import utils
    det = detector("fp16")
    x0, y0 = _busy_tiles(det)[0]                     # a window of the sky whose grid holds the busiest tile
    x0, y0 = (x0 if x0 <= 948 else x0 - 410), (y0 if y0 <= 948 else y0 - 410)
    mos = det.mosaic_to_device(np.ascontiguousarray(_sky()[y0:y0 + 1100, x0:x0 + 1100]))
    cfg = _cfg()
    tiles = utils.generate_tiles(0, 1099, 0, 1099, 512, 512, 0.8, 0.8)
    shapes = sorted({(t[3] - t[2], t[1] - t[0]) for t in tiles})
    assert len(tiles) == 9 and len(shapes) == 4

    def run(mode, conf):
        monkeypatch.setenv("CY_SPARSE_BOX", mode)
        det.counters(reset=True)
        res = []
        for th, tw in shapes:
            xy = [(t[0], t[2]) for t in tiles if (t[3] - t[2], t[1] - t[0]) == (th, tw)]
            out = (torch.zeros((len(xy), 300, 6), device="cuda"), torch.full((len(xy),), -1, dtype=torch.int32, device="cuda"),
                   torch.full((len(xy),), -1, dtype=torch.int32, device="cuda"))
            d, c, s = det.detect_tiles(mos, xy, th, tw, 512, cfg, conf, 0.5, 0.3, 0.8, out=out)
            torch.cuda.synchronize()
            res.append((d.cpu().numpy(), c.cpu().numpy(), s.cpu().numpy()))
        return res, det.counters()
    for conf in (0.7, 0.05):
        ref, cref = run("0", conf)
        ndet = sum(int(c[s == 0].sum()) for _, c, s in ref)
        assert ndet >= 1, "no detection at conf %.2f: the comparison checks nothing" % conf
        for k in range(2):
            got, cgot = run("2", conf)
            assert cgot == cref
            for (d0, c0, s0), (d1, c1, s1) in zip(ref, got):
                assert c0.tobytes() == c1.tobytes() and s0.tobytes() == s1.tobytes()
                assert d0.tobytes() == d1.tobytes(), "conf %.2f, sparse run %d: detections differ" % (conf, k)
        print("conf %.2f: %d detections on 9 tiles, byte-equal" % (conf, ndet))
