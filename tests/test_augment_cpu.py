"""Test-time augmentation, host side (no GPU): the library's view geometry (cy_augment_geometry) against ultralytics' formulas
worked out in Python float arithmetic, and the torch-CPU restatement (tests/augment_ref.py) reduced to the single plain view
against the oracle's own model call."""
import numpy as np
import pytest
import torch
from caesar_yolo_amd import lib as L
import augment_ref as AR


def _anchors(H, W):
    return sum(((H + s - 1) // s) * ((W + s - 1) // s) for s in (8, 16, 32))


@pytest.mark.parametrize("H,W", [(128, 128), (256, 256), (512, 512), (640, 640), (1024, 1024),
                                 # ragged letterboxed shapes: a 640 x 360 frame at imgsz 640, a 200 x 230 one at 256
                                 (384, 640), (224, 256)])
def test_augment_geometry_matches_python(H, W):
    views, total = L.augment_geometry(H, W)
    anchors = []
    for k, (s, f) in enumerate(zip(AR.SCALES, AR.FLIPS)):
        v = views[k]
        ch, cw, Hp, Wp = AR.view_geometry(H, W, s)
        assert (v["ch"], v["cw"], v["Hp"], v["Wp"]) == (ch, cw, Hp, Wp), (k, v)
        assert Hp % 32 == 0 and Wp % 32 == 0
        assert v["scale"] == float(s) and v["flip"] == int(f == 3)
        assert v["A"] == _anchors(Hp, Wp)
        anchors.append(v["A"])
    off = 0
    for v, (lo, hi) in zip(views, AR.clip_ranges(anchors)):
        assert (v["lo"], v["hi"], v["off"]) == (lo, hi, off)
        off += hi - lo
    assert total == off


def test_augment_geometry_of_the_issue_table():
    """View sizes and concatenated anchor counts at 512, 640 and 1024 px (content -> padded)."""
    want = {512: ((424, 448), (343, 352)), 640: ((531, 544), (428, 448)), 1024: ((849, 864), (686, 704))}
    for n, ((c1, p1), (c2, p2)) in want.items():
        views, total = L.augment_geometry(n, n)
        assert (views[1]["ch"], views[1]["Hp"], views[2]["ch"], views[2]["Hp"]) == (c1, p1, c2, p2)
    assert L.augment_geometry(640, 640)[1] == 8000 + 6069 + 980 == 15049
    assert L.augment_geometry(1024, 1024)[1] == 38209


def test_augment_geometry_rejects_bad_sizes():
    for hw in ((100, 128), (0, 64), (64, 16)):
        with pytest.raises(L.CyError):
            L.augment_geometry(*hw)


def test_restatement_with_the_plain_view_is_the_oracle_call():
    """predict_augment with views [1] (no flip) = OracleYOLO.predict_raw: same detections, same anchor indices, bit for bit."""
    from caesar_yolo_amd import weights as W
    from oracle import yolov8_ref as Y
    import os
    import tempfile
    path = os.path.join(tempfile.gettempdir(), "cy_test_seeded_n_3_aug.cyw")
    if not os.path.exists(path):
        W.make_seeded_file(path, "n", 3)
    scale, names, wd, _ = W.read_cyw(path)
    om = Y.OracleYOLO(wd, names, scale)
    img = np.random.default_rng(5).uniform(0, 255, (96, 120, 3))
    d_ref, a_ref, raw, pred = om.predict_raw(img, 128, 0.01, 0.6)
    d, a, raws, p = AR.predict_augment(om.net, img, 128, 0.01, 0.6, scales=(1,), flips=(None,))
    assert d_ref.shape[0] > 0
    assert torch.equal(p, pred) and torch.equal(raws[0], raw)
    assert torch.equal(d, d_ref) and torch.equal(a, a_ref)
    # the three standard views on the same input: a different prediction (more anchors) and the clip of _clip_augmented
    _, _, raws3, p3 = AR.predict_augment(om.net, img, 128, 0.01, 0.6)
    views, total = L.augment_geometry(128, 128)
    assert p3.shape[-1] == total and [r.shape[-1] for r in raws3] == [v["A"] for v in views]
    assert torch.equal(p3[..., :views[0]["hi"]], pred[..., :views[0]["hi"]])
