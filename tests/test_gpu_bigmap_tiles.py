"""Preprocessing and the detect pass on tiles of a 46341 x 46339 mosaic (tests/bigmap_cases.py: MH, MW) whose rows hold pixel 2^29,
2^30 and 3 * 2^29, and on the tile that ends on the mosaic's last pixel; and the 4 GiB tile-span limit of the preprocessing
(fill_pre_args: a tile is addressed with 32-bit byte offsets from its own first pixel).

The statement is translation: cy_preproc_planes + cy_preproc_params give, byte for byte, what the same call gives on a small
mosaic that holds the same pixels at small origins, and cy_detect_tiles gives the same detections.  The small case is tied to
float64 by tests/test_gpu_preproc*.py.  No skip path: when the mosaics cannot be allocated the tests error."""
import os

import numpy as np
import pytest
import torch

import bigmap_cases as B
from caesar_yolo_amd import lib as L
from caesar_yolo_amd import preprocessing as PP
from gpu_common import ROOT, assert_same_detections, detector

pytestmark = pytest.mark.gpu

T = 160
CHAN3 = dict(sigma_clip_baseline=0, sigma_clip_low=10, sigma_clip_up=10, zscale_contrast=0.25)
PROGRAMS = {
    "1 channel": lambda: [PP.SigmaClipper(sigma_low=1, sigma_up=1), PP.ZScaleTransformer(contrasts=[0.25] * 3), PP.MinMaxNormalizer(norm_min=0, norm_max=255)],
    "3 channels": lambda: [PP.ChanResizer(nchans=3), PP.Chan3Trasformer(**CHAN3), PP.MinMaxNormalizer(norm_min=0, norm_max=255)],
}
NTILES = 4


def textures():
    """Four 160 x 160 tiles of texture: windows of the synthetic field of tests/golden/preproc.npz, each its own."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "preproc.npz"))["in/syn192"].astype(np.float32)
    t = [g[:T, :T], g[32:, 32:], g[:T, 32:][:, ::-1], g[32:, :T][::-1]]
    assert all(a.shape == (T, T) and np.isfinite(a).all() for a in t)
    return [np.ascontiguousarray(a) for a in t]


def big_tiles():
    """[(x, y)] of the tiles on the big mosaic: pixel 2^29, 2^30 and 3 * 2^29 at (80, 80) of a tile, and the last tile of the mosaic."""
    xy = []
    for index in (1 << 29, 1 << 30, 3 << 29):
        y, x = B.rc(index)
        assert T // 2 <= x <= B.MW - T and T // 2 <= y <= B.MH - T
        xy.append((x - T // 2, y - T // 2))
    return xy + [(B.MW - T, B.MH - T)]


def place(det, shape, xy, tiles):
    m = torch.zeros(shape, dtype=torch.float32, device=det.tdev)
    for (x, y), t in zip(xy, tiles):
        m[y:y + T, x:x + T] = torch.from_numpy(t).to(det.tdev)
    torch.cuda.synchronize()
    return m


SMALL_XY = [(1, 0), (T + 3, 1), (2 * T + 6, 2), (3 * T + 9 - 2, 3)]      # origins that are not 4-aligned, the last tile flush in the corner
SMALL_SHAPE = (T + 3, 4 * T + 7)


@pytest.fixture(scope="module")
def det():
    return detector("fp32", max_batch=NTILES, max_imgsz=160)


@pytest.fixture(scope="module")
def small(det):
    """The small mosaic and what every program gives on it: {program: (planes bytes, status, params bytes)}."""
    assert SMALL_XY[-1] == (SMALL_SHAPE[1] - T, SMALL_SHAPE[0] - T)
    m = place(det, SMALL_SHAPE, SMALL_XY, textures())
    out = {}
    for name, stages in PROGRAMS.items():
        cfg = PP.DataPreprocessor(stages()).program()
        planes, status = det.preproc_planes(m, SMALL_XY, T, T, cfg)
        torch.cuda.synchronize()
        out[name] = (planes.cpu().numpy(), status.cpu().numpy(), det.preproc_params(NTILES).copy())
        assert (out[name][1] == 0).all() and np.isfinite(out[name][0]).all() and len(np.unique(out[name][0])) > 1000, name
    return m, out


@pytest.fixture(scope="module")
def big(det):
    m = place(det, (B.MH, B.MW), big_tiles(), textures())
    yield m
    del m
    torch.cuda.empty_cache()


def same_bytes(det, mosaic, xy, small_out, what):
    for name, stages in PROGRAMS.items():
        cfg = PP.DataPreprocessor(stages()).program()
        planes, status = det.preproc_planes(mosaic, xy, T, T, cfg)
        torch.cuda.synchronize()
        params = det.preproc_params(len(xy))
        want = small_out[name]
        sel = slice(NTILES - len(xy), NTILES)                        # a single tile stands for the last one
        assert np.array_equal(status.cpu().numpy(), want[1][sel]), (what, name)
        for c in range(max(int(cfg.nprog), 1)):                        # the stages the program has: the other rows are not written by the call
            n = int(cfg.prog[c].n)
            assert params[:, c, :n].tobytes() == np.ascontiguousarray(want[2][sel][:, c, :n]).tobytes(), \
                "%s, %s: the stage parameters of channel %d differ" % (what, name, c)
        g, w = planes.cpu().numpy(), np.ascontiguousarray(want[0][sel])
        assert g.tobytes() == w.tobytes(), "%s, %s: %d plane values differ" % (what, name, int((g.view(np.uint64) != w.view(np.uint64)).sum()))


def test_preprocessing_is_the_same_at_large_offsets(det, small, big):
    same_bytes(det, big, big_tiles(), small[1], "big mosaic")


def test_detections_are_the_same_at_large_offsets(det, small, big):
    cfg = PP.DataPreprocessor(PROGRAMS["1 channel"]()).program()
    args = (T, T, 160, cfg, 0.25, 0.5, 0.3, 0.8)
    d0, c0, s0 = (t.cpu().numpy() for t in det.detect_tiles(small[0], SMALL_XY, *args))
    d1, c1, s1 = (t.cpu().numpy() for t in det.detect_tiles(big, big_tiles(), *args))
    assert (s0 == 0).all() and np.array_equal(s1, s0) and np.array_equal(c1, c0) and c0.sum() > 0, (c0, c1, s0, s1)
    for b in range(NTILES):
        n = int(c0[b])
        assert_same_detections(d1[b, :n, :4], d1[b, :n, 4], d1[b, :n, 5], d0[b, :n, :4], d0[b, :n, 4], d0[b, :n, 5], what="tile %d" % b)
    print("detect_tiles: %s detections per tile, the same on both mosaics" % c0.tolist())


def test_the_tile_span_limit(det, small):
    """A mosaic of 160 rows at the largest width fill_pre_args accepts: the tile against its right edge (the last pixel of the
    mosaic, its rows 4 GiB - 256 bytes apart from first to last) gives the bytes of the small mosaic; one column more is refused."""
    limit = 0xFFFFFF00
    MW = (limit // 4 - T) // (T - 1)                                 # the largest MW with ((th - 1) MW + tw) 4 <= limit
    assert ((T - 1) * MW + T) * 4 <= limit < ((T - 1) * (MW + 1) + T) * 4 and T * (MW + 1) < 1 << 31
    buf = torch.zeros(T * (MW + 1), dtype=torch.float32, device=det.tdev)
    m = buf[:T * MW].view(T, MW)
    m[:, MW - T:] = torch.from_numpy(textures()[-1]).to(det.tdev)
    torch.cuda.synchronize()
    same_bytes(det, m, [(MW - T, 0)], small[1], "160 x %d" % MW)
    wide = buf.view(T, MW + 1)
    cfg = PP.DataPreprocessor(PROGRAMS["1 channel"]()).program()
    with pytest.raises(L.CyError, match=r"tile rows span more than 4 GiB of the mosaic.*\(status -5\)"):      # CY_ERR_UNSUPPORTED
        det.preproc_planes(wide, [(MW + 1 - T, 0)], T, T, cfg)
    with pytest.raises(L.CyError, match=r"tile rows span more than 4 GiB of the mosaic.*\(status -5\)"):
        det.detect_tiles(wide, [(0, 0)], T, T, 160, cfg, 0.25, 0.5, 0.3, 0.8)
    del m, wide, buf
    torch.cuda.empty_cache()
