"""cy_find_peaks on the GPU against its numpy float64 restatement (tests/peaks_ref.py) on the inputs of tests/peaks_cases.py.

total, the number and the order of the rows, and x, y, v, rms, snr, npix, nabove are exact integer or single IEEE operations on both
sides: equal.  sum, sw, swx, swy add the same float64 terms in another order, so |gpu - ref| <= 2 m 2^-53 sum|t_i| with m = npix terms
and sum|t_i| from the reference (peaks_ref.sum_bound, the bound tests/test_gpu_islands.py derives).  Nothing here was tuned on the
GPU.

The chain-level test runs measure.Chain on the real detector over the scene of tests/peaks_chain_ref.py: 160 x 160, unit Gaussian
noise (seed 11) and two circular Gaussians of amplitude 50, sigma 2 at (40, 40) and (115, 110); the hand-made source list boxes only
the first.  The same chain runs on the CPU with the numpy references of tests/ standing in for the detector (measure_ref, bkg_ref,
island_ref, deblend_ref, fit_ref, residual_ref, peaks_ref; tests/test_peaks_cpu.py::test_chain_scene_on_the_references): at this seed
the references alone find exactly one peak, the unboxed Gaussian at (115, 110) with snr 50.9, nabove 25 and in_source None, and leave
none within 6 px of the boxed one (its fit: peak 50.17 at (40.02, 39.99), res_rms 0.92, largest |residual| 2.05), so both statements
hold before the GPU is asked."""
import ctypes as C

import numpy as np
import pytest
import torch

import peaks_cases as PC
import peaks_chain_ref as CR
import peaks_ref as PR
from caesar_yolo_amd import lib as L
from caesar_yolo_amd import measure
from gpu_common import detector

pytestmark = pytest.mark.gpu
EXACT = [0, 1, 2, 3, 4, 5, 6, 11]


@pytest.fixture(scope="module")
def det():
    return detector("fp32", max_batch=1, max_imgsz=160)


def upload(det, a, offset=False):
    """The array as it is, NaN included; offset: in a buffer that starts one float behind a 16-byte boundary."""
    a = np.ascontiguousarray(a, np.float32)
    if not offset:
        dev = torch.from_numpy(a.copy()).to(det.tdev)
    else:
        buf = torch.zeros(a.size + 8, dtype=torch.float32, device=det.tdev)
        assert buf.data_ptr() % 16 == 0
        dev = buf[1:1 + a.size].view(a.shape)
        dev.copy_(torch.from_numpy(a.copy()))
        assert dev.data_ptr() % 16 == 4 and dev.is_contiguous()
    torch.cuda.synchronize()
    return dev


@pytest.fixture(scope="module")
def resident(det):
    return {c.name: (upload(det, c.map, c.offset), upload(det, c.rms, c.offset)) for c in PC.cases()}


def check_rows(name, rows, total, want, absum, cap=None):
    n = len(want) if cap is None else min(len(want), cap)
    assert total == len(want), "%s: %d peaks, the reference has %d" % (name, total, len(want))
    assert rows.shape == (n, L.CY_PEAK_FIELDS), name
    want, absum = want[:n], absum[:n]
    assert np.array_equal(rows[:, EXACT], want[:, EXACT]), "%s: first differing row %s" % (
        name, np.nonzero((rows[:, EXACT] != want[:, EXACT]).any(1))[0][:1])
    d, bound = np.abs(rows[:, PR.SUMS] - want[:, PR.SUMS]), PR.sum_bound(want, absum)
    assert (d <= bound).all(), "%s: a sum off by %g, bound %g" % (name, d.max(), bound[np.unravel_index(np.argmax(d - bound), d.shape)])
    return float((d / np.maximum(bound, 1e-300)).max()) if n else 0.0


@pytest.mark.parametrize("case", PC.cases(), ids=lambda c: c.name)
def test_case(det, resident, case):
    m, r = resident[case.name]
    want, absum = PC.reference()[case.name]
    rows, total = det.find_peaks(m, r, case.k_sigma, case.radius, case.sign)
    worst = check_rows(case.name, rows, total, want, absum)
    print("%s: %d peaks, largest difference of a sum %.3f of its bound" % (case.name, total, worst))
    rows2, total2 = det.find_peaks(m, r, case.k_sigma, case.radius, case.sign)
    assert total2 == total and rows2.tobytes() == rows.tobytes(), "%s: a second call gave other bytes" % case.name


def test_the_cases_hold_what_they_are_for():
    ref = {k: v[0] for k, v in PC.reference().items()}
    assert len(ref["lattice"]) == 2304 and len(ref["none"]) == 0 and len(ref["1x1"]) == 1 and len(ref["1x1_below"]) == 0
    assert len(ref["scene"]) > 300
    for nseg, name in ((1, "one_segment_and_1"), (2, "two_segments_and_1")):
        xy = {(int(r[0]), int(r[1])) for r in ref[name]}
        for b in range(1, nseg + 1):
            assert {(b * PC.SEG - 1, 0), (b * PC.SEG, 4), (b * PC.SEG - 1, 8)} <= xy and (b * PC.SEG, 8) not in xy


def test_unaligned_pointers_give_the_same_rows(det, resident):
    a, _ = det.find_peaks(*resident["64x96"], 3.0, 2, 1)
    b, _ = det.find_peaks(*resident["64x96_offset"], 3.0, 2, 1)
    assert len(a) > 0 and a.tobytes() == b.tobytes()


def test_holes_are_the_peaks_of_the_negated_map(det, resident):
    c = PC.case("70x75")
    neg = upload(det, -c.map)
    pos, npos = det.find_peaks(resident["70x75"][0], resident["70x75"][1], c.k_sigma, c.radius, 1)
    got, ngot = det.find_peaks(neg, resident["70x75"][1], c.k_sigma, c.radius, -1)
    want = pos.copy()
    want[:, 2] = -want[:, 2]
    assert ngot == npos > 0 and got.tobytes() == want.tobytes()


def test_truncation(det, resident):
    m, r = resident["lattice"]
    want, absum = PC.reference()["lattice"]
    full, total = det.find_peaks(m, r, 5.0, 1, 1)
    for cap in (1, 100, 2303, 2304, 2305):
        rows, t = det.find_peaks(m, r, 5.0, 1, 1, cap=cap)
        assert t == total == 2304 and rows.tobytes() == full[:cap].tobytes(), cap
    rows, t = det.find_peaks(m, r, 5.0, 1, 1, cap=0)
    assert t == 2304 and rows.shape == (0, L.CY_PEAK_FIELDS)
    # the C entry: rows beyond min(total, cap) stay as they were, and cap == 0 takes a null h_rows
    buf = np.full((2400, L.CY_PEAK_FIELDS), -7.0, np.float64)
    tot = C.c_longlong(-1)
    dp = C.POINTER(C.c_double)
    L.check(det.lib.cy_find_peaks(det.ctx, det._p(m), det._p(r), 96, 96, 5.0, 1, 1, 2400, buf.ctypes.data_as(dp), C.byref(tot), det._stream()), det.ctx)
    assert tot.value == 2304 and buf[:2304].tobytes() == full.tobytes() and (buf[2304:] == -7.0).all()
    buf[:] = -7.0
    L.check(det.lib.cy_find_peaks(det.ctx, det._p(m), det._p(r), 96, 96, 5.0, 1, 1, 50, buf.ctypes.data_as(dp), C.byref(tot), det._stream()), det.ctx)
    assert tot.value == 2304 and buf[:50].tobytes() == full[:50].tobytes() and (buf[50:] == -7.0).all()
    L.check(det.lib.cy_find_peaks(det.ctx, det._p(m), det._p(r), 96, 96, 5.0, 1, 1, 0, None, C.byref(tot), det._stream()), det.ctx)
    assert tot.value == 2304


def test_argument_errors(det, resident):
    m, r = resident["64x96"]
    lib, dp = det.lib, C.POINTER(C.c_double)
    buf = np.zeros((4, L.CY_PEAK_FIELDS), np.float64)
    tot = C.c_longlong(0)
    good = dict(ctx=det.ctx, m=det._p(m), r=det._p(r), MH=64, MW=96, k=5.0, radius=2, sign=1, cap=4, rows=buf.ctypes.data_as(dp), tot=C.byref(tot))

    def call(**kw):
        a = dict(good, **kw)
        return lib.cy_find_peaks(a["ctx"], a["m"], a["r"], a["MH"], a["MW"], a["k"], a["radius"], a["sign"], a["cap"], a["rows"], a["tot"], det._stream())
    assert call() == 0
    bad = [dict(ctx=None), dict(m=None), dict(r=None), dict(tot=None), dict(rows=None), dict(MH=0), dict(MW=-1), dict(MH=1 << 16, MW=1 << 15),
           dict(MH=(1 << 24) + 1, MW=1), dict(radius=0), dict(radius=9), dict(sign=0), dict(sign=2), dict(k=0.0), dict(k=-1.0),
           dict(k=float("nan")), dict(k=float("inf")), dict(cap=-1), dict(cap=(1 << 20) + 1)]
    for kw in bad:
        assert call(**kw) == -1, kw                          # CY_ERR_ARG
    call(m=None)
    assert b"null argument" in lib.cy_last_error(det.ctx)
    call(radius=9)
    assert b"radius" in lib.cy_last_error(det.ctx)
    call(MH=1 << 16, MW=1 << 15)
    assert b"2^31" in lib.cy_last_error(det.ctx)
    call(MH=(1 << 24) + 1, MW=1)
    assert b"segment table" in lib.cy_last_error(det.ctx)
    with pytest.raises(L.CyError):
        det.find_peaks(m, resident["70x75"][1])
    with pytest.raises(L.CyError):
        det.find_peaks(m.double(), r)
    with pytest.raises(L.CyError):
        det.find_peaks(m.cpu(), r)


def test_kernel_time_is_kept():
    from caesar_yolo_amd.model import HipDetector
    from gpu_common import seeded_weights
    fresh = HipDetector(seeded_weights("l", 5)[0], device=0, precision="fp32", max_batch=1, max_imgsz=160)      # a context of its own
    assert fresh.peaks_kernel_ms() == -1.0
    c = PC.case("ties")
    fresh.find_peaks(upload(fresh, c.map), upload(fresh, c.rms), c.k_sigma, c.radius, c.sign)
    assert fresh.peaks_kernel_ms() >= 0.0
    fresh.close()


# ---- the chain on the real detector
def test_chain_finds_the_source_that_has_no_box(det):
    img, sources = CR.scene()
    dev = upload(det, img)
    stats = {}
    chain = measure.Chain(det, dev, sources, CR.CONFIG).run(measure.plan(CR.CONFIG), stats)
    print("peaks: found %d kept %d, first %s" % (stats["peaks_found"], stats["peaks_kept"], chain.peak_list[:1]))
    CR.check(chain.peak_list, sources)
    assert chain.hole_list is None and "holes_found" not in stats
    assert stats["peaks_found"] >= stats["peaks_kept"] == len(chain.peak_list) and stats["peaks_truncated"] == 0
    assert stats["peaks_kernel_ms"] >= 0.0 and stats["peaks_ms"] > 0.0
    assert set(chain.peak_list[0]) == set(measure.PEAK_KEYS)
