"""cy_atrous_step on the GPU against its numpy float64 restatement (tests/atrous_ref.py) on the inputs of tests/atrous_cases.py.

Every product and every sum of the definition is one IEEE float64 operation in a fixed order, contraction is off in the kernel, and
the two roundings to fp32 are single operations: smooth and detail equal the reference bit for bit, compared as uint32 (no output
is NaN: a non-finite input counts as 0, and a sum of finite terms of at most 2 FLT_MAX is finite or an infinity).  Nothing here was
tuned on the GPU.

The scale search: measure.Chain.scale_peaks() on the real detector with .resid preset to a fixed fp32 map, against the same chain over
the numpy references (tests/atrous_chain_ref.py).  The planes are bit-equal; the noise meshes are bit-equal (as tests/test_gpu_background.py
holds them), so the peak rows compare as tests/test_gpu_peaks.py compares them: counts, order and the single-operation fields equal,
the four sums within peaks_ref.sum_bound.  The chain-level test runs the whole chain on the scene of tests/atrous_chain_ref.py, whose
two statements the references alone satisfy at the committed seed (tests/test_atrous_cpu.py::test_chain_scene_on_the_references: both
blobs strongest at scale 5 with snr 16.9 and 13.7, at (90, 99) and (181, 170); no pixel peak at 5 sigma anywhere)."""
import ctypes as C

import numpy as np
import pytest
import torch

import atrous_cases as AC
import atrous_chain_ref as ACR
import atrous_ref as AR
import peaks_ref as PR
from caesar_yolo_amd import lib as L
from caesar_yolo_amd import measure
from gpu_common import detector

pytestmark = pytest.mark.gpu
GUARD = 64                                                    # floats before and after every output buffer
SENTINEL = -7.5
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


def guarded(det, shape, offset=False):
    """-> (whole buffer, the output map inside it): GUARD sentinel floats (+ 1 with offset) in front of the map and GUARD behind."""
    n, lead = int(np.prod(shape)), GUARD + (1 if offset else 0)
    buf = torch.full((lead + n + GUARD,), SENTINEL, dtype=torch.float32, device=det.tdev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[lead:lead + n].view(shape)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(name, what, got, want):
    g, w = bits(got), bits(want)
    if not np.array_equal(g, w):
        y, x = (int(v[0]) for v in np.nonzero(g != w))
        raise AssertionError("%s %s: %d of %d pixels differ; first (%d, %d): %r on the GPU, %r in the reference" % (
            name, what, int((g != w).sum()), g.size, y, x, got[y, x], want[y, x]))


def assert_guards(name, buf, view):
    host, n = buf.cpu().numpy(), view.numel()
    lead = host.size - n - GUARD
    assert (host[:lead] == SENTINEL).all() and (host[lead + n:] == SENTINEL).all(), "%s: a guard float was written" % name


@pytest.mark.parametrize("want", [("smooth", "detail"), ("smooth",), ("detail",)], ids=lambda w: "+".join(w))
@pytest.mark.parametrize("case", AC.cases(), ids=lambda c: c.name)
def test_case(det, case, want):
    dev = upload(det, case.map, case.offset)
    ref = dict(zip(("smooth", "detail"), AC.reference()[case.name]))
    assert not np.isnan(ref["smooth"]).any() and not np.isnan(ref["detail"]).any()
    bufs = [guarded(det, case.map.shape, case.offset) for _ in range(2)]
    out = det.atrous_step(dev, case.step, want=want, out=tuple(v for _, v in bufs))
    torch.cuda.synchronize()
    first = []
    for name, o, (buf, view) in zip(("smooth", "detail"), out, bufs):
        if name not in want:
            assert o is None and (buf.cpu().numpy() == SENTINEL).all(), "%s: %s was written although not wanted" % (case.name, name)
            continue
        assert o is view
        got = o.cpu().numpy()
        assert_bits(case.name, name, got, ref[name])
        assert_guards(case.name, buf, view)
        first.append(got.tobytes())
    assert_bits(case.name, "input", dev.cpu().numpy(), case.map)            # the input is read only
    again = det.atrous_step(dev, case.step, want=want)                      # new maps: a second call gives the same bytes
    assert [o.cpu().numpy().tobytes() for o in again if o is not None] == first, "%s: a second call gave other bytes" % case.name


def test_the_cases_hold_what_they_are_for():
    for name in ("tall_s1", "tall_s3"):
        c = AC.case(name)
        assert AC.items(c.map.shape[0], c.map.shape[1], c.step) > AC.GRID_MAX
    for name in ("constant_s1", "constant_s8"):
        smooth, detail = AC.reference()[name]
        assert np.array_equal(bits(smooth), bits(AC.case(name).map)) and not bits(detail).any()
    assert np.isinf(AC.reference()["special_s1"][1]).any() and np.isfinite(AC.reference()["special_s1"][0]).all()


def test_unaligned_pointers_give_the_same_planes(det):
    for s in AC.STEPS:
        a = det.atrous_step(upload(det, AC.case("64x96_s%d" % s).map), s)
        b = det.atrous_step(upload(det, AC.case("64x96_offset_s%d" % s).map, True), s)
        assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))


def test_argument_errors(det):
    c = AC.case("64x96_s1")
    dev = upload(det, c.map)
    (sbuf, sm), (dbuf, dt) = guarded(det, c.map.shape), guarded(det, c.map.shape)
    lib, n = det.lib, c.map.size
    good = dict(ctx=det.ctx, i=det._p(dev), MH=64, MW=96, step=1, s=det._p(sm), d=det._p(dt))
    addr = lambda t, k=0: C.c_void_p(t.data_ptr() + 4 * k)

    def call(**kw):
        a = dict(good, **kw)
        return lib.cy_atrous_step(a["ctx"], a["i"], a["MH"], a["MW"], a["step"], a["s"], a["d"], det._stream())

    def untouched():
        torch.cuda.synchronize()
        return bool((sbuf == SENTINEL).all()) and bool((dbuf == SENTINEL).all())
    bad = [dict(ctx=None), dict(i=None), dict(s=None, d=None), dict(MH=0), dict(MW=0), dict(MH=-3), dict(MW=-1), dict(step=0), dict(step=-1),
           dict(step=65), dict(step=1 << 20), dict(MH=1 << 16, MW=1 << 15), dict(MH=(1 << 31) - 1, MW=(1 << 31) - 1),
           # an output over the input: the same buffer, one float into it from either side; the outputs over each other
           dict(s=addr(dev)), dict(d=addr(dev)), dict(s=addr(dev, n - 1)), dict(d=addr(dev, 1 - n)), dict(i=addr(sm, n - 1)), dict(i=addr(dt, 1 - n)),
           dict(d=addr(sm)), dict(d=addr(sm, n - 1)), dict(s=addr(dt, 1 - n))]
    for kw in bad:
        assert call(**kw) == -1, kw                          # CY_ERR_ARG
        assert untouched(), kw
    for kw, text in ((dict(i=None), b"null argument"), (dict(s=None, d=None), b"both null"), (dict(step=65), b"step outside"),
                     (dict(MH=1 << 16, MW=1 << 15), b"2^31"), (dict(s=addr(dev)), b"overlaps the input"), (dict(d=addr(sm)), b"d_smooth overlaps d_detail")):
        call(**kw)
        assert text in lib.cy_last_error(det.ctx), (kw, lib.cy_last_error(det.ctx))
    # buffers that touch do not overlap: the three maps back to back in one allocation
    trio = torch.full((3 * n,), SENTINEL, dtype=torch.float32, device=det.tdev)
    trio[:n] = dev.reshape(-1)
    assert call(i=addr(trio), s=addr(trio, n), d=addr(trio, 2 * n)) == 0
    torch.cuda.synchronize()
    got = trio.cpu().numpy()
    assert_bits("adjacent", "smooth", got[n:2 * n].reshape(64, 96), AC.reference()[c.name][0])
    assert_bits("adjacent", "detail", got[2 * n:].reshape(64, 96), AC.reference()[c.name][1])
    assert call() == 0
    with pytest.raises(L.CyError):
        det.atrous_step(dev, 1, want=())
    with pytest.raises(L.CyError):
        det.atrous_step(dev, 0)
    with pytest.raises(L.CyError):
        det.atrous_step(dev, 1, out=(dev, None))
    with pytest.raises(L.CyError):
        det.atrous_step(dev, 1, out=(torch.zeros((64, 95), dtype=torch.float32, device=det.tdev), None))
    with pytest.raises(L.CyError):
        det.atrous_step(dev.double(), 1)
    with pytest.raises(L.CyError):
        det.atrous_step(dev.cpu(), 1)


def test_kernel_time_is_kept():
    from caesar_yolo_amd.model import HipDetector
    from gpu_common import seeded_weights
    fresh = HipDetector(seeded_weights("l", 5)[0], device=0, precision="fp32", max_batch=1, max_imgsz=160)      # a context of its own
    assert fresh.atrous_kernel_ms() == -1.0
    fresh.atrous_step(upload(fresh, AC.case("70x75_s2").map), 2)
    assert fresh.atrous_kernel_ms() > 0.0
    fresh.close()


# ---- the scale search
def check_rows(what, rows, want, absum):
    assert rows.shape == want.shape, "%s: %d rows, the reference has %d" % (what, len(rows), len(want))
    assert np.array_equal(rows[:, EXACT], want[:, EXACT]), what
    d, bound = np.abs(rows[:, PR.SUMS] - want[:, PR.SUMS]), PR.sum_bound(want, absum)
    assert (d <= bound).all(), "%s: a sum off by %g" % (what, d.max())


def assert_same_search(got, ref, absums):
    """Two chains after scale_peaks(): planes bit-equal, raw rows as test_gpu_peaks.py holds them, the lists equal up to the sums."""
    assert sorted(got.scale_planes) == sorted(ref.scale_planes) == sorted(got.scale_rows) == sorted(ref.scale_rows)
    for (j, w), absum in zip(sorted(ref.scale_planes.items()), absums):
        assert_bits("scale %d" % j, "plane", got.scale_planes[j].cpu().numpy(), w)
        check_rows("scale %d" % j, got.scale_rows[j], ref.scale_rows[j], absum)
    same = [k for k in measure.SCALE_PEAK_KEYS if k not in ("x", "y", "flux_sum", "flux", "ra", "dec")]
    assert len(got.scale_list) == len(ref.scale_list)
    for a, b in zip(got.scale_list, ref.scale_list):
        assert [a[k] for k in same] == [b[k] for k in same] and tuple(a) == measure.SCALE_PEAK_KEYS
        assert abs(a["x"] - b["x"]) <= 1e-9 and abs(a["y"] - b["y"]) <= 1e-9 and abs(a["flux_sum"] - b["flux_sum"]) <= 1e-9 * (1.0 + abs(b["flux_sum"]))


def test_scale_search_on_a_fixed_map(det):
    img, _ = ACR.scene()                                      # stands for a residual map: nothing is fitted here
    ref_det = ACR.RefDetector()
    chains = []
    for d, m in ((det, upload(det, img)), (ref_det, img)):
        chain = measure.Chain(d, m, [], ACR.CONFIG)
        chain.resid = m
        chain.scale_peaks()
        chains.append(chain)
    got, ref = chains
    assert sorted(ref.scale_planes) == [2, 3, 4, 5] and len(ref.scale_list) >= 4
    assert [(lv["step"], lv.get("cell"), lv.get("radius")) for lv in got.scale_levels] == [(1, None, None), (2, 32, 2), (4, 64, 4), (8, 128, 8), (16, 256, 8)]
    assert_same_search(got, ref, ref_det.absums)
    st = got.scale_stats
    assert st["atrous_kernel_ms"] > 0.0 and st["scales_background_kernel_ms"] > 0.0 and st["scales_peaks_kernel_ms"] > 0.0
    assert st["scales_found"] >= st["scales_kept"] == len(got.scale_list) >= st["scales_strongest"] >= 2 and st["scales_truncated"] == 0


def test_chain_finds_the_blobs_no_pixel_shows(det):
    img, sources = ACR.scene()
    chain, stats = ACR.run(det, upload(det, img), sources)
    print("scales: %s" % [(p["scale"], p["x_peak"], p["y_peak"], round(p["snr"], 2), p["strongest"]) for p in chain.scale_list])
    ACR.check(chain.peak_list, chain.scale_list)
    assert sources[0]["ncomponents"] == 1 and sources[0]["res_nscale_peaks"] == 0 and sources[0]["res_scale_peak_snr"] is None
    assert {"scales_ms", "atrous_kernel_ms", "scales_background_kernel_ms", "scales_peaks_kernel_ms", "scales_found", "scales_kept",
            "scales_strongest", "scales_truncated"} <= set(stats)
    assert measure.peak_lists(chain)["residual_scale_peaks"] is chain.scale_list
