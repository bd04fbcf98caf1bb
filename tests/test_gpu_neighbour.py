"""The forward kernels beside a busy neighbour stream and behind a chosen LDS history.

The rest of the suite runs every kernel alone on an idle GPU, behind the same predecessor every time.  A wait that covers one
LDS-DMA too few, or a read of LDS that the workgroup did not write, passes all of it: the late bytes arrive in time, the stale
bytes are the same ones every time.  Two probes vary what those tests hold fixed:

  * LDS history (`HipDetector.lds_fill`, cy_debug_lds_fill): a kernel that writes one 32-bit pattern over all LDS of every CU runs
    before the kernel under test.  A result that depends on inherited LDS differs between patterns, and is NaN behind 0x7e7e7e7e.
  * Busy neighbour: a second context runs forwards of nine 256-px tiles on another stream while the victim's forward runs, so that
    memory takes longer and arrives in another order.  Overlap is measured with events, not assumed.

(a) every conv shape that only the augmentation views bring (tests/view_shapes.py, derived from the dispatch on the CPU by
    tests/test_view_shapes_cpu.py) through cy_conv_slices behind three LDS patterns: byte-equal, within layer_ref.conv_bound;
(b) the B = 1 forward at 256, 224 and 192 px beside the neighbour: prediction rows and every materialised conv output byte-equal to
    the solo run, 8 repeats per size;
(c) the same at 224 and 192 px with the neighbour's queue alternating forwards and NaN fills of LDS.
The pipeline scenario of DESIGN.md's open defect (an augmented one-tile call on the small lane beside a nine-tile call of the same
context) is not here: it reproduces the defect when other contexts are alive in the process, and its cause is open.

What the probes cannot show: which CU a workgroup lands on and when memory arrives are not under the test's control, so a pass
bounds the rate of a fault, it does not exclude one; LDS surviving a kernel boundary is observed behaviour of this GPU, no contract."""
import math
import time
import numpy as np
import pytest
import torch
import conv_slices_ref as R
import view_shapes as V
from gpu_common import detector, seeded_weights, netin_from_chw

pytestmark = pytest.mark.gpu

NAN16, ZERO, ONE16 = 0x7e7e7e7e, 0, 0x3c003c00               # two fp16 NaN, zeros, two fp16 1.0
CONTEXTS = ("fp16x3", "fp16")
REPEATS = 8
WORST = {}                                                    # (precision, kernel) -> worst |got - ref| / bound over the cases run


# ------------------------------------------------------------------------------------------------ (a) LDS history, kernel level
CASES = [(prec, n) + c for prec in CONTEXTS for n, c in enumerate(V.gpu_cases(prec))]


def _run(det, t, pattern):
    dev = {k: getattr(t, k).cuda() for k in ("in0", "res", "out") if getattr(t, k) is not None}
    torch.cuda.synchronize()
    filled = det.lds_fill(pattern)
    name, passes = det.conv_slices(t.w.numpy(), t.b.numpy(), t.geom[5], t.geom[6], t.act, dev["in0"], t.c0, dev["out"], in0_coff=t.in0_coff, res=dev.get("res"),
                                   res_coff=t.res_coff, out_coff=t.out_coff, rows=t.rows["out_ro"] if t.layout == "rows" else None)
    torch.cuda.synchronize()
    return dev["out"].cpu(), name, passes, filled


@pytest.mark.parametrize("i", range(len(CASES)), ids=["%s-%s" % (c[0], c[2]) for c in CASES])
def test_conv_behind_three_lds_histories(i, monkeypatch):
    prec, n, what, row, inv = CASES[i]
    monkeypatch.setenv("CY_BATCH_INVARIANT", inv)
    rows = V.rows_layout(row)
    # fp16x3: odd cases with an fp16-exact filter (the two-pass form, which the seeded images run), even ones the three-pass form
    t = R.build(prec, (1,) + row[1:7], True, "rows" if rows else "dense", 7000 + n, rows=rows, w16=prec == "fp16x3" and n % 2 == 1)
    if not row[7]:
        t.res = t.r = None
    det = detector(prec)
    outs = []
    for pattern in (NAN16, ZERO, ONE16):
        got, name, passes, filled = _run(det, t, pattern)
        assert name.split(" ")[0] == V.KERNEL_VARIANT[row[0]], "%s ran %r, the table says %s" % (what, name, V.KERNEL_VARIANT[row[0]])
        assert filled >= 64 * 1024 and passes == ((2 if n % 2 == 1 else 3) if prec == "fp16x3" else 0)
        outs.append(got)
    ratio = R.check(t, outs[0], name, passes)
    WORST[(prec, row[0])] = max(WORST.get((prec, row[0]), 0.0), ratio)
    print("LDS_HISTORY %s %s [%s] passes %d, %d B of LDS filled per CU: worst ratio %.3f" % (prec, what, name.split(" ")[0], passes, filled, ratio))
    for pattern, o in zip(("zeros", "fp16 ones"), outs[1:]):
        same = o.numpy().tobytes() == outs[0].numpy().tobytes()
        if not same:
            d = (o.double() - outs[0].double())
            nd = int((o.contiguous().view(torch.int16 if o.dtype == torch.float16 else torch.int32)
                      != outs[0].contiguous().view(torch.int16 if o.dtype == torch.float16 else torch.int32)).sum())
            raise AssertionError("%s %s [%s]: the output behind an LDS of %s differs from the one behind NaN in %d elements, by up to %.3g"
                                 % (prec, what, name, pattern, nd, float(torch.nan_to_num(d.abs(), nan=float("inf")).max())))


def test_report_worst_ratio_per_kernel():
    """Printed, not asserted (every case asserted its own): the worst ratio to the float64 bound per kernel over the cases above."""
    for (prec, kernel), r in sorted(WORST.items()):
        print("LDS_HISTORY worst ratio %s %s: %.3f" % (prec, kernel, r))
    assert all(r <= 1.0 for r in WORST.values())


# ------------------------------------------------------------------------------------------------ (b), (c) busy neighbour, forward level
_POOL = []


def _pairs():
    """Pairs of a pool of four streams.  The runtime maps streams onto four hardware queues; two streams on one queue serialise."""
    if not _POOL:
        _POOL.extend(torch.cuda.Stream() for _ in range(4))
    return [(_POOL[a], _POOL[b]) for a in range(4) for b in range(a + 1, 4)]


def _input(B, size, dtype, seed):
    x = torch.rand((B, 3, size, size), generator=torch.Generator().manual_seed(seed))
    return netin_from_chw(x, dtype)


def _read_all(det, names):
    """{conv name: bytes} of every conv output the last forward materialised (the rest ran inside a neighbour's kernel, or a later
    layer reuses their buffer; the head's outputs are the prediction rows)."""
    from caesar_yolo_amd.lib import CyError
    out, shape = {}, {}
    for name in names:
        try:
            a = det.read_conv(name, 1 << 21)
        except CyError as e:
            if any(s in str(e) for s in ("not materialised", "ran fused", "read from d_pred")):
                continue
            raise
        out[name], shape[name] = a.tobytes(), a.shape
    return out, shape


def _ms(fn, reps=3):
    """GPU milliseconds of fn() on the current stream (mean of reps, after one warm-up), and host seconds to queue it."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    host = (time.perf_counter() - t0) / reps
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, host


def _gate_cycles(ms):
    """Cycles of torch's spin kernel that last about `ms` (calibrated once)."""
    if "per_ms" not in _GATE:
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(2000000)
        e1.record()
        torch.cuda.synchronize()
        _GATE["per_ms"] = 2000000 / max(e0.elapsed_time(e1), 1e-3)
    return int(ms * _GATE["per_ms"])


_GATE = {}


def _beside(victim, vin, vpred, neigh, nin, npred, K, s_n, s_v, gate_ms, fill):
    """K neighbour forwards on s_n and the victim's forward on s_v, both queued whole behind a gate (a spin kernel on the current
    stream) so that queueing takes no part in the timing; the victim starts behind the neighbour's first event.
    -> (ms from the neighbour's start to the victim's, victim's ms, ms from the victim's end to the neighbour's, neighbour's ms)"""
    ev = {k: torch.cuda.Event(enable_timing=True) for k in ("n0", "n1", "v0", "v1")}
    gate = torch.cuda.Event()
    torch.cuda._sleep(_gate_cycles(gate_ms))
    gate.record()
    with torch.cuda.stream(s_n):
        s_n.wait_event(gate)
        ev["n0"].record()
        for _ in range(K):
            if fill:
                neigh.lds_fill(NAN16)
            neigh.forward(nin, out=npred)
        ev["n1"].record()
    with torch.cuda.stream(s_v):
        s_v.wait_event(ev["n0"])
        ev["v0"].record()
        victim.forward(vin, out=vpred)
        ev["v1"].record()
    torch.cuda.synchronize()
    return ev["n0"].elapsed_time(ev["v0"]), ev["v0"].elapsed_time(ev["v1"]), ev["v1"].elapsed_time(ev["n1"]), ev["n0"].elapsed_time(ev["n1"])


def _explain(det, vin, order, solo, got, shape, what):
    """The first differing layer of a compared pass -> AssertionError naming it, its variant (from a separate profiled pass), its
    map and how far the values differ."""
    name = next(n for n in order if n in solo and got[n] != solo[n])
    det.profile(1)
    det.forward(vin)
    torch.cuda.synchronize()
    variant = det.layer_variant(name)
    det.profile(0)
    a, b = np.frombuffer(solo[name], np.float32), np.frombuffer(got[name], np.float32)
    diff = a.view(np.int32) != b.view(np.int32)
    with np.errstate(invalid="ignore"):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))[diff]
    raise AssertionError("%s: first differing layer %s [%s], output %s: %d of %d elements differ, by up to %.3g (%d NaN); %d layers differ in all"
                         % (what, name, variant or "in its neighbour's launch", "x".join(map(str, shape[name])), int(diff.sum()), a.size,
                            float(np.nanmax(d)) if np.isfinite(d).any() else float("nan"), int(np.isnan(b).sum()),
                            sum(1 for n in solo if got[n] != solo[n])))


def _neighbour_test(prec, sizes, fill):
    victim = detector(prec, max_batch=1, max_imgsz=256)
    neigh = detector(prec, max_batch=9, max_imgsz=256)
    order = list(seeded_weights()[3])
    nin = _input(9, 256, neigh.dtype, 99)
    npred = neigh.forward(nin)
    t_n, h_n = _ms(lambda: neigh.forward(nin, out=npred))
    pairs, pi = _pairs(), 0
    for size in sizes:
        vin = _input(1, size, victim.dtype, 1000 + size)
        vpred = victim.forward(vin)
        torch.cuda.synchronize()
        solo_pred = vpred.cpu().numpy().tobytes()
        solo, shape = _read_all(victim, order)
        assert len(solo) >= 40 and np.isfinite(np.frombuffer(solo_pred, np.float32)).all()
        t_v, h_v = _ms(lambda: victim.forward(vin, out=vpred))
        # the neighbour runs at least three times as long as the victim does alone; one more forward for the victim's slow-down beside it
        K = max(3, int(math.ceil(3.0 * t_v / t_n)) + 1)
        gate_ms = 2000.0 * (K * h_n + h_v) + 2.0
        print("NEIGHBOUR %s %d px%s: solo victim %.3f ms (queued in %.3f), one neighbour forward %.3f ms (queued in %.3f), K = %d, gate %.1f ms"
              % (prec, size, " + LDS fills" if fill else "", t_v, 1e3 * h_v, t_n, 1e3 * h_n, K, gate_ms))
        done = 0
        while done < REPEATS:
            assert pi < len(pairs), "%s %d px: no pair of the four streams overlapped the victim with the neighbour" % (prec, size)
            vpred.fill_(float("nan"))
            lead, t_vb, tail, t_nb = _beside(victim, vin, vpred, neigh, nin, npred, K, pairs[pi][0], pairs[pi][1], gate_ms, fill)
            inside = lead >= 0.0 and tail >= 0.0
            print("NEIGHBOUR %s %d px repeat %d pair %d: victim [%.3f, %.3f] ms inside neighbour [0, %.3f] ms: %s"
                  % (prec, size, done, pi, lead, lead + t_vb, t_nb, inside))
            what = "%s %d px beside %d forwards of 9 x 256 px%s (repeat %d)" % (prec, size, K, " and LDS fills" if fill else "", done)
            got_pred = vpred.cpu().numpy().tobytes()
            got, _ = _read_all(victim, order)
            assert sorted(got) == sorted(solo)
            if any(got[n] != solo[n] for n in solo):
                _explain(victim, vin, order, solo, got, shape, what)
            if got_pred != solo_pred:
                a, b = np.frombuffer(solo_pred, np.float32), np.frombuffer(got_pred, np.float32)
                raise AssertionError("%s: every conv output read equals the solo run's, yet %d prediction values differ (%d NaN): the head's outputs"
                                     % (what, int((a.view(np.int32) != b.view(np.int32)).sum()), int(np.isnan(b).sum())))
            if inside:
                done += 1
            else:
                pi += 1                                   # these two streams share a hardware queue (or the victim outlasted the neighbour)


@pytest.mark.parametrize("prec", CONTEXTS)
def test_forward_beside_a_busy_neighbour(prec):
    _neighbour_test(prec, (256, 224, 192), False)


@pytest.mark.parametrize("prec", CONTEXTS)
def test_forward_beside_a_neighbour_that_fills_lds(prec):
    _neighbour_test(prec, (224, 192), True)
