"""Every conv kernel of csrc/conv_igemm.hip on channel slices with guard channels, through cy_conv_slices: the layouts the
forward pass uses (tests/conv_slices_ref.py: dense, slices, shared, concat, upcat, rows), each held to layer_ref.conv_bound's
per-element bound, with every guard element of the output buffer compared bit for bit and NaN in every input and residual
channel outside the slices.

One table (SHAPES, X3, F32, ROW_CASES of tests/conv_slices_ref.py, which tests/test_conv_plan_cpu.py reads too).  Every case names
the variant its shape and switches must select (the first word of conv_variant_name's label) and the
test asserts the name the entry reports; test_table_covers_every_variant compares the names asserted with the names the library
lists.  Shapes: the smallest that select each kernel (tests/test_gpu_conv_tail.py: Cout 200 / 72 / 40 leave one lane group full,
one ragged and one empty), at B >= 2 and on maps that are no multiples of the kernel's patch, so that pixel index x ct runs across
images and ragged rows.  Half of the cases run without activation; every case but the rows has a residual.
Each case prints its worst |got - ref| / bound."""
import pytest
import torch
import conv_slices_ref as R
from gpu_common import detector

pytestmark = pytest.mark.gpu

from conv_slices_ref import SHAPES, X3, F32, ROW_CASES, TWO, G128, G64, WIDE, DUAL, WIDE64, STRIP, D256, D128, HEAD      # the tables: shared with test_conv_plan_cpu.py


def _even(g):
    return (g[0], g[1] + g[1] % 2, g[2] + g[2] % 2) + g[3:]


CASES = []          # (id, prec, geom, inv, env, variant, layout, act, seed)
for prec, table in (("fp16", SHAPES), ("fp16x3", X3), ("fp32", F32)):
    for i, (name, (geom, inv, env, variant, two)) in enumerate(table.items()):
        for j, layout in enumerate(("dense", "slices", "shared") + (TWO if two else ())):
            CASES.append(("%s-%s-%s" % (prec, name, layout), prec, _even(geom) if layout == "upcat" else geom, inv if prec == "fp16" else "1",
                          env, variant, layout, (i + j) % 2 == 0, 100 * i + j))

def _run(t, det):
    """One call of the entry on device copies of the case's buffers -> (output buffer on the host, variant, passes)."""
    dev = {k: getattr(t, k).cuda() for k in ("in0", "in1", "res", "out") if getattr(t, k) is not None}
    out = dev["out"]
    rows = t.rows["out_ro"] if t.layout == "rows" else None
    name, passes = det.conv_slices(t.w.numpy(), t.b.numpy(), t.geom[5], t.geom[6], t.act, dev["in0"], t.c0, out, in0_coff=t.in0_coff,
                                   up0=t.up0, in1=dev.get("in1"), in1_coff=t.in1_coff, c1=t.c1, res=out if t.shared else dev.get("res"),
                                   res_coff=t.res_coff, out_coff=t.out_coff, rows=rows)
    torch.cuda.synchronize()
    return out.cpu(), name, passes


def _one(prec, t, variant, what):
    got, name, passes = _run(t, detector(prec))
    assert name.split(" ")[0] == variant, "%s ran %r, the table says %s" % (what, name, variant)
    assert passes in ((2, 3) if prec == "fp16x3" else (0,))
    ratio = R.check(t, got, name, passes)
    print("CONV_SLICES %s [%s] passes %d: worst ratio %.3f" % (what, variant, passes, ratio))
    return got, name, passes


@pytest.mark.parametrize("n", range(len(CASES)), ids=[c[0] for c in CASES])
def test_conv_on_slices(n, monkeypatch):
    what, prec, geom, inv, env, variant, layout, act, seed = CASES[n]
    monkeypatch.setenv("CY_BATCH_INVARIANT", inv)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    # fp16x3: odd cases with an fp16-exact filter (the two-pass form), even ones with the general three-pass form
    t = R.build(prec, geom, act, layout, seed, w16=prec == "fp16x3" and n % 2 == 1)
    _, _, passes = _one(prec, t, variant, what)
    if prec == "fp16x3":
        assert passes == (2 if n % 2 == 1 else 3)


@pytest.mark.parametrize("n", range(len(ROW_CASES)), ids=[c[0] for c in ROW_CASES])
def test_conv_into_prediction_rows(n, monkeypatch):
    what, prec, geom, hd, variant, rows, seed = ROW_CASES[n]
    monkeypatch.setenv("CY_HEAD_DIRECT", str(hd))
    t = R.build(prec, geom, False, "rows", seed, rows=rows, w16=n % 2 == 1)
    _one(prec, t, variant, what)


def test_table_covers_every_variant():
    """The names asserted across the two tables are the names the library lists (runs after the tables in file order; on its own
    it reads the tables' expectations, which the cases assert)."""
    from caesar_yolo_amd import lib as L
    lib = L.load()
    listed = set()
    while lib.cy_conv_variant_name(len(listed)) is not None:
        listed.add(lib.cy_conv_variant_name(len(listed)).decode().split(" ")[0])
    asserted = set(c[5] for c in CASES) | set(c[4] for c in ROW_CASES)
    assert asserted == listed, "variants without a case: %s; names no variant has: %s" % (sorted(listed - asserted), sorted(asserted - listed))
    for prec, want in (("fp16", listed), ("fp16x3", {WIDE, DUAL, WIDE64, STRIP, D256, D128, HEAD, G128, G64}), ("fp32", {G128, G64})):
        assert set(c[5] for c in CASES if c[1] == prec) | set(c[4] for c in ROW_CASES if c[1] == prec) == want, prec


REPEAT = [n for n, c in enumerate(CASES) if c[6] == "slices"]


@pytest.mark.parametrize("n", REPEAT, ids=[CASES[n][0] for n in REPEAT])
def test_sliced_launch_is_repeatable(n, monkeypatch):
    """The whole output buffer, guards included, has the same bytes after every run of the same sliced case: a store that races
    with a neighbour's shows as a rare difference, not as a steady error."""
    what, prec, geom, inv, env, variant, layout, act, seed = CASES[n]
    monkeypatch.setenv("CY_BATCH_INVARIANT", inv)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = R.build(prec, geom, act, layout, seed)
    first, name, _ = _run(t, detector(prec))
    assert name.split(" ")[0] == variant
    for _ in range(4):
        again, _, _ = _run(t, detector(prec))
        assert again.numpy().tobytes() == first.numpy().tobytes(), what


def _refused(det, t, **change):
    """The entry must refuse the case with `change` applied, and leave the output buffer as it was."""
    from caesar_yolo_amd.lib import CyError
    from caesar_yolo_amd import lib as L
    import ctypes as C
    dev = {k: getattr(t, k).cuda() for k in ("in0", "in1", "res", "out") if getattr(t, k) is not None}
    a = L.cy_conv_layout()
    a.d_in0, a.in0_ct, a.in0_coff, a.c0, a.up0 = dev["in0"].data_ptr(), t.in0.shape[-1], t.in0_coff, t.c0, int(t.up0)
    if t.in1 is not None:
        a.d_in1, a.in1_ct, a.in1_coff, a.c1 = dev["in1"].data_ptr(), t.in1.shape[-1], t.in1_coff, t.c1
    if t.res is not None:
        a.d_res, a.res_ct, a.res_coff = dev["res"].data_ptr(), t.res.shape[-1], t.res_coff
    a.d_out, a.out_ct, a.out_coff = dev["out"].data_ptr(), t.out.shape[-1], t.out_coff
    if t.layout == "rows":
        a.rows, a.out_bs, a.out_ro = 1, t.rows["out_bs"], t.rows["out_ro"]
    a.B, a.Hi, a.Wi, a.Cin, a.Cout, a.k, a.s, a.act = t.geom + (int(t.act),)
    for k, v in change.items():
        setattr(a, k, dev["in0"].data_ptr() if v == "in0" else dev["out"].data_ptr() if v == "out" else v)
    w, b = t.w.numpy(), t.b.numpy()
    fp = C.POINTER(C.c_float)
    rc = det.lib.cy_conv_slices(det.ctx, C.byref(a), w.ctypes.data_as(fp), b.ctypes.data_as(fp), None, 0, None, det._stream())
    with pytest.raises(CyError):
        L.check(rc, det.ctx)
    assert rc == -1, "%s: status %d, not CY_ERR_ARG" % (change, rc)
    torch.cuda.synchronize()
    assert dev["out"].cpu().numpy().tobytes() == t.out.numpy().tobytes(), "refused with %s, yet the output buffer changed" % (change,)


@pytest.mark.parametrize("prec", ["fp16", "fp16x3", "fp32"])
def test_entry_refuses_bad_layouts(prec):
    det = detector(prec)
    s = R.build(prec, (2, 9, 11, 128, 72, 1, 1), True, "slices", 1)
    for change in (dict(in0_coff=s.in0.shape[-1] - s.c0 + 8), dict(out_coff=s.out.shape[-1] - 72 + 8), dict(res_coff=s.res.shape[-1] - 72 + 8),
                   dict(in0_coff=12), dict(out_coff=20), dict(res_coff=4), dict(in0_ct=s.in0.shape[-1] + 4), dict(out_ct=s.out.shape[-1] + 4),
                   dict(res_ct=s.res.shape[-1] + 4), dict(c0=120), dict(c0=124, Cin=124), dict(up0=1), dict(d_out="in0"), dict(d_res="out"),
                   dict(k=5), dict(s=3), dict(B=0), dict(d_in0=None), dict(d_out=None)):
        _refused(det, s, **change)
    c = R.build(prec, (2, 10, 12, 128, 72, 1, 1), True, "concat", 2)
    for change in (dict(c1=56), dict(c1=60, Cin=124), dict(c0=32 if prec != "fp32" else 16, c1=96 if prec != "fp32" else 112),
                   dict(in1_coff=c.in1.shape[-1] - c.c1 + 8), dict(d_in1=None), dict(d_out="in0")):
        _refused(det, c, **change)
    u = R.build(prec, (2, 10, 12, 128, 72, 1, 1), True, "upcat", 3)
    _refused(det, u, Hi=9)
    _refused(det, u, Wi=11)
    k3 = R.build(prec, (2, 10, 12, 128, 72, 3, 1), True, "slices", 4)
    _refused(det, k3, up0=1)
    _refused(det, k3, d_in1="out", c1=64, c0=64, in1_ct=128)
    r = R.build(prec, (2, 3, 5, 128, 5, 1, 1), False, "rows", 5, rows=dict(out_ct=69, out_coff=64, out_bs=3 * 5 + 29, out_ro=17))
    for change in (dict(out_ro=30), dict(out_ro=-1), dict(out_bs=31), dict(act=1), dict(out_coff=72), dict(d_res="in0", res_ct=8, Cout=8, out_ct=72)):
        _refused(det, r, **change)
