"""The checker of tests/conv_slices_ref.py can fail: driven by a torch stand-in for the device it accepts the correct
computation in every layout and rejects every seeded fault -- the address errors a kernel can make with channel slices (a
store past Cout, a shifted output slice, a residual offset ignored, a pixel stride taken from the wrong field, the upsample
read at full resolution, the row offset dropped) and two arithmetic ones (a tap dropped at one border pixel, a second
rounding before the store).  No GPU; the host-side parts of the entry (variant names, exports) are checked too."""
import pytest
import torch
import conv_slices_ref as R

ROWS = dict(out_ct=64 + 5, out_coff=64, out_bs=3 * 5 + 11, out_ro=7)
G3 = (2, 5, 7, 64, 40, 3, 1)           # 3x3: ragged Cout (two groups of 16 and one of 8)
G1 = (2, 4, 6, 72, 40, 1, 1)           # 1x1, two segments of 64 + 8 channels; even map for the upsample
GH = (2, 3, 5, 64, 5, 1, 1)            # class branch of the head, nc = 5


def _case(prec, layout, act=True):
    if layout == "rows":
        return R.build(prec, GH, False, "rows", 5, rows=ROWS)
    return R.build(prec, G1 if layout in ("concat", "upcat") else G3, act, layout, 11)


@pytest.mark.parametrize("act", [True, False])
@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_correct_device_passes(prec, layout, act):
    t = _case(prec, layout, act)
    ratio = R.check(t, R.emulate(t), "stand-in")
    print("CONV_SLICES_CPU %s %s act=%d: worst ratio %.3f" % (prec, layout, act, ratio))
    assert 0.0 < ratio <= 1.0


def test_buffers_hold_their_guards():
    for layout in R.LAYOUTS:
        t = _case("fp16", layout)
        m = R.out_mask(t)
        assert int(m.sum()) == t.geom[0] * t.Ho * t.Wo * t.geom[4]
        assert bool(torch.isfinite(t.out.float()).all())
        guards = t.out.float()[~m]
        if layout != "dense":
            assert guards.numel() > 0 and bool((guards[1:] != guards[:-1]).any())
        for buf, coff, c in ((t.in0, t.in0_coff, t.c0), (t.in1, t.in1_coff, t.c1), (t.res, t.res_coff, t.geom[4])):
            if buf is None:
                continue
            inside = torch.zeros(buf.shape[-1], dtype=torch.bool)
            inside[coff:coff + c] = True
            assert bool(torch.isnan(buf[..., ~inside].float()).all()) and bool(torch.isfinite(buf[..., inside].float()).all())
    t = _case("fp16", "rows")
    assert t.out.dtype == torch.float32 and t.rows["out_ro"] > 0 and t.rows["out_ro"] + t.Ho * t.Wo < t.rows["out_bs"]


# each fault on a layout in which it moves an address (with ct == C and offset 0 several wrong formulas give the right one)
MUTANT_LAYOUT = {"store_past_cout": "slices", "out_coff_plus8": "slices", "res_coff_ignored": "slices", "in0_ct_is_c0": "slices",
                 "in1_at_in0_stride": "concat", "up_full_res": "upcat", "out_ro_dropped": "rows", "tap_dropped": "shared",
                 "double_rounding": "dense"}


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_rejected(mutant, prec):
    t = _case(prec, MUTANT_LAYOUT[mutant])
    R.check(t, R.emulate(t), "stand-in")
    bad = R.emulate(t, mutant)
    assert bad.numpy().tobytes() != R.emulate(t).numpy().tobytes(), "the mutant changed nothing"
    with pytest.raises(AssertionError) as info:
        R.check(t, bad, mutant)
    print("CONV_SLICES_CPU mutant %s %s: %s" % (mutant, prec, str(info.value).split("\n")[0][:200]))


def test_store_past_cout_is_caught_by_the_guards_alone():
    """The spilled vector leaves every slice element right: only the guard comparison can see it."""
    t = _case("fp16", "slices")
    bad = R.emulate(t, "store_past_cout")
    assert torch.equal(R.out_slice(t, bad), R.out_slice(t, R.emulate(t)))
    with pytest.raises(AssertionError, match="guard element"):
        R.check(t, bad)


def test_dense_layout_hides_the_address_faults():
    """Why the sliced layouts exist: with ct == C and offset 0 these faults compute the same addresses."""
    t = _case("fp16", "dense")
    good = R.emulate(t)
    for mutant in ("res_coff_ignored", "in0_ct_is_c0"):
        assert torch.equal(R.emulate(t, mutant).view(torch.int16), good.view(torch.int16)), mutant


def test_variant_names_are_listed_on_the_host():
    from caesar_yolo_amd import lib as L
    lib = L.load()
    names = []
    while lib.cy_conv_variant_name(len(names)) is not None:
        names.append(lib.cy_conv_variant_name(len(names)).decode())
        assert len(names) < 64
    assert len(names) == 13 and len(set(n.split(" ")[0] for n in names)) == 13
    assert lib.cy_conv_variant_name(-1) is None and lib.cy_conv_variant_name(len(names) + 5) is None
