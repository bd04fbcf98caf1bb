"""The per-pixel tail of the conv epilogue (store_px / store_px_split in csrc/cy_conv_dev.h): every kernel that calls it, and
the pixels-direct and persistent 64-channel kernels with tails of their own, is driven through both branches -- whole
16-channel groups as vectors, a ragged group scalar by scalar -- with a residual.
Each case's channel count leaves one lane group full, one ragged and one empty (200 = 12 x 16 + 8 of a 256-channel tile,
72 = 4 x 16 + 8 of 128, 40 = 2 x 16 + 8 of 64); the shapes are the smallest that select each kernel, read off conv_variant and
launch_conv.  The check is test_conv_bn_silu's own (F.conv2d reference, its tolerances: 4e-3 of max(scale, 1) for fp16 on
fp16-rounded operands, 2e-5 for fp32 and fp16x3)."""
import pytest
from test_gpu_conv import test_conv_bn_silu as check_conv

pytestmark = pytest.mark.gpu

DIRECT = {"CY_DIRECT_MIN_BLOCKS": "1"}

# (B, H, W, Cin, Cout, k, s), CY_BATCH_INVARIANT, further knobs; the comment names the kernel the case selects
FP16 = [
    ((1, 10, 32, 128, 200, 3, 1), "1", {}),       # conv3x3_wide_kernel<2>: one-patch wide kernel, 128-channel tiles (Cout % 16 != 0: not persistent)
    ((3, 9, 15, 128, 200, 3, 1), "1", {}),        # conv3x3_wide_kernel<2, dual> (CY_WIDE_DUAL=2, set by the check itself)
    ((1, 10, 20, 128, 200, 3, 1), "1", {}),       # conv3x3_halo2_kernel: two taps per barrier (two 64-channel slabs)
    ((1, 10, 20, 64, 200, 3, 1), "1", {}),        # conv3x3_halo_kernel<2, 2> (one slab)
    ((1, 10, 32, 128, 40, 3, 1), "1", {}),        # conv3x3_wide_kernel<1>: 64-channel tiles
    ((2, 10, 18, 128, 40, 3, 1), "1", {}),        # conv3x3_pp_kernel<2>: 8 channels per lane
    ((2, 20, 18, 64, 40, 3, 1), "1", {}),         # conv3x3_c64_kernel<64>: the persistent kernel's own tail
    ((2, 9, 11, 128, 200, 1, 1), "1", DIRECT),    # conv1x1_direct_kernel<4, 2, 3>: 256-channel tile
    ((2, 9, 11, 128, 72, 1, 1), "1", DIRECT),     # conv1x1_direct_kernel<2, 2, 2>: 128-channel tile
    ((2, 18, 22, 128, 200, 3, 2), "1", DIRECT),   # conv1x1_direct_kernel<4, 2, 3, K3>: strided 3x3
    ((2, 9, 11, 128, 40, 1, 1), "1", {}),         # head1x1_kernel inside the network (fp16 slice, SiLU, residual)
    ((2, 9, 15, 72, 200, 1, 1), "1", {}),         # conv_igemm_kernel<4, 2, 4, 3>: 256 x 128 ring (135 px x 256 tiles as seen by the thresholds)
    ((2, 9, 11, 72, 40, 1, 1), "1", {}),          # conv_igemm_kernel<4, 1, 2>: generic 128 x 64
    ((2, 9, 11, 72, 200, 1, 1), "0", {}),         # conv_igemm_kernel<2, 2, 4>: generic 128 x 128 (thresholds see the real batch)
]
# fp16x3: the kernels that carry the split tail -- wide, dual, wide-64, the three direct forms, head, both generic tiles
X3 = [FP16[i] for i in (0, 1, 4, 7, 8, 9, 10, 13, 12)]
# fp32: the generic kernel keeps its own float stores; the two tiles
F32 = [FP16[13], FP16[12]]

# (CY_BATCH_INVARIANT only moves thresholds of the fp16 context: fp16x3 and fp32 select by geometry alone and run with "1",
# whatever the fp16 entry of the same shape says -- FP16[13] is reused here for its shape, not for its "0")
ALL = [("fp16",) + c for c in FP16] + [(p, g, "1", k) for p, cases in (("fp16x3", X3), ("fp32", F32)) for g, _, k in cases]


@pytest.mark.parametrize("n", range(len(ALL)), ids=["%s-%s-inv%s" % (p, "x".join(map(str, g)), inv) for p, g, inv, _ in ALL])
def test_conv_tail_with_residual(n, monkeypatch):
    prec, geom, inv, knobs = ALL[n]
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    check_conv(prec, inv, geom + (n % 2 == 0, True), monkeypatch)      # every case with a residual, half without activation
