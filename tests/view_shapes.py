"""The convolution shapes that only the augmentation views bring: every distinct
    (kernel name, Hi, Wi, Cin, Cout, k, s, res)
that a B = 1 forward takes at 224 x 224 or 192 x 192 but not at 256 x 256, for the two seeded images (YOLOv8 l and YOLO11 l, five
classes) in the fp16 and the fp16x3 context.  The fp16x3 rows hold for split 2 and split 3 alike.

The rows are recorded results of the dispatch (conv_plan_main's IMAGE mode at the parent commit, queries `1 H W prec split inv`) and
live as plain data in tests/golden/view_shapes.txt:
    IMAGE PRECISION INV | KERNEL | Hi Wi Cin Cout k s res
INV 0 is the query with batch invariance off; INV 1 is what a forward pass runs at default switches (CY_BATCH_INVARIANT=1: the
fp16 context then selects as if the batch were large; fp16x3 selects by geometry alone, its two sets are equal).
tests/test_view_shapes_cpu.py asks the dispatch of this tree for the same set differences and compares; a dispatch change that moves
a view onto another kernel fails there first.  tests/test_gpu_neighbour.py runs every row through cy_conv_slices.

Lines marked `IMAGE PRECISION INV 256` are the rest of the dispatch: one shape of the 256-px input per kernel that the B = 1
forwards take there and that no view row names, so that the GPU test runs every kernel of the B = 1 dispatch once."""
import os
import conv_slices_ref as R

IMAGES = ("seeded:l:5", "seeded11:l:5")
CONTEXTS = (("fp16", (0,)), ("fp16x3", (2, 3)))                # precision, the splits it is asked with
INVS = (0, 1)
SIZES = (256, 224, 192)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "view_shapes.txt")

# kernel (conv_kernel_name) -> first word of the variant cy_conv_slices reports for it (conv_variant_name)
KERNEL_VARIANT = {"conv1x1_direct_kernel<2,2,2>": R.D128, "conv1x1_direct_kernel<2,4,2,K3>": R.D128, "conv1x1_direct_kernel<4,2,3>": R.D256,
                  "conv1x1_direct_kernel<4,2,3,K3>": R.D256, "conv3x3_c64_kernel<32>": R.C64, "conv3x3_c64_kernel<64>": R.C64,
                  "conv3x3_halo2_kernel": R.HALO, "conv3x3_halo_kernel<2,2>": R.HALO, "conv3x3_pp_kernel<2>": R.PP,
                  "conv3x3_wide_kernel<2,dual>": R.DUAL, "conv3x3_widep_kernel<10> strip": R.STRIP, "conv_igemm_kernel<2,2,4>": R.G128,
                  "conv_igemm_kernel<4,1,2>": R.G64, "conv_igemm_kernel<4,2,4,3>": R.BIG, "head1x1_kernel": R.HEAD,
                  "conv3x3_wide_kernel<2> one patch": R.WIDE, "conv3x3_wide_kernel<1>": R.WIDE64,
                  "conv1x1_direct_kernel<4,2,3,K3,FUSE2>": R.D256}
# The first op of a pixel-wise pair (fp16 context, default switches) runs with the second op's filter in one launch.  cy_conv_slices
# takes one convolution, so such a row runs there on the kernel of the single op; the pair itself runs in the forward-level tests.
UNFUSED = {"conv1x1_direct_kernel<4,2,3,K3,FUSE2>": "conv1x1_direct_kernel<4,2,3,K3>"}


def _read():
    view, rest = {}, {}
    for ln in open(GOLDEN):
        if ln.startswith("#") or not ln.strip():
            continue
        head, kernel, geom = [f.strip() for f in ln.split(" | ")]
        head = head.split()
        row = (kernel,) + tuple(int(v) for v in geom.split())
        assert len(row) == 8 and kernel in KERNEL_VARIANT and len(head) in (3, 4), ln
        (rest if len(head) == 4 else view).setdefault((head[0], head[1], int(head[2])), []).append(row)
    return view, rest


# {(image, precision, inv): [row]}: the view rows, and the one-per-remaining-kernel rows of the 256-px input
TABLE, REST_256 = _read()


def rows_layout(row):
    """The head's output convolutions write fp32 prediction rows without activation: the `rows` layout of conv_slices_ref.  Every
    other row runs dense.  -> dict(out_ct, out_coff, out_bs, out_ro) or None."""
    kernel, Hi, Wi, _, Cout, k, s, res = row
    if kernel != "head1x1_kernel":
        return None
    assert k == 1 and s == 1 and not res
    # the box branch (64 columns at 0) or a class branch (behind the 64 box columns) of a level with rows before and behind it
    box = Cout == 64
    return dict(out_ct=64 + (5 if box else Cout), out_coff=0 if box else 64, out_bs=Hi * Wi + 29, out_ro=17)


def gpu_cases(prec):
    """[(id, row, CY_BATCH_INVARIANT)] of one context: the view rows of both images without repeats, then the rest of the B = 1
    dispatch.  A row that both settings of batch invariance give runs at the default (1); one that only one gives, at that one."""
    seen, out = set(), []
    for tag, table in (("view", TABLE), ("256", REST_256)):
        for inv in (1, 0):
            for image in IMAGES:
                for row in table.get((image, prec, inv), ()):
                    row = (UNFUSED.get(row[0], row[0]),) + row[1:]
                    if row not in seen:
                        seen.add(row)
                        out.append(("%s-%s-%s%s%s" % (tag, row[0].replace(" ", "_"), "x".join(map(str, row[1:7])), "-res" if row[7] else "",
                                                      "" if inv else "-inv0"), row, str(inv)))
    return out
