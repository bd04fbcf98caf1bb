// The conv dispatch: integer logic over ConvArgs and ConvKnobs (cy_conv_plan.h).  No HIP.
#include "cy_conv_plan.h"
#include "cy_plan.h"
#include <stdlib.h>

namespace cy {

// Kernel variants (also the keys of the profiling summary)
static const char* const kVariantNames[CONV_NUM_VARIANTS] = {
    "conv_igemm_kernel<2,2,4> generic 128x128", "conv_igemm_kernel<4,1,2> generic 128x64",
    "conv3x3_halo2_kernel 3x3 s1 16x16px x128ch (halo<2,2> for odd slab counts)", "conv3x3_pp_kernel<2> 3x3 s1 16x16px x64ch",
    "conv3x3_c64_kernel<64|32> 3x3 s1 persistent, Cin 64 or 32", "conv_igemm_kernel<4,2,4,3> generic 256x128, 3-slab ring",
    "conv3x3_wide_kernel 3x3 s1 16x32px x128ch, K slabs of 32",
    "conv1x1_direct_kernel<4,2> 1x1 256px x256ch, pixels to regs", "conv1x1_direct_kernel<2,2> 1x1 256px x128ch, pixels to regs",
    "conv3x3_wide_kernel<WN=1> 3x3 s1 16x32px x64ch", "conv3x3_wide_kernel<dual> 3x3 s1 2 images x 16x16px x128ch",
    "conv3x3_widep_kernel<strip> 3x3 s1 512 flattened px x128ch, persistent",
    "head1x1_kernel detect-head output 1x1, weights stationary in LDS, fp32 rows"};
const char* conv_variant_name(int v) { return v >= 0 && v < CONV_NUM_VARIANTS ? kVariantNames[v] : "?"; }

// the instantiation behind each launcher call of launch_conv (template arguments as the launchers take them)
static const char* const kKernelNames[CK_NUM_KERNELS] = {
    "conv3x3_wide_kernel<2> one patch", "conv3x3_widep_kernel<0> persistent", "conv3x3_widep_kernel<10> strip", "conv3x3_widep_kernel<12> strip",
    "conv3x3_wide_kernel<1>", "conv3x3_wide_kernel<2,dual>",
    "conv3x3_halo2_kernel", "conv3x3_halo_kernel<2,2>", "conv3x3_pp_kernel<2>", "conv3x3_c64_kernel<64>", "conv3x3_c64_kernel<32>",
    "conv1x1_direct_kernel<4,2,3>", "conv1x1_direct_kernel<4,2,3,K3>", "conv1x1_direct_kernel<4,2,3,FUSE2>", "conv1x1_direct_kernel<4,2,3,K3,FUSE2>",
    "conv1x1_direct_kernel<2,2,2>", "conv1x1_direct_kernel<2,4,2,K3>",
    "head1x1_kernel", "conv_igemm_kernel<2,2,4>", "conv_igemm_kernel<4,1,2>", "conv_igemm_kernel<4,2,4,3>"};
const char* conv_kernel_name(ConvKernel k) { return k >= 0 && k < CK_NUM_KERNELS ? kKernelNames[k] : (k == CK_BAD_ARGS ? "bad fp16x3 arguments" : "?"); }

// Batch-invariant kernel selection (default; CY_BATCH_INVARIANT=0 turns it off): every batch-size threshold below (and the
// stem fusion) is evaluated as if the batch held >= 256 tiles, so a layer always runs the SAME kernel and a tile's fp16
// results do not depend on how many tiles share its batch: catalogs are identical for any world size / batch split, as the
// reference's are for any MPI size.  Price: big-batch kernels on small batches (1 % of the 16k-mosaic rate; a single
// image runs kernels tuned for 256).  With 0 the thresholds see the real batch: fastest per batch size, last-bit differences
// between batch sizes.
ConvKnobs conv_knobs_env() {
    ConvKnobs k;
    auto knob = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
    k.batch_invariant = knob("CY_BATCH_INVARIANT", 1); k.strip = knob("CY_STRIP", 1); k.wide_dual = knob("CY_WIDE_DUAL", 1);
    if (const char* e = getenv("CY_DIRECT_MIN_BLOCKS")) k.direct_min_blocks = atol(e);
    k.head_direct = knob("CY_HEAD_DIRECT", 1); k.narrow_direct = knob("CY_NARROW_DIRECT", 1); k.head_pair = knob("CY_HEAD_PAIR", 1);
    k.wide_persist = knob("CY_WIDE_PERSIST", 1); k.x3_persist = knob("CY_X3_PERSIST", 0);
    k.direct_persist = knob("CY_DIRECT_PERSIST", 1); k.direct_persist_grid = knob("CY_DIRECT_PERSIST_GRID", 0);
    return k;
}

// The second weight copy (64-byte K chunks) is what the wide / strip / dual kernels and conv3x3_c64_kernel<32> read: every
// `a.wgt32` in conv_variant_x3 and conv_variant below relies on this predicate covering the layer (fp16x3: all 3x3 s1 layers with
// Cin % 64 == 0; fp16: those with more than 32 output channels -- the wide / strip / dual / wide-64 conditions -- and the Cin 32,
// Cout <= 64 layers of c64<32>).  A layer outside it takes the next kernel down the list, which reads wgt.
bool conv_second_copy(Precision p, int ci, int co, int k, int s, bool down_copy) {
    return p == PREC_F16X3 ? (k == 3 && s == 1 && ci % 64 == 0)
                           : p == PREC_F16 && k == 3 && ((s == 1 && ((ci % 64 == 0 && co >= 33) || (ci == 32 && co <= 64))) ||
                                                         (down_copy && s == 2 && ci == 64 && co == 128));
}

ConvArgs conv_geometry(const Plan& p, const Op& o, int B, int H, int W, int cm, int A, const int a_off[3]) {
    const ConvDesc& d = p.convs[o.conv];
    ConvArgs a{};
    const Tensor& t0 = p.tensors[o.in0];
    a.in0_ct = cm * t0.C; a.in0_coff = o.in0_coff; a.c0 = o.c0; a.up0 = o.up0;
    a.in0_lo = t0.C;
    int lev_in = o.up0 ? t0.level - 1 : t0.level;
    if (o.in1 >= 0) {
        const Tensor& t1 = p.tensors[o.in1];
        a.in1_ct = cm * t1.C; a.in1_coff = o.in1_coff; a.c1 = o.c1; a.in1_lo = t1.C;
        lev_in = t1.level;
    }
    a.B = B; a.Hi = H >> lev_in; a.Wi = W >> lev_in; a.k = d.k; a.s = d.s; a.act = d.act;
    a.Ho = d.s == 2 ? a.Hi / 2 : a.Hi; a.Wo = d.s == 2 ? a.Wi / 2 : a.Wi;
    a.Cin = d.cin; a.Cout = d.cout;
    if (o.out >= 0) {
        const Tensor& to = p.tensors[o.out];
        a.out_ct = cm * to.C; a.out_coff = o.out_coff; a.out_bs = a.Ho * a.Wo; a.out_ro = 0; a.out_f32 = 0; a.out_lo = to.C;
    } else {
        a.out_ct = 64 + p.nc; a.out_coff = o.pred_coff; a.out_bs = A; a.out_ro = a_off[o.pred_level]; a.out_f32 = 1;
    }
    if (o.res >= 0) { a.res_ct = cm * p.tensors[o.res].C; a.res_coff = o.res_coff; a.res_lo = p.tensors[o.res].C; }
    return a;
}

// idle share of the MFMA lanes of the 2-D patch form (16 x 32-pixel patches) and of the strip form on an H x W map
static double wide2d_cover(int H, int W) { return (double)((H + 15) / 16 * 16) * ((W + 31) / 32 * 32) / ((double)H * W); }
static double strip_cover(int H, int W) { return (double)(H + 1) * (W + 1) / ((double)H * W); }
// maps from 17 px wide (narrower ones down to 13 px belong to the dual-image / two-tap kernels), and the maps of a few pixels that no
// patch shape fits (8 x 8 and 4 x 4: the stride-16 / 32 levels of 128- and 256-px inputs): 27 % / 56 % idle lanes there instead of 75 % / 94 %
static bool strip_small(const ConvArgs& a) { return a.Wi >= 3 && a.Wi <= 12 && a.Hi >= 3 && a.Hi <= 126; }
static bool strip_fits(const ConvArgs& a) {
    return ((a.Wi >= 17 && a.Hi >= 17 && a.Wi <= 126) || strip_small(a)) && a.Cout % 16 == 0 && (long)a.B * (a.Hi + 1) * (a.Wi + 1) < (1L << 22);
}

// head1x1_kernel: which layers it takes -- the detect head's output 1x1s (fp32 prediction rows, no activation) and, since
// the end of round 4, every other single-segment 1x1 with <= 64 output channels and Cin a multiple of 64 (fp16 / split outputs into a
// channel slice, SiLU, residual).  Geometry only (no batch threshold), so a tile's result does not depend on its batch.
int head_rows(const ConvArgs& a) { const int c = a.Cout < 16 ? a.Cout : 16; const int g = (c + 3) / 4; return 16 * (g < 4 ? g : 4); }
static bool head_direct(const ConvArgs& a, int passes, const ConvKnobs& k) {
    if (!k.head_direct) return false;
    if (!(a.k == 1 && a.s == 1 && a.c1 == 0 && !a.up0 && a.Cin >= 64 && a.Cin % 64 == 0 && a.c0 == a.Cin && pad64(a.Cout) == 64 && a.Ho == a.Hi && a.Wo == a.Wi))
        return false;
    if (a.out_f32 ? (a.res || a.act) : (a.out_bs != a.Ho * a.Wo || a.out_ro != 0 || !k.narrow_direct)) return false;      // head rows: no residual / activation; inside the network: plain pixel order
    return (size_t)passes * (a.Cin / 64) * head_rows(a) * 128 <= 65536;
}

// the two output convolutions of a stride level as one launch (head1x1_pair_kernel): a = box branch (64 channels at column 0),
// b = class branch (nc channels at column 64) of the same pixels and prediction rows
int head_pair_pitch(int rowlen) { int tp = rowlen; while (tp % 8 != 4) ++tp; return tp; }      // conflict-free b128 rows
size_t head_pair_lds(Precision p, const ConvArgs& a, const ConvArgs& b) {
    const size_t pa = p == PREC_F16X3 ? a.split : 1, pb = p == PREC_F16X3 ? b.split : 1;
    return pa * (a.Cin / 64) * 64 * 128 + pb * (b.Cin / 64) * head_rows(b) * 128 + (size_t)8 * 16 * head_pair_pitch(a.out_ct) * 4;
}
bool head_pair_ok(Precision p, const ConvArgs& a, const ConvChoice& ca, const ConvArgs& b, const ConvChoice& cb, const ConvKnobs& k) {
    if (p == PREC_F32 || !k.head_pair) return false;
    if (ca.variant != CONV_HEAD_1X1 || cb.variant != CONV_HEAD_1X1) return false;
    if (a.B != b.B || a.Ho != b.Ho || a.Wo != b.Wo || a.out != b.out || a.out_ct != b.out_ct || a.out_bs != b.out_bs || a.out_ro != b.out_ro) return false;
    if (a.out_coff != 0 || a.Cout != 64 || b.out_coff != 64 || b.Cout < 1 || b.Cout != a.out_ct - 64) return false;
    return head_pair_lds(p, a, b) <= 128 * 1024;
}

// fp16x3 context: the kernels that carry the three-pass K walk -- the 512-px wide 3x3 kernel (128- / 64-channel / dual-image forms),
// the pixels-direct 1x1 / strided-3x3 kernel and the generic implicit GEMM for everything else.  The choice depends on the layer's
// geometry only, so a tile's result does not depend on the batch it travels in -- with one bound: the strip form addresses the
// flattened batch with 22 bits (strip_fits: B * (H + 1) * (W + 1) < 2^22), which a launch can only exceed beyond the 4 GiB a tensor
// may hold in this context (128 tiles of 640^2: 2^19.6 entries on the largest strip-form map), where cy_forward refuses the batch.
static int conv_variant_x3(const ConvArgs& a, const ConvKnobs& k) {
    const bool narrow = pad64(a.Cout) <= 64;
    if (a.k == 3 && a.s == 1 && a.c1 == 0 && !a.up0 && !a.out_f32 && a.Cin % 64 == 0 && a.wgt32 && a.out_bs == a.Ho * a.Wo && a.out_ro == 0) {
        const int wpad = (a.Wi + 31) / 32 * 32;
        const bool fits = (wpad - a.Wi) * 8 <= a.Wi;
        if (narrow && a.Wi % 32 == 0) return CONV_WIDE_64;
        if (narrow && a.Cin >= 128 && k.strip && strip_small(a) && strip_fits(a)) return CONV_STRIP_128;       // (see conv_variant)
        // strip form where 16 x 32 patches would idle > 4 % more lanes (geometry only: no batch threshold in this context)
        if (!narrow && k.strip && strip_fits(a) && strip_cover(a.Hi, a.Wi) + 0.04 < wide2d_cover(a.Hi, a.Wi)) return CONV_STRIP_128;
        if (!narrow && fits) return CONV_WIDE_128;
        if (!narrow && a.Wi <= 16 && a.Wi >= 14) return CONV_WIDE_DUAL;
    }
    if (!a.out_f32 && a.Cin % 64 == 0 && !narrow &&
        ((a.k == 1 && a.s == 1 && (a.c1 == 0 || a.c0 % 64 == 0)) || (a.k == 3 && a.s == 2 && a.c1 == 0 && !a.up0)))
        return pad64(a.Cout) >= 256 ? CONV_DIRECT_256 : CONV_DIRECT_128;
    if (head_direct(a, a.split, k)) return CONV_HEAD_1X1;
    return narrow ? CONV_GENERIC_64 : CONV_GENERIC_128;
}

static int conv_variant(Precision p, const ConvArgs& a, const ConvKnobs& k) {
    if (p == PREC_F16X3) return conv_variant_x3(a, k);
    const bool narrow = pad64(a.Cout) <= 64;
    const long Bv = k.batch_invariant && a.B < 256 ? 256 : a.B;     // the batch size the thresholds see
    // 3x3 stride-1 layers (fp16 context; the fp32 parity context keeps the generic kernel): halo-reuse kernels.
    //   Cout <= 64  : ping-pong kernel with 64-channel tiles (256 px x 64 ch per workgroup)
    //   Cout >= 128 : 8x16-pixel patches x 128 channels, two workgroups per CU
    if (p == PREC_F16 && a.k == 3 && a.s == 1 && a.c1 == 0 && !a.up0 && !a.out_f32 && a.Cin == 32 && narrow && a.wgt32 &&
        a.out_bs == a.Ho * a.Wo && a.out_ro == 0)
        return CONV_C64_PERSIST;                             // 32-channel variant of the persistent kernel
    if (p == PREC_F16 && a.k == 3 && a.s == 1 && a.c1 == 0 && !a.up0 && !a.out_f32 && a.Cin % 64 == 0 &&
        a.out_bs == a.Ho * a.Wo && a.out_ro == 0) {
        // 64-channel variant of the wide kernel for the box-head convs with deep inputs, when it fills the chip
        if (narrow && a.wgt32 && a.Cin >= 128 && a.Wi % 32 == 0 && Bv * ((a.Hi + 15) / 16) * (a.Wi / 32) >= 256) return CONV_WIDE_64;
        // 64 output channels on maps of a few pixels with deep inputs (the box head of 128- / 256-px inputs): the strip form with half
        // of its channel tile empty still beats the 16 x 16-pixel patches of the 64-channel kernels there (68 -> ~250 TFLOP/s on 4 x 4 maps)
        if (narrow && a.wgt32 && a.Cin >= 128 && k.strip && strip_small(a) && strip_fits(a)) return CONV_STRIP_128;
        if (narrow && a.Cin == 64) return CONV_C64_PERSIST;
        if (narrow) return CONV_PP_64;
        // strip form of the wide kernel (maps flattened to one dimension) where 16 x 32-pixel patches would leave > 4 % more of the MFMA
        // lanes idle: 80 / 40 / 20-px maps of 640-px inputs, 52 x 64 / 26 x 32 maps of the ragged 416 x 512 tiles.  CY_STRIP: 0 off,
        // 2 regardless of the launch size (tests).
        if (k.strip && a.wgt32 && strip_fits(a) && strip_cover(a.Hi, a.Wi) + 0.04 < wide2d_cover(a.Hi, a.Wi) &&
            (k.strip > 1 || strip_small(a) || Bv * (long)(a.Hi + 1) * (a.Wi + 1) / 512 * ((pad64(a.Cout) + 127) / 128) >= 200))      // (about one strip per CU; tiny maps: every alternative idles more)
            return CONV_STRIP_128;
        const int wpad = (a.Wi + 31) / 32 * 32;
        if (a.wgt32 && (wpad - a.Wi) * 8 <= a.Wi) return CONV_WIDE_128;     // <= 12.5 % of the patch columns idle
        // two 16-px-wide images side by side: +8 % over the two-tap halo kernel once it still fills the chip (half as many
        // workgroups), slower below that; CY_WIDE_DUAL=2 forces it (tests)
        if (k.wide_dual && a.wgt32 && a.Wi <= 16 && a.Wi >= 14 &&
            ((Bv + 1) / 2) * ((a.Hi + 15) / 16) * ((pad64(a.Cout) + 127) / 128) >= (k.wide_dual > 1 ? 1 : 224))
            return CONV_WIDE_DUAL;
        return CONV_HALO8_128;
    }
    if (p == PREC_F16 && head_direct(a, 1, k)) return CONV_HEAD_1X1;
    if (narrow) return CONV_GENERIC_64;
    // 1x1: pixels-direct kernel once there is at least one 256-pixel tile per CU (below that the 128x128 tiles of the generic
    // kernel fill the chip better).  CY_DIRECT_MIN_BLOCKS lets the parity tests force the path.
    if (p == PREC_F16 && !a.out_f32 && a.Cin % 64 == 0 &&
        ((a.k == 1 && a.s == 1 && (a.c1 == 0 || a.c0 % 64 == 0)) || (a.k == 3 && a.s == 2 && a.c1 == 0 && !a.up0 && (a.Cin >= 128 || pad64(a.Cout) < 256)))) {
        const long min_blocks = k.direct_min_blocks;
        const int bn = pad64(a.Cout) >= 256 ? 256 : 128;
        const long blocks = ((Bv * a.Ho * a.Wo + 255) / 256) * ((pad64(a.Cout) + bn - 1) / bn);
        if (min_blocks >= 0 && blocks >= min_blocks) return bn == 256 ? CONV_DIRECT_256 : CONV_DIRECT_128;
    }
    // 1x1 and strided convs with enough 256-pixel tiles to fill the chip: deeper-pipelined 256x128 tile
    const long M = Bv * a.Ho * a.Wo;
    if (p == PREC_F16 && (M / 256) * ((pad64(a.Cout) + 127) / 128) >= 256) return CONV_GENERIC_BIG;
    return CONV_GENERIC_128;
}

// Persistent form of the pixels-direct 256-channel tile (conv1x1_direct_kernel<4,2,3,...,PERSIST>; same arithmetic in the same order:
// bit-identical outputs; fp16 context, not the fused pair): one workgroup per CU walks the tiles and requests the next tile's first
// chunks and bias under the current tile's last chunks and epilogue.  Taken when every CU gets at least two tiles (512 tiles: 256
// CUs) and a tile has at least as many K chunks as the ring has slots (the boundary logic assumes a tile's own prologue is behind
// it); CY_DIRECT_PERSIST: 0 off, 2 regardless of the launch size (tests).  The real batch counts, under batch invariance too: the
// two forms give the same bits.  Measured per layer at batch 256 on 512-px tiles, three processes, against the one-tile form's own
// range (profiles/direct_persist.md): 1x1 layers -6..-14 %, strided 3x3 layers -19..-22 %, faster in at least two of three
// processes each; the one layer that was not is excluded by the chunk condition below.
static long direct_tiles(const ConvArgs& a) { return (((long)a.B * a.Ho * a.Wo + 255) / 256) * ((pad64(a.Cout) + 255) / 256); }
static bool direct_persist_form(Precision p, ConvKernel kernel, const ConvArgs& a, const ConvKnobs& k) {
    if (p != PREC_F16 || (kernel != CK_DIRECT_256_K1 && kernel != CK_DIRECT_256_K3) || !k.direct_persist || a.out_f32) return false;
    if ((a.Cin / 64) * (a.k == 3 ? 9 : 1) < 3 || (a.k == 3 && a.c1)) return false;
    // at two or three tiles per CU only from 16 chunks on: 512 -> 512 on 16 x 16 maps (model.8.cv1: 512 tiles of 8 chunks) measured
    // 0.054-0.057 ms against the one-tile form's 0.053 in three of three processes, while the 16- and 20-chunk layers on the same
    // maps (model.8.cv2, 9.cv2, 21.cv1, 21.cv2) are 6-10 % faster and 8-chunk layers with eight tiles per CU (model.6.cv1) 8 % faster
    const long tiles = direct_tiles(a), chunks = (a.Cin / 64) * (a.k == 3 ? 9 : 1);
    return k.direct_persist > 1 || (tiles >= 512 && (tiles >= 1024 || chunks >= 16));
}
const char* conv_choice_name(const ConvChoice& c) {
    if (c.direct_persist) return c.kernel == CK_DIRECT_256_K3 ? "conv1x1_direct_kernel<4,2,3,K3,PERSIST>" : "conv1x1_direct_kernel<4,2,3,PERSIST>";
    return conv_kernel_name(c.kernel);
}

// the instantiation below the variant
static ConvKernel conv_kernel(Precision p, int variant, const ConvArgs& a, const ConvKnobs& k) {
    const bool x3 = p == PREC_F16X3;
    switch (variant) {
        case CONV_C64_PERSIST: return a.Cin == 32 ? CK_C64_32 : CK_C64_64;
        case CONV_HALO8_128: return (a.Cin / 64) % 2 == 0 ? CK_HALO2 : CK_HALO_2_2;      // two taps per barrier: walks the 64-channel slabs in pairs
        case CONV_PP_64: return CK_PP_2;
        case CONV_GENERIC_BIG: return CK_GENERIC_BIG;
        case CONV_WIDE_128: {
            // fp16x3: persistent form (bit-identical) with CY_X3_PERSIST=1: measured before it became a default
            if (x3) return k.x3_persist && a.Cout % 16 == 0 ? CK_WIDE_128_PERSIST : CK_WIDE_128;
            // persistent form (same arithmetic in the same order: bit-identical outputs) when every CU gets at least two patches
            // and the output tile has whole 16-channel groups; CY_WIDE_PERSIST: 0 off, 2 regardless of the launch size (tests).
            // The real batch counts here, under batch invariance too: the two forms give the same bits.
            const long patches = (long)a.B * ((a.Wi + 31) / 32) * ((a.Hi + 15) / 16) * ((pad64(a.Cout) + 127) / 128);
            // Measured per layer at batch 256: 18-stage layers (Cin 128: model.4 / model.15 bottlenecks) -4..-6 %, 36-stage ones
            // -1.7..+1.5 %: taken for up to two slab pairs.
            if (k.wide_persist && a.Cout % 16 == 0 && (k.wide_persist > 1 || (patches >= 512 && a.Cin <= 128))) return CK_WIDE_128_PERSIST;
            return CK_WIDE_128;
        }
        case CONV_STRIP_128: return a.Wi <= 62 ? CK_STRIP_10 : CK_STRIP_12;
        case CONV_WIDE_64: return CK_WIDE_64;
        case CONV_WIDE_DUAL: return CK_WIDE_DUAL;
        case CONV_DIRECT_256:
            // (tried, not kept: 128 px x 256 ch tiles with two workgroups per CU, 2-12 % slower on every 256-channel 1x1 layer but
            // model.4.cv1 (-4 %): twice the weight pieces per MFMA cost more than the overlap buys; a 4-slot ring for this tile:
            // 256 VGPRs with spills, 3-10 % slower)
            // weight requests on 4 waves (one per SIMD) for the strided 3x3 layers, on all 8 for the 1x1s (same bits either way).  Measured
            // per layer at batch 256: four requesting waves are 2-5 % faster on model.5 / model.7 and 1-6 % slower on the 1x1s
            // back-to-back pair (the runtime sets wgt2 when this layer's only reader is a 256 -> <= 256 1x1 and the tile holds all channels)
            if (!x3 && a.wgt2 && pad64(a.Cout) == 256 && a.c1 == 0 && !a.res && !a.out_f32) return a.k == 3 ? CK_DIRECT_256_K3_FUSE2 : CK_DIRECT_256_K1_FUSE2;
            return a.k == 3 ? CK_DIRECT_256_K3 : CK_DIRECT_256_K1;
        case CONV_DIRECT_128:     // strided 3x3 (model.1): 64 px per wave, so every weight fragment feeds four MFMAs (-8 % vs 32 px)
            // 1x1 with a 128-channel tile = the HBM-bound layers (model.2.cv1/cv2): two workgroups per CU (126 VGPRs, one chunk
            // ahead) overlap each other's prologue/epilogue: -12 % against one workgroup with a 4-chunk ring
            return a.k == 3 ? CK_DIRECT_128_K3 : CK_DIRECT_128_K1;
        case CONV_HEAD_1X1: return CK_HEAD;
        case CONV_GENERIC_64: return CK_GENERIC_64;
        default: return CK_GENERIC_128;
    }
}

ConvChoice conv_choose(Precision p, const ConvArgs& a, const ConvKnobs& k) {
    ConvChoice c;
    c.variant = conv_variant(p, a, k);
    c.kernel = p == PREC_F16X3 && ((a.split != 2 && a.split != 3) || !a.oscale) ? CK_BAD_ARGS : conv_kernel(p, c.variant, a, k);
    c.direct_persist = direct_persist_form(p, c.kernel, a, k) ? 1 : 0;
    c.persist_grid = k.direct_persist_grid;
    return c;
}

}  // namespace cy
