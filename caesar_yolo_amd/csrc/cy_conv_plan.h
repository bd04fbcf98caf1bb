// Which kernel runs a convolution: the launch arguments, the run-time switches and the one decision over them (host side, no HIP;
// linked alone into tests/host/conv_plan_main.cpp and run on the CPU by tests/test_conv_plan_cpu.py).  The kernels and their
// launchers are in conv_igemm.hip; launch_conv there makes the launcher call that a ConvChoice names and decides nothing.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define CY_HOST_DEVICE __host__ __device__
#else
#define CY_HOST_DEVICE
#endif

namespace cy {

struct Plan;
struct Op;

// PREC_F16X3 ("fp16x3", the fast parity context): every activation is stored as TWO fp16 values hi = fp16(x), lo = fp16(x - hi)
// (22 significand bits), weights likewise after a per-output-channel power-of-two scale that keeps their low halves out of the
// fp16 subnormal range; a product x*w is evaluated as hi*hi + lo*hi + hi*lo on the fp16 matrix cores with fp32 accumulation
// (the dropped lo*lo term is 2^-22 relative), i.e. a layer is the tuned fp16 kernel over 3x the K.  Activation buffers keep the
// NHWC channel-slice scheme with 2*C halves per pixel: [C high halves | C low halves].
enum Precision { PREC_F16 = 0, PREC_F32 = 1, PREC_F16X3 = 2 };

// One fused Conv2d(+folded BN bias)(+SiLU)(+residual) over NHWC activations, as an implicit GEMM:
//   out[pix, n] = act( sum_{tap,c} in[pix(tap), c] * w[n, tap, c] + bias[n] ) (+ res[pix, n])
// Input may be the channel-concat of two NHWC segments (k == 1 only); segment 0 may be read through a
// nearest x2 upsample (nn.Upsample + Concat of yolov8 layers 10-11 / 13-14 folded into the consumer).
struct ConvArgs {
    const void* in0; int in0_ct, in0_coff, c0, up0;   // segment 0: base, channels per pixel of the buffer, channel offset, #channels
    const void* in1; int in1_ct, in1_coff, c1;        // segment 1 (c1 == 0: absent)
    const void* wgt;                                   // packed [K chunk][k*k][Cout_pad128][128 B]; rows permuted per 64 (pack_weights)
    const void* wgt32; uint32_t wgt32_bytes;           // second copy with 64-byte K chunks (3x3 s1 fp16 layers, conv3x3_wide_kernel) or null
    const float* bias;                                 // [Cout_pad64]
    void* out; int out_ct, out_coff;                   // NHWC destination slice
    int out_bs, out_ro;                                // destination pixel = b*out_bs + out_ro + (ho*Wo+wo)
    int out_f32;                                       // 1: store fp32 regardless of the activation type (detect head)
    const void* res; int res_ct, res_coff;             // residual source (same pixel grid) or null
    int B, Hi, Wi, Ho, Wo, Cin, Cout, k, s, act;
    uint32_t in0_bytes, in1_bytes, wgt_bytes;          // buffer extents for the hardware range check
    int dbg;                                           // developer ablation bits (0 in production)
    // fp16x3 context (split = passes over K: 3, or 2 when the layer's weights are fp16-exact up to a per-channel scale; 0 elsewhere): *_ct are in halves (2 * channels of the tensor); the low halves of a slice sit *_lo halves behind
    // its high halves.  wgt / wgt32 then hold 3 passes over K: [w_hi | w_lo | w_hi] against inputs [x_lo | x_hi | x_hi]; oscale[n] is
    // the power of two that undoes the weight scale of output channel n (applied to the accumulator before the bias).
    int split, in0_lo, in1_lo, out_lo, res_lo;
    const float* oscale;                               // [Cout_pad128] or null
    // back-to-back fusion (fp16 context, pixels-direct kernel with a 256-channel tile that holds ALL output channels of its pixels): the
    // fused Conv+bias+SiLU result of this layer is not stored but multiplied, in registers, by the 1x1 convolution that is its only
    // reader: wgt2 = that layer's packed weights with its INPUT channels permuted to the accumulator order of the kernel
    // (pack_weights_fused2), bias2 / act2 / out2* its bias, activation and destination slice (same pixel grid).  wgt2 == null: off.
    const void* wgt2; uint32_t wgt2_bytes; const float* bias2; int act2, cout2;
    void* out2; int out2_ct, out2_coff;
};

CY_HOST_DEVICE inline int pad64(int c) { return (c + 63) / 64 * 64; }
CY_HOST_DEVICE inline int pad128(int c) { return (c + 127) / 128 * 128; }

// Kernel variants: the keys of the profiling summary and what cy_conv_slices reports
enum ConvVariant { CONV_GENERIC_128 = 0, CONV_GENERIC_64, CONV_HALO8_128, CONV_PP_64, CONV_C64_PERSIST, CONV_GENERIC_BIG, CONV_WIDE_128, CONV_DIRECT_256, CONV_DIRECT_128, CONV_WIDE_64, CONV_WIDE_DUAL, CONV_STRIP_128, CONV_HEAD_1X1, CONV_NUM_VARIANTS };
const char* conv_variant_name(int v);

// One value per launcher call of launch_conv: the instantiation that runs, below the variant.  The three-pass (SPLIT) form of a
// kernel follows from the precision and is not a value of its own; neither are the ACT / RES instantiations a launcher picks.
enum ConvKernel {
    CK_WIDE_128 = 0, CK_WIDE_128_PERSIST, CK_STRIP_10, CK_STRIP_12, CK_WIDE_64, CK_WIDE_DUAL,
    CK_HALO2, CK_HALO_2_2, CK_PP_2, CK_C64_64, CK_C64_32,
    CK_DIRECT_256_K1, CK_DIRECT_256_K3, CK_DIRECT_256_K1_FUSE2, CK_DIRECT_256_K3_FUSE2, CK_DIRECT_128_K1, CK_DIRECT_128_K3,
    CK_HEAD, CK_GENERIC_128, CK_GENERIC_64, CK_GENERIC_BIG, CK_NUM_KERNELS,
    CK_BAD_ARGS = -1       // fp16x3 context without a pass count of 2 or 3 or without oscale: launch_conv returns hipErrorInvalidValue
};
const char* conv_kernel_name(ConvKernel k);

// The environment switches of the decision (selection among kernels that compute the same result; the parity tests force every
// form through them).  conv_knobs_env() is the only place that reads them: once per forward pass / test entry call.
struct ConvKnobs {
    int batch_invariant = 1;        // CY_BATCH_INVARIANT: 0 = the thresholds see the real batch
    int strip = 1;                  // CY_STRIP: 0 off, 2 regardless of the launch size
    int wide_dual = 1;              // CY_WIDE_DUAL: 0 off, 2 regardless of the launch size
    long direct_min_blocks = 256;   // CY_DIRECT_MIN_BLOCKS: negative = the pixels-direct kernel off
    int head_direct = 1;            // CY_HEAD_DIRECT
    int narrow_direct = 1;          // CY_NARROW_DIRECT
    int head_pair = 1;              // CY_HEAD_PAIR
    int wide_persist = 1;           // CY_WIDE_PERSIST: 0 off, 2 regardless of the launch size
    int x3_persist = 0;             // CY_X3_PERSIST: 1 = persistent wide kernel in the fp16x3 context
    int direct_persist = 1;         // CY_DIRECT_PERSIST: persistent form of the pixels-direct 256-channel tile; 0 off, 2 regardless of the launch size
    int direct_persist_grid = 0;    // CY_DIRECT_PERSIST_GRID: workgroups of that form (tests: several tiles per workgroup in a small launch); 0 = one per CU
};
ConvKnobs conv_knobs_env();

// direct_persist: CK_DIRECT_256_K1 / _K3 in the fp16 context run in their persistent form (same kernel template, trailing argument; same
// bits) -- a form below the kernel value, as the ACT / RES instantiations are; persist_grid: ConvKnobs::direct_persist_grid, for the launcher
struct ConvChoice { int variant; ConvKernel kernel; int direct_persist = 0; int persist_grid = 0; };
const char* conv_choice_name(const ConvChoice& c);      // conv_kernel_name, with the persistent form named
ConvChoice conv_choose(Precision p, const ConvArgs& a, const ConvKnobs& k);     // the whole decision, once

// whether upload_conv makes the second weight copy (64-byte K chunks, ConvArgs::wgt32) of a layer; down_copy: the loader's
// 3x3 s2 64 -> 128 layer gets it too (stem_down_kernel reads its weight fragments from it)
bool conv_second_copy(Precision p, int ci, int co, int k, int s, bool down_copy);

// every non-pointer field of a convolution op's launch arguments in a pass over B tiles of H x W: channel counts and offsets,
// *_lo, B / Hi / Wi / Ho / Wo / k / s / act / Cin / Cout, out_bs / out_ro / out_f32 (cm = halves per activation value, A = anchors
// of a prediction block, a_off = first anchor of each stride level).  Pointers, byte extents, split and oscale are the caller's.
ConvArgs conv_geometry(const Plan& p, const Op& o, int B, int H, int W, int cm, int A, const int a_off[3]);

// head1x1_kernel / head1x1_pair_kernel: rows of the weight panel, LDS pitch and bytes of the pair, and whether one launch of the
// pair kernel can run box branch a and class branch b of a stride level (ca / cb: their choices)
int head_rows(const ConvArgs& a);
int head_pair_pitch(int rowlen);
size_t head_pair_lds(Precision p, const ConvArgs& a, const ConvArgs& b);
bool head_pair_ok(Precision p, const ConvArgs& a, const ConvChoice& ca, const ConvArgs& b, const ConvChoice& cb, const ConvKnobs& k);

}  // namespace cy
