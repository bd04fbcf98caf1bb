// Internal launch interfaces between the runtime (cy_context.cpp) and the gfx950 kernels.
// Nothing here is part of the C-ABI (see include/caesar_yolo_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "cy_measure_jobs.h"
#include "cy_conv_plan.h"      // Precision, ConvArgs, ConvVariant, ConvChoice, pad64 / pad128: the conv dispatch (host code without HIP)

namespace cy {

// Environment switches come in two classes.  env_knob(): selection among kernels / schedules that all compute the same
// result (CY_BATCH_INVARIANT, CY_DUAL_FORWARD, CY_STEM_FUSE, CY_WIDE_DUAL, CY_DIRECT_MIN_BLOCKS, ... -- the parity tests force
// every variant through them), always available.  dev_knob(): developer ablation switches that SKIP work and therefore
// invalidate results (CY_DBG, CY_SD_DBG): read only in a diagnostic build (-DCY_DEV_KNOBS=1, `CY_STAMPS=1 python
// __graft_entry__.py --force`); in the product binary they are the constant default.
#ifndef CY_DEV_KNOBS
#define CY_DEV_KNOBS 0
#endif
inline int env_knob(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
inline int dev_knob(const char* name, int dflt) { return CY_DEV_KNOBS ? env_knob(name, dflt) : dflt; }

// Launch of a kernel that needs more dynamic LDS than the 64 KiB a kernel gets by default.  lds_cap(): raises the limit of one
// kernel instantiation to `cap` bytes, once (the flag is a function-local static of a template keyed on the kernel: one per
// instantiation; the attribute call's own status is not looked at: a launch above the limit fails and reports that).
// launch_lds(): does that on the kernel's first launch, launches with `lds` bytes and returns the launch's error.
// A launcher that picks among several instantiations at run time and wants all of them ready before the first launch calls
// lds_cap() for each and then launch_lds() for the one it picked.
template <auto Kernel> void lds_cap(size_t cap) {
    static bool done = false;
    if (done) return;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)cap);
    done = true;
}
template <auto Kernel, typename... A> hipError_t launch_lds(dim3 grid, dim3 block, size_t lds, size_t cap, hipStream_t s, A... args) {
    lds_cap<Kernel>(cap);
    hipLaunchKernelGGL(Kernel, grid, block, lds, s, args...);
    return hipGetLastError();
}

// First layer (Cin = 3 stored as 4, k=3, s=2): direct convolution.
struct StemArgs {
    const void* in; void* out; const float* w; const float* bias;   // w: [27][Cout] fp32 (tap-major, then c)
    const void* wpk;                                                // fp16 context: [64][32] packed panel (pack_stem_weights)
    int B, Hi, Wi, Ho, Wo, Cout, out_ct, out_coff;
    int out_lo;                                                     // fp16x3 context: fp32 input, output as high / low halves (see ConvArgs)
};

// model.0 + model.1 of the YOLOv8/YOLO11 graphs in one kernel (fp16 context): the 64-channel half-resolution map (8 MB
// per 512x512 tile) never goes to HBM
struct StemDownArgs {
    const void* in; uint32_t in_bytes; int B, Hi, Wi;                  // NHWC4 fp16 network input
    const void* wpk2; const float* bias0;                               // stem panel [64][64] fp16 (pack_stem_weights2), bias
    const void* wgt32; uint32_t wgt32_bytes; const float* bias1;        // 3x3 s2 64->128 weights, 64-byte K chunks (pack_weights(..., 64))
    void* out; int out_ct, out_coff;
    int H1, W1, Ho, Wo;                                                 // stem map, output map
    int dbg;                                                            // developer timing switches (CY_SD_DBG): skip a phase
};

// Fused Bottleneck(64 -> 64 -> 64, 3x3 + 3x3 stride 1, SiLU, optional shortcut) on NHWC fp16 channel slices (bneck64.hip)
struct BneckArgs {
    const void* in; int in_ct, in_coff; uint32_t in_bytes;     // input slice (also the residual when shortcut)
    void* out; int out_ct, out_coff;                            // output slice (same pixel grid)
    const void* wfrag;                                          // pack_bneck_weights: [conv][block][k-step][lane] x 16 B
    const float* bias1; const float* bias2;                     // folded biases of cv1 / cv2
    int B, H, W, shortcut;
    int dbg;                                                    // developer ablation bits (0 in production)
};
constexpr size_t BNECK_WFRAG_BYTES = 2 * 4 * 18 * 1024;
hipError_t launch_bneck64(const BneckArgs& a, hipStream_t s);
void pack_bneck_weights(const float* W1, const float* W2, void* dst);      // W: [64][64][3][3] fp32

struct PoolArgs {   // MaxPool2d(5,1,2) on a channel slice of an NHWC buffer, -inf padding
    const void* src; void* dst; int ct, src_coff, dst_coff, C, B, H, W;
    int lo;                                            // fp16x3 context: offset of the low halves (0: plain)
};

// YOLO11 operators (cy_extra.hip)
struct DwArgs {     // depth-wise 3x3 stride 1 over NHWC channel slices; w: [9][C] fp32, bias [C] fp32
    const void* in; int in_ct, in_coff; void* out; int out_ct, out_coff; const void* res; int res_ct, res_coff;
    const float* w; const float* bias; int B, H, W, C, act;
    int blk, gstride, goff;                            // input channel of output channel c: (c/blk)*gstride + goff + c%blk (blk = 0: c)
    int in_lo, out_lo, res_lo;                         // fp16x3 context: offsets of the low halves (see ConvArgs)
    int xcd;                                           // set by the launch: workgroups in XCD-contiguous order
};
struct AttnArgs {   // softmax(q^T k * scale) applied to v, per head; qkv channels per head: [q kd | k kd | v hd]
    const void* qkv; int ct, coff; void* out; int out_ct, out_coff; int B, N, heads, kd, hd; float scale;
    int lo, out_lo;                                    // fp16x3 context: offsets of the low halves of qkv / out
};
hipError_t launch_dwconv(Precision p, const DwArgs& a, hipStream_t s);
hipError_t launch_attention(Precision p, const AttnArgs& a, hipStream_t s);

hipError_t launch_conv(Precision p, const ConvChoice& choice, const ConvArgs& a, hipStream_t s);      // the launcher call conv_choose named (cy_conv_plan.h)
// the two output 1x1s of a detect-head level (box branch a, class branch b) in one launch of head1x1_pair_kernel (conv_igemm.hip), where head_pair_ok
hipError_t launch_head_pair(Precision p, const ConvArgs& a, const ConvArgs& b, hipStream_t s);
void debug_read_stamps(unsigned long long* out8, bool reset);
void debug_read_wg_life(unsigned long long* out, int n);        // entry, exit, CU per workgroup of the pixels-direct kernel (n x 3), stamped builds
void debug_read_wg_stamps(unsigned long long* out, int n);     // raw per-workgroup phase records (n x 4), stamped builds   // developer diagnostics (CY_DBG=64)
void debug_read_pre_stamps(unsigned long long* out8, bool reset);
void debug_fastdiv(const double* d_a, const double* d_b, double* d_fast, double* d_ref, int n);      // fast_div vs `/` (cy_preproc.hip)   // phases of pre_stats_kernel (cy_preproc.hip), stamped builds only
void debug_reduce(const double* d_val, const float* d_key, int nrows, int len, unsigned long long* d_out);      // cy_reduce.h on its own (cy_measure.hip)
hipError_t launch_lds_fill(unsigned pattern, hipStream_t s, int* bytes);      // test hook: `pattern` over all LDS of one workgroup per CU (cy_extra.hip)
hipError_t launch_stem(Precision p, const StemArgs& a, hipStream_t s);
hipError_t launch_stem_down(const StemDownArgs& a, hipStream_t s);
long stem_down_blocks(const StemDownArgs& a);
void pack_stem_weights2(const float* W, int cout, void* dst);     // 64*64 fp16, k = tap*4 + c (taps 0..7), 32 + c (tap 8)
hipError_t launch_pool5(Precision p, const PoolArgs& a, hipStream_t s);

// Host-side weight packing into the layout launch_conv expects.
//   W: [Cout][Cin][k][k] fp32 -> dst: [Cout_pad64][k*k][Cin] (fp16 or fp32), rows permuted within each 64-row group
//   so that MFMA row (ni, rr) holds channel 64*blk + 16*(rr>>2) + 4*ni + (rr&3).
size_t packed_weight_bytes(Precision p, int cout, int cin, int k, int chunk_bytes = 128);
void pack_weights(Precision p, const float* W, int cout, int cin, int k, void* dst, int chunk_bytes = 128);
// second layer of a back-to-back pair (ConvArgs::wgt2): [cout2][cin2] 1x1 weights, cin2 = 256, packed like pack_weights(PREC_F16, ...,
// k = 1) with input channel 64 c + 16 q + 8 kk + j stored at K position 64 c + 32 kk + 8 q + j (what lane quarter q of the first
// layer's accumulators holds, in the order the MFMA B operand wants it)
void pack_weights_fused2(const float* W2, int cout2, int cin2, void* dst);
// fp16x3 context: scaled [hi | lo | hi] passes (each pass padded to whole K chunks); oscale: [pad128(cout)] floats, 2^-s per channel.
// passes = 2: [w16 | w16] of a filter that is exactly fp16 values times a per-channel scale (oscale = scale); x3_passes() tells which
// form a layer admits (scale: [cout] or null = ones).
int x3_passes(const float* W, int cout, int cin, int k, const float* scale);
size_t packed_weight_bytes_x3(int cout, int cin, int k, int chunk_bytes = 128, int passes = 3);
void pack_weights_x3(const float* W, int cout, int cin, int k, void* dst, float* oscale, int chunk_bytes = 128, int passes = 3, const float* scale = nullptr);
// fp32 NHWC [npix][C] <-> high/low halves [npix][2C] (test entry cy_conv_bn_silu, debug reads)
hipError_t launch_x3_split(const float* in, void* out, long npix, int C, hipStream_t s);
hipError_t launch_x3_merge(const void* in, float* out, long npix, int C, hipStream_t s);
void pack_stem_weights(const float* W, int cout, void* dst);      // 64*32 fp16
// Workgroups b and b + 8 share an XCD (round-robin dispatch over the 8 XCDs, each with its own L2): give each XCD a contiguous run of
// work items so that neighbours in the index space (adjacent image rows of a stencil, channel blocks of the same pixels) meet in one L2.
// Bijective for any number of workgroups.
__device__ __forceinline__ int xcd_contiguous(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}

// ---- detection post-processing --------------------------------------------------------------
struct DecodeArgs {
    const float* pred;       // [B][A][64+nc] raw head output (box logits, class logits)
    int B, A, nc;
    int lvl_h[3], lvl_w[3];  // grid of each stride-8/16/32 level
    float conf;
    // outputs: candidates per tile (fixed capacity cap), in anchor order
    float* cand;             // [B][cap][6]  x1,y1,x2,y2 (letterboxed px), score, class
    int* cand_anchor;        // [B][cap]
    int* cand_count;         // [B] (may exceed cap; clamped by consumers)
    int cap;
};
hipError_t launch_decode(const DecodeArgs& a, hipStream_t s);

// ---- box branch of the detect head at candidate anchors only (detect_post.hip: mark; cy_sparse_box.hip: the three stages) ----
enum BoxWalk { BOX_WALK_WIDE = 0, BOX_WALK_PP = 1, BOX_WALK_C64 = 2 };     // K walk + epilogue of the dense kernel of stage 1
constexpr int BOX_GRID = 512;                   // workgroups (four waves of 64 list entries) per level and stage: a fixed grid, the
                                                // waves stride over the lists by the device-side counts
struct BoxLevel {
    int sparse;                                 // 0: this level's box branch ran dense in the forward pass; nothing is done here
    int H, W, a_off;                            // map of the level, its first anchor in a prediction block
    int cap;                                    // B * H * W: entries the lists, the slot map and s1 / s2 hold
    const void* feat; int feat_ct, feat_coff, cin; uint32_t feat_bytes;      // input of stage 1: NHWC fp16 feature map, channel slice
    const void* w1; uint32_t w1_bytes; const float* b1; int walk1;           // cv2.l.0: wgt32 (BOX_WALK_WIDE) or wgt, bias
    const void* w2; uint32_t w2_bytes; const float* b2;                      // cv2.l.1: wgt (128-byte K chunks), bias
    const void* w3; uint32_t w3_bytes; const float* b3;                      // cv2.l.2: wgt, bias
    int* map;                                   // [cap] slot of a listed pixel in plist / s1, -1: not needed (set by the caller), -2: flagged; the three
                                                // levels' maps are ONE array of B * A words: L[l].map = L[0].map + B * L[l].a_off
    int* plist; int* clist;                     // [cap] stage-1 pixels (entry = slot) / candidate pixels, as b * H * W + y * W + x, in the atomics' order
    int* counts;                                // [2] entries of plist, of clist (zeroed by the caller)
    void* s1; void* s2;                         // [cap][64] fp16: stage-1 values by slot, stage-2 values by candidate entry
};
struct BoxArgs {
    BoxLevel L[3];
    float* pred; int B, A, nc;                  // [B][A][64+nc]: class columns are final, box columns are written at candidates
    float conf;
};
hipError_t launch_box_mark(const BoxArgs& a, hipStream_t s);      // candidate test of decode_kernel -> clist, map, plist, counts
hipError_t launch_box_sparse(const BoxArgs& a, hipStream_t s);    // stages 1-3 over the lists

struct NmsArgs {
    const float* cand; const int* cand_anchor; const int* cand_count; int cap;   // from decode
    int B; float iou; int max_det;
    // letterbox undo (ultralytics scale_boxes): x = (x - padw)/gain, clamp to [0,w0]x[0,h0]
    float gain; int padw, padh, w0, h0;
    float* det;              // [B][max_det][6]
    int* det_anchor;         // [B][max_det] anchor index of each kept detection (parity witness)
    int* det_count;          // [B]
    // workspace
    uint64_t* keys;          // [B][cap_pow2]
    uint64_t* mask;          // [B][cap][cap/64]
    int* counters;           // context counters (cy_detect_counters) or null: [1] += 1 for a tile whose candidates overflowed cap
};
hipError_t launch_nms(const NmsArgs& a, hipStream_t s);

struct MergeArgs {          // Analyzer.process_detections on device
    const float* det; const int* det_count; int B, max_det;
    float score_thr; double soft, hard;
    float* out; int* out_count; int* out_src;    // [B][max_det][6], [B], [B][max_det] (index into det rows)
    int* err;               // [B] number of degenerate boxes dropped (reference would assert)
    int* counters;          // context counters or null: [0] += degenerate boxes dropped
};
hipError_t launch_iou_merge(const MergeArgs& a, hipStream_t s);
// gathered tile records -> per-tile counts / status / prefix (hdr: 3 T + 1 ints) and the valid detections in tile-id order (out)
hipError_t launch_compact_records(const float* g, long long rows, const long long* perm, int T, int stride, int* hdr, float* out, hipStream_t s);

// ---- preprocessing ---------------------------------------------------------------------------
enum PreOp { OP_BKG = 1, OP_SHIFT = 2, OP_CLIP = 3, OP_ZSCALE = 4, OP_HISTEQ = 5, OP_MINMAX = 6 };
struct PreStage { int op; double p0, p1, p2; int flag; };   // op parameters (see cy_preproc.hip)
constexpr int MAX_STAGES = 8;
constexpr int MAX_PRE_BATCH = 256;
struct PreProgram { int n; PreStage st[MAX_STAGES]; };
struct PreArgs {
    const float* mosaic; int MH, MW;      // resident mosaic, native-endian fp32, non-finite already 0
    int txy[2 * 256];                      // tile origins x0,y0 in mosaic pixels, B <= 256 (kernel argument: no staging copy)
    int B, th, tw;                         // tile box of this shape class
    PreProgram prog[3]; int nprog;         // 1: one program broadcast to 3 channels; 3: per-channel programs
    double* params;                        // [B][3][MAX_STAGES][4] solved stage parameters (workspace / witness)
    double* histeq;                        // [B][3][520] bin centres [0:256] + cdf [256:512] for OP_HISTEQ (workspace)
    int* status;                           // [B] 0 ok, 1 preprocessing returned None, 2 constant-row check failed
    // network input
    void* out; int out_prec; int H, W, top, left;   // NHWC4 letterboxed canvas, fill 114/255
    double* scratch;                       // [B][3][th*tw] fp64 preprocessed image when a resize is needed, else null
    int new_h, new_w;                      // resized size (== th,tw when no resize)
    int* counters;                         // context counters or null: [2] += median-bracket hits, [3] += misses (cy_preproc.hip)
    int variant;                           // developer A/B switch of the statistics kernel (CY_PRE_VARIANT; 0 = shipped form)
    int fuse01;                            // set by the launch: programs 0 and 1 run in one workgroup (shared initial set)
};
hipError_t launch_preproc(const PreArgs& a, hipStream_t s);
hipError_t launch_preproc_planes(const PreArgs& a, hipStream_t s);    // statistics + checks + float64 planes into a.scratch (no packing)
hipError_t launch_letterbox_pack(const PreArgs& a, hipStream_t s);   // uses scratch/th/tw/new_*/H/W/top/left/out only
hipError_t launch_mosaic_prepare(float* data, size_t n, int big_endian, hipStream_t s);

// ---- test-time augmentation (ultralytics DetectionModel._predict_augment) ------------------------
// Views of a letterboxed batch: bilinear resize (torch upsample_bilinear2d, align_corners=False) of the (optionally left-right
// flipped) fp32 source to ch x cw, right / bottom padding with 0.447 up to Hp x Wp, NHWC4 in the context's input type.
struct AugView {
    void* out;                     // [B][Hp][Wp][4]
    int ch, cw, Hp, Wp;            // content size (int(H * s), int(W * s)), padded size (multiple of 32)
    int flip;                      // 1: x.flip(3) before the resize
};
struct AugPackArgs {
    const float* src; int B, H, W;  // fp32 NHWC4 letterboxed batch (the values view 0 is made of)
    AugView v[3]; int nview;        // one launch writes them all (blockIdx.z = view)
    int out_prec;                   // PREC_F16: fp16 stores (rounded once, from fp32); else fp32
};
hipError_t launch_augment_pack(const AugPackArgs& a, hipStream_t s);

// Decode of the three views' raw head outputs into ONE candidate list per tile (blockIdx.z = view): boxes de-scaled by the
// view's scale s, x centre de-flipped with the original width, anchors outside [lo, hi) dropped (_clip_augmented), candidate
// index = off + (anchor - lo) in the concatenated order.  Candidates feed nms_kernel unchanged.
struct AugDecodeView {
    const float* pred; int A; int lvl_h[3], lvl_w[3];
    float s; int flip; int lo, hi, off;
};
struct AugDecodeArgs {
    AugDecodeView v[3]; int nview;
    int B, nc; float conf; float W0;      // W0: width of view 0 (the de-flip reference)
    float* cand; int* cand_anchor; int* cand_count; int cap;
};
hipError_t launch_decode_augmented(const AugDecodeArgs& a, hipStream_t s);

// ---- catalog source measurement (cy_measure.hip) ---------------------------------------------------
constexpr int MEAS_FIELDS = 12;    // CY_MEAS_FIELDS
struct MeasureArgs {
    const float* img; int MH, MW;   // resident image as cy_mosaic_prepare leaves it (blank = 0); MH * MW < 2^31
    const int* win;                 // [n][8] inclusive pixel windows {bx0, bx1, by0, by1 | gx0, gx1, gy0, gy1}: box, box grown by the ring;
                                    // both inside the image, the grown one containing the box; bx1 < bx0 or by1 < by0 = empty
    int n;
    double* out;                    // [n][MEAS_FIELDS]
};
hipError_t launch_measure(const MeasureArgs& a, hipStream_t s);

// ---- source islands (cy_islands.hip) ---------------------------------------------------------------
constexpr int ISL_FIELDS = 20;                 // CY_ISL_FIELDS
// ISL_LDS_MAX, ISL_MAX_AREA, ISL_OFF_LDS, ISL_OFF_TOO_LARGE: cy_measure_jobs.h
struct IslandArgs {
    const float* img; int MH, MW;   // as MeasureArgs
    const int* win;                 // [n][4] inclusive box windows {bx0, bx1, by0, by1} inside the image; bx1 < bx0 or by1 < by0 = empty
    const double* thr;              // [n][3] {seed_thr, merge_thr, bkg}
    const long long* off;           // [n][2] {first label of the source in ws | ISL_OFF_LDS | ISL_OFF_TOO_LARGE, first mask byte in mask}
    int n, conn;                    // conn: 4 or 8
    unsigned* ws;                   // labels of the windows above ISL_LDS_MAX pixels, one u32 per pixel (null when there is none)
    unsigned char* mask;            // zeroed by the caller; null: no mask wanted
    double* out;                    // [n][ISL_FIELDS]
};
hipError_t launch_islands(const IslandArgs& a, hipStream_t s);

// ---- source components (cy_deblend.hip) ------------------------------------------------------------
constexpr int DBL_FIELDS = 8, DBL_COMP_FIELDS = 12;    // CY_DBL_FIELDS, CY_DBL_COMP_FIELDS; DBL_MAX_COMP: cy_measure_jobs.h
constexpr int DBL_RADIUS_MAX = 8;
struct DeblendArgs {
    const float* img; int MH, MW;   // as MeasureArgs
    const int* win;                 // [n][4] as IslandArgs
    const double* thr;              // [n][4] {seed_thr, merge_thr, bkg, peak_thr}
    const long long* off;           // [n][2] as IslandArgs
    int n, conn, radius;            // conn: 4 or 8; radius: 1 .. DBL_RADIUS_MAX
    unsigned* ws;                   // labels of the windows above ISL_LDS_MAX pixels, one u32 per pixel (null when there is none) ...
    unsigned* ws_up;                // ... and their `up` words, a second slice of the same size with the same offsets
    unsigned char* mask;            // zeroed by the caller; null: no mask wanted
    double* out;                    // [n][DBL_FIELDS]
    double* comp;                   // [n][DBL_MAX_COMP][DBL_COMP_FIELDS], zeroed by the caller
};
hipError_t launch_deblend(const DeblendArgs& a, hipStream_t s);

// ---- component fits (cy_fit.hip) -------------------------------------------------------------------
// FIT_FIELDS, FIT_MAX_AREA and struct FitJob: cy_measure_jobs.h
constexpr int FIT_NSUM = 28;                   // F, g (6), H upper triangle (21)
constexpr int FIT_LDS_MAX = 4096;              // largest job (list entries) whose values and indices live in LDS: 32 KiB per workgroup
constexpr int FIT_MIN_PIX = 7, FIT_MAX_ITER = 256;
struct FitArgs {
    const float* img; int MH, MW;   // as MeasureArgs
    const FitJob* jobs; int njobs;
    const unsigned* list; long long nlist;      // window indices dy * W + dx, increasing inside a job
    int max_iter;                   // 1 .. FIT_MAX_ITER
    double* out; int nrows;         // [nrows][FIT_FIELDS], zeroed by the caller; the kernel writes the jobs' rows
};
hipError_t launch_fit(const FitArgs& a, hipStream_t s);

// ---- joint fits of blends (cy_blend.hip) -----------------------------------------------------------
// BLEND_FIELDS, BLEND_MAX_MEMBERS and struct BlendJob: cy_measure_jobs.h
constexpr int BLEND_CHUNK = 128;               // list entries whose residual and Jacobian rows are in LDS at a time
constexpr int BLEND_NSUM_MAX = 325;            // F, g (24), H upper triangle (300) at four members
struct BlendArgs {
    const float* img; int MH, MW;   // as MeasureArgs
    const BlendJob* jobs; int njobs;
    const unsigned* list; long long nlist;      // window indices dy * W + dx, increasing inside a job
    int max_iter;                   // 1 .. FIT_MAX_ITER
    double* out; int nrows;         // [nrows][BLEND_FIELDS], zeroed by the caller; the kernel writes the rows of the jobs' members
};
hipError_t launch_blend(const BlendArgs& a, hipStream_t s);

// ---- model and residual maps (cy_residual.hip) -----------------------------------------------------
// RND_FIELDS, RND_HALF_MAX, RND_TILE, RES_FIELDS: cy_measure_jobs.h
constexpr int RND_CHUNK = 64;                  // components of a tile that are in LDS at a time: 4 KiB per workgroup
struct RenderArgs {
    const float* img; int MH, MW;   // as MeasureArgs
    const double* comp;             // [m][6] {A, x0, y0, a, b, c}, x0 / y0 in image pixels
    const int* rect;                // [m][4] inclusive support rectangles {sx0, sx1, sy0, sy1} inside the image (read for listed components only)
    const int* tile_off;            // [ntx * nty + 1] first list entry of every RND_TILE x RND_TILE tile, tiles row-major
    const int* tile_list;           // per tile the rendered components whose rectangle meets it, in increasing index
    int ntx, nty;                   // ceil(MW / RND_TILE), ceil(MH / RND_TILE)
    const float* bkg;               // [MH][MW] or null (0)
    float *model, *resid;           // [MH][MW] each; either may be null, not both
};
hipError_t launch_render(const RenderArgs& a, hipStream_t s);
struct ResidualArgs {
    const float* img; const float* model; int MH, MW;   // image as MeasureArgs, model map of the same shape
    const int* win;                 // [n][4] as IslandArgs
    const long long* off;           // [n][2] {ISL_OFF_TOO_LARGE for a window above ISL_MAX_AREA, first mask byte in mask}
    const double* bkg;              // [n]
    const unsigned char* mask;      // the windows' bytes, non-zero: in the island set
    int n;
    double* out;                    // [n][RES_FIELDS]
};
hipError_t launch_residual_stats(const ResidualArgs& a, hipStream_t s);

// ---- residual peaks (cy_peaks.hip) -----------------------------------------------------------------
// PEAK_FIELDS, PEAK_RADIUS_MAX, PEAK_SEG, PEAK_SEG_WORDS, PEAK_MAX_SEG: cy_measure_jobs.h
struct PeakArgs {
    const float* map; const float* rms; int MH, MW;   // two maps of one shape; MH * MW < 2^31
    double k_sigma; int radius, sign;                 // k_sigma > 0; radius 1 .. PEAK_RADIUS_MAX; sign +1 or -1
    int nsx, nseg;                  // segments of a row (ceil(MW / PEAK_SEG)) and of the image (MH * nsx <= PEAK_MAX_SEG); nsx * PEAK_SEG + radius fits int
    unsigned* count;                // [nseg] peaks of every segment (count pass)
    unsigned* offset;               // [nseg] peaks of the segments before it (scan pass)
    unsigned long long* bits;       // [nseg][PEAK_SEG_WORDS] peak bitmap (count pass): word 4 w + j, bit l = pixel 4 (64 w + l) + j of the segment
    long long* total;               // [1] peaks of the image (scan pass)
    double* rows; int cap;          // [cap][PEAK_FIELDS]; cap == 0: the fill pass is not launched
};
hipError_t launch_peaks(const PeakArgs& a, hipStream_t s);     // the three passes, queued in order

// ---- a trous wavelet level (cy_atrous.hip) -----------------------------------------------------------
// ATR_STEP_MAX, ATR_COLS, ATR_CHUNK, ATR_GRID_MAX: cy_measure_jobs.h; the geometry: plan_atrous (cy_measure_plan.h)
struct AtrousArgs {
    const float* in; int MH, MW, step;                // MH * MW < 2^31; 1 <= step <= ATR_STEP_MAX
    float* smooth; float* detail;                     // [MH][MW] each, one of them may be null; neither overlaps `in` or the other
    int ncb, nres, nchunk, items, grid;               // as AtrousPlan
};
hipError_t launch_atrous(const AtrousArgs& a, hipStream_t s);

// ---- aperture sums at given positions (cy_aperture.hip) ----------------------------------------------
// APER_*, AperJob: cy_measure_jobs.h; the jobs: plan_apertures (cy_measure_plan.h)
struct ApertureArgs {
    const float* map; const float* rms; int MH, MW;   // rms may be null; MH * MW < 2^31
    const AperJob* jobs; int n, K;                    // 1 <= n <= APER_JOBS_MAX, 1 <= K <= APER_RINGS_MAX
    double* out;                                      // [n][APER_FIELDS]; the kernel writes every field of every row
};
hipError_t launch_apertures(const ApertureArgs& a, hipStream_t s);

// ---- Gaussian fits at given positions (cy_peakfit.hip) ------------------------------------------------
// PFIT_*, PeakFitJob: cy_measure_jobs.h; the jobs: plan_peak_fits (cy_measure_plan.h)
constexpr int PFIT_LDS_MAX = 8192;             // largest window (pixels) whose member values live in LDS: 32 KiB per workgroup (R <= 44)
struct PeakFitArgs {
    const float* map; int MH, MW;   // MH * MW < 2^31
    const PeakFitJob* jobs; int n;  // the whole job table: a neighbour is named by its index in it
    const int* run; int nrun;       // the jobs that are fitted, one workgroup each: 1 <= nrun <= n <= PFIT_JOBS_MAX
    int max_iter;                   // 1 .. FIT_MAX_ITER
    double* out;                    // [nrun][PFIT_FIELDS]: workgroup t writes every field of row t
};
hipError_t launch_peak_fits(const PeakFitArgs& a, hipStream_t s);

// ---- joint fits of groups of peaks (cy_peakgroup.hip) --------------------------------------------------
// PGRP_FIELDS, PeakGroupJob: cy_measure_jobs.h; the groups: plan_peak_groups (cy_measure_plan.h)
constexpr int PGRP_LDS_MAX = 8192;             // largest group window (pixels) whose member values live in LDS: 32 KiB per workgroup
struct PeakGroupArgs {
    const float* map; int MH, MW;   // MH * MW < 2^31
    const PeakFitJob* jobs; int n;  // the whole job table: members and outside neighbours are named by their indices in it
    const PeakGroupJob* groups; int ngroups;       // one workgroup each: 1 <= ngroups <= n / 2
    int max_iter;                   // 1 .. FIT_MAX_ITER
    double* out;                    // [ngroups][BLEND_MAX_MEMBERS][PGRP_FIELDS]: workgroup t writes the rows of its M members
                                    // (fields 0 .. 35 and nexcluded; the others are the host's), zeroed by the caller
};
hipError_t launch_peak_groups(const PeakGroupArgs& a, hipStream_t s);

// ---- residuals on the discs of given jobs (cy_disc_residual.hip) -----------------------------------------
// DRES_FIELDS, PeakFitJob: cy_measure_jobs.h; the jobs: plan_peak_fits (cy_measure_plan.h)
struct DiscResidualArgs {
    const float* map; const float* model; int MH, MW;      // model may be null; MH * MW < 2^31
    const PeakFitJob* jobs; int n;  // the whole job table: a neighbour is named by its index in it
    const int* run; int nrun;       // the jobs that are measured, one workgroup each: 1 <= nrun <= n <= PFIT_JOBS_MAX
    double* out;                    // [nrun][DRES_FIELDS]: workgroup t writes every field of row t
};
hipError_t launch_disc_residuals(const DiscResidualArgs& a, hipStream_t s);

// ---- forced photometry: linear fits of fixed shapes (cy_forced.hip) ---------------------------------------
// FORCED_*, ForcedJob: cy_measure_jobs.h; the jobs: plan_forced (cy_measure_plan.h)
struct ForcedArgs {
    const float* map; const float* rms; int MH, MW;        // rms may be null; MH * MW < 2^31
    const ForcedJob* jobs; int n;   // the whole job table: a neighbour is named by its index in it
    const int* run; int nrun;       // the jobs that are fitted, one workgroup each: 1 <= nrun <= n <= FORCED_JOBS_MAX
    double ns2; int fit_bkg;        // nsigma * nsigma, rounded once on the host; 0 or 1
    double* out;                    // [nrun][FORCED_FIELDS]: workgroup t writes every field of row t
};
hipError_t launch_forced(const ForcedArgs& a, hipStream_t s);

// ---- background and noise mesh (cy_background.hip) -------------------------------------------------
constexpr int BKG_FIELDS = 8;                 // CY_BKG_FIELDS
constexpr int BKG_CELL_MIN = 4, BKG_CELL_MAX = 4096, BKG_NITER_MAX = 32;
constexpr int BKG_LDS_MAX = 128 * 128;         // largest cell (pixels) that is copied into LDS: 64 KiB per workgroup
struct BackgroundArgs {
    const float* img; int MH, MW;   // as MeasureArgs
    int cell, ncy, ncx;             // ncx = ceil(MW / cell), ncy = ceil(MH / cell)
    double k; int niter;            // clip width (> 0) and number of clips (0 .. BKG_NITER_MAX)
    double* out;                    // [ncy][ncx][BKG_FIELDS]
};
hipError_t launch_background(const BackgroundArgs& a, hipStream_t s);
struct BackgroundExpandArgs {
    const double* mesh;             // [ncy][ncx][2] {bkg, rms}, filled
    int ncy, ncx, cell, MH, MW;
    float *bkg, *rms;               // [MH][MW] each; either may be null
};
hipError_t launch_background_expand(const BackgroundExpandArgs& a, hipStream_t s);

}  // namespace cy
