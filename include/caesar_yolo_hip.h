/* caesar_yolo_hip.h -- C-ABI of the MI355X-native tiled-YOLO detect path (libcaesar_yolo_hip.so, gfx950).
 *
 * Drop-in boundary for the one hot path of SKA-INAF/caesar-yolo: everything `Analyzer.predict` does between
 * receiving a tile and handing back merged boxes.  Citations are reference files (relative to the reference
 * checkout) whose behaviour each entry point replaces.
 *
 * Conventions
 *   - every function returns 0 on success or a negative cy_status; nothing throws across the boundary
 *     (the reference catches any exception from the model call and skips the tile: caesar_yolo/evaluation.py:194-196,
 *     caesar_yolo/inference.py:615-618); `cy_last_error` gives the text;
 *   - `d_*` pointers are DEVICE pointers owned by the caller (e.g. torch tensors' data_ptr()), `h_*` are host
 *     pointers; `stream` is a hipStream_t passed as void* (NULL = default stream); all launches are asynchronous;
 *   - one context per GPU; a context is not thread-safe; no allocation happens after cy_load_weights.
 */
#ifndef CAESAR_YOLO_HIP_H
#define CAESAR_YOLO_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct cy_ctx cy_ctx;

enum cy_status { CY_OK = 0, CY_ERR_ARG = -1, CY_ERR_HIP = -2, CY_ERR_IO = -3, CY_ERR_STATE = -4, CY_ERR_UNSUPPORTED = -5 };
/* CY_F16: fp16 operands, fp32 accumulate (fast); CY_F32: exact fp32 FMA chains on v_mfma_f32_16x16x4_f32 (reference arithmetic,
 * slow); CY_F16X3: the fast parity context -- activations and weights carried as fp16 high + low halves (22 significand bits),
 * every product evaluated as hi*hi + lo*hi + hi*lo on the fp16 matrix cores with fp32 accumulation (3x the K of CY_F16).
 * Range: in CY_F16 and CY_F16X3 an activation is stored through an fp16 high half, so |activation| must stay below 65504 (beyond
 * that the value becomes inf; only CY_F32 has the fp32 range).  Weights have no such limit (scaled per output channel).
 * Buffers the caller hands to cy_forward / cy_preproc / cy_letterbox_pack / cy_conv_bn_silu and the other kernel-level test
 * entries are fp32 in the CY_F32 and CY_F16X3 contexts and fp16 in CY_F16. */
enum cy_precision { CY_F16 = 0, CY_F32 = 1, CY_F16X3 = 2 };

#define CY_MAX_DET 300        /* ultralytics max_det */
#define CY_DET_STRIDE 6       /* x1,y1,x2,y2,score,class */
#define CY_MAX_STAGES 8
#define CY_MAX_CAND 65535     /* candidates per tile and anchors per input: the 16-bit slot and anchor fields of the NMS sort key */

typedef struct cy_config {
    int precision;            /* cy_precision */
    int max_batch;            /* tiles per launch the workspace is sized for */
    int max_h, max_w;         /* largest letterboxed network input (multiple of 32) */
    int max_cand;             /* candidate capacity per tile before NMS (<= CY_MAX_CAND); 0 -> the anchor count of a
                                 max_h x max_w input (no overflow possible: NMS then keeps the top max_nms = 30000 by score,
                                 as ultralytics); a tile that overflows an explicit capacity is counted in cy_detect_counters.
                                 cy_create refuses max_h x max_w with more than CY_MAX_CAND anchors (from 1792 x 1792) */
} cy_config;

/* Preprocessing program: the CLI-fixed stage order of scripts/run.py:272-302, one op list per output channel.
 * ops follow caesar_yolo/preprocessing.py: BKG :591-658, SHIFT :664-717, CLIP :723-771, ZSCALE :934-971,
 * HISTEQ :977-1012, MINMAX :75-111.  Chan3Trasformer (:1020-1072) = three different programs. */
enum cy_pre_op { CY_OP_BKG = 1, CY_OP_SHIFT = 2, CY_OP_CLIP = 3, CY_OP_ZSCALE = 4, CY_OP_HISTEQ = 5, CY_OP_MINMAX = 6 };
typedef struct cy_pre_stage {
    int op;
    double p0, p1, p2;        /* BKG: sigma, mask_fract | SHIFT: sigma | CLIP: sigma_low, sigma_up | ZSCALE: contrast | MINMAX: norm_min, norm_max */
    int flag;                 /* BKG: use_mask_box */
} cy_pre_stage;
typedef struct cy_pre_program { int n; cy_pre_stage st[CY_MAX_STAGES]; } cy_pre_program;
typedef struct cy_preproc_cfg {
    int nprog;                /* 0: no preprocessing (raw pixel values go to the network, as without --preprocessing);
                                 1: one program, result replicated to 3 channels; 3: one program per channel */
    cy_pre_program prog[3];
} cy_preproc_cfg;

typedef struct cy_conv_desc { char name[48]; int cin, cout, k, s, act; } cy_conv_desc;

typedef struct cy_letterbox {  /* ultralytics LetterBox geometry for an (h0,w0) image at imgsz */
    int new_h, new_w, top, left, H, W;
} cy_letterbox;

/* ---- lifetime -------------------------------------------------------------------------------- */
/* replaces `model = YOLO(weights_path)` (scripts/run.py:347) + device selection (caesar_yolo/inference.py:205-217) */
int cy_create(int device, const cy_config* cfg, cy_ctx** out);
int cy_destroy(cy_ctx* ctx);
const char* cy_last_error(const cy_ctx* ctx);
int cy_load_weights(cy_ctx* ctx, const char* path);                 /* CYW1 file (caesar_yolo_amd/weights.py) */
int cy_load_weights_mem(cy_ctx* ctx, const void* buf, size_t nbytes);
int cy_num_classes(const cy_ctx* ctx);                               /* len(model.names), caesar_yolo/evaluation.py:46-47 */
const char* cy_class_name(const cy_ctx* ctx, int i);
/* fp16x3 context: how many convolutions run the two-pass form (filter = fp16 values x a per-channel scale, exactly: what a
 * checkpoint stored in fp16 and folded with its BatchNorm in fp32 is -- ultralytics' own load path) and how
 * many the general three-pass form.  out2[0] = two-pass layers, out2[1] = three-pass layers (both 0 in the other contexts). */
int cy_weight_passes(const cy_ctx* ctx, int* out2);

/* ---- host-only helpers (no GPU needed) ------------------------------------------------------- */
int cy_plan_num_convs(char scale, int nc);
int cy_plan_conv_desc(char scale, int nc, int idx, cy_conv_desc* out);
int cy_letterbox_geometry(int h0, int w0, int imgsz, cy_letterbox* out);
int cy_num_anchors(int H, int W);
size_t cy_pred_elems(const cy_ctx* ctx, int B, int H, int W);        /* floats in the raw head output [B][A][64+nc] */

/* ---- stages ---------------------------------------------------------------------------------- */
/* utils.read_fits / read_fits_crop value semantics (caesar_yolo/utils.py:219, :394): big-endian FITS floats ->
 * native, non-finite -> 0, in place on the HBM-resident mosaic */
int cy_mosaic_prepare(cy_ctx* ctx, float* d_data, size_t n, int big_endian, void* stream);

/* Analyzer.predict steps evaluation.py:146-176 for B tiles of one shape (th x tw) cropped from the resident mosaic:
 * 3-channel cube, DataPreprocessor pipeline, None / constant-row rejection, then the model's own LetterBox + BGR
 * flip + /255.  h_tiles: B x {x0, y0} tile origins in mosaic pixels.
 * d_netin: [B][H][W][4] (fp16 or fp32 per context precision); d_status[B]: 0 ok, 1 pipeline returned None, 2 row check */
int cy_preproc(cy_ctx* ctx, const float* d_mosaic, int MH, int MW, const int* h_tiles, int B, int th, int tw,
               int imgsz, const cy_preproc_cfg* cfg, void* d_netin, int* d_status, void* stream);
/* the same statistics and rejection checks, but the output is the preprocessed image itself, d_planes [B][3][th*tw] float64
 * in image channel order = what `DataPreprocessor.__call__` hands back to Analyzer.predict (caesar_yolo/evaluation.py:157-161,
 * before the model's LetterBox): full-precision parity witness, and the picture Analyzer.draw_results plots (:351-411) */
int cy_preproc_planes(cy_ctx* ctx, const float* d_mosaic, int MH, int MW, const int* h_tiles, int B, int th, int tw,
                      const cy_preproc_cfg* cfg, double* d_planes, int* d_status, void* stream);
/* witness for parity tests: solved per-stage parameters of the last cy_preproc call, [B][3][CY_MAX_STAGES][4] doubles */
int cy_preproc_params(cy_ctx* ctx, double* h_out, int B);

/* the model's own input handling for caller-supplied images (the `model(ndarray)` surface, evaluation.py:181-193):
 * d_planes [B][3][h0][w0] float64 (image channel order, nominal range [0,255]) -> LetterBox + flip + /255 -> d_netin */
int cy_letterbox_pack(cy_ctx* ctx, const double* d_planes, int B, int h0, int w0, int imgsz, void* d_netin, void* stream);

/* DetectionModel.forward: d_netin [B][H][W][4] -> d_pred [B][A][64+nc] fp32 raw head output */
int cy_forward(cy_ctx* ctx, const void* d_netin, int B, int H, int W, float* d_pred, void* stream);
/* per-launch timing of the forward kernels with hipEvents on the caller's stream (bench.py roofline): enable, run
 * cy_forward / cy_detect_tiles as usual, then read the totals per kernel variant (up to 8 entries: the conv variants,
 * stem, pool); flops are the ALGORITHMIC 2*MACs of the launches timed */
typedef struct cy_prof_entry { char kernel[64]; double ms; double flops; long launches; } cy_prof_entry;
int cy_profile_enable(cy_ctx* ctx, int on);    /* 0 off, 1 every cy_forward call, N > 1 every N-th call (sampling) */
int cy_profile_summary(cy_ctx* ctx, cy_prof_entry* out, int cap);
/* the same for the launches of one lane of cy_detect_tiles only: 0 = the caller's stream (full batches, incl. the second stream of
 * a split batch), 1 = the small-batch lane, -1 = all */
int cy_profile_summary_lane(cy_ctx* ctx, cy_prof_entry* out, int cap, int lane);
int cy_profile_layers(cy_ctx* ctx, cy_prof_entry* out, int cap);    /* the same, one entry per convolution (graph order) */
/* name of the kernel variant that the last timed launch of one named convolution ran (profiling enabled); an empty string when the
 * convolution had no launch of its own (it ran inside the kernel of a neighbouring layer, or no forward was timed) */
int cy_profile_layer_variant(cy_ctx* ctx, const char* conv_name, char* out, int cap);
/* copy the output of one named convolution of the last cy_forward to host as fp32 [B][C][Ho][Wo] (test hook) */
int cy_debug_read_conv(cy_ctx* ctx, const char* conv_name, float* h_out, size_t cap_elems, int* dims4);
/* test hooks for an op-by-op check of the forward pass (never set on the hot path).  cy_debug_stop_after: the following cy_forward
 * calls end after the first n_ops ops of the plan (n_ops <= 0: the whole plan, the default).  A launch that runs two plan ops (stem +
 * model.1, a back-to-back 1x1 pair, a fused bottleneck) whose first op lies below n_ops runs whole; a box-branch output convolution
 * that waits for its class branch (the head pair) is not launched by a pass that stops before the class branch, so its rows of
 * d_pred keep what the caller put there.  A stopped pass first fills the workspace with 0xFF bytes (NaN in fp16 and fp32), so what
 * it leaves unwritten reads as NaN, and never runs as two half-batches.  cy_debug_ops_done: the number of plan
 * ops the last cy_forward completed (n_ops + 1 after such a two-op launch), or a negative error code.
 * cy_debug_read_tensor: channels [coff, coff + C) of plan tensor `tensor` as the last cy_forward left them, as fp32 [B][C][h][w]
 * (fp16x3 context: high + low half); tensor 0, the caller's input, is refused. */
int cy_debug_stop_after(cy_ctx* ctx, int n_ops);
/* test hook for the deferred box branch of the plain detect path (fp16 context): cy_forward's pass with the box branch of every
 * supported level computed ONLY at the anchors whose best class score passes `conf` (as CY_SPARSE_BOX=2 does inside
 * cy_detect_tiles).  Class columns of d_pred are written at every anchor; box columns (0..63) of a deferred level at candidates
 * only, the rest keep what the caller put there.  h_sparse3[l] = 1 when level l was deferred, 0 when its shape kept the dense
 * branch (then all of its box columns are written).  Other contexts: all levels dense. */
int cy_debug_sparse_box(cy_ctx* ctx, const void* d_netin, int B, int H, int W, float* d_pred, float conf, int* h_sparse3, void* stream);
int cy_debug_ops_done(cy_ctx* ctx);
int cy_debug_read_tensor(cy_ctx* ctx, int tensor, int coff, int C, float* h_out, size_t cap_elems, int* dims4);

/* Detect decode + non_max_suppression + scale_boxes:
 * d_det [B][300][6], d_det_anchor [B][300] (anchor index of each kept box), d_count [B] */
int cy_decode_nms(cy_ctx* ctx, const float* d_pred, int B, int H, int W, int h0, int w0, float conf, float iou,
                  float* d_det, int* d_det_anchor, int* d_count, void* stream);

/* developer diagnostics: in-kernel cycle stamps of the 3x3 halo kernel (enabled with CY_DBG=64) */
int cy_debug_stamps(unsigned long long* out8, int reset);
/* developer diagnostics: the pack kernel's quotient by a per-tile constant (d_fast) beside the float64 division (d_ref), element-wise on
 * device arrays of n doubles: must agree bit for bit (tests/test_gpu_preproc.py) */
int cy_debug_fastdiv(const double* d_a, const double* d_b, double* d_fast, double* d_ref, int n);
/* developer diagnostics: the block reduction of the measurement kernels (csrc/cy_reduce.h) on its own.  d_val (float64) and d_key
 * (float32) hold nrows rows of len entries, len >= 0; one workgroup of 256 threads per row, thread t on entries t, t + 256, ..  d_out
 * [nrows][2][8] 64-bit words, per finishing style (0: thread 0, 1: every thread, as the last thread sees it): bits of the float64 sum
 * of d_val, entry count, first maximum of the valid keys (non-zero and finite): float bits and index (none: -inf, 0xFFFFFFFF),
 * smallest and largest index of a valid key (none: INT_MAX, -1, sign-extended), the first maximum's index again as a 64-bit
 * reduction (none: LLONG_MAX) and the smallest valid index as an unsigned one (none: all ones).  Launched on the null stream, not
 * waited for.  tests/test_gpu_reduce.py compares every word with tests/reduce_ref.py */
int cy_debug_reduce(const double* d_val, const float* d_key, int nrows, int len, unsigned long long* d_out);
/* test hook (never called on the hot path): sets what the kernels queued behind it on `stream` inherit in LDS.  One kernel, one
 * workgroup per CU, each with the largest dynamic LDS the device grants a workgroup (queried, not assumed), writes pattern32 over
 * all of it with plain vector LDS stores.  Returns that size in bytes (> 0), or a negative error code; it does not wait for the
 * kernel.  That LDS keeps its bytes across a kernel boundary is observed behaviour of this GPU and no contract: a test may use the
 * hook to make a read of LDS the workgroup did not write visible, never to pass data.  Which CU a workgroup lands on is the
 * dispatcher's choice; a CU busy with another stream's work may be missed. */
int cy_debug_lds_fill(cy_ctx* ctx, unsigned pattern32, void* stream);
/* number of pre-NMS candidates per tile of the last cy_decode_nms call (diagnostics) */
int cy_debug_cand_counts(cy_ctx* ctx, int* h_out, int B);

/* Analyzer.process_detections (caesar_yolo/evaluation.py:252-346): score re-filter, IoU graph, connected components,
 * best score per component.  d_out [B][300][6], d_out_count [B], d_out_src [B][300] = row of d_det kept */
int cy_iou_merge(cy_ctx* ctx, const float* d_det, const int* d_count, int B, float score_thr, double thr_soft,
                 double thr_hard, float* d_out, int* d_out_count, int* d_out_src, void* stream);

/* the whole per-tile path for B same-shape tiles; status/det/count as above (merged detections in tile pixels).
 * Consecutive calls are software-pipelined on internal side streams (preprocessing / post-processing of neighbouring
 * batches overlap the forward pass): give every in-flight call its own output buffers and call cy_detect_flush before
 * reading them -- after it, work queued on `stream` is ordered behind all outstanding batches */
int cy_detect_tiles(cy_ctx* ctx, const float* d_mosaic, int MH, int MW, const int* h_tiles, int B, int th, int tw,
                    int imgsz, const cy_preproc_cfg* cfg, float conf, float iou, double thr_soft, double thr_hard,
                    float* d_out, int* d_out_count, int* d_status, void* stream);

int cy_detect_flush(cy_ctx* ctx, void* stream);
/* Ordering contract of unflushed cy_detect_tiles calls.  The internal streams are ordered behind `stream` (everything the caller
 * queued on it so far) at: the first call after cy_load_weights / cy_detect_flush; the first call after cy_mosaic_prepare; the
 * first call that names a d_mosaic buffer this pipeline has not seen yet; the first call after cy_detect_fence.  Any OTHER work
 * the caller queues on `stream` between two unflushed calls -- a re-upload into a mosaic buffer already used, a memset of an
 * output buffer -- is NOT ordered before the internal streams touch those buffers: call cy_detect_fence after queuing it (the
 * next cy_detect_tiles then waits for it; costs the overlap of that one batch's preprocessing with the previous forward), or
 * prepare every buffer before the first call (what caesar_yolo_amd.inference.TileEngine does).
 * "A buffer this pipeline has seen" is its ADDRESS: a caching allocator (PyTorch's) may hand a NEW mosaic tensor the address of one
 * freed inside the same unflushed pipeline, and that buffer then counts as seen although its upload is still queued on `stream`.
 * A caller that allocates mosaic buffers between unflushed calls must call cy_detect_fence after every upload (uploads through
 * cy_mosaic_prepare are fenced by the library itself). */
int cy_detect_fence(cy_ctx* ctx, void* stream);

/* Rank 0 after the gather (replaces the unpickling of the workers' source lists, caesar_yolo/inference.py:936-984): d_gathered holds
 * the ranks' fixed-capacity tile records, n_rows rows of row_floats = 300*6 + 3 floats {detections | count | status | tile id};
 * d_perm[t] = row index (over all ranks) of tile t (an index outside [0, n_rows) makes tile t a rejected tile with status CY_ERR_ARG).  Writes d_hdr = {count[T] (0 for a rejected tile) | status[T] | exclusive prefix[T] | total}
 * (3 T + 1 ints) and the valid detections in tile-id order into d_out (room for T * 300 * 6 floats): what cy_make_tile_records takes. */
int cy_compact_records(const float* d_gathered, long long n_rows, const long long* d_perm, int T, int row_floats, int* d_hdr, float* d_out, void* stream);
/* the same with the context named: launches on the context's device whatever device is current (the form above launches on the
 * CURRENT device: the caller must have selected the device that owns the buffers) */
int cy_compact_records_ctx(cy_ctx* ctx, const float* d_gathered, long long n_rows, const long long* d_perm, int T, int row_floats, int* d_hdr, float* d_out, void* stream);

/* events the reference would not survive silently, accumulated over cy_decode_nms / cy_iou_merge / cy_detect_tiles calls:
 * out4[0] degenerate boxes (x1 >= x2 or y1 >= y2) dropped before the IoU merge -- the reference aborts on them inside
 * get_iou's assert (caesar_yolo/utils.py:78-81); out4[1] tiles with more candidates than the
 * context's explicit max_cand (the default capacity, the anchor count, cannot overflow; NMS keeps the top max_nms = 30000
 * by score as ultralytics does, but the surplus over max_cand is dropped in arrival order, so a non-zero count means "raise
 * max_cand"); out4[2], out4[3]: performance diagnostics of the sigma-clip statistics (median
 * selections served by the one-pass bracket / fallen back to the three-pass radix select).  Synchronises the device.
 * reset != 0 clears them. */
int cy_detect_counters(cy_ctx* ctx, long long* out4, int reset);

/* single fused Conv+bias+SiLU layer on caller tensors (kernel-level parity tests).
 * d_in [B][Hi][Wi][Cin], d_out [B][Ho][Wo][Cout] in the context precision; h_w [Cout][Cin][k][k], h_b [Cout] fp32;
 * d_res optional residual [B][Ho][Wo][Cout] */
int cy_conv_bn_silu(cy_ctx* ctx, const void* d_in, int B, int Hi, int Wi, int Cin, const float* h_w, const float* h_b,
                    int Cout, int k, int s, int act, const void* d_res, void* d_out, void* stream);

/* the same layer in the layout the forward pass gives a convolution (kernel-level tests): channel slices of wider NHWC buffers.
 * d_in0 [B][H0][W0][in0_ct], the c0 channels from in0_coff on; up0 != 0: read through the nearest x2 upsample, H0 = Hi / 2,
 *   W0 = Wi / 2 (else H0 = Hi, W0 = Wi).  d_in1 [B][Hi][Wi][in1_ct] (c1 channels from in1_coff on; c1 == 0: absent): the input is
 *   the channel concatenation of the two segments.  d_res optional [B][Ho][Wo][res_ct], the Cout channels from res_coff on; it may
 *   be d_out itself with a disjoint slice (the C2f bottleneck pattern).  d_out [B][Ho][Wo][out_ct], the Cout channels from out_coff
 *   on; or, rows != 0, fp32 prediction rows [B][out_bs][out_ct] in every context, pixel (ho, wo) of image b in row
 *   b * out_bs + out_ro + ho * Wo + wo (no residual, no activation).  Buffers are exactly that large; what lies outside the output
 *   slice is left as it was.  Tensors are in the context precision (fp32 in CY_F16X3: every buffer is split whole into high / low
 *   halves, the output buffer too, and merged back).
 * Refused with CY_ERR_ARG before anything is launched: a slice outside its ct; a ct, offset, c0 or c1 that is no multiple of 8
 *   (a dense output / residual, ct == Cout at offset 0, may have any width; the ct of prediction rows is free); c0 + c1 != Cin;
 *   c1 != 0 unless k == 1, s == 1 and c0 is a multiple of the K chunk (64 channels, 32 in CY_F32); up0 unless k == 1, s == 1 and
 *   Hi, Wi even; rows with out_ro + Ho * Wo > out_bs, a residual or an activation; d_out equal to an input.
 * variant (variant_cap bytes, may be null): the name of the kernel variant that ran; passes (may be null): passes over K of the
 *   CY_F16X3 filter (2 or 3), 0 in the other contexts.  cy_conv_bn_silu is the dense call of this entry.
 * cy_conv_variant_name: name of variant idx (host only), NULL past the last one. */
typedef struct cy_conv_layout {
    const void* d_in0; int in0_ct, in0_coff, c0, up0;
    const void* d_in1; int in1_ct, in1_coff, c1;
    const void* d_res; int res_ct, res_coff;
    void* d_out; int out_ct, out_coff;
    int rows, out_bs, out_ro;
    int B, Hi, Wi, Cin, Cout, k, s, act;
} cy_conv_layout;
int cy_conv_slices(cy_ctx* ctx, const cy_conv_layout* layout, const float* h_w, const float* h_b, char* variant,
                   int variant_cap, int* passes, void* stream);
const char* cy_conv_variant_name(int idx);

/* one fused Bottleneck(64, 64, shortcut) = x [+] SiLU(cv2(SiLU(cv1(x)))) with two folded 3x3 convs, as the forward runs the
 * stride-4 C2f blocks of yolov8l in the fp16 context (kernel-level parity tests).  d_in, d_out [B][H][W][64] fp16;
 * h_w1, h_w2 [64][64][3][3], h_b1, h_b2 [64] fp32 */
int cy_bottleneck64(cy_ctx* ctx, const void* d_in, int B, int H, int W, const float* h_w1, const float* h_b1,
                    const float* h_w2, const float* h_b2, int shortcut, void* d_out, void* stream);

/* kernel-level test entries of the YOLO11 / SPPF operators: one launch of the kernel the forward runs for that op, on channel slices
 * of caller NHWC tensors [pix][ct] in the context precision (fp32 in CY_F16X3: split into high / low halves, run, merged back, as
 * the forward stores them).  Synchronous on `stream`.
 * cy_dwconv3x3: out[., c] = act(sum_{3x3} in[., map(c)] * w + b[c]) (+ res[., c]), zero padding, stride 1; h_w [C][1][3][3],
 *   h_b [C] fp32; map(c) = c (blk = 0) or (c / blk) * gstride + goff + c % blk (the C2PSA positional-encoding conv reading v
 *   out of qkv).  C, every ct / coff and blk / gstride / goff are multiples of 8; d_res may be null.
 * cy_attention: per head h, out[b][n][out_coff + h*hd + c] = sum_m softmax_m(q_n . k_m * kd^-0.5) v_m[c] over the per-head
 *   [q kd | k kd | v hd] channel blocks of d_qkv [B][N][ct] starting at coff; kd <= 64.  N above 10240 (the per-query kernel's
 *   LDS) -> CY_ERR_UNSUPPORTED, nothing launched.
 * cy_maxpool5: MaxPool2d(5, 1, 2) with -inf padding, slice src_coff -> slice dst_coff of [B][H][W][ct] tensors; d_src and d_dst
 *   may be the same buffer (SPPF) with disjoint slices.  C, ct and the offsets are multiples of 8. */
int cy_dwconv3x3(cy_ctx* ctx, const void* d_in, int B, int H, int W, int C, int in_ct, int in_coff, const float* h_w,
                 const float* h_b, int act, int blk, int gstride, int goff, const void* d_res, int res_ct, int res_coff,
                 void* d_out, int out_ct, int out_coff, void* stream);
int cy_attention(cy_ctx* ctx, const void* d_qkv, int B, int N, int ct, int coff, int heads, int kd, int hd, void* d_out,
                 int out_ct, int out_coff, void* stream);
int cy_maxpool5(cy_ctx* ctx, const void* d_src, int B, int H, int W, int C, int ct, int src_coff, void* d_dst, int dst_coff,
                void* stream);

/* ---- test-time augmentation (ultralytics `model(img, augment=True)`, DetectionModel._predict_augment) ----------------------
 * Three views of the letterboxed batch: (scale 1, no flip), (0.83, left-right flip), (0.67, no flip); a scaled view is the
 * bilinear resize (align_corners=False) of the flipped / plain batch to (int(H s), int(W s)), padded right and bottom with 0.447
 * up to multiples of 32.  Each view's Detect output is divided by s, the flipped view's x centre mirrored with W, the stride-32
 * anchors of view 0 and the stride-8 anchors of view 2 dropped, and the three concatenated before the unchanged NMS and
 * scale_boxes.  Kept-box indices (d_det_anchor) are positions in that concatenation. */
typedef struct cy_augment_view {
    double scale; int flip;   /* 1, 0.83, 0.67; 1 = left-right flip */
    int ch, cw;               /* resized content (int(H * scale), int(W * scale)) */
    int Hp, Wp;               /* padded network input (ceil(H * scale / 32) * 32, ...) */
    int A;                    /* anchors of the view's head output */
    int lo, hi;               /* anchors kept: [lo, hi) */
    int off;                  /* position of anchor lo in the concatenation */
} cy_augment_view;
typedef struct cy_augment_geom { cy_augment_view v[3]; int total; } cy_augment_geom;
/* host-only: the views of an H x W letterboxed input (multiples of 32) */
int cy_augment_geometry(int H, int W, cy_augment_geom* out);
/* allocates, once, the per-buffer-set view inputs, view head outputs and the larger candidate buffers (capacity: the
 * concatenated anchor count of a max_h x max_w input, or max_cand when given).  Fails with CY_ERR_ARG when that anchor
 * count exceeds CY_MAX_CAND (from 1376 x 1376).  The calls below fail with CY_ERR_STATE on a context without it. */
int cy_enable_augment(cy_ctx* ctx);
/* cy_letterbox_pack into an fp32 canvas whatever the context precision (the source of the views in the fp16 context) */
int cy_letterbox_pack_f32(cy_ctx* ctx, const double* d_planes, int B, int h0, int w0, int imgsz, float* d_out, void* stream);
/* view kernel (kernel-level test entry): d_src fp32 [B][H][W][4] letterboxed -> d_view1 / d_view2 [B][Hp][Wp][4] in the context's
 * input type; d_view0 (fp16 context only, may be NULL) receives the fp16 copy of d_src.  One launch. */
int cy_augment_pack(cy_ctx* ctx, const float* d_src, int B, int H, int W, void* d_view0, void* d_view1, void* d_view2, void* stream);
/* the views' raw head outputs (as cy_forward writes them) -> decode + NMS over the concatenation + scale_boxes; H, W = view 0 */
int cy_decode_nms_augmented(cy_ctx* ctx, const float* d_pred0, const float* d_pred1, const float* d_pred2, int B, int H, int W,
                            int h0, int w0, float conf, float iou, float* d_det, int* d_det_anchor, int* d_count, void* stream);
/* cy_detect_tiles with augment != 0: the same per-tile path, pipelining and ordering contract, on the three views (their forwards
 * back to back on the forward stream); augment = 0 is cy_detect_tiles itself.  Plain and augmented calls may alternate in one
 * unflushed pipeline (cy_detect_flush covers both). */
int cy_detect_tiles_augmented(cy_ctx* ctx, const float* d_mosaic, int MH, int MW, const int* h_tiles, int B, int th, int tw,
                              int imgsz, const cy_preproc_cfg* cfg, float conf, float iou, double thr_soft, double thr_hard,
                              int augment, float* d_out, int* d_out_count, int* d_status, void* stream);

/* ---- catalog source measurement (an addition: the reference's catalog stops at boxes) ----------------------------------
 * Flux, peak, centroid moments and the local background of n catalog boxes on the resident image d_img [MH][MW] (fp32 as
 * cy_mosaic_prepare leaves it: blank pixels are 0; a pixel is VALID when it is != 0 and finite).  h_boxes: n x {x1, y1, x2, y2}
 * float64 in 0-based pixels of d_img (a pixel's centre at its index); they may lie partly or wholly outside the image.
 *   box window  ix in [max(0, ceil(x1)), min(MW - 1, floor(x2))], iy likewise with MH; it may be empty
 *   ring        the box window grown by `ring` pixels on each side, clipped to the image, minus the box window (an empty box
 *               window has no ring)
 * h_out row, CY_MEAS_FIELDS float64:
 *   [0] npix, [1] nring  valid pixels of the box window / of the ring
 *   [2] bkg   exact median of the ring's valid pixels (even count: (a + b) / 2), [3] rms = 1.4826 * exact median of |v - bkg|;
 *             both 0 when nring == 0
 *   [4] peak  largest valid pixel of the box window, [5] x_peak, [6] y_peak its first occurrence in row-major order
 *   [7] sum   of (v - bkg) over the valid pixels of the box window
 *   [8] sw, [9] swx, [10] swy   sums of w, w * ix, w * iy with w = v - bkg where that is > 0, else 0
 *   [11] reserved (0)
 *   npix == 0: peak = sum = sw = swx = swy = 0, x_peak = y_peak = -1.
 * Counts, medians and the peak do not depend on summation order; the sums are float64 with a fixed association (two calls give
 * the same bits).  One launch (one workgroup per box) and one copy to h_out; synchronous on `stream`.  n == 0: CY_OK, nothing
 * launched.  ring < 0, MH / MW <= 0, a null pointer, or an image of 2^31 pixels or more: CY_ERR_ARG.  Needs no loaded weights. */
#define CY_MEAS_FIELDS 12   /* npix nring bkg rms peak x_peak y_peak sum sw swx swy reserved */
int cy_measure_sources(cy_ctx* ctx, const float* d_img, int MH, int MW, const double* h_boxes, int n, int ring,
                       double* h_out /* [n][CY_MEAS_FIELDS] */, void* stream);
/* milliseconds the kernel of the last cy_measure_sources call took (hipEvents around the launch); -1 before the first call */
int cy_measure_kernel_ms(const cy_ctx* ctx, double* out_ms);

/* ---- source islands (an addition, the second measurement step) -------------------------------------------------------------
 * Seed / merge-threshold connected components of the box windows of n catalog boxes.  Image, validity of a pixel, pixel-centre
 * convention and box window are those of cy_measure_sources.  h_thr: n x {seed_thr, merge_thr, bkg} float64.
 *   candidate   valid pixel of the box window with (double)v >= merge_thr; seed: a candidate with (double)v >= seed_thr.  A NaN
 *               threshold leaves the source without candidates (or seeds)
 *   component   maximal set of candidates connected through `conn` = 8 or 4 neighbours inside the box window
 *   island set  union of the components that hold a seed; main island: the component of the window's peak pixel (largest valid
 *               pixel, first in row-major order), which is a seed whenever there is one
 * h_out row, CY_ISL_FIELDS float64, with dx = ix - wx0, dy = iy - wy0 (wx0, wy0: first column / row of the box window) and
 * w = (double)v - bkg:
 *   [0] status   0 measured; 1 the window has more than 2^24 pixels: nothing measured, every other field as for an empty window
 *   [1] nseed, [2] nislands, [3] npix (island set), [4] npix_main, [5] nborder (island-set pixels on the window's outer rows / columns)
 *   [6] xmin, [7] xmax, [8] ymin, [9] ymax   bounding box of the island set in image pixels; -1 when npix == 0
 *   [10] S = sum w, [11] Sx = sum w * dx, [12] Sy = sum w * dy, [13] Sxx = sum w * (dx * dx), [14] Syy = sum w * (dy * dy),
 *   [15] Sxy = sum w * (dx * dy), [16] S_main = sum w over the main island, [17..19] reserved (0)
 *   Empty window or no seed: counts and sums 0, bounding box -1, status 0.
 * h_mask (may be NULL): one byte per pixel of every box window, windows concatenated in source order, row-major inside a window:
 * 0 not in the island set, 1 in it, 2 in the main island.  h_mask_off: n + 1 offsets, [0] = 0 and [i + 1] - [i] = pixels of window
 * i; required with h_mask and checked against the windows.
 * Counts, bounding box and mask do not depend on any order; the sums are float64 with a fixed association (two calls give the same
 * bytes).  One launch (one workgroup per source, labels in LDS for windows of up to 4096 pixels, else in a workspace allocated
 * for the call) and the copies to h_out / h_mask; synchronous on `stream`.  n == 0: CY_OK, nothing launched.  conn not 4 or 8,
 * MH / MW <= 0, a null pointer, an image of 2^31 pixels or more, seed_thr < merge_thr, or h_mask_off that disagrees with the
 * windows: CY_ERR_ARG.  Needs no loaded weights. */
#define CY_ISL_FIELDS 20
int cy_measure_islands(cy_ctx* ctx, const float* d_img, int MH, int MW, const double* h_boxes, const double* h_thr /* n x {seed, merge, bkg} */,
                       int n, int conn, double* h_out /* [n][CY_ISL_FIELDS] */, unsigned char* h_mask /* may be NULL */,
                       const long long* h_mask_off /* n + 1 offsets, required with h_mask */, void* stream);
/* milliseconds the kernel of the last cy_measure_islands call took (hipEvents around the launch); -1 before the first call */
int cy_islands_kernel_ms(const cy_ctx* ctx, double* out_ms);

/* ---- source components (an addition, the fourth measurement step) -----------------------------------------------------------
 * The island set of every box split into components by local peaks and steepest-ascent basins.  Image, valid pixel, pixel-centre
 * convention, box window, candidate, seed, component of candidates (`conn` = 8 or 4), island set and main island are exactly those
 * of cy_measure_islands.  h_thr: n x {seed_thr, merge_thr, bkg, peak_thr} float64.  Inside one box window, pixel index
 * i = dy * W + dx:
 *   rank      pixel p outranks q when v(p) > v(q), or when v(p) == v(q) and i(p) < i(q): a total order on valid pixels
 *   up(p)     for an island-set pixel: the highest-ranked of p and its `conn` neighbours that are candidates inside the window
 *             (those neighbours are in p's component by construction)
 *   summit    a pixel with up(p) == p.  Following up from any island-set pixel reaches a summit (rank rises strictly on the way)
 *   basin     of a summit: the pixels that end at it
 *   peak      a summit s that outranks every island-set pixel of its own component with |dx| <= radius and |dy| <= radius
 *             (radius in [1, 8]) and either has (double)v(s) >= peak_thr or is the top-ranked pixel of its component: every island
 *             has at least one peak whatever peak_thr is, and a NaN peak_thr leaves exactly those
 *   order     peaks are ordered by rank over the whole window; npeaks is their number.  The first CY_DBL_MAX_COMP are KEPT and
 *             become components 0 .. ncomp - 1; the rest are demoted to ordinary summits and status becomes 2
 *   assign    the basin of a kept peak belongs to that peak's component.  The basin of any other summit s belongs to the kept peak
 *             t of the same island that minimises the integer squared distance (dx_s - dx_t)^2 + (dy_s - dy_t)^2, ties to the
 *             lower component index.  An island with no kept peak (only with status 2) leaves its pixels UNASSIGNED.  Basins are
 *             never split
 * h_out row, CY_DBL_FIELDS float64:
 *   [0] status   0 measured; 1 the window has more than 2^24 pixels: nothing measured; 2 measured, more than CY_DBL_MAX_COMP peaks
 *   [1] nsummits, [2] npeaks, [3] ncomp, [4] npix (island set: field [3] of cy_measure_islands for the same arguments),
 *   [5] npix_unassigned, [6..7] reserved (0).  Empty window or no seed: all 0.
 * h_comp row of component k (rows at and beyond ncomp are 0), CY_DBL_COMP_FIELDS float64, with dx, dy relative to the window's first
 * pixel and w = (double)v - bkg, the expressions and roundings of cy_measure_islands:
 *   [0] npix, [1] peak = v of the kept peak, [2] x_peak, [3] y_peak its position in image pixels
 *   [4] S, [5] Sx, [6] Sy, [7] Sxx, [8] Syy, [9] Sxy
 *   [10] main   1 when the component lies in the main island, [11] nsummits   basins merged into it
 * h_mask (may be NULL), h_mask_off: laid out as for cy_measure_islands; byte 0 not in the island set, k + 1 component k,
 * 255 unassigned.
 * Counts, peaks, positions and mask do not depend on any order; the sums are float64 with a fixed association (two calls give
 * the same bytes).  One launch (one workgroup per source; two u32 per pixel in LDS for windows of up to 4096 pixels, else in a
 * workspace allocated for the call) and one copy per output; synchronous on `stream`.  n == 0: CY_OK, nothing read or launched.
 * Argument errors as for cy_measure_islands, and radius outside [1, 8]: CY_ERR_ARG.  Needs no loaded weights. */
#define CY_DBL_MAX_COMP 16
#define CY_DBL_FIELDS 8        /* status nsummits npeaks ncomp npix npix_unassigned reserved reserved */
#define CY_DBL_COMP_FIELDS 12  /* npix peak x_peak y_peak S Sx Sy Sxx Syy Sxy main nsummits */
int cy_deblend_islands(cy_ctx* ctx, const float* d_img, int MH, int MW, const double* h_boxes,
                       const double* h_thr /* n x {seed, merge, bkg, peak} */, int n, int conn, int radius,
                       double* h_out /* [n][CY_DBL_FIELDS] */, double* h_comp /* [n][CY_DBL_MAX_COMP][CY_DBL_COMP_FIELDS] */,
                       unsigned char* h_mask /* may be NULL */, const long long* h_mask_off /* n + 1 offsets, required with h_mask */,
                       void* stream);
/* milliseconds the kernel of the last cy_deblend_islands call took (hipEvents around the launch); -1 before the first call */
int cy_deblend_kernel_ms(const cy_ctx* ctx, double* out_ms);

/* ---- component fits (an addition, the fifth measurement step) ---------------------------------------------------------------
 * One elliptical Gaussian fitted to every component of cy_deblend_islands, unweighted Levenberg-Marquardt in float64.  Image, valid
 * pixel, pixel-centre convention and box window are those of cy_measure_islands; h_mask / h_mask_off are laid out as
 * cy_deblend_islands writes them (both required here).  h_bkg: one background per source; h_ncomp: its number of components.
 *   job      one per (source, component k) with k < ncomp.  Its LIST is the window pixels whose mask byte is k + 1, in increasing
 *            window index i = dy * W + dx; its pixel set is the valid pixels of the list, npix their number.  A pixel that is not
 *            valid keeps its list position and contributes nothing.  Bytes 0, 255 and bytes above ncomp belong to no job
 *   data     y_i = (double)v_i - bkg at (dx, dy) relative to the window's first pixel
 *   model    m = A * exp(-0.5 * q), q = (a*u)*u + ((2*b)*u)*v + (c*v)*v, u = dx - x0, v = dy - y0; p = (A, x0, y0, a, b, c) with
 *            (a, b, c) the inverse covariance.  The fit runs on x0, y0 relative to the window (start - wx0, result + wx0)
 *   admissible   all six finite, A > 0, a > 0, c > 0, a * c - b * b > 0
 *   sweep    r = y - m; J = (e, m*(a*u + b*v), m*(b*u + c*v), ((-0.5*m)*u)*u, ((-m)*u)*v, ((-0.5*m)*v)*v) with e = exp(-0.5 * q);
 *            F = sum r*r, g_i = sum J_i*r, H_ij = sum J_i*J_j (i <= j): 28 float64 sums at one p, every product rounded on its own
 *   solve    Cholesky of M = H + lambda * diag(H) (M_jj = H_jj + lambda * H_jj), row by row, inner sums subtracted term by term in
 *            increasing index; L z = g, L^T d = z.  A pivot that is not positive and finite is a rejection without a trial
 *   iterate  lambda = 1e-3, sweep at the start; for it = 1 .. max_iter: solve; small = all |d_j| <= 1e-10 * (|p_j| + 1e-6); when
 *            p + d is admissible, sweep there (F'): F' < F accepts (lambda = max(lambda / 10, 1e-12)) and the job has converged when
 *            small holds or F - F' <= 1e-14 * F.  A rejected trial (not admissible, or not F' < F) with small true has converged at
 *            the old p.  Any other rejection: lambda *= 10, and lambda > 1e12 stops with status 2.  niter = the `it` of the stop
 * h_fit row of job (source, k), CY_FIT_FIELDS float64 (rows at and beyond ncomp are 0):
 *   [0] status   0 converged; 1 the window has more than 2^24 pixels: nothing done, every other field 0; 2 max_iter or the lambda
 *                limit reached, the last accepted p reported; 3 npix < 7: start reported as given, niter = 0; 4 start not admissible:
 *                reported as given, niter = 0 (4 is tested before 3).  With 3 and 4, F, lambda and H are 0
 *   [1] niter, [2] npix, [3] F, [4] lambda, [5..10] A x0 y0 a b c (x0, y0 in image pixels), [11..31] H upper triangle row-major,
 *   F and H at the reported p
 * The runtime builds the job table and the lists in one pass over the mask bytes and uploads them; one launch (one workgroup of 256
 * threads per job; a job of up to 4096 list entries keeps values and indices in LDS, a larger one re-reads them) and one copy back;
 * synchronous on `stream`.  The sums are float64 with a fixed association, entry q of the list on thread q mod 256 (two calls give
 * the same bytes).  n == 0, or no job at all: CY_OK, nothing launched.  A null pointer, MH / MW <= 0, an image of 2^31 pixels or
 * more, max_iter outside [1, 256], an h_ncomp entry outside [0, 16], h_mask_off that disagrees with the windows, or a mask byte
 * in 17 .. 254: CY_ERR_ARG.  Needs no loaded weights. */
#define CY_FIT_FIELDS 32
/* status niter npix F lambda A x0 y0 a b c, then H upper triangle row-major (21);
   x0, y0 in image pixels */
int cy_fit_components(cy_ctx* ctx, const float* d_img, int MH, int MW,
                      const double* h_boxes, const double* h_bkg /* n */, const int* h_ncomp /* n */,
                      const double* h_start /* [n][CY_DBL_MAX_COMP][6], x0 y0 in image pixels */,
                      int n, int max_iter,
                      const unsigned char* h_mask, const long long* h_mask_off /* n + 1 */,
                      double* h_fit /* [n][CY_DBL_MAX_COMP][CY_FIT_FIELDS] */, void* stream);
/* milliseconds the kernel of the last cy_fit_components call that launched one took (hipEvents around the launch); -1 before it */
int cy_fit_kernel_ms(const cy_ctx* ctx, double* out_ms);

/* ---- joint fits of blends (an addition, the sixth measurement step) ---------------------------------------------------------
 * The sum of the Gaussians of every group of touching components fitted to the union of their basins, unweighted Levenberg-
 * Marquardt in float64.  Image, valid pixel, pixel-centre convention, box window, h_mask / h_mask_off, h_bkg, h_ncomp, the data
 * y = (double)v - bkg, the single-Gaussian model, its Jacobian expressions and roundings (every product rounded on its own) and
 * "admissible" are exactly those of cy_fit_components.
 *   adjacent   components k and l (both < ncomp) of one source are adjacent when some window pixel with mask byte k + 1 has a pixel
 *              with byte l + 1 among its 8 neighbours inside the window: always 8, whatever `conn` the islands were built with.
 *              Bytes 0, 255 and bytes above ncomp link nothing
 *   group      a connected set of the adjacency graph; its id is its lowest member index, its M members are taken in increasing
 *              index and the slot of a member is its position in that order
 *   job        one per group with 2 <= M <= CY_BLEND_MAX_MEMBERS.  Its LIST is the window pixels whose byte belongs to a member, in
 *              increasing window index i = dy * W + dx; its pixel set is the valid pixels of the list, npix their number.  A list
 *              entry that is not valid keeps its position and contributes nothing
 *   model      m = (..(m_0 + m_1) + ..) + m_{M-1}, m_s = A_s * exp(-0.5 * q_s) of member s in slot order;
 *              p = (p_0, .., p_{M-1}), P = 6 M parameters, member by member, each (A, x0, y0, a, b, c); admissible when every
 *              member is
 *   sweep      r = y - m; per entry the vector w = (r, J_0, .., J_{P-1}), J the members' six Jacobian entries one after the other.
 *              F = sum w_0 w_0, g_i = sum w_0 w_{1+i}, H_ij = sum w_{1+i} w_{1+j} (i <= j): the upper triangle of w^T w row-major,
 *              1 + P + P (P + 1) / 2 float64 sums (325 at M = 4).  ASSOCIATION: every sum is one plain sequential sum, started
 *              at 0 and taken over the list in increasing list position, every product rounded before it is added
 *   solve, iterate   as cy_fit_components on P parameters: Cholesky of H + lambda * diag(H) row by row, inner sums subtracted term
 *              by term in increasing index; lambda = 1e-3, accept: max(lambda / 10, 1e-12), reject: lambda *= 10 and status 2
 *              above 1e12; small = all P of |d_j| <= 1e-10 * (|p_j| + 1e-6); converged when small or F - F' <= 1e-14 * F;
 *              max_iter in [1, 256]
 *   covariance at the reported p of a status 0 or 2 job, C = inv(H): H = L L^T by the same Cholesky with lambda = 0; X = inv(L)
 *              column by column, X_cc = 1 / L_cc, X_ic = (0 - L_ic X_cc - .. - L_i,i-1 X_i-1,c) / L_ii (terms in increasing
 *              index); C_ij = X_ji X_jj + .. + X_P-1,i X_P-1,j (i <= j, increasing index, from 0).  A pivot that is not positive
 *              and finite: cov_ok = 0 and the C fields are 0.  Only every member's own 6 x 6 diagonal block of C is reported
 * h_out row of (source, component k), CY_BLEND_FIELDS float64 (rows at and beyond ncomp are 0):
 *   [0] status   0 converged; 1 the window has more than 2^24 pixels: nothing done, every other field 0; 2 max_iter or the lambda
 *                limit reached, the last accepted p reported; 3 npix < 6 M + 1: starts reported as given, niter = 0; 4 some member's
 *                start is not admissible (tested before 3): starts reported as given, niter = 0; 5 the group has more than
 *                CY_BLEND_MAX_MEMBERS members: nothing fitted, start reported as given, niter = npix = 0; 6 the component is alone
 *                in its group: no job, group = k, nmembers = 1, every other field 0.  With 3, 4 and 5, F, lambda, cov_ok and C are 0
 *   [1] niter, [2] npix, [3] F, [4] lambda   the job's, the same on every member's row
 *   [5] group, [6] nmembers, [7] slot, [8..13] A x0 y0 a b c of the member (x0, y0 in image pixels; the fit runs relative to the
 *   window), [14] cov_ok, [15..35] the upper triangle of the member's block of C, row-major
 * The runtime finds the adjacency bits, the groups (union-find), the job table and the lists in one pass over the mask bytes; one
 * launch (one workgroup of 256 threads per job, thread t adding sums t and t + 256 over the whole list; a job of up to 4096 list
 * entries keeps values and indices in LDS, a larger one re-reads them) and one copy back; synchronous on `stream`.  Two calls
 * give the same bytes.  n == 0, or no job at all: CY_OK, nothing launched.  Argument errors are exactly those of
 * cy_fit_components.  Needs no loaded weights. */
#define CY_BLEND_FIELDS 36
#define CY_BLEND_MAX_MEMBERS 4
/* status niter npix F lambda group nmembers slot A x0 y0 a b c cov_ok, then the member's block of C, upper triangle row-major (21) */
int cy_fit_blends(cy_ctx* ctx, const float* d_img, int MH, int MW,
                  const double* h_boxes, const double* h_bkg /* n */, const int* h_ncomp /* n */,
                  const double* h_start /* [n][CY_DBL_MAX_COMP][6], x0 y0 in image pixels */,
                  int n, int max_iter,
                  const unsigned char* h_mask, const long long* h_mask_off /* n + 1 */,
                  double* h_out /* [n][CY_DBL_MAX_COMP][CY_BLEND_FIELDS] */, void* stream);
/* milliseconds the kernel of the last cy_fit_blends call that launched one took (hipEvents around the launch); -1 before it */
int cy_blend_kernel_ms(const cy_ctx* ctx, double* out_ms);

/* ---- model and residual maps (an addition, the seventh measurement step) ---------------------------------------------------
 * The sum of m elliptical Gaussians rendered over the whole resident image d_img [MH][MW], and the image minus background minus
 * that model.  Image, valid pixel and pixel-centre convention are those of cy_measure_sources; the single-Gaussian model, its
 * expression for q (every product rounded on its own) and "admissible" are exactly those of cy_fit_components.  h_comp: m x
 * {A, x0, y0, a, b, c} float64 with x0, y0 in image pixels.
 *   term       of component k at pixel (ix, iy): A * exp(-0.5 * q), q = (a*u)*u + ((2*b)*u)*v + (c*v)*v, u = (double)ix - x0,
 *              v = (double)iy - y0
 *   support    component k contributes to the pixels of its support rectangle and to no others.  The rectangle is decided on the
 *              host in float64, every operation rounded on its own: det = a*c - b*b, hx = min(ceil(nsigma * sqrt(c / det)),
 *              CY_RND_HALF_MAX), hy = min(ceil(nsigma * sqrt(a / det)), CY_RND_HALF_MAX), a half-width that is not finite counting
 *              as above the cap; columns [max(0, floor(x0) - hx), min(MW - 1, floor(x0) + 1 + hx)], rows likewise with y0, hy and
 *              MH, compared in double before any conversion to int (a centre at 1e300 is a rectangle that misses the image)
 *   model      model(ix, iy) = one plain sequential float64 sum, started at 0, of the terms of the contributing components in
 *              increasing k
 * h_rows row of component k, CY_RND_FIELDS float64:
 *   [0] status   0 rendered; 1 not admissible, skipped; 2 rendered with a capped half-width (either one); 3 the rectangle misses
 *                the image, skipped
 *   [1] sx0, [2] sx1, [3] sy0, [4] sy1   the rectangle, inclusive, in image pixels; -1 when skipped
 *   [5] ntiles   32 x 32 tiles of the image (tile (ty, tx) covers ix in [32 tx, 32 tx + 31], iy likewise) the rectangle touches; 0
 *                when skipped.  [6..7] reserved (0)
 * d_model (may be NULL): (float)model at every pixel of the image, 0 where nothing contributes.  d_resid (may be NULL, not both):
 * (float)(((double)v - bkg) - model) on valid pixels, 0 on the others; bkg = (double)d_bkg[p], or 0 when d_bkg is NULL.  m == 0 is
 * legal: the model is 0 everywhere and the residual is v - bkg.
 * The runtime builds, per 32 x 32 tile, the list of rendered components whose rectangle meets it, in increasing index, and uploads
 * it; one launch (one workgroup of 256 threads per tile, the tile's components staged through LDS 64 at a time; no atomics) writes
 * both maps in one pass; synchronous on `stream`.  A pixel's value does not depend on the tiling: two calls give the same bytes.
 * nsigma outside [1, 8] or NaN, MH / MW <= 0, a null image, both outputs null, an image of 2^31 pixels or more, m outside
 * [0, 2^20], a null h_comp / h_rows with m > 0, or a tile table above 2^27 entries: CY_ERR_ARG.  h_rows is written only when the
 * call returns CY_OK.  Needs no loaded weights. */
#define CY_RND_FIELDS 8       /* status sx0 sx1 sy0 sy1 ntiles reserved reserved */
#define CY_RND_HALF_MAX 256
int cy_render_gaussians(cy_ctx* ctx, const float* d_img, int MH, int MW,
                        const double* h_comp /* [m][6] A x0 y0 a b c, x0 y0 in image pixels */, int m, double nsigma,
                        const float* d_bkg /* [MH][MW] or NULL */, float* d_model /* or NULL */, float* d_resid /* or NULL, not both */,
                        double* h_rows /* [m][CY_RND_FIELDS] */, void* stream);
/* milliseconds the kernel of the last cy_render_gaussians call took (hipEvents around the launch); -1 before the first call */
int cy_render_kernel_ms(const cy_ctx* ctx, double* out_ms);
/* cy_render_gaussians with amplitudes of either sign: a component is admissible with A != 0 in place of A > 0, and a negative one
 * lowers the model where a positive one raises it.  Everything else, word for word: the other conditions of "admissible", the
 * support rectangles, the rows, the order of the sum, the residual, the checks and cy_render_kernel_ms, which both entries set.
 * The second residual (--subtract_peaks) subtracts fitted peaks and fitted holes in one such call. */
int cy_render_signed_gaussians(cy_ctx* ctx, const float* d_img, int MH, int MW, const double* h_comp /* [m][6] */, int m, double nsigma,
                               const float* d_bkg, float* d_model, float* d_resid, double* h_rows /* [m][CY_RND_FIELDS] */, void* stream);

/* The residual of n catalog boxes against a model map d_model [MH][MW] (as cy_render_gaussians writes it).  Box window as
 * cy_measure_sources; h_mask / h_mask_off laid out as cy_deblend_islands writes them (both required; h_mask_off is checked
 * against the windows as in cy_fit_components); the island set of a window is the pixels whose mask byte is non-zero.  h_bkg:
 * one background per source.  On a valid pixel p: r = ((double)v - bkg_i) - (double)d_model[p]; other pixels contribute nothing.
 * h_out row, CY_RES_FIELDS float64:
 *   [0] status   0 measured; 1 the window has more than 2^24 pixels: nothing measured, every other field as for an empty window
 *   [1] npix_win, [2] npix_isl   valid pixels of the window / of its island set
 *   [3] sum_win = sum r, [4] sumsq_win = sum r * r over the window; [5] sum_isl, [6] sumsq_isl over the island set
 *   [7] maxabs_isl   largest |r| of the island set, [8] x_max, [9] y_max its first occurrence in row-major order, in image pixels;
 *                    0, -1, -1 when npix_isl == 0
 *   [10] model_isl = sum of (double)d_model[p] over the island set, [11] reserved (0)
 *   Empty window: counts and sums 0, position -1, status 0.
 * Counts, the maximum and its position do not depend on any order; the five sums are float64 with a fixed association, that of
 * cy_measure_islands: window pixel i = dy * W + dx on thread i mod 256, sequential per thread, a shuffle tree per wave of 64, the
 * four waves in order (two calls give the same bytes).  One launch (one workgroup per source) and one copy to h_out; synchronous
 * on `stream`.  n == 0: CY_OK, nothing launched.  n < 0, MH / MW <= 0, a null pointer, an image of 2^31 pixels or more, or
 * h_mask_off that disagrees with the windows: CY_ERR_ARG.  Needs no loaded weights. */
#define CY_RES_FIELDS 12      /* status npix_win npix_isl sum_win sumsq_win sum_isl sumsq_isl maxabs_isl x_max y_max model_isl reserved */
int cy_measure_residuals(cy_ctx* ctx, const float* d_img, const float* d_model, int MH, int MW, const double* h_boxes,
                         const double* h_bkg /* n */, int n, const unsigned char* h_mask, const long long* h_mask_off /* n + 1 */,
                         double* h_out /* [n][CY_RES_FIELDS] */, void* stream);
/* milliseconds the kernel of the last cy_measure_residuals call took (hipEvents around the launch); -1 before the first call */
int cy_residual_kernel_ms(const cy_ctx* ctx, double* out_ms);

/* ---- residual peaks (an addition: the local maxima of a map above k_sigma times a noise map) -------------------------------
 * d_map, d_rms: device fp32 maps [MH][MW]: the residual map of cy_render_gaussians and the rms map of cy_expand_background (any
 * pair of maps of one shape will do).  Pixel index i = iy * MW + ix, a pixel's centre at its index.
 *   u(p)       sign * d_map[p], sign +1 or -1 (the negation is exact; -1 finds holes, i.e. over-subtraction)
 *   valid(p)   u(p) is non-zero and finite (the residual map is 0 on the invalid pixels of the image)
 *   noisy(p)   d_rms[p] is finite and > 0
 *   above(p)   valid(p), noisy(p) and (double)u(p) >= k_sigma * (double)d_rms[p]: one float64 product, then the comparison
 *   rank       p outranks q when u(p) > u(q), or u(p) == u(q) and i(p) < i(q): the rule of cy_deblend_islands, over the whole image
 *   N(p)       the pixels q of the image with |qx - px| <= radius and |qy - py| <= radius: clipped at the edges, p included
 *   peak       above(p), and p outranks every valid q of N(p) other than itself (whether q is noisy does not matter here)
 * h_rows row of a peak, CY_PEAK_FIELDS float64, rows in increasing (y, x), i.e. in increasing pixel index:
 *   [0] x, [1] y   the pixel
 *   [2] v = (double)d_map[p] (signed), [3] rms = (double)d_rms[p], [4] snr = (double)u(p) / rms: one division
 *   [5] npix       valid q of N(p), [6] nabove   q of N(p) with above(q)
 *   [7] sum        sum of (double)u(q) over the valid q of N(p)
 *   [8] sw, [9] swx, [10] swy   sums of w, w * (qx - px), w * (qy - py) with w = max((double)u(q), 0) over the valid q of N(p)
 *                  (the products are exact); sw > 0 at a peak
 *   [11] reserved (0)
 * *h_total: the number of peaks of the whole image.  The first min(total, cap) rows are written, the rest of h_rows is left
 * untouched; cap == 0 only counts (h_rows may then be NULL).  Counts, positions, v, rms and snr do not depend on any order; the four
 * sums are plain sequential float64 sums over N(p) row by row (two calls give the same bytes).
 * The image is cut into segments of 1024 consecutive pixels of one row (the last of a row may be shorter), segments in row-major
 * order.  Three launches: one workgroup per segment tests every pixel and counts the segment's peaks (only a pixel that is above
 * reads its neighbourhood), one workgroup forms the exclusive prefix sum of the counts, one workgroup per segment writes its rows
 * at the segment's offset.  No workgroup waits for another, no atomics; synchronous on `stream`.  A null ctx / d_map / d_rms /
 * h_total, a null h_rows with cap > 0, MH / MW <= 0, radius outside [1, CY_PEAK_RADIUS_MAX], sign not +1 or -1, k_sigma not
 * finite or <= 0, cap outside [0, CY_PEAK_CAP_MAX], an image of 2^31 pixels or more, one of more than 2^24 segments, or a row whose
 * last segment plus the radius ends beyond column 2^31 - 1 (MW above 2^31 - 1024): CY_ERR_ARG.  Needs no loaded weights. */
#define CY_PEAK_FIELDS 12      /* x y v rms snr npix nabove sum sw swx swy reserved */
#define CY_PEAK_RADIUS_MAX 8
#define CY_PEAK_CAP_MAX (1 << 20)
int cy_find_peaks(cy_ctx* ctx, const float* d_map, const float* d_rms, int MH, int MW, double k_sigma, int radius, int sign,
                  int cap, double* h_rows /* [cap][CY_PEAK_FIELDS] */, long long* h_total, void* stream);
/* milliseconds the three kernels of the last cy_find_peaks call took (hipEvents around the launches); -1 before the first call */
int cy_peaks_kernel_ms(const cy_ctx* ctx, double* out_ms);

/* ---- a trous wavelet level (an addition: one level of the B3-spline "starlet" decomposition of a map) ------------------------
 * d_in: device fp32 map [MH][MW] (the residual map of cy_render_gaussians, or the smooth plane of the level before).  All in float64:
 *   a(x, y)     (double)d_in[y][x] when that value is finite, else 0.0
 *   fold(i, N)  0 when N == 1; otherwise p = 2 (N - 1), i = i mod p (non-negative), and p - i when i >= N, else i: mirror without
 *               repeating the edge, valid for any offset, also when 2 * step >= N
 *   h           (1/16, 1/4, 3/8, 1/4, 1/16), exact in binary; s = step
 *   R(x, r)     = h0 * a(fold(x - 2s, MW), r), then += h1 * a(fold(x - s, MW), r), += h2 * a(x, r), += h3 * a(fold(x + s, MW), r),
 *               += h4 * a(fold(x + 2s, MW), r): float64 sums in exactly this order, products and sums rounded separately
 *   C(x, y)     the same five-term expression over R(x, fold(y + (k - 2) s, MH)), k = 0 .. 4, in that order
 *   d_smooth[y][x] = (float)C, one rounding to nearest even;  d_detail[y][x] = (float)(a(x, y) - (double)(float)C)
 * Multiply and add are not contracted in the kernel, so every operation is one IEEE operation and a restatement in the same order
 * gives the same bits (R depends on (x, row) only: the kernel forms each row sum once per column and walks the rows of one residue
 * class y mod s with the last five row sums in registers; no LDS, no atomics, and it reads nothing outside the image).  Either
 * output may be NULL, not both.  Two calls give the same bytes; synchronous on `stream`; needs no loaded weights.  A null ctx or
 * d_in, both outputs null, MH or MW <= 0, step outside [1, CY_ATROUS_STEP_MAX] (any integer, not only powers of two), an image of
 * 2^31 pixels or more, or an output whose MH * MW floats overlap the input's or the other output's: CY_ERR_ARG, nothing launched. */
#define CY_ATROUS_STEP_MAX 64
int cy_atrous_step(cy_ctx* ctx, const float* d_in, int MH, int MW, int step,
                   float* d_smooth /* or NULL */, float* d_detail /* or NULL */, void* stream);
/* milliseconds the kernel of the last cy_atrous_step call took (hipEvents around the launch); -1 before the first call */
int cy_atrous_kernel_ms(const cy_ctx* ctx, double* out_ms);

/* ---- aperture sums at given positions (an addition: concentric circular apertures, a curve of growth) --------------------------
 * d_map: device fp32 map [MH][MW] (the residual map of cy_render_gaussians: a masked pixel is 0); d_rms: the rms map of the same
 * shape, or NULL.  h_jobs: [n][3] {cx, cy, unit} in image pixels, pixel centres at integers; h_factors: [K], 1 <= K <=
 * CY_APER_RINGS_MAX.  Everything in float64, every product and sum rounded on its own (no contraction):
 *   radii     r_k = h_factors[k] * unit, r2_k = r_k * r_k, k = 1 .. K
 *   valid(q)  the value of d_map at q is non-zero and finite (the rule of cy_find_peaks)
 *   d2(q)     dx = (double)qx - cx, dy = (double)qy - cy, d2 = dx*dx + dy*dy: two products and one sum
 *   ring      q lies in ring k when k is the smallest index with d2 <= r2_k: ring 1 is a disc, a boundary belongs to the inner
 *             ring, a pixel beyond r2_K belongs to no ring
 *   window    decided on the host in double before any conversion to int: columns [max(0, ceil(cx - r_K)), min(MW - 1,
 *             floor(cx + r_K))], rows likewise with cy and MH; only pixels of the window are looked at
 * Row i of h_out, CY_APER_FIELDS float64:
 *   [0] status    0 measured;  1 unit not finite or <= 0, or r_K not finite or above CY_APER_RADIUS_MAX;  2 cx or cy not finite, or
 *                 the window misses the image or holds no pixel (status 1 is decided first).  Not measured: [1..4] are -1 and every
 *                 other field 0
 *   [1..4]        x0 x1 y0 y1, the window, inclusive
 *   [5] clipped   1 when the window before the clip to the image leaves the image
 *   [6] bkg_med   the exact median of (double)v over the valid pixels of ring K: the element of rank (n - 1) / 2 for an odd n, the
 *                 float64 mean of the two middle elements for an even n
 *   [7] bkg_mad   the exact median, by the same rule, of |(double)v - bkg_med| over the same pixels; both 0 without a valid pixel
 *   ring k at [CY_APER_HEAD + CY_APER_RING_FIELDS (k - 1)]: npix, the valid pixels of the ring; sum of (double)v; sumsq of v*v; svar,
 *                 the sum of rms*rms over the valid pixels of the ring whose d_rms is finite and > 0 (0 with a NULL d_rms).  Rings
 *                 above K are 0
 * Association of the three sums of a ring, that of cy_measure_residuals: window pixel i = dy * W + dx goes to thread i mod 256,
 * every thread sums sequentially in increasing i starting from +0.0, a tree with offsets 32, 16 .. 1 adds the 64 lanes of a wave
 * (lane l takes lane l + offset), and the four waves are added in order.  Counts and the medians depend on no order.  One workgroup
 * per job; no atomics outside LDS, where they are integer counts.  Two calls give the same bytes; synchronous on `stream`; needs no
 * loaded weights; the maps are only read.
 * CY_ERR_ARG, nothing launched and h_out untouched: a null ctx; MH or MW <= 0; an image of 2^31 pixels or more; n outside
 * [0, CY_APER_JOBS_MAX]; K outside [1, CY_APER_RINGS_MAX]; with n > 0 a null d_map, h_jobs, h_factors or h_out; factors that are
 * not finite, not positive or not strictly increasing (checked whenever h_factors is given).  n == 0: CY_OK, nothing launched. */
#define CY_APER_RINGS_MAX 8
#define CY_APER_RADIUS_MAX 256
#define CY_APER_HEAD 8
#define CY_APER_RING_FIELDS 4      /* npix sum sumsq svar */
#define CY_APER_FIELDS (CY_APER_HEAD + CY_APER_RING_FIELDS * CY_APER_RINGS_MAX)   /* 40 */
#define CY_APER_JOBS_MAX (1 << 20)
int cy_aperture_sums(cy_ctx* ctx, const float* d_map, const float* d_rms /* or NULL */, int MH, int MW,
                     const double* h_jobs /* [n][3] cx cy unit, image pixels */, int n,
                     const double* h_factors /* [K] */, int K, double* h_out /* [n][CY_APER_FIELDS] */, void* stream);
/* milliseconds the kernel of the last cy_aperture_sums call took (hipEvents around the launch); -1 before the first call */
int cy_aperture_kernel_ms(const cy_ctx* ctx, double* out_ms);

/* ---- Gaussian fits at given positions (an addition: a shape for every residual and scale peak) --------------------------------
 * One elliptical Gaussian per job, fitted to the pixels of a disc around the job's centre on d_map (device fp32 [MH][MW], the
 * residual map of cy_render_gaussians).  h_jobs: [n][CY_PFIT_JOB_FIELDS] {cx, cy, R, bkg, sign, A, x0, y0, a, b, c}: the centre and
 * radius of the disc, and the start of the fit with x0, y0 in image pixels.  Everything in float64, every product and sum rounded
 * on its own (no contraction); valid pixel and pixel-centre convention as cy_aperture_sums.
 *   planner    on the host, before any device work.  Status 1: R not finite, <= 0 or > CY_PFIT_RADIUS_MAX, sign not exactly +1 or
 *              -1, or bkg not finite.  Status 5 (status 1 is tested first): cx or cy not finite, or the window holds no pixel of
 *              the image.  The window is columns [ceil(cx - R), floor(cx + R)], rows likewise with cy, clipped to the image;
 *              clipped = 1 when the unclipped window leaves the image.  A job with status 1 or 5 reports the window as -1 and
 *              zeros elsewhere and launches no work
 *   neighbours of a job e with planner status 0: the other jobs f of the call with planner status 0 and D2 = (cx_f - cx_e)^2 +
 *              (cy_f - cy_e)^2 < 4 * (R_e * R_e), ordered by (D2, job index); the first CY_PFIT_NEIGH_MAX are kept, nneigh =
 *              min(count, 8), crowded = 1 when count > 8.  Coincident centres (D2 = 0) are neighbours
 *   pixel set  window pixel (qx, qy) is a member of job e when d2_e = (qx - cx_e)^2 + (qy - cy_e)^2 <= R_e * R_e and d2_f >= d2_e
 *              for every kept neighbour f; distances in image coordinates; a pixel that ties belongs to both jobs.  npix: the
 *              valid members; nexcluded: the valid pixels inside the disc that a neighbour took
 *   data       y = sign * ((double)v - bkg).  Model, "admissible", the 28 sums, the 6 x 6 Cholesky and the iteration are word for
 *              word those of cy_fit_components; the fit runs on x0 - wx0, y0 - wy0 (relative to the window's first pixel) and
 *              reports image pixels.  A is reported positive: the caller applies the sign
 *   LIST and ASSOCIATION   the job's list is every pixel of the window in increasing window index i = dy * W + dx, entry i on
 *              thread i mod 256; a pixel that is not a valid member keeps its position and contributes nothing; then the block
 *              reduction of the measurement kernels.  Two calls give the same bytes
 *   after the planner   status 4: the start is not admissible (tested before 3); 3: npix < 7; 0: converged; 2: max_iter or the
 *              lambda limit reached.  With 3 and 4 the start is reported as given, niter = 0 and F, lambda and H are 0
 * Row i of h_out, CY_PFIT_FIELDS float64: [0] status, [1] niter, [2] npix, [3] F, [4] lambda, [5..10] A x0 y0 a b c, [11..31] H
 * upper triangle row-major, [32..35] wx0 wx1 wy0 wy1, [36] clipped, [37] nneigh, [38] crowded, [39] nexcluded.
 * One launch: one workgroup of 256 threads per planner-status-0 job; a window of up to 8192 pixels keeps its members' values in
 * LDS, a larger one evaluates membership again in every sweep.  Synchronous on `stream`; needs no loaded weights; the map is only
 * read.  CY_ERR_ARG with a message (cy_last_error), nothing launched and h_out untouched, checked in this order after a null ctx:
 * MH or MW <= 0; an image of 2^31 pixels or more; n outside [0, CY_PFIT_JOBS_MAX]; max_iter outside [1, 256]; with n > 0 a null
 * d_map, h_jobs or h_out.  n == 0: CY_OK, nothing launched. */
#define CY_PFIT_JOB_FIELDS 11    /* cx cy R bkg sign A x0 y0 a b c   (x0, y0 in image pixels) */
#define CY_PFIT_FIELDS     40
#define CY_PFIT_RADIUS_MAX 256
#define CY_PFIT_NEIGH_MAX  8
#define CY_PFIT_JOBS_MAX   (1 << 20)
int cy_fit_peaks(cy_ctx* ctx, const float* d_map, int MH, int MW, const double* h_jobs /* [n][CY_PFIT_JOB_FIELDS] */, int n,
                 int max_iter, double* h_out /* [n][CY_PFIT_FIELDS] */, void* stream);
/* milliseconds the kernel of the last cy_fit_peaks call that launched one took (hipEvents around the launch); -1 before it */
int cy_peakfit_kernel_ms(const cy_ctx* ctx, double* out_ms);

/* ---- joint fits of groups of peaks (an addition: neighbouring peaks are fitted together, not on halves of their shared pixels) --
 * The sum of M elliptical Gaussians fitted to the union of the discs of M linked jobs on d_map.  h_jobs: as cy_fit_peaks, the start
 * usually that call's result.  Everything in float64, every product and sum rounded on its own.
 *   planner    per job the status (1 / 5), the window, clipped and the kept-neighbour list are those of cy_fit_peaks
 *   link       two planner-status-0 jobs e, f with equal sign are LINKED when D2 < Lm * Lm, Lm = link * max(R_e, R_f), D2 =
 *              (cx_f - cx_e)^2 + (cy_f - cy_e)^2 formed as for the neighbours.  Strict; symmetric; coincident centres are linked.
 *              nlinked: the jobs directly linked to a job
 *   group      a connected set of the link graph.  Its id is its lowest job index; its M members are taken in increasing job
 *              index, a member's slot is its position in that order
 *   job        one per group with 2 <= M <= CY_BLEND_MAX_MEMBERS.  Its window is the bounding box of the members' windows.
 *              Window pixel q belongs to the group's pixel set when for some member e: d2_e <= R_e * R_e, and d2_f >= d2_e for
 *              every kept neighbour f of e that is NOT a member of the group.  Jobs outside the group keep their nearest-centre
 *              share; inside the group nothing is divided.  npix: the valid pixels of the set; nexcluded: the valid pixels inside
 *              some member's disc that are in no member's share
 *   data       y = sign * ((double)v - bkg) with bkg (and sign) of the member in slot 0
 *   model and algebra   the sums (w = (r, J_0 .. J_{P-1}), upper triangle of w^T w row-major), the solve, the iteration, `small`,
 *              the convergence test and the covariance blocks (C = inv(H), each member's own 6 x 6 block) are word for word those
 *              of cy_fit_blends.  The job's LIST is every pixel of the group window in increasing window index; a pixel that is
 *              not a valid member keeps its position and contributes nothing; every sum is one plain sequential sum in list
 *              order.  Two calls give the same bytes.  The fit runs relative to the window's first pixel and reports image
 *              pixels; A is reported positive
 *   status     tested in this order: 1 and 5 as cy_fit_peaks; 6 the job is alone (no launch, group = own index, nmembers = 1,
 *              the job's own window and clipped flag); 7 the group has more than CY_BLEND_MAX_MEMBERS members (the start reported
 *              as given); 4 some member's start is not admissible (tested before 3); 3 npix < 6 M + 1; 0 converged; 2 max_iter
 *              or the lambda limit reached.  3, 4 and 7 report the starts bit for bit, niter = 0, F, lambda, cov_ok and C are 0
 * Row i of h_out, CY_PGRP_FIELDS float64: [0 .. 35] the fields of a cy_fit_blends row (`group` is a job index), [36..39] wx0 wx1
 * wy0 wy1 of the group window, [40] clipped (any member's), [41] nexcluded, [42] nlinked, [43] 0.  Rows of statuses 1 and 5: the
 * status, the window as -1 and zeros elsewhere.
 * One launch: one workgroup of 256 threads per group job; a group window of up to 8192 pixels keeps its members' values in LDS, a
 * larger one evaluates membership again in every sweep.  Synchronous on `stream`; needs no loaded weights; the map is only read.
 * CY_ERR_ARG with a message, nothing launched and h_out untouched, checked in the order of cy_fit_peaks, with link not finite,
 * <= 0 or > 2 after max_iter.  n == 0, or no group job: CY_OK, nothing launched. */
#define CY_PGRP_FIELDS 44
int cy_fit_peak_groups(cy_ctx* ctx, const float* d_map, int MH, int MW, const double* h_jobs /* [n][CY_PFIT_JOB_FIELDS], as cy_fit_peaks */,
                       int n, double link, int max_iter, double* h_out /* [n][CY_PGRP_FIELDS] */, void* stream);
/* milliseconds the kernel of the last cy_fit_peak_groups call that launched one took (hipEvents around the launch); -1 before it */
int cy_peakgroup_kernel_ms(const cy_ctx* ctx, double* out_ms);

/* ---- residuals on the discs of given jobs (an addition: what a map still holds where a peak was fitted) -------------------------
 * Count, sum, sum of squares and largest |r| of d_map (device fp32 [MH][MW]) on the pixel set of every job, and the sum of a
 * second map d_model (same shape, or NULL) over the same pixels.  The chain gives it the second residual (the residual map minus
 * the fitted peaks, cy_render_signed_gaussians with d_img = the residual map) and the peak model, with the jobs of cy_fit_peaks: a row
 * then says what the fit of that job left behind on exactly the pixels it was fitted to.  h_jobs: [n][CY_PFIT_JOB_FIELDS] as
 * cy_fit_peaks; only cx, cy, R, bkg and sign are read, sign is validated and otherwise unused, the start is ignored.  Everything in
 * float64, every product and sum rounded on its own (no contraction); valid pixel and pixel-centre convention as
 * cy_aperture_sums.
 *   planner    that of cy_fit_peaks, word for word: statuses 1 and 5, the window, clipped, the neighbours (nneigh) and with them
 *              the PIXEL SET: window pixel (qx, qy) is a member of job e when d2_e <= R_e * R_e and d2_f >= d2_e for every kept
 *              neighbour f; a pixel that ties belongs to both jobs.  npix: the valid members; nexcluded: the valid pixels inside
 *              the disc that a neighbour took
 *   data       on a valid member p: r = (double)v - bkg, one rounded operation, no sign applied
 *   LIST and ASSOCIATION   window pixel i = dy * W + dx sits on thread i mod 256, every sum runs sequentially per thread over
 *              increasing i; then the block reduction of the measurement kernels: sums for the three sums and the two counts,
 *              the first maximum for |r| with the window index.  Two calls give the same bytes
 * Row i of h_out, CY_DRES_FIELDS float64: [0] status (0 measured; 1 / 5 the planner's), [1] npix, [2] nexcluded, [3] sum r,
 * [4] sum r * r, [5] maxabs = the largest |r|, [6] x_max, [7] y_max its first occurrence in window-index order, in image pixels
 * (npix == 0: -1, -1 and maxabs 0), [8] model_sum = the sum of (double)d_model[p] over the members (0 when d_model is NULL),
 * [9] reserved (0), [10..13] wx0 wx1 wy0 wy1, [14] clipped, [15] nneigh.  Rows of statuses 1 and 5: the status, the window and the
 * position as -1 and zeros elsewhere.
 * One launch: one workgroup of 256 threads per planner-status-0 job, one sweep over its window, pixel addresses formed in 64 bits.
 * Synchronous on `stream`; needs no loaded weights; the maps are only read.  CY_ERR_ARG with a message (cy_last_error), nothing
 * launched and h_out untouched, checked in this order after a null ctx: MH or MW <= 0; an image of 2^31 pixels or more; n outside
 * [0, CY_PFIT_JOBS_MAX]; with n > 0 a null d_map, h_jobs or h_out.  n == 0, or no planner-status-0 job: CY_OK, nothing launched,
 * and cy_disc_residual_kernel_ms keeps its value. */
#define CY_DRES_FIELDS 16   /* status npix nexcluded sum sumsq maxabs x_max y_max model_sum reserved wx0 wx1 wy0 wy1 clipped nneigh */
int cy_disc_residuals(cy_ctx* ctx, const float* d_map, const float* d_model /* or NULL */, int MH, int MW,
                      const double* h_jobs /* [n][CY_PFIT_JOB_FIELDS], as cy_fit_peaks */, int n,
                      double* h_out /* [n][CY_DRES_FIELDS] */, void* stream);
/* milliseconds the kernel of the last cy_disc_residuals call that launched one took (hipEvents around the launch); -1 before it */
int cy_disc_residual_kernel_ms(const cy_ctx* ctx, double* out_ms);

/* ---- forced photometry (an addition: linear fits of fixed shapes on any map) -----------------------------------------------
 * The amplitude of a Gaussian of FIXED position and shape on d_map (device fp32 [MH][MW]), with an error, for every job: a
 * weighted linear least-squares problem per job whose unknowns are the job's amplitude, the amplitudes of its overlapping
 * neighbours and (fit_bkg) a local constant.  d_rms: a noise map of the same shape, or NULL (unit weights).  The chain gives it
 * the components it rendered, on the detection image and on any co-registered map.  h_jobs: [n][CY_FORCED_JOB_FIELDS] {x0, y0, a,
 * b, c, bkg}, positions in image pixels.  Image, valid pixel and pixel-centre conventions are those of cy_measure_sources; a
 * usable rms r is finite and > 0.  Everything in float64, every product and sum rounded on its own (no contraction).
 *   q            q = (a*u)*u + ((2*b)*u)*v + (c*v)*v, u = ix - x0, v = iy - y0: the expression of cy_render_gaussians
 *   admissible   the five shape and position fields and bkg finite, a > 0, c > 0, a*c - b*b > 0 (cy_fit_components' rule without
 *                the amplitude); otherwise status 1
 *   rectangle    the support rectangle of cy_render_gaussians for (x0, y0, a, b, c) and nsigma, by the same code: half-widths
 *                capped at CY_RND_HALF_MAX (status 2), status 3 when it misses the image; at most 514 x 514 pixels
 *   runnable     a job of status 0 or 2
 *   neighbours   of job k: the runnable jobs f != k whose clipped rectangle intersects k's, ordered by (D2, f), D2 = dx*dx + dy*dy
 *                of the centres.  Walking that order, a candidate whose x0 y0 a b c compare equal to k's or to those of a
 *                neighbour kept before it is dropped and counted in ndup (an exact duplicate would make the system singular);
 *                otherwise it is kept while fewer than CY_FORCED_NEIGH_MAX = 7 are kept, and sets crowded = 1 when they are
 *   unknowns     K = 1 + nneigh + fit_bkg <= 9, in this order: the job's amplitude, the neighbours' in kept order, the constant
 *   pixel set    window pixel (ix, iy) of k's rectangle with q_k <= nsigma * nsigma (the product rounded once), a valid v and,
 *                with d_rms, a usable rms.  A pixel inside the ellipse that fails the second or third test counts in nexcluded.
 *                Neighbours contribute their wings on k's pixels whether or not the pixel lies inside their own ellipse
 *   per pixel    s = 1 / (double)rms (1 without d_rms); w = (((double)v - bkg) * s, e_0 * s, .., e_nneigh * s, [s]) with
 *                e_i = exp(-0.5 * q_i); the sums are the upper triangle of w^T w (at most 55): syy = w_0 w_0, b_i = w_0 w_{1+i},
 *                N_ij = w_{1+i} w_{1+j}
 *   ORDER        window pixel i = wy * W + wx sits on thread i mod 256; every sum runs sequentially per thread over increasing i,
 *                then the block reduction of the measurement kernels (six steps with offsets 32 .. 1 inside a wave, then the four
 *                waves in order).  Two calls give the same bytes
 *   solve        npix < K: status 5.  Cholesky N = L L^T row by row: t = N_jj - L_j0^2 - .. - L_j,j-1^2 subtracted term by term in
 *                increasing k; the pivot fails, and the status is 4, when !(t > N_jj * 2^-40) or t is not finite; L_ij = (N_ji -
 *                sum_k<j L_ik L_jk) / L_jj likewise.  z = L^-1 b by forward and x = L^-T z by back substitution, X = L^-1 column by
 *                column, C_ij = sum_k>=max(i,j) X_ki X_kj added in increasing k
 *   chi2         a second sweep over the same pixel set in the same order: the sum of (w_0 - m)^2 with m = x_0 w_1, then
 *                + x_i w_{1+i} in increasing i, every product rounded; not the cancelling syy - x.b
 * Row i of h_out, CY_FORCED_FIELDS float64: [0] status (0 fitted, 1 not admissible, 2 fitted with a capped half-width, 3 the
 * rectangle misses the image, 4 no positive pivot, 5 npix < K, an empty set included), [1] npix, [2] nexcluded, [3] K, [4] nneigh,
 * [5] crowded, [6] ndup, [7] amp = x_0, [8] amp_var = C_00, [9] bkg_off (the constant), [10] bkg_var, [11] cov_amp_bkg (all three 0
 * with fit_bkg == 0), [12] chi2, [13] syy, [14] n00 = N_00, [15] b0, [16] corr_max = the largest |C_0i| / sqrt(C_00 * C_ii) over the
 * neighbours (0 without any), [17..20] wx0 wx1 wy0 wy1, [21] capped, [22] [23] 0.  Rows of status 1 and 3: the status, the window as
 * -1 and zeros.  Rows of status 4 and 5: the counts, the sums and the window, zeros for the solution (fields 7 .. 12 and 16).
 * One launch: one workgroup of 256 threads per runnable job, two sweeps over its window, pixel addresses formed in 64 bits.
 * Synchronous on `stream`; needs no loaded weights; the maps are only read.  CY_ERR_ARG with a message (cy_last_error), nothing
 * launched and h_out untouched, checked in this order: a null ctx or d_map; MH or MW <= 0; an image of 2^31 pixels or more; nsigma
 * outside [1, 8] or NaN; fit_bkg not 0 or 1; n outside [0, CY_FORCED_JOBS_MAX]; with n > 0 a null h_jobs or h_out.  n == 0, or no
 * runnable job: CY_OK, nothing launched, and cy_forced_kernel_ms keeps its value. */
#define CY_FORCED_JOB_FIELDS 6   /* x0 y0 a b c bkg */
#define CY_FORCED_FIELDS 24      /* status npix nexcluded K nneigh crowded ndup amp amp_var bkg_off bkg_var cov_amp_bkg chi2 syy n00 b0
                                    corr_max wx0 wx1 wy0 wy1 capped 0 0 */
#define CY_FORCED_NEIGH_MAX 7
#define CY_FORCED_JOBS_MAX (1 << 20)
int cy_forced_fit(cy_ctx* ctx, const float* d_map, const float* d_rms /* or NULL */, int MH, int MW,
                  const double* h_jobs /* [n][CY_FORCED_JOB_FIELDS] */, int n, double nsigma, int fit_bkg,
                  double* h_out /* [n][CY_FORCED_FIELDS] */, void* stream);
/* milliseconds the kernel of the last cy_forced_fit call that launched one took (hipEvents around the launch); -1 before it */
int cy_forced_kernel_ms(const cy_ctx* ctx, double* out_ms);

/* ---- background and noise mesh (an addition: a global noise map for the measurement steps) ---------------------------------
 * Iteratively clipped median and MAD of every cell of a mesh over the resident image d_img [MH][MW].  Image, validity of a pixel
 * and pixel-centre convention are those of cy_measure_sources.
 *   mesh   ncx = ceil(MW / cell), ncy = ceil(MH / cell); cell (cy, cx) covers ix in [cx * cell, min(MW, (cx + 1) * cell) - 1], iy
 *          likewise: the last row / column of cells may be partial
 *   med(V) exact median of a set of pixels as float64 (even count: (a + b) / 2), sig(V) = 1.4826 * exact median of |v - med(V)|
 *   clip   V_0 = the cell's valid pixels; lo = med(V_j) - k * sig(V_j), hi = med(V_j) + k * sig(V_j), V_{j+1} = the v of V_j with
 *          lo <= (double)v <= hi; so V_j = V_0 inside [L_j, H_j], L_j = max(L_{j-1}, lo_{j-1}), H_j = min(H_{j-1}, hi_{j-1}).
 *          An empty V_j is not clipped again (its median and sig count as 0)
 * h_out row, CY_BKG_FIELDS float64, rows in cell order [ncy][ncx]:
 *   [0] n0 = |V_0|, [1] n = |V_niter|, [2] bkg = med(V_niter), [3] rms = sig(V_niter)
 *   [4] L, [5] H   the final interval; -inf, +inf when niter == 0 or n0 == 0
 *   [6] rounds     clips that removed at least one pixel, [7] reserved (0)
 *   n == 0: bkg = rms = 0.
 * Every field is a count, a selection or one rounded operation on selections: none depends on the order in which pixels are
 * visited (two calls give the same bytes).  One launch (one workgroup per cell; a cell of up to 128 x 128 pixels is held in LDS,
 * a larger one is re-read from the image) and one copy to h_out; synchronous on `stream`.  cell outside [4, 4096], k not > 0 (or
 * NaN), niter outside [0, 32], MH / MW <= 0, a null pointer, or an image of 2^31 pixels or more: CY_ERR_ARG.  Needs no loaded
 * weights. */
#define CY_BKG_FIELDS 8   /* n0 n bkg rms L H rounds reserved */
int cy_measure_background(cy_ctx* ctx, const float* d_img, int MH, int MW, int cell, double k, int niter,
                          double* h_out /* [ncy][ncx][CY_BKG_FIELDS] */, void* stream);
/* milliseconds the kernel of the last cy_measure_background call took (hipEvents around the launch); -1 before the first call */
int cy_background_kernel_ms(const cy_ctx* ctx, double* out_ms);
/* A filled mesh h_mesh [ncy][ncx] x {bkg, rms} float64 (host) expanded to per-pixel fp32 maps [MH][MW] in the caller's device
 * buffers d_bkg / d_rms (either may be NULL, not both).  The centre of cell cx is cx * cell + (cell - 1) / 2.0, also for a
 * partial edge cell.  At pixel ix: t = (ix - (cell - 1) / 2.0) / cell clamped to [0, ncx - 1], i0 = min(floor(t), ncx - 2),
 * fx = t - i0 (i0 = 0, fx = 0 when ncx == 1); iy likewise; value = (m00 * (1 - fx) + m01 * fx) * (1 - fy) + (m10 * (1 - fx) +
 * m11 * fx) * fy in float64, every operation rounded on its own, then rounded to fp32: constant outside the outermost centres.
 * One upload, one launch; synchronous on `stream`.  cell outside [4, 4096], MH / MW <= 0, a null mesh or two null outputs, an
 * image of 2^31 pixels or more, or ncy / ncx that are not ceil(MH / cell) / ceil(MW / cell): CY_ERR_ARG.  Needs no loaded weights. */
int cy_expand_background(cy_ctx* ctx, const double* h_mesh /* [ncy][ncx][2], filled */, int ncy, int ncx, int cell, int MH, int MW,
                         float* d_bkg, float* d_rms, void* stream);

/* ---- catalog records and cross-tile merge (host code, no GPU) --------------------------------- */
/* Analyzer.make_json_results (caesar_yolo/evaluation.py:418-469: int() truncation, tile-local edge rule, tile origin)
 * followed by SFinder.find_sources_at_edge (caesar_yolo/inference.py:663-726).
 * det: n x 6 floats {x1,y1,x2,y2,score,class} in TILE pixels, grouped by tile in ascending tile order;
 * det_tile: n tile ids; tiles: T x 4 ints {xmin, xmax_excl, ymin, ymax_excl} (utils.generate_tiles order);
 * rec: n x 8 doubles {x1,y1,x2,y2,score,class_id,tile_id,edge}, edge = 0 | 1 (tile-local rule only, int in the
 * reference JSON) | 2 (set True by find_sources_at_edge) */
int cy_make_tile_records(const float* det, const int* det_tile, int n, const int* tiles, int T, double* rec);
/* SFinder.merge_edge_sources (caesar_yolo/inference.py:731-931) on those records.
 * out: up to n x 8 doubles {x1,y1,x2,y2,score,class_id,edge,merged}; returns the number of output sources (>= 0) */
int cy_merge_edge_sources(const double* rec, int n, const int* tiles, int T, double* out);

#ifdef __cplusplus
}
#endif
#endif
