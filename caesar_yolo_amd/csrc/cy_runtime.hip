// Runtime behind the C-ABI (include/caesar_yolo_hip.h): context, weight upload, workspace, and the host loops that
// enqueue the gfx950 kernels.  One context per GPU / per process (one process per GPU under torch.distributed).
#include "../../include/caesar_yolo_hip.h"
#include "cy_kernels.h"
#include "cy_measure_plan.h"
#include "cy_plan.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace cy;

// device copies of one convolution: views into cy_ctx::weights (load) or into the owner of a test entry call
struct DevConv { void* w = nullptr; float* bias = nullptr; size_t wbytes = 0; float* stem_w = nullptr; void* w32 = nullptr; size_t w32bytes = 0;
                 float* oscale = nullptr;       // fp16x3 context: 2^-e per output channel (undoes the weight scale in the epilogue)
                 void* w2f = nullptr; size_t w2fbytes = 0;   // on the SECOND layer of a back-to-back pair: its weights in the first layer's accumulator order (pack_weights_fused2)
                 int passes = 3;                // fp16x3 context: passes over K -- 3, or 2 when the filter is fp16-exact up to a per-channel scale (then oscale = that scale)
                 float* dw_w = nullptr;         // dw_w: depth-wise 3x3 weights [9][C] fp32 (YOLO11)
                 void* bneck = nullptr; };      // on a bottleneck's cv1: register-fragment weights of the fused cv1+cv2 kernel (bneck64.hip)

// the measurement steps whose kernel time the context keeps (cy_ctx::step_ms)
enum MeasureStep { STEP_SOURCES = 0, STEP_ISLANDS, STEP_DEBLEND, STEP_FIT, STEP_BLEND, STEP_BACKGROUND, STEP_RENDER, STEP_RESIDUAL, STEP_PEAKS, STEP_ATROUS, STEP_APERTURE, STEP_PEAKFIT, STEP_PEAKGROUP, STEP_DISCRES, STEP_FORCED, STEP_COUNT };

// Owner of device allocations: one hipMalloc per buffer, every one freed on destruction or reset().  Whoever needs device memory
// beyond one launch holds one (the context: model weights, stage buffers and workspaces, counters; a kernel-level test entry: the
// scratch of that call, freed on every return path); the pointers handed out are views.  In the fp16x3 context the test entries take
// fp32 [pix][ct] caller tensors and run the kernel on split copies [pix][2 ct] (high halves, then the low halves ct behind: the
// forward's layout, channel offsets included); split() makes such a copy, the caller merges the written one back with launch_x3_merge.
struct DevOwner {
    std::vector<void*> p;
    DevOwner() = default;
    DevOwner(const DevOwner&) = delete;
    DevOwner& operator=(const DevOwner&) = delete;
    ~DevOwner() { reset(); }
    void reset() { for (void* q : p) hipFree(q); p.clear(); }
    template <class T> hipError_t alloc(size_t bytes, T** out) {
        void* d = nullptr;
        const hipError_t e = hipMalloc(&d, bytes);
        if (e == hipSuccess) p.push_back(d);
        *out = static_cast<T*>(d);
        return e;
    }
    template <class T> hipError_t upload(const void* host, size_t bytes, T** out) {      // alloc + blocking copy of a host span
        const hipError_t e = alloc(bytes, out);
        return e == hipSuccess ? hipMemcpy(*out, host, bytes, hipMemcpyHostToDevice) : e;
    }
    hipError_t split(const void* t, long npix, int ct, void** out, hipStream_t s) {
        hipError_t e = alloc((size_t)npix * ct * 4, out);
        return e == hipSuccess ? cy::launch_x3_split(reinterpret_cast<const float*>(t), *out, npix, ct, s) : e;
    }
};

struct cy_ctx {
    int device = 0;
    cy_config cfg{};
    Precision prec = PREC_F16;
    std::string err;
    bool loaded = false;
    Plan plan;
    std::vector<std::string> names;
    std::vector<DevConv> dconv;
    DevOwner weights, buffers, aug_mem, counter_mem;   // what `dconv` views / workspaces and stage buffers / augment buffers / `counters`
    // workspace
    char* ws = nullptr; size_t ws_bytes = 0;           // activations
    // second workspace + stream: cy_detect_tiles runs batches of 64..239 tiles as two concurrent half-batches (forward_split)
    char* ws2 = nullptr; size_t ws2_bytes = 0; hipStream_t s_fwd2 = nullptr; hipEvent_t ev_split[2] = {nullptr, nullptr};
    char* ws3 = nullptr; size_t ws3_bytes = 0; hipStream_t s_small = nullptr;     // small-batch lane: its own workspace and (lowest-priority) stream
    int* box_scr[3] = {nullptr, nullptr, nullptr};      // per workspace (ws, ws2, ws3): slot maps, work lists and counts of the deferred box branch (box_scratch)
    std::vector<size_t> toff; std::vector<size_t> tbytes;   // per tensor, for the last forward geometry
    int lastB = 0, lastH = 0, lastW = 0;
    // stage buffers (sized at load for max_batch), two sets: cy_detect_tiles software-pipelines consecutive batches
    // (preprocessing of batch i+1 and post-processing of batch i-1 run on side streams beside the forward of batch i)
    struct StageBufs {
        void* netin = nullptr; float* pred = nullptr;
        float* cand = nullptr; int* cand_anchor = nullptr; int* cand_count = nullptr; uint64_t* keys = nullptr;
        float* det = nullptr; int* det_anchor = nullptr; int* det_count = nullptr; int* merge_err = nullptr; int* out_src = nullptr;
        double* pre_params = nullptr; double* pre_histeq = nullptr; double* pre_scratch = nullptr;
    } sb[3];                                            // [0], [1]: alternating sets of the batch pipeline; [2]: small batches (side forward stream)
    int slot = 0;                                       // buffer set used by the stage entry points
    StageBufs& S() { return sb[slot]; }
    // test-time augmentation (cy_enable_augment): per buffer set the inputs / head outputs of views 1 and 2, the fp32 letterboxed
    // source of the fp16 context (its view 0 is fp16), and candidate buffers sized for the concatenated anchors of the three views
    struct AugBufs {
        void* view[2] = {nullptr, nullptr}; float* pred[2] = {nullptr, nullptr}; float* src32 = nullptr;
        float* cand = nullptr; int* cand_anchor = nullptr; uint64_t* keys = nullptr;
    } ab[3];
    bool aug = false;
    int acap = 0, acap_pow2 = 0;
    AugBufs& AB() { return ab[slot]; }
    size_t pre_scratch_elems = 0;
    int cap = 0, cap_pow2 = 0;
    hipStream_t s_pre = nullptr, s_post = nullptr;      // side streams of the pipelined cy_detect_tiles
    hipEvent_t ev_call = nullptr, ev_pre[3] = {nullptr, nullptr, nullptr}, ev_fwd[3] = {nullptr, nullptr, nullptr}, ev_post[3] = {nullptr, nullptr, nullptr};
    unsigned long batches = 0;                          // cy_detect_tiles calls on the main pipeline since load / flush
    unsigned long small_batches = 0;                    // ... and on the small-batch lane (buffer set 2, forward on s_fwd2)
    bool mosaic_dirty = true;                           // cy_mosaic_prepare / cy_detect_fence ran on the caller's stream since the last cy_detect_tiles
    const void* seen_mosaic[16] = {nullptr}; int n_seen = 0;   // mosaic buffers already ordered behind the caller's stream in this pipeline
    int* counters = nullptr;                            // device: [0] degenerate boxes dropped by the IoU merge, [1] tiles whose candidates overflowed `cap`
    double step_ms[STEP_COUNT] = {-1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0};   // kernel time of the last launch of each measurement step (cy_*_kernel_ms)
    // optional per-launch timing of the forward ops (hipEvents on the caller's stream)
    bool profiling = false;
    bool split_last = false;                             // the last forward ran as two half-batches (debug reads see only one)
    std::vector<char> fused_last;                        // per plan op, of the last forward: it ran as the first of a fused launch (Op::fuse says which): its
                                                         // output was not materialised, and the op behind it ran inside that launch
    int stop_after = 0;                                  // cy_debug_stop_after: cy_forward ends after this many plan ops (<= 0: the whole plan)
    int ops_done = 0;                                    // plan ops the last cy_forward completed (a fused launch counts both of its ops)
    int prof_stride = 1; unsigned long fwd_calls = 0;   // profiling on: every prof_stride-th cy_forward call is timed
    std::vector<hipEvent_t> ev_pool; size_t ev_used = 0;
    struct ProfRec { size_t e0, e1; int kind; double flops; int conv; int lane; };    // lane: 0 main stream(s), 1 small-batch lane
    std::vector<ProfRec> prof;
};

namespace {
thread_local std::string g_err;
int fail(cy_ctx* c, int code, const std::string& m) { if (c) c->err = m; g_err = m; return code; }
#define HIPCHK(c, x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(c, CY_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline size_t esize(Precision p) { return p == PREC_F16 ? 2 : 4; }      // bytes per activation value (fp16x3: two fp16 halves)
inline Precision io_prec(Precision p) { return p == PREC_F16X3 ? PREC_F32 : p; }   // type of the network input buffer
// candidate capacity per tile: n (<= CY_MAX_CAND) rounded up to 64, kept within the 16-bit slot field of the NMS sort key
inline int cand_capacity(int n) { const int r = (n + 63) / 64 * 64; return r > CY_MAX_CAND ? CY_MAX_CAND : r; }
// depth-wise 3x3 filter [C][1][3][3] -> the [9][C] fp32 layout of dwconv3x3_kernel (weight loader, test entry cy_dwconv3x3)
std::vector<float> dw_weights(const float* W, int C) {
    std::vector<float> dw(9 * (size_t)C);
    for (int ch = 0; ch < C; ++ch) for (int t = 0; t < 9; ++t) dw[(size_t)t * C + ch] = W[(size_t)ch * 9 + t];
    return dw;
}
const char* const ATTN_TOO_LARGE = "attention map too large for this kernel (stride-32 map of the input must have <= 10240 pixels)";

// synchronise, then report the first error of the call (as cy_conv_bn_silu)
int entry_done(cy_ctx* c, hipError_t e, hipStream_t s) {
    const hipError_t e2 = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(c, CY_ERR_HIP, hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(c, CY_ERR_HIP, hipGetErrorString(e2));
    return CY_OK;
}
const char* const IMAGE_TOO_LARGE = "image of 2^31 pixels or more (32-bit pixel counts per window)";

// One kernel launch of a measurement entry between two events on the caller's stream.  The entry names its device buffers in
// the order it wants them allocated (upload / zeros / scratch) and its copies back (download), then calls run(): copies and memsets
// are queued before the first event and the copies back after the second, so that the events enclose the kernel alone; run()
// synchronises, stores the elapsed time as the step's kernel time (-1 when anything queued failed) and reports the call's first error.
// A failure before anything is queued (device, allocation, first event) is reported with the failing call's name in front, without
// a synchronise, and leaves the stored time as it was.
struct TimedLaunch {
    struct Copy { void* dst; const void* src; size_t bytes; };      // src null: zero dst
    cy_ctx* c; hipStream_t st; hipError_t e;
    const char* early = nullptr;                                     // the call that failed before anything was queued
    DevOwner sc;
    std::vector<Copy> before, after;
    TimedLaunch(cy_ctx* c_, void* stream) : c(c_), st((hipStream_t)stream), e(hipSetDevice(c_->device)) {
        if (e != hipSuccess) early = "hipSetDevice(c->device)";
    }
    template <class T> T* scratch(size_t count) {
        void* d = nullptr;
        if (e == hipSuccess && (e = sc.alloc(std::max<size_t>(count, 1) * sizeof(T), &d)) != hipSuccess) early = "sc.alloc(bytes, &d)";      // an empty table still gets a buffer
        return reinterpret_cast<T*>(d);
    }
    template <class T> T* upload(const T* src, size_t count) {
        T* d = scratch<T>(count);
        if (count) before.push_back(Copy{d, src, count * sizeof(T)});
        return d;
    }
    template <class T> T* zeros(size_t count) {
        T* d = scratch<T>(count);
        before.push_back(Copy{d, nullptr, count * sizeof(T)});
        return d;
    }
    template <class T> void download(T* host, const T* dev, size_t count) { after.push_back(Copy{host, dev, count * sizeof(T)}); }
    template <class Launch> int run(MeasureStep step, Launch&& launch) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (e == hipSuccess && (e = hipEventCreate(&e0)) != hipSuccess) early = "hipEventCreate(&e0)";
        if (early) return fail(c, CY_ERR_HIP, std::string(early) + ": " + hipGetErrorString(e));
        e = hipEventCreate(&e1);
        for (const Copy& q : before)
            if (e == hipSuccess) e = q.src ? hipMemcpyAsync(q.dst, q.src, q.bytes, hipMemcpyHostToDevice, st) : hipMemsetAsync(q.dst, 0, q.bytes, st);
        if (e == hipSuccess) e = hipEventRecord(e0, st);
        if (e == hipSuccess) e = launch(st);
        if (e == hipSuccess) e = hipEventRecord(e1, st);
        for (const Copy& q : after)
            if (e == hipSuccess) e = hipMemcpyAsync(q.dst, q.src, q.bytes, hipMemcpyDeviceToHost, st);
        const int rc = entry_done(c, e, st);
        float ms = -1.0f;
        if (rc == CY_OK && hipEventElapsedTime(&ms, e0, e1) != hipSuccess) ms = -1.0f;
        c->step_ms[step] = ms;
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        return rc;
    }
};
inline bool ch8(int v) { return v >= 0 && v % 8 == 0; }     // channel offset / stride usable by the 8-channel vector accesses

void free_all(cy_ctx* c) {
    for (auto e : c->ev_pool) hipEventDestroy(e);
    c->ev_pool.clear(); c->ev_used = 0; c->prof.clear();
    c->dconv.clear();
    c->weights.reset(); c->buffers.reset(); c->aug_mem.reset(); c->counter_mem.reset();
    c->ws = c->ws2 = c->ws3 = nullptr; c->ws2_bytes = c->ws3_bytes = 0; c->counters = nullptr;
    c->box_scr[0] = c->box_scr[1] = c->box_scr[2] = nullptr;
    for (auto& b : c->sb) b = cy_ctx::StageBufs();
    for (auto& b : c->ab) b = cy_ctx::AugBufs();
    if (c->s_fwd2) { hipStreamDestroy(c->s_fwd2); c->s_fwd2 = nullptr; }
    c->s_small = nullptr;                                   // (an alias of s_fwd2)
    if (c->s_pre) { hipStreamDestroy(c->s_pre); c->s_pre = nullptr; }
    if (c->s_post) { hipStreamDestroy(c->s_post); c->s_post = nullptr; }
    hipEvent_t* evs[] = {&c->ev_split[0], &c->ev_split[1], &c->ev_call, &c->ev_pre[0], &c->ev_pre[1], &c->ev_pre[2], &c->ev_fwd[0], &c->ev_fwd[1],
                         &c->ev_fwd[2], &c->ev_post[0], &c->ev_post[1], &c->ev_post[2]};
    for (hipEvent_t* e : evs) if (*e) { hipEventDestroy(*e); *e = nullptr; }
    c->batches = 0; c->small_batches = 0;
    c->loaded = false; c->aug = false; c->acap = 0; c->acap_pow2 = 0; c->lastB = 0;
}

// bias[cout] -> device, zero-padded to a multiple of 128 channels (the kernels read whole tiles of it)
hipError_t upload_bias(DevOwner& own, const float* b, int co, float** out) {
    std::vector<float> bias((co + 127) / 128 * 128, 0.0f);
    memcpy(bias.data(), b, 4 * (size_t)co);
    return own.upload(bias.data(), 4 * bias.size(), out);
}

// The device copies of one dense convolution (weight loader and cy_conv_bn_silu): bias, the packed main panel, and the second copy
// with 64-byte K chunks for the kernels that read that form (conv3x3_wide_kernel / conv3x3_c64_kernel<32>); in the fp16x3 context
// also the pass count and the per-channel output scale.  down_copy: the 3x3 s2 64 -> 128 layer gets the second copy too
// (stem_down_kernel reads its weight fragments from it, and conv_choose looks at wgt32: the loader asks for it, the test entry not).
// Which layers get the second copy: conv_second_copy (cy_conv_plan.cpp), beside the variant conditions that rely on it.
hipError_t upload_conv(DevOwner& own, Precision prec, const float* W, const float* b, const float* wscale, int co, int ci, int k, int s,
                       bool down_copy, DevConv& dc) {
    hipError_t e = upload_bias(own, b, co, &dc.bias);
    if (e != hipSuccess) return e;
    const bool x3 = prec == PREC_F16X3;
    std::vector<float> osc((co + 127) / 128 * 128);
    std::vector<char> packed;
    // two passes when the filter is exactly an fp16 filter times a per-channel scale (CY_X3_PASSES=3 forces the general form)
    if (x3) dc.passes = env_knob("CY_X3_PASSES", 0) == 3 ? 3 : x3_passes(W, co, ci, k, wscale);
    auto panel = [&](int chunk, void** dst, size_t* bytes) {
        *bytes = x3 ? packed_weight_bytes_x3(co, ci, k, chunk, dc.passes) : packed_weight_bytes(prec, co, ci, k, chunk);
        packed.resize(*bytes);
        if (x3) pack_weights_x3(W, co, ci, k, packed.data(), osc.data(), chunk, dc.passes, wscale);
        else pack_weights(prec, W, co, ci, k, packed.data(), chunk);
        return own.upload(packed.data(), *bytes, dst);
    };
    e = panel(128, &dc.w, &dc.wbytes);
    if (e == hipSuccess && x3) e = own.upload(osc.data(), 4 * osc.size(), &dc.oscale);
    if (e == hipSuccess && conv_second_copy(prec, ci, co, k, s, down_copy)) e = panel(64, &dc.w32, &dc.w32bytes);
    return e;
}

// Everything of a load behind the header, on a freed context: the conv records one by one (host checks in cy_plan.cpp, then the
// device copies), the plan's checks, the extra weight forms of the marked pairs, workspace, stage buffers, streams and events.
int build_model(cy_ctx* c, Reader& r, const FileHeader& h, Plan& plan) {
    c->dconv.resize(h.nconv);
    std::vector<const float*> Wsrc(h.nconv, nullptr);        // folded fp32 weights inside the file (for the pairs' packing below)
    int stem_conv = -1;
    for (auto& o : plan.ops) if (o.kind == OPK_STEM) stem_conv = o.conv;
    for (uint32_t i = 0; i < h.nconv; ++i) {
        ConvRecord rec;
        const std::string msg = next_conv(r, h, &plan, i, &rec);
        if (!msg.empty()) return fail(c, CY_ERR_IO, msg);
        const ConvDesc& d = rec.d;
        const float* W = rec.W;
        Wsrc[i] = W;
        DevConv& dc = c->dconv[i];
        if (d.groups > 1) {   // depth-wise 3x3 (YOLO11): [9][C] fp32 for dwconv3x3_kernel
            if (d.groups != d.cin || d.cout != d.cin || d.k != 3 || d.s != 1 || d.cout % 8) return fail(c, CY_ERR_UNSUPPORTED, "only depth-wise 3x3 stride-1 grouped convs are supported: " + d.name);
            HIPCHK(c, upload_bias(c->weights, rec.b, d.cout, &dc.bias));
            const std::vector<float> dw = dw_weights(W, d.cout);
            HIPCHK(c, c->weights.upload(dw.data(), 4 * dw.size(), &dc.dw_w));
            continue;
        }
        if ((int)i == stem_conv) {   // stem: [27][Cout] fp32, t = (kh*3+kw)*3 + c over the 3 network input channels
            if (d.cout > 64 || d.cout % 16) return fail(c, CY_ERR_UNSUPPORTED, "stem width not supported by the gfx950 stem kernel");
            HIPCHK(c, upload_bias(c->weights, rec.b, d.cout, &dc.bias));
            const int co = d.cout;
            std::vector<float> sw(27 * (size_t)co);
            for (int o = 0; o < co; ++o) for (int cch = 0; cch < 3; ++cch) for (int t = 0; t < 9; ++t)
                sw[(size_t)(t * 3 + cch) * co + o] = W[((size_t)o * 3 + cch) * 9 + t];
            HIPCHK(c, c->weights.upload(sw.data(), 4 * sw.size(), &dc.stem_w));
            if (c->prec == PREC_F16 && co == 64) {
                std::vector<char> pk(64 * 32 * 2 + 64 * 64 * 2);          // panel of stem_mfma_kernel, then the one of stem_down_kernel
                pack_stem_weights(W, co, pk.data());
                pack_stem_weights2(W, co, pk.data() + 64 * 32 * 2);
                HIPCHK(c, c->weights.upload(pk.data(), pk.size(), &dc.w));
            }
            continue;
        }
        if (d.cin % 8) return fail(c, CY_ERR_UNSUPPORTED, "conv input channels must be a multiple of 8: " + d.name);
        HIPCHK(c, upload_conv(c->weights, c->prec, W, rec.b, rec.wscale, d.cout, d.cin, d.k, d.s, true, dc));
    }
    if (h.v2) {
        const std::string bad = validate_plan(plan);
        if (!bad.empty()) return fail(c, CY_ERR_IO, bad);
    }
    mark_fusions(plan);
    if (c->prec == PREC_F16) {
        for (size_t i = 0; i < plan.ops.size(); ++i) {          // back-to-back pairs: the second layer's weights in accumulator order
            if (plan.ops[i].fuse != FUSE_PW_PAIR) continue;
            const int c2 = plan.ops[i + 1].conv;
            const ConvDesc& d2 = plan.convs[c2];
            DevConv& dc2 = c->dconv[c2];
            dc2.w2fbytes = packed_weight_bytes(PREC_F16, d2.cout, d2.cin, 1);
            std::vector<char> pk(dc2.w2fbytes);
            pack_weights_fused2(Wsrc[c2], d2.cout, d2.cin, pk.data());
            HIPCHK(c, c->weights.upload(pk.data(), pk.size(), &dc2.w2f));
        }
        std::vector<char> wf(BNECK_WFRAG_BYTES);
        for (size_t i = 0; i < plan.ops.size(); ++i) {
            if (plan.ops[i].fuse != FUSE_BNECK_PAIR) continue;
            const int c1 = plan.ops[i].conv, c2 = plan.ops[i + 1].conv;
            pack_bneck_weights(Wsrc[c1], Wsrc[c2], wf.data());
            HIPCHK(c, c->weights.upload(wf.data(), wf.size(), &c->dconv[c1].bneck));
        }
    }
    c->plan = plan; c->names = h.names;
    // ---- workspace for (max_batch, max_h, max_w)
    const cy_config& g = c->cfg;
    const size_t es = esize(c->prec), nc = (size_t)plan.nc;
    size_t act = 0;
    for (auto& t : plan.tensors) act += align_up((size_t)g.max_batch * (g.max_h >> t.level) * (g.max_w >> t.level) * t.C * es, 256);
    c->ws_bytes = act;
    HIPCHK(c, c->buffers.alloc(c->ws_bytes, &c->ws));
    const int A = cy_num_anchors(g.max_h, g.max_w);
    // candidates per tile: cap >= the anchor count of the largest letterboxed tile, so an overflow cannot happen; nms_kernel
    // sorts them all and keeps ultralytics' top max_nms = 30000 by score.  An explicit max_cand is honoured, and a tile that
    // overflows it is counted (cy_detect_counters) -- its surplus candidates are dropped in arrival order.  cy_create has
    // checked both against CY_MAX_CAND (the 16-bit fields of the NMS sort key).
    c->cap = cand_capacity(g.max_cand > 0 ? g.max_cand : A);
    c->cap_pow2 = 1; while (c->cap_pow2 < c->cap) c->cap_pow2 <<= 1;
    const size_t Bm = g.max_batch;
    c->pre_scratch_elems = Bm * 3 * (size_t)g.max_h * g.max_w;
    DevOwner& own = c->buffers;
    for (auto& b : c->sb) {
        HIPCHK(c, own.alloc(Bm * g.max_h * g.max_w * 4 * es, &b.netin));
        HIPCHK(c, own.alloc(Bm * A * (64 + nc) * sizeof(float), &b.pred));
        HIPCHK(c, own.alloc(Bm * c->cap * 6 * sizeof(float), &b.cand));
        HIPCHK(c, own.alloc(Bm * c->cap * sizeof(int), &b.cand_anchor));
        HIPCHK(c, own.alloc(Bm * sizeof(int), &b.cand_count));
        HIPCHK(c, own.alloc(Bm * c->cap_pow2 * sizeof(uint64_t), &b.keys));
        HIPCHK(c, own.alloc(Bm * CY_MAX_DET * 6 * sizeof(float), &b.det));
        HIPCHK(c, own.alloc(Bm * CY_MAX_DET * sizeof(int), &b.det_anchor));
        HIPCHK(c, own.alloc(Bm * sizeof(int), &b.det_count));
        HIPCHK(c, own.alloc(Bm * sizeof(int), &b.merge_err));
        HIPCHK(c, own.alloc(Bm * CY_MAX_DET * sizeof(int), &b.out_src));
        HIPCHK(c, own.alloc(Bm * 3 * CY_MAX_STAGES * 4 * sizeof(double), &b.pre_params));
        HIPCHK(c, own.alloc(Bm * 3 * 520 * sizeof(double), &b.pre_histeq));
        HIPCHK(c, own.alloc(c->pre_scratch_elems * sizeof(double), &b.pre_scratch));
    }
    HIPCHK(c, c->counter_mem.alloc(4 * sizeof(int), &c->counters));
    HIPCHK(c, hipMemset(c->counters, 0, 4 * sizeof(int)));
    // side streams at the LOWEST priority: preprocessing and decode/NMS/merge fill the gaps of the conv stack on the caller's
    // stream instead of competing with it for CUs.  Round 4: confining them to a
    // subset of the CUs instead (hipExtStreamCreateWithCUMask, 64 / 32 / 16 CUs spread over the XCDs) costs 10-12 % of the S16k rate
    // (8950 -> 8000 / 8000 / 7910 tiles/s): the pass then waits for its side kernels.
    int prio_lo = 0, prio_hi = 0;
    hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);          // lo = numerically greatest = lowest priority
    HIPCHK(c, hipStreamCreateWithPriority(&c->s_pre, hipStreamNonBlocking, prio_lo));
    HIPCHK(c, hipStreamCreateWithPriority(&c->s_post, hipStreamNonBlocking, prio_lo));
    hipEvent_t* evs[] = {&c->ev_call, &c->ev_pre[0], &c->ev_pre[1], &c->ev_pre[2], &c->ev_fwd[0], &c->ev_fwd[1], &c->ev_fwd[2], &c->ev_post[0], &c->ev_post[1], &c->ev_post[2]};
    for (hipEvent_t* e : evs) HIPCHK(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    c->loaded = true;
    return CY_OK;
}

// Order of a load: what the header and plan section allow to be checked is checked BEFORE the old model is freed (a refused header
// leaves the context as it was); then the old model goes first, so that the peak is one model and not two; then the new one is
// built.  Any failure behind the free leaves the context freed and unloaded: every entry that needs a model refuses it, and a
// later load of a sound file on the same context works.
int upload_weights(cy_ctx* c, const void* buf, size_t nbytes) {
    Reader r{(const unsigned char*)buf, nbytes};
    Plan plan;
    FileHeader h;
    const std::string msg = parse_header(r, &plan, &h);
    if (!msg.empty()) return fail(c, h.unsupported ? CY_ERR_UNSUPPORTED : CY_ERR_IO, msg);
    HIPCHK(c, hipSetDevice(c->device));
    free_all(c);
    const int rc = build_model(c, r, h, plan);
    if (rc) free_all(c);
    return rc;
}

int layout_tensors(cy_ctx* c, int B, int H, int W, size_t capacity) {
    const size_t es = esize(c->prec);
    c->toff.assign(c->plan.tensors.size(), 0);
    c->tbytes.assign(c->plan.tensors.size(), 0);
    size_t off = 0;
    for (size_t i = 0; i < c->plan.tensors.size(); ++i) {
        const Tensor& t = c->plan.tensors[i];
        const size_t b = (size_t)B * (H >> t.level) * (W >> t.level) * t.C * es;
        c->toff[i] = off; c->tbytes[i] = b;
        off += align_up(b, 256);
        if (b >= 0xFFFFFF00ull) return fail(c, CY_ERR_ARG, "a tensor exceeds the 4 GiB buffer-addressing limit; lower the batch");
    }
    if (off > capacity) return fail(c, CY_ERR_ARG, "batch/shape exceeds the workspace sized at cy_create");
    c->lastB = B; c->lastH = H; c->lastW = W;
    return CY_OK;
}
}  // namespace

extern "C" {

int cy_create(int device, const cy_config* cfg, cy_ctx** out) {
    if (!cfg || !out) return fail(nullptr, CY_ERR_ARG, "null argument");
    if (cfg->max_batch < 1 || cfg->max_h < 32 || cfg->max_w < 32 || cfg->max_h % 32 || cfg->max_w % 32)
        return fail(nullptr, CY_ERR_ARG, "max_batch >= 1 and max_h/max_w multiples of 32 required");
    if (cfg->precision != CY_F16 && cfg->precision != CY_F32 && cfg->precision != CY_F16X3) return fail(nullptr, CY_ERR_ARG, "bad precision");
    const int A = cy_num_anchors(cfg->max_h, cfg->max_w);
    if (A > CY_MAX_CAND)
        return fail(nullptr, CY_ERR_ARG, "max_h x max_w = " + std::to_string(cfg->max_h) + " x " + std::to_string(cfg->max_w) + ": " +
                                             std::to_string(A) + " anchors, more than CY_MAX_CAND = " + std::to_string(CY_MAX_CAND) +
                                             " (16-bit anchor field of the NMS sort key)");
    if (cfg->max_cand > CY_MAX_CAND)
        return fail(nullptr, CY_ERR_ARG, "max_cand " + std::to_string(cfg->max_cand) + " exceeds CY_MAX_CAND = " + std::to_string(CY_MAX_CAND) +
                                             " (16-bit slot field of the NMS sort key)");
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || device < 0 || device >= n)
        return fail(nullptr, CY_ERR_HIP, std::string("no such HIP device (this library has no CPU fallback): hipGetDeviceCount -> ") +
                                             hipGetErrorString(e) + ", " + std::to_string(n) + " device(s), requested " + std::to_string(device));
    cy_ctx* c = new cy_ctx();
    c->device = device; c->cfg = *cfg; c->prec = cfg->precision == CY_F16 ? PREC_F16 : (cfg->precision == CY_F16X3 ? PREC_F16X3 : PREC_F32);
    *out = c;
    return CY_OK;
}

int cy_destroy(cy_ctx* c) {
    if (!c) return CY_OK;
    hipSetDevice(c->device);
    free_all(c);
    delete c;
    return CY_OK;
}

const char* cy_last_error(const cy_ctx* c) { return c ? c->err.c_str() : g_err.c_str(); }

int cy_load_weights_mem(cy_ctx* c, const void* buf, size_t nbytes) {
    if (!c || !buf) return fail(c, CY_ERR_ARG, "null argument");
    return upload_weights(c, buf, nbytes);
}

int cy_load_weights(cy_ctx* c, const char* path) {
    if (!c || !path) return fail(c, CY_ERR_ARG, "null argument");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(c, CY_ERR_IO, std::string("cannot open ") + path);
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<char> buf(n);
    const size_t got = fread(buf.data(), 1, n, f);
    fclose(f);
    if ((long)got != n) return fail(c, CY_ERR_IO, "short read");
    return upload_weights(c, buf.data(), buf.size());
}

int cy_num_classes(const cy_ctx* c) { return c && c->loaded ? c->plan.nc : -1; }
int cy_weight_passes(const cy_ctx* c, int* out2) {
    if (!c || !c->loaded || !out2) return CY_ERR_ARG;
    out2[0] = out2[1] = 0;
    if (c->prec == PREC_F16X3)
        for (const auto& d : c->dconv) if (d.oscale) out2[d.passes == 2 ? 0 : 1] += 1;
    return CY_OK;
}
const char* cy_class_name(const cy_ctx* c, int i) {
    if (!c || !c->loaded || i < 0 || i >= (int)c->names.size()) return nullptr;
    return c->names[i].c_str();
}

int cy_plan_num_convs(char scale, int nc) { Plan p = build_plan(scale, nc); return p.ok ? (int)p.convs.size() : CY_ERR_ARG; }
int cy_plan_conv_desc(char scale, int nc, int idx, cy_conv_desc* out) {
    Plan p = build_plan(scale, nc);
    if (!p.ok || !out || idx < 0 || idx >= (int)p.convs.size()) return CY_ERR_ARG;
    const ConvDesc& d = p.convs[idx];
    memset(out, 0, sizeof(*out));
    strncpy(out->name, d.name.c_str(), sizeof(out->name) - 1);
    out->cin = d.cin; out->cout = d.cout; out->k = d.k; out->s = d.s; out->act = d.act;
    return CY_OK;
}

int cy_letterbox_geometry(int h0, int w0, int imgsz, cy_letterbox* o) {
    // ultralytics LetterBox(auto=True, scaleup=True, center=True, stride=32): SURVEY.md Appendix A.1 step 2
    if (!o || h0 < 1 || w0 < 1 || imgsz < 32) return CY_ERR_ARG;
    const double r = std::fmin((double)imgsz / h0, (double)imgsz / w0);
    o->new_w = py_round(w0 * r); o->new_h = py_round(h0 * r);
    double dw = (imgsz - o->new_w) % 32, dh = (imgsz - o->new_h) % 32;
    if (dw < 0) dw += 32;
    if (dh < 0) dh += 32;
    dw /= 2; dh /= 2;
    o->top = py_round(dh - 0.1); o->left = py_round(dw - 0.1);
    const int bottom = py_round(dh + 0.1), right = py_round(dw + 0.1);
    o->H = o->new_h + o->top + bottom; o->W = o->new_w + o->left + right;
    return CY_OK;
}

int cy_num_anchors(int H, int W) { int n = 0; for (int s = 8; s <= 32; s *= 2) n += ((H + s - 1) / s) * ((W + s - 1) / s); return n; }
size_t cy_pred_elems(const cy_ctx* c, int B, int H, int W) {
    return c && c->loaded ? (size_t)B * cy_num_anchors(H, W) * (64 + c->plan.nc) : 0;
}

int cy_mosaic_prepare(cy_ctx* c, float* d_data, size_t n, int big_endian, void* stream) {
    if (!c || !d_data) return fail(c, CY_ERR_ARG, "null argument");
    HIPCHK(c, launch_mosaic_prepare(d_data, n, big_endian, (hipStream_t)stream));
    c->mosaic_dirty = true;
    return CY_OK;
}

// A request to compute the box branch of the detect head at candidate anchors only (forward_on): the confidence threshold of the
// decode that will read the rows; sparse[l] is set to whether level l was deferred (else it ran dense).
struct BoxReq { float conf; int sparse[3]; int force = 0; };      // force: as CY_SPARSE_BOX=2 (test entry)
// The lowest confidence threshold from which on the deferred form is taken by default: with every anchor a candidate the gather
// kernels do the dense pixel count at lower efficiency.  Measured on the benchmark's tiles (profiles/sparse_box.md).
constexpr float BOX_CONF_FLOOR = 0.25f;

static int forward_on(cy_ctx* c, const void* d_netin, int B, int H, int W, float* d_pred, hipStream_t s, char* ws, size_t ws_cap,
                      bool may_profile, int stop = 0, BoxReq* box = nullptr);

// slot maps [B * A], the two work lists [B * A each] and the counts [8] of a pass on workspace `ws`, allocated on first use for the
// context's largest batch; *out stays null when this pass holds more anchors than that (the pass then runs dense)
static int box_scratch(cy_ctx* c, const char* ws, size_t tot, int** out) {
    const size_t max_tot = (size_t)c->cfg.max_batch * cy_num_anchors(c->cfg.max_h, c->cfg.max_w);
    *out = nullptr;
    if (tot > max_tot) return CY_OK;
    const int k = ws == c->ws ? 0 : (ws == c->ws2 ? 1 : 2);
    if (!c->box_scr[k]) HIPCHK(c, c->buffers.alloc((3 * max_tot + 8) * sizeof(int), &c->box_scr[k]));
    *out = c->box_scr[k];
    return CY_OK;
}

int cy_forward(cy_ctx* c, const void* d_netin, int B, int H, int W, float* d_pred, void* stream) {
    if (!c || !c->loaded) return fail(c, CY_ERR_STATE, "weights not loaded");
    c->split_last = false;
    return forward_on(c, d_netin, B, H, W, d_pred, (hipStream_t)stream, c->ws, c->ws_bytes, true, c->stop_after);
}

// The forward of one batch as TWO half-batches on two streams (own workspace each).  Every layer is one kernel launch
// whose last round of workgroups leaves part of the chip idle, and kernels of one stream cannot overlap: the other half's
// kernels fill those tails.  Measured on MI355X (tools/concurrent_forward.py, forward only): -6.8 % at 208 tiles, -3.7 % at
// 224, -1.3 % at 254.  Used for 64..239 tiles (the per-rank shares at N >= 2); a full batch stays on one stream, so that the
// per-launch event timing of bench.py at N = 1 means exclusive use of the GPU.  CY_DUAL_FORWARD: 0 off, 2 from 2 tiles on.
// ONE extra forward stream serves both the second half of a split batch and the small-batch lane.  With a stream of its own per
// role a context had five streams (caller's, preprocessing, post-processing, split, small lane) and the HIP runtime maps streams
// onto FOUR hardware queues: whichever two shared a queue serialised -- measured as a per-rank pass of 41.6 instead of 24.6 ms when
// one process used both roles (a rank of the N = 2 / 4 partitions: full batches of 64..239 tiles AND ragged classes; order of
// stream creation decided which pair collided).  A small batch now queues behind the second half of a split batch when both are
// in flight; at N = 1 (no split batches) and N = 8 (a rank has either kind) nothing changes.
static int ensure_side_forward_stream(cy_ctx* c) {
    if (c->s_fwd2) return CY_OK;
    HIPCHK(c, hipStreamCreateWithFlags(&c->s_fwd2, hipStreamNonBlocking));
    return CY_OK;
}
static int ensure_second_workspace(cy_ctx* c) {
    if (c->ws2) return CY_OK;
    c->ws2_bytes = c->ws_bytes / 2 + (1u << 20);            // the second half is never the larger one
    HIPCHK(c, c->buffers.alloc(c->ws2_bytes, &c->ws2));
    int rc = ensure_side_forward_stream(c);
    if (rc) return rc;
    for (auto& ev : c->ev_split) HIPCHK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return CY_OK;
}
// The small-batch lane (cy_detect_tiles): small batches run their forward on the side forward stream with a workspace of their
// own, so that their ~105 launches of a few workgroups each take what the full batch beside them leaves free.
static int ensure_small_lane(cy_ctx* c) {
    if (c->ws3) return CY_OK;
    c->ws3_bytes = c->ws_bytes / 3 + (1u << 20);            // a small batch holds at most max_batch / 3 tiles
    HIPCHK(c, c->buffers.alloc(c->ws3_bytes, &c->ws3));
    int rc = ensure_side_forward_stream(c);
    if (rc) return rc;
    c->s_small = c->s_fwd2;                                 // (shared: see ensure_side_forward_stream)
    return CY_OK;
}
static int dual_mode() { return env_knob("CY_DUAL_FORWARD", 1); }

static int forward_split(cy_ctx* c, const void* d_netin, int B, int H, int W, float* d_pred, hipStream_t sm, BoxReq* box = nullptr) {
    const int mode = dual_mode();
    const bool split = c->prec == PREC_F16 && mode != 0 && B >= 2 && (mode > 1 || (B >= 64 && B < 240));      // (fp16x3: a 128-tile batch already fills the chip 3x longer per launch)
    c->split_last = split;
    if (!split) return forward_on(c, d_netin, B, H, W, d_pred, sm, c->ws, c->ws_bytes, true, 0, box);
    int rc0 = ensure_second_workspace(c);
    if (rc0) return rc0;
    const int h = B - B / 2;
    const size_t in_half = (size_t)h * H * W * 4 * esize(c->prec);
    const size_t pred_half = (size_t)h * cy_num_anchors(H, W) * (64 + c->plan.nc);
    HIPCHK(c, hipEventRecord(c->ev_split[0], sm));           // everything the forward waits for is already queued on sm
    HIPCHK(c, hipStreamWaitEvent(c->s_fwd2, c->ev_split[0], 0));
    int rc = forward_on(c, d_netin, h, H, W, d_pred, sm, c->ws, c->ws_bytes, true, 0, box);
    if (rc) return rc;
    rc = forward_on(c, (const char*)d_netin + in_half, B - h, H, W, d_pred + pred_half, c->s_fwd2, c->ws2, c->ws2_bytes, false, 0, box);
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->ev_split[1], c->s_fwd2));
    HIPCHK(c, hipStreamWaitEvent(sm, c->ev_split[1], 0));
    return CY_OK;
}

// stop > 0 (cy_debug_stop_after, through cy_forward only): the pass ends once `stop` plan ops have run.  A fused launch whose first
// op lies below `stop` runs whole; a box-branch output convolution still deferred for its head pair is NOT launched (its
// prediction rows stay as the caller left them), so a stopped pass never runs a launch the whole pass would not.
static int forward_on(cy_ctx* c, const void* d_netin, int B, int H, int W, float* d_pred, hipStream_t s, char* ws, size_t ws_cap,
                      bool may_profile, int stop, BoxReq* box) {
    if (!d_netin || !d_pred || B < 1 || H % 32 || W % 32 || H < 32 || W < 32) return fail(c, CY_ERR_ARG, "bad forward arguments");
    int rc = layout_tensors(c, B, H, W, ws_cap);
    if (rc) return rc;
    const Plan& p = c->plan;
    // a stopped pass (test hook) starts from a workspace of NaN bit patterns (0xFFFF / 0xFFFFFFFF), so that an element its ops
    // leave unwritten cannot pass for the value an earlier pass over the same input left there
    if (stop > 0 && (size_t)stop < p.ops.size() && !c->toff.empty())
        HIPCHK(c, hipMemsetAsync(ws, 0xFF, c->toff.back() + c->tbytes.back(), s));
    const size_t es = esize(c->prec);
    const bool x3 = c->prec == PREC_F16X3;
    const int cm = x3 ? 2 : 1;                           // halves per activation value: pixel strides are cm * C, the low halves C behind
    const int A = cy_num_anchors(H, W);
    int a_off[3], acc = 0;
    for (int l = 0; l < 3; ++l) { a_off[l] = acc; acc += (H >> (3 + l)) * (W >> (3 + l)); }
    auto tptr = [&](int t) -> char* { return t == 0 ? (char*)const_cast<void*>(d_netin) : ws + c->toff[t]; };
    auto stamp = [&]() -> size_t {
        if (c->ev_used == c->ev_pool.size()) { hipEvent_t e; hipEventCreate(&e); c->ev_pool.push_back(e); }
        hipEventRecord(c->ev_pool[c->ev_used], s);
        return c->ev_used++;
    };
    const bool prof_now = may_profile && c->profiling && (c->fwd_calls++ % (unsigned long)c->prof_stride) == 0;
    size_t ev_prev = prof_now ? stamp() : 0;
    int cur_conv = -1;
    auto prof_done = [&](int kind, double flops) {
        if (!prof_now) return;
        const size_t e = stamp();
        c->prof.push_back({ev_prev, e, kind, flops, cur_conv, (c->ws3 && ws == c->ws3) ? 1 : 0});
        ev_prev = e;
    };
    // The pairs of ops that one kernel can run carry a mark from the load (Op::fuse, cy_plan.cpp: the shape of the plan); here each
    // mark meets its run-time gate, read per call.
    // model.0 + model.1 in one kernel (fp16 context) when the stem's only reader is a 3x3 s2 64->128 SiLU conv (the widths the loader
    // packed both weight forms for) and the launch fills the chip.  CY_STEM_FUSE: 0 = off, 2 = regardless of size (parity tests).
    const int fuse_env = env_knob("CY_STEM_FUSE", 1);
    c->fused_last.assign(p.ops.size(), 0);
    const int pw_env = env_knob("CY_FUSE_PW", 1);             // back-to-back pairs (pw_pair); read per call: the parity tests run both forms
    const ConvKnobs knobs = conv_knobs_env();                 // the switches of the conv dispatch, likewise: one read for the whole pass

    auto conv_args = [&](const Op& o) -> ConvArgs {           // the launch arguments of a convolution op of this pass
        ConvArgs a = conv_geometry(p, o, B, H, W, cm, A, a_off);      // every non-pointer field
        auto span = [&](int t) -> uint32_t {           // bytes addressable from tptr(t) for B images
            const Tensor& tt = p.tensors[t];
            return (uint32_t)((size_t)B * (H >> tt.level) * (W >> tt.level) * tt.C * es);
        };
        a.in0 = tptr(o.in0); a.in0_bytes = span(o.in0);
        a.split = x3 ? c->dconv[o.conv].passes : 0; a.oscale = c->dconv[o.conv].oscale;
        if (o.in1 >= 0) { a.in1 = tptr(o.in1); a.in1_bytes = span(o.in1); }
        a.wgt = c->dconv[o.conv].w; a.wgt_bytes = (uint32_t)c->dconv[o.conv].wbytes; a.bias = c->dconv[o.conv].bias;
        a.wgt32 = c->dconv[o.conv].w32; a.wgt32_bytes = (uint32_t)c->dconv[o.conv].w32bytes;
        a.out = o.out >= 0 ? tptr(o.out) : (void*)d_pred;
        if (o.res >= 0) a.res = tptr(o.res);
        return a;
    };

    // Deferred box branch (box != null: the plain detect path, cy_detect_tiles, and the test entry cy_debug_sparse_box).  decode_kernel
    // reads an anchor's 64 box logits only when its class scores pass `conf`, so the three marked ops of a level (Op::box) are not
    // launched; behind the pass, on the same stream, the candidates and the pixels they need are listed from the finished class
    // columns and the branch is computed there (cy_sparse_box.hip), bit for bit what the dense kernels write.  A level is taken when
    // its three dense variants are ones the sparse kernels reproduce: by geometry only, so a tile's path does not depend on its batch.
    // CY_SPARSE_BOX (read per call): 0 dense, 1 (default) sparse from conf >= BOX_CONF_FLOOR on, 2 sparse at any conf (tests).
    auto box_level = [&](const Op& o) { return o.box == 3 ? o.pred_level : p.tensors[o.in0].level - 3; };
    bool box_sparse[3] = {false, false, false};
    BoxArgs bx{};
    if (box && c->prec == PREC_F16 && !(stop > 0)) {
        const int mode = box->force ? 2 : env_knob("CY_SPARSE_BOX", 1);
        int* scr = nullptr;
        const size_t tot = (size_t)B * A;                      // list entries / map words of the three levels together
        if (mode >= 2 || (mode == 1 && box->conf >= BOX_CONF_FLOOR)) {
            rc = box_scratch(c, ws, tot, &scr);
            if (rc) return rc;
        }
        if (scr) {
            bx.pred = d_pred; bx.B = B; bx.A = A; bx.nc = p.nc; bx.conf = box->conf;
            for (int l = 0; l < 3; ++l) {
                BoxLevel& L = bx.L[l];
                L.H = H >> (3 + l); L.W = W >> (3 + l); L.a_off = a_off[l]; L.cap = B * L.H * L.W;
                L.map = scr + (size_t)B * a_off[l]; L.plist = L.map + tot; L.clist = L.map + 2 * tot; L.counts = scr + 3 * tot + 2 * l;
            }
            for (size_t i = 0; i + 2 < p.ops.size(); ++i) {
                if (p.ops[i].box != 1) continue;
                const Op& o1 = p.ops[i]; const Op& o2 = p.ops[i + 1]; const Op& o3 = p.ops[i + 2];
                const int l = o3.pred_level;
                const ConvArgs a1 = conv_args(o1), a2 = conv_args(o2), a3 = conv_args(o3);
                const int v1 = conv_choose(c->prec, a1, knobs).variant;
                if (v1 != CONV_WIDE_64 && v1 != CONV_PP_64 && v1 != CONV_C64_PERSIST) continue;
                if (v1 == CONV_C64_PERSIST && a1.Cin != 64) continue;
                if (conv_choose(c->prec, a2, knobs).variant != CONV_C64_PERSIST || a2.Cin != 64 || conv_choose(c->prec, a3, knobs).variant != CONV_HEAD_1X1) continue;
                BoxLevel& L = bx.L[l];
                L.sparse = 1;
                L.feat = a1.in0; L.feat_ct = a1.in0_ct; L.feat_coff = a1.in0_coff; L.cin = a1.Cin; L.feat_bytes = a1.in0_bytes;
                L.walk1 = v1 == CONV_WIDE_64 ? BOX_WALK_WIDE : (v1 == CONV_PP_64 ? BOX_WALK_PP : BOX_WALK_C64);
                L.w1 = v1 == CONV_WIDE_64 ? a1.wgt32 : a1.wgt; L.w1_bytes = v1 == CONV_WIDE_64 ? a1.wgt32_bytes : a1.wgt_bytes; L.b1 = a1.bias;
                L.w2 = a2.wgt; L.w2_bytes = a2.wgt_bytes; L.b2 = a2.bias;
                L.w3 = a3.wgt; L.w3_bytes = a3.wgt_bytes; L.b3 = a3.bias;
                L.s1 = a1.out; L.s2 = a2.out;                  // the branch's own (now unused) tensors: [cap][64] fp16 each
                box_sparse[l] = true;
            }
        }
    }
    if (box) for (int l = 0; l < 3; ++l) box->sparse[l] = box_sparse[l];

    struct HeadPend { ConvArgs a; ConvChoice ch; double flops; int conv; bool on; };
    HeadPend pend[3] = {};                                    // deferred box-branch output convolutions, per stride level
    const int bneck_env = env_knob("CY_BNECK_FUSE", 0);       // off by default (slower than two launches so far, see bneck64.hip); read per call: the parity tests run both forms
    auto run_op = [&](const Op& o, const Op* next, bool* fused) -> int {
        cur_conv = o.conv;
        if (o.box && box_sparse[box_level(o)]) return CY_OK;      // computed at the candidate anchors, behind the pass (below)
        if (bneck_env && c->prec == PREC_F16 && o.fuse == FUSE_BNECK_PAIR && c->dconv[o.conv].bneck) {
            const Op& n = *next;
            const Tensor& ti = p.tensors[o.in0]; const Tensor& to = p.tensors[n.out];
            BneckArgs a{};
            a.in = tptr(o.in0); a.in_ct = ti.C; a.in_coff = o.in0_coff;
            a.B = B; a.H = H >> ti.level; a.W = W >> ti.level;
            a.in_bytes = (uint32_t)((size_t)B * a.H * a.W * ti.C * es);
            a.out = tptr(n.out); a.out_ct = to.C; a.out_coff = n.out_coff;
            a.wfrag = c->dconv[o.conv].bneck; a.bias1 = c->dconv[o.conv].bias; a.bias2 = c->dconv[n.conv].bias;
            a.shortcut = n.res >= 0;
            HIPCHK(c, launch_bneck64(a, s));
            prof_done(CONV_NUM_VARIANTS + 4, 2.0 * (2.0 * B * a.H * a.W * 64.0 * 64.0 * 9.0));
            *fused = true;
            return CY_OK;
        }
        if (o.fuse == FUSE_STEM_DOWN && c->prec == PREC_F16 && fuse_env && c->dconv[o.conv].w && c->dconv[next->conv].w32) {
            const Op& n = *next;
            const Tensor& ti = p.tensors[o.in0]; const Tensor& t1 = p.tensors[o.out]; const Tensor& to = p.tensors[n.out];
            StemDownArgs a{};
            a.B = B; a.Hi = H >> ti.level; a.Wi = W >> ti.level; a.H1 = H >> t1.level; a.W1 = W >> t1.level;
            a.Ho = a.H1 / 2; a.Wo = a.W1 / 2;
            a.in = tptr(o.in0); a.in_bytes = (uint32_t)((size_t)B * a.Hi * a.Wi * ti.C * es);
            a.wpk2 = reinterpret_cast<const char*>(c->dconv[o.conv].w) + 64 * 32 * 2; a.bias0 = c->dconv[o.conv].bias;
            a.wgt32 = c->dconv[n.conv].w32; a.wgt32_bytes = (uint32_t)c->dconv[n.conv].w32bytes; a.bias1 = c->dconv[n.conv].bias;
            a.out = tptr(n.out); a.out_ct = to.C; a.out_coff = n.out_coff;
            if (fuse_env > 1 || knobs.batch_invariant || stem_down_blocks(a) >= 256) {
                HIPCHK(c, launch_stem_down(a, s));
                prof_done(CONV_NUM_VARIANTS, 2.0 * B * a.H1 * a.W1 * 64 * 27.0 + 2.0 * B * a.Ho * a.Wo * 128.0 * 64 * 9);
                *fused = true;
                return CY_OK;
            }
        }
        if (o.kind == OPK_STEM) {
            const Tensor& ti = p.tensors[o.in0]; const Tensor& to = p.tensors[o.out];
            StemArgs a{};
            a.in = tptr(o.in0); a.out = tptr(o.out); a.w = c->dconv[o.conv].stem_w; a.bias = c->dconv[o.conv].bias; a.wpk = c->dconv[o.conv].w;
            a.B = B; a.Hi = H >> ti.level; a.Wi = W >> ti.level; a.Ho = H >> to.level; a.Wo = W >> to.level;
            a.Cout = p.convs[o.conv].cout; a.out_ct = cm * to.C; a.out_coff = o.out_coff; a.out_lo = x3 ? to.C : 0;
            HIPCHK(c, launch_stem(c->prec, a, s));
            prof_done(CONV_NUM_VARIANTS, 2.0 * B * a.Ho * a.Wo * a.Cout * 27.0);
        } else if (o.kind == OPK_POOL) {
            const Tensor& t = p.tensors[o.in0];
            PoolArgs a{};
            a.src = tptr(o.in0); a.dst = tptr(o.out); a.ct = cm * t.C; a.src_coff = o.in0_coff; a.dst_coff = o.out_coff; a.lo = x3 ? t.C : 0;
            a.C = o.c0; a.B = B; a.H = H >> t.level; a.W = W >> t.level;
            HIPCHK(c, launch_pool5(c->prec, a, s));
            prof_done(CONV_NUM_VARIANTS + 1, 0.0);
        } else if (o.kind == OPK_DWCONV) {
            const ConvDesc& d = p.convs[o.conv];
            const Tensor& ti = p.tensors[o.in0]; const Tensor& to = p.tensors[o.out];
            DwArgs a{};
            a.in = tptr(o.in0); a.in_ct = cm * ti.C; a.in_coff = o.in0_coff; a.out = tptr(o.out); a.out_ct = cm * to.C; a.out_coff = o.out_coff;
            a.in_lo = ti.C; a.out_lo = to.C;
            if (o.res >= 0) { a.res = tptr(o.res); a.res_ct = cm * p.tensors[o.res].C; a.res_coff = o.res_coff; a.res_lo = p.tensors[o.res].C; }
            a.w = c->dconv[o.conv].dw_w; a.bias = c->dconv[o.conv].bias;
            a.B = B; a.H = H >> ti.level; a.W = W >> ti.level; a.C = d.cout; a.act = d.act;
            a.blk = o.p0; a.gstride = o.p1; a.goff = o.p2;
            if (!a.w || ti.level != to.level) return fail(c, CY_ERR_STATE, "malformed depth-wise op");
            HIPCHK(c, launch_dwconv(c->prec, a, s));
            prof_done(CONV_NUM_VARIANTS + 2, 2.0 * B * a.H * a.W * (double)a.C * 9.0);
        } else if (o.kind == OPK_ATTN) {
            const Tensor& ti = p.tensors[o.in0]; const Tensor& to = p.tensors[o.out];
            AttnArgs a{};
            a.qkv = tptr(o.in0); a.ct = cm * ti.C; a.coff = o.in0_coff; a.out = tptr(o.out); a.out_ct = cm * to.C; a.out_coff = o.out_coff;
            a.lo = ti.C; a.out_lo = to.C;
            a.B = B; a.N = (H >> ti.level) * (W >> ti.level); a.heads = o.p0; a.kd = o.p1; a.hd = o.p2;
            a.scale = 1.0f / sqrtf((float)a.kd);
            if (a.heads < 1 || ti.level != to.level) return fail(c, CY_ERR_STATE, "malformed attention op");
            hipError_t e = launch_attention(c->prec, a, s);
            if (e == hipErrorInvalidValue) return fail(c, CY_ERR_UNSUPPORTED, ATTN_TOO_LARGE);
            HIPCHK(c, e);
            prof_done(CONV_NUM_VARIANTS + 3, 2.0 * B * a.heads * (double)a.N * a.N * (a.kd + a.hd));
        } else {
            ConvArgs a = conv_args(o);
            double flops = 2.0 * B * a.Ho * a.Wo * (double)a.Cout * a.Cin * a.k * a.k;
            ConvChoice ch = conv_choose(c->prec, a, knobs);        // the op's kernel: decided here, launched and named in the profile from this value
            if (pw_env && c->prec == PREC_F16 && o.fuse == FUSE_PW_PAIR && c->dconv[next->conv].w2f && ch.variant == CONV_DIRECT_256) {
                const Op& n = *next;
                const ConvDesc& d2 = p.convs[n.conv];
                const Tensor& to2 = p.tensors[n.out];
                a.wgt2 = c->dconv[n.conv].w2f; a.wgt2_bytes = (uint32_t)c->dconv[n.conv].w2fbytes; a.bias2 = c->dconv[n.conv].bias;
                a.act2 = d2.act; a.cout2 = d2.cout;
                a.out2 = tptr(n.out); a.out2_ct = to2.C; a.out2_coff = n.out_coff;
                flops += 2.0 * B * a.Ho * a.Wo * (double)d2.cout * d2.cin;
                ch = conv_choose(c->prec, a, knobs);                 // with wgt2 set: the fused-pair instantiation
                *fused = true;
            }
            // the two output convolutions of a detect-head level (box branch at column 0, class branch at column 64 of the same
            // prediction rows) as ONE launch: the box branch's launch is deferred until the class branch's arguments are known
            // (nothing else reads the prediction rows inside the forward pass); CY_HEAD_PAIR=0 / other shapes: one launch each
            if (o.out < 0 && o.pred_coff == 0 && c->prec != PREC_F32 && knobs.head_pair && ch.variant == CONV_HEAD_1X1) {
                HeadPend& h = pend[o.pred_level];
                if (h.on) { cur_conv = h.conv; HIPCHK(c, launch_conv(c->prec, h.ch, h.a, s)); prof_done(h.ch.variant, h.flops); cur_conv = o.conv; }
                h.a = a; h.ch = ch; h.flops = flops; h.conv = o.conv; h.on = true;
                return CY_OK;
            }
            if (o.out < 0 && o.pred_coff == 64 && pend[o.pred_level].on) {
                HeadPend& h = pend[o.pred_level];
                h.on = false;
                if (head_pair_ok(c->prec, h.a, h.ch, a, ch, knobs)) {
                    HIPCHK(c, launch_head_pair(c->prec, h.a, a, s));
                    prof_done(CONV_HEAD_1X1, flops + h.flops);
                    return CY_OK;
                }
                cur_conv = h.conv; HIPCHK(c, launch_conv(c->prec, h.ch, h.a, s)); prof_done(h.ch.variant, h.flops); cur_conv = o.conv;
            }
            HIPCHK(c, launch_conv(c->prec, ch, a, s));
            prof_done(ch.variant, flops);
        }
        return CY_OK;
    };
    const size_t n_run = stop > 0 && (size_t)stop < p.ops.size() ? (size_t)stop : p.ops.size();
    size_t i = 0;
    for (; i < n_run; ++i) {
        bool fused = false;
        rc = run_op(p.ops[i], i + 1 < p.ops.size() ? &p.ops[i + 1] : nullptr, &fused);
        if (rc) return rc;
        if (fused) c->fused_last[i++] = 1;                   // the next op ran inside this one's kernel
    }
    c->ops_done = (int)(i < p.ops.size() ? i : p.ops.size());
    if (n_run < p.ops.size()) return CY_OK;                   // stopped: a deferred box branch stays unlaunched
    for (HeadPend& h : pend)                                  // a box branch whose class branch never came (no such plan today)
        if (h.on) { h.on = false; cur_conv = h.conv; HIPCHK(c, launch_conv(c->prec, h.ch, h.a, s)); prof_done(h.ch.variant, h.flops); }
    if (box_sparse[0] || box_sparse[1] || box_sparse[2]) {
        // the deferred box branches, behind the class columns on the same stream (the next pass on this stream overwrites the feature
        // maps they read): slot maps to -1, counts to 0, then mark and the three stages.  No host read, no synchronisation; untimed in the
        // profile summary.
        HIPCHK(c, hipMemsetAsync(bx.L[0].map, 0xFF, (size_t)B * A * sizeof(int), s));
        HIPCHK(c, hipMemsetAsync(bx.L[0].counts, 0, 8 * sizeof(int), s));
        HIPCHK(c, launch_box_mark(bx, s));
        HIPCHK(c, launch_box_sparse(bx, s));
    }
    return CY_OK;
}

int cy_profile_enable(cy_ctx* c, int on) {
    if (!c) return CY_ERR_ARG;
    c->profiling = on != 0;
    c->prof_stride = on > 1 ? on : 1;                    // on = N > 1: time every N-th forward call only (an event per launch costs ~3 % at N = 1)
    c->fwd_calls = 0;
    c->prof.clear(); c->ev_used = 0;
    return CY_OK;
}

static int profile_summary_lane(cy_ctx* c, cy_prof_entry* out, int cap, int lane);
int cy_profile_summary(cy_ctx* c, cy_prof_entry* out, int cap) { return profile_summary_lane(c, out, cap, -1); }
int cy_profile_summary_lane(cy_ctx* c, cy_prof_entry* out, int cap, int lane) { return profile_summary_lane(c, out, cap, lane); }

static int profile_summary_lane(cy_ctx* c, cy_prof_entry* out, int cap, int lane) {
    // one entry per forward kernel variant (conv variants in ConvVariant order, then stem, pool)
    const int n = CONV_NUM_VARIANTS + 5;
    if (!c || !out || cap < n) return fail(c, CY_ERR_ARG, "bad arguments");
    HIPCHK(c, hipDeviceSynchronize());
    for (int k = 0; k < n; ++k) {
        memset(&out[k], 0, sizeof(out[k]));
        static const char* const extra[5] = {"stem_kernel", "pool5_kernel", "dwconv3x3_kernel", "attention_kernel",
                                             "bneck64_kernel fused 3x3+3x3 64ch bottleneck, weights in registers"};
        const char* nm = k < CONV_NUM_VARIANTS ? conv_variant_name(k) : extra[k - CONV_NUM_VARIANTS];
        strncpy(out[k].kernel, nm, sizeof(out[k].kernel) - 1);
    }
    for (const auto& r : c->prof) {
        if (lane >= 0 && r.lane != lane) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev_pool[r.e0], c->ev_pool[r.e1]) != hipSuccess) continue;
        out[r.kind].ms += ms; out[r.kind].flops += r.flops; out[r.kind].launches += 1;
    }
    return n;
}

int cy_profile_layers(cy_ctx* c, cy_prof_entry* out, int cap) {
    if (!c || !c->loaded || !out) return fail(c, CY_ERR_ARG, "bad arguments");
    const int n = (int)c->plan.convs.size();
    if (cap < n) return fail(c, CY_ERR_ARG, "need one entry per conv");
    HIPCHK(c, hipDeviceSynchronize());
    for (int i = 0; i < n; ++i) { memset(&out[i], 0, sizeof(out[i])); strncpy(out[i].kernel, c->plan.convs[i].name.c_str(), sizeof(out[i].kernel) - 1); }
    for (const auto& r : c->prof) {
        if (r.conv < 0) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev_pool[r.e0], c->ev_pool[r.e1]) != hipSuccess) continue;
        out[r.conv].ms += ms; out[r.conv].flops += r.flops; out[r.conv].launches += 1;
    }
    return n;
}

int cy_profile_layer_variant(cy_ctx* c, const char* conv_name, char* out, int cap) {
    if (!c || !c->loaded || !conv_name || !out || cap < 1) return fail(c, CY_ERR_ARG, "bad arguments");
    static const char* const extra[5] = {"stem_kernel", "pool5_kernel", "dwconv3x3_kernel", "attention_kernel", "bneck64_kernel"};
    out[0] = 0;
    const int n = (int)c->plan.convs.size();
    for (int i = 0; i < n; ++i) {
        if (c->plan.convs[i].name != conv_name) continue;
        for (const auto& r : c->prof)                          // the last launch timed for this convolution
            if (r.conv == i) {
                const char* nm = r.kind < CONV_NUM_VARIANTS ? conv_variant_name(r.kind) : extra[r.kind - CONV_NUM_VARIANTS];
                strncpy(out, nm, (size_t)cap - 1); out[cap - 1] = 0;
            }
        return CY_OK;
    }
    return fail(c, CY_ERR_ARG, std::string("no such conv: ") + conv_name);
}

int cy_debug_stop_after(cy_ctx* c, int n_ops) {
    if (!c) return CY_ERR_ARG;
    c->stop_after = n_ops > 0 ? n_ops : 0;
    return CY_OK;
}

int cy_debug_sparse_box(cy_ctx* c, const void* d_netin, int B, int H, int W, float* d_pred, float conf, int* h_sparse3, void* stream) {
    if (!c || !c->loaded) return fail(c, CY_ERR_STATE, "weights not loaded");
    if (!h_sparse3) return fail(c, CY_ERR_ARG, "null argument");
    c->split_last = false;
    BoxReq box{conf, {0, 0, 0}, 1};
    const int rc = forward_on(c, d_netin, B, H, W, d_pred, (hipStream_t)stream, c->ws, c->ws_bytes, false, 0, &box);
    for (int l = 0; l < 3; ++l) h_sparse3[l] = box.sparse[l];
    return rc;
}

int cy_debug_ops_done(cy_ctx* c) {
    if (!c || !c->loaded) return fail(c, CY_ERR_ARG, "bad arguments");
    if (c->lastB == 0) return fail(c, CY_ERR_STATE, "no forward has run");
    return c->ops_done;
}

int cy_debug_read_tensor(cy_ctx* c, int tensor, int coff, int C, float* h_out, size_t cap, int* dims4) {
    if (!c || !c->loaded || !h_out) return fail(c, CY_ERR_ARG, "bad arguments");
    if (c->lastB == 0) return fail(c, CY_ERR_STATE, "no forward has run");
    if (c->split_last) return fail(c, CY_ERR_STATE, "the last batch ran as two half-batches (CY_DUAL_FORWARD=0 keeps it in one workspace)");
    const Plan& p = c->plan;
    if (tensor == 0) return fail(c, CY_ERR_ARG, "tensor 0 is the caller's network input, not a workspace tensor");
    if (tensor < 0 || (size_t)tensor >= p.tensors.size()) return fail(c, CY_ERR_ARG, "no such tensor");
    const Tensor& t = p.tensors[tensor];
    if (coff < 0 || C < 1 || (long)coff + C > t.C) return fail(c, CY_ERR_ARG, "channel slice outside its tensor");
    const int Ho = c->lastH >> t.level, Wo = c->lastW >> t.level, B = c->lastB;
    const size_t n = (size_t)B * C * Ho * Wo;
    if (n > cap) return fail(c, CY_ERR_ARG, "output buffer too small");
    HIPCHK(c, hipDeviceSynchronize());
    std::vector<char> host(c->tbytes[tensor]);
    HIPCHK(c, hipMemcpy(host.data(), c->ws + c->toff[tensor], host.size(), hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b) for (int h = 0; h < Ho; ++h) for (int w = 0; w < Wo; ++w) for (int ch = 0; ch < C; ++ch) {
        const size_t px = ((size_t)b * Ho + h) * Wo + w;
        float v;
        if (c->prec == PREC_F16X3) {
            const _Float16* hp = reinterpret_cast<_Float16*>(host.data()) + px * 2 * t.C + coff + ch;
            v = (float)hp[0] + (float)hp[t.C];
        } else v = c->prec == PREC_F16 ? (float)reinterpret_cast<_Float16*>(host.data())[px * t.C + coff + ch]
                                       : reinterpret_cast<float*>(host.data())[px * t.C + coff + ch];
        h_out[(((size_t)b * C + ch) * Ho + h) * Wo + w] = v;
    }
    if (dims4) { dims4[0] = B; dims4[1] = C; dims4[2] = Ho; dims4[3] = Wo; }
    return CY_OK;
}

int cy_debug_read_conv(cy_ctx* c, const char* conv_name, float* h_out, size_t cap, int* dims4) {
    if (!c || !c->loaded || !conv_name || !h_out) return fail(c, CY_ERR_ARG, "bad arguments");
    if (c->lastB == 0) return fail(c, CY_ERR_STATE, "no forward has run");
    if (c->split_last) return fail(c, CY_ERR_STATE, "the last batch ran as two half-batches (CY_DUAL_FORWARD=0 keeps it in one workspace)");
    const Plan& p = c->plan;
    for (size_t i = 0; i < p.ops.size(); ++i) {
        const Op& o = p.ops[i];
        if (o.conv < 0 || p.convs[o.conv].name != conv_name) continue;      // pool and attention ops carry no convolution
        if (o.out < 0) return fail(c, CY_ERR_UNSUPPORTED, "head outputs are read from d_pred");
        // the bottlenecks of one C2f share the buffer of their cv1 outputs: all but the last one's are gone after the pass
        for (const Op* q = &o + 1; q < p.ops.data() + p.ops.size(); ++q) {
            const int qc = q->conv >= 0 ? p.convs[q->conv].cout : q->c0;
            if (q->out == o.out && q->out_coff < o.out_coff + p.convs[o.conv].cout && o.out_coff < q->out_coff + qc)
                return fail(c, CY_ERR_STATE, "this layer's output was not materialised beyond its reader: a later layer of the same block reuses its buffer");
        }
        if (i < c->fused_last.size() && c->fused_last[i])
            return fail(c, CY_ERR_STATE, o.fuse == FUSE_BNECK_PAIR ? "this bottleneck ran fused: its cv1 output was not materialised; unset CY_BNECK_FUSE"
                                         : o.fuse == FUSE_PW_PAIR ? "this layer ran fused with the 1x1 convolution behind it: its output was not materialised; CY_FUSE_PW=0 runs the two layers apart"
                                         : "the stem output was not materialised (fused into the next layer's kernel); set CY_STEM_FUSE=0");
        return cy_debug_read_tensor(c, o.out, o.out_coff, p.convs[o.conv].cout, h_out, cap, dims4);
    }
    return fail(c, CY_ERR_ARG, std::string("no such conv: ") + conv_name);
}

// One launch_conv on caller buffers with the layout the plan executor gives a convolution: channel slices of wider NHWC buffers,
// two input segments, the x2 upsample of segment 0, a residual slice, fp32 prediction rows.  Every rule below is checked on the
// host before anything is uploaded or launched.  A dense output / residual tensor (ct == Cout, offset 0) may have any width, as
// cy_conv_bn_silu always allowed (Cout = 5: no whole vector group is ever stored).
int cy_conv_slices(cy_ctx* c, const cy_conv_layout* L, const float* h_w, const float* h_b, char* variant, int variant_cap,
                   int* passes, void* stream) {
    if (!c || !L || !L->d_in0 || !h_w || !h_b || !L->d_out) return fail(c, CY_ERR_ARG, "null argument");
    const int B = L->B, Hi = L->Hi, Wi = L->Wi, Cin = L->Cin, Cout = L->Cout, k = L->k, s = L->s;
    if ((k != 1 && k != 3) || (s != 1 && s != 2) || Cin % 8 || Cin < 8 || Cout < 1 || B < 1 || Hi < 1 || Wi < 1)
        return fail(c, CY_ERR_ARG, "unsupported conv geometry");
    const bool x3 = c->prec == PREC_F16X3, rows = L->rows != 0, has1 = L->c1 != 0;
    const int cm = x3 ? 2 : 1, pad = k / 2, Ho = (Hi + 2 * pad - k) / s + 1, Wo = (Wi + 2 * pad - k) / s + 1;
    const int chunk = c->prec == PREC_F32 ? 32 : 64;                // channels of one K chunk (BKE)
    auto dense = [&](int ct, int coff) { return ct == Cout && coff == 0; };
    if (!ch8(L->in0_ct) || !ch8(L->in0_coff) || !ch8(L->c0) || L->c0 < 8 || L->in0_coff + L->c0 > L->in0_ct)
        return fail(c, CY_ERR_ARG, "segment 0: slice outside its tensor, or a channel count / offset not a multiple of 8");
    if (L->c1 < 0 || (has1 && (!L->d_in1 || !ch8(L->in1_ct) || !ch8(L->in1_coff) || !ch8(L->c1) || L->in1_coff + L->c1 > L->in1_ct)))
        return fail(c, CY_ERR_ARG, "segment 1: slice outside its tensor, or a channel count / offset not a multiple of 8");
    if (L->c0 + L->c1 != Cin) return fail(c, CY_ERR_ARG, "c0 + c1 != Cin");
    if (has1 && (k != 1 || s != 1 || L->c0 % chunk)) return fail(c, CY_ERR_ARG, "two segments: 1x1 stride 1 only, c0 a multiple of the K chunk (64 channels, 32 in fp32)");
    if (L->up0 && (k != 1 || s != 1 || Hi % 2 || Wi % 2)) return fail(c, CY_ERR_ARG, "upsampled segment 0: 1x1 stride 1 on even maps only");
    if (L->out_coff < 0 || L->out_coff + Cout > L->out_ct || (!rows && !dense(L->out_ct, L->out_coff) && (!ch8(L->out_ct) || !ch8(L->out_coff))))
        return fail(c, CY_ERR_ARG, "output: slice outside its tensor, or a channel count / offset not a multiple of 8");
    if (L->d_res && (L->res_coff < 0 || L->res_coff + Cout > L->res_ct || (!dense(L->res_ct, L->res_coff) && (!ch8(L->res_ct) || !ch8(L->res_coff)))))
        return fail(c, CY_ERR_ARG, "residual: slice outside its tensor, or a channel count / offset not a multiple of 8");
    if (rows && (L->out_ro < 0 || (long)L->out_ro + (long)Ho * Wo > L->out_bs || L->d_res || L->act))
        return fail(c, CY_ERR_ARG, "prediction rows: out_ro + Ho * Wo must fit out_bs; no residual, no activation");
    if (L->d_out == L->d_in0 || (has1 && L->d_out == L->d_in1)) return fail(c, CY_ERR_ARG, "the output must not alias an input");
    if (L->d_res && L->d_res == L->d_out) {            // the C2f pattern: residual and output are disjoint slices of one buffer
        if (L->res_ct != L->out_ct || (L->res_coff < L->out_coff + Cout && L->out_coff < L->res_coff + Cout))
            return fail(c, CY_ERR_ARG, "residual and output in one buffer must be disjoint slices of the same width");
    }
    const int H0 = L->up0 ? Hi / 2 : Hi, W0 = L->up0 ? Wi / 2 : Wi;
    const long n0 = (long)B * H0 * W0, n1 = (long)B * Hi * Wi, nout = (long)B * Ho * Wo;
    const size_t es = esize(c->prec);
    if ((size_t)n0 * L->in0_ct * es >= (1ull << 32) || (has1 && (size_t)n1 * L->in1_ct * es >= (1ull << 32)))
        return fail(c, CY_ERR_ARG, "input buffer of 4 GiB or more");
    HIPCHK(c, hipSetDevice(c->device));
    // fp16x3 context: caller tensors are fp32 NHWC; every buffer is split whole into [ct high | ct low] halves here (the output
    // buffer too, so that what lies outside the slice travels through), the layer runs on the split kernels exactly as inside the
    // forward pass, and the output buffer is merged back to fp32.  Prediction rows are fp32 in every context.
    hipStream_t st = (hipStream_t)stream;
    DevOwner sc;
    DevConv dc;
    void *in0 = const_cast<void*>(L->d_in0), *in1 = const_cast<void*>(L->d_in1), *res = const_cast<void*>(L->d_res), *out = L->d_out;
    const bool split_out = x3 && !rows;
    hipError_t e = upload_conv(sc, c->prec, h_w, h_b, nullptr, Cout, Cin, k, s, false, dc);
    if (e == hipSuccess && x3) e = sc.split(L->d_in0, n0, L->in0_ct, &in0, st);
    if (e == hipSuccess && x3 && has1) e = sc.split(L->d_in1, n1, L->in1_ct, &in1, st);
    if (e == hipSuccess && split_out) e = sc.split(L->d_out, nout, L->out_ct, &out, st);
    if (e == hipSuccess && x3 && L->d_res) {
        if (L->d_res == L->d_out) res = out;
        else e = sc.split(L->d_res, nout, L->res_ct, &res, st);
    }
    if (e == hipSuccess) {
        ConvArgs a{};
        a.in0 = in0; a.in0_ct = cm * L->in0_ct; a.in0_coff = L->in0_coff; a.c0 = L->c0; a.up0 = L->up0 != 0;
        a.in0_bytes = (uint32_t)((size_t)n0 * L->in0_ct * es); a.in0_lo = x3 ? L->in0_ct : 0;
        if (has1) {
            a.in1 = in1; a.in1_ct = cm * L->in1_ct; a.in1_coff = L->in1_coff; a.c1 = L->c1;
            a.in1_bytes = (uint32_t)((size_t)n1 * L->in1_ct * es); a.in1_lo = x3 ? L->in1_ct : 0;
        }
        a.wgt = dc.w; a.wgt_bytes = (uint32_t)dc.wbytes; a.bias = dc.bias; a.wgt32 = dc.w32; a.wgt32_bytes = (uint32_t)dc.w32bytes;
        a.oscale = dc.oscale; a.split = x3 ? dc.passes : 0;
        a.B = B; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.Cin = Cin; a.Cout = Cout; a.k = k; a.s = s; a.act = L->act;
        a.out = out; a.out_coff = L->out_coff;
        if (rows) { a.out_ct = L->out_ct; a.out_bs = L->out_bs; a.out_ro = L->out_ro; a.out_f32 = 1; }
        else { a.out_ct = cm * L->out_ct; a.out_lo = x3 ? L->out_ct : 0; a.out_bs = Ho * Wo; }
        if (L->d_res) { a.res = res; a.res_ct = cm * L->res_ct; a.res_coff = L->res_coff; a.res_lo = x3 ? L->res_ct : 0; }
        const ConvChoice ch = conv_choose(c->prec, a, conv_knobs_env());
        if (variant && variant_cap > 0) snprintf(variant, (size_t)variant_cap, "%s", conv_variant_name(ch.variant));
        if (passes) *passes = a.split;
        e = launch_conv(c->prec, ch, a, st);
    }
    if (e == hipSuccess && split_out) e = launch_x3_merge(out, reinterpret_cast<float*>(L->d_out), nout, L->out_ct, st);
    return entry_done(c, e, st);
}

const char* cy_conv_variant_name(int idx) { return idx >= 0 && idx < CONV_NUM_VARIANTS ? conv_variant_name(idx) : nullptr; }

// the dense call of cy_conv_slices: every ct the channel count, every offset 0, one segment, no rows
int cy_conv_bn_silu(cy_ctx* c, const void* d_in, int B, int Hi, int Wi, int Cin, const float* h_w, const float* h_b,
                    int Cout, int k, int s, int act, const void* d_res, void* d_out, void* stream) {
    if (!c || !d_in || !h_w || !h_b || !d_out) return fail(c, CY_ERR_ARG, "null argument");
    cy_conv_layout L{};
    L.d_in0 = d_in; L.in0_ct = Cin; L.c0 = Cin;
    L.d_res = d_res; L.res_ct = Cout;
    L.d_out = d_out; L.out_ct = Cout;
    L.B = B; L.Hi = Hi; L.Wi = Wi; L.Cin = Cin; L.Cout = Cout; L.k = k; L.s = s; L.act = act;
    return cy_conv_slices(c, &L, h_w, h_b, nullptr, 0, nullptr, stream);
}

int cy_bottleneck64(cy_ctx* c, const void* d_in, int B, int H, int W, const float* h_w1, const float* h_b1, const float* h_w2,
                    const float* h_b2, int shortcut, void* d_out, void* stream) {
    if (!c || !d_in || !h_w1 || !h_b1 || !h_w2 || !h_b2 || !d_out || B < 1 || H < 1 || W < 1) return fail(c, CY_ERR_ARG, "bad arguments");
    if (c->prec != PREC_F16) return fail(c, CY_ERR_UNSUPPORTED, "the fused bottleneck kernel exists in the fp16 context only");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<char> wf(BNECK_WFRAG_BYTES);
    pack_bneck_weights(h_w1, h_w2, wf.data());
    std::vector<float> bias(h_b1, h_b1 + 64);
    bias.insert(bias.end(), h_b2, h_b2 + 64);
    DevOwner sc;
    void* dw = nullptr; float* db = nullptr;
    hipError_t e = sc.upload(wf.data(), wf.size(), &dw);
    if (e == hipSuccess) e = sc.upload(bias.data(), 128 * sizeof(float), &db);
    if (e == hipSuccess) {
        BneckArgs a{};
        a.in = d_in; a.in_ct = 64; a.in_coff = 0; a.in_bytes = (uint32_t)((size_t)B * H * W * 64 * 2);
        a.out = d_out; a.out_ct = 64; a.out_coff = 0; a.wfrag = dw; a.bias1 = db; a.bias2 = db + 64;
        a.B = B; a.H = H; a.W = W; a.shortcut = shortcut != 0;
        e = launch_bneck64(a, (hipStream_t)stream);
    }
    return entry_done(c, e, (hipStream_t)stream);
}

// ---- kernel-level test entries of the YOLO11 operators: one launch_dwconv / launch_attention / launch_pool5 with the argument
// structs filled as the OPK_DWCONV / OPK_ATTN / OPK_POOL branches of the plan executor fill them
int cy_dwconv3x3(cy_ctx* c, const void* d_in, int B, int H, int W, int C, int in_ct, int in_coff, const float* h_w, const float* h_b,
                 int act, int blk, int gstride, int goff, const void* d_res, int res_ct, int res_coff, void* d_out, int out_ct,
                 int out_coff, void* stream) {
    if (!c || !d_in || !h_w || !h_b || !d_out) return fail(c, CY_ERR_ARG, "null argument");
    if (B < 1 || H < 1 || W < 1 || C < 8 || C % 8 || blk < 0) return fail(c, CY_ERR_ARG, "unsupported depth-wise geometry");
    const int last = blk ? ((C - 1) / blk) * gstride + goff + (C - 1) % blk : C - 1;      // highest input channel read
    if (!ch8(in_ct) || !ch8(in_coff) || !ch8(out_ct) || !ch8(out_coff) || !ch8(blk) || (blk && (!ch8(gstride) || !ch8(goff))) ||
        in_coff + last >= in_ct || out_coff + C > out_ct || (d_res && (!ch8(res_ct) || !ch8(res_coff) || res_coff + C > res_ct)))
        return fail(c, CY_ERR_ARG, "channel slice outside its tensor, or an offset / stride not a multiple of 8");
    if (d_out == d_in || d_out == d_res) return fail(c, CY_ERR_ARG, "the output must not alias the input or the residual");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const bool x3 = c->prec == PREC_F16X3;
    const int cm = x3 ? 2 : 1;
    const long npix = (long)B * H * W;
    const std::vector<float> dw = dw_weights(h_w, C);
    DevOwner sc;
    void *wd = nullptr, *bd = nullptr, *in = const_cast<void*>(d_in), *res = const_cast<void*>(d_res), *out = d_out;
    hipError_t e = sc.alloc(4 * dw.size(), &wd);
    if (e == hipSuccess) e = sc.alloc(4 * (size_t)C, &bd);
    if (e == hipSuccess) e = hipMemcpy(wd, dw.data(), 4 * dw.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(bd, h_b, 4 * (size_t)C, hipMemcpyHostToDevice);
    if (e == hipSuccess && x3) e = sc.split(d_in, npix, in_ct, &in, st);
    if (e == hipSuccess && x3 && d_res) e = sc.split(d_res, npix, res_ct, &res, st);
    if (e == hipSuccess && x3) e = sc.split(d_out, npix, out_ct, &out, st);
    if (e == hipSuccess) {
        DwArgs a{};
        a.in = in; a.in_ct = cm * in_ct; a.in_coff = in_coff; a.out = out; a.out_ct = cm * out_ct; a.out_coff = out_coff;
        a.in_lo = in_ct; a.out_lo = out_ct;
        if (d_res) { a.res = res; a.res_ct = cm * res_ct; a.res_coff = res_coff; a.res_lo = res_ct; }
        a.w = reinterpret_cast<const float*>(wd); a.bias = reinterpret_cast<const float*>(bd);
        a.B = B; a.H = H; a.W = W; a.C = C; a.act = act != 0;
        a.blk = blk; a.gstride = gstride; a.goff = goff;
        e = launch_dwconv(c->prec, a, st);
    }
    if (e == hipSuccess && x3) e = launch_x3_merge(out, reinterpret_cast<float*>(d_out), npix, out_ct, st);
    return entry_done(c, e, st);
}

int cy_attention(cy_ctx* c, const void* d_qkv, int B, int N, int ct, int coff, int heads, int kd, int hd, void* d_out, int out_ct,
                 int out_coff, void* stream) {
    if (!c || !d_qkv || !d_out) return fail(c, CY_ERR_ARG, "null argument");
    if (B < 1 || N < 1 || heads < 1 || kd < 1 || kd > 64 || hd < 1) return fail(c, CY_ERR_ARG, "unsupported attention geometry");
    if (coff < 0 || coff + heads * (2 * kd + hd) > ct || out_coff < 0 || out_coff + heads * hd > out_ct)
        return fail(c, CY_ERR_ARG, "channel slice outside its tensor");
    if (d_out == d_qkv) return fail(c, CY_ERR_ARG, "the output must not alias the input");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const bool x3 = c->prec == PREC_F16X3;
    const int cm = x3 ? 2 : 1;
    const long npix = (long)B * N;
    DevOwner sc;
    void *qkv = const_cast<void*>(d_qkv), *out = d_out;
    hipError_t e = hipSuccess;
    if (x3) e = sc.split(d_qkv, npix, ct, &qkv, st);
    if (e == hipSuccess && x3) e = sc.split(d_out, npix, out_ct, &out, st);
    if (e == hipSuccess) {
        AttnArgs a{};
        a.qkv = qkv; a.ct = cm * ct; a.coff = coff; a.out = out; a.out_ct = cm * out_ct; a.out_coff = out_coff;
        a.lo = ct; a.out_lo = out_ct;
        a.B = B; a.N = N; a.heads = heads; a.kd = kd; a.hd = hd;
        a.scale = 1.0f / sqrtf((float)a.kd);
        e = launch_attention(c->prec, a, st);
        if (e == hipErrorInvalidValue) {
            entry_done(c, hipSuccess, st);
            return fail(c, CY_ERR_UNSUPPORTED, ATTN_TOO_LARGE);
        }
    }
    if (e == hipSuccess && x3) e = launch_x3_merge(out, reinterpret_cast<float*>(d_out), npix, out_ct, st);
    return entry_done(c, e, st);
}

int cy_maxpool5(cy_ctx* c, const void* d_src, int B, int H, int W, int C, int ct, int src_coff, void* d_dst, int dst_coff,
                void* stream) {
    if (!c || !d_src || !d_dst) return fail(c, CY_ERR_ARG, "null argument");
    if (B < 1 || H < 1 || W < 1 || C < 8 || C % 8) return fail(c, CY_ERR_ARG, "unsupported pool geometry");
    if (!ch8(ct) || !ch8(src_coff) || !ch8(dst_coff) || src_coff + C > ct || dst_coff + C > ct)
        return fail(c, CY_ERR_ARG, "channel slice outside its tensor, or an offset / stride not a multiple of 8");
    if (d_src == d_dst && src_coff < dst_coff + C && dst_coff < src_coff + C) return fail(c, CY_ERR_ARG, "overlapping source and destination slices");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    const bool x3 = c->prec == PREC_F16X3;
    const int cm = x3 ? 2 : 1;
    const long npix = (long)B * H * W;
    DevOwner sc;
    void *src = const_cast<void*>(d_src), *dst = d_dst;
    hipError_t e = hipSuccess;
    if (x3) e = sc.split(d_dst, npix, ct, &dst, st);
    if (e == hipSuccess && x3) { if (d_src == d_dst) src = dst; else e = sc.split(d_src, npix, ct, &src, st); }   // SPPF: one buffer
    if (e == hipSuccess) {
        PoolArgs a{};
        a.src = src; a.dst = dst; a.ct = cm * ct; a.src_coff = src_coff; a.dst_coff = dst_coff; a.lo = x3 ? ct : 0;
        a.C = C; a.B = B; a.H = H; a.W = W;
        e = launch_pool5(c->prec, a, st);
    }
    if (e == hipSuccess && x3) e = launch_x3_merge(dst, reinterpret_cast<float*>(d_dst), npix, ct, st);
    return entry_done(c, e, st);
}

int cy_debug_stamps(unsigned long long* out8, int reset) {
    if (!out8) return CY_ERR_ARG;
    if (reset <= -(1 << 20)) { debug_read_wg_life(out8, -reset - (1 << 20)); return CY_OK; }      // pixels-direct kernel, entry / exit / CU per workgroup: (-reset - 2^20) x 3 values
    if (reset < 0) { debug_read_wg_stamps(out8, -reset); return CY_OK; }      // raw per-workgroup records: out8 holds (-reset) x 4 values
    if (reset >= 2) debug_read_pre_stamps(out8, reset == 3);       // 2 / 3: the statistics kernel's phase stamps (read / read + reset)
    else debug_read_stamps(out8, reset != 0);
    return CY_OK;
}

int cy_debug_fastdiv(const double* d_a, const double* d_b, double* d_fast, double* d_ref, int n) {
    if (!d_a || !d_b || !d_fast || !d_ref || n < 1) return CY_ERR_ARG;
    debug_fastdiv(d_a, d_b, d_fast, d_ref, n);
    return hipGetLastError() == hipSuccess ? CY_OK : CY_ERR_HIP;
}

int cy_debug_reduce(const double* d_val, const float* d_key, int nrows, int len, unsigned long long* d_out) {
    if (!d_out || nrows < 1 || len < 0 || (len > 0 && (!d_val || !d_key))) return CY_ERR_ARG;
    debug_reduce(d_val, d_key, nrows, len, d_out);
    return hipGetLastError() == hipSuccess ? CY_OK : CY_ERR_HIP;
}

// asynchronous on `stream`, like cy_forward: the point is what the kernels queued behind it find in LDS
int cy_debug_lds_fill(cy_ctx* c, unsigned pattern32, void* stream) {
    if (!c) return CY_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int bytes = 0;
    HIPCHK(c, launch_lds_fill(pattern32, (hipStream_t)stream, &bytes));
    return bytes;
}

int cy_debug_cand_counts(cy_ctx* c, int* h_out, int B) {
    if (!c || !c->loaded || !h_out || B < 1 || B > c->cfg.max_batch) return fail(c, CY_ERR_ARG, "bad arguments");
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(h_out, c->S().cand_count, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
    return CY_OK;
}

int cy_preproc_params(cy_ctx* c, double* h_out, int B) {
    if (!c || !c->loaded || !h_out || B < 1 || B > c->cfg.max_batch) return fail(c, CY_ERR_ARG, "bad arguments");
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(h_out, c->S().pre_params, (size_t)B * 3 * CY_MAX_STAGES * 4 * sizeof(double), hipMemcpyDeviceToHost));
    return CY_OK;
}

static int fill_pre_args(cy_ctx* c, const float* d_mosaic, int MH, int MW, const int* h_tiles, int B, int th, int tw,
                         const cy_preproc_cfg* cfg, int* d_status, PreArgs& a) {
    if (cfg->nprog != 0 && cfg->nprog != 1 && cfg->nprog != 3) return fail(c, CY_ERR_ARG, "nprog must be 0, 1 or 3");
    if (B > MAX_PRE_BATCH) return fail(c, CY_ERR_ARG, "at most 256 tiles per preprocessing call");
    for (int b = 0; b < B; ++b) {
        a.txy[2 * b] = h_tiles[2 * b]; a.txy[2 * b + 1] = h_tiles[2 * b + 1];
        if (h_tiles[2 * b] < 0 || h_tiles[2 * b + 1] < 0 || h_tiles[2 * b] + tw > MW || h_tiles[2 * b + 1] + th > MH)
            return fail(c, CY_ERR_ARG, "tile outside the mosaic");
    }
    // the statistics passes address a tile through a raw buffer resource with 32-bit byte offsets
    if (((long)(th - 1) * MW + tw) * 4L > 0xFFFFFF00L)
        return fail(c, CY_ERR_UNSUPPORTED, "tile rows span more than 4 GiB of the mosaic: crop the image or run it in tiles");
    a.mosaic = d_mosaic; a.MH = MH; a.MW = MW; a.B = B; a.th = th; a.tw = tw;
    a.nprog = cfg->nprog;
    for (int i = 0; i < 3; ++i) {
        a.prog[i].n = cfg->prog[i].n;
        if (a.prog[i].n < 0 || a.prog[i].n > MAX_STAGES) return fail(c, CY_ERR_ARG, "too many stages");
        bool reversed = false;               // a decreasing map so far (MINMAX with norm_max < norm_min)
        for (int j = 0; j < a.prog[i].n; ++j) {
            const cy_pre_stage& st = cfg->prog[i].st[j];
            if (st.op < CY_OP_BKG || st.op > CY_OP_MINMAX) return fail(c, CY_ERR_ARG, "unknown preprocessing op");
            // the statistics kernel selects medians by the order of the RAW pixels, which needs every earlier map to be
            // non-decreasing (cy_preproc.hip); the CLI order (scripts/run.py:272-302) puts MINMAX last, so this never fires there
            if (reversed && (st.op == CY_OP_BKG || st.op == CY_OP_SHIFT || st.op == CY_OP_CLIP))
                return fail(c, CY_ERR_UNSUPPORTED, "a sigma-clip stage after a MINMAX stage with norm_max < norm_min is not supported");
            if (st.op == CY_OP_MINMAX && st.p1 < st.p0) reversed = !reversed;
            a.prog[i].st[j] = PreStage{st.op, st.p0, st.p1, st.p2, st.flag};
        }
    }
    a.params = c->S().pre_params; a.histeq = c->S().pre_histeq; a.status = d_status; a.counters = c->counters;
    return CY_OK;
}

static int preproc_as(cy_ctx* c, const float* d_mosaic, int MH, int MW, const int* h_tiles, int B, int th, int tw, int imgsz,
                      const cy_preproc_cfg* cfg, void* d_netin, Precision out_prec, int* d_status, void* stream);

int cy_preproc(cy_ctx* c, const float* d_mosaic, int MH, int MW, const int* h_tiles, int B, int th, int tw, int imgsz,
               const cy_preproc_cfg* cfg, void* d_netin, int* d_status, void* stream) {
    if (!c || !c->loaded) return fail(c, CY_ERR_STATE, "weights not loaded");
    return preproc_as(c, d_mosaic, MH, MW, h_tiles, B, th, tw, imgsz, cfg, d_netin, io_prec(c->prec), d_status, stream);
}

// cy_preproc with the type of the network-input canvas named (the augmented path of the fp16 context packs fp32)
static int preproc_as(cy_ctx* c, const float* d_mosaic, int MH, int MW, const int* h_tiles, int B, int th, int tw, int imgsz,
                      const cy_preproc_cfg* cfg, void* d_netin, Precision out_prec, int* d_status, void* stream) {
    if (!d_mosaic || !h_tiles || !cfg || !d_netin || !d_status || B < 1 || B > c->cfg.max_batch)
        return fail(c, CY_ERR_ARG, "bad preproc arguments");
    cy_letterbox lb;
    if (cy_letterbox_geometry(th, tw, imgsz, &lb)) return fail(c, CY_ERR_ARG, "bad tile/imgsz");
    if (lb.H > c->cfg.max_h || lb.W > c->cfg.max_w) return fail(c, CY_ERR_ARG, "letterboxed tile exceeds max_h/max_w of the context");
    PreArgs a{};
    int rc = fill_pre_args(c, d_mosaic, MH, MW, h_tiles, B, th, tw, cfg, d_status, a);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    a.out = d_netin; a.out_prec = out_prec; a.H = lb.H; a.W = lb.W; a.top = lb.top; a.left = lb.left;
    a.new_h = lb.new_h; a.new_w = lb.new_w;
    const bool resize = (lb.new_h != th) || (lb.new_w != tw);
    if (resize && (size_t)B * 3 * th * tw > c->pre_scratch_elems) return fail(c, CY_ERR_ARG, "resize scratch too small");
    a.scratch = resize ? c->S().pre_scratch : nullptr;
    HIPCHK(c, launch_preproc(a, s));
    return CY_OK;
}

int cy_preproc_planes(cy_ctx* c, const float* d_mosaic, int MH, int MW, const int* h_tiles, int B, int th, int tw,
                      const cy_preproc_cfg* cfg, double* d_planes, int* d_status, void* stream) {
    if (!c || !c->loaded) return fail(c, CY_ERR_STATE, "weights not loaded");
    if (!d_mosaic || !h_tiles || !cfg || !d_planes || !d_status || B < 1 || B > c->cfg.max_batch || th < 1 || tw < 1)
        return fail(c, CY_ERR_ARG, "bad preproc arguments");
    PreArgs a{};
    int rc = fill_pre_args(c, d_mosaic, MH, MW, h_tiles, B, th, tw, cfg, d_status, a);
    if (rc) return rc;
    a.scratch = d_planes;
    HIPCHK(c, launch_preproc_planes(a, (hipStream_t)stream));
    return CY_OK;
}

// planes -> the letterboxed network input of type out_prec
static int letterbox_pack_as(cy_ctx* c, const double* d_planes, int B, int h0, int w0, int imgsz, void* d_out, Precision out_prec, void* stream) {
    if (!c || !c->loaded) return fail(c, CY_ERR_STATE, "weights not loaded");
    if (!d_planes || !d_out || B < 1 || B > c->cfg.max_batch) return fail(c, CY_ERR_ARG, "bad arguments");
    cy_letterbox lb;
    if (cy_letterbox_geometry(h0, w0, imgsz, &lb)) return fail(c, CY_ERR_ARG, "bad image/imgsz");
    if (lb.H > c->cfg.max_h || lb.W > c->cfg.max_w) return fail(c, CY_ERR_ARG, "letterboxed image exceeds max_h/max_w of the context");
    PreArgs a{};
    a.B = B; a.th = h0; a.tw = w0; a.scratch = const_cast<double*>(d_planes);
    a.out = d_out; a.out_prec = out_prec; a.H = lb.H; a.W = lb.W; a.top = lb.top; a.left = lb.left;
    a.new_h = lb.new_h; a.new_w = lb.new_w;
    HIPCHK(c, launch_letterbox_pack(a, (hipStream_t)stream));
    return CY_OK;
}
int cy_letterbox_pack(cy_ctx* c, const double* d_planes, int B, int h0, int w0, int imgsz, void* d_netin, void* stream) {
    return letterbox_pack_as(c, d_planes, B, h0, w0, imgsz, d_netin, c ? io_prec(c->prec) : PREC_F32, stream);
}
int cy_letterbox_pack_f32(cy_ctx* c, const double* d_planes, int B, int h0, int w0, int imgsz, float* d_out, void* stream) {
    return letterbox_pack_as(c, d_planes, B, h0, w0, imgsz, d_out, PREC_F32, stream);
}

// NMS over the candidates a decode left in (cand, cand_anchor, keys: capacity cap per tile) + ultralytics scale_boxes (gain / pad from
// the letterboxed and the original shape), for the plain and the augmented decode
static int nms_on(cy_ctx* c, const float* cand, const int* cand_anchor, uint64_t* keys, int cap, int B, int H, int W, int h0, int w0,
                  float iou, float* d_det, int* d_det_anchor, int* d_count, hipStream_t s) {
    NmsArgs n{};
    n.cand = cand; n.cand_anchor = cand_anchor; n.cand_count = c->S().cand_count; n.cap = cap; n.B = B; n.iou = iou;
    n.max_det = CY_MAX_DET;
    const double gain = std::fmin((double)H / h0, (double)W / w0);
    n.gain = (float)gain;
    n.padw = py_round((W - w0 * gain) / 2 - 0.1); n.padh = py_round((H - h0 * gain) / 2 - 0.1);
    n.w0 = w0; n.h0 = h0;
    n.det = d_det; n.det_anchor = d_det_anchor; n.det_count = d_count; n.keys = keys; n.mask = nullptr;
    n.counters = c->counters;
    HIPCHK(c, launch_nms(n, s));
    return CY_OK;
}

int cy_decode_nms(cy_ctx* c, const float* d_pred, int B, int H, int W, int h0, int w0, float conf, float iou,
                  float* d_det, int* d_det_anchor, int* d_count, void* stream) {
    if (!c || !c->loaded) return fail(c, CY_ERR_STATE, "weights not loaded");
    if (!d_pred || !d_det || !d_det_anchor || !d_count || B < 1 || B > c->cfg.max_batch) return fail(c, CY_ERR_ARG, "bad arguments");
    if (H > c->cfg.max_h || W > c->cfg.max_w) return fail(c, CY_ERR_ARG, "input exceeds max_h/max_w of the context");
    hipStream_t s = (hipStream_t)stream;
    DecodeArgs d{};
    d.pred = d_pred; d.B = B; d.A = cy_num_anchors(H, W); d.nc = c->plan.nc; d.conf = conf;
    for (int l = 0; l < 3; ++l) { d.lvl_h[l] = H >> (3 + l); d.lvl_w[l] = W >> (3 + l); }
    d.cand = c->S().cand; d.cand_anchor = c->S().cand_anchor; d.cand_count = c->S().cand_count; d.cap = c->cap;
    HIPCHK(c, hipMemsetAsync(c->S().cand_count, 0, B * sizeof(int), s));
    HIPCHK(c, launch_decode(d, s));
    return nms_on(c, c->S().cand, c->S().cand_anchor, c->S().keys, c->cap, B, H, W, h0, w0, iou, d_det, d_det_anchor, d_count, s);
}

int cy_iou_merge(cy_ctx* c, const float* d_det, const int* d_count, int B, float score_thr, double soft, double hard,
                 float* d_out, int* d_out_count, int* d_out_src, void* stream) {
    if (!c || !c->loaded) return fail(c, CY_ERR_STATE, "weights not loaded");
    if (!d_det || !d_count || !d_out || !d_out_count || B < 1 || B > c->cfg.max_batch) return fail(c, CY_ERR_ARG, "bad arguments");
    MergeArgs m{};
    m.det = d_det; m.det_count = d_count; m.B = B; m.max_det = CY_MAX_DET; m.score_thr = score_thr; m.soft = soft; m.hard = hard;
    m.out = d_out; m.out_count = d_out_count; m.out_src = d_out_src ? d_out_src : c->S().out_src; m.err = c->S().merge_err;
    m.counters = c->counters;
    HIPCHK(c, launch_iou_merge(m, (hipStream_t)stream));
    return CY_OK;
}

// One batch of the pipelined detect pass, plain or augmented.  The callers differ in three places: `pack` queues what builds the
// network input(s) on the preprocessing stream, `forwards` runs one forward per view through the lane's `fwd(in, H, W, pred)`, and
// `decode` queues decode + NMS into the buffer set's detections on the post-processing stream.
extern "C++" template <class Pack, class Forwards, class Decode>
static int pipeline_batch(cy_ctx* c, const float* d_mosaic, int B, float conf, double soft, double hard, float* d_out, int* d_out_count,
                          void* stream, Pack&& pack, Forwards&& forwards, Decode&& decode) {
    // Software pipeline over consecutive calls (batches): three streams, two buffer sets (+ the small-batch lane below).
    //   s_pre  : preprocessing of batch i      (waits: forward of batch i-2 has consumed this set's network input)
    //   stream : forward of batch i            (waits: preprocessing i; post-processing i-2 has consumed this set's head output)
    //   s_post : decode/NMS/IoU-merge of batch i (waits: forward i)
    // so the latency-bound statistics / NMS / merge kernels (a few dozen workgroups) run beside the conv stack of the
    // neighbouring batches instead of serialising with it.  Outputs are complete after cy_detect_flush(ctx, stream).
    hipStream_t sm = (hipStream_t)stream;
    // Small batches (the ragged edge classes of a grid: 39 + 39 + 1 of the 1600 tiles of the 16k mosaic) take their own lane:
    // buffer set 2, forward on the second stream / workspace.  A batch of 1-39 tiles is a chain of ~105 kernels of a few
    // workgroups each -- 4.2 ms for ONE tile, 6.2 ms for 39, i.e. 8 % of a pass for 4 % of its pixels when run in line -- but
    // hardly any work: beside the full batches of the main lane it costs about its share of the chip.  The caller
    // interleaves them with the full batches (TileEngine).  CY_SMALL_LANE=0 keeps every batch on the main lane.
    // "small" is relative to the context: at most a third of max_batch (and < 64 tiles).  With the CLI default --tile_batch 64
    // the equal-sized batches of 50-63 tiles stay on the main lane with its two buffer sets (the lane has ONE set: consecutive
    // small batches serialise preprocessing behind forward).  CY_SMALL_LANE is read per call (the tests compare both settings).
    const bool small = env_knob("CY_SMALL_LANE", 1) && c->prec != PREC_F32 && B < 64 && (long)B * 3 <= c->cfg.max_batch;
    int rc = CY_OK;
    if (small) { rc = ensure_small_lane(c); if (rc) return rc; }
    const int sl = small ? 2 : (int)(c->batches & 1);
    const bool reuse = small ? c->small_batches >= 1 : c->batches >= 2;
    hipStream_t sf = small ? c->s_small : sm;
    // Stream budget.  The HIP runtime maps streams onto four hardware queues; two BUSY streams on one queue serialise (DESIGN.md
    // section 5).  A context owns four: the caller's, preprocessing, post-processing and the second forward stream (small-batch lane /
    // second half of a split batch).  A collective library in the process (RCCL: one stream per communicator) is a fifth, and even idle
    // it displaces one of ours onto a shared queue: measured at N = 1 with a one-rank RCCL group, 176.7 -> 187.7 ms per pass.
    // CY_SIDE_STREAMS (read per call; TileEngine sets 3 when a process group exists): 2 = four streams (default); 1 = post-processing
    // shares the preprocessing stream (the NMS of batch i-1 then delays the statistics of batch i+1: 191.7 ms); 3 = post-processing
    // shares the SECOND FORWARD stream (decode / NMS / merge are ~1 ms per batch next to a small-batch forward that runs beside the
    // main lane anyway), i.e. three streams + the library's = four queues.
    const int side_mode = env_knob("CY_SIDE_STREAMS", 2);
    if (side_mode == 3) { rc = ensure_side_forward_stream(c); if (rc) return rc; }
    hipStream_t spost = side_mode == 1 ? c->s_pre : (side_mode == 3 ? c->s_fwd2 : c->s_post);
    struct SlotReset { cy_ctx* c; ~SlotReset() { c->slot = 0; } } slot_reset{c};      // the stage entry points use set 0 outside this call
    c->slot = sl;
    // order the side streams after whatever the caller already queued on `stream` -- only where that matters: the first batch
    // after load / flush, or after cy_mosaic_prepare.  Later batches are ordered by ev_fwd / ev_post alone, so that the
    // preprocessing of batch i does not wait for the forward of batch i-1 that is already queued on `stream`.
    // A mosaic buffer this pipeline has not seen yet may still be the target of an upload queued on `stream`: order behind it too.
    bool seen = false;
    for (int i = 0; i < c->n_seen; ++i) seen = seen || c->seen_mosaic[i] == (const void*)d_mosaic;
    if (c->batches + c->small_batches == 0 || c->mosaic_dirty || !seen) {
        HIPCHK(c, hipEventRecord(c->ev_call, sm));
        HIPCHK(c, hipStreamWaitEvent(c->s_pre, c->ev_call, 0));
        if (c->mosaic_dirty || c->batches + c->small_batches == 0) c->n_seen = 0;
        if (c->n_seen < 16) c->seen_mosaic[c->n_seen++] = d_mosaic;        // (a 17th distinct buffer is simply ordered again every time)
        c->mosaic_dirty = false;
    }
    if (reuse) HIPCHK(c, hipStreamWaitEvent(c->s_pre, c->ev_fwd[sl], 0));
    rc = pack(c->s_pre);
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->ev_pre[sl], c->s_pre));
    HIPCHK(c, hipStreamWaitEvent(sf, c->ev_pre[sl], 0));
    if (reuse) HIPCHK(c, hipStreamWaitEvent(sf, c->ev_post[sl], 0));
    rc = forwards([&](const void* in, int H, int W, float* pred, BoxReq* box = nullptr) -> int {
        if (!small) return forward_split(c, in, B, H, W, pred, sm, box);
        c->split_last = false;
        return forward_on(c, in, B, H, W, pred, sf, c->ws3, c->ws3_bytes, true, 0, box);      // (profiled like the main lane)
    });
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->ev_fwd[sl], sf));
    HIPCHK(c, hipStreamWaitEvent(spost, c->ev_fwd[sl], 0));
    rc = decode(spost);
    if (!rc) rc = cy_iou_merge(c, c->S().det, c->S().det_count, B, conf, soft, hard, d_out, d_out_count, nullptr, spost);
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->ev_post[sl], spost));
    if (small) c->small_batches++; else c->batches++;
    return CY_OK;
}

int cy_detect_tiles(cy_ctx* c, const float* d_mosaic, int MH, int MW, const int* h_tiles, int B, int th, int tw, int imgsz,
                    const cy_preproc_cfg* cfg, float conf, float iou, double soft, double hard,
                    float* d_out, int* d_out_count, int* d_status, void* stream) {
    if (!c || !c->loaded) return fail(c, CY_ERR_STATE, "weights not loaded");
    cy_letterbox lb;
    if (cy_letterbox_geometry(th, tw, imgsz, &lb)) return fail(c, CY_ERR_ARG, "bad tile/imgsz");
    BoxReq box{conf, {0, 0, 0}};
    return pipeline_batch(c, d_mosaic, B, conf, soft, hard, d_out, d_out_count, stream,
        [&](hipStream_t s) { return cy_preproc(c, d_mosaic, MH, MW, h_tiles, B, th, tw, imgsz, cfg, c->S().netin, d_status, s); },
        [&](auto&& fwd) { return fwd(c->S().netin, lb.H, lb.W, c->S().pred, &box); },      // the plain path: box logits at this call's candidates only
        [&](hipStream_t s) { return cy_decode_nms(c, c->S().pred, B, lb.H, lb.W, th, tw, conf, iou, c->S().det, c->S().det_anchor, c->S().det_count, s); });
}

int cy_detect_fence(cy_ctx* c, void* stream) {
    if (!c || !c->loaded) return fail(c, CY_ERR_STATE, "weights not loaded");
    (void)stream;
    c->mosaic_dirty = true;                  // the next cy_detect_tiles records an event on ITS stream and orders the side streams behind it
    return CY_OK;
}

int cy_detect_flush(cy_ctx* c, void* stream) {
    if (!c || !c->loaded) return fail(c, CY_ERR_STATE, "weights not loaded");
    hipStream_t sm = (hipStream_t)stream;
    const unsigned long n = c->batches < 2 ? c->batches : 2;
    for (unsigned long k = 0; k < n; ++k) {
        const int sl = (int)((c->batches - 1 - k) & 1);
        HIPCHK(c, hipStreamWaitEvent(sm, c->ev_post[sl], 0));
        HIPCHK(c, hipStreamWaitEvent(sm, c->ev_pre[sl], 0));
    }
    if (c->small_batches) {          // the small-batch lane (one buffer set: its batches are ordered among themselves)
        HIPCHK(c, hipStreamWaitEvent(sm, c->ev_post[2], 0));
        HIPCHK(c, hipStreamWaitEvent(sm, c->ev_pre[2], 0));
    }
    c->batches = 0; c->small_batches = 0; c->n_seen = 0;     // the next call starts a new pipeline: it orders the side streams behind `stream` again
    return CY_OK;
}

int cy_compact_records(const float* d_gathered, long long n_rows, const long long* d_perm, int T, int row_floats, int* d_hdr, float* d_out, void* stream) {
    if (!d_gathered || !d_perm || !d_hdr || !d_out || T < 1 || n_rows < 1 || row_floats != CY_MAX_DET * CY_DET_STRIDE + 3)
        return fail(nullptr, CY_ERR_ARG, "bad arguments");
    const hipError_t e = launch_compact_records(d_gathered, n_rows, d_perm, T, row_floats, d_hdr, d_out, (hipStream_t)stream);
    if (e != hipSuccess) return fail(nullptr, CY_ERR_HIP, hipGetErrorString(e));
    return CY_OK;
}

int cy_compact_records_ctx(cy_ctx* c, const float* d_gathered, long long n_rows, const long long* d_perm, int T, int row_floats, int* d_hdr, float* d_out, void* stream) {
    if (!c) return CY_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = cy_compact_records(d_gathered, n_rows, d_perm, T, row_floats, d_hdr, d_out, stream);
    if (rc != CY_OK) return fail(c, rc, "cy_compact_records failed (bad arguments or launch error)");
    return CY_OK;
}

int cy_detect_counters(cy_ctx* c, long long* out4, int reset) {
    if (!c || !c->loaded || !out4) return fail(c, CY_ERR_ARG, "bad arguments");
    int h[4] = {0, 0, 0, 0};
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(h, c->counters, sizeof(h), hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) out4[i] = h[i];
    if (reset) HIPCHK(c, hipMemset(c->counters, 0, sizeof(h)));
    return CY_OK;
}

// ---- measurement entries ----------------------------------------------------------------------
// Each one: argument checks, the host-side plan (cy_measure_plan.cpp), the kernel's arguments, one TimedLaunch.
static_assert(CY_MEAS_FIELDS == MEAS_FIELDS, "header and kernel disagree on the measurement row");
static_assert(CY_ISL_FIELDS == ISL_FIELDS, "header and kernel disagree on the island row");
static_assert(CY_DBL_FIELDS == DBL_FIELDS && CY_DBL_COMP_FIELDS == DBL_COMP_FIELDS && CY_DBL_MAX_COMP == DBL_MAX_COMP,
              "header and kernel disagree on the component rows");
static_assert(CY_FIT_FIELDS == FIT_FIELDS, "header and kernel disagree on the fit row");
static_assert(CY_BLEND_FIELDS == BLEND_FIELDS && CY_BLEND_MAX_MEMBERS == BLEND_MAX_MEMBERS, "header and kernel disagree on the blend row");
static_assert(CY_BKG_FIELDS == BKG_FIELDS, "header and kernel disagree on the background row");
static_assert(CY_RND_FIELDS == RND_FIELDS && CY_RND_HALF_MAX == RND_HALF_MAX, "header and planner disagree on the render row");
static_assert(CY_RES_FIELDS == RES_FIELDS, "header and kernel disagree on the residual row");
static_assert(CY_PEAK_FIELDS == PEAK_FIELDS && CY_PEAK_RADIUS_MAX == PEAK_RADIUS_MAX && CY_PEAK_CAP_MAX == PEAK_CAP_MAX,
              "header and kernel disagree on the peak row");
static_assert(CY_ATROUS_STEP_MAX == ATR_STEP_MAX, "header and kernel disagree on the largest a trous step");
static_assert(CY_APER_RINGS_MAX == APER_RINGS_MAX && CY_APER_RADIUS_MAX == APER_RADIUS_MAX && CY_APER_HEAD == APER_HEAD &&
              CY_APER_RING_FIELDS == APER_RING_FIELDS && CY_APER_FIELDS == APER_FIELDS && CY_APER_JOBS_MAX == APER_JOBS_MAX,
              "header and kernel disagree on the aperture row");
static_assert(CY_PFIT_JOB_FIELDS == PFIT_JOB_FIELDS && CY_PFIT_FIELDS == PFIT_FIELDS && CY_PFIT_RADIUS_MAX == PFIT_RADIUS_MAX &&
              CY_PFIT_NEIGH_MAX == PFIT_NEIGH_MAX && CY_PFIT_JOBS_MAX == PFIT_JOBS_MAX, "header and kernel disagree on the peak fit row");
static_assert(CY_PGRP_FIELDS == PGRP_FIELDS && CY_PGRP_FIELDS == CY_BLEND_FIELDS + 8, "header and kernel disagree on the peak group row");
static_assert(CY_DRES_FIELDS == DRES_FIELDS, "header and kernel disagree on the disc residual row");
static_assert(CY_FORCED_JOB_FIELDS == FORCED_JOB_FIELDS && CY_FORCED_FIELDS == FORCED_FIELDS && CY_FORCED_NEIGH_MAX == FORCED_NEIGH_MAX &&
              CY_FORCED_JOBS_MAX == FORCED_JOBS_MAX, "header and kernel disagree on the forced fit row");

int cy_measure_sources(cy_ctx* c, const float* d_img, int MH, int MW, const double* h_boxes, int n, int ring, double* h_out, void* stream) {
    if (!c) return fail(c, CY_ERR_ARG, "null argument");
    if (n < 0 || ring < 0 || MH <= 0 || MW <= 0) return fail(c, CY_ERR_ARG, "n >= 0, ring >= 0 and MH, MW > 0 required");
    if (n == 0) return CY_OK;
    if (!d_img || !h_boxes || !h_out) return fail(c, CY_ERR_ARG, "null argument");
    if ((long long)MH * MW >= (1LL << 31)) return fail(c, CY_ERR_ARG, IMAGE_TOO_LARGE);
    const std::vector<int> win = ring_windows(h_boxes, n, ring, MH, MW);
    TimedLaunch t(c, stream);
    MeasureArgs a{};
    a.img = d_img; a.MH = MH; a.MW = MW; a.n = n;
    a.win = t.upload(win.data(), win.size());
    a.out = t.scratch<double>((size_t)n * CY_MEAS_FIELDS);
    t.download(h_out, a.out, (size_t)n * CY_MEAS_FIELDS);
    return t.run(STEP_SOURCES, [&](hipStream_t s) { return launch_measure(a, s); });
}

int cy_measure_islands(cy_ctx* c, const float* d_img, int MH, int MW, const double* h_boxes, const double* h_thr, int n, int conn,
                       double* h_out, unsigned char* h_mask, const long long* h_mask_off, void* stream) {
    if (!c) return fail(c, CY_ERR_ARG, "null argument");
    if (n < 0 || (conn != 4 && conn != 8) || MH <= 0 || MW <= 0) return fail(c, CY_ERR_ARG, "n >= 0, conn 4 or 8 and MH, MW > 0 required");
    if (n == 0) return CY_OK;
    if (!d_img || !h_boxes || !h_thr || !h_out || (h_mask && !h_mask_off)) return fail(c, CY_ERR_ARG, "null argument");
    if ((long long)MH * MW >= (1LL << 31)) return fail(c, CY_ERR_ARG, IMAGE_TOO_LARGE);
    IslandTable tab;
    if (const char* msg = plan_islands(h_boxes, h_thr, 3, h_mask ? h_mask_off : nullptr, n, MH, MW, tab)) return fail(c, CY_ERR_ARG, msg);
    const bool masks = h_mask && tab.nmask > 0;
    TimedLaunch t(c, stream);
    IslandArgs a{};
    a.img = d_img; a.MH = MH; a.MW = MW; a.n = n; a.conn = conn;
    a.win = t.upload(tab.win.data(), tab.win.size());
    a.off = t.upload(tab.off.data(), tab.off.size());
    a.thr = t.upload(h_thr, (size_t)n * 3);
    a.out = t.scratch<double>((size_t)n * CY_ISL_FIELDS);
    a.ws = tab.nws ? t.scratch<unsigned>((size_t)tab.nws) : nullptr;           // every label is written before it is read: no memset
    a.mask = masks ? t.zeros<unsigned char>((size_t)tab.nmask) : nullptr;      // the kernel writes the non-zero bytes only
    t.download(h_out, a.out, (size_t)n * CY_ISL_FIELDS);
    if (masks) t.download(h_mask, a.mask, (size_t)tab.nmask);
    return t.run(STEP_ISLANDS, [&](hipStream_t s) { return launch_islands(a, s); });
}

int cy_deblend_islands(cy_ctx* c, const float* d_img, int MH, int MW, const double* h_boxes, const double* h_thr, int n, int conn, int radius,
                       double* h_out, double* h_comp, unsigned char* h_mask, const long long* h_mask_off, void* stream) {
    if (!c) return fail(c, CY_ERR_ARG, "null argument");
    if (n < 0 || (conn != 4 && conn != 8) || radius < 1 || radius > DBL_RADIUS_MAX || MH <= 0 || MW <= 0)
        return fail(c, CY_ERR_ARG, "n >= 0, conn 4 or 8, 1 <= radius <= 8 and MH, MW > 0 required");
    if (n == 0) return CY_OK;
    if (!d_img || !h_boxes || !h_thr || !h_out || !h_comp || (h_mask && !h_mask_off)) return fail(c, CY_ERR_ARG, "null argument");
    if ((long long)MH * MW >= (1LL << 31)) return fail(c, CY_ERR_ARG, IMAGE_TOO_LARGE);
    IslandTable tab;
    if (const char* msg = plan_islands(h_boxes, h_thr, 4, h_mask ? h_mask_off : nullptr, n, MH, MW, tab)) return fail(c, CY_ERR_ARG, msg);
    const bool masks = h_mask && tab.nmask > 0;
    const size_t ncomp = (size_t)n * CY_DBL_MAX_COMP * CY_DBL_COMP_FIELDS;
    TimedLaunch t(c, stream);
    DeblendArgs a{};
    a.img = d_img; a.MH = MH; a.MW = MW; a.n = n; a.conn = conn; a.radius = radius;
    a.win = t.upload(tab.win.data(), tab.win.size());
    a.off = t.upload(tab.off.data(), tab.off.size());
    a.thr = t.upload(h_thr, (size_t)n * 4);
    a.out = t.scratch<double>((size_t)n * CY_DBL_FIELDS);
    a.comp = t.zeros<double>(ncomp);                                           // the kernel writes the rows below ncomp only
    a.ws = tab.nws ? t.scratch<unsigned>((size_t)tab.nws * 2) : nullptr;       // labels, then `up` words; every word is written before it is read
    a.ws_up = a.ws ? a.ws + tab.nws : nullptr;
    a.mask = masks ? t.zeros<unsigned char>((size_t)tab.nmask) : nullptr;      // the kernel writes the non-zero bytes only
    t.download(h_out, a.out, (size_t)n * CY_DBL_FIELDS);
    t.download(h_comp, a.comp, ncomp);
    if (masks) t.download(h_mask, a.mask, (size_t)tab.nmask);
    return t.run(STEP_DEBLEND, [&](hipStream_t s) { return launch_deblend(a, s); });
}

// the argument checks cy_fit_components and cy_fit_blends share: the call's result, or FIT_GO_ON when there is something to plan
constexpr int FIT_GO_ON = 1;
static int fit_arguments(cy_ctx* c, const void* d_img, const FitInputs& in, int max_iter, const void* h_out) {
    if (!c) return fail(c, CY_ERR_ARG, "null argument");
    if (in.n < 0 || max_iter < 1 || max_iter > FIT_MAX_ITER || in.MH <= 0 || in.MW <= 0)
        return fail(c, CY_ERR_ARG, "n >= 0, 1 <= max_iter <= 256 and MH, MW > 0 required");
    if (in.n == 0) return CY_OK;
    if (!d_img || !in.boxes || !in.bkg || !in.ncomp || !in.start || !in.mask || !in.mask_off || !h_out) return fail(c, CY_ERR_ARG, "null argument");
    if ((long long)in.MH * in.MW >= (1LL << 31)) return fail(c, CY_ERR_ARG, IMAGE_TOO_LARGE);
    return FIT_GO_ON;
}

int cy_fit_components(cy_ctx* c, const float* d_img, int MH, int MW, const double* h_boxes, const double* h_bkg, const int* h_ncomp,
                      const double* h_start, int n, int max_iter, const unsigned char* h_mask, const long long* h_mask_off, double* h_fit,
                      void* stream) {
    const FitInputs in{MH, MW, n, h_boxes, h_bkg, h_ncomp, h_start, h_mask, h_mask_off};
    int rc = fit_arguments(c, d_img, in, max_iter, h_fit);
    if (rc != FIT_GO_ON) return rc;
    FitPlan p;
    if (const char* msg = plan_fit(in, p)) return fail(c, CY_ERR_ARG, msg);
    const size_t nrows = (size_t)n * DBL_MAX_COMP;
    std::memset(h_fit, 0, nrows * CY_FIT_FIELDS * sizeof(double));
    for (int i = 0; i < n; ++i)
        if (p.large[i])
            for (int k = 0; k < h_ncomp[i]; ++k) h_fit[((size_t)i * DBL_MAX_COMP + k) * CY_FIT_FIELDS] = 1.0;
    if (p.jobs.empty()) return CY_OK;
    std::vector<double> got(nrows * CY_FIT_FIELDS);
    TimedLaunch t(c, stream);
    FitArgs a{};
    a.img = d_img; a.MH = MH; a.MW = MW; a.njobs = (int)p.jobs.size(); a.nlist = (long long)p.list.size(); a.max_iter = max_iter;
    a.jobs = t.upload(p.jobs.data(), p.jobs.size());
    a.list = t.upload(p.list.data(), p.list.size());
    a.out = t.zeros<double>(got.size()); a.nrows = (int)nrows;                 // the kernel writes the jobs' rows only
    t.download(got.data(), a.out, got.size());
    rc = t.run(STEP_FIT, [&](hipStream_t s) { return launch_fit(a, s); });
    if (rc != CY_OK) return rc;
    for (const FitJob& j : p.jobs) write_back(got.data(), h_start, p.win0.data(), CY_FIT_FIELDS, 5, &j.row, 1, h_fit);
    return CY_OK;
}

int cy_fit_blends(cy_ctx* c, const float* d_img, int MH, int MW, const double* h_boxes, const double* h_bkg, const int* h_ncomp,
                  const double* h_start, int n, int max_iter, const unsigned char* h_mask, const long long* h_mask_off, double* h_out,
                  void* stream) {
    const FitInputs in{MH, MW, n, h_boxes, h_bkg, h_ncomp, h_start, h_mask, h_mask_off};
    int rc = fit_arguments(c, d_img, in, max_iter, h_out);
    if (rc != FIT_GO_ON) return rc;
    BlendPlan p;
    if (const char* msg = plan_blend(in, p)) return fail(c, CY_ERR_ARG, msg);
    std::memcpy(h_out, p.rows.data(), p.rows.size() * sizeof(double));
    if (p.jobs.empty()) return CY_OK;
    std::vector<double> got(p.rows.size());
    TimedLaunch t(c, stream);
    BlendArgs a{};
    a.img = d_img; a.MH = MH; a.MW = MW; a.njobs = (int)p.jobs.size(); a.nlist = (long long)p.list.size(); a.max_iter = max_iter;
    a.jobs = t.upload(p.jobs.data(), p.jobs.size());
    a.list = t.upload(p.list.data(), p.list.size());
    a.out = t.zeros<double>(got.size()); a.nrows = n * DBL_MAX_COMP;           // the kernel writes the members' rows only
    t.download(got.data(), a.out, got.size());
    rc = t.run(STEP_BLEND, [&](hipStream_t s) { return launch_blend(a, s); });
    if (rc != CY_OK) return rc;
    for (const BlendJob& j : p.jobs) {
        int rows[BLEND_MAX_MEMBERS];
        for (int m = 0; m < j.M; ++m) rows[m] = j.row0 + j.comp[m];
        write_back(got.data(), h_start, p.win0.data(), CY_BLEND_FIELDS, 8, rows, j.M, h_out);
    }
    return CY_OK;
}

int cy_measure_background(cy_ctx* c, const float* d_img, int MH, int MW, int cell, double k, int niter, double* h_out, void* stream) {
    if (!c) return fail(c, CY_ERR_ARG, "null argument");
    if (MH <= 0 || MW <= 0 || cell < BKG_CELL_MIN || cell > BKG_CELL_MAX || !(k > 0.0) || niter < 0 || niter > BKG_NITER_MAX)
        return fail(c, CY_ERR_ARG, "MH, MW > 0, 4 <= cell <= 4096, k > 0 and 0 <= niter <= 32 required");
    if (!d_img || !h_out) return fail(c, CY_ERR_ARG, "null argument");
    if ((long long)MH * MW >= (1LL << 31)) return fail(c, CY_ERR_ARG, "image of 2^31 pixels or more (32-bit pixel counts per cell)");
    TimedLaunch t(c, stream);
    BackgroundArgs a{};
    a.img = d_img; a.MH = MH; a.MW = MW; a.cell = cell; a.ncy = (MH + cell - 1) / cell; a.ncx = (MW + cell - 1) / cell; a.k = k; a.niter = niter;
    const size_t nout = (size_t)a.ncy * a.ncx * CY_BKG_FIELDS;
    a.out = t.scratch<double>(nout);
    t.download(h_out, a.out, nout);
    return t.run(STEP_BACKGROUND, [&](hipStream_t s) { return launch_background(a, s); });
}

// cy_render_gaussians and cy_render_signed_gaussians: one body, the planner told which amplitudes it admits
static int render_entry(cy_ctx* c, const float* d_img, int MH, int MW, const double* h_comp, int m, double nsigma, const float* d_bkg,
                        float* d_model, float* d_resid, double* h_rows, void* stream, bool signed_amp) {
    if (!c) return fail(c, CY_ERR_ARG, "null argument");
    if (MH <= 0 || MW <= 0 || !(nsigma >= 1.0 && nsigma <= 8.0)) return fail(c, CY_ERR_ARG, "MH, MW > 0 and 1 <= nsigma <= 8 required");
    if (!d_img || (!d_model && !d_resid) || (m > 0 && (!h_comp || !h_rows))) return fail(c, CY_ERR_ARG, "null argument");
    if ((long long)MH * MW >= (1LL << 31)) return fail(c, CY_ERR_ARG, "image of 2^31 pixels or more");
    RenderPlan p;
    if (const char* msg = plan_render(h_comp, m, nsigma, MH, MW, p, signed_amp)) return fail(c, CY_ERR_ARG, msg);
    TimedLaunch t(c, stream);
    RenderArgs a{};
    a.img = d_img; a.MH = MH; a.MW = MW; a.ntx = p.ntx; a.nty = p.nty; a.bkg = d_bkg; a.model = d_model; a.resid = d_resid;
    a.comp = t.upload(h_comp, (size_t)m * 6);
    a.rect = t.upload(p.rect.data(), p.rect.size());
    a.tile_off = t.upload(p.tile_off.data(), p.tile_off.size());
    a.tile_list = t.upload(p.tile_list.data(), p.tile_list.size());
    const int rc = t.run(STEP_RENDER, [&](hipStream_t s) { return launch_render(a, s); });
    if (rc == CY_OK && m > 0) std::memcpy(h_rows, p.rows.data(), p.rows.size() * sizeof(double));      // rows only beside maps that were written
    return rc;
}

int cy_render_gaussians(cy_ctx* c, const float* d_img, int MH, int MW, const double* h_comp, int m, double nsigma, const float* d_bkg,
                        float* d_model, float* d_resid, double* h_rows, void* stream) {
    return render_entry(c, d_img, MH, MW, h_comp, m, nsigma, d_bkg, d_model, d_resid, h_rows, stream, false);
}

int cy_render_signed_gaussians(cy_ctx* c, const float* d_img, int MH, int MW, const double* h_comp, int m, double nsigma, const float* d_bkg,
                               float* d_model, float* d_resid, double* h_rows, void* stream) {
    return render_entry(c, d_img, MH, MW, h_comp, m, nsigma, d_bkg, d_model, d_resid, h_rows, stream, true);
}

int cy_measure_residuals(cy_ctx* c, const float* d_img, const float* d_model, int MH, int MW, const double* h_boxes, const double* h_bkg,
                         int n, const unsigned char* h_mask, const long long* h_mask_off, double* h_out, void* stream) {
    if (!c) return fail(c, CY_ERR_ARG, "null argument");
    if (n < 0 || MH <= 0 || MW <= 0) return fail(c, CY_ERR_ARG, "n >= 0 and MH, MW > 0 required");
    if (n == 0) return CY_OK;
    if (!d_img || !d_model || !h_boxes || !h_bkg || !h_mask || !h_mask_off || !h_out) return fail(c, CY_ERR_ARG, "null argument");
    if ((long long)MH * MW >= (1LL << 31)) return fail(c, CY_ERR_ARG, IMAGE_TOO_LARGE);
    IslandTable tab;
    if (const char* msg = plan_residuals(h_boxes, h_mask_off, n, MH, MW, tab)) return fail(c, CY_ERR_ARG, msg);
    TimedLaunch t(c, stream);
    ResidualArgs a{};
    a.img = d_img; a.model = d_model; a.MH = MH; a.MW = MW; a.n = n;
    a.win = t.upload(tab.win.data(), tab.win.size());
    a.off = t.upload(tab.off.data(), tab.off.size());
    a.bkg = t.upload(h_bkg, (size_t)n);
    a.mask = t.upload(h_mask, (size_t)tab.nmask);
    a.out = t.scratch<double>((size_t)n * CY_RES_FIELDS);
    t.download(h_out, a.out, (size_t)n * CY_RES_FIELDS);
    return t.run(STEP_RESIDUAL, [&](hipStream_t s) { return launch_residual_stats(a, s); });
}

int cy_find_peaks(cy_ctx* c, const float* d_map, const float* d_rms, int MH, int MW, double k_sigma, int radius, int sign, int cap,
                  double* h_rows, long long* h_total, void* stream) {
    if (!c) return fail(c, CY_ERR_ARG, "null argument");
    if (MH <= 0 || MW <= 0 || radius < 1 || radius > PEAK_RADIUS_MAX || (sign != 1 && sign != -1) || !(k_sigma > 0.0) || !std::isfinite(k_sigma) ||
        cap < 0 || cap > PEAK_CAP_MAX)
        return fail(c, CY_ERR_ARG, "MH, MW > 0, 1 <= radius <= 8, sign +1 or -1, a finite k_sigma > 0 and 0 <= cap <= 2^20 required");
    if (!d_map || !d_rms || !h_total || (cap > 0 && !h_rows)) return fail(c, CY_ERR_ARG, "null argument");
    PeakPlan p;
    if (const char* msg = plan_peaks(MH, MW, radius, cap, p)) return fail(c, CY_ERR_ARG, msg);
    long long total = 0;
    TimedLaunch t(c, stream);
    PeakArgs a{};
    a.map = d_map; a.rms = d_rms; a.MH = MH; a.MW = MW; a.k_sigma = k_sigma; a.radius = radius; a.sign = sign;
    a.nsx = p.nsx; a.nseg = (int)p.nseg; a.cap = cap;
    a.count = t.scratch<unsigned>((size_t)p.nseg);                             // every entry of the three tables is written before it is read
    a.offset = t.scratch<unsigned>((size_t)p.nseg);
    a.bits = t.scratch<unsigned long long>((size_t)p.words);
    a.total = t.scratch<long long>(1);
    a.rows = t.scratch<double>((size_t)p.row_values);
    t.download(&total, a.total, 1);
    const int rc = t.run(STEP_PEAKS, [&](hipStream_t s) { return launch_peaks(a, s); });
    if (rc != CY_OK) return rc;
    // the rows that exist, and no others: the rest of h_rows stays as it is (the tables live as long as t)
    const long long nrows = std::min<long long>(total, cap);
    if (nrows > 0) HIPCHK(c, hipMemcpy(h_rows, a.rows, (size_t)nrows * CY_PEAK_FIELDS * sizeof(double), hipMemcpyDeviceToHost));
    *h_total = total;
    return CY_OK;
}

int cy_atrous_step(cy_ctx* c, const float* d_in, int MH, int MW, int step, float* d_smooth, float* d_detail, void* stream) {
    if (!c) return fail(c, CY_ERR_ARG, "null argument");
    AtrousPlan p;
    if (const char* msg = plan_atrous(MH, MW, step, (unsigned long long)reinterpret_cast<uintptr_t>(d_in), (unsigned long long)reinterpret_cast<uintptr_t>(d_smooth),
                                      (unsigned long long)reinterpret_cast<uintptr_t>(d_detail), p))
        return fail(c, CY_ERR_ARG, msg);
    TimedLaunch t(c, stream);
    AtrousArgs a{};
    a.in = d_in; a.MH = MH; a.MW = MW; a.step = step; a.smooth = d_smooth; a.detail = d_detail;
    a.ncb = p.ncb; a.nres = p.nres; a.nchunk = p.nchunk; a.items = (int)p.items; a.grid = p.grid;
    return t.run(STEP_ATROUS, [&](hipStream_t s) { return launch_atrous(a, s); });
}

int cy_aperture_sums(cy_ctx* c, const float* d_map, const float* d_rms, int MH, int MW, const double* h_jobs, int n, const double* h_factors,
                     int K, double* h_out, void* stream) {
    if (!c) return fail(c, CY_ERR_ARG, "null argument");
    AperPlan p;
    if (const char* msg = plan_apertures(h_jobs, n, h_factors, K, MH, MW, d_map != nullptr, h_jobs != nullptr, h_out != nullptr, p))
        return fail(c, CY_ERR_ARG, msg);
    if (n == 0) return CY_OK;
    TimedLaunch t(c, stream);
    ApertureArgs a{};
    a.map = d_map; a.rms = d_rms; a.MH = MH; a.MW = MW; a.n = n; a.K = K;
    a.jobs = t.upload(p.jobs.data(), p.jobs.size());
    a.out = t.scratch<double>((size_t)n * CY_APER_FIELDS);
    t.download(h_out, a.out, (size_t)n * CY_APER_FIELDS);
    return t.run(STEP_APERTURE, [&](hipStream_t s) { return launch_apertures(a, s); });
}

int cy_fit_peaks(cy_ctx* c, const float* d_map, int MH, int MW, const double* h_jobs, int n, int max_iter, double* h_out, void* stream) {
    if (!c) return fail(c, CY_ERR_ARG, "null argument");
    PeakFitPlan p;
    if (const char* msg = plan_peak_fits(h_jobs, n, max_iter, MH, MW, d_map != nullptr, h_out != nullptr, p)) return fail(c, CY_ERR_ARG, msg);
    if (n == 0) return CY_OK;
    std::vector<double> got(p.run.size() * CY_PFIT_FIELDS);
    if (!p.run.empty()) {
        TimedLaunch t(c, stream);
        PeakFitArgs a{};
        a.map = d_map; a.MH = MH; a.MW = MW; a.n = n; a.nrun = (int)p.run.size(); a.max_iter = max_iter;
        a.jobs = t.upload(p.jobs.data(), p.jobs.size());
        a.run = t.upload(p.run.data(), p.run.size());
        a.out = t.scratch<double>(got.size());
        t.download(got.data(), a.out, got.size());
        const int rc = t.run(STEP_PEAKFIT, [&](hipStream_t s) { return launch_peak_fits(a, s); });
        if (rc != CY_OK) return rc;                                            // h_out as it was
    }
    size_t next = 0;                                                           // p.run is in increasing job index
    for (int i = 0; i < n; ++i) {
        const bool ran = next < p.run.size() && p.run[next] == i;
        peak_fit_row(p.jobs[(size_t)i], h_jobs + (size_t)i * CY_PFIT_JOB_FIELDS, ran ? &got[next * CY_PFIT_FIELDS] : nullptr,
                     h_out + (size_t)i * CY_PFIT_FIELDS);
        next += ran;
    }
    return CY_OK;
}

int cy_fit_peak_groups(cy_ctx* c, const float* d_map, int MH, int MW, const double* h_jobs, int n, double link, int max_iter, double* h_out,
                       void* stream) {
    if (!c) return fail(c, CY_ERR_ARG, "null argument");
    PeakGroupPlan p;
    if (const char* msg = plan_peak_groups(h_jobs, n, link, max_iter, MH, MW, d_map != nullptr, h_out != nullptr, p)) return fail(c, CY_ERR_ARG, msg);
    if (n == 0) return CY_OK;
    std::vector<double> got(p.groups.size() * CY_BLEND_MAX_MEMBERS * CY_PGRP_FIELDS);
    if (!p.groups.empty()) {
        TimedLaunch t(c, stream);
        PeakGroupArgs a{};
        a.map = d_map; a.MH = MH; a.MW = MW; a.n = n; a.ngroups = (int)p.groups.size(); a.max_iter = max_iter;
        a.jobs = t.upload(p.fits.jobs.data(), p.fits.jobs.size());
        a.groups = t.upload(p.groups.data(), p.groups.size());
        a.out = t.zeros<double>(got.size());                                   // the kernel writes the members' rows only
        t.download(got.data(), a.out, got.size());
        const int rc = t.run(STEP_PEAKGROUP, [&](hipStream_t s) { return launch_peak_groups(a, s); });
        if (rc != CY_OK) return rc;                                            // h_out as it was
    }
    std::memcpy(h_out, p.rows.data(), p.rows.size() * sizeof(double));
    peak_group_rows(p, h_jobs, got.data(), h_out);
    return CY_OK;
}

int cy_disc_residuals(cy_ctx* c, const float* d_map, const float* d_model, int MH, int MW, const double* h_jobs, int n, double* h_out,
                      void* stream) {
    if (!c) return fail(c, CY_ERR_ARG, "null argument");
    PeakFitPlan p;                                                             // the planner of cy_fit_peaks as it stands; no iteration here: max_iter 1
    if (const char* msg = plan_peak_fits(h_jobs, n, 1, MH, MW, d_map != nullptr, h_out != nullptr, p)) return fail(c, CY_ERR_ARG, msg);
    if (n == 0) return CY_OK;
    std::vector<double> got(p.run.size() * CY_DRES_FIELDS);
    if (!p.run.empty()) {
        TimedLaunch t(c, stream);
        DiscResidualArgs a{};
        a.map = d_map; a.model = d_model; a.MH = MH; a.MW = MW; a.n = n; a.nrun = (int)p.run.size();
        a.jobs = t.upload(p.jobs.data(), p.jobs.size());
        a.run = t.upload(p.run.data(), p.run.size());
        a.out = t.scratch<double>(got.size());
        t.download(got.data(), a.out, got.size());
        const int rc = t.run(STEP_DISCRES, [&](hipStream_t s) { return launch_disc_residuals(a, s); });
        if (rc != CY_OK) return rc;                                            // h_out as it was
    }
    size_t next = 0;                                                           // p.run is in increasing job index
    for (int i = 0; i < n; ++i) {
        const bool ran = next < p.run.size() && p.run[next] == i;
        disc_residual_row(p.jobs[(size_t)i], ran ? &got[next * CY_DRES_FIELDS] : nullptr, h_out + (size_t)i * CY_DRES_FIELDS);
        next += ran;
    }
    return CY_OK;
}

int cy_forced_fit(cy_ctx* c, const float* d_map, const float* d_rms, int MH, int MW, const double* h_jobs, int n, double nsigma, int fit_bkg,
                  double* h_out, void* stream) {
#pragma clang fp contract(off)          // nsigma * nsigma is rounded once
    if (!c) return fail(c, CY_ERR_ARG, "null argument");
    ForcedPlan p;
    if (const char* msg = plan_forced(h_jobs, n, nsigma, fit_bkg, MH, MW, d_map != nullptr, h_out != nullptr, p)) return fail(c, CY_ERR_ARG, msg);
    if (n == 0) return CY_OK;
    std::vector<double> got(p.run.size() * CY_FORCED_FIELDS);
    if (!p.run.empty()) {
        TimedLaunch t(c, stream);
        ForcedArgs a{};
        a.map = d_map; a.rms = d_rms; a.MH = MH; a.MW = MW; a.n = n; a.nrun = (int)p.run.size();
        a.ns2 = nsigma * nsigma; a.fit_bkg = fit_bkg;
        a.jobs = t.upload(p.jobs.data(), p.jobs.size());
        a.run = t.upload(p.run.data(), p.run.size());
        a.out = t.scratch<double>(got.size());
        t.download(got.data(), a.out, got.size());
        const int rc = t.run(STEP_FORCED, [&](hipStream_t s) { return launch_forced(a, s); });
        if (rc != CY_OK) return rc;                                            // h_out as it was
    }
    size_t next = 0;                                                           // p.run is in increasing job index
    for (int i = 0; i < n; ++i) {
        const bool ran = next < p.run.size() && p.run[next] == i;
        forced_row(p.jobs[(size_t)i], fit_bkg, ran ? &got[next * CY_FORCED_FIELDS] : nullptr, h_out + (size_t)i * CY_FORCED_FIELDS);
        next += ran;
    }
    return CY_OK;
}

// kernel time of the last call of a measurement step that launched (hipEvents around the launch); -1 before it and after a failed call
static int step_kernel_ms(const cy_ctx* c, MeasureStep step, double* out_ms) {
    if (!c || !out_ms) return CY_ERR_ARG;
    *out_ms = c->step_ms[step];
    return CY_OK;
}
int cy_measure_kernel_ms(const cy_ctx* c, double* out_ms) { return step_kernel_ms(c, STEP_SOURCES, out_ms); }
int cy_islands_kernel_ms(const cy_ctx* c, double* out_ms) { return step_kernel_ms(c, STEP_ISLANDS, out_ms); }
int cy_deblend_kernel_ms(const cy_ctx* c, double* out_ms) { return step_kernel_ms(c, STEP_DEBLEND, out_ms); }
int cy_fit_kernel_ms(const cy_ctx* c, double* out_ms) { return step_kernel_ms(c, STEP_FIT, out_ms); }
int cy_blend_kernel_ms(const cy_ctx* c, double* out_ms) { return step_kernel_ms(c, STEP_BLEND, out_ms); }
int cy_background_kernel_ms(const cy_ctx* c, double* out_ms) { return step_kernel_ms(c, STEP_BACKGROUND, out_ms); }
int cy_render_kernel_ms(const cy_ctx* c, double* out_ms) { return step_kernel_ms(c, STEP_RENDER, out_ms); }
int cy_residual_kernel_ms(const cy_ctx* c, double* out_ms) { return step_kernel_ms(c, STEP_RESIDUAL, out_ms); }
int cy_peaks_kernel_ms(const cy_ctx* c, double* out_ms) { return step_kernel_ms(c, STEP_PEAKS, out_ms); }
int cy_atrous_kernel_ms(const cy_ctx* c, double* out_ms) { return step_kernel_ms(c, STEP_ATROUS, out_ms); }
int cy_aperture_kernel_ms(const cy_ctx* c, double* out_ms) { return step_kernel_ms(c, STEP_APERTURE, out_ms); }
int cy_peakfit_kernel_ms(const cy_ctx* c, double* out_ms) { return step_kernel_ms(c, STEP_PEAKFIT, out_ms); }
int cy_peakgroup_kernel_ms(const cy_ctx* c, double* out_ms) { return step_kernel_ms(c, STEP_PEAKGROUP, out_ms); }
int cy_disc_residual_kernel_ms(const cy_ctx* c, double* out_ms) { return step_kernel_ms(c, STEP_DISCRES, out_ms); }
int cy_forced_kernel_ms(const cy_ctx* c, double* out_ms) { return step_kernel_ms(c, STEP_FORCED, out_ms); }

int cy_expand_background(cy_ctx* c, const double* h_mesh, int ncy, int ncx, int cell, int MH, int MW, float* d_bkg, float* d_rms, void* stream) {
    if (!c) return fail(c, CY_ERR_ARG, "null argument");
    if (MH <= 0 || MW <= 0 || cell < BKG_CELL_MIN || cell > BKG_CELL_MAX) return fail(c, CY_ERR_ARG, "MH, MW > 0 and 4 <= cell <= 4096 required");
    if (!h_mesh || (!d_bkg && !d_rms)) return fail(c, CY_ERR_ARG, "null argument");
    if ((long long)MH * MW >= (1LL << 31)) return fail(c, CY_ERR_ARG, "image of 2^31 pixels or more");
    if (ncx != (MW + cell - 1) / cell || ncy != (MH + cell - 1) / cell) return fail(c, CY_ERR_ARG, "mesh shape disagrees with MH, MW and cell");
    const size_t bytes = (size_t)ncy * ncx * 2 * sizeof(double);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    DevOwner sc;
    void* d_mesh = nullptr;
    HIPCHK(c, sc.alloc(bytes, &d_mesh));
    hipError_t e = hipMemcpyAsync(d_mesh, h_mesh, bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        BackgroundExpandArgs a{};
        a.mesh = reinterpret_cast<const double*>(d_mesh); a.ncy = ncy; a.ncx = ncx; a.cell = cell; a.MH = MH; a.MW = MW;
        a.bkg = d_bkg; a.rms = d_rms;
        e = launch_background_expand(a, st);
    }
    return entry_done(c, e, st);
}

// ---- test-time augmentation -------------------------------------------------------------------
// ultralytics DetectionModel._predict_augment: scales (1, 0.83, 0.67), flips (none, left-right, none), gs = 32; sizes in double as
// Python computes them (int(h * s) truncates, ceil(h * s / gs) * gs pads); _clip_augmented with g = 1 + 4 + 16 drops the stride-32
// anchors of view 0 and the stride-8 anchors of view 2.
static const double AUG_SCALE[3] = {1.0, 0.83, 0.67};
static const int AUG_FLIP[3] = {0, 1, 0};

int cy_augment_geometry(int H, int W, cy_augment_geom* o) {
    if (!o || H < 32 || W < 32 || H % 32 || W % 32) return CY_ERR_ARG;
    int off = 0;
    for (int k = 0; k < 3; ++k) {
        cy_augment_view& v = o->v[k];
        const double s = AUG_SCALE[k];
        v.scale = s; v.flip = AUG_FLIP[k];
        v.ch = (int)(H * s); v.cw = (int)(W * s);
        v.Hp = (int)std::ceil(H * s / 32.0) * 32; v.Wp = (int)std::ceil(W * s / 32.0) * 32;
        v.A = cy_num_anchors(v.Hp, v.Wp);
        const int g = v.A / 21;                                  // stride-32 cells (views are multiples of 32: A = 21 g)
        v.lo = k == 2 ? g * 16 : 0;
        v.hi = k == 0 ? v.A - g : v.A;
        v.off = off;
        off += v.hi - v.lo;
    }
    o->total = off;
    return CY_OK;
}

int cy_enable_augment(cy_ctx* c) {
    if (!c || !c->loaded) return fail(c, CY_ERR_STATE, "weights not loaded");
    if (c->aug) return CY_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const cy_config& g = c->cfg;
    cy_augment_geom ag;
    if (cy_augment_geometry(g.max_h, g.max_w, &ag)) return fail(c, CY_ERR_ARG, "bad context geometry");
    const size_t es = esize(c->prec), Bm = g.max_batch;
    // candidates per tile: as the plain path (cap = anchors of the largest input; NMS keeps the top max_nms by score), over the
    // concatenation of the three views; an explicit max_cand is honoured
    if (ag.total > CY_MAX_CAND)
        return fail(c, CY_ERR_ARG, "test-time augmentation of a " + std::to_string(g.max_h) + " x " + std::to_string(g.max_w) +
                                   " context: " + std::to_string(ag.total) + " concatenated anchors, more than CY_MAX_CAND = " +
                                   std::to_string(CY_MAX_CAND) + " (16-bit index of the NMS sort key)");
    c->acap = cand_capacity(g.max_cand > 0 ? g.max_cand : ag.total);
    c->acap_pow2 = 1; while (c->acap_pow2 < c->acap) c->acap_pow2 <<= 1;
    const int nc = c->plan.nc;
    c->aug_mem.reset();                                     // (what an earlier attempt that failed half-way left)
    for (auto& b : c->ab) {
        b = cy_ctx::AugBufs();
        for (int k = 0; k < 2; ++k) {
            const cy_augment_view& v = ag.v[k + 1];
            HIPCHK(c, c->aug_mem.alloc(Bm * v.Hp * v.Wp * 4 * es, &b.view[k]));
            HIPCHK(c, c->aug_mem.alloc(Bm * v.A * (64 + nc) * sizeof(float), &b.pred[k]));
        }
        if (c->prec == PREC_F16) HIPCHK(c, c->aug_mem.alloc(Bm * g.max_h * g.max_w * 4 * sizeof(float), &b.src32));
        HIPCHK(c, c->aug_mem.alloc(Bm * c->acap * 6 * sizeof(float), &b.cand));
        HIPCHK(c, c->aug_mem.alloc(Bm * c->acap * sizeof(int), &b.cand_anchor));
        HIPCHK(c, c->aug_mem.alloc(Bm * c->acap_pow2 * sizeof(uint64_t), &b.keys));
    }
    c->aug = true;
    return CY_OK;
}

// the view kernel on (src, H, W) -> the views named (view 0 only in the fp16 context: its fp16 copy of src)
static int augment_pack_on(cy_ctx* c, const float* d_src, int B, int H, int W, void* d_view0, void* d_view1, void* d_view2,
                           hipStream_t s) {
    cy_augment_geom ag;
    if (cy_augment_geometry(H, W, &ag)) return fail(c, CY_ERR_ARG, "bad view-0 size (multiples of 32 required)");
    AugPackArgs a{};
    a.src = d_src; a.B = B; a.H = H; a.W = W; a.out_prec = io_prec(c->prec);
    void* outs[3] = {d_view0, d_view1, d_view2};
    for (int k = 0; k < 3; ++k) {
        if (!outs[k]) continue;
        const cy_augment_view& v = ag.v[k];
        a.v[a.nview++] = AugView{outs[k], v.ch, v.cw, v.Hp, v.Wp, v.flip};
    }
    if (a.nview == 0) return CY_OK;
    HIPCHK(c, launch_augment_pack(a, s));
    return CY_OK;
}

int cy_augment_pack(cy_ctx* c, const float* d_src, int B, int H, int W, void* d_view0, void* d_view1, void* d_view2, void* stream) {
    if (!c || !c->loaded) return fail(c, CY_ERR_STATE, "weights not loaded");
    if (!c->aug) return fail(c, CY_ERR_STATE, "test-time augmentation not enabled on this context (cy_enable_augment)");
    if (!d_src || !d_view1 || !d_view2 || B < 1 || B > c->cfg.max_batch || H > c->cfg.max_h || W > c->cfg.max_w)
        return fail(c, CY_ERR_ARG, "bad arguments");
    if (d_view0 && c->prec != PREC_F16) return fail(c, CY_ERR_ARG, "view 0 is the source itself outside the fp16 context");
    return augment_pack_on(c, d_src, B, H, W, d_view0, d_view1, d_view2, (hipStream_t)stream);
}

// decode of the three views + NMS over the concatenation + scale_boxes, into the given outputs, on the context's buffer set
static int decode_nms_aug_on(cy_ctx* c, const float* const* d_pred, int B, int H, int W, int h0, int w0, float conf, float iou,
                             float* d_det, int* d_det_anchor, int* d_count, hipStream_t s) {
    cy_augment_geom ag;
    if (cy_augment_geometry(H, W, &ag)) return fail(c, CY_ERR_ARG, "bad view-0 size (multiples of 32 required)");
    AugDecodeArgs d{};
    d.nview = 3; d.B = B; d.nc = c->plan.nc; d.conf = conf; d.W0 = (float)W;
    for (int k = 0; k < 3; ++k) {
        const cy_augment_view& v = ag.v[k];
        AugDecodeView& q = d.v[k];
        q.pred = d_pred[k]; q.A = v.A; q.s = (float)v.scale; q.flip = v.flip; q.lo = v.lo; q.hi = v.hi; q.off = v.off;
        for (int l = 0; l < 3; ++l) { q.lvl_h[l] = v.Hp >> (3 + l); q.lvl_w[l] = v.Wp >> (3 + l); }
    }
    d.cand = c->AB().cand; d.cand_anchor = c->AB().cand_anchor; d.cand_count = c->S().cand_count; d.cap = c->acap;
    HIPCHK(c, hipMemsetAsync(c->S().cand_count, 0, B * sizeof(int), s));
    HIPCHK(c, launch_decode_augmented(d, s));
    return nms_on(c, c->AB().cand, c->AB().cand_anchor, c->AB().keys, c->acap, B, H, W, h0, w0, iou, d_det, d_det_anchor, d_count, s);      // (scale_boxes against view 0)
}

int cy_decode_nms_augmented(cy_ctx* c, const float* d_pred0, const float* d_pred1, const float* d_pred2, int B, int H, int W,
                            int h0, int w0, float conf, float iou, float* d_det, int* d_det_anchor, int* d_count, void* stream) {
    if (!c || !c->loaded) return fail(c, CY_ERR_STATE, "weights not loaded");
    if (!c->aug) return fail(c, CY_ERR_STATE, "test-time augmentation not enabled on this context (cy_enable_augment)");
    if (!d_pred0 || !d_pred1 || !d_pred2 || !d_det || !d_det_anchor || !d_count || B < 1 || B > c->cfg.max_batch)
        return fail(c, CY_ERR_ARG, "bad arguments");
    if (H > c->cfg.max_h || W > c->cfg.max_w) return fail(c, CY_ERR_ARG, "view 0 exceeds max_h/max_w of the context");
    const float* preds[3] = {d_pred0, d_pred1, d_pred2};
    return decode_nms_aug_on(c, preds, B, H, W, h0, w0, conf, iou, d_det, d_det_anchor, d_count, (hipStream_t)stream);
}

int cy_detect_tiles_augmented(cy_ctx* c, const float* d_mosaic, int MH, int MW, const int* h_tiles, int B, int th, int tw,
                              int imgsz, const cy_preproc_cfg* cfg, float conf, float iou, double soft, double hard, int augment,
                              float* d_out, int* d_out_count, int* d_status, void* stream) {
    if (!augment)
        return cy_detect_tiles(c, d_mosaic, MH, MW, h_tiles, B, th, tw, imgsz, cfg, conf, iou, soft, hard, d_out, d_out_count, d_status, stream);
    // cy_detect_tiles' pipeline (pipeline_batch), with three views per batch: the view kernel runs on the preprocessing stream
    // behind the letterbox pack, the three forwards back to back on the forward stream, and the augmented decode + NMS + IoU merge
    // on the post-processing stream.  The view buffers belong to the buffer set, so the events that order a set's reuse order
    // them too, and plain and augmented calls mix freely in one unflushed pipeline.
    if (!c || !c->loaded) return fail(c, CY_ERR_STATE, "weights not loaded");
    if (!c->aug) return fail(c, CY_ERR_STATE, "test-time augmentation not enabled on this context (cy_enable_augment)");
    cy_letterbox lb;
    if (cy_letterbox_geometry(th, tw, imgsz, &lb)) return fail(c, CY_ERR_ARG, "bad tile/imgsz");
    if (lb.H > c->cfg.max_h || lb.W > c->cfg.max_w) return fail(c, CY_ERR_ARG, "letterboxed tile exceeds max_h/max_w of the context");
    cy_augment_geom ag;
    if (cy_augment_geometry(lb.H, lb.W, &ag)) return fail(c, CY_ERR_ARG, "bad letterboxed size");
    return pipeline_batch(c, d_mosaic, B, conf, soft, hard, d_out, d_out_count, stream,
        [&](hipStream_t s) {
            // view 0 = the letterboxed batch; in the fp16 context it is packed in fp32 first, and the view kernel writes all three views
            const bool f16 = c->prec == PREC_F16;
            float* src32 = f16 ? c->AB().src32 : (float*)c->S().netin;
            const int rc = preproc_as(c, d_mosaic, MH, MW, h_tiles, B, th, tw, imgsz, cfg, src32, PREC_F32, d_status, s);
            return rc ? rc : augment_pack_on(c, src32, B, lb.H, lb.W, f16 ? c->S().netin : nullptr, c->AB().view[0], c->AB().view[1], s);
        },
        [&](auto&& fwd) {
            const void* vin[3] = {c->S().netin, c->AB().view[0], c->AB().view[1]};
            float* vpred[3] = {c->S().pred, c->AB().pred[0], c->AB().pred[1]};
            int rc = CY_OK;
            for (int k = 0; k < 3 && !rc; ++k) rc = fwd(vin[k], ag.v[k].Hp, ag.v[k].Wp, vpred[k]);
            return rc;
        },
        [&](hipStream_t s) {
            const float* preds[3] = {c->S().pred, c->AB().pred[0], c->AB().pred[1]};
            return decode_nms_aug_on(c, preds, B, lb.H, lb.W, th, tw, conf, iou, c->S().det, c->S().det_anchor, c->S().det_count, s);
        });
}

}  // extern "C"
