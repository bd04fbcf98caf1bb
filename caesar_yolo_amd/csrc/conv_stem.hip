// Layer 0 of the network, Conv(3, C, 3, 2) on the NHWC4 input, and its fusion with the first down convolution (layer 1).
#include "cy_kernels.h"
#include "cy_conv_dev.h"
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace cy {

// ------------------------------------------------------------------------------------------------ stem
// Layer 0: Conv(3, C, 3, 2) on the NHWC4 network input.  K = 27 is too small for the matrix cores to matter; the
// layer is bound by its 64-channel output write.  One thread = one output pixel x 16 output channels.
template <typename T, bool SPLIT = false>      // SPLIT (fp16x3 context): T = float input, output as fp16 high / low halves
__global__ __launch_bounds__(256) void stem_kernel(const StemArgs a) {
    __shared__ float w[27 * 64];
    __shared__ float bs[64];
    const int co_blocks = a.Cout / 16;
    for (int i = threadIdx.x; i < 27 * a.Cout; i += 256) w[i] = a.w[i];
    for (int i = threadIdx.x; i < a.Cout; i += 256) bs[i] = a.bias[i];
    __syncthreads();
    const long total = (long)a.B * a.Ho * a.Wo * co_blocks;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int cb = (int)(idx % co_blocks);
        const long pix = idx / co_blocks;
        const int wo = (int)(pix % a.Wo);
        const int ho = (int)((pix / a.Wo) % a.Ho);
        const int b = (int)(pix / ((long)a.Wo * a.Ho));
        float x[27];
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int hi = ho * 2 - 1 + kh, wi = wo * 2 - 1 + kw;
                const bool ok = (unsigned)hi < (unsigned)a.Hi && (unsigned)wi < (unsigned)a.Wi;
                typedef T vec4 __attribute__((ext_vector_type(4)));
                vec4 pv = {(T)0, (T)0, (T)0, (T)0};
                if (ok) pv = *reinterpret_cast<const vec4*>(reinterpret_cast<const T*>(a.in) +
                                                            (((long)b * a.Hi + hi) * a.Wi + wi) * 4);
#pragma unroll
                for (int c = 0; c < 3; ++c) x[(kh * 3 + kw) * 3 + c] = (float)pv[c];
            }
        float acc[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0.0f;
#pragma unroll
        for (int t = 0; t < 27; ++t)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] = fmaf(x[t], w[t * a.Cout + cb * 16 + j], acc[j]);
        if constexpr (SPLIT) {
            float v16[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) v16[j] = silu_fast(acc[j] + bs[cb * 16 + j]);
            store_split16(reinterpret_cast<f16*>(a.out) + pix * a.out_ct + a.out_coff + cb * 16, a.out_lo, v16);
            continue;
        }
        T* dst = reinterpret_cast<T*>(a.out) + pix * a.out_ct + a.out_coff + cb * 16;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float v = acc[j] + bs[cb * 16 + j];
            dst[j] = (T)((sizeof(T) == 2) ? silu_fast(v) : silu_exact(v));
        }
    }
}

// The same layer with FOUR horizontally adjacent output pixels per thread (maps whose width is a multiple of 4): the form above reads
// every weight from LDS for a single FMA and is bound by that (16-byte LDS reads for 4 lanes' worth of FMAs: 20 TFLOP/s of fp32 in the
// fp16x3 context, 4.9 % of its forward pass); here a weight read feeds four pixels, and the four pixels' 3 x 9 input columns are loaded
// once (27 loads instead of 36).  Per output value the FMA chain is the one above (taps ascending, fmaf), so results are bit-identical
// (tests/test_gpu_forward.py::test_stem_four_pixel_form_is_bit_identical).  CY_STEM_QUAD=0: the form above.
template <typename T, bool SPLIT = false>
__global__ __launch_bounds__(256) void stem_quad_kernel(const StemArgs a) {
    __shared__ __attribute__((aligned(16))) float w[27 * 64];
    __shared__ float bs[64];
    const int co_blocks = a.Cout / 16, wq = a.Wo >> 2;
    for (int i = threadIdx.x; i < 27 * a.Cout; i += 256) w[i] = a.w[i];
    for (int i = threadIdx.x; i < a.Cout; i += 256) bs[i] = a.bias[i];
    __syncthreads();
    const long total = (long)a.B * a.Ho * wq * co_blocks;
    typedef T vec4 __attribute__((ext_vector_type(4)));
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int cb = (int)(idx % co_blocks);
        const long q = idx / co_blocks;
        const int wo0 = (int)(q % wq) * 4;
        const int ho = (int)((q / wq) % a.Ho);
        const int b = (int)(q / ((long)wq * a.Ho));
        float acc[4][16];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[p][j] = 0.0f;
#pragma unroll 1
        for (int kh = 0; kh < 3; ++kh) {
            const int hi = ho * 2 - 1 + kh;
            const bool row_ok = (unsigned)hi < (unsigned)a.Hi;
            const int hic = hi < 0 ? 0 : (hi >= a.Hi ? a.Hi - 1 : hi);
            vec4 r[9];
#pragma unroll
            for (int ci = 0; ci < 9; ++ci) {
                const int wi = wo0 * 2 - 1 + ci;
                // loaded at clamped coordinates and zeroed by a select (a conditional load is a branch with a full wait behind it)
                const int wic = wi < 0 ? 0 : (wi >= a.Wi ? a.Wi - 1 : wi);
                const vec4 t = *reinterpret_cast<const vec4*>(reinterpret_cast<const T*>(a.in) + (((long)b * a.Hi + hic) * a.Wi + wic) * 4);
                r[ci] = (row_ok && (unsigned)wi < (unsigned)a.Wi) ? t : vec4{(T)0, (T)0, (T)0, (T)0};
            }
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    asm volatile("" ::: "memory");           // weights of one tap at a time (hoisted, all 432 of them would live in registers)
                    const float* wr = w + ((kh * 3 + kw) * 3 + c) * a.Cout + cb * 16;
                    float wv[16];
#pragma unroll
                    for (int j4 = 0; j4 < 4; ++j4) {
                        const f32x4 t4 = *reinterpret_cast<const f32x4*>(wr + 4 * j4);
                        wv[4 * j4] = t4[0]; wv[4 * j4 + 1] = t4[1]; wv[4 * j4 + 2] = t4[2]; wv[4 * j4 + 3] = t4[3];
                    }
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const float xv = (float)r[2 * p + kw][c];
#pragma unroll
                        for (int j = 0; j < 16; ++j) acc[p][j] = fmaf(xv, wv[j], acc[p][j]);
                    }
                }
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const long pix = ((long)b * a.Ho + ho) * a.Wo + wo0 + p;
            if constexpr (SPLIT) {
                float v16[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) v16[j] = silu_fast(acc[p][j] + bs[cb * 16 + j]);
                store_split16(reinterpret_cast<f16*>(a.out) + pix * a.out_ct + a.out_coff + cb * 16, a.out_lo, v16);
            } else {
                T* dst = reinterpret_cast<T*>(a.out) + pix * a.out_ct + a.out_coff + cb * 16;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const float v = acc[p][j] + bs[cb * 16 + j];
                    dst[j] = (T)((sizeof(T) == 2) ? silu_fast(v) : silu_exact(v));
                }
            }
        }
    }
}

// fp16 context: the stem as a K=32 (27 padded) MFMA GEMM.  A wave turns 16 output pixels x 64 channels per step:
// the 64x32 weight panel lives in registers for the whole kernel (A operand), each lane gathers the 8 im2col values of
// its (pixel, k-chunk) from the NHWC4 image with the halo zeroed, and stores 16 contiguous channels of its pixel.
// Bound by the 64-channel output write (8 MB per 512x512 tile), not by arithmetic.
__global__ __launch_bounds__(256) void stem_mfma_kernel(const StemArgs a, const f16* __restrict__ wpk) {
    const int lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
    f16x8 wb[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) wb[ni] = *reinterpret_cast<const f16x8*>(wpk + (ni * 16 + fr) * 32 + fq * 8);
    float bv[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) bv[j] = a.bias[fq * 16 + j];
    // k = 8*fq + j  ->  tap = k/3 (kh = tap/3, kw = tap%3), channel = k%3; k >= 27 is zero padding
    int dh[8], dw[8], dc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 8 * fq + j, tap = k / 3;
        dh[j] = tap / 3 - 1; dw[j] = tap % 3 - 1; dc[j] = k < 27 ? k % 3 : -1;
    }
    const long ngroups = ((long)a.B * a.Ho * a.Wo + 15) / 16;
    const long npix = (long)a.B * a.Ho * a.Wo;
    const int wave_id = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwaves = gridDim.x * 4;
    const f16* in = reinterpret_cast<const f16*>(a.in);
    const bool rows16 = (a.Wo & 15) == 0;                   // a group of 16 pixels never straddles an image row: the
    const int gw = a.Wo >> 4;                               // (b, ho, wo) split is wave-uniform -> scalar divisions
    for (int g = wave_id; g < (int)ngroups; g += nwaves) {
        const long pix = (long)g * 16 + fr;
        const bool pv = pix < npix;
        int wo, ho, b;
        if (rows16) {
            const int row = g / gw;                          // = b*Ho + ho (uniform)
            wo = (g - row * gw) * 16 + fr;
            b = row / a.Ho;
            ho = row - b * a.Ho;
        } else {
            wo = (int)(pix % a.Wo); ho = (int)((pix / a.Wo) % a.Ho); b = (int)(pix / ((long)a.Wo * a.Ho));
        }
        f16x8 xa;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int hi = 2 * ho + dh[j], wi = 2 * wo + dw[j];
            const bool ok = pv && dc[j] >= 0 && (unsigned)hi < (unsigned)a.Hi && (unsigned)wi < (unsigned)a.Wi;
            xa[j] = ok ? in[(((long)b * a.Hi + hi) * a.Wi + wi) * 4 + dc[j]] : (f16)0.0f;
        }
        f32x4 acc[4];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            acc[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
            acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb[ni], xa, acc[ni], 0, 0, 0);
        }
        if (pv) {
            f16x8 o0, o1;
            float v16[16];
            bias_act16(acc[0], acc[1], acc[2], acc[3], bv, true, v16);
#pragma unroll
            for (int j = 0; j < 8; ++j) { o0[j] = (f16)v16[j]; o1[j] = (f16)v16[8 + j]; }
            f16* dst = reinterpret_cast<f16*>(a.out) + pix * a.out_ct + a.out_coff + fq * 16;
            *reinterpret_cast<f16x8*>(dst) = o0;
            *reinterpret_cast<f16x8*>(dst + 8) = o1;
        }
    }
}

hipError_t launch_stem(Precision p, const StemArgs& a, hipStream_t s) {
    if (a.Cout > 64 || a.Cout % 16) return hipErrorInvalidValue;
    if (p == PREC_F16 && a.Cout == 64 && a.wpk) {
        const long ngroups = ((long)a.B * a.Ho * a.Wo + 15) / 16;
        const int grid = (int)((ngroups + 3) / 4 < 4096 ? (ngroups + 3) / 4 : 4096);
        hipLaunchKernelGGL(stem_mfma_kernel, dim3(grid), dim3(256), 0, s, a, reinterpret_cast<const f16*>(a.wpk));
        return hipGetLastError();
    }
    if (p != PREC_F16 && a.Wo % 4 == 0 && env_knob("CY_STEM_QUAD", 1)) {      // four pixels per thread (bit-identical; read per call: tests)
        const long total4 = (long)a.B * a.Ho * (a.Wo / 4) * (a.Cout / 16);
        const int grid4 = (int)((total4 + 255) / 256 < 16384 ? (total4 + 255) / 256 : 16384);
        if (p == PREC_F16X3) hipLaunchKernelGGL((stem_quad_kernel<float, true>), dim3(grid4), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(stem_quad_kernel<float>, dim3(grid4), dim3(256), 0, s, a);
        return hipGetLastError();
    }
    const long total = (long)a.B * a.Ho * a.Wo * (a.Cout / 16);
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    if (p == PREC_F16) hipLaunchKernelGGL(stem_kernel<f16>, dim3(grid), dim3(256), 0, s, a);
    else if (p == PREC_F16X3) hipLaunchKernelGGL((stem_kernel<float, true>), dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(stem_kernel<float>, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

// packed stem weights for stem_mfma_kernel: [64 rows, permuted like pack_weights][32] fp16, k = (kh*3+kw)*3 + c
void pack_stem_weights(const float* W, int cout, void* dst) {
    f16* o = reinterpret_cast<f16*>(dst);
    for (int row = 0; row < 64; ++row) {
        const int ni = (row >> 4) & 3, rr = row & 15;
        const int n = (rr >> 2) * 16 + ni * 4 + (rr & 3);
        for (int k = 0; k < 32; ++k) {
            float v = 0.0f;
            if (n < cout && k < 27) { const int tap = k / 3, c = k % 3; v = W[((size_t)n * 3 + c) * 9 + tap]; }
            o[row * 32 + k] = (f16)v;
        }
    }
}

// ------------------------------------------------------------------------------------------------ stem + first down conv
// model.0 (3x3 s2, 3 -> 64) and model.1 (3x3 s2, 64 -> 128) fused.  As separate layers they are the two slowest launches
// of the forward pass and both HBM-bound: the 64-channel half-resolution map is 8.4 MB per 512x512 tile, written once and
// read back ~1.6 times (the nine taps of a stride-2 conv come back long after each other: the L2 does not hold them).
// Here a workgroup owns 8 x 32 output pixels of model.1 x all 128 channels:
//   phase 1: the 17 x 65 stem pixels under them are computed on the matrix cores (K = 9 taps x 4 NHWC channels = 36,
//            padded to 64: a lane's k-chunk is two whole input pixels = two 8-byte loads) and written, bias + SiLU applied,
//            to LDS as fp16 [row][64 ch] (138 KiB).  Stem pixels outside the map are model.1's zero padding: zeros.
//            Rows are split by column parity (even columns first), so the 16 pixels of a stride-2 fragment are 16
//            CONSECUTIVE LDS rows and the usual chunk ^ (row & 7) swizzle keeps ds_read_b128 conflict-free.
//   phase 2: 9 taps x 2 K-halves; a wave owns 64 px x 64 ch, reads its pixel fragments from LDS and its weight fragments
//            straight from global memory (the 147 KB panel is L2-resident; no LDS left for it), one step ahead.
// HBM traffic: input (0.5 MB/tile x 1.08 halo) + output (4.2 MB/tile) instead of + 8.4 MB written + >= 8.4 MB read.
// Measured at batch 256 (CY_SD_DBG phase switches): 1.38 ms against 1.03 + 1.13 ms for the two layers; phase 1 0.70 ms (one
// exposed gather latency + 144 SiLU per lane per tile), phase 2 0.39 ms, epilogue + stores 0.38 ms.  An 8 x 16-pixel variant
// with two workgroups per CU (72 KiB, 114 VGPRs) was no faster: its 8-MFMA steps are too short to cover the weight fetch.
constexpr int SD_TH = 8, SD_TW = 32, SD_PH = 2 * SD_TH + 1, SD_PW = 2 * SD_TW + 1, SD_EVEN = SD_TW + 1;
constexpr int SD_ROWS = SD_PH * SD_PW, SD_FRAGS = (SD_ROWS + 15) / 16, SD_LDS = SD_FRAGS * 16 * 128;

__device__ __forceinline__ u32x2 load_b64(__amdgpu_buffer_rsrc_t rs, unsigned voff) {
    return __builtin_amdgcn_raw_buffer_load_b64(rs, voff, 0, 0);
}

__global__ __launch_bounds__(512) void stem_down_kernel(const StemDownArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave & 1, wm = wave >> 1;
    const int tiles_x = (a.Wo + SD_TW - 1) / SD_TW, tiles_y = (a.Ho + SD_TH - 1) / SD_TH;
    int id = xcd_remap(blockIdx.x, gridDim.x);
    const int tx = id % tiles_x; id /= tiles_x;
    const int ty = id % tiles_y;
    const int b = id / tiles_y;
    const int oy0 = ty * SD_TH, ox0 = tx * SD_TW;
    const int sy0 = 2 * oy0 - 1, sx0 = 2 * ox0 - 1;          // stem-map coordinates of LDS pixel (0, 0)
    const auto rsi = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.in), 0, a.in_bytes, 0x00020000);
    const auto rsw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wgt32), 0, a.wgt32_bytes, 0x00020000);

    // weight fragments of step (tap, h): rows wn*64 + ni*16 + fr of chunk h, bytes fq*16.. ; cpad = 128 rows of 64 B
    constexpr int SD_RING = 4;                                // ring: fragments are requested three steps ahead (a ring of 8 measured
    f16x8 wa[SD_RING][4];                                     // 6 % slower: its 28 loads per lane up front delay phase 1's gathers)
    const unsigned wl = (unsigned)((wn * 64 + fr) * 64 + fq * 16);
    auto load_wa = [&](f16x8* dst, int step) {
        const int h = step & 1, tap = step >> 1;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) dst[ni] = __builtin_bit_cast(f16x8, load_b128(rsw, wl + ni * 1024, (h * 9 + tap) * 8192));
    };
#pragma unroll
    for (int st = 0; st < SD_RING - 1; ++st) load_wa(wa[st], st);      // in flight during phase 1

    if (!(a.dbg & 1)) {   // ---- phase 1: stem pixels -> LDS
        const f16* wp = reinterpret_cast<const f16*>(a.wpk2);
        f16x8 sw0[4], sw1[4];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            sw0[ni] = *reinterpret_cast<const f16x8*>(wp + (ni * 16 + fr) * 64 + fq * 8);
            sw1[ni] = *reinterpret_cast<const f16x8*>(wp + (ni * 16 + fr) * 64 + 32 + fq * 8);
        }
        float bv[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) bv[j] = a.bias0[fq * 16 + j];
        const int t0 = 2 * fq, t1 = 2 * fq + 1;              // the two taps of this lane's k-chunk; tap 8 rides in the second MFMA (fq = 0)
        const int dh0 = t0 / 3 - 1, dw0 = t0 % 3 - 1, dh1 = t1 / 3 - 1, dw1 = t1 % 3 - 1;
        const int d0 = (dh0 * a.Wi + dw0) * 8, d1 = (dh1 * a.Wi + dw1) * 8, d2 = (a.Wi + 1) * 8;
        constexpr int NG = (SD_FRAGS + 7) / 8;
        u32x2 q0[NG], q1[NG], q2[NG];
        unsigned inmask = 0;
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
            const int g = gi * 8 + wave, p = g * 16 + fr;
            const int sy = p / SD_PW, q = p - sy * SD_PW;
            const int sx = q < SD_EVEN ? 2 * q : 2 * (q - SD_EVEN) + 1;
            const int Y = sy0 + sy, X = sx0 + sx;
            const bool inmap = p < SD_ROWS && (unsigned)Y < (unsigned)a.H1 && (unsigned)X < (unsigned)a.W1;
            inmask |= inmap ? (1u << gi) : 0u;
            // input pixel (2Y + dh, 2X + dw): with Hi = 2*H1 and Wi = 2*W1 only the -1 row / column can fall outside
            const int hc = 2 * Y, wc = 2 * X;
            const int base = ((b * a.Hi + hc) * a.Wi + wc) * 8;
            const bool ok0 = inmap && ((hc + dh0) | (wc + dw0)) >= 0, ok1 = inmap && ((hc + dh1) | (wc + dw1)) >= 0;
            q0[gi] = load_b64(rsi, ok0 ? (unsigned)(base + d0) : CY_OOB);
            q1[gi] = load_b64(rsi, ok1 ? (unsigned)(base + d1) : CY_OOB);
            q2[gi] = load_b64(rsi, (inmap && fq == 0) ? (unsigned)(base + d2) : CY_OOB);
        }
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
            const int g = gi * 8 + wave;
            if (g >= SD_FRAGS) break;                         // wave-uniform
            const int p = g * 16 + fr;
            const bool inmap = (inmask >> gi) & 1u;
            // the fourth NHWC channel is padding: its weights are zero, and masking it keeps a stray NaN out of the sum
            const u32x4 u0 = {q0[gi].x, q0[gi].y & 0xFFFFu, q1[gi].x, q1[gi].y & 0xFFFFu};
            const u32x4 u1 = {q2[gi].x, q2[gi].y & 0xFFFFu, 0u, 0u};
            const f16x8 x0 = __builtin_bit_cast(f16x8, u0), x1 = __builtin_bit_cast(f16x8, u1);
            f32x4 acc[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(sw0[ni], x0, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(sw1[ni], x1, acc[ni], 0, 0, 0);
            }
            f16x8 o0, o1;
            float v16[16];
            bias_act16(acc[0], acc[1], acc[2], acc[3], bv, true, v16);
#pragma unroll
            for (int j = 0; j < 8; ++j) { o0[j] = (f16)v16[j]; o1[j] = (f16)v16[8 + j]; }
            const unsigned keep = inmap ? 0xFFFFFFFFu : 0u;   // a select on the packed result: a `?:` around silu becomes 16 branches
            const u32x4 k4 = {keep, keep, keep, keep};
            char* row = smem + p * 128;
            *reinterpret_cast<u32x4*>(row + (((2 * fq) ^ (p & 7)) << 4)) = __builtin_bit_cast(u32x4, o0) & k4;
            *reinterpret_cast<u32x4*>(row + (((2 * fq + 1) ^ (p & 7)) << 4)) = __builtin_bit_cast(u32x4, o1) & k4;
        }
    }
    __syncthreads();

    // ---- phase 2: 3x3 stride 2 over the LDS patch
    f32x4 acc[4][4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[ni][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int pl = wm * 4 * SD_PW + fr;                      // LDS row of (first output row of this wave, tap (0,0), column fr)
    if (!(a.dbg & 2))
#pragma unroll
    for (int step = 0; step < 18; ++step) {
        const int tap = step >> 1, h = step & 1, kh = tap / 3, kw = tap % 3;
        if (step + SD_RING - 1 < 18) load_wa(wa[(step + SD_RING - 1) % SD_RING], step + SD_RING - 1);
        __builtin_amdgcn_sched_barrier(0);                   // (left alone the compiler sinks each load to just before its MFMAs)
        f16x8 xb[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int cm = (2 * (m >> 1) + kh) * SD_PW + (m & 1) * 16 + (kw == 1 ? SD_EVEN : (kw == 2 ? 1 : 0));
            const int p = pl + cm;
            xb[m] = *reinterpret_cast<const f16x8*>(smem + p * 128 + (((h * 4 + fq) ^ (p & 7)) << 4));
        }
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int m = 0; m < 4; ++m)
                acc[ni][m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[step % SD_RING][ni], xb[m], acc[ni][m], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }

    const int cbase = wn * 64 + fq * 16;
    float bv[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) bv[j] = a.bias1[cbase + j];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int oy = oy0 + wm * 2 + (m >> 1), ox = ox0 + (m & 1) * 16 + fr;
        if (oy >= a.Ho || ox >= a.Wo || (a.dbg & 4)) continue;
        const long pix = ((long)b * a.Ho + oy) * a.Wo + ox;
        f16x8 o0, o1;
        float v16[16];
        bias_act16(acc[0][m], acc[1][m], acc[2][m], acc[3][m], bv, true, v16);
#pragma unroll
        for (int j = 0; j < 8; ++j) { o0[j] = (f16)v16[j]; o1[j] = (f16)v16[8 + j]; }
        f16* dst = reinterpret_cast<f16*>(a.out) + pix * a.out_ct + a.out_coff + cbase;
        *reinterpret_cast<f16x8*>(dst) = o0;
        *reinterpret_cast<f16x8*>(dst + 8) = o1;
    }
}

// Two-group form of stem_down_kernel (same arithmetic, same outputs): the one-group kernel runs its three parts one after the other
// on all eight waves -- stem pixels -> LDS 0.66 ms (gather latency + 144 SiLUs per lane), 3x3 s2 from LDS 0.47 ms (MFMAs, weights
// from L2), epilogue + stores 0.30 ms per 256 tiles -- and its 138 KiB patch leaves no room for a second workgroup.  Here a
// persistent workgroup (one per CU) has two groups of four waves (waves w and w + 4 share a SIMD), each with its own 72 KiB
// patch of 8 x 16 output pixels; the patches of the workgroup alternate between the groups, and in every phase one group fills
// its patch (VALU / memory latency) while the other convolves and stores its previous one (matrix cores): one barrier per phase.
constexpr int S2_TH = 8, S2_TW = 16, S2_PH = 2 * S2_TH + 1, S2_PW = 2 * S2_TW + 1, S2_EVEN = S2_TW + 1;
constexpr int S2_ROWS = S2_PH * S2_PW, S2_FRAGS = (S2_ROWS + 15) / 16, S2_BUF = S2_FRAGS * 16 * 128, S2_LDS = 2 * S2_BUF;
static_assert(S2_FRAGS % 4 == 0, "fragments split evenly over the four waves of a group");

__global__ __launch_bounds__(512) void stem_down2_kernel(const StemDownArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, w4 = wave & 3, wn = w4 & 1, wm = w4 >> 1;
    char* const buf = smem + grp * S2_BUF;                   // this group's patch
    const int tiles_x = (a.Wo + S2_TW - 1) / S2_TW, tiles_y = (a.Ho + S2_TH - 1) / S2_TH;
    const int npatch = a.B * tiles_y * tiles_x;
    const int NP = (int)blockIdx.x < npatch ? (npatch - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;     // patches of this workgroup
    const auto rsi = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.in), 0, a.in_bytes, 0x00020000);
    const auto rsw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wgt32), 0, a.wgt32_bytes, 0x00020000);

    // weight fragments of step (tap, h) of the 3x3 s2 conv: rows w4*32 + ni*16 + fr of chunk h, bytes fq*16..
    // Round 3: a wave convolves ALL 8 output rows of the patch x 32 channels (was 4 rows x 64 channels).  The weight fragments come
    // straight from L2, per wave and per patch: 4 fragments x 18 steps = 72 KB per wave, 288 KB per patch -- at the 16-17 B per cycle a
    // CU's fetch path sustains (section 4 of DESIGN.md) that alone was ~9 us per patch, the whole phase.  Two fragments per step feeding
    // eight pixel fragments halve it (the pixel fragments are LDS reads); outputs are bit-identical (same K order per output).
    // Measured: 1.17-1.25 -> 1.09-1.11 ms per 256 tiles, less than the halved fetch promised: the FILL phase (27 eight-byte gathers per
    // wave and patch + 144 SiLUs per lane) now sets the phase time.  A weight-STATIONARY form was built on that reading and thrown away
    // again: four-wave workgroups, two per CU, 14 of the 18 K steps of a wave's 32-channel weight slice held in registers for the whole
    // kernel (112 VGPRs), the stem panel in LDS, gathers three fragments at a time -- bit-identical, 1.20 ms (no fetch of weights per
    // patch, but no fill / convolve overlap inside a workgroup either, and 32 B of scratch at the 256-register limit).
    constexpr int RING = 4;
    f16x8 wa[RING][2];
    const unsigned wl = (unsigned)((w4 * 32 + fr) * 64 + fq * 16);
    auto load_wa = [&](f16x8* dst, int step) {
        const int h = step & 1, tap = step >> 1;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) dst[ni] = __builtin_bit_cast(f16x8, load_b128(rsw, wl + ni * 1024, (h * 9 + tap) * 8192));
    };
    const f16* wp = reinterpret_cast<const f16*>(a.wpk2);
    const int t0 = 2 * fq, t1 = 2 * fq + 1;                  // the two taps of this lane's k-chunk; tap 8 rides in the second MFMA (fq = 0)
    const int dh0 = t0 / 3 - 1, dw0 = t0 % 3 - 1, dh1 = t1 / 3 - 1, dw1 = t1 % 3 - 1;
    const int d0 = (dh0 * a.Wi + dw0) * 8, d1 = (dh1 * a.Wi + dw1) * 8, d2 = (a.Wi + 1) * 8;

    auto coords = [&](int n, int& b, int& oy0, int& ox0) {
        int id = (int)blockIdx.x + n * (int)gridDim.x;
        const int tx = id % tiles_x; id /= tiles_x;
        oy0 = (id % tiles_y) * S2_TH; ox0 = tx * S2_TW; b = id / tiles_y;
    };

    // ---- fill: the 17 x 33 stem pixels under patch n -> this group's LDS patch (bias + SiLU applied, fp16, zeros outside the map)
    auto fill = [&](int n) {
        int b, oy0, ox0;
        coords(n, b, oy0, ox0);
        const int sy0 = 2 * oy0 - 1, sx0 = 2 * ox0 - 1;      // stem-map coordinates of LDS pixel (0, 0)
        // stem panel and bias: re-read per patch (L2 hits, beside the gathers) rather than 48 registers held across the convolution
        f16x8 sw0[4], sw1[4];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            sw0[ni] = *reinterpret_cast<const f16x8*>(wp + (ni * 16 + fr) * 64 + fq * 8);
            sw1[ni] = *reinterpret_cast<const f16x8*>(wp + (ni * 16 + fr) * 64 + 32 + fq * 8);
        }
        float bv0[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) bv0[j] = a.bias0[fq * 16 + j];
        constexpr int NG = S2_FRAGS / 4;
        u32x2 q0[NG], q1[NG], q2[NG];
        unsigned inmask = 0;
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
            const int g = gi * 4 + w4, p = g * 16 + fr;
            const int sy = p / S2_PW, q = p - sy * S2_PW;
            const int sx = q < S2_EVEN ? 2 * q : 2 * (q - S2_EVEN) + 1;
            const int Y = sy0 + sy, X = sx0 + sx;
            const bool inmap = p < S2_ROWS && (unsigned)Y < (unsigned)a.H1 && (unsigned)X < (unsigned)a.W1;
            inmask |= inmap ? (1u << gi) : 0u;
            const int hc = 2 * Y, wc = 2 * X;
            const int base = ((b * a.Hi + hc) * a.Wi + wc) * 8;
            const bool ok0 = inmap && ((hc + dh0) | (wc + dw0)) >= 0, ok1 = inmap && ((hc + dh1) | (wc + dw1)) >= 0;
            q0[gi] = load_b64(rsi, ok0 ? (unsigned)(base + d0) : CY_OOB);
            q1[gi] = load_b64(rsi, ok1 ? (unsigned)(base + d1) : CY_OOB);
            q2[gi] = load_b64(rsi, (inmap && fq == 0) ? (unsigned)(base + d2) : CY_OOB);
        }
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
            const int g = gi * 4 + w4, p = g * 16 + fr;
            const bool inmap = (inmask >> gi) & 1u;
            // the fourth NHWC channel is padding: its weights are zero, and masking it keeps a stray NaN out of the sum
            const u32x4 u0 = {q0[gi].x, q0[gi].y & 0xFFFFu, q1[gi].x, q1[gi].y & 0xFFFFu};
            const u32x4 u1 = {q2[gi].x, q2[gi].y & 0xFFFFu, 0u, 0u};
            const f16x8 x0 = __builtin_bit_cast(f16x8, u0), x1 = __builtin_bit_cast(f16x8, u1);
            f32x4 acc[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(sw0[ni], x0, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                acc[ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(sw1[ni], x1, acc[ni], 0, 0, 0);
            }
            f16x8 o0, o1;
            float v16[16];
            bias_act16(acc[0], acc[1], acc[2], acc[3], bv0, true, v16);
#pragma unroll
            for (int j = 0; j < 8; ++j) { o0[j] = (f16)v16[j]; o1[j] = (f16)v16[8 + j]; }
            const unsigned keep = inmap ? 0xFFFFFFFFu : 0u;
            const u32x4 k4 = {keep, keep, keep, keep};
            char* row = buf + p * 128;
            *reinterpret_cast<u32x4*>(row + (((2 * fq) ^ (p & 7)) << 4)) = __builtin_bit_cast(u32x4, o0) & k4;
            *reinterpret_cast<u32x4*>(row + (((2 * fq + 1) ^ (p & 7)) << 4)) = __builtin_bit_cast(u32x4, o1) & k4;
        }
        // the first weight fragments of the convolution that follows the barrier: in flight across it
#pragma unroll
        for (int st = 0; st < RING - 1; ++st) load_wa(wa[st], st);
    };

    // ---- convolve + store: 3x3 stride 2 over this group's patch (wave: 4 output rows x 16 columns x 64 channels)
    auto conv_store = [&](int n) {
        int b, oy0, ox0;
        coords(n, b, oy0, ox0);
        f32x4 acc[2][8];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int m = 0; m < 8; ++m) acc[ni][m] = f32x4{0.f, 0.f, 0.f, 0.f};
        unsigned xrow[8];                                     // lane part of a pixel-fragment address for (row offset & 7) = c
#pragma unroll
        for (int c = 0; c < 8; ++c) xrow[c] = (unsigned)(fr * 128 + ((fq ^ ((fr + c) & 7)) << 4));
#pragma unroll
        for (int step = 0; step < 18; ++step) {
            const int tap = step >> 1, h = step & 1, kh = tap / 3, kw = tap % 3;
            if (step + RING - 1 < 18) load_wa(wa[(step + RING - 1) % RING], step + RING - 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mh = 0; mh < 2; ++mh) {                  // two half-steps of four pixel fragments (16 registers)
                f16x8 xb[4];
#pragma unroll
                for (int m4 = 0; m4 < 4; ++m4) {
                    const int m = mh * 4 + m4;
                    const int cm = (2 * m + kh) * S2_PW + (kw == 1 ? S2_EVEN : (kw == 2 ? 1 : 0));
                    // row p = fr + cm, chunk (h*4 + fq) ^ (p & 7): one of eight lane bases (by cm & 7), the second K half = bit 6 flipped
                    xb[m4] = *reinterpret_cast<const f16x8*>(buf + ((xrow[cm & 7] ^ (unsigned)(h * 64)) + cm * 128));
                }
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                    for (int m4 = 0; m4 < 4; ++m4)
                        acc[ni][mh * 4 + m4] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[step % RING][ni], xb[m4], acc[ni][mh * 4 + m4], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // packed rows w4*32 + ni*16 + (4 fq + j) hold channels 64 (w4 >> 1) + 16 fq + 4 (2 (w4 & 1) + ni) + j: 8 contiguous channels per lane
        const int cbase = (w4 >> 1) * 64 + fq * 16 + (w4 & 1) * 8;
        f32x2 bv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[j] = f32x2{a.bias1[cbase + 2 * j], a.bias1[cbase + 2 * j + 1]};
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int oy = oy0 + m, ox = ox0 + fr;
            if (oy >= a.Ho || ox >= a.Wo) continue;
            const long pix = ((long)b * a.Ho + oy) * a.Wo + ox;
            f16x8 o;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {          // bias + SiLU, two values per instruction (as bias_act16)
                    f32x2 t = f32x2{acc[ni][m][2 * hh], acc[ni][m][2 * hh + 1]} + bv[ni * 2 + hh];
                    f32x2 e = t * f32x2{-1.44269504088896341f, -1.44269504088896341f};
                    e = f32x2{__builtin_amdgcn_exp2f(e[0]), __builtin_amdgcn_exp2f(e[1])} + f32x2{1.0f, 1.0f};
                    t = t * f32x2{__builtin_amdgcn_rcpf(e[0]), __builtin_amdgcn_rcpf(e[1])};
                    o[ni * 4 + 2 * hh] = (f16)t[0]; o[ni * 4 + 2 * hh + 1] = (f16)t[1];
                }
            *reinterpret_cast<f16x8*>(reinterpret_cast<f16*>(a.out) + pix * a.out_ct + a.out_coff + cbase) = o;
        }
    };

    // Patch n of the workgroup belongs to group n & 1; phase n: its group fills it, phase n + 1: the same group convolves it, so in
    // every phase one group fills and the other convolves.  Phases 0 .. NP, one barrier each; every wave executes NP + 1 of them
    // (group 1 sits out phase 0; the group that does not own the last patch sits out the last phase).  One straight-line loop
    // body for both groups: with a per-phase branch on the role the two instruction streams cost 388 B of scratch.
    auto phase_barrier = [&]() {
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
    };
    if (grp) phase_barrier();
#pragma unroll 1
    for (int n = grp; n < NP; n += 2) {
        fill(n);
        phase_barrier();
        conv_store(n);
        phase_barrier();
    }
    if (((NP + grp) & 1) == 0) phase_barrier();
}

long stem_down_blocks(const StemDownArgs& a) {
    return (long)a.B * ((a.Ho + SD_TH - 1) / SD_TH) * ((a.Wo + SD_TW - 1) / SD_TW);
}

hipError_t launch_stem_down(const StemDownArgs& a, hipStream_t s) {
    if (a.Hi != 2 * a.H1 || a.Wi != 2 * a.W1) return hipErrorInvalidValue;
    StemDownArgs b2 = a; b2.dbg = dev_knob("CY_SD_DBG", 0);
    // the two-group persistent form once every workgroup gets at least two patches (both wave groups busy), else the one-group
    // form; their outputs are bit for bit the same, so the choice may depend on the launch size.  CY_STEM_V = 1 / 2 forces one
    // (read per call: tests).  256 tiles of 512^2: 1.44-1.47 -> 1.18-1.20 ms alone, 2.38 -> 1.58 ms inside the pipelined pass.
    const int v = env_knob("CY_STEM_V", 0);
    const long np = (long)a.B * ((a.Ho + S2_TH - 1) / S2_TH) * ((a.Wo + S2_TW - 1) / S2_TW);
    if (v == 2 || (v == 0 && np >= 512))
        return launch_lds<stem_down2_kernel>(dim3((unsigned)(np < 256 ? np : 256)), dim3(512), S2_LDS, S2_LDS, s, b2);
    return launch_lds<stem_down_kernel>(dim3((unsigned)stem_down_blocks(a)), dim3(512), SD_LDS, SD_LDS, s, b2);
}

// stem panel of stem_down_kernel: [64 rows, permuted like pack_weights][64] fp16; k = tap*4 + c for taps 0..7, 32 + c for
// tap 8 (c = NHWC4 channel, the fourth is zero)
void pack_stem_weights2(const float* W, int cout, void* dst) {
    f16* o = reinterpret_cast<f16*>(dst);
    for (int row = 0; row < 64; ++row) {
        const int ni = (row >> 4) & 3, rr = row & 15;
        const int n = (rr >> 2) * 16 + ni * 4 + (rr & 3);
        for (int k = 0; k < 64; ++k) {
            const int tap = k < 32 ? k / 4 : 8, c = k < 32 ? k % 4 : k - 32;
            float v = 0.0f;
            if (n < cout && c < 3 && k < 36) v = W[((size_t)n * 3 + c) * 9 + tap];
            o[row * 64 + k] = (f16)v;
        }
    }
}

}  // namespace cy
