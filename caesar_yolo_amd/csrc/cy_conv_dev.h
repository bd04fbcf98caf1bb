// Device-side prelude of the convolution kernels (conv_igemm.hip, conv_stem.hip, conv_weights.hip, bneck64.hip, cy_extra.hip):
// vector types, the buffer-load sentinel, SiLU, the bias / activation / store steps of the epilogue for the 16 channels a lane
// holds of one pixel, and the LDS-DMA wrappers.  Everything here is __device__ __forceinline__ or a type: no symbols.
#pragma once
#include "cy_kernels.h"

namespace cy {

typedef _Float16 f16;
typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

#define CY_OOB 0xFFFFFF00u
#define CY_WAIT_VM(N) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory")

__device__ __forceinline__ float silu_exact(float x) { return x / (1.0f + expf(-x)); }
// fp16 context: x * sigmoid(x) with the hardware exp2/rcp (1 ulp each; the result is rounded to fp16 anyway):
// 5 VALU instructions per element instead of the ~50 of an IEEE-exact division
__device__ __forceinline__ float silu_fast(float x) {
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.44269504088896341f));
}
// The epilogue of the fp16 kernels for the 16 values a lane holds of one pixel (four accumulators of four channels): bias +
// SiLU with two values per VALU instruction where the ISA has a packed fp32 form (add, mul; exp2 and rcp stay scalar), and
// the activation switch as ONE uniform branch (written per value it becomes a v_cndmask per value behind an unconditional SiLU).
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void bias_act16(const f32x4& a0, const f32x4& a1, const f32x4& a2, const f32x4& a3, const float (&bv)[16],
                                           bool act, float (&v)[16]) {
    const f32x4 acc[4] = {a0, a1, a2, a3};
    if (act) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x2 t = f32x2{acc[ni][2 * h], acc[ni][2 * h + 1]} + f32x2{bv[ni * 4 + 2 * h], bv[ni * 4 + 2 * h + 1]};
                f32x2 e = t * f32x2{-1.44269504088896341f, -1.44269504088896341f};
                e = f32x2{__builtin_amdgcn_exp2f(e[0]), __builtin_amdgcn_exp2f(e[1])} + f32x2{1.0f, 1.0f};
                t = t * f32x2{__builtin_amdgcn_rcpf(e[0]), __builtin_amdgcn_rcpf(e[1])};
                v[ni * 4 + 2 * h] = t[0]; v[ni * 4 + 2 * h + 1] = t[1];
            }
    } else {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[ni * 4 + j] = acc[ni][j] + bv[ni * 4 + j];
    }
}

// fp16x3 context: the same epilogue with the accumulator first multiplied by the power of two that undoes the weight scale of its
// output channel, and the result stored as two fp16 halves hi = fp16(v), lo = fp16(v - hi) (lo_off halves behind hi)
__device__ __forceinline__ void scale_bias_act16(const f32x4& a0, const f32x4& a1, const f32x4& a2, const f32x4& a3, const float (&bv)[16],
                                                 const float (&sc)[16], bool act, float (&v)[16]) {
    const f32x4 acc[4] = {a0, a1, a2, a3};
    if (act) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x2 t = f32x2{acc[ni][2 * h], acc[ni][2 * h + 1]} * f32x2{sc[ni * 4 + 2 * h], sc[ni * 4 + 2 * h + 1]} +
                          f32x2{bv[ni * 4 + 2 * h], bv[ni * 4 + 2 * h + 1]};
                f32x2 e = t * f32x2{-1.44269504088896341f, -1.44269504088896341f};
                e = f32x2{__builtin_amdgcn_exp2f(e[0]), __builtin_amdgcn_exp2f(e[1])} + f32x2{1.0f, 1.0f};
                t = t * f32x2{__builtin_amdgcn_rcpf(e[0]), __builtin_amdgcn_rcpf(e[1])};
                v[ni * 4 + 2 * h] = t[0]; v[ni * 4 + 2 * h + 1] = t[1];
            }
    } else {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[ni * 4 + j] = acc[ni][j] * sc[ni * 4 + j] + bv[ni * 4 + j];
    }
}
__device__ __forceinline__ void store_split16(f16* dst, int lo_off, const float (&v)[16]) {
    f16x8 h0, h1, l0, l1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        h0[j] = (f16)v[j]; h1[j] = (f16)v[8 + j];
        l0[j] = (f16)(v[j] - (float)h0[j]); l1[j] = (f16)(v[8 + j] - (float)h1[j]);
    }
    *reinterpret_cast<f16x8*>(dst) = h0;
    *reinterpret_cast<f16x8*>(dst + 8) = h1;
    *reinterpret_cast<f16x8*>(dst + lo_off) = l0;
    *reinterpret_cast<f16x8*>(dst + lo_off + 8) = l1;
}
__device__ __forceinline__ void store_split1(f16* dst, int lo_off, float v) {
    const f16 h = (f16)v;
    dst[0] = h; dst[lo_off] = (f16)(v - (float)h);
}
// virtual K chunk of the fp16x3 passes [x_lo | x_hi | x_hi] (against weights [w_hi | w_lo | w_hi]) -> physical chunk; lo = 1 in the
// first pass.  The two small cross terms come FIRST: the fp32 accumulator of the MFMA rounds at every step by an amount relative
// to its current magnitude, so they are summed while it is still ~2^-11 of the final value (their rounding is then negligible)
// and the x_hi * w_hi chain runs last, exactly as long as in the fp16 context.
__device__ __forceinline__ int x3_chunk(int v, int per_pass, int& lo) {
    lo = v < per_pass;
    if (v >= 2 * per_pass) return v - 2 * per_pass;
    if (v >= per_pass) return v - per_pass;
    return v;
}

template <typename T> struct Elem;
template <> struct Elem<f16> { static constexpr int BKE = 64, EPC = 8, ES = 2; };
template <> struct Elem<float> { static constexpr int BKE = 32, EPC = 4, ES = 4; };

__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    // blocks b and b+8 share an XCD (round-robin dispatch): give each XCD a contiguous run of tiles so that
    // neighbouring tiles (same activation rows, different channel blocks) hit one L2.  Bijective for any nwg.
    const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}

// LDS-DMA and buffer-load wrappers.  Non-template: inside a template kernel a buffer builtin whose soffset is not a constant makes this clang drop
// the kernel's host-side instantiation without a diagnostic; called through these, the builtin is never value-dependent.
typedef __attribute__((address_space(3))) void lds_ptr_t;
__device__ __forceinline__ void dma_piece(__amdgpu_buffer_rsrc_t rs, lds_ptr_t* dst, unsigned voff, unsigned soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, dst, 16, voff, soff, 0, 0);     // soffset is NOT range-checked (voffset is)
}
__device__ __forceinline__ u32x4 load_b128(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
    return __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
}

// 16 floats of a lane (bias, output scale) from LDS as four 16-byte reads
__device__ __forceinline__ void load16(const float* lds, float (&v)[16]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(lds + j * 4);
        v[j * 4] = t[0]; v[j * 4 + 1] = t[1]; v[j * 4 + 2] = t[2]; v[j * 4 + 3] = t[3];
    }
}

// The per-pixel tail of the epilogue: the N (16, or 8 in the ping-pong kernel) activated values v a lane holds of one pixel, channels
// cbase .. cbase + N - 1 of a layer with cout channels, get the residual added and are stored as fp16.  out / res are the tensors'
// first elements and oidx / ridx the element index of channel cbase of this pixel in them (res == null: no residual).  Whole groups
// go as 16-byte vectors, a ragged group scalar by scalar, channels >= cout are not touched.  The last argument says where the
// residual vectors of a whole group come from: LoadRes{} -- they are loaded here -- or the array of vectors the caller already
// holds in registers (requested ahead of its arithmetic; they are not loaded again).
struct LoadRes {};
template <int N, typename P>
__device__ __forceinline__ void store_px(f16* out, long oidx, const f16* res, long ridx, int cbase, int cout, float (&v)[N], const P& pre) {
    if (cbase + N <= cout) {
        f16* dst = out + oidx;
        if (res) {
            f16x8 r[N / 8];
#pragma unroll
            for (int h8 = 0; h8 < N / 8; ++h8) {
                if constexpr (__is_same(P, LoadRes)) r[h8] = *reinterpret_cast<const f16x8*>(res + ridx + 8 * h8);
                else r[h8] = pre[h8];
            }
#pragma unroll
            for (int h8 = 0; h8 < N / 8; ++h8)
#pragma unroll
                for (int j = 0; j < 8; ++j) v[8 * h8 + j] += (float)r[h8][j];
        }
        f16x8 o[N / 8];
#pragma unroll
        for (int h8 = 0; h8 < N / 8; ++h8)
#pragma unroll
            for (int j = 0; j < 8; ++j) o[h8][j] = (f16)v[8 * h8 + j];
#pragma unroll
        for (int h8 = 0; h8 < N / 8; ++h8) *reinterpret_cast<f16x8*>(dst + 8 * h8) = o[h8];
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            if (cbase + j >= cout) continue;
            float t = v[j];
            if (res) t += (float)res[ridx + j];
            out[oidx + j] = (f16)t;
        }
    }
}

// The same for the fp16x3 context: the residual is the sum of its high and low halves (res_lo elements apart, added as
// (float)hi + (float)lo), the result is stored as high / low halves (out_lo apart).  pre = {hi 0-7, hi 8-15, lo 0-7, lo 8-15}.
template <typename P>
__device__ __forceinline__ void store_px_split(f16* out, long oidx, int out_lo, const f16* res, long ridx, int res_lo, int cbase, int cout,
                                               float (&v)[16], const P& pre) {
    f16* dst = out + oidx;
    if (cbase + 16 <= cout) {
        if (res) {
            f16x8 r[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (__is_same(P, LoadRes)) r[i] = *reinterpret_cast<const f16x8*>(res + ridx + (i >> 1) * res_lo + (i & 1) * 8);
                else r[i] = pre[i];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) { v[j] += (float)r[0][j] + (float)r[2][j]; v[8 + j] += (float)r[1][j] + (float)r[3][j]; }
        }
        store_split16(dst, out_lo, v);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (cbase + j >= cout) continue;
            float t = v[j];
            if (res) t += (float)res[ridx + j] + (float)res[ridx + res_lo + j];
            store_split1(dst + j, out_lo, t);
        }
    }
}

}  // namespace cy
