// The box branch of the detect head at candidate anchors only (fp16 context, plain detect path).
//
// decode_kernel reads the 64 DFL logits of an anchor only when its best class score passes `conf`: on survey tiles that is a few
// dozen of 5376 anchors.  The forward pass therefore leaves the three ops of each level's box branch (Op::box: cv2.l.0 3x3 Cin -> 64,
// cv2.l.1 3x3 64 -> 64, cv2.l.2 1x1 64 -> 64) unlaunched; box_mark_kernel and box_compact_kernel (detect_post.hip) list the candidate
// anchors of the batch and, de-duplicated through a per-pixel slot map, the stage-1 pixels they need (their in-map 3x3
// neighbourhoods); the three launches here compute
//   stage 1: cv2.l.0 + bias + SiLU as fp16 at the listed pixels        -> s1[slot][64]
//   stage 2: cv2.l.1 + bias + SiLU as fp16 at the candidate pixels     -> s2[candidate][64]   (a neighbour outside the map is zero)
//   stage 3: cv2.l.2 + bias as fp32 into columns 0..63 of the candidate's prediction row
// as a gather implicit GEMM: a wave owns 16 * MI list entries and loads its MFMA operands straight from global memory, two steps
// ahead: 16 bytes of a pixel (or the zero of the buffer range check) and 16 bytes of a row of the layer's packed filter per lane.
// Loads are issued in the COALESCED lane order -- lane l fetches chunk l & 3 of row l >> 2, so that four neighbouring lanes share a
// 64-byte segment -- and moved to the MFMA order (lane fr + 16 fq holds chunk fq of row fr) with ds_bpermute just before use.  In
// the MFMA order itself every lane quad touches four segments, and the texture addresser, not the matrix pipe, set the pace:
// ~3000 cycles per 16-MFMA step in the first form of this kernel.
//
// BIT-IDENTICAL to the dense kernels: every output value is one chain of v_mfma_f32_16x16x32_f16 into one fp32 accumulator, and
// the chain only depends on which 32 products each MFMA sums (and in which k slot) and on the order of the MFMAs.  The dense
// kernels walk K in one of two ways, reproduced here with the dense kernels' own packed filters:
//   WALK32 (conv3x3_wide_kernel, wgt32 = 64-byte K chunks): 32-channel slab outer, taps 0..8 inner, lane quarter fq holds channels
//          32 slab + 8 fq .. + 7
//   WALK64 (conv3x3_pp_kernel, conv3x3_c64_kernel<64>, head1x1_kernel, wgt = 128-byte K chunks): 64-channel chunk outer, taps
//          inner, two K steps kk = 0, 1 per tap with channels 64 chunk + 32 kk + 8 fq .. + 7
// Packed row 16 ni + rr holds output channel 16 (rr >> 2) + 4 ni + (rr & 3), so lane (fr, fq) ends with channels 16 fq .. 16 fq + 15
// of pixel fr in acc[0..3], as in the dense kernels, and runs their epilogue (cy_conv_dev.h).  Which entry of a list a pixel is,
// and which lane computes it, does not enter any value.
#include "cy_conv_dev.h"

namespace cy {

namespace {
constexpr int MI = 4, PG = 16 * MI;                       // pixel fragments / list entries per wave and trip

// coalesced load order -> MFMA order: lane fr + 16 fq takes the vector lane 4 fr + fq loaded
__device__ __forceinline__ f16x8 to_mfma_order(const u32x4& v, int src4) {
    u32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = (unsigned)__builtin_amdgcn_ds_bpermute(src4, (int)v[j]);
    return __builtin_bit_cast(f16x8, r);
}

// One K walk of a wave's PG entries.  xoff[mi][tap]: byte offset of the 16 bytes lane l LOADS of tap `tap`: entry mi * 16 + (l >> 2),
// channel 8 (l & 3) of the pixel (CY_OOB: zero).  NB blocks of 2 * TAPS steps (WALK32: two slabs x nine taps; WALK64: TAPS taps x two K steps).
template <bool WALK32, int TAPS>
__device__ __forceinline__ void walk(f32x4 (&acc)[4][MI], const unsigned (&xoff)[MI][TAPS], __amdgpu_buffer_rsrc_t rsx, __amdgpu_buffer_rsrc_t rsw,
                                     int nblocks, int lane) {
    static_assert(!WALK32 || TAPS == 9, "the 32-channel walk is the wide 3x3 kernel's");
    constexpr int NS = 2 * TAPS, RING = 3, CPAD = 128;    // packed filters have pad128(64) rows per tap
    const int lr = lane >> 2, lc = lane & 3;              // row and chunk this lane loads
    const int src4 = 4 * (4 * (lane & 15) + (lane >> 4));  // (byte address of) the lane whose load this lane's MFMA operand is
    const unsigned wlane = WALK32 ? (unsigned)(lr * 64 + lc * 16) : (unsigned)(lr * 128 + lc * 16);
    u32x4 x[RING][MI], w[RING][4];
    auto load = [&](int slot, int cb, int u) {
        unsigned xs, ws;                                   // uniform parts
        int tap;
        if constexpr (WALK32) {
            const int slab = 2 * cb + u / 9;
            tap = u % 9;
            xs = (unsigned)slab * 64u;
            ws = (unsigned)((slab * 9 + tap) * CPAD) * 64u;
        } else {
            const int kk = u & 1;
            tap = u >> 1;
            xs = (unsigned)cb * 128u + (unsigned)kk * 64u;
            ws = (unsigned)((cb * TAPS + tap) * CPAD) * 128u + (unsigned)kk * 64u;
        }
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) w[slot][ni] = load_b128(rsw, wlane + (unsigned)(ni * 16 * (WALK32 ? 64 : 128)), ws);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) x[slot][mi] = load_b128(rsx, xoff[mi][tap], xs);
    };
    load(0, 0, 0);
    load(1, 0, 1);
#pragma unroll 1
    for (int cb = 0; cb < nblocks; ++cb) {
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            if (u + 2 < NS) load((u + 2) % RING, cb, u + 2);
            else if (cb + 1 < nblocks) load((u + 2) % RING, cb + 1, u + 2 - NS);
            f16x8 wf[4], xf[MI];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) wf[ni] = to_mfma_order(w[u % RING][ni], src4);
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) xf[mi] = to_mfma_order(x[u % RING][mi], src4);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[ni], xf[mi], acc[ni][mi], 0, 0, 0);
        }
    }
    static_assert(NS % RING == 0 || NS == 2, "ring slots are compile-time per step only when a block is a whole number of ring turns");
}

// bias + SiLU of the 16 channels a lane holds of one pixel, as fp16.  PACKED: the wide / c64 kernels' form (bias_act16); else the
// ping-pong kernel's value-by-value form.
template <bool PACKED>
__device__ __forceinline__ void act_store(const f32x4 (&acc)[4][MI], int mi, const float (&bv)[16], f16* dst) {
    float v[16];
    if constexpr (PACKED) {
        bias_act16(acc[0][mi], acc[1][mi], acc[2][mi], acc[3][mi], bv, true, v);
    } else {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int j = 0; j < 4; ++j) v[ni * 4 + j] = silu_fast(acc[ni][mi][j] + bv[ni * 4 + j]);
    }
    f16x8 o0, o1;
#pragma unroll
    for (int j = 0; j < 8; ++j) { o0[j] = (f16)v[j]; o1[j] = (f16)v[8 + j]; }
    *reinterpret_cast<f16x8*>(dst) = o0;
    *reinterpret_cast<f16x8*>(dst + 8) = o1;
}

__device__ __forceinline__ void zero(f32x4 (&acc)[4][MI]) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// stage 1 of one level: the entries of plist (global pixel index b * H * W + y * W + x; entry e is slot e) from the feature map
template <bool WALK32, bool PACKED>
__device__ __forceinline__ void stage1(const BoxLevel& L, int wid, int nwaves, int lane) {
    const int fr = lane & 15, fq = lane >> 4, lr = lane >> 2, lc = lane & 3;
    const int n = min(L.counts[0], L.cap);
    const int HW = L.H * L.W;
    const auto rsx = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(L.feat), 0, L.feat_bytes, 0x00020000);
    const auto rsw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(L.w1), 0, L.w1_bytes, 0x00020000);
    float bv[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) bv[j] = L.b1[fq * 16 + j];
    for (int g = wid; g * PG < n; g += nwaves) {
        unsigned xoff[MI][9];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int e = g * PG + mi * 16 + lr;
            const int p = e < n ? L.plist[e] : 0;
            const int b = p / HW, r = p - b * HW, y = r / L.W, x = r - y * L.W;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
                const bool ok = e < n && (unsigned)yy < (unsigned)L.H && (unsigned)xx < (unsigned)L.W;
                xoff[mi][tap] = ok ? (unsigned)((b * HW + yy * L.W + xx) * L.feat_ct + L.feat_coff + lc * 8) * 2u : CY_OOB;
            }
        }
        f32x4 acc[4][MI];
        zero(acc);
        walk<WALK32, 9>(acc, xoff, rsx, rsw, L.cin / 64, lane);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int e = g * PG + mi * 16 + fr;
            if (e < n) act_store<PACKED>(acc, mi, bv, reinterpret_cast<f16*>(L.s1) + (size_t)e * 64 + fq * 16);
        }
    }
}
}  // namespace

__global__ __launch_bounds__(256) void box_stage1_kernel(const BoxArgs a) {
    const BoxLevel& L = a.L[blockIdx.y];
    if (!L.sparse) return;
    const int lane = threadIdx.x & 63, wid = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    if (L.walk1 == BOX_WALK_WIDE) stage1<true, true>(L, wid, nwaves, lane);
    else if (L.walk1 == BOX_WALK_PP) stage1<false, false>(L, wid, nwaves, lane);
    else stage1<false, true>(L, wid, nwaves, lane);
}

// stage 2: the entries of clist from s1 through the slot map (conv3x3_c64_kernel<64>'s walk and epilogue)
__global__ __launch_bounds__(256) void box_stage2_kernel(const BoxArgs a) {
    const BoxLevel& L = a.L[blockIdx.y];
    if (!L.sparse) return;
    const int lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4, wid = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    const int n = min(L.counts[1], L.cap), HW = L.H * L.W;
    const auto rsx = __builtin_amdgcn_make_buffer_rsrc(L.s1, 0, (unsigned)L.cap * 128u, 0x00020000);
    const auto rsw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(L.w2), 0, L.w2_bytes, 0x00020000);
    float bv[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) bv[j] = L.b2[fq * 16 + j];
    for (int g = wid; g * PG < n; g += nwaves) {
        unsigned xoff[MI][9];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int e = g * PG + mi * 16 + (lane >> 2);
            const int p = e < n ? L.clist[e] : 0;
            const int b = p / HW, r = p - b * HW, y = r / L.W, x = r - y * L.W;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
                const bool ok = e < n && (unsigned)yy < (unsigned)L.H && (unsigned)xx < (unsigned)L.W;
                const int slot = ok ? L.map[b * HW + yy * L.W + xx] : -1;      // every in-map neighbour of a candidate was listed by the mark kernel
                xoff[mi][tap] = slot >= 0 && slot < L.cap ? (unsigned)(slot * 128 + (lane & 3) * 16) : CY_OOB;
            }
        }
        f32x4 acc[4][MI];
        zero(acc);
        walk<false, 9>(acc, xoff, rsx, rsw, 1, lane);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int e = g * PG + mi * 16 + fr;
            if (e < n) act_store<true>(acc, mi, bv, reinterpret_cast<f16*>(L.s2) + (size_t)e * 64 + fq * 16);
        }
    }
}

// stage 3: the 1x1 of the entries of clist from s2 into the prediction rows (head1x1_kernel's walk and epilogue)
__global__ __launch_bounds__(256) void box_stage3_kernel(const BoxArgs a) {
    const BoxLevel& L = a.L[blockIdx.y];
    if (!L.sparse) return;
    const int lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4, wid = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    const int n = min(L.counts[1], L.cap), HW = L.H * L.W;
    const auto rsx = __builtin_amdgcn_make_buffer_rsrc(L.s2, 0, (unsigned)L.cap * 128u, 0x00020000);
    const auto rsw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(L.w3), 0, L.w3_bytes, 0x00020000);
    float bv[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) bv[j] = L.b3[fq * 16 + j];
    for (int g = wid; g * PG < n; g += nwaves) {
        unsigned xoff[MI][1];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int e = g * PG + mi * 16 + (lane >> 2);
            xoff[mi][0] = e < n ? (unsigned)(e * 128 + (lane & 3) * 16) : CY_OOB;
        }
        f32x4 acc[4][MI];
        zero(acc);
        walk<false, 1>(acc, xoff, rsx, rsw, 1, lane);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int e = g * PG + mi * 16 + fr;
            if (e >= n) continue;
            const int p = L.clist[e], b = p / HW, r = p - b * HW;
            typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
            float* dst = a.pred + ((size_t)b * a.A + L.a_off + r) * (64 + a.nc) + fq * 16;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                *reinterpret_cast<f32x4u*>(dst + 4 * ni) = f32x4u{acc[ni][mi][0] + bv[ni * 4], acc[ni][mi][1] + bv[ni * 4 + 1], acc[ni][mi][2] + bv[ni * 4 + 2],
                                                                  acc[ni][mi][3] + bv[ni * 4 + 3]};
        }
    }
}

// the three stages of every sparse level of a batch, queued in order behind launch_box_mark
hipError_t launch_box_sparse(const BoxArgs& a, hipStream_t s) {
    for (const BoxLevel& L : a.L)
        if (L.sparse && (L.cin % 64 || L.cin < 64 || L.cap < 1 || (size_t)L.cap * 128 >= 0xFFFFFF00ull)) return hipErrorInvalidValue;
    const dim3 grid(BOX_GRID, 3), block(256);
    hipLaunchKernelGGL(box_stage1_kernel, grid, block, 0, s, a);
    hipLaunchKernelGGL(box_stage2_kernel, grid, block, 0, s, a);
    hipLaunchKernelGGL(box_stage3_kernel, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace cy
