// Fused Conv2d + folded-BN bias + SiLU (+ residual, + concat/upsample gather, + channel-slice store) as an
// implicit GEMM on CDNA4 matrix cores (gfx950 only).
//
// Replaces ultralytics `Conv.forward_fuse` / `Bottleneck` / `Concat` / `nn.Upsample` as executed inside the
// reference's model call (caesar_yolo/evaluation.py:181-193; graph: SURVEY.md Appendix A.1 step 4, Appendix B).
//
// GEMM view (per launch): D[n, m] = sum_k W[n, k] * X[m, k]
//   m = output pixel (b, ho, wo) over the whole tile batch, n = output channel, k = (tap, input channel).
//   The weights are the MFMA "A" operand and the im2col rows the "B" operand, so an accumulator lane holds
//   FOUR CONSECUTIVE CHANNELS of ONE pixel: with the 64-row weight permutation done at pack time a lane owns 16
//   contiguous channels of a pixel and the NHWC store is 16-byte vectors (no LDS transpose in the epilogue).
//   f16: v_mfma_f32_16x16x32_f16 (fp32 accumulate).  f32 (parity mode): v_mfma_f32_16x16x4_f32 = exact fp32 FMA chain.
//
// Data movement: K is walked in 128-byte slabs per row (64 halves / 32 floats of one filter tap).  Each lane moves
// 16-byte pieces global -> LDS directly (`buffer_load_dwordx4 ... lds`, no VGPR staging, no ds_write); the buffer
// range check supplies the zero padding of the 3x3 halo and of ragged channel counts (an out-of-range offset
// writes 0).  The LDS image is double-buffered and XOR-swizzled through the SOURCE address so that ds_read_b128
// fragment reads are conflict-free (slot = chunk ^ (row & 7): conflict-free for any 16 consecutive rows, whatever the first row -- the 3x3 taps of the
// halo kernels read at arbitrary row offsets; a 256-byte bank row holds two 128-byte tile rows).
//
// This file holds the implicit-GEMM kernels and their launchers, and launch_conv, which makes the launcher call that a ConvChoice
// names (the decision itself is host code without HIP: conv_choose, cy_conv_plan.cpp), and nothing else: the
// device prelude and the shared epilogue steps are in cy_conv_dev.h, the stem kernels in conv_stem.hip, weight packing in
// conv_weights.hip, the SPPF pool with the other non-GEMM layer operators in cy_extra.hip.
#include "cy_kernels.h"
#include "cy_conv_dev.h"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

namespace cy {

// developer diagnostics: per-segment s_memtime sums of the 3x3 kernels' stage loop, summed over waves.  Compiled in only
// with -DCY_STAMPS_ENABLED=1 (then enabled at run time by CY_DBG bit 6); a stamped build is for SHARES, not for timing.
#ifndef CY_STAMPS_ENABLED
#define CY_STAMPS_ENABLED 0
#endif
__device__ unsigned long long g_stamps[8];
constexpr int WG_STAMP_SLOTS = 4096;
__device__ unsigned long long g_wg_stamps[WG_STAMP_SLOTS * 4];     // per-workgroup phase records of the wide kernel (stamped builds)
__device__ unsigned long long g_wg_life[WG_STAMP_SLOTS * 3];       // pixels-direct kernel: entry, exit (100 MHz counter) and CU of each workgroup
__device__ __forceinline__ unsigned long long stamp_now() {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}
__device__ __forceinline__ unsigned long long stamp_real() {       // constant 100 MHz counter: wall time in units of 10 ns
    unsigned long long t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}

// the lane's number from the hardware (not from threadIdx.x, and not hoisted): for code that runs once per tile inside a loop whose
// registers are all taken, so that no lane constant is carried -- or spilled -- across the loop
__device__ __forceinline__ int lane_now() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

// NSTAGE = 2: the slab for step s+1 is requested while step s computes and drained at the barrier (two workgroups of
// four waves per CU hide each other's drains).  NSTAGE = 3 (the 256x128 tile, eight waves, one workgroup per CU): slabs
// are requested TWO steps ahead and the wait before a barrier is a counted vmcnt that leaves the newest request in
// flight, so an L2 round trip (about one step's worth of MFMA time for K-slabs of 64) is off the critical path.
template <typename T, int WM, int WN, int MI, int NSTAGE = 2, bool SPLIT = false>
__global__ __launch_bounds__(WM * WN * 64, (WM * WN == 4 ? 2 : 1)) void conv_igemm_kernel(const ConvArgs a) {
    static_assert(!SPLIT || sizeof(T) == 2, "fp16x3: fp16 operands");
    constexpr int BM = WM * MI * 16, BN = WN * 64, NT = WM * WN * 64, RPR = NT / 8;
    constexpr int BKE = Elem<T>::BKE, EPC = Elem<T>::EPC, ES = Elem<T>::ES;
    constexpr int AROWS = BM / RPR, BROWS = BN / RPR;        // rows each thread stages per slab (RPR rows per round)
    constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = A_BYTES + B_BYTES;
    constexpr int DIST = NSTAGE - 1, PER = AROWS + BROWS;    // slabs in flight; DMA instructions per slab per wave
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int M = a.B * a.Ho * a.Wo;
    const int ntn = (pad64(a.Cout) + BN - 1) / BN;
    const int nwg = gridDim.x;
    const int id = xcd_remap(blockIdx.x, nwg);
    const int m0 = (id / ntn) * BM, n0 = (id % ntn) * BN;
    const int taps = a.k * a.k, cpad = pad128(a.Cout);
    const int pchunks = (a.Cin + BKE - 1) / BKE;             // K chunks of one pass over the input channels
    const int cchunks = SPLIT ? a.split * pchunks : pchunks; // fp16x3: three passes (x_lo w_hi, x_hi w_lo, x_hi w_hi), or two (x_lo w, x_hi w: fp16-exact weights)
    const int nslab = taps * cchunks;

    const auto rs0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.in0), 0, a.in0_bytes, 0x00020000);
    const auto rs1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.c1 ? a.in1 : a.in0), 0,
                                                       a.c1 ? a.in1_bytes : a.in0_bytes, 0x00020000);
    const auto rsw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wgt), 0, a.wgt_bytes, 0x00020000);

    // ---- per-thread staging geometry: chunk q of rows (tid>>3) + 32*i
    const int q = tid & 7, r0 = tid >> 3;
    int pix0[AROWS], pix1[AROWS];
    unsigned vmask[AROWS];
    const int pad = a.k >> 1;
    const int HoWo = a.Ho * a.Wo;
#pragma unroll
    for (int i = 0; i < AROWS; ++i) {
        const int m = m0 + r0 + RPR * i;
        unsigned vm = 0;
        int p0 = 0, p1 = 0;
        if (m < M) {
            const int b = m / HoWo, r = m - b * HoWo;
            const int ho = r / a.Wo, wo = r - ho * a.Wo;
            const int hi0 = ho * a.s - pad, wi0 = wo * a.s - pad;
            for (int kh = 0; kh < a.k; ++kh)
                for (int kw = 0; kw < a.k; ++kw)
                    if ((unsigned)(hi0 + kh) < (unsigned)a.Hi && (unsigned)(wi0 + kw) < (unsigned)a.Wi)
                        vm |= 1u << (kh * a.k + kw);
            if (a.up0) p0 = (b * (a.Hi >> 1) + (ho >> 1)) * (a.Wi >> 1) + (wo >> 1);
            else p0 = (b * a.Hi + hi0) * a.Wi + wi0;
            p1 = (b * a.Hi + hi0) * a.Wi + wi0;
        }
        pix0[i] = p0; pix1[i] = p1; vmask[i] = vm;
    }

    // LDS-DMA staging: `buffer_load_dwordx4 ... lds` writes wave-uniform base + lane*16, i.e. one wave-instruction
    // fills 8 consecutive 128-byte tile rows.  Row r = 8*wave + 32*i + (lane>>3), slot = lane&7 is exactly lane-linear,
    // so the XOR swizzle moves to the SOURCE: the lane that owns slot s of row r fetches logical chunk s ^ ((r>>1)&7)
    // (the same involution the fragment reads apply).  ((r>>1)&7 does not depend on i because 32*i>>1 is 0 mod 8.)
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int cq = q ^ (r0 & 7);
    typedef __attribute__((address_space(3))) void lds_void;
    auto dma = [&](int stage, int tap, int cc) {
        int lo = 0;
        const int ccp = SPLIT ? x3_chunk(cc, pchunks, lo) : cc;       // physical chunk of the input (the weights are packed per virtual chunk)
        const int lo0 = SPLIT && lo ? a.in0_lo : 0, lo1 = SPLIT && lo ? a.in1_lo : 0;
        const int c = ccp * BKE + cq * EPC;
        const int kh = tap / a.k, kw = tap - kh * a.k;
        const int dpix = kh * a.Wi + kw;
        const bool cin_ok = c < a.Cin;
        const bool seg1 = ccp * BKE >= a.c0;              // wave-uniform: segment boundaries are multiples of BKE
        char* A = smem + stage * STAGE + wave_u * (8 * 128);
        char* Bm = A + A_BYTES;
#pragma unroll
        for (int i = 0; i < AROWS; ++i) {
            const bool ok = cin_ok && ((vmask[i] >> tap) & 1u);
            unsigned off;
            if (!seg1) off = (unsigned)((pix0[i] + (a.up0 ? 0 : dpix)) * a.in0_ct + a.in0_coff + lo0 + c) * ES;
            else       off = (unsigned)((pix1[i] + dpix) * a.in1_ct + a.in1_coff + lo1 + (c - a.c0)) * ES;
            off = ok ? off : CY_OOB;
            lds_void* dst = (lds_void*)(A + i * (RPR * 128));
            if (seg1) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs1, dst, 16, off, 0, 0, 0);
            else      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, dst, 16, off, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < BROWS; ++i) {
            const int n = n0 + r0 + RPR * i;
            const unsigned off = (unsigned)(((cc * taps + tap) * cpad + n) * 128 + cq * 16);      // rows are padded to 128: always valid
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_void*)(Bm + i * (RPR * 128)), 16, off, 0, 0, 0);
        }
    };

    f32x4 acc[4][MI];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fq = lane >> 4;
    auto compute = [&](int stage) {
        const char* A = smem + stage * STAGE;
        const char* Bm = A + A_BYTES;
        if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int qf = fq + 4 * kk;
                f16x8 xa[MI], wb[4];
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    const int r = wm * (MI * 16) + mi * 16 + fr;
                    xa[mi] = *reinterpret_cast<const f16x8*>(A + r * 128 + ((qf ^ (r & 7)) << 4));
                }
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    const int r = wn * 64 + ni * 16 + fr;
                    wb[ni] = *reinterpret_cast<const f16x8*>(Bm + r * 128 + ((qf ^ (r & 7)) << 4));
                }
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi)
                        acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb[ni], xa[mi], acc[ni][mi], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                float xa[MI], wb[4];
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    const int r = wm * (MI * 16) + mi * 16 + fr;
                    xa[mi] = *reinterpret_cast<const float*>(A + r * 128 + ((ks ^ (r & 7)) << 4) + fq * 4);
                }
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    const int r = wn * 64 + ni * 16 + fr;
                    wb[ni] = *reinterpret_cast<const float*>(Bm + r * 128 + ((ks ^ (r & 7)) << 4) + fq * 4);
                }
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi)
                        acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[ni], xa[mi], acc[ni][mi], 0, 0, 0);
            }
        }
    };

    // ---- main loop: the DMA for slab s+1 is in flight while slab s is on the matrix pipe; one barrier per slab
    // (__syncthreads drains vmcnt, which is what orders the landed DMA before the next slab's ds_reads)
    if constexpr (NSTAGE == 2) {
        int tap = 0, cc = 0;
        dma(0, 0, 0);
        __syncthreads();
        for (int s = 0; s < nslab; ++s) {
            int ntap = tap, ncc = cc + 1;
            if (ncc == cchunks) { ncc = 0; ++ntap; }
            if ((s + 1) < nslab) dma((s + 1) & 1, ntap, ncc);
            compute(s & 1);
            __syncthreads();
            tap = ntap; cc = ncc;
        }
    } else {
        // ring of NSTAGE slabs, requests DIST steps ahead.  Slot (s+DIST) % NSTAGE last held slab s-1, whose readers are
        // all past the barrier that ended step s-1 when step s issues into it.
        int itap = 0, icc = 0, islot = 0;                    // issue cursor
        auto issue = [&]() {
            dma(islot, itap, icc);
            if (++icc == cchunks) { icc = 0; ++itap; }
            if (++islot == NSTAGE) islot = 0;
        };
#pragma unroll
        for (int d = 0; d < DIST; ++d)
            if (d < nslab) issue();
        if (nslab >= DIST) { CY_WAIT_VM((DIST - 1) * PER); } else { CY_WAIT_VM(0); }
        __builtin_amdgcn_s_barrier();
        int slot = 0;
        for (int s = 0; s < nslab; ++s) {
            const bool more = s + DIST < nslab;
            if (more) issue();
            compute(slot);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // fragment reads of this slot are done (WAR on the ring)
            if (more) { CY_WAIT_VM((DIST - 1) * PER); } else { CY_WAIT_VM(0); }
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            if (++slot == NSTAGE) slot = 0;
        }
    }

    // ---- epilogue: bias + SiLU (+ residual) and 16 contiguous channels per lane per pixel
    const int cbase = n0 + wn * 64 + fq * 16;
    float bv[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) bv[j] = a.bias[cbase + j];       // bias is padded to Cout_pad64
    float sc[SPLIT ? 16 : 1];
    if constexpr (SPLIT) {
#pragma unroll
        for (int j = 0; j < 16; ++j) sc[j] = a.oscale[cbase + j];
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int m = m0 + wm * (MI * 16) + mi * 16 + fr;
        if (m >= M) continue;
        const int b = m / HoWo, r = m - b * HoWo;
        const long opix = (long)b * a.out_bs + a.out_ro + r;
        float v[16];
        if constexpr (SPLIT) {
            scale_bias_act16(acc[0][mi], acc[1][mi], acc[2][mi], acc[3][mi], bv, sc, a.act != 0, v);
            if (!a.out_f32) {
                store_px_split(reinterpret_cast<f16*>(a.out), opix * a.out_ct + a.out_coff + cbase, a.out_lo, reinterpret_cast<const f16*>(a.res),
                               (long)m * a.res_ct + a.res_coff + cbase, a.res_lo, cbase, a.Cout, v, LoadRes{});
                continue;
            }
        } else {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float x = acc[ni][mi][j] + bv[ni * 4 + j];
                if (a.act) x = (sizeof(T) == 2) ? silu_fast(x) : silu_exact(x);
                v[ni * 4 + j] = x;
            }
        }
        if constexpr (sizeof(T) == 2) {
            if (!a.out_f32) {
                store_px(reinterpret_cast<f16*>(a.out), opix * a.out_ct + a.out_coff + cbase, reinterpret_cast<const f16*>(a.res),
                         (long)m * a.res_ct + a.res_coff + cbase, cbase, a.Cout, v, LoadRes{});
                continue;
            }
        }
        // what is left: the fp32 context, and fp32 prediction rows (out_f32) from fp16 operands
        const bool full = (cbase + 16 <= a.Cout) && !a.out_f32;
        if (full) {
            T* dst = reinterpret_cast<T*>(a.out) + opix * a.out_ct + a.out_coff + cbase;
            if (a.res) {
                const T* rp = reinterpret_cast<const T*>(a.res) + (long)m * a.res_ct + a.res_coff + cbase;
#pragma unroll
                for (int j4 = 0; j4 < 4; ++j4) {
                    const f32x4 rv = *reinterpret_cast<const f32x4*>(rp + 4 * j4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[4 * j4 + j] += rv[j];
                }
            }
#pragma unroll
            for (int j4 = 0; j4 < 4; ++j4)
                *reinterpret_cast<f32x4*>(dst + 4 * j4) = f32x4{v[4 * j4], v[4 * j4 + 1], v[4 * j4 + 2], v[4 * j4 + 3]};
        } else if (a.out_f32 && !a.res && cbase + 16 <= a.Cout) {
            // fp32 head output (box logits): rows of the prediction buffer are 64+nc floats, so only dword-aligned; four
            // 16-byte stores per lane through a 4-byte-aligned vector type instead of sixteen scattered dword stores
            typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
            float* dst = reinterpret_cast<float*>(a.out) + opix * a.out_ct + a.out_coff + cbase;
#pragma unroll
            for (int j4 = 0; j4 < 4; ++j4)
                *reinterpret_cast<f32x4u*>(dst + 4 * j4) = f32x4u{v[4 * j4], v[4 * j4 + 1], v[4 * j4 + 2], v[4 * j4 + 3]};
        } else {
            // ragged channel count (class logits, nc channels): scalar stores
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int c = cbase + j;
                if (c >= a.Cout) continue;
                float x = v[j];
                if (a.res) x += (float)(reinterpret_cast<const T*>(a.res)[(long)m * a.res_ct + a.res_coff + c]);
                if (a.out_f32) reinterpret_cast<float*>(a.out)[opix * a.out_ct + a.out_coff + c] = x;
                else reinterpret_cast<T*>(a.out)[opix * a.out_ct + a.out_coff + c] = (T)x;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ detect-head output 1x1
// The last convolution of each head branch (ultralytics Detect: cv2.x.2 = Conv2d(64, 4 * reg_max, 1), cv3.x.2 = Conv2d(c3, nc, 1);
// no activation, fp32 rows of the prediction buffer) is a GEMM with K = 64..256 and <= 64 output channels: 1-4 K slabs, so the
// generic 128 px x 64 ch tile spends its time in prologue, barriers and epilogue (35 TFLOP/s; the layer is HBM-bound at 0.4-0.5 KB
// per pixel).  Here the WEIGHTS ARE STATIONARY: a workgroup copies the layer's whole packed filter (8-48 KB) to LDS once, in the
// generic kernel's swizzled image, and its four waves then stream 32-pixel groups of the flattened batch (grid-stride over groups):
// a lane loads its MFMA B operand -- 16 bytes of a pixel -- straight from global memory one K chunk ahead of the MFMAs that use
// it, across group boundaries, so the request stream never drains; no barrier after the fill.
// Per output value the MFMA chain is the generic kernel's (same instruction, same operands, same K order: chunks ascending, two
// K steps of 32 each, fp16x3: the virtual chunks [x_lo | x_hi (| x_hi)]) and so is the epilogue: results are bit-identical
// (tests/test_gpu_forward.py::test_head_output_kernel_is_bit_identical).  Rows of 16 packed weight rows that hold no real channel
// (nc = 5: two of four) are neither copied nor multiplied.  nrows = 16 * (row groups kept).
template <bool SPLIT>
__global__ __launch_bounds__(256) void head1x1_kernel(const ConvArgs a, const int nrows) {
    constexpr int MI = 2, PG = 16 * MI, D = 4;              // D: K chunks in flight per wave (register ring)
    constexpr int TP = 68;                                   // pitch (floats) of the store-transpose rows: conflict-free b128 writes and reads
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const int M = a.B * a.Ho * a.Wo, HoWo = a.Ho * a.Wo, cpad = pad128(a.Cout);
    const int pch = a.Cin / 64, vch = SPLIT ? a.split * pch : pch;
    const int niv = nrows >> 4;
    const bool tstore = a.Cout == 64 && a.out_f32;           // whole 64-float slices: stores go through a per-wave LDS transpose
    float* const tbuf = reinterpret_cast<float*>(smem + vch * nrows * 128) + wave * (PG * TP);

    for (int i = tid; i < vch * nrows * 8; i += 256) {
        const int q = i & 7, rr = i >> 3, r = rr % nrows, cc = rr / nrows;
        const u32x4 w = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(a.wgt) + ((size_t)cc * cpad + r) * 128 + q * 16);
        *reinterpret_cast<u32x4*>(smem + (cc * nrows + r) * 128 + ((q ^ (r & 7)) << 4)) = w;
    }
    __syncthreads();

    const auto rs0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.in0), 0, a.in0_bytes, 0x00020000);
    const int ngrp = (M + PG - 1) / PG, stride = gridDim.x * 4;
    const int cbase = fq * 16;
    float bv[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) bv[j] = a.bias[cbase + j];
    float sc[SPLIT ? 16 : 1];
    if constexpr (SPLIT) {
#pragma unroll
        for (int j = 0; j < 16; ++j) sc[j] = a.oscale[cbase + j];
    }

    u32x4 x[D][MI][2];
    int gi = blockIdx.x * 4 + wave, vi = 0;                 // issue cursor (group, virtual chunk)
    auto issue = [&](u32x4 (&xs)[MI][2]) {
        if (gi >= ngrp) return;
        int lo = 0;
        const int ccp = SPLIT ? x3_chunk(vi, pch, lo) : vi;
        const int lo0 = SPLIT && lo ? a.in0_lo : 0;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int m = gi * PG + mi * 16 + fr;
            const unsigned base = (unsigned)(m * a.in0_ct + a.in0_coff + lo0 + ccp * 64 + fq * 8) * 2;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) xs[mi][kk] = load_b128(rs0, m < M ? base + kk * 64 : CY_OOB, 0);
        }
        if (++vi == vch) { vi = 0; gi += stride; }
    };

    f32x4 acc[4][MI];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};

    int g = gi, v = 0;                                       // compute cursor
    auto step = [&](u32x4 (&xc)[MI][2], u32x4 (&xn)[MI][2]) {
        issue(xn);                                           // the slot the previous step consumed
        const char* Wl = smem + v * nrows * 128;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int qf = fq + 4 * kk;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                if (ni < niv) {
                    const int r = ni * 16 + fr;
                    const f16x8 wb = *reinterpret_cast<const f16x8*>(Wl + r * 128 + ((qf ^ (r & 7)) << 4));
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi)
                        acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb, __builtin_bit_cast(f16x8, xc[mi][kk]), acc[ni][mi], 0, 0, 0);
                }
            }
        }
        if (++v < vch) return;
        v = 0;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int m = g * PG + mi * 16 + fr;
            float o[16];
            if constexpr (SPLIT) {
                scale_bias_act16(acc[0][mi], acc[1][mi], acc[2][mi], acc[3][mi], bv, sc, a.act != 0, o);
            } else {
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float xo = acc[ni][mi][j] + bv[ni * 4 + j];
                        if (a.act) xo = silu_fast(xo);
                        o[ni * 4 + j] = xo;
                    }
            }
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (!a.out_f32) {
                // narrow 1x1 layers inside the network (YOLO11 C3k branches, small YOLOv8 scales): fp16 (or high / low halves) into a
                // channel slice, optional residual -- the generic kernel's epilogue, value for value
                if (m >= M) continue;
                const long oidx = (long)m * a.out_ct + a.out_coff + cbase, ridx = (long)m * a.res_ct + a.res_coff + cbase;
                if constexpr (SPLIT) store_px_split(reinterpret_cast<f16*>(a.out), oidx, a.out_lo, reinterpret_cast<const f16*>(a.res), ridx, a.res_lo, cbase, a.Cout, o, LoadRes{});
                else store_px(reinterpret_cast<f16*>(a.out), oidx, reinterpret_cast<const f16*>(a.res), ridx, cbase, a.Cout, o, LoadRes{});
                continue;
            }
            if (tstore) {
#pragma unroll
                for (int j4 = 0; j4 < 4; ++j4)
                    *reinterpret_cast<f32x4*>(tbuf + (mi * 16 + fr) * TP + cbase + 4 * j4) = f32x4{o[4 * j4], o[4 * j4 + 1], o[4 * j4 + 2], o[4 * j4 + 3]};
                continue;
            }
            if (m >= M) continue;
            const int b = m / HoWo, r = m - b * HoWo;
            float* dst = reinterpret_cast<float*>(a.out) + ((long)b * a.out_bs + a.out_ro + r) * a.out_ct + a.out_coff + cbase;
            if (cbase + 16 <= a.Cout) {
                typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
#pragma unroll
                for (int j4 = 0; j4 < 4; ++j4)
                    *reinterpret_cast<f32x4u*>(dst + 4 * j4) = f32x4u{o[4 * j4], o[4 * j4 + 1], o[4 * j4 + 2], o[4 * j4 + 3]};
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (cbase + j < a.Cout) dst[j] = o[j];
            }
        }
        if (tstore) {
            // wave-private transpose: a store instruction now covers four pixels' 256-byte slices (16 lanes x 16 bytes each) instead
            // of 16-byte pieces of sixteen different rows
            typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int i = 0; i < PG / 4; ++i) {
                const int px = 4 * i + fq, m = g * PG + px;
                const f32x4 t = *reinterpret_cast<const f32x4*>(tbuf + px * TP + fr * 4);
                if (m < M) {
                    const int b = m / HoWo, r = m - b * HoWo;
                    float* dst = reinterpret_cast<float*>(a.out) + ((long)b * a.out_bs + a.out_ro + r) * a.out_ct + a.out_coff + fr * 4;
                    *reinterpret_cast<f32x4u*>(dst) = f32x4u{t[0], t[1], t[2], t[3]};
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // the transpose rows are free again before the next group writes them
        }
        g += stride;
    };

#pragma unroll
    for (int d = 0; d < D - 1; ++d) issue(x[d]);
    while (true) {
        if (g >= ngrp) break;
        step(x[0], x[3]);
        if (g >= ngrp) break;
        step(x[1], x[0]);
        if (g >= ngrp) break;
        step(x[2], x[1]);
        if (g >= ngrp) break;
        step(x[3], x[2]);
    }
}

// Both output convolutions of one stride level in ONE launch (default; CY_HEAD_PAIR=0: one launch each): a workgroup (8 waves) holds
// both filters in LDS, a wave streams the K chunks of its 32 pixels from the box branch (64 channels) and then from the class
// branch (256) through the same register ring, keeps two accumulator sets, and writes WHOLE prediction rows: the 64 + nc floats
// of 16 pixels go through a wave-private LDS tile and leave as one contiguous run of dword stores (16 x 276 bytes for nc = 5)
// instead of a 256-byte slice and a 20-byte slice per row from two kernels.  Same MFMA chains, same epilogue arithmetic: bit-identical.
template <bool SPLIT>
__global__ __launch_bounds__(512) void head1x1_pair_kernel(const ConvArgs a, const ConvArgs b, const int nrows_b, const int TP) {
    constexpr int MI = 2, PG = 16 * MI, D = 4, NW = 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const int M = a.B * a.Ho * a.Wo, HoWo = a.Ho * a.Wo;
    const int pcha = a.Cin / 64, vcha = SPLIT ? a.split * pcha : pcha;
    const int pchb = b.Cin / 64, vchb = SPLIT ? b.split * pchb : pchb;
    const int vch = vcha + vchb, nivb = nrows_b >> 4, rowlen = a.out_ct;
    char* const Wa = smem;
    char* const Wb = smem + vcha * 64 * 128;
    float* const tbuf = reinterpret_cast<float*>(Wb + vchb * nrows_b * 128) + wave * (16 * TP);

    {
        const int cpa = pad128(a.Cout), cpb = pad128(b.Cout);
        for (int i = tid; i < vcha * 64 * 8; i += NW * 64) {
            const int q = i & 7, rr = i >> 3, r = rr & 63, cc = rr >> 6;
            const u32x4 w = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(a.wgt) + ((size_t)cc * cpa + r) * 128 + q * 16);
            *reinterpret_cast<u32x4*>(Wa + (cc * 64 + r) * 128 + ((q ^ (r & 7)) << 4)) = w;
        }
        for (int i = tid; i < vchb * nrows_b * 8; i += NW * 64) {
            const int q = i & 7, rr = i >> 3, r = rr % nrows_b, cc = rr / nrows_b;
            const u32x4 w = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(b.wgt) + ((size_t)cc * cpb + r) * 128 + q * 16);
            *reinterpret_cast<u32x4*>(Wb + (cc * nrows_b + r) * 128 + ((q ^ (r & 7)) << 4)) = w;
        }
    }
    __syncthreads();

    const auto rsa = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.in0), 0, a.in0_bytes, 0x00020000);
    const auto rsb = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(b.in0), 0, b.in0_bytes, 0x00020000);
    const int ngrp = (M + PG - 1) / PG, stride = gridDim.x * NW;
    const int cbase = fq * 16;
    float bva[16], bvb[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) { bva[j] = a.bias[cbase + j]; bvb[j] = b.bias[cbase + j]; }
    float sca[SPLIT ? 16 : 1], scb[SPLIT ? 16 : 1];
    if constexpr (SPLIT) {
#pragma unroll
        for (int j = 0; j < 16; ++j) { sca[j] = a.oscale[cbase + j]; scb[j] = b.oscale[cbase + j]; }
    }

    u32x4 x[D][MI][2];
    int gi = blockIdx.x * NW + wave, vi = 0;
    auto issue = [&](u32x4 (&xs)[MI][2]) {
        if (gi >= ngrp) return;
        const bool sb = vi >= vcha;                          // wave-uniform: which branch this chunk belongs to
        const int vv = sb ? vi - vcha : vi, pch = sb ? pchb : pcha;
        int lo = 0;
        const int ccp = SPLIT ? x3_chunk(vv, pch, lo) : vv;
        const int ct = sb ? b.in0_ct : a.in0_ct, coff = sb ? b.in0_coff : a.in0_coff;
        const int lo0 = SPLIT && lo ? (sb ? b.in0_lo : a.in0_lo) : 0;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int m = gi * PG + mi * 16 + fr;
            const unsigned base = (unsigned)(m * ct + coff + lo0 + ccp * 64 + fq * 8) * 2;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const unsigned off = m < M ? base + kk * 64 : CY_OOB;
                xs[mi][kk] = sb ? load_b128(rsb, off, 0) : load_b128(rsa, off, 0);
            }
        }
        if (++vi == vch) { vi = 0; gi += stride; }
    };

    f32x4 acca[4][MI], accb[4][MI];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) { acca[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f}; accb[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    int g = gi, v = 0;
    auto step = [&](u32x4 (&xc)[MI][2], u32x4 (&xn)[MI][2]) {
        issue(xn);
        if (v < vcha) {
            const char* Wl = Wa + v * 64 * 128;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int qf = fq + 4 * kk;
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    const int r = ni * 16 + fr;
                    const f16x8 wb = *reinterpret_cast<const f16x8*>(Wl + r * 128 + ((qf ^ (r & 7)) << 4));
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi)
                        acca[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb, __builtin_bit_cast(f16x8, xc[mi][kk]), acca[ni][mi], 0, 0, 0);
                }
            }
        } else {
            const char* Wl = Wb + (v - vcha) * nrows_b * 128;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int qf = fq + 4 * kk;
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    if (ni < nivb) {
                        const int r = ni * 16 + fr;
                        const f16x8 wb = *reinterpret_cast<const f16x8*>(Wl + r * 128 + ((qf ^ (r & 7)) << 4));
#pragma unroll
                        for (int mi = 0; mi < MI; ++mi)
                            accb[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb, __builtin_bit_cast(f16x8, xc[mi][kk]), accb[ni][mi], 0, 0, 0);
                    }
                }
            }
        }
        if (++v < vch) return;
        v = 0;
        const int mg = g * PG;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            float oa[16], ob[16];
            if constexpr (SPLIT) {
                scale_bias_act16(acca[0][mi], acca[1][mi], acca[2][mi], acca[3][mi], bva, sca, false, oa);
                scale_bias_act16(accb[0][mi], accb[1][mi], accb[2][mi], accb[3][mi], bvb, scb, false, ob);
            } else {
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int j = 0; j < 4; ++j) { oa[ni * 4 + j] = acca[ni][mi][j] + bva[ni * 4 + j]; ob[ni * 4 + j] = accb[ni][mi][j] + bvb[ni * 4 + j]; }
            }
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) { acca[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f}; accb[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f}; }
            float* trow = tbuf + fr * TP;
#pragma unroll
            for (int j4 = 0; j4 < 4; ++j4)
                *reinterpret_cast<f32x4*>(trow + cbase + 4 * j4) = f32x4{oa[4 * j4], oa[4 * j4 + 1], oa[4 * j4 + 2], oa[4 * j4 + 3]};
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (cbase + j < b.Cout) trow[64 + cbase + j] = ob[j];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            // 16 whole rows: one contiguous run in the prediction buffer unless the run crosses into the next image
            const int m0 = mg + mi * 16;
            const int npx = M - m0 < 16 ? M - m0 : 16;
            if (npx > 0) {
                const int b0 = m0 / HoWo, r0 = m0 - b0 * HoWo;
                float* const obase = reinterpret_cast<float*>(a.out);
                const int nit = (16 * rowlen + 63) >> 6;
                int px = 0, c = lane;
                for (int i = 0; i < nit; ++i) {
                    if (px < npx) {
                        int r = r0 + px, bb = b0;
                        while (r >= HoWo) { r -= HoWo; ++bb; }
                        obase[((long)bb * a.out_bs + a.out_ro + r) * rowlen + c] = tbuf[px * TP + c];
                    }
                    c += 64;
                    if (c >= rowlen) { c -= rowlen; ++px; }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        g += stride;
    };

#pragma unroll
    for (int d = 0; d < D - 1; ++d) issue(x[d]);
    while (true) {
        if (g >= ngrp) break;
        step(x[0], x[3]);
        if (g >= ngrp) break;
        step(x[1], x[0]);
        if (g >= ngrp) break;
        step(x[2], x[1]);
        if (g >= ngrp) break;
        step(x[3], x[2]);
    }
}

// ------------------------------------------------------------------------------------------------ 3x3 stride-1, halo reuse
// 90 % of the network's FLOPs are 3x3 stride-1 convolutions.  As a plain implicit GEMM every filter tap re-fetches its
// im2col rows, so a 128x128 tile moves 32 KB L2->LDS per 2.1 MFLOP (64 flop/B) and the kernel is bound by the L2->LDS
// path, not by the matrix cores.  Here a workgroup owns a TH x 16 patch of output pixels of one image: per 64-channel
// slab it stages the (TH+2) x 18 input halo ONCE and the nine taps read it at shifted rows (the MFMA B-operand row of a
// lane is a pixel, so a tap is just a row offset in the LDS image), while only the 128 x 64 weight slab changes per tap.
// L2->LDS traffic per flop drops ~3x (TH=16: 185 KB per 37.7 MFLOP = 204 flop/B).  Zero padding of the halo and of
// ragged image edges comes from the buffer range check, as in the generic kernel.

template <int WM, int RING>
__global__ __launch_bounds__(WM * 128) void conv3x3_halo_kernel(const ConvArgs a) {
    constexpr int TH = 4 * WM, TW = 16, NT = WM * 128, NW = NT / 64, BN = 128;
    constexpr int PR = (TH + 2) * (TW + 2);                 // halo rows (one row = one pixel, 64 channels = 128 B)
    constexpr int NWI = (PR + 7) / 8;                        // wave-instructions per halo load (8 rows each)
    constexpr int PROUNDS = (NWI + NW - 1) / NW;             // every wave issues exactly PROUNDS pieces (uniform vmcnt)
    constexpr int P_BYTES = PROUNDS * NW * 1024, W_BYTES = BN * 128;
    constexpr int WROUNDS = (BN / 8) / NW;
    constexpr int DIST = RING - 1;                           // weight slabs in flight: tap t+DIST is fetched while tap t computes
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const Pbuf = smem;
    char* const Wbuf = smem + 2 * P_BYTES;               // [halo 0 | halo 1 | weight ring]
    typedef __attribute__((address_space(3))) void lds_void;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int H = a.Hi, W = a.Wi;
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const int cpad = pad128(a.Cout);                      // packed weight rows (zero rows past Cout)
    const int ntn = (pad64(a.Cout) + BN - 1) / BN;
    const int id = xcd_remap(blockIdx.x, gridDim.x);
    const int nt = id % ntn;
    int rest = id / ntn;
    const int tx = rest % tiles_x; rest /= tiles_x;
    const int ty = rest % tiles_y;
    const int b = rest / tiles_y;
    const int y0 = ty * TH, x0 = tx * TW, n0 = nt * BN;
    const int chunks = a.Cin / 64;

    const auto rs0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.in0), 0, a.in0_bytes, 0x00020000);
    const auto rsw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wgt), 0, a.wgt_bytes, 0x00020000);

    // ---- per-thread halo geometry: round j moves halo row (j*NW + wave)*8 + (lane>>3), LDS slot lane&7
    unsigned poff[PROUNDS];
#pragma unroll
    for (int j = 0; j < PROUNDS; ++j) {
        const int wi = j * NW + wave;
        const int r = wi * 8 + (lane >> 3);
        const int ry = r / (TW + 2), rx = r - ry * (TW + 2);
        const int y = y0 + ry - 1, x = x0 + rx - 1;
        const int q = (lane & 7) ^ (r & 7);
        const bool ok = r < PR && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        poff[j] = ok ? (unsigned)(((b * H + y) * W + x) * a.in0_ct + a.in0_coff + q * 8) * 2u : CY_OOB;
    }
    unsigned woff[WROUNDS];
#pragma unroll
    for (int j = 0; j < WROUNDS; ++j) {
        const int row = (j * NW + wave) * 8 + (lane >> 3);
        const int q = (lane & 7) ^ (row & 7);
        woff[j] = (unsigned)((n0 + row) * 128 + q * 16);
    }
    auto dma_patch = [&](int buf, int ch) {
#pragma unroll
        for (int j = 0; j < PROUNDS; ++j) {
            const int wi = j * NW + wave;                   // rows >= PR land in the padded tail of the buffer as zeros
            const unsigned off = poff[j] == CY_OOB ? CY_OOB : poff[j] + (unsigned)(ch * 128);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, (lds_void*)(Pbuf + buf * P_BYTES + wi * 1024), 16, off, 0, 0, 0);
        }
    };
    auto dma_w = [&](int buf, int ch, int tap) {
#pragma unroll
        for (int j = 0; j < WROUNDS; ++j) {
            const unsigned off = woff[j] + (unsigned)((ch * 9 + tap) * cpad * 128);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_void*)(Wbuf + buf * W_BYTES + (j * NW + wave) * 1024), 16, off, 0, 0, 0);
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fq = lane >> 4;

    auto compute = [&](const char* P, const char* Wb, int kh, int kw) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int qf = fq + 4 * kk;
            f16x8 xa[4], wb[4];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const int r = (wm * 4 + mi + kh) * (TW + 2) + kw + fr;
                xa[mi] = *reinterpret_cast<const f16x8*>(P + r * 128 + ((qf ^ (r & 7)) << 4));
            }
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int r = wn * 64 + ni * 16 + fr;
                wb[ni] = *reinterpret_cast<const f16x8*>(Wb + r * 128 + ((qf ^ (r & 7)) << 4));
            }
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
                    acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb[ni], xa[mi], acc[ni][mi], 0, 0, 0);
        }
    };

    // ---- pipeline.  Weight slabs live in a 3-slot ring: the slab of tap t+2 is requested while tap t computes, so the
    // wait in front of a barrier only covers a DMA issued a whole tap earlier (counted vmcnt, raw s_barrier: the most
    // recent requests stay in flight across the barrier).  The next 64-channel halo is requested at tap 0 of a slab.
    const int total = chunks * 9;
    auto w_issue = [&](int n) { const int ch = n / 9; dma_w(n % RING, ch, n - ch * 9); };
    dma_patch(0, 0);
    w_issue(0);
    if (DIST > 1 && total > 1) { w_issue(1); CY_WAIT_VM((DIST - 1) * WROUNDS); } else { CY_WAIT_VM(0); }
    __builtin_amdgcn_s_barrier();
    int it = 0;
    const bool stamps = CY_STAMPS_ENABLED && (a.dbg & 64) != 0;
    unsigned long long acc_dma = 0, acc_cmp = 0, acc_wait = 0, acc_bar = 0;
    const unsigned long long t_begin = stamps ? stamp_now() : 0;
    for (int ch = 0; ch < chunks; ++ch) {
        const char* P = Pbuf + (ch & 1) * P_BYTES;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap, ++it) {
            const bool pre_p = tap == 0 && ch + 1 < chunks, pre_w = it + DIST < total;
            unsigned long long t0 = 0, t1 = 0, t2 = 0, t3 = 0;
            if (stamps) { __builtin_amdgcn_sched_barrier(0); t0 = stamp_now(); __builtin_amdgcn_sched_barrier(0); }
            if (pre_p) dma_patch((ch + 1) & 1, ch + 1);
            if (pre_w) w_issue(it + DIST);
            if (stamps) { __builtin_amdgcn_sched_barrier(0); t1 = stamp_now(); __builtin_amdgcn_sched_barrier(0); }
            const int kh = tap / 3, kw = tap - kh * 3;
            compute(P, Wbuf + (it % RING) * W_BYTES, kh, kw);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // this tap's fragment reads are done (WAR on the ring)
            if (stamps) { __builtin_amdgcn_sched_barrier(0); t2 = stamp_now(); __builtin_amdgcn_sched_barrier(0); }
            if (pre_w && DIST > 1) { CY_WAIT_VM((DIST - 1) * WROUNDS); }   // all but the newest slab request have landed
            else { CY_WAIT_VM(0); }
            if (stamps) { __builtin_amdgcn_sched_barrier(0); t3 = stamp_now(); __builtin_amdgcn_sched_barrier(0); }
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            if (stamps) {
                __builtin_amdgcn_sched_barrier(0);
                const unsigned long long t4 = stamp_now();
                acc_dma += t1 - t0; acc_cmp += t2 - t1; acc_wait += t3 - t2; acc_bar += t4 - t3;
            }
        }
    }

    if (stamps && lane == 0) {
        const unsigned long long t_end = stamp_now();
        atomicAdd(&g_stamps[0], acc_dma); atomicAdd(&g_stamps[1], acc_cmp); atomicAdd(&g_stamps[2], acc_wait);
        atomicAdd(&g_stamps[3], acc_bar); atomicAdd(&g_stamps[4], t_end - t_begin); atomicAdd(&g_stamps[5], (unsigned long long)total);
        atomicAdd(&g_stamps[6], 1ull);
    }
    // ---- epilogue (same per-lane channel layout as the generic kernel)
    const int cbase = n0 + wn * 64 + fq * 16;
    float bv[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) bv[j] = a.bias[cbase + j];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const int y = y0 + wm * 4 + mi, x = x0 + fr;
        if (y >= H || x >= W) continue;
        const long pix = ((long)b * H + y) * W + x;
        float v[16];
        bias_act16(acc[0][mi], acc[1][mi], acc[2][mi], acc[3][mi], bv, a.act != 0, v);
        store_px(reinterpret_cast<f16*>(a.out), pix * a.out_ct + a.out_coff + cbase, reinterpret_cast<const f16*>(a.res),
                 pix * a.res_ct + a.res_coff + cbase, cbase, a.Cout, v, LoadRes{});
    }
}

// ------------------------------------------------------------------------------------------------ 3x3 stride-1, ping-pong
// Same data flow as conv3x3_halo_kernel (halo staged once per 64-channel slab, weights per tap), but the eight waves of
// the workgroup run as two groups half an iteration apart (waves 0-3 / 4-7 = the two waves of each SIMD): while one
// group issues its DMA pieces and fragment reads for tap t, its SIMD partner is on the matrix pipe with tap t (or t-1).
// PMC on the lock-step version showed every SIMD's MFMA pipe only ~45 % busy with both waves waiting at the same
// barrier; staggering by wave >= 4 is what MI355X_MICROARCH.md ("Two waves per SIMD", item 9) measures as the fix.
//   group A (waves 0-3): LOAD(t) at half-step 2t,   COMPUTE(t) at 2t+1
//   group B (waves 4-7): LOAD(t) at half-step 2t+1, COMPUTE(t) at 2t+2      (one s_barrier ends every half-step)
// Weight slabs sit in a 4-slot ring and are requested two taps ahead: slot (t+2)%4 last held tap t-2, whose last reader
// (B, half-step 2t-2) is done before A issues at 2t.  The halo of slab ch+1 is requested at tap 1 of slab ch.
// Each wave waits (counted vmcnt) for everything but its newest requests at the end of LOAD; the following barrier
// publishes the landed pieces to all readers.
template <int NI>
__global__ __launch_bounds__(512) void conv3x3_pp_kernel(const ConvArgs a) {
    constexpr int TH = 16, TW = 16, NW = 8, WN = 2, BN = WN * NI * 16, RING = 4;
    constexpr int PR = (TH + 2) * (TW + 2), NWI = (PR + 7) / 8, PROUNDS = (NWI + NW - 1) / NW;
    constexpr int P_BYTES = (NWI + 1) * 1024, W_BYTES = BN * 128;       // +1 KB dummy row block for the padded rounds
    constexpr int WPIECES = BN / 8, WROUNDS = (WPIECES + NW - 1) / NW;  // BN=128: 2 per wave; BN=64: 1 per wave
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const Pbuf = smem;
    char* const Wbuf = smem + 2 * P_BYTES;
    typedef __attribute__((address_space(3))) void lds_void;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;
    const int wm = wave >> 1, wn = wave & 1;
    const int H = a.Hi, W = a.Wi;
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const int cpad = pad128(a.Cout);                      // packed weight rows (zero rows past Cout)
    const int ntn = (pad64(a.Cout) + BN - 1) / BN;
    const int id = xcd_remap(blockIdx.x, gridDim.x);
    const int nt = id % ntn;
    int rest = id / ntn;
    const int tx = rest % tiles_x; rest /= tiles_x;
    const int ty = rest % tiles_y;
    const int b = rest / tiles_y;
    const int y0 = ty * TH, x0 = tx * TW, n0 = nt * BN;
    const int chunks = a.Cin / 64, total = chunks * 9;

    const auto rs0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.in0), 0, a.in0_bytes, 0x00020000);
    const auto rsw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wgt), 0, a.wgt_bytes, 0x00020000);

    unsigned poff[PROUNDS];
#pragma unroll
    for (int j = 0; j < PROUNDS; ++j) {
        const int r = (j * NW + wave) * 8 + (lane >> 3);
        const int ry = r / (TW + 2), rx = r - ry * (TW + 2);
        const int y = y0 + ry - 1, x = x0 + rx - 1;
        const int q = (lane & 7) ^ (r & 7);
        const bool ok = r < PR && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        poff[j] = ok ? (unsigned)(((b * H + y) * W + x) * a.in0_ct + a.in0_coff + q * 8) * 2u : CY_OOB;
    }
    unsigned woff[WROUNDS];
#pragma unroll
    for (int j = 0; j < WROUNDS; ++j) {
        const int row = ((j * NW + wave) % WPIECES) * 8 + (lane >> 3);
        const int q = (lane & 7) ^ (row & 7);
        woff[j] = (unsigned)((n0 + row) * 128 + q * 16);
    }
    auto dma_patch = [&](int buf, int ch) {
#pragma unroll
        for (int j = 0; j < PROUNDS; ++j) {
            const int wi = j * NW + wave;
            const unsigned off = poff[j] == CY_OOB ? CY_OOB : poff[j] + (unsigned)(ch * 128);
            char* dst = Pbuf + buf * P_BYTES + (wi < NWI ? wi : NWI) * 1024;      // rounds past the halo hit the dummy block
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, (lds_void*)dst, 16, off, 0, 0, 0);
        }
    };
    auto dma_w = [&](int n) {                               // weight slab of global tap index n -> ring slot n % RING
        const int ch = n / 9, tap = n - ch * 9;
#pragma unroll
        for (int j = 0; j < WROUNDS; ++j) {
            const unsigned off = woff[j] + (unsigned)((ch * 9 + tap) * cpad * 128);
            char* dst = Wbuf + (n % RING) * W_BYTES + ((j * NW + wave) % WPIECES) * 1024;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_void*)dst, 16, off, 0, 0, 0);
        }
    };

    f32x4 acc[NI][4];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fq = lane >> 4;
    f16x8 xa0[4], wb0[NI], xa1[4], wb1[NI];

    auto read_frags = [&](const char* P, const char* Wb, int kh, int kw, int kk, f16x8* xa, f16x8* wb) {
        const int qf = fq + 4 * kk;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int r = (wm * 4 + mi + kh) * (TW + 2) + kw + fr;
            xa[mi] = *reinterpret_cast<const f16x8*>(P + r * 128 + ((qf ^ (r & 7)) << 4));
        }
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            const int r = wn * (NI * 16) + ni * 16 + fr;
            wb[ni] = *reinterpret_cast<const f16x8*>(Wb + r * 128 + ((qf ^ (r & 7)) << 4));
        }
    };
    auto mfma_all = [&](const f16x8* xa, const f16x8* wb) {
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb[ni], xa[mi], acc[ni][mi], 0, 0, 0);
    };

    // ---- prologue: halo 0 and the first two weight slabs, fully landed before anyone reads
    dma_patch(0, 0);
    dma_w(0);
    if (total > 1) dma_w(1);
    CY_WAIT_VM(0);
    __builtin_amdgcn_s_barrier();
    if (grp == 1) __builtin_amdgcn_s_barrier();             // group B runs half an iteration behind

    int it = 0;
#pragma unroll 1
    for (int ch = 0; ch < chunks; ++ch) {
        const char* P = Pbuf + (ch & 1) * P_BYTES;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap, ++it) {
            const char* Wb = Wbuf + (it % RING) * W_BYTES;
            const int kh = tap / 3, kw = tap - kh * 3;
            // -------- LOAD(it): requests two taps ahead, fragment reads of the first 32 channels
            const bool pre_p = tap == 1 && ch + 1 < chunks, pre_w = it + 2 < total;
            if (pre_w) dma_w(it + 2);
            if (pre_p) dma_patch((ch + 1) & 1, ch + 1);      // issued after the slab so the halo may stay in flight
            read_frags(P, Wb, kh, kw, 0, xa0, wb0);
            if (pre_p) { CY_WAIT_VM(WROUNDS + PROUNDS); }    // the slab of tap it+1 (requested last iteration) has landed
            else if (pre_w) { CY_WAIT_VM(WROUNDS); }
            else { CY_WAIT_VM(0); }
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            // -------- COMPUTE(it)
            read_frags(P, Wb, kh, kw, 1, xa1, wb1);
            __builtin_amdgcn_sched_barrier(0);
            if (a.dbg & 32) __builtin_amdgcn_s_setprio(1);
            mfma_all(xa0, wb0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            mfma_all(xa1, wb1);
            if (a.dbg & 32) __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
        }
    }
    if (grp == 0) __builtin_amdgcn_s_barrier();             // pairs with group B's last barrier

    // ---- epilogue: lane owns NI*4 contiguous channels of one pixel
    // packed weight row wn*NI*16 + ni*16 + rr holds channel 64*blk + 16*(rr>>2) + 4*ni_g + (rr&3), ni_g = (wn*NI+ni)&3
    const int cbase = n0 + ((wn * NI) >> 2) * 64 + fq * 16 + ((wn * NI) & 3) * 4;
    float bv[NI * 4];
#pragma unroll
    for (int j = 0; j < NI * 4; ++j) bv[j] = a.bias[cbase + j];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const int y = y0 + wm * 4 + mi, x = x0 + fr;
        if (y >= H || x >= W) continue;
        const long pix = ((long)b * H + y) * W + x;
        float v[NI * 4];
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float t = acc[ni][mi][j] + bv[ni * 4 + j];
                if (a.act) t = silu_fast(t);
                v[ni * 4 + j] = t;
            }
        store_px(reinterpret_cast<f16*>(a.out), pix * a.out_ct + a.out_coff + cbase, reinterpret_cast<const f16*>(a.res),
                 pix * a.res_ct + a.res_coff + cbase, cbase, a.Cout, v, LoadRes{});
    }
}

template <int NI>
static hipError_t launch_pp(const ConvArgs& a, hipStream_t s) {
    constexpr int BN = 2 * NI * 16, PR = 18 * 18, NWI = (PR + 7) / 8;
    const size_t lds = 2 * (NWI + 1) * 1024 + 4 * BN * 128;
    const int blocks = a.B * ((a.Hi + 15) / 16) * ((a.Wi + 15) / 16) * ((pad64(a.Cout) + BN - 1) / BN);
    return launch_lds<conv3x3_pp_kernel<NI>>(dim3(blocks), dim3(512), lds, lds, s, a);
}

// ------------------------------------------------------------------------------------------------ 3x3 s1, Cin = 64: persistent
// The six bottleneck convolutions of the full-resolution C2f (64 -> 64 channels over 1M pixels per 64-tile batch) have
// only nine K-slabs per output patch, so a one-patch-per-workgroup kernel spends most of its time in prologue/epilogue
// (measured: 16 rounds x ~10 us).  Here a workgroup is persistent (one per CU): the whole 64 x (9 x 64) weight panel is
// staged in LDS ONCE (72 KB) next to two input-halo buffers (2 x 42 KB), and the nine taps of a patch run without a barrier.
// KC = input channels (64, or 32 with 64-byte LDS rows and the 64-byte-chunk weight copy: the 32-channel bottlenecks of the
// n/s scales and of YOLO11's C3k blocks; the output side still walks all 64 packed rows, half of them zero for Cout = 32).
//
// Two wave groups.  Round 1's form had four waves (one per SIMD) and a double-buffered halo; its in-kernel stamps showed, per
// patch and wave, 6.2k cycles of fragment reads + MFMAs, 5.2k of epilogue (bias, SiLU, residual, stores), 1.9k of LDS-DMA issue
// and next to no waiting -- with ONE wave per SIMD all of it is serial.  Now a workgroup has 8 waves = two groups of four
// (waves w and w + 4 share a SIMD); its patches alternate between the groups, and in every phase one group runs the MFMAs of
// its patch while the other runs the "back" of its previous one: request the halo of its next patch into its own (single)
// halo buffer, epilogue, wait.  One workgroup barrier per phase orders both hand-overs (halo landed -> readable; halo read ->
// writable).  256 tiles of 128x128x64: 0.43-0.48 -> 0.35-0.39 ms per conv (3.5 TB/s of HBM traffic without, 4.5 TB/s with a
// residual input: the kernel is now bound by memory, not by issue; making the halo requests and the epilogue cheaper -- uniform
// address parts in soffset, an interior-patch path without border tests, packed fp32 math -- no longer moved it).
template <int KC, bool ACT, bool RES>
__global__ __launch_bounds__(512) void conv3x3_c64_kernel(const ConvArgs a) {
    constexpr int TH = 16, TW = 16, NG = 4, NI = 4;      // NG waves per group, each 64 px x 64 ch
    constexpr int RB = KC * 2, RPP = 1024 / RB, NCH = KC / 8, KK = KC / 32;
    constexpr int PR = (TH + 2) * (TW + 2), NWI = (PR + RPP - 1) / RPP, PROUNDS = (NWI + NG - 1) / NG;
    auto swz = [](int chunk, int row) { return KC == 64 ? (chunk ^ (row & 7)) : (chunk ^ (((row >> 2) & 1) << 1)); };
    constexpr int P_BYTES = (NWI + 1) * 1024;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef __attribute__((address_space(3))) void lds_void;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, wm = wave & 3;
    const int fr = lane & 15, fq = lane >> 4;
    const int H = a.Hi, W = a.Wi;
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const int npatch = a.B * tiles_y * tiles_x;
    // halo requests: offset = (per-lane part, fixed for the whole launch, in voffset) + (per-patch part, uniform, in soffset).
    // soffset is unsigned and the per-patch part starts one row + one pixel before the patch, so the resource base is moved
    // back by that much (num_records widened to match); only voffset is range-checked: lanes outside the image get CY_OOB.
    const unsigned bias_bytes = (unsigned)((W + 1) * a.in0_ct) * 2u;
    const auto rs0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(a.in0)) - bias_bytes, 0,
                                                       a.in0_bytes + 2 * bias_bytes, 0x00020000);

    constexpr int W_BYTES = 9 * 64 * RB, WPIECES = W_BYTES / 1024, PPT = 64 / RPP;
    char* const Wl = smem;
    char* const P = smem + W_BYTES + grp * P_BYTES;           // this group's halo buffer
    {
        const auto rsw = KC == 64 ? __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wgt), 0, a.wgt_bytes, 0x00020000)
                                  : __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wgt32), 0, a.wgt32_bytes, 0x00020000);
#pragma unroll
        for (int j = 0; j < (WPIECES + 7) / 8; ++j) {
            const int pc = j * 8 + wave;
            if (pc >= WPIECES) break;                       // (36 pieces for KC = 32)
            const int tap = pc / PPT, row = (pc % PPT) * RPP + lane / NCH;
            const int q = swz(lane % NCH, row);
            const unsigned off = (unsigned)((tap * 128 + row) * RB + q * 16);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_void*)(Wl + pc * 1024), 16, off, 0, 0, 0);
        }
    }
    const int cbase = fq * 16;
    f32x2 bv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bv[j] = f32x2{a.bias[cbase + 2 * j], a.bias[cbase + 2 * j + 1]};

    // per-lane parts of the PROUNDS halo pieces this wave requests: byte offset relative to the halo's first pixel, and the
    // halo row / column (packed) for the border test
    unsigned rel[PROUNDS];
#pragma unroll
    for (int j = 0; j < PROUNDS; ++j) {
        const int wi = j * NG + wm;
        const int r = wi * RPP + lane / NCH;
        const int ry = r / (TW + 2), rx = r - ry * (TW + 2);
        const int q = swz(lane % NCH, r);
        rel[j] = r < PR ? (unsigned)(((ry * W + rx) * a.in0_ct + q * 8) * 2) : CY_OOB;
    }
    const int rlane = lane / NCH;
    auto dma_patch = [&](int pidx) {                       // by the four waves of the group that owns the patch
        const int tx = pidx % tiles_x, ty = (pidx / tiles_x) % tiles_y, b = pidx / (tiles_x * tiles_y);
        const int y0 = ty * TH, x0 = tx * TW;
        const unsigned so = bias_bytes + (unsigned)((((b * H + y0 - 1) * W + x0 - 1) * a.in0_ct + a.in0_coff) * 2);
        const bool interior = y0 >= 1 && x0 >= 1 && y0 + TH + 1 <= H && x0 + TW + 1 <= W;
        if (interior) {
#pragma unroll
            for (int j = 0; j < PROUNDS; ++j) {
                const int wi = j * NG + wm;
                dma_piece(rs0, (lds_ptr_t*)(P + (wi < NWI ? wi : NWI) * 1024), rel[j], so);
            }
        } else {
            // halo rows [ylo, yhi) and columns [xlo, xhi) are inside the image
            const int ylo = y0 >= 1 ? 0 : 1, yhi = H - y0 + 1, xlo = x0 >= 1 ? 0 : 1, xhi = W - x0 + 1;
#pragma unroll
            for (int j = 0; j < PROUNDS; ++j) {
                const int wi = j * NG + wm;
                const int r = wi * RPP + rlane, ry = (r * 3641) >> 16, rx = r - ry * (TW + 2);      // r / 18 for r < 400
                const bool ok = ry >= ylo && ry < yhi && rx >= xlo && rx < xhi;
                dma_piece(rs0, (lds_ptr_t*)(P + (wi < NWI ? wi : NWI) * 1024), ok ? rel[j] : CY_OOB, so);
            }
        }
    };

    // patch n of this workgroup = blockIdx.x + n * gridDim.x, owned by group n & 1; NP of them
    const int NP = (int)blockIdx.x < npatch ? (npatch - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
    if (grp < NP) dma_patch(blockIdx.x + grp * gridDim.x);
    // (the builtin, not inline asm: the compiler then knows that the bias loads above have landed; with the asm form it
    // put an `s_waitcnt vmcnt(0)` in front of the first use of bv[] INSIDE the loop, i.e. between the halo requests of a
    // back phase and its epilogue, which exposed the whole DMA latency there)
    __builtin_amdgcn_s_waitcnt(0x0F70);                    // vmcnt(0)
    __builtin_amdgcn_s_barrier();

    // fragment addresses as (one of a few lane-dependent bases) + (a compile-time offset): the swizzle of halo row R0 + c depends
    // on (R0 + c) & 7 only, and the second K half (chunk + 4) is the swizzle of row + 4, so eight bases cover all 72 fragments
    // of a patch (computed one by one they are 36 live registers, which at two waves per SIMD spill)
    const int R0 = wm * 4 * (TW + 2) + fr;
    unsigned xb[8], wb0[KK];
#pragma unroll
    for (int k8 = 0; k8 < 8; ++k8) xb[k8] = (unsigned)(R0 * RB + (swz(fq, (R0 + k8) & 7) << 4));
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) wb0[kk] = (unsigned)(fr * RB + (swz(fq + 4 * kk, fr) << 4));
    f32x4 acc[NI][4];
    const bool vec_out = cbase + 16 <= a.Cout;
    const int out_lane = fr * a.out_ct + cbase, res_lane = fr * a.res_ct + cbase;       // element offsets of the lane inside a patch row
    // phase ph: group ph & 1 runs the MFMAs of patch ph; the other group the back of patch ph - 1 (+ the halo of patch ph + 1)
    for (int ph = 0; ph <= NP; ++ph) {
        if ((ph & 1) == grp) {
            if (ph < NP) {
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
                f16x8 xa[2][4], wb[2][NI];
                auto load_group = [&](int g, f16x8* x, f16x8* w) {
                    const int tap = g / KK, kk = g % KK, kh = tap / 3, kw = tap - kh * 3;
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi) {
                        const int c = (mi + kh) * (TW + 2) + kw;                     // halo row = R0 + c
                        x[mi] = *reinterpret_cast<const f16x8*>(P + xb[(c + 4 * kk) & 7] + c * RB);
                    }
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
                        w[ni] = *reinterpret_cast<const f16x8*>(Wl + wb0[kk] + (tap * 64 + ni * 16) * RB);
                };
                load_group(0, xa[0], wb[0]);
#pragma unroll
                for (int g = 0; g < 9 * KK; ++g) {
                    if (g + 1 < 9 * KK) load_group(g + 1, xa[(g + 1) & 1], wb[(g + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                        for (int mi = 0; mi < 4; ++mi)
                            acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb[g & 1][ni], xa[g & 1][mi], acc[ni][mi], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this group is done reading its halo
            }
        } else if (ph >= 1) {
            f16x8 rres[4][2];
            const int pidx = blockIdx.x + (ph - 1) * gridDim.x;
            const int tx = pidx % tiles_x, ty = (pidx / tiles_x) % tiles_y, b = pidx / (tiles_x * tiles_y);
            const int yw = ty * TH + wm * 4, x = tx * TW + fr;                 // first of the wave's four rows; the lane's column
            const long rowpix = ((long)b * H + yw) * W + tx * TW;              // uniform: first pixel of the wave's first row
            const bool xok = x < W;
            if (RES) {                                     // residual of the patch: its latency hides under the DMA issue and the SiLUs below
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) {
                    const bool ok = yw + mi < H && xok && vec_out;
                    // (masked lanes read the start of the patch's first pixel: valid memory, never used)
                    const f16* rp = reinterpret_cast<const f16*>(a.res) + ((rowpix + (yw + mi < H ? (long)mi * W : 0)) * a.res_ct + a.res_coff) + (ok ? res_lane : 0);
                    rres[mi][0] = *reinterpret_cast<const f16x8*>(rp);
                    rres[mi][1] = *reinterpret_cast<const f16x8*>(rp + 8);
                }
            }
            if (ph + 1 < NP) dma_patch(blockIdx.x + (ph + 1) * gridDim.x);
            // bias + SiLU in place, two values per instruction where the ISA has a packed form
            if (ACT) {
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            f32x2 t = f32x2{acc[ni][mi][2 * h], acc[ni][mi][2 * h + 1]} + bv[ni * 2 + h];
                            f32x2 e = t * f32x2{-1.44269504088896341f, -1.44269504088896341f};
                            e = f32x2{__builtin_amdgcn_exp2f(e[0]), __builtin_amdgcn_exp2f(e[1])} + f32x2{1.0f, 1.0f};
                            t = t * f32x2{__builtin_amdgcn_rcpf(e[0]), __builtin_amdgcn_rcpf(e[1])};
                            acc[ni][mi][2 * h] = t[0]; acc[ni][mi][2 * h + 1] = t[1];
                        }
            } else {
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[ni][mi][j] += bv[ni * 2 + (j >> 1)][j & 1];
            }
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                if (yw + mi >= H) break;                   // (uniform)
                if (!xok) continue;
                if (vec_out) {
                    f16* dst = reinterpret_cast<f16*>(a.out) + ((rowpix + (long)mi * W) * a.out_ct + a.out_coff) + out_lane;
                    float v[16];
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[ni * 4 + j] = acc[ni][mi][j];
                    if (RES) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) { v[j] += (float)rres[mi][0][j]; v[8 + j] += (float)rres[mi][1][j]; }
                    }
                    f16x8 o0, o1;
#pragma unroll
                    for (int j = 0; j < 8; ++j) { o0[j] = (f16)v[j]; o1[j] = (f16)v[8 + j]; }
                    *reinterpret_cast<f16x8*>(dst) = o0;
                    *reinterpret_cast<f16x8*>(dst + 8) = o1;
                } else {
                    const long pix = rowpix + (long)mi * W + fr;
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const int c = cbase + j;
                        if (c >= a.Cout) continue;
                        float t = acc[j >> 2][mi][j & 3];
                        if (RES) t += (float)(reinterpret_cast<const f16*>(a.res)[pix * a.res_ct + a.res_coff + c]);
                        reinterpret_cast<f16*>(a.out)[pix * a.out_ct + a.out_coff + c] = (f16)t;
                    }
                }
            }
            CY_WAIT_VM(0);                                 // the halo requested above has landed (and the stores are out)
        }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int KC>
static hipError_t launch_c64(const ConvArgs& a, hipStream_t s) {
    constexpr int RPP = 1024 / (KC * 2), NWI = (18 * 18 + RPP - 1) / RPP;
    const size_t lds = 9 * 64 * KC * 2 + 2 * (NWI + 1) * 1024;
    lds_cap<conv3x3_c64_kernel<KC, true, false>>(lds);        // all four before the first launch of any
    lds_cap<conv3x3_c64_kernel<KC, true, true>>(lds);
    lds_cap<conv3x3_c64_kernel<KC, false, false>>(lds);
    lds_cap<conv3x3_c64_kernel<KC, false, true>>(lds);
    const int npatch = a.B * ((a.Hi + 15) / 16) * ((a.Wi + 15) / 16);
    const dim3 grid(npatch < 256 ? npatch : 256), block(512);                      // one persistent workgroup per CU
    if (a.act && a.res) return launch_lds<conv3x3_c64_kernel<KC, true, true>>(grid, block, lds, lds, s, a);
    if (a.act) return launch_lds<conv3x3_c64_kernel<KC, true, false>>(grid, block, lds, lds, s, a);
    if (a.res) return launch_lds<conv3x3_c64_kernel<KC, false, true>>(grid, block, lds, lds, s, a);
    return launch_lds<conv3x3_c64_kernel<KC, false, false>>(grid, block, lds, lds, s, a);
}

// ------------------------------------------------------------------------------------------------ 3x3 s1, two taps per barrier
// Variant of conv3x3_halo_kernel for 16x16-pixel patches (8 waves, one workgroup per CU, all 160 KiB of LDS): a pipeline
// stage holds the weight slabs of TWO taps, so a wave issues 64 MFMAs between barriers instead of 32 and the per-stage
// cost (DMA issue, vmcnt drain, s_barrier: ~600 cycles in the stamped build) is paid half as often.  Input channels are
// walked in pairs of 64-channel slabs (18 taps = 9 stages, fully unrolled, so every fragment address is a constant
// offset); the two halo buffers hold the even / odd slab of the pair and are refilled as soon as their last tap is done.
__global__ __launch_bounds__(512) void conv3x3_halo2_kernel(const ConvArgs a) {
    constexpr int TH = 16, TW = 16, NW = 8, BN = 128;
    constexpr int PR = (TH + 2) * (TW + 2), NWI = (PR + 7) / 8, PROUNDS = (NWI + NW - 1) / NW;
    constexpr int P_BYTES = PROUNDS * NW * 1024, SLAB = BN * 128, W_BYTES = 2 * SLAB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const Pbuf = smem;
    char* const Wbuf = smem + 2 * P_BYTES;
    typedef __attribute__((address_space(3))) void lds_void;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int H = a.Hi, W = a.Wi;
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const int cpad = pad128(a.Cout);                      // packed weight rows (zero rows past Cout)
    const int ntn = (pad64(a.Cout) + BN - 1) / BN;
    const int id = xcd_remap(blockIdx.x, gridDim.x);
    const int nt = id % ntn;
    int rest = id / ntn;
    const int tx = rest % tiles_x; rest /= tiles_x;
    const int ty = rest % tiles_y;
    const int b = rest / tiles_y;
    const int y0 = ty * TH, x0 = tx * TW, n0 = nt * BN;
    const int chunks = a.Cin / 64, pairs = chunks / 2;      // launch_conv guarantees an even number of slabs

    const auto rs0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.in0), 0, a.in0_bytes, 0x00020000);
    const auto rsw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wgt), 0, a.wgt_bytes, 0x00020000);
    unsigned poff[PROUNDS];
#pragma unroll
    for (int j = 0; j < PROUNDS; ++j) {
        const int r = (j * NW + wave) * 8 + (lane >> 3);
        const int ry = r / (TW + 2), rx = r - ry * (TW + 2);
        const int y = y0 + ry - 1, x = x0 + rx - 1;
        const int q = (lane & 7) ^ (r & 7);
        const bool ok = r < PR && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        poff[j] = ok ? (unsigned)(((b * H + y) * W + x) * a.in0_ct + a.in0_coff + q * 8) * 2u : CY_OOB;
    }
    unsigned woff[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = (j * NW + wave) * 8 + (lane >> 3);
        woff[j] = (unsigned)((n0 + row) * 128 + ((lane & 7) ^ (row & 7)) * 16);
    }
    auto dma_patch = [&](int buf, int ch) {
#pragma unroll
        for (int j = 0; j < PROUNDS; ++j) {
            // the uniform part of the offset goes in soffset, which is not range-checked: an OOB sentinel stays OOB
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, (lds_void*)(Pbuf + buf * P_BYTES + (j * NW + wave) * 1024), 16, poff[j], ch * 128, 0, 0);
        }
    };
    auto dma_slab = [&](int buf, int t, int ch, int tap) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (lds_void*)(Wbuf + buf * W_BYTES + t * SLAB + (j * NW + wave) * 1024), 16, woff[j], (ch * 9 + tap) * cpad * 128, 0, 0);
        }
    };
    f32x4 acc[4][4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fq = lane >> 4;
    auto compute = [&](const char* P, const char* Wb, int kh, int kw) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int qf = fq + 4 * kk;
            f16x8 xa[4], wb[4];
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const int r = (wm * 4 + mi + kh) * (TW + 2) + kw + fr;
                xa[mi] = *reinterpret_cast<const f16x8*>(P + r * 128 + ((qf ^ (r & 7)) << 4));
            }
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int r = wn * 64 + ni * 16 + fr;
                wb[ni] = *reinterpret_cast<const f16x8*>(Wb + r * 128 + ((qf ^ (r & 7)) << 4));
            }
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
                    acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb[ni], xa[mi], acc[ni][mi], 0, 0, 0);
        }
    };

    // prologue: halo of slab 0, weight stage 0 (taps 0,1 of slab 0)
    dma_patch(0, 0);
    dma_slab(0, 0, 0, 0);
    dma_slab(0, 1, 0, 1);
    __syncthreads();
    int g = 0;                                               // global stage counter: weight stage buffer = g & 1
    const bool stamps = CY_STAMPS_ENABLED && (a.dbg & 64) != 0;
    unsigned long long acc_dma = 0, acc_cmp = 0, acc_wait = 0, acc_bar = 0;
    const unsigned long long t_begin = stamps ? stamp_now() : 0;
    unsigned long long t0s = t_begin;
#pragma unroll 1
    for (int cp = 0; cp < pairs; ++cp) {
#pragma unroll
        for (int st = 0; st < 9; ++st, ++g) {
            // requests for the next stage / the halo buffers that have just become free
            if (st < 8) {
                const int u0 = 2 * (st + 1), u1 = u0 + 1;
                dma_slab((g + 1) & 1, 0, 2 * cp + u0 / 9, u0 % 9);
                dma_slab((g + 1) & 1, 1, 2 * cp + u1 / 9, u1 % 9);
            } else if (cp + 1 < pairs) {
                dma_slab((g + 1) & 1, 0, 2 * cp + 2, 0);
                dma_slab((g + 1) & 1, 1, 2 * cp + 2, 1);
            }
            if (st == 0) dma_patch(1, 2 * cp + 1);                                  // odd slab of this pair (needed from stage 4)
            if (st == 5 && cp + 1 < pairs) dma_patch(0, 2 * cp + 2);                // even slab of the next pair
            unsigned long long t1 = 0, t2 = 0, t3 = 0;
            if (stamps) { __builtin_amdgcn_sched_barrier(0); t1 = stamp_now(); __builtin_amdgcn_sched_barrier(0); }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int u = 2 * st + t, tap = u % 9;
                compute(Pbuf + (u / 9) * P_BYTES, Wbuf + (g & 1) * W_BYTES + t * SLAB, tap / 3, tap % 3);
            }
            if (stamps) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0); t2 = stamp_now(); __builtin_amdgcn_sched_barrier(0);
                CY_WAIT_VM(0);
                __builtin_amdgcn_sched_barrier(0); t3 = stamp_now(); __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
            if (stamps) {
                __builtin_amdgcn_sched_barrier(0);
                const unsigned long long t4 = stamp_now();
                acc_dma += t1 - t0s; acc_cmp += t2 - t1; acc_wait += t3 - t2; acc_bar += t4 - t3;
                t0s = t4;
            }
        }
    }

    if (stamps && lane == 0) {
        const unsigned long long t_end = stamp_now();
        atomicAdd(&g_stamps[0], acc_dma); atomicAdd(&g_stamps[1], acc_cmp); atomicAdd(&g_stamps[2], acc_wait);
        atomicAdd(&g_stamps[3], acc_bar); atomicAdd(&g_stamps[4], t_end - t_begin); atomicAdd(&g_stamps[5], (unsigned long long)(pairs * 9));
        atomicAdd(&g_stamps[6], 1ull);
    }
    const int cbase = n0 + wn * 64 + fq * 16;
    float bv[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) bv[j] = a.bias[cbase + j];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const int y = y0 + wm * 4 + mi, x = x0 + fr;
        if (y >= H || x >= W) continue;
        const long pix = ((long)b * H + y) * W + x;
        float v[16];
        bias_act16(acc[0][mi], acc[1][mi], acc[2][mi], acc[3][mi], bv, a.act != 0, v);
        store_px(reinterpret_cast<f16*>(a.out), pix * a.out_ct + a.out_coff + cbase, reinterpret_cast<const f16*>(a.res),
                 pix * a.res_ct + a.res_coff + cbase, cbase, a.Cout, v, LoadRes{});
    }
}

static hipError_t launch_halo2(const ConvArgs& a, hipStream_t s) {
    constexpr int NWI = (18 * 18 + 7) / 8, PROUNDS = (NWI + 7) / 8;
    const size_t lds = 2 * PROUNDS * 8 * 1024 + 2 * 2 * 128 * 128;
    const int blocks = a.B * ((a.Hi + 15) / 16) * ((a.Wi + 15) / 16) * ((pad64(a.Cout) + 127) / 128);
    return launch_lds<conv3x3_halo2_kernel>(dim3(blocks), dim3(512), lds, lds, s, a);
}

// ------------------------------------------------------------------------------------------------ 3x3 s1, 512 px x 128 ch
// The halo kernels above are not limited by matrix-pipe or LDS bandwidth but by the cost of getting bytes into LDS: every
// 1 KiB LDS-DMA piece holds its issuing wave for 60-180 cycles (MI355X_MICROARCH.md, "LDS-DMA piece issue cost"), and
// conv3x3_halo2_kernel needs 41 pieces per 64 MFMAs of every wave.  Weight bytes per flop only depend on the number of
// PIXELS a workgroup owns, so this variant doubles them: a 16 x 32-pixel patch (512 px) x 128 channels, each wave a
// 128 px x 64 ch tile (acc = 128 VGPRs).  To make that fit in LDS the K slab is 32 channels (LDS rows of 64 B):
//   halo 18 x 34 px x 64 B = 38.3 KiB (x2 buffers), weight stage = two taps x 128 rows x 64 B = 16 KiB (x3 ring)  -> 128 KiB
// One stage is again 64 MFMAs per wave but only ~25 DMA pieces and 24 instead of 32 fragment reads, and the ring is
// deep enough to request weights two stages ahead (counted vmcnt; halo pieces stay in flight for 2-3 stages).
// 64-byte rows: chunk' = chunk ^ 2*((row>>2)&1) is conflict-free for the ds_read_b128 lane groups at any row offset.
// Weights come from the second packed copy with 64-byte K chunks (ConvArgs::wgt32).
// WN = 1: the 64-channel variant (BN = 64): eight waves of 64 px x 64 ch (two image rows each), one DMA piece of weights
// per wave and stage, 32 MFMAs per wave between barriers.
// DUAL = true: maps at most 16 pixels wide (the stride-32 level of a 512-px tile): the 32 patch columns are the 16 columns of
// TWO consecutive images, each with its own left/right halo column (patch rows of 36 instead of 34 pixels).
template <bool TAIL, int WN, bool DUAL = false, int TPS = 2, bool SPLIT = false>
__global__ __launch_bounds__(512) void conv3x3_wide_kernel(const ConvArgs a) {
    // TAIL and TPS are single-valued; they keep their places because the profile summaries read WN, DUAL and SPLIT by position
    static_assert(TAIL && TPS == 2, "the last 16 MFMAs of a stage run behind its barrier; two taps per stage");
    // SPLIT (fp16x3 context): three passes over the input channels -- halo slabs of [x_lo | x_hi | x_hi] against the weight
    // slabs [w_hi | w_lo | w_hi] of the packed copy, i.e. the same stage loop over 3x the slab pairs; scaled / split epilogue
    // TPS = taps per stage (between two barriers)
    constexpr int NST = 18 / TPS;
    constexpr int TH = 16, TW = 32, NW = 8, BN = 64 * WN, PWID = DUAL ? 36 : TW + 2, HALF = DUAL ? 18 : 16;
    constexpr int RPW = TH / (NW / WN), MIW = 2 * RPW, WPS = WN == 2 ? TPS : 1;   // image rows / pixel fragments per wave; weight pieces per wave and stage
    constexpr int PR = (TH + 2) * PWID, NPC = (PR + 15) / 16, PROUNDS = (NPC + NW - 1) / NW;
    constexpr int P_BYTES = PROUNDS * NW * 1024, SLAB = BN * 64, W_BYTES = TPS * SLAB, RING = 3;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const Pbuf = smem;
    char* const Wbuf = smem + 2 * P_BYTES;
    typedef __attribute__((address_space(3))) void lds_void;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = WN == 2 ? wave >> 1 : wave, wn = WN == 2 ? wave & 1 : 0;
    const int H = a.Hi, W = a.Wi;
    const int tiles_x = DUAL ? 1 : (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const int cpad = pad128(a.Cout);                      // packed weight rows (zero rows past Cout)
    const int ntn = (pad64(a.Cout) + BN - 1) / BN;
    const int id = xcd_remap(blockIdx.x, gridDim.x);
    const int nt = id % ntn;
    int rest = id / ntn;
    const int tx = rest % tiles_x; rest /= tiles_x;
    const int ty = rest % tiles_y;
    const int b = rest / tiles_y;
    const int y0 = ty * TH, x0 = tx * TW, n0 = nt * BN;
    const int ppairs = a.Cin / 64;                          // pairs of 32-channel slabs in one pass over the input channels
    const int pairs = SPLIT ? a.split * ppairs : ppairs;     // a.split = passes of the fp16x3 context (3, or 2 for fp16-exact weights)
    const bool stamps = CY_STAMPS_ENABLED && (a.dbg & 64) != 0;      // diagnostic builds: phase stamps of the workgroup
    const unsigned long long t_entry = stamps ? stamp_real() : 0;

    const auto rs0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.in0), 0, a.in0_bytes, 0x00020000);
    const auto rsw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wgt32), 0, a.wgt32_bytes, 0x00020000);
    unsigned poff[PROUNDS];
#pragma unroll
    for (int j = 0; j < PROUNDS; ++j) {
        const int r = (j * NW + wave) * 16 + (lane >> 2);
        const int ry = r / PWID, rx = r - ry * PWID;
        const int half = DUAL ? rx / 18 : 0;                 // DUAL: which of the block's two images this patch column belongs to
        const int bb = DUAL ? 2 * b + half : b;
        const int y = y0 + ry - 1, x = DUAL ? rx - half * 18 - 1 : x0 + rx - 1;
        const int q = (lane & 3) ^ (((r >> 2) & 1) << 1);
        const bool ok = r < PR && bb < a.B && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        poff[j] = ok ? (unsigned)(((bb * H + y) * W + x) * a.in0_ct + a.in0_coff + q * 8) * 2u : CY_OOB;
    }
    unsigned woff;
    {   // WN = 2: every wave moves rows wave*16.. of BOTH taps of a stage; WN = 1: wave -> (tap wave>>2, rows (wave&3)*16..)
        const int row = (WN == 2 ? wave : (wave & 3)) * 16 + (lane >> 2);
        woff = (unsigned)((n0 + row) * 64 + ((lane & 3) ^ (((row >> 2) & 1) << 1)) * 16);
    }
    auto dma_patch = [&](int buf, int slab) {               // slab: 32-channel slab index
        unsigned so = (unsigned)slab * 64u;
        if constexpr (SPLIT) {                               // virtual slab -> physical slab (+ the offset of the low halves in the first pass)
            int lo;
            so = (unsigned)x3_chunk(slab, 2 * ppairs, lo) * 64u;
            if (lo) so += (unsigned)a.in0_lo * 2u;
        }
#pragma unroll
        for (int j = 0; j < PROUNDS; ++j)                    // uniform part in soffset: not range-checked, so the OOB sentinel of
            dma_piece(rs0, (lds_ptr_t*)(Pbuf + buf * P_BYTES + (j * NW + wave) * 1024), poff[j], so);   // a lane survives it
    };
    auto dma_stage = [&](int ring, int slab0, int u0) {     // taps u0 .. u0+TPS-1 of the pair starting at slab slab0 (u in 0..17)
        if constexpr (WN == 2) {
#pragma unroll
            for (int t = 0; t < TPS; ++t) {
                const int u = u0 + t, sl = slab0 + u / 9, tap = u % 9;
                dma_piece(rsw, (lds_ptr_t*)(Wbuf + ring * W_BYTES + t * SLAB + wave * 1024), woff, (sl * 9 + tap) * cpad * 64);
            }
        } else {
            const int t = wave >> 2, u = u0 + t, sl = slab0 + u / 9, tap = u % 9;
            dma_piece(rsw, (lds_ptr_t*)(Wbuf + ring * W_BYTES + t * SLAB + (wave & 3) * 1024), woff, (sl * 9 + tap) * cpad * 64);
        }
    };
    f32x4 acc[4][MIW];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int mi = 0; mi < MIW; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fq = lane >> 4;
    // Fragment addresses = per-lane base + compile-time offset.  A halo row is r = wm*4*PWID + base + fr with `base`
    // known at compile time per (tap, mi) and wm*4*PWID = 0 mod 8, so the swizzle bit ((r>>2)&1) only depends on
    // base & 7 and the lane: eight lane bases cover every tap.  Weight rows are 0 mod 16 + fr: one lane base.
    unsigned pb[8];
    const int rw0 = wm * RPW * PWID;                         // first halo row of this wave's pixels (0 mod 8 for WN = 2, 0 or 4 for WN = 1)
#pragma unroll
    for (int c = 0; c < 8; ++c)
        pb[c] = (unsigned)(rw0 * 64 + fr * 64 + ((fq ^ ((((c + fr + (rw0 & 7)) >> 2) & 1) << 1)) << 4));
    const unsigned wl = (unsigned)(2 * P_BYTES + (wn * 64 + fr) * 64 + ((fq ^ (((fr >> 2) & 1) << 1)) << 4));
    // One stage = two taps = four half-steps of 16 MFMAs (4 channel blocks x 4 pixel fragments).  The fragment reads of
    // half-step h+1 are issued before the MFMAs of half-step h (register double buffer), and a scheduling fence after
    // each half-step keeps the compiler from hoisting more than that (the kernel sits at the 256-VGPR limit: 128 acc).
    f16x8 xa[2][4], wb[2][4];
    auto load_x = [&](f16x8* dst, int pbuf_off, int kh, int kw, int half) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int mi = half * 4 + m;
            const int base = ((mi >> 1) + kh) * PWID + (mi & 1) * HALF + kw;
            dst[m] = *reinterpret_cast<const f16x8*>(smem + pb[base & 7] + (pbuf_off + base * 64));
        }
    };
    auto load_w = [&](f16x8* dst, int wbuf_off) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) dst[ni] = *reinterpret_cast<const f16x8*>(smem + wl + (wbuf_off + ni * 1024));
    };
    auto mma = [&](const f16x8* w, const f16x8* x, int half) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int m = 0; m < 4; ++m)
                acc[ni][half * 4 + m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[ni], x[m], acc[ni][half * 4 + m], 0, 0, 0);
    };
    auto stage_compute = [&](int st) {                       // taps u = TPS*st .. of the current slab pair
        const int u0 = TPS * st, u1 = u0 + 1, t0 = u0 % 9, t1 = u1 % 9;
        const int p0 = (u0 / 9) * P_BYTES, p1 = (u1 / 9) * P_BYTES, w0 = (st % 3) * W_BYTES, w1 = w0 + SLAB;
        if constexpr (WN == 2) {
            load_w(wb[0], w0);
            load_x(xa[0], p0, t0 / 3, t0 % 3, 0);
            load_x(xa[1], p0, t0 / 3, t0 % 3, 1);
            mma(wb[0], xa[0], 0);
            __builtin_amdgcn_sched_barrier(0);
            load_w(wb[1], w1);
            load_x(xa[0], p1, t1 / 3, t1 % 3, 0);
            mma(wb[0], xa[1], 1);
            __builtin_amdgcn_sched_barrier(0);
            load_x(xa[1], p1, t1 / 3, t1 % 3, 1);
            mma(wb[1], xa[0], 0);
            __builtin_amdgcn_sched_barrier(0);              // the last 16 MFMAs are issued behind the stage barrier
        } else {                                             // one half-step (4 fragments = this wave's 64 pixels) per tap
            load_w(wb[0], w0);
            load_x(xa[0], p0, t0 / 3, t0 % 3, 0);
            load_w(wb[1], w1);
            load_x(xa[1], p1, t1 / 3, t1 % 3, 0);
            mma(wb[0], xa[0], 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // Workgroup time over the layers of the benchmark: ~12 us + 1.35 us per stage (18 / 36 / 72 stages: 36 / 60 / 110 us), i.e. a third of
    // an 18-stage workgroup is launch + prologue round trip + epilogue (128 SiLUs per lane at 26 issue cycles each, two waves per
    // SIMD) + stores.  Starting the first round of workgroups in 2 / 4 / 8 phases a fraction of a workgroup apart (so that the CUs'
    // read and write bursts stop coinciding) only added the idle time it cost: +4.4 / +6.4 / +6.6 % on the forward pass.
    // Phase records of a stamped build (tools/stamp_wide.py, 256 tiles): 18-stage workgroups (Cin 128, 64x64 maps) spend 3.7 us before
    // the loop, 24.9 us in it (1.39 us per stage), 3.2 us issuing the epilogue (6.9 us with a residual input) and 0.7 us draining
    // stores = 32.6 us of a 36.2 us slot (the rest is the hand-over between workgroups); 36-stage ones 2.3 + 49.5 + 3.2 + 0.7 of 60.
    // A PERSISTENT form was tried a second time with those figures in hand (one workgroup per CU walking patches, the next patch's
    // bias / halo / first two weight stages requested right behind the last stage barrier so that they land under the epilogue,
    // residual vectors as a ring of four fragments to stay inside 256 VGPRs): 28.9-29.0 ms forward against 28.0, every layer
    // slower (residual layers +14 %).  The hardware's own hand-over between one-patch workgroups is the better pipeline here.
    // A STAGGERED form was tried as well (MI355X_MICROARCH.md "Two waves per SIMD" item 9: waves 4-7 half a stage behind waves 0-3 --
    // between two barriers 16 + 48 MFMAs of two stages for the first group, 32 + 32 for the second; four-slot weight ring addressed
    // at run time, odd halo slab requested a stage later; one stage loop per group, else the two streams cost 580 B of scratch;
    // bit-identical outputs): 29.10 vs 28.79-28.98 ms forward on the same box, 18-stage layers 5 % slower, 36- and 72-stage layers
    // unchanged.  Nor does it matter WHEN the second wave of a SIMD issues its requests (round 3: waves 4-7 issuing theirs in mid-stage,
    // behind their first 32 MFMAs, so that the two waves of a SIMD never wait at the memory pipeline together: every wide layer within
    // +-0.5 % at batch 256).  So the 1.39 us per stage is not a lock-step effect either.  It is the clock: s_memtime / s_memrealtime over the loop
    // give 1.76 GHz for 18-, 36- and 72-stage layers, at which a stage's 2 x 64 MFMAs per SIMD (2048 cycles) would take 1.16 us:
    // the loop runs at 84 % of the matrix-core rate at the clock the chip holds under this load.
    // (tried in round 2, not kept: s_setprio 1 for waves 4-7 before the loop -- static priority for the second-dispatched half,
    // MI355X_MICROARCH.md "Two waves per SIMD" item 4: 8026 vs 8048 tiles/s on the S16k benchmark; and a PERSISTENT form, one
    // workgroup per CU walking the patches with the next patch's halo / first weight stages requested behind the last stage
    // barrier so that their round trip runs under the epilogue: 7807 vs 7851 tiles/s with the same restructured body, which
    // itself cost 2.5 % through spills at the 256-VGPR limit -- the exposed prologue is not where the time goes)
    // the workgroup's BN bias values go to LDS with the very first request (wave 0; it is the oldest of that wave's requests,
    // so every counted wait below covers it): the epilogue then reads them in ~100 cycles instead of paying an exposed L2
    // round trip per workgroup (one workgroup per CU: nothing else would hide it)
    float* const bias_lds = reinterpret_cast<float*>(smem + 2 * P_BYTES + RING * W_BYTES);
    if (wave == 0) {
        const auto rsb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.bias), 0, (unsigned)pad64(a.Cout) * 4u, 0x00020000);
        dma_piece(rsb, (lds_ptr_t*)bias_lds, lane * 16 < BN * 4 ? (unsigned)(n0 * 4 + lane * 16) : CY_OOB, 0);
    }
    // prologue: halo of slab 0, weight stages 0 and 1
    dma_patch(0, 0);
    dma_stage(0, 0, 0);
    dma_stage(1, 0, TPS);
    CY_WAIT_VM(WPS);
    __builtin_amdgcn_s_barrier();
    const unsigned long long t_loop = stamps ? stamp_real() : 0, c_loop = stamps ? stamp_now() : 0;
#pragma unroll 1
    for (int cp = 0; cp < pairs; ++cp) {
        const bool more = cp + 1 < pairs;
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            // stage g = NST*cp + st uses ring slot st % 3; request the weights of stage g+2 and the halo buffers just freed
            const bool has_w = st + 2 < NST || more;
            if (st + 2 < NST) dma_stage((st + 2) % 3, 2 * cp, TPS * (st + 2));
            else if (more) dma_stage((st + 2) % 3, 2 * cp + 2, TPS * (st + 2 - NST));
            // halo: odd slab of this pair (first read in stage NST/2, rounded up) and even slab of the next pair (its buffer
            // is free once the stage holding tap 8 is done)
            if (st == 0) dma_patch(1, 2 * cp + 1);
            if (st == 5 && more) dma_patch(0, 2 * cp + 2);
            stage_compute(st);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            // the weights of stage g+1 (requested first thing in stage g-1) must have landed; younger requests may fly on
            if (st == 0 || st == 1) { CY_WAIT_VM(WPS + PROUNDS); }
            else if (st == 5 || st == 6) { if (more) { CY_WAIT_VM(WPS + PROUNDS); } else { CY_WAIT_VM(WPS); } }
            else if (has_w) { CY_WAIT_VM(WPS); }
            else { CY_WAIT_VM(0); }
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            mma(wb[1], xa[1], WN == 2 ? 1 : 0);    // operands are in registers: overlaps the next stage's DMA issue / first reads
        }
    }

    const unsigned long long t_epi = stamps ? stamp_real() : 0, c_epi = stamps ? stamp_now() : 0;
    const int cbase = n0 + wn * 64 + fq * 16;
    if constexpr (SPLIT) {
        // fp16x3 epilogue: acc * oscale + bias, SiLU, residual = its high + low halves (requested two pixel fragments at a
        // time: the accumulators leave no room for more), result stored as high / low halves
        float bv[16], sc[16];
        load16(bias_lds + wn * 64 + fq * 16, bv);
#pragma unroll
        for (int j = 0; j < 16; ++j) sc[j] = a.oscale[cbase + j];
        const bool vec = cbase + 16 <= a.Cout;
        const bool res_vec = a.res != nullptr && vec;
        const auto rsr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.res ? a.res : a.out), 0,
                                                           a.res ? (unsigned)((long)a.B * H * W * a.res_ct * 2) : 0u, 0x00020000);
#pragma unroll
        for (int g4 = 0; g4 < MIW; g4 += 2) {
            f16x8 rv[2][4];
            if (res_vec) {
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const int mi = g4 + m;
                    const int y = y0 + wm * RPW + (mi >> 1), x = DUAL ? fr : x0 + (mi & 1) * 16 + fr;
                    const int bb = DUAL ? 2 * b + (mi & 1) : b;
                    const bool ok = y < H && x < W && bb < a.B;
                    const unsigned ro = ok ? (unsigned)((((bb * H + y) * W + x) * a.res_ct + a.res_coff + cbase) * 2) : CY_OOB;
                    rv[m][0] = __builtin_bit_cast(f16x8, load_b128(rsr, ro, 0));
                    rv[m][1] = __builtin_bit_cast(f16x8, load_b128(rsr, ro, 16));
                    rv[m][2] = __builtin_bit_cast(f16x8, load_b128(rsr, ro, a.res_lo * 2));
                    rv[m][3] = __builtin_bit_cast(f16x8, load_b128(rsr, ro, a.res_lo * 2 + 16));
                }
            }
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int mi = g4 + m;
                const int y = y0 + wm * RPW + (mi >> 1), x = DUAL ? fr : x0 + (mi & 1) * 16 + fr;
                const int bb = DUAL ? 2 * b + (mi & 1) : b;
                if (y >= H || x >= W || bb >= a.B) continue;
                const long pix = ((long)bb * H + y) * W + x;
                float v[16];
                scale_bias_act16(acc[0][mi], acc[1][mi], acc[2][mi], acc[3][mi], bv, sc, a.act != 0, v);
                store_px_split(reinterpret_cast<f16*>(a.out), pix * a.out_ct + a.out_coff + cbase, a.out_lo, reinterpret_cast<const f16*>(a.res),
                               pix * a.res_ct + a.res_coff + cbase, a.res_lo, cbase, a.Cout, v, rv[m]);
            }
        }
    } else {
    // Residual (bottleneck shortcut): all of this wave's 2*MIW vectors are requested up front (the fragment registers are
    // free now), so the epilogue pays ONE memory round trip instead of one per pixel fragment (1 workgroup per CU: nothing
    // else hides it).  Out-of-range pixels read the zero of the buffer range check.
    const bool res_vec = a.res != nullptr && cbase + 16 <= a.Cout;
    f16x8 rv[MIW][2];
    if (res_vec) {
        const auto rsr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.res), 0, (unsigned)((long)a.B * H * W * a.res_ct * 2), 0x00020000);
#pragma unroll
        for (int mi = 0; mi < MIW; ++mi) {
            const int y = y0 + wm * RPW + (mi >> 1), x = DUAL ? fr : x0 + (mi & 1) * 16 + fr;
            const int bb = DUAL ? 2 * b + (mi & 1) : b;
            const bool ok = y < H && x < W && bb < a.B;
            const unsigned ro = ok ? (unsigned)((((bb * H + y) * W + x) * a.res_ct + a.res_coff + cbase) * 2) : CY_OOB;
            rv[mi][0] = __builtin_bit_cast(f16x8, load_b128(rsr, ro, 0));
            rv[mi][1] = __builtin_bit_cast(f16x8, load_b128(rsr, ro, 16));
        }
    }
    float bv[16];
    load16(bias_lds + wn * 64 + fq * 16, bv);
#pragma unroll
    for (int mi = 0; mi < MIW; ++mi) {
        const int y = y0 + wm * RPW + (mi >> 1), x = DUAL ? fr : x0 + (mi & 1) * 16 + fr;
        const int bb = DUAL ? 2 * b + (mi & 1) : b;
        if (y >= H || x >= W || bb >= a.B) continue;
        const long pix = ((long)bb * H + y) * W + x;
        float v[16];
        bias_act16(acc[0][mi], acc[1][mi], acc[2][mi], acc[3][mi], bv, a.act != 0, v);
        store_px(reinterpret_cast<f16*>(a.out), pix * a.out_ct + a.out_coff + cbase, reinterpret_cast<const f16*>(a.res),
                 pix * a.res_ct + a.res_coff + cbase, cbase, a.Cout, v, rv[mi]);
    }
    }
    // diagnostic builds: one record per workgroup (wave 0, plain stores; units of 10 ns): [0] entry -> loop (address setup, prologue
    // round trip), [1] stage loop, [2] epilogue issue, [3] the stage loop again in s_memtime ticks (clock = [3] / [1]).  (Summing with atomics from 16k waves stretched the
    // kernel 4x and the epilogue figures with it.)
    if (stamps) {
        const unsigned long long t_st = stamp_real();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long t_end = stamp_real();
        if (tid == 0) {
            unsigned long long* rec = g_wg_stamps + (size_t)(blockIdx.x % WG_STAMP_SLOTS) * 4;
            rec[0] = t_loop - t_entry; rec[1] = t_epi - t_loop; rec[2] = t_st - t_epi; rec[3] = c_epi - c_loop;   // [3]: the loop in s_memtime ticks
        }
    }
}

template <int WN, bool DUAL = false, bool SPLIT = false>
static hipError_t launch_wide(const ConvArgs& a, hipStream_t s) {
    constexpr int PR = 18 * (DUAL ? 36 : 34), NPC = (PR + 15) / 16, PROUNDS = (NPC + 7) / 8, BN = 64 * WN;
    const size_t lds = 2 * PROUNDS * 8 * 1024 + 3 * 2 * BN * 64 + 1024;       // halo x2, weight ring, bias
    const int bx = DUAL ? (a.B + 1) / 2 : a.B * ((a.Wi + 31) / 32);
    const int blocks = bx * ((a.Hi + 15) / 16) * ((pad64(a.Cout) + BN - 1) / BN);
    return launch_lds<conv3x3_wide_kernel<true, WN, DUAL, 2, SPLIT>>(dim3(blocks), dim3(512), lds, lds, s, a);
}

// ------------------------------------------------------------------------------------------------ 3x3 s1, 512 px x 128 ch, persistent
// conv3x3_wide_kernel<true, 2> as ONE workgroup per CU walking the patches (patch n of a workgroup = blockIdx.x + n * gridDim.x
// in the same XCD-aware order).  What a one-patch workgroup pays outside its stage loop -- per-workgroup records of the stamped
// build: 2.3-3.7 us from entry to the first MFMA (the 70 KiB prologue arrives at the ~11 B/cycle a CU gets when every CU asks at
// once), 3.2-6.9 us of epilogue, 0.7 us of store drain and 3.6-4.3 us until the next workgroup runs on the CU -- is a third of an
// 18-stage (Cin = 128) patch.  Here the NEXT patch's prologue (bias, first halo slab, first two weight stages) is requested right
// behind the last stage barrier and lands under the epilogue of the current patch, and there is no hand-over.
// Two earlier persistent forms lost to the one-patch kernel (+3 %, residual layers +14 %).  The vector-memory counter is in-order:
// a residual load issued after the next patch's 70 KiB of LDS-DMA cannot be waited for without waiting for all of that DMA, so
// the epilogue stood still for the whole prologue.  Here the order of requests is  bias(next) -> residual(this) -> halo / weights
// (next)  and the epilogue waits with a counted vmcnt that leaves exactly the DMA in flight; the output stores are buffer stores
// issued by every lane (out-of-range lanes carry the out-of-range offset and are dropped by the range check), so the number of
// operations between the DMA and the next patch's first wait is a compile-time constant too.
// STRIP form (STRIP = halo pieces per requesting wave and slab: 10 for maps up to 62 px wide, 12 up to 95): a workgroup owns 512
// consecutive ENTRIES of the batch flattened to one dimension -- image after image, row after row, with ONE zero entry after each
// row and one zero row after each image (row stride RS = W + 1, image stride IS = (H + 1) * RS).  Zero padding of a 3x3 filter is
// then just those shared zero entries: tap (kh, kw) of entry e is entry e + (kh - 1) * RS + (kw - 1) for EVERY entry, so any 16
// consecutive entries are an MFMA pixel fragment and a map of any size is covered with (RS / W) * ((H + 1) / H) - 1 idle lanes
// (80 x 80: 2.5 %, 40 x 40: 5 %, 20 x 20: 10 %, 52 x 64 of a ragged tile: 3.5 %) instead of the 17-61 % that 16 x 32-pixel patches
// waste on 80 / 40 / 20-px maps.  Price: a halo of RS + 1 entries on both sides (676 staged entries for 80-px rows against 612).
struct StripGeo { int RS, IS, NE; unsigned long long mRS, mIS; };      // NE = B * IS entries; m* = ceil(2^40 / divisor)
__device__ __forceinline__ int strip_div(int e, unsigned long long m) { return (int)(((unsigned long long)(unsigned)e * m) >> 40); }

template <bool SPLIT, bool RES, int STRIP = 0>
__global__ __launch_bounds__(512) void conv3x3_widep_kernel(const ConvArgs a, const int total, const StripGeo sg) {
    // SPLIT (fp16x3 context): three passes over the halo slabs [x_lo | x_hi | x_hi] against the packed weight slabs [w_hi | w_lo | w_hi]
    // (see conv3x3_wide_kernel); epilogue acc * oscale + bias, SiLU, + residual (hi + lo), stored as high / low halves
    constexpr int NST = 9, TH = 16, TW = 32, NW = 8, BN = 128, PWID = TW + 2;
    // Only waves 0-3 (one per SIMD) issue LDS-DMA.  A wave whose request does not fit the memory pipeline waits at the issue, and
    // cannot issue MFMAs meanwhile; with every wave issuing its share at the same point of a stage both waves of a SIMD wait
    // together and the matrix pipe idles (a slab pair WITH its requests takes 13.3-15.6 us, the last pair of a patch, which has
    // none left to issue, 9 us).  With the requests on one wave per SIMD its partner (waves 4-7) has the pipe meanwhile.
    constexpr int NDW = 4;                                   // requesting waves
    constexpr int RPW = 4, MIW = 8, WPS = 2 * (NW / NDW);    // weight pieces per requesting wave and stage
    constexpr int PR = (TH + 2) * PWID, NPC = (PR + 15) / 16, PROUNDS = STRIP ? STRIP : (NPC + NDW - 1) / NDW;      // halo pieces per requesting wave and slab
    constexpr int P_BYTES = PROUNDS * NDW * 1024, SLAB = BN * 64, W_BYTES = 2 * SLAB, RING = 3;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const Pbuf = smem;
    char* const Wbuf = smem + 2 * P_BYTES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int H = a.Hi, W = a.Wi;
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const int cpad = pad128(a.Cout);
    const int ntn = (pad64(a.Cout) + BN - 1) / BN;
    const int ppairs = a.Cin / 64;                          // slab pairs of one pass over the input channels
    const int pairs = SPLIT ? a.split * ppairs : ppairs;     // a.split = passes of the fp16x3 context (3, or 2 for fp16-exact weights)
    const auto rs0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.in0), 0, a.in0_bytes, 0x00020000);
    const auto rsw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wgt32), 0, a.wgt32_bytes, 0x00020000);
    const auto rsb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.bias), 0, (unsigned)pad64(a.Cout) * 4u, 0x00020000);
    const auto rss = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(SPLIT ? a.oscale : a.bias), 0, (unsigned)pad64(a.Cout) * 4u, 0x00020000);
    const unsigned out_bytes = (unsigned)((long)a.B * H * W * a.out_ct * 2);
    const auto rso = __builtin_amdgcn_make_buffer_rsrc(a.out, 0, out_bytes, 0x00020000);
    const auto rsr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(RES ? a.res : a.in0), 0,
                                                       RES ? (unsigned)((long)a.B * H * W * a.res_ct * 2) : 0u, 0x00020000);
    const int fr = lane & 15, fq = lane >> 4;

    // patch v -> (image, first row / column, first channel)
    int pb_, py0, px0, pn0;
    auto geometry = [&](int v) {
        const int id = xcd_remap(v, total);
        pn0 = (id % ntn) * BN;
        int rest = id / ntn;
        if constexpr (STRIP != 0) { px0 = rest * 512; py0 = 0; pb_ = 0; return; }       // px0 = first entry of the strip
        px0 = (rest % tiles_x) * TW; rest /= tiles_x;
        py0 = (rest % tiles_y) * TH;
        pb_ = rest / tiles_y;
    };
    // developer ablation (diagnostic builds; results invalid): bit 0 no requests inside the stage loop, bit 1 no fragment reads, bit 2 no MFMAs
    const bool no_dma = CY_STAMPS_ENABLED && (a.dbg & 1), no_rd = CY_STAMPS_ENABLED && (a.dbg & 2), no_mma = CY_STAMPS_ENABLED && (a.dbg & 4);
    const bool dmaw = wave < NDW && !no_dma;
    // halo piece j of a requesting wave: entries (j * NDW + wave) * 16 + (lane >> 2) of the 18 x 34 halo; the offsets are computed at
    // the request (a dozen VALU instructions of a wave that is about to wait for the memory pipeline anyway) instead of living in
    // ten registers next to the 128 accumulators
    auto dma_patch = [&](int buf, int slab, int gb, int gy0, int gx0) {
        if (!dmaw) return;
        int l4 = lane >> 2;
        asm volatile("" : "+v"(l4));                         // (keeps the optimiser from hoisting the ten offsets out of the stage loop)
        const unsigned lq = (unsigned)(lane & 3);
        unsigned slab_so = (unsigned)slab * 64u;             // fp16x3: virtual slab -> physical slab (+ the low halves in the first pass)
        if constexpr (SPLIT) {
            int lo;
            slab_so = (unsigned)x3_chunk(slab, 2 * ppairs, lo) * 64u;
            if (lo) slab_so += (unsigned)a.in0_lo * 2u;
        }
        if constexpr (STRIP != 0) {
            // staged entry le of the strip = entry gx0 - RS - 1 + le of the flattened batch -> (image, row, column) or a zero
            const int hl = 514 + 2 * sg.RS;
#pragma unroll
            for (int j = 0; j < PROUNDS; ++j) {
                const int le = (j * NDW + wave) * 16 + l4;
                const int e = gx0 - sg.RS - 1 + le;
                const bool in = le < hl && (unsigned)e < (unsigned)sg.NE;
                const int ec = in ? e : 0;
                const int bb = strip_div(ec, sg.mIS), r = ec - bb * sg.IS;
                const int y = strip_div(r, sg.mRS), x = r - y * sg.RS;
                const unsigned q = lq ^ (unsigned)(((le >> 2) & 1) << 1);
                const bool ok = in && y < H && x < W;
                const unsigned off = ok ? (unsigned)(((bb * H + y) * W + x) * a.in0_ct + a.in0_coff + (int)q * 8) * 2u : CY_OOB;
                dma_piece(rs0, (lds_ptr_t*)(Pbuf + buf * P_BYTES + (j * NDW + wave) * 1024), off, slab_so);
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < PROUNDS; ++j) {
            const int r = (j * NDW + wave) * 16 + l4;
            const int ry = (r * 1928) >> 16, rx = r - ry * PWID;       // r / 34 for r < 1024
            const int y = gy0 + ry - 1, x = gx0 + rx - 1;
            const unsigned q = lq ^ (unsigned)(((r >> 2) & 1) << 1);
            const bool ok = r < PR && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
            const unsigned off = ok ? (unsigned)(((gb * H + y) * W + x) * a.in0_ct + a.in0_coff + (int)q * 8) * 2u : CY_OOB;
            dma_piece(rs0, (lds_ptr_t*)(Pbuf + buf * P_BYTES + (j * NDW + wave) * 1024), off, slab_so);
        }
    };
    // (lane-dependent LDS / weight addresses are recomputed at the top of every patch instead of living through the epilogue,
    // where the 128 accumulators + 64 residual registers leave no room for them)
    unsigned woff = 0;
    auto weight_lane_offset = [&]() { const int row = wave * 32 + (lane >> 2); woff = (unsigned)(row * 64 + ((lane & 3) ^ (((row >> 2) & 1) << 1)) * 16); };
    auto dma_stage = [&](int ring, int slab0, int u0, int n0) {      // requesting wave w: rows w*32 .. w*32+31 of both taps
        if (!dmaw) return;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int u = u0 + t, sl = slab0 + u / 9, tap = u % 9;
#pragma unroll
            for (int h = 0; h < 2; ++h)
                dma_piece(rsw, (lds_ptr_t*)(Wbuf + ring * W_BYTES + t * SLAB + (wave * 2 + h) * 1024), woff,
                          (unsigned)((sl * 9 + tap) * cpad * 64 + n0 * 64 + h * 1024));
        }
    };
    // two slots of 2 KiB, alternating per patch: [bias 512 B | 512 B written with zeros | oscale 512 B (fp16x3) | zeros]
    float* const bias_lds = reinterpret_cast<float*>(smem + 2 * P_BYTES + RING * W_BYTES);
    auto dma_bias = [&](int slot, int n0) {
        if (wave != 0) return;
        dma_piece(rsb, (lds_ptr_t*)(bias_lds + slot * 512), lane * 16 < BN * 4 ? (unsigned)(n0 * 4 + lane * 16) : CY_OOB, 0);
        if constexpr (SPLIT) dma_piece(rss, (lds_ptr_t*)(bias_lds + slot * 512 + 256), lane * 16 < BN * 4 ? (unsigned)(n0 * 4 + lane * 16) : CY_OOB, 0);
    };

    f32x4 acc[4][MIW];
    unsigned pb[STRIP ? 9 : 8], wl = 0;
    const int rw0 = wm * RPW * PWID;
    auto fragment_bases = [&]() {
        // opaque to the optimiser: otherwise it hoists these 9 registers out of the patch loop and spills around the epilogue
        int lz = lane;
        asm volatile("" : "+v"(lz));
        const int r_ = lz & 15, q_ = lz >> 4;
        if constexpr (STRIP != 0) {
            // strip form: one lane base per TAP -- staged row of (tap, fragment 0) = kh * RS + kw + wm * 128 + fr; fragment m is 16 m rows
            // (1 KiB, same swizzle phase) further on
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int R0 = (t / 3) * sg.RS + (t % 3) + wm * 128 + r_;
                pb[t] = (unsigned)(R0 * 64 + ((q_ ^ (((R0 >> 2) & 1) << 1)) << 4));
            }
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c)
                pb[c] = (unsigned)(rw0 * 64 + r_ * 64 + ((q_ ^ ((((c + r_ + (rw0 & 7)) >> 2) & 1) << 1)) << 4));
        }
        wl = (unsigned)(2 * P_BYTES + (wn * 64 + r_) * 64 + ((q_ ^ (((r_ >> 2) & 1) << 1)) << 4));
    };
    f16x8 xa[2][4], wb[2][4];
    auto load_x = [&](f16x8* dst, int pbuf_off, int kh, int kw, int half) {
        if (no_rd) return;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int mi = half * 4 + m;
            if constexpr (STRIP != 0) {
                dst[m] = *reinterpret_cast<const f16x8*>(smem + pb[kh * 3 + kw] + (pbuf_off + mi * 1024));
            } else {
                const int base = ((mi >> 1) + kh) * PWID + (mi & 1) * 16 + kw;
                dst[m] = *reinterpret_cast<const f16x8*>(smem + pb[base & 7] + (pbuf_off + base * 64));
            }
        }
    };
    auto load_w = [&](f16x8* dst, int wbuf_off) {
        if (no_rd) return;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) dst[ni] = *reinterpret_cast<const f16x8*>(smem + wl + (wbuf_off + ni * 1024));
    };
    auto mma = [&](const f16x8* w, const f16x8* x, int half) {
        if (no_mma) return;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int m = 0; m < 4; ++m)
                acc[ni][half * 4 + m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[ni], x[m], acc[ni][half * 4 + m], 0, 0, 0);
    };
    auto stage_compute = [&](int st) {
        const int u0 = 2 * st, u1 = u0 + 1, t0 = u0 % 9, t1 = u1 % 9;
        const int p0 = (u0 / 9) * P_BYTES, p1 = (u1 / 9) * P_BYTES, w0 = (st % 3) * W_BYTES, w1 = w0 + SLAB;
        load_w(wb[0], w0);
        load_x(xa[0], p0, t0 / 3, t0 % 3, 0);
        load_x(xa[1], p0, t0 / 3, t0 % 3, 1);
        mma(wb[0], xa[0], 0);
        __builtin_amdgcn_sched_barrier(0);
        load_w(wb[1], w1);
        load_x(xa[0], p1, t1 / 3, t1 % 3, 0);
        mma(wb[0], xa[1], 1);
        __builtin_amdgcn_sched_barrier(0);
        load_x(xa[1], p1, t1 / 3, t1 % 3, 1);
        mma(wb[1], xa[0], 0);
        __builtin_amdgcn_sched_barrier(0);                  // the last 16 MFMAs of the stage are issued behind the stage barrier
    };

    const bool stamps = CY_STAMPS_ENABLED && (a.dbg & 64) != 0;      // diagnostic builds: phase records of the workgroup's SECOND patch
    unsigned long long t_l0 = 0, t_l1 = 0, t_rw = 0, t_ep = 0;
    const unsigned long long t_begin = stamps ? stamp_real() : 0;
    // ---- first patch: prologue as in the one-patch kernel
    int v = blockIdx.x, n = 0;
    if (v >= total) return;
    geometry(v);
    weight_lane_offset();
    dma_bias(0, pn0);
    dma_patch(0, 0, pb_, py0, px0);
    dma_stage(0, 0, 0, pn0);
    dma_stage(1, 0, 2, pn0);
    CY_WAIT_VM(WPS);
    __builtin_amdgcn_s_barrier();
#pragma unroll 1
    for (;;) {
        const int b = pb_, y0 = py0, x0 = px0, n0 = pn0;
        const int vn = v + (int)gridDim.x;
        const bool next = vn < total;
        if (stamps) {
            const unsigned long long t = stamp_real();
            if (n == 2 && tid == 0) {                             // [0] requests + residual wait, [1] stage loop, [2] epilogue, [3] (unused)
                unsigned long long* rec = g_wg_stamps + (size_t)(blockIdx.x % WG_STAMP_SLOTS) * 4;
                rec[0] = t_rw - t_l1; rec[1] = t_l1 - t_l0; rec[2] = t_ep - t_rw;
            }
            t_l0 = t;
        }
        fragment_bases();
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int mi = 0; mi < MIW; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
        // The stream of stages never drains at a patch boundary: in the LAST slab pair of a patch the requests that would fetch
        // "the next pair" fetch the first halo slab and the first two weight stages of the NEXT patch instead, at the same steady
        // rate (a burst of the whole 70 KiB prologue holds the issuing waves for 3.3 us: the memory pipeline takes ~11 B per cycle
        // and CU, and a wave whose request does not fit waits).  The halo offsets of the next patch replace this patch's in the same
        // registers once its last halo request is out (stage 0 of the last pair).
#pragma unroll 1
        for (int cp = 0; cp < pairs; ++cp) {
            const bool more = cp + 1 < pairs;
            const bool chain = more || next;                     // something follows this pair
#pragma unroll
            for (int st = 0; st < NST; ++st) {
                const bool has_w = st + 2 < NST || chain;
                if (st + 2 < NST) dma_stage((st + 2) % 3, 2 * cp, 2 * (st + 2), n0);
                else if (more) dma_stage((st + 2) % 3, 2 * cp + 2, 2 * (st + 2 - NST), n0);
                else if (next) dma_stage((st + 2) % 3, 0, 2 * (st + 2 - NST), pn0);
                if (st == 0) dma_patch(1, 2 * cp + 1, b, y0, x0);
                if (st == 1 && !more && next) { geometry(vn); dma_bias((n + 1) & 1, pn0); }
                if (st == 5 && more) dma_patch(0, 2 * cp + 2, b, y0, x0);
                if (st == 5 && !more && next) dma_patch(0, 0, pb_, py0, px0);
                stage_compute(st);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (st == 0 || st == 1) { CY_WAIT_VM(WPS + PROUNDS); }
                else if (st == 5 || st == 6) { if (chain) { CY_WAIT_VM(WPS + PROUNDS); } else { CY_WAIT_VM(WPS); } }
                else if (has_w) { CY_WAIT_VM(WPS); }
                else { CY_WAIT_VM(0); }
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
                mma(wb[1], xa[1], 1);
            }
        }
        if (stamps) t_l1 = stamp_real();
        // ---- epilogue of this patch.  Stage 0 of the next patch needs nothing but what the last barrier has already published.
        const float* bl = bias_lds + (n & 1) * 512 + wn * 64 + fq * 16;
        float bv[16];
        if constexpr (!SPLIT) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(bl + j * 4);
                bv[j * 4] = t[0]; bv[j * 4 + 1] = t[1]; bv[j * 4 + 2] = t[2]; bv[j * 4 + 3] = t[3];
            }
        }
        const int cbase = n0 + wn * 64 + fq * 16;
        const bool chan_ok = cbase + 16 <= a.Cout;
        // pixel index of fragment mi of this lane = pix0 + (mi >> 1) * W + (mi & 1) * 16; rows past H are uniform per fragment pair
        const int xl = x0 + fr;
        const unsigned pix0 = (unsigned)((b * H + y0 + wm * RPW) * W + xl);
        const bool okx0 = xl < W && chan_ok, okx1 = xl + 16 < W && chan_ok;
        const unsigned cb2 = (unsigned)cbase * 2u;
        // strip form: entry of (fragment mi, this lane) -> (image, row, column) by two magic divisions (any map size: the 128 entries of a
        // wave may span several rows and, on maps of a few pixels, several images)
        const int e0 = x0 + wm * 128 + fr;
        auto pixel = [&](int mi, unsigned& pix) -> bool {
            if constexpr (STRIP != 0) {
                const int e = e0 + 16 * mi;
                const int ec = e < sg.NE ? e : 0;
                const int bb = strip_div(ec, sg.mIS), r = ec - bb * sg.IS;
                const int yy = strip_div(r, sg.mRS), xx = r - yy * sg.RS;
                pix = (unsigned)((bb * H + yy) * W + xx);
                return e < sg.NE && yy < H && xx < W && chan_ok;
            } else {
                pix = pix0 + (unsigned)((mi >> 1) * W + (mi & 1) * 16);
                return (y0 + wm * RPW + (mi >> 1) < H) && ((mi & 1) ? okx1 : okx0);
            }
        };
        if constexpr (SPLIT) {
            // residual = high + low halves: four 16-byte loads per pixel fragment, requested two fragments ahead of the arithmetic (a ring
            // of three fragments: 48 registers; the compiler places the waits).  The stores are issued by every lane (out-of-range ones
            // are dropped by the range check).
            f16x8 rq[3][4];
            auto res_load = [&](int mi) {
                unsigned pix;
                const bool ok = pixel(mi, pix);
                const unsigned ro = ok ? (pix * (unsigned)a.res_ct + (unsigned)a.res_coff) * 2u + cb2 : CY_OOB;
                rq[mi % 3][0] = __builtin_bit_cast(f16x8, load_b128(rsr, ro, 0));
                rq[mi % 3][1] = __builtin_bit_cast(f16x8, load_b128(rsr, ro, 16));
                rq[mi % 3][2] = __builtin_bit_cast(f16x8, load_b128(rsr, ro, a.res_lo * 2));
                rq[mi % 3][3] = __builtin_bit_cast(f16x8, load_b128(rsr, ro, a.res_lo * 2 + 16));
            };
            if (RES) { res_load(0); res_load(1); }
            if (stamps) t_rw = stamp_real();
#pragma unroll
            for (int mi = 0; mi < MIW; ++mi) {
                if (RES && mi + 2 < MIW) res_load(mi + 2);
                float bg[16], sc[16];          // (re-read from the LDS slot per fragment: 32 registers that need not live through the epilogue)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(bl + j * 4), u = *reinterpret_cast<const f32x4*>(bl + 256 + j * 4);
                    bg[j * 4] = t[0]; bg[j * 4 + 1] = t[1]; bg[j * 4 + 2] = t[2]; bg[j * 4 + 3] = t[3];
                    sc[j * 4] = u[0]; sc[j * 4 + 1] = u[1]; sc[j * 4 + 2] = u[2]; sc[j * 4 + 3] = u[3];
                }
                float vv[16];
                scale_bias_act16(acc[0][mi], acc[1][mi], acc[2][mi], acc[3][mi], bg, sc, a.act != 0, vv);
                if (RES) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        vv[j] += (float)rq[mi % 3][0][j] + (float)rq[mi % 3][2][j];
                        vv[8 + j] += (float)rq[mi % 3][1][j] + (float)rq[mi % 3][3][j];
                    }
                }
                f16x8 h0, h1, l0, l1;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    h0[j] = (f16)vv[j]; h1[j] = (f16)vv[8 + j];
                    l0[j] = (f16)(vv[j] - (float)h0[j]); l1[j] = (f16)(vv[8 + j] - (float)h1[j]);
                }
                unsigned pix;
                const bool ok = pixel(mi, pix);
                const unsigned so = ok ? (pix * (unsigned)a.out_ct + (unsigned)a.out_coff) * 2u + cb2 : CY_OOB;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, h0), rso, so, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, h1), rso, so, 16, 0);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, l0), rso, so, a.out_lo * 2, 0);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, l1), rso, so, a.out_lo * 2 + 16, 0);
            }
        } else {
        f16x8 rv[MIW][2];
        if (RES) {
#pragma unroll
            for (int mi = 0; mi < MIW; ++mi) {
                unsigned pix;
                const bool ok = pixel(mi, pix);
                const unsigned ro = ok ? (pix * (unsigned)a.res_ct + (unsigned)a.res_coff) * 2u + cb2 : CY_OOB;
                rv[mi][0] = __builtin_bit_cast(f16x8, load_b128(rsr, ro, 0));
                rv[mi][1] = __builtin_bit_cast(f16x8, load_b128(rsr, ro, 16));
            }
            CY_WAIT_VM(0);                                       // (older than them: only the second weight stage of the next patch)
        }
        if (stamps) t_rw = stamp_real();
#pragma unroll
        for (int mi = 0; mi < MIW; ++mi) {
            float vv[16];
            bias_act16(acc[0][mi], acc[1][mi], acc[2][mi], acc[3][mi], bv, a.act != 0, vv);
            if (RES) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { vv[j] += (float)rv[mi][0][j]; vv[8 + j] += (float)rv[mi][1][j]; }
            }
            f16x8 o0, o1;
#pragma unroll
            for (int j = 0; j < 8; ++j) { o0[j] = (f16)vv[j]; o1[j] = (f16)vv[8 + j]; }
            unsigned pix;
            const bool ok = pixel(mi, pix);
            const unsigned so = ok ? (pix * (unsigned)a.out_ct + (unsigned)a.out_coff) * 2u + cb2 : CY_OOB;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o0), rso, so, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o1), rso, so, 16, 0);
        }
        }
        if (stamps) t_ep = stamp_real();
        if (stamps && !next && tid == 0) g_wg_stamps[(size_t)(blockIdx.x % WG_STAMP_SLOTS) * 4 + 3] = t_ep - t_begin;    // [3] the workgroup's whole life
        if (!next) break;
        v = vn; ++n;
    }
}

template <int STRIP, bool SPLIT = false>
static hipError_t launch_widep_t(const ConvArgs& a, hipStream_t s, int total, const StripGeo& sg) {
    constexpr int PR = 18 * 34, NPC = (PR + 15) / 16, PROUNDS = STRIP ? STRIP : (NPC + 3) / 4;
    const size_t lds = 2 * PROUNDS * 4 * 1024 + 3 * 2 * 128 * 64 + 4096;        // halo x2, weight ring, bias (+ oscale) x2
    lds_cap<conv3x3_widep_kernel<SPLIT, false, STRIP>>(lds);       // both before the first launch of either
    lds_cap<conv3x3_widep_kernel<SPLIT, true, STRIP>>(lds);
    static const int ncu = [] { int dev = 0, n = 256; hipGetDevice(&dev); hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev); return n > 0 ? n : 256; }();
    const int grid = total < ncu ? total : ncu;
    if (a.res) return launch_lds<conv3x3_widep_kernel<SPLIT, true, STRIP>>(dim3(grid), dim3(512), lds, lds, s, a, total, sg);
    return launch_lds<conv3x3_widep_kernel<SPLIT, false, STRIP>>(dim3(grid), dim3(512), lds, lds, s, a, total, sg);
}

static hipError_t launch_widep(const ConvArgs& a, hipStream_t s) {
    const int total = a.B * ((a.Wi + 31) / 32) * ((a.Hi + 15) / 16) * ((pad64(a.Cout) + 127) / 128);
    return a.split ? launch_widep_t<0, true>(a, s, total, StripGeo{}) : launch_widep_t<0>(a, s, total, StripGeo{});
}

template <int STRIP, bool SPLIT = false>
static hipError_t launch_strip(const ConvArgs& a, hipStream_t s) {
    StripGeo sg;
    sg.RS = a.Wi + 1; sg.IS = (a.Hi + 1) * sg.RS; sg.NE = a.B * sg.IS;
    sg.mRS = ((1ull << 40) + sg.RS - 1) / sg.RS; sg.mIS = ((1ull << 40) + sg.IS - 1) / sg.IS;
    const int total = ((sg.NE + 511) / 512) * ((pad64(a.Cout) + 127) / 128);
    return launch_widep_t<STRIP, SPLIT>(a, s, total, sg);
}

// ------------------------------------------------------------------------------------------------ 1x1 (and 3x3 stride 2), pixels direct to registers
// A 1x1 convolution has no tap reuse, so staging the pixel operand through LDS only costs: in the tiled kernels above two
// thirds of the LDS-DMA pieces (60-180 issue cycles each) carry pixels that exactly one wave reads exactly once.  In NHWC
// the MFMA B-operand fragment of a lane (pixel fr, channels 8*(fq+4*kk)..+7) is 16 contiguous bytes in global memory, so
// here every wave loads its own pixels straight into registers (buffer_load_dwordx4, zero fill from the range check,
// RING-1 K chunks ahead) and only the weights - shared by all eight waves - go through LDS (RING slots, requested RING-1
// chunks ahead, counted vmcnt).  A wave owns MI*16 pixels x all BN = 64*NB channels of the workgroup's tile:
//   per 64-channel K chunk and wave: NB DMA pieces + 2*MI register loads for 8*NB*MI MFMAs (NB=4, MI=2: 8 for 64).
// Also handles the two-segment input (nearest-x2 upsample + concat) of layers 12 and 15: per-lane addresses anyway.
// FUSE2 (round 4; NB = 4, the tile holds all 256 output channels of its pixels): back-to-back fusion with the 1x1 convolution that is
// this layer's only reader (yolov8 model.3 -> model.4.cv1).  After the K loop a lane holds, per 64-channel block g, the 16 contiguous
// channels 64 g + 16 fq + 0..15 of its pixels: bias + SiLU, rounded to fp16 exactly as the store would, they ARE the MFMA B operand of
// the second GEMM for K chunk g once that layer's input channels are permuted at pack time (pack_weights_fused2) -- no LDS, no lane
// movement.  The second layer's four weight chunks (128 KB) are requested into the dead ring (+ one slot) right behind the loop and
// land under the first epilogue's arithmetic; its result is stored through the same epilogue form.  The 256-channel map between the
// two layers (2 MB per 512^2 tile) is never written or read.
// PERSIST (fp16 context, the 256-channel tile, not FUSE2; CY_DIRECT_PERSIST): one workgroup per CU walks tiles blockIdx.x,
// blockIdx.x + gridDim.x, ... of the order the one-tile form launches them in, and the request stream does not stop at a tile
// boundary.  The ring slot of a chunk is its running number over the workgroup's tiles mod RING (one flat loop over all the chunks,
// its RING steps written out; a tile ends behind whichever step its last chunk falls on), so the WAR / RAW argument of the one-tile
// loop holds across the boundary unchanged:
// a slot is requested into one barrier after its last read, and read one barrier after the counted wait that covers it.  While the
// last DIST chunks of a tile are computed, the requests going out are chunks 0 .. DIST-1 of the next tile (lane addresses, tap
// cursor and weight rows rebased at that point: nothing of the current tile is requested after it) and, ahead of them from wave 0,
// its bias slice into the other of two bias buffers -- the oldest request of the tile, so every counted wait of the tile covers it,
// as in the one-tile form.  The epilogue's stores (and residual loads) sit in the in-order vmcnt queue BEHIND the next tile's first
// DIST chunks and AHEAD of what its first iterations request: the steady-state count then waits for more than it needs (for part of
// the stores as well), never for less; a wait assumes only requests that were issued.  Chunk order, K order, MFMA order and
// epilogue are the one-tile form's: the outputs are bit-identical (tests/test_gpu_direct_persist.py).  Tiles of fewer than RING
// chunks keep the one-tile form (direct_persist_form, cy_conv_plan.cpp).
// Anatomy of the one-tile form at batch 256 (stamped build, us per workgroup; profiles/direct_persist.md): 512 -> 512 on 32 x 32:
// entry -> loop 3.8 | loop 19.7 | epilogue 3.9 | exit -> entry of the CU's next workgroup 2.2; 2048 -> 512: 3.6 | 81.5 | 4.0 | 2.2;
// 640 -> 256 on 64 x 64: 4.2 | 25.4 | 3.8 | 2.2; 3x3 s2 256 -> 512: 3.4 | 86.6 | 4.0 | 2.3 -- about 10 us per tile outside the loop.
// What the persistent form gains per layer (-6..-14 % on the 1x1 layers, -19..-22 % on the strided 3x3 ones) is that AND the exact
// vmcnt counts of its unconditional requests (see the step).  Tried and dropped on the way: the one-tile loop entered at a ring phase
// per tile with `c >= 0 && c < chunks` guards on the unrolled steps (the skipped-step paths make the compiler wait vmcnt(4..11) for
// the pixel registers: it waits for the weight pieces just requested); the flat loop as an unrolled `for` with an exit (not
// unrolled: the pixel ring went to scratch); four requesting waves in the strided form (the count that is safe for the other four
// makes the requesting ones wait for half of the pieces just requested).
// Registers: 251-256 VGPRs, no scratch -- the per-tile code (lane_addrs, the rebase, the epilogue) takes the lane's number from
// lane_now() and its divisors through an opaque copy, so that no lane constant or reciprocal is carried over the K loop; the bias
// values are read per pixel group and the residual one half at a time.
template <int NB, int MI, int RING, bool K3, bool SPLIT = false, int NDW = 8, bool FUSE2 = false, bool PERSIST = false>
__global__ __launch_bounds__(512, (NB * MI <= 4 && RING == 2) ? 2 : 1) void conv1x1_direct_kernel(const ConvArgs a) {
    static_assert(!FUSE2 || (NB == 4 && !SPLIT), "back-to-back fusion: 256-channel tile, fp16 context");
    static_assert(!PERSIST || (NB == 4 && RING == 3 && !SPLIT && !FUSE2), "persistent form: 256-channel tile, fp16 context, not the fused pair");
    // NDW = number of waves that request the weight chunks (LDS-DMA): 8 = every wave its share; 4 = waves 0-3 only (one per SIMD),
    // so that a request waiting for room in the memory pipeline holds one wave of a SIMD while its partner keeps the matrix pipe busy
    // SPLIT (fp16x3 context): three passes over the K chunks -- pixels [x_lo | x_hi | x_hi] (the low halves a.in*_lo halves behind
    // the high ones) against the packed weight chunks [w_hi | w_lo | w_hi]; scaled / split epilogue
    constexpr int NW = 8, BN = 64 * NB, BM = NW * MI * 16, W_BYTES = BN * 128, DIST = RING - 1;
    constexpr int WPW = BN / 8 / NDW, APW = 2 * MI, PER = WPW + APW;     // weight pieces per requesting wave and chunk; pixel loads; both
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const bool stamps = CY_STAMPS_ENABLED && (a.dbg & 64) != 0;      // diagnostic builds: per-workgroup phase records (see the wide kernel)
    const unsigned long long t_entry = stamps ? stamp_real() : 0;
    typedef __attribute__((address_space(3))) void lds_void;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const int HoWo = a.Ho * a.Wo, M = a.B * HoWo;
    const int cpad = pad128(a.Cout);
    const int ntn = (pad64(a.Cout) + BN - 1) / BN;
    const int total = PERSIST ? ((M + BM - 1) / BM) * ntn : (int)gridDim.x;       // tiles of the launch
    int tile = blockIdx.x;                                                       // PERSIST: the tile being computed
    const int id = xcd_remap(tile, total);
    int m0 = (id / ntn) * BM, n0 = (id % ntn) * BN;
    // K chunk c = slab * taps + tap (the order of the packed weights).  k = 3 (strided 3x3 layers): every tap is the same
    // per-lane centre-pixel address plus a UNIFORM shift, which rides in soffset; soffset is unsigned, so the resource base
    // is moved back by the largest negative shift (one row + one pixel) and the shift is biased by the same amount.  Lanes
    // whose tap falls outside the image get the OOB sentinel in voffset (the only part that is range-checked) -> zeros.
    // K3 = false is the plain 1x1 kernel: none of the tap arithmetic is compiled in.
    constexpr int taps = K3 ? 9 : 1, pad = K3 ? 1 : 0, kk3 = K3 ? 3 : 1;
    const int pchunks = (a.Cin / 64) * taps, c0chunks = a.c1 ? a.c0 / 64 : pchunks;     // chunks of one pass; of its first segment
    const int chunks = SPLIT ? a.split * pchunks : pchunks;
    const unsigned bias_bytes = K3 ? (unsigned)((a.Wi + 1) * a.in0_ct) * 2u : 0u;

    // (num_records widened by the bias so that the check passes whether or not the hardware adds soffset before it)
    const auto rs0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(a.in0)) - bias_bytes, 0,
                                                       a.in0_bytes + 2 * bias_bytes, 0x00020000);
    const auto rs1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.c1 ? a.in1 : a.in0), 0,
                                                       a.c1 ? a.in1_bytes : a.in0_bytes, 0x00020000);
    const auto rsw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wgt), 0, a.wgt_bytes, 0x00020000);
    unsigned v0[MI], v1[MI], vmask[MI];                     // lane addresses of the tile whose chunks are being REQUESTED
    auto lane_addrs = [&](int mt) __attribute__((always_inline)) {
    const int ln = PERSIST ? lane_now() : lane;
    int fr = ln & 15, fq = ln >> 4, HoWo = a.Ho * a.Wo, Wo = a.Wo;
    // PERSIST: recomputed per tile -- neither the lane parts nor the reciprocals of the two divisors are kept in registers over the K loop
    if constexpr (PERSIST) asm volatile("" : "+s"(HoWo), "+s"(Wo));
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int m = mt + (wave * MI + mi) * 16 + fr;
        v0[mi] = v1[mi] = CY_OOB;
        vmask[mi] = 0;
        if (m < M) {
            const int b = m / HoWo, r = m - b * HoWo, ho = r / Wo, wo = r - ho * Wo;
            int p0;
            if (a.up0) p0 = (b * (a.Hi >> 1) + (ho >> 1)) * (a.Wi >> 1) + (wo >> 1);
            else p0 = (b * a.Hi + ho * a.s) * a.Wi + wo * a.s;                      // centre tap: always inside the image
            v0[mi] = (unsigned)(p0 * a.in0_ct + a.in0_coff + fq * 8) * 2u;
            v1[mi] = (unsigned)(m * a.in1_ct + a.in1_coff + fq * 8) * 2u;
            unsigned vm = 0;
#pragma unroll
            for (int kh = 0; kh < kk3; ++kh)
#pragma unroll
                for (int kw = 0; kw < kk3; ++kw)
                    if ((unsigned)(ho * a.s + kh - pad) < (unsigned)a.Hi && (unsigned)(wo * a.s + kw - pad) < (unsigned)a.Wi)
                        vm |= 1u << (kh * kk3 + kw);
            vmask[mi] = vm;
        }
    }
    };
    lane_addrs(m0);
    // piece j of requesting wave w = rows (j * NDW + w) * 8 .. +7 of the chunk: the lane part (row & 7 = lane >> 3) is the same for
    // every j, the rest is uniform and rides in soffset
    // developer ablation (diagnostic builds; results invalid): bit 0 no weight requests in the loop, bit 1 no weight fragment reads,
    // bit 2 no MFMAs, bit 3 no pixel loads in the loop.  Round 3, 1024 -> 256 channels on 64 x 64 maps at batch 256, us per K chunk in a
    // stamped build: everything 2.57 | no weight requests 2.42 | no fragment reads 2.34 | no MFMAs 1.70 | no pixel loads 1.59 | MFMAs +
    // fragment reads 1.35 | MFMAs alone 1.16 | barriers alone 0.33.  The loop waits for its operands: per chunk a workgroup fetches
    // 32 KB of pixels and 32 KB of weights, and 64 KB per ~3900 cycles = 16-17 B per cycle and CU is the rate every fetch-heavy kernel
    // of this library tops out at (the wide kernel's requests alone: 15.7 B per cycle).  More requests in flight do not help -- touching
    // the pixel lines 1 / 2 / 4 chunks ahead of the register ring (4-byte LDS-DMA into a dump area) made every 1x1 layer 9-21 % SLOWER --
    // only fewer bytes per MFMA would, and the 256 px x 256 ch tile is the largest the 128 accumulator registers of 8 waves allow.
    // The lane -> address map of the pixel loads costs a little: the MFMA operand layout puts four DIFFERENT pixels (four 128-byte
    // lines, 16 bytes of each) into every quad of lanes.  A timing-only build whose quads read 64 contiguous bytes of ONE pixel (same
    // bytes per instruction, wrong lanes) ran the 1x1 layers 1.5-9.6 % and the strided 3x3 layers 4.6-7.5 % faster (0.39 ms of the
    // 27.4 ms forward pass at batch 256); getting the data back into operand order is a 4 x 4 lane transpose per register (four
    // ds_bpermute_b32 per load, or ~20 DPP / permlane-swap moves).  Built with ds_bpermute (the next chunk's registers transposed behind
    // the current chunk's MFMAs; bit-identical, 234 conv / forward tests green): every layer 2-14 % SLOWER (forward 28.34 vs 27.80 ms):
    // the 16 permutes per wave and chunk cost two to three times what the better access pattern gives.  Not kept.
    // Round 4: the eight requests of a chunk (four weight pieces, four pixel loads per wave) issued one behind each of the chunk's eight
    // MFMA groups instead of together at its start, where all eight waves stand behind the barrier (same order, same counted waits;
    // bit-identical, 296 conv / forward tests green): forward 27.31-27.48 vs 27.37-27.38 ms, the K-heavy layers 0-2 % SLOWER.  Not kept.
    // Also round 4: a persistent-kernel grid of ncu - 8 / 16 / 32 workgroups (CUs left to the side streams) changes nothing in the
    // config-5 pass (4864-4893 vs 4890-4905 tiles/s).
    const bool no_dma = CY_STAMPS_ENABLED && (a.dbg & 1), no_rd = CY_STAMPS_ENABLED && (a.dbg & 2), no_mma = CY_STAMPS_ENABLED && (a.dbg & 4),
               no_px = CY_STAMPS_ENABLED && (a.dbg & 8);
    const bool reqw = wave < NDW;
    auto weight_rows = [&](int nt, int ln) { return (unsigned)((nt + wave * 8 + (ln >> 3)) * 128 + ((ln & 7) ^ (ln >> 3)) * 16); };
    unsigned woff0 = weight_rows(n0, lane);                       // (PERSIST: of the tile whose chunks are being requested)
    u32x4 xa[RING][MI][2];
    int ltap = 0, lslab = 0;                                // cursor of load_a (called for c = 0, 1, 2, ... in order)
    auto load_a = [&](int slot, int cv) {                   // the uniform part of the address rides in soffset (not range-checked)
        if (no_px) return;
        int lo = 0;
        const int c = SPLIT ? x3_chunk(cv, pchunks, lo) : cv;           // physical chunk (the weights are packed per virtual chunk)
        const unsigned lo0 = SPLIT && lo ? (unsigned)a.in0_lo * 2u : 0u, lo1 = SPLIT && lo ? (unsigned)a.in1_lo * 2u : 0u;
        if constexpr (PERSIST && !K3) {                     // the segment selected, not branched on: one group of loads on every path (see the steps)
            const bool seg1 = c >= c0chunks;
            if (c == c0chunks) {                            // first chunk of the second segment: its lane addresses from here to the tile's end
#pragma unroll                                              // (load_a is called for c = 0, 1, 2, ... in order; lane_addrs restores v0 for the next tile)
                for (int mi = 0; mi < MI; ++mi) v0[mi] = v1[mi];
            }
            const auto rs = seg1 ? rs1 : rs0;
            const unsigned so = (unsigned)((seg1 ? c - c0chunks : c) * 128);
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
                    xa[slot][mi][kk] = load_b128(rs, v0[mi], so + kk * 64);
            return;
        }
        if (!(PERSIST && K3) && c >= c0chunks) {            // (no strided 3x3 layer has a second segment: its persistent form keeps no v1)
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
                    xa[slot][mi][kk] = load_b128(rs1, v1[mi], ((c - c0chunks) * 64 + kk * 32) * 2 + lo1);
        } else if constexpr (!K3) {
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
                    xa[slot][mi][kk] = load_b128(rs0, v0[mi], (c * 64 + kk * 32) * 2 + lo0);
        } else {
            const int kh = ltap / 3, kw = ltap - kh * 3;
            const unsigned so = bias_bytes + (unsigned)((((kh - 1) * a.Wi + (kw - 1)) * a.in0_ct + lslab * 64) * 2) + lo0;
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                const unsigned vo = ((vmask[mi] >> ltap) & 1u) ? v0[mi] : CY_OOB;
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) xa[slot][mi][kk] = load_b128(rs0, vo, so + kk * 64);
            }
            if (++ltap == 9) { ltap = 0; ++lslab; if (SPLIT && lslab * 9 == pchunks) lslab = 0; }
        }
    };
    auto dma_w = [&](int slot, int c) {
        if ((NDW < NW && !reqw) || no_dma) return;
#pragma unroll
        for (int j = 0; j < WPW; ++j)
            dma_piece(rsw, (lds_ptr_t*)(smem + slot * W_BYTES + (j * NDW + wave) * 1024), woff0, c * cpad * 128 + j * NDW * 1024);
    };
    // counted wait of a requesting wave: all but its n youngest requests have landed (the other waves have no LDS-DMA of their own;
    // the loads of their pixel registers are waited for by the compiler at the use)
    auto wait_w = [&](int n) {
        if (NDW < NW && !reqw) return;
        if (n == APW + 2 * PER) { CY_WAIT_VM(APW + 2 * PER); }
        else if (n == APW + PER) { CY_WAIT_VM(APW + PER); }
        else { CY_WAIT_VM(APW); }
    };
    f32x4 acc[NB * 4][MI];
#pragma unroll
    for (int ni = 0; ni < NB * 4; ++ni)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto compute_x = [&](int slot, const u32x4 (&xs)[MI][2]) {
        const char* Wb = smem + slot * W_BYTES;
        // 2*NB groups of (4 weight fragments, 4*MI MFMAs); the fragments of group i+1 are read before the MFMAs of group i
        f16x8 wb[2][4];
        auto load_wb = [&](f16x8* dst, int gi) {
            if (no_rd) return;
            const int kk = gi / NB, g = gi % NB, qf = fq + 4 * kk;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int r = g * 64 + ni * 16 + fr;
                dst[ni] = *reinterpret_cast<const f16x8*>(Wb + r * 128 + ((qf ^ (r & 7)) << 4));
            }
        };
        load_wb(wb[0], 0);
#pragma unroll
        for (int gi = 0; gi < 2 * NB; ++gi) {
            const int kk = gi / NB, g = gi % NB;
            if (gi + 1 < 2 * NB) load_wb(wb[(gi + 1) & 1], gi + 1);
            if (!no_mma)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
                    acc[g * 4 + ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                        wb[gi & 1][ni], __builtin_bit_cast(f16x8, xs[mi][kk]), acc[g * 4 + ni][mi], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto compute = [&](int slot) { compute_x(slot, xa[slot]); };

    // the tile's BN bias values -> LDS with the very first request (wave 0; oldest request: every counted wait covers it), so
    // that the epilogue does not start with an exposed L2 round trip
    float* const bias_lds = reinterpret_cast<float*>(smem + (FUSE2 ? 4 : RING) * W_BYTES);
    if (wave == 0) {
        const auto rsb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.bias), 0, (unsigned)pad64(a.Cout) * 4u, 0x00020000);
        dma_piece(rsb, (lds_ptr_t*)bias_lds, lane * 16 < BN * 4 ? (unsigned)(n0 * 4 + lane * 16) : CY_OOB, 0);
    }
    // prologue: chunks 0..DIST-1 requested (weights first, then pixels, per chunk: the order the counted waits assume)
#pragma unroll
    for (int d = 0; d < DIST; ++d)
        if (PERSIST || d < chunks) { dma_w(d, d); load_a(d, d); }       // (PERSIST: at least RING chunks)
    // weights of chunk 0 landed; what was requested after them may stay in flight (DIST is 2 or 3)
    if (chunks >= DIST) wait_w(APW + (DIST - 1) * PER);
    else if (DIST == 3 && chunks == 2) wait_w(APW + PER);
    else wait_w(APW);
    __builtin_amdgcn_s_barrier();
    const unsigned long long t_loop = stamps ? stamp_real() : 0, c_loop = stamps ? stamp_now() : 0;
    if constexpr (!PERSIST) {
#pragma unroll 1
    for (int cb = 0; cb < chunks; cb += RING) {
#pragma unroll
        for (int u = 0; u < RING; ++u) {
            const int c = cb + u;
            if (c < chunks) {
                if (c + DIST < chunks) { dma_w((u + DIST) % RING, c + DIST); load_a((u + DIST) % RING, c + DIST); }
                compute(u);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                // weights of chunk c+1 must have landed; everything requested after them may stay in flight
                if (c + DIST < chunks) wait_w(APW + (DIST - 1) * PER);
                else if (DIST == 3 && c + 2 < chunks) wait_w(APW + PER);
                else wait_w(APW);
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    }

    const unsigned long long t_epi = stamps ? stamp_real() : 0, c_epi = stamps ? stamp_now() : 0;
    if constexpr (FUSE2) {
        // every wave is past the loop's last barrier: the ring is free.  Second layer: chunks 0..3 -> slots 0..3 (the launch gives
        // this form a fourth slot), bias2 behind the first bias
        const auto rsw2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wgt2), 0, a.wgt2_bytes, 0x00020000);
        const int cpad2 = pad128(a.cout2);
        if ((NDW == NW || reqw)) {
#pragma unroll
            for (int c2 = 0; c2 < 4; ++c2)
#pragma unroll
                for (int j = 0; j < WPW; ++j)
                    dma_piece(rsw2, (lds_ptr_t*)(smem + c2 * W_BYTES + (j * NDW + wave) * 1024), woff0, c2 * cpad2 * 128 + j * NDW * 1024);
        }
        float* const bias2_lds = reinterpret_cast<float*>(smem + 4 * W_BYTES) + 256;
        if (wave == 0) {
            const auto rsb2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.bias2), 0, (unsigned)pad64(a.cout2) * 4u, 0x00020000);
            dma_piece(rsb2, (lds_ptr_t*)bias2_lds, lane * 16 < BN * 4 ? (unsigned)(lane * 16) : CY_OOB, 0);
        }
        // first epilogue in registers: bias + SiLU, rounded to fp16 like the store it replaces -> B fragments of the second GEMM
        float* const bias1_lds = reinterpret_cast<float*>(smem + 4 * W_BYTES);
        u32x4 x2[4][MI][2];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float bv[16];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(bias1_lds + g * 64 + fq * 16 + j * 4);
                bv[j * 4] = t[0]; bv[j * 4 + 1] = t[1]; bv[j * 4 + 2] = t[2]; bv[j * 4 + 3] = t[3];
            }
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                float v[16];
                bias_act16(acc[g * 4][mi], acc[g * 4 + 1][mi], acc[g * 4 + 2][mi], acc[g * 4 + 3][mi], bv, a.act != 0, v);
                f16x8 h0, h1;
#pragma unroll
                for (int j = 0; j < 8; ++j) { h0[j] = (f16)v[j]; h1[j] = (f16)v[8 + j]; }
                x2[g][mi][0] = __builtin_bit_cast(u32x4, h0); x2[g][mi][1] = __builtin_bit_cast(u32x4, h1);
            }
        }
#pragma unroll
        for (int ni = 0; ni < NB * 4; ++ni)
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
        CY_WAIT_VM(0);
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int c2 = 0; c2 < 4; ++c2) compute_x(c2, x2[c2]);
        // second epilogue: bias2 + activation, 16 contiguous channels per lane and 64-channel block
#pragma unroll
        for (int g = 0; g < NB; ++g) {
            const int cbase = g * 64 + fq * 16;
            if (cbase >= pad64(a.cout2)) continue;
            float bv[16];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(bias2_lds + g * 64 + fq * 16 + j * 4);
                bv[j * 4] = t[0]; bv[j * 4 + 1] = t[1]; bv[j * 4 + 2] = t[2]; bv[j * 4 + 3] = t[3];
            }
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                const int m = m0 + (wave * MI + mi) * 16 + fr;
                if (m >= M) continue;
                const int b = m / HoWo, r = m - b * HoWo;
                const long opix = (long)b * a.out_bs + a.out_ro + r;
                float v[16];
                bias_act16(acc[g * 4][mi], acc[g * 4 + 1][mi], acc[g * 4 + 2][mi], acc[g * 4 + 3][mi], bv, a.act2 != 0, v);
                f16* dst = reinterpret_cast<f16*>(a.out2) + opix * a.out2_ct + a.out2_coff + cbase;
                if (cbase + 16 <= a.cout2) {
                    f16x8 o0, o1;
#pragma unroll
                    for (int j = 0; j < 8; ++j) { o0[j] = (f16)v[j]; o1[j] = (f16)v[8 + j]; }
                    *reinterpret_cast<f16x8*>(dst) = o0;
                    *reinterpret_cast<f16x8*>(dst + 8) = o1;
                } else {
#pragma unroll
                    for (int j = 0; j < 16; ++j)
                        if (cbase + j < a.cout2) dst[j] = (f16)v[j];
                }
            }
        }
        return;
    }
    // ---- epilogue: per 64-channel block the same 16-contiguous-channels-per-lane layout as the other kernels
    auto epilogue = [&](const float* bias_l) __attribute__((always_inline)) {
    const int ln = PERSIST ? lane_now() : lane;
    int fr = ln & 15, fq = ln >> 4, HoWo = a.Ho * a.Wo;
    if constexpr (PERSIST) asm volatile("" : "+s"(HoWo));      // (as in lane_addrs)
#pragma unroll
    for (int g = 0; g < NB; ++g) {
        const int cbase = n0 + g * 64 + fq * 16;
        if (cbase >= pad64(a.Cout)) continue;
        float bv[16];
        auto load_bv = [&](int off) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(bias_l + off + j * 4);
            bv[j * 4] = t[0]; bv[j * 4 + 1] = t[1]; bv[j * 4 + 2] = t[2]; bv[j * 4 + 3] = t[3];
        }
        };
        if constexpr (!PERSIST) load_bv(g * 64 + fq * 16);
        float sc[SPLIT ? 16 : 1];
        if constexpr (SPLIT) {
#pragma unroll
            for (int j = 0; j < 16; ++j) sc[j] = a.oscale[cbase + j];
        }
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            const int m = m0 + (wave * MI + mi) * 16 + fr;
            if (m >= M) continue;
            const int b = m / HoWo, r = m - b * HoWo;
            const long opix = (long)b * a.out_bs + a.out_ro + r;
            float v[16];
            if constexpr (SPLIT) {
                scale_bias_act16(acc[g * 4][mi], acc[g * 4 + 1][mi], acc[g * 4 + 2][mi], acc[g * 4 + 3][mi], bv, sc, a.act != 0, v);
                f16* dst = reinterpret_cast<f16*>(a.out) + opix * a.out_ct + a.out_coff + cbase;
                const f16* rp = a.res ? reinterpret_cast<const f16*>(a.res) + (long)m * a.res_ct + a.res_coff + cbase : nullptr;
                if (cbase + 16 <= a.Cout) {
                    if (rp) {
                        const f16x8 r0v = *reinterpret_cast<const f16x8*>(rp), r1v = *reinterpret_cast<const f16x8*>(rp + 8);
                        const f16x8 q0v = *reinterpret_cast<const f16x8*>(rp + a.res_lo), q1v = *reinterpret_cast<const f16x8*>(rp + a.res_lo + 8);
#pragma unroll
                        for (int j = 0; j < 8; ++j) { v[j] += (float)r0v[j] + (float)q0v[j]; v[8 + j] += (float)r1v[j] + (float)q1v[j]; }
                    }
                    store_split16(dst, a.out_lo, v);
                } else {
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        if (cbase + j >= a.Cout) continue;
                        float t = v[j];
                        if (rp) t += (float)rp[j] + (float)rp[a.res_lo + j];
                        store_split1(dst + j, a.out_lo, t);
                    }
                }
                continue;
            }
            if constexpr (PERSIST) {        // the 16 bias values read again per pixel group (the same values): not held in registers across the
                int off = g * 64 + fq * 16;     // stores and residual loads of the group before, where the next tile's first pixel chunks are live too
                asm volatile("" : "+v"(off));
                load_bv(off);
            }
            bias_act16(acc[g * 4][mi], acc[g * 4 + 1][mi], acc[g * 4 + 2][mi], acc[g * 4 + 3][mi], bv, a.act != 0, v);
            if (cbase + 16 <= a.Cout) {
                f16* dst = reinterpret_cast<f16*>(a.out) + opix * a.out_ct + a.out_coff + cbase;
                if (a.res) {
                    const f16* rp = reinterpret_cast<const f16*>(a.res) + (long)m * a.res_ct + a.res_coff + cbase;
                    if constexpr (PERSIST) {        // one half at a time: the next tile's first pixel chunks are live in registers here
                        const f16x8 r0v = *reinterpret_cast<const f16x8*>(rp);
#pragma unroll
                        for (int j = 0; j < 8; ++j) v[j] += (float)r0v[j];
                        __builtin_amdgcn_sched_barrier(0);
                        const f16x8 r1v = *reinterpret_cast<const f16x8*>(rp + 8);
#pragma unroll
                        for (int j = 0; j < 8; ++j) v[8 + j] += (float)r1v[j];
                    } else {
                    const f16x8 r0v = *reinterpret_cast<const f16x8*>(rp), r1v = *reinterpret_cast<const f16x8*>(rp + 8);
#pragma unroll
                    for (int j = 0; j < 8; ++j) { v[j] += (float)r0v[j]; v[8 + j] += (float)r1v[j]; }
                    }
                }
                f16x8 o0, o1;
#pragma unroll
                for (int j = 0; j < 8; ++j) { o0[j] = (f16)v[j]; o1[j] = (f16)v[8 + j]; }
                *reinterpret_cast<f16x8*>(dst) = o0;
                *reinterpret_cast<f16x8*>(dst + 8) = o1;
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int c = cbase + j;
                    if (c >= a.Cout) continue;
                    float t = v[j];
                    if (a.res) t += (float)(reinterpret_cast<const f16*>(a.res)[(long)m * a.res_ct + a.res_coff + c]);
                    reinterpret_cast<f16*>(a.out)[opix * a.out_ct + a.out_coff + c] = (f16)t;
                }
            }
        }
    }
    };
    if constexpr (!PERSIST) {
        epilogue(bias_lds);
    } else {
        const int stride = gridDim.x;
        int bsel = 0, c = 0;                                // bias buffer of the tile; chunk of the tile
        int tnext = tile + stride;
        bool more = tnext < total;
        // One flat loop over the chunks of all the workgroup's tiles: the chunk with running number g sits in slot g % RING = u, and a
        // tile ends (epilogue, accumulators cleared, next tile) behind whichever step its last chunk falls on.  No step is ever skipped,
        // so the compiler's count of the loads in flight is the same on every path.
        // (the steps are written out, not an unrolled loop: an unrolled loop with an exit in its body is not unrolled, and a
        // run-time slot index puts the pixel ring into scratch)
                auto step = [&](auto U) __attribute__((always_inline)) -> bool {           // one chunk in slot U; true behind the workgroup's last tile
                    constexpr int u = decltype(U)::value;
                    {
                        // one request per step, always: chunk c + DIST of this tile, or chunk c + DIST - chunks of the NEXT tile (same slot
                        // arithmetic), or -- behind the workgroup's last tile -- the same instructions with out-of-range lane addresses
                        // (zeros into a dead slot and dead registers, no memory traffic).  With the request unconditional the compiler
                        // counts the pixel loads in flight exactly; behind a conditional one it waits vmcnt(0) for the pixel registers
                        // of every RING-th chunk, as it does in the one-tile form.
                        int cq = c + DIST;
                        if (cq >= chunks) {
                            cq -= chunks;
                            if (cq == 0) {                  // first request past the tile: rebase the request state, bias slice first
                                ltap = 0; lslab = 0;
                                if (more) {
                                    const int idn = xcd_remap(tnext, total);
                                    const int ln = lane_now();         // (as in lane_addrs: nothing kept in registers over the K loop)
                                    lane_addrs((idn / ntn) * BM);
                                    woff0 = weight_rows((idn % ntn) * BN, ln);
                                    if (wave == 0) {
                                        const auto rsb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.bias), 0, (unsigned)pad64(a.Cout) * 4u, 0x00020000);
                                        dma_piece(rsb, (lds_ptr_t*)(bias_lds + (bsel ^ 1) * 256), ln * 16 < BN * 4 ? (unsigned)((idn % ntn) * BN * 4 + ln * 16) : CY_OOB, 0);
                                    }
                                } else {
                                    lane_addrs(M);          // every lane out of range
                                    woff0 = CY_OOB;
                                }
                            }
                        }
                        dma_w((u + DIST) % RING, cq); load_a((u + DIST) % RING, cq);
                        compute(u);
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        // weights of the next chunk (of this tile or of the next) must have landed; what was requested after them may
                        // stay in flight.  Behind a tile boundary the epilogue's stores and residual loads are among the younger
                        // operations as well: the wait then covers more than it needs
                        wait_w(APW + (DIST - 1) * PER);
                        __builtin_amdgcn_sched_barrier(0);
                        __builtin_amdgcn_s_barrier();
                        __builtin_amdgcn_sched_barrier(0);
                        if (++c == chunks) {                // the tile's last chunk
                            epilogue(bias_lds + bsel * 256);
                            if (!more) return true;
#pragma unroll
                            for (int ni = 0; ni < NB * 4; ++ni)
#pragma unroll
                                for (int mi = 0; mi < MI; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
                            tile = tnext; tnext = tile + stride; more = tnext < total;
                            const int idn = xcd_remap(tile, total);
                            m0 = (idn / ntn) * BM; n0 = (idn % ntn) * BN;
                            c = 0; bsel ^= 1;
                        }
                    }
                    return false;
                };
        static_assert(!PERSIST || RING == 3, "three steps written out");
#pragma unroll 1
        for (;;) {
            if (step(std::integral_constant<int, 0>{})) break;
            if (step(std::integral_constant<int, 1>{})) break;
            if (step(std::integral_constant<int, 2>{})) break;
        }
        CY_WAIT_VM(0);                                     // the zero requests behind the last tile: landed before the workgroup gives its LDS back
    }
    if (stamps && tid == 0) {
        unsigned long long* rec = g_wg_stamps + (size_t)(blockIdx.x % WG_STAMP_SLOTS) * 4;
        const unsigned long long t_exit = stamp_real();
        rec[0] = t_loop - t_entry; rec[1] = t_epi - t_loop; rec[2] = t_exit - t_epi; rec[3] = c_epi - c_loop;
        // the workgroup's whole life and where it ran: entry, exit, (XCC id << 16) | (SE, SH, CU fields of HW_ID)
        unsigned long long* life = g_wg_life + (size_t)(blockIdx.x % WG_STAMP_SLOTS) * 3;
        life[0] = t_entry; life[1] = t_exit;
        life[2] = ((unsigned long long)(__builtin_amdgcn_s_getreg(20 | (31 << 11)) & 15u) << 16) | (__builtin_amdgcn_s_getreg(4 | (31 << 11)) & 0xff00u);
    }
}

template <int NB, int MI, int RING, bool K3, bool SPLIT = false, int NDW = 8, bool FUSE2 = false>
static hipError_t launch_direct(const ConvArgs& a, hipStream_t s) {
    constexpr int BN = 64 * NB, BM = 8 * MI * 16;
    const size_t lds = (FUSE2 ? 4 : RING) * BN * 128 + 2048;             // weight ring (four slots for the second layer of a fused pair), bias (x2)
    const int M = a.B * a.Ho * a.Wo;
    const int blocks = ((M + BM - 1) / BM) * ((pad64(a.Cout) + BN - 1) / BN);
    return launch_lds<conv1x1_direct_kernel<NB, MI, RING, K3, SPLIT, NDW, FUSE2>>(dim3(blocks), dim3(512), lds, lds, s, a);
}

// persistent form of the 256-channel tile (fp16 context): one workgroup per CU walks the tiles; grid_cap > 0 (CY_DIRECT_PERSIST_GRID,
// tests) caps the grid so that small launches walk several tiles per workgroup
template <bool K3, int NDW>
static hipError_t launch_direct_persist(const ConvArgs& a, hipStream_t s, int grid_cap) {
    constexpr int BN = 256, BM = 256, RING = 3;
    const size_t lds = RING * BN * 128 + 2048;                            // weight ring, two bias buffers
    const int M = a.B * a.Ho * a.Wo;
    const int tiles = ((M + BM - 1) / BM) * ((pad64(a.Cout) + BN - 1) / BN);
    if ((a.Cin / 64) * (K3 ? 9 : 1) < RING || (K3 && a.c1)) return hipErrorInvalidValue;      // (conv_kernel never chooses it there)
    static const int ncu = [] { int dev = 0, n = 256; hipGetDevice(&dev); hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev); return n > 0 ? n : 256; }();
    const int cap = grid_cap > 0 ? grid_cap : ncu;
    const int grid = tiles < cap ? tiles : cap;
    return launch_lds<conv1x1_direct_kernel<4, 2, RING, K3, false, NDW, false, true>>(dim3(grid), dim3(512), lds, lds, s, a);
}

template <int WM, int RING>
static hipError_t launch_halo(const ConvArgs& a, hipStream_t s) {
    constexpr int TH = 4 * WM, NT = WM * 128;
    constexpr int PR = (TH + 2) * 18, NWI = (PR + 7) / 8, NW = NT / 64, PROUNDS = (NWI + NW - 1) / NW;
    const size_t lds = 2 * PROUNDS * NW * 1024 + RING * 128 * 128;
    const int blocks = a.B * ((a.Hi + TH - 1) / TH) * ((a.Wi + 15) / 16) * ((pad64(a.Cout) + 127) / 128);
    return launch_lds<conv3x3_halo_kernel<WM, RING>>(dim3(blocks), dim3(NT), lds, lds, s, a);
}

template <typename T, int WM, int WN, int MI, int NSTAGE = 2, bool SPLIT = false>
static hipError_t launch_t(const ConvArgs& a, hipStream_t s) {
    constexpr int BM = WM * MI * 16, BN = WN * 64;
    const int M = a.B * a.Ho * a.Wo;
    const int ntm = (M + BM - 1) / BM, ntn = (pad64(a.Cout) + BN - 1) / BN;
    const size_t lds = NSTAGE * (BM + BN) * 128;
    return launch_lds<conv_igemm_kernel<T, WM, WN, MI, NSTAGE, SPLIT>>(dim3(ntm * ntn), dim3(WM * WN * 64), lds, lds, s, a);
}

// head1x1_kernel's launch (which layers it takes: head_direct, cy_conv_plan.cpp)
template <bool SPLIT>
static hipError_t launch_head(const ConvArgs& a, hipStream_t s) {
    const int nrows = head_rows(a);
    const size_t lds = (size_t)(SPLIT ? a.split : 1) * (a.Cin / 64) * nrows * 128 + (a.Cout == 64 && a.out_f32 ? 4 * 32 * 68 * 4 : 0);     // weights + store transpose
    const long M = (long)a.B * a.Ho * a.Wo;
    const long wgs = (M + 127) / 128;                             // one 32-pixel group per wave at least
    return launch_lds<head1x1_kernel<SPLIT>>(dim3((unsigned)(wgs < 512 ? wgs : 512)), dim3(256), lds, 65536 + 4 * 32 * 68 * 4, s, a, nrows);      // persistent: two 4-wave workgroups per CU
}

// the two output convolutions of a stride level as one launch (head1x1_pair_kernel): a = box branch (64 channels at column 0),
// b = class branch (nc channels at column 64) of the same pixels and prediction rows (head_pair_ok, cy_conv_plan.cpp)
hipError_t launch_head_pair(Precision p, const ConvArgs& a, const ConvArgs& b, hipStream_t s) {
    const size_t lds = head_pair_lds(p, a, b);
    lds_cap<head1x1_pair_kernel<false>>(128 * 1024);              // both before the first launch of either
    lds_cap<head1x1_pair_kernel<true>>(128 * 1024);
    const long M = (long)a.B * a.Ho * a.Wo;
    const long wgs = (M + 255) / 256;                             // one 32-pixel group per wave at least
    const unsigned grid = (unsigned)(wgs < 256 ? wgs : 256);           // persistent: one 8-wave workgroup per CU is what the register file holds
    if (p == PREC_F16X3) return launch_lds<head1x1_pair_kernel<true>>(dim3(grid), dim3(512), lds, 128 * 1024, s, a, b, head_rows(b), head_pair_pitch(a.out_ct));
    return launch_lds<head1x1_pair_kernel<false>>(dim3(grid), dim3(512), lds, 128 * 1024, s, a, b, head_rows(b), head_pair_pitch(a.out_ct));
}

// The launcher call a ConvChoice names: one per kernel value, no decision.  Only the instantiation follows from the precision: the
// three-pass (SPLIT) form in the fp16x3 context, the float form of the generic kernel in fp32 (conv_choose gives a context the
// kernels it has).  with_dbg: the developer ablation bits of the kernels that look at them (0 in the product binary).
static ConvArgs with_dbg(const ConvArgs& a) { ConvArgs b = a; b.dbg = dev_knob("CY_DBG", 0); return b; }

hipError_t launch_conv(Precision p, const ConvChoice& choice, const ConvArgs& a, hipStream_t s) {
    const bool x3 = p == PREC_F16X3, f32 = p == PREC_F32;
    switch (choice.kernel) {
        case CK_WIDE_128: return x3 ? launch_wide<2, false, true>(a, s) : launch_wide<2>(with_dbg(a), s);
        case CK_WIDE_128_PERSIST: return x3 ? launch_widep(a, s) : launch_widep(with_dbg(a), s);
        case CK_STRIP_10: return x3 ? launch_strip<10, true>(a, s) : launch_strip<10>(a, s);
        case CK_STRIP_12: return x3 ? launch_strip<12, true>(a, s) : launch_strip<12>(a, s);
        case CK_WIDE_64: return x3 ? launch_wide<1, false, true>(a, s) : launch_wide<1>(a, s);
        case CK_WIDE_DUAL: return x3 ? launch_wide<2, true, true>(a, s) : launch_wide<2, true>(a, s);
        case CK_HALO2: return launch_halo2(with_dbg(a), s);
        case CK_HALO_2_2: return launch_halo<2, 2>(with_dbg(a), s);
        case CK_PP_2: return launch_pp<2>(a, s);
        case CK_C64_64: return launch_c64<64>(a, s);
        case CK_C64_32: return launch_c64<32>(a, s);
        // (the persistent form of the 256-channel tile: every wave requests in the strided form too, so that the compiler's count of the
        // pixel loads in flight holds for all waves)
        case CK_DIRECT_256_K1: return x3 ? launch_direct<4, 2, 3, false, true>(a, s) : choice.direct_persist ? launch_direct_persist<false, 8>(with_dbg(a), s, choice.persist_grid)
                                                                                       : launch_direct<4, 2, 3, false>(with_dbg(a), s);
        case CK_DIRECT_256_K3: return x3 ? launch_direct<4, 2, 3, true, true>(a, s) : choice.direct_persist ? launch_direct_persist<true, 8>(with_dbg(a), s, choice.persist_grid)
                                                                                      : launch_direct<4, 2, 3, true, false, 4>(with_dbg(a), s);
        case CK_DIRECT_256_K1_FUSE2: return launch_direct<4, 2, 3, false, false, 8, true>(with_dbg(a), s);
        case CK_DIRECT_256_K3_FUSE2: return launch_direct<4, 2, 3, true, false, 4, true>(with_dbg(a), s);
        case CK_DIRECT_128_K1: return x3 ? launch_direct<2, 2, 2, false, true>(a, s) : launch_direct<2, 2, 2, false>(a, s);
        case CK_DIRECT_128_K3: return x3 ? launch_direct<2, 4, 2, true, true>(a, s) : launch_direct<2, 4, 2, true>(a, s);
        case CK_HEAD: return x3 ? launch_head<true>(a, s) : launch_head<false>(a, s);
        case CK_GENERIC_BIG: return launch_t<f16, 4, 2, 4, 3>(a, s);
        case CK_GENERIC_64: return x3 ? launch_t<f16, 4, 1, 2, 2, true>(a, s) : f32 ? launch_t<float, 4, 1, 2>(a, s) : launch_t<f16, 4, 1, 2>(a, s);
        case CK_GENERIC_128: return x3 ? launch_t<f16, 2, 2, 4, 2, true>(a, s) : f32 ? launch_t<float, 2, 2, 4>(a, s) : launch_t<f16, 2, 2, 4>(a, s);
        default: return hipErrorInvalidValue;      // CK_BAD_ARGS
    }
}

void debug_read_wg_stamps(unsigned long long* out, int n) {      // raw per-workgroup records (n x 4) of stamped builds
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wg_stamps), (size_t)(n < WG_STAMP_SLOTS ? n : WG_STAMP_SLOTS) * 4 * sizeof(unsigned long long));
}

void debug_read_wg_life(unsigned long long* out, int n) {        // entry, exit, CU of the pixels-direct kernel's workgroups (n x 3), stamped builds
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wg_life), (size_t)(n < WG_STAMP_SLOTS ? n : WG_STAMP_SLOTS) * 3 * sizeof(unsigned long long));
}

void debug_read_stamps(unsigned long long* out8, bool reset) {
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_stamps), 8 * sizeof(unsigned long long));
    if (CY_STAMPS_ENABLED && out8[6] == 0) {        // no summed stamps: average the wide kernel's per-workgroup records instead
        static unsigned long long rec[WG_STAMP_SLOTS * 4];
        hipMemcpyFromSymbol(rec, HIP_SYMBOL(g_wg_stamps), sizeof(rec));
        for (int i = 0; i < WG_STAMP_SLOTS; ++i)
            if (rec[i * 4 + 1]) { out8[6] += 1; for (int j = 0; j < 4; ++j) out8[j] += rec[i * 4 + j]; }
        out8[4] = out8[0] + out8[1] + out8[2] + out8[3];
        if (reset) { memset(rec, 0, sizeof(rec)); hipMemcpyToSymbol(HIP_SYMBOL(g_wg_stamps), rec, sizeof(rec)); }
    }
    if (reset) { unsigned long long z[8] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof(z)); }
}

}  // namespace cy
