// Host-side weight packing into the layouts the convolution kernels stage (slab-major panels, the fp16x3 passes, the second layer
// of a fused pair), and the fp32 <-> high / low halves element kernels of the fp16x3 context.
#include "cy_kernels.h"
#include "cy_conv_dev.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace cy {

// ------------------------------------------------------------------------------------------------ weights
// Packed layout ("slab-major"): [K chunk of 128 B][tap][row in Cout_pad128][128 B] (zero rows past Cout, so no kernel
// needs a range check on weight rows).  The unit every kernel stages -- the
// rows n0..n0+BN of one (chunk, tap) -- is ONE contiguous run of BN*128 bytes, so a DMA wave-instruction (8 rows) reads
// 1 KiB of consecutive cache lines instead of 8 lines a whole filter row (k*k*Cin elements) apart.  K is zero-padded to
// a whole chunk; rows are permuted per 64 so that a lane of the MFMA result holds 16 contiguous output channels.
size_t packed_weight_bytes(Precision p, int cout, int cin, int k, int chunk_bytes) {
    const int epb = chunk_bytes / (p == PREC_F16 ? 2 : 4);
    return (size_t)((cin + epb - 1) / epb) * k * k * pad128(cout) * chunk_bytes;
}

void pack_weights(Precision p, const float* W, int cout, int cin, int k, void* dst, int chunk_bytes) {
    const int taps = k * k, cp = pad128(cout), epb = chunk_bytes / (p == PREC_F16 ? 2 : 4), chunks = (cin + epb - 1) / epb;
    memset(dst, 0, packed_weight_bytes(p, cout, cin, k, chunk_bytes));
    for (int row = 0; row < cp; ++row) {
        const int blk = row >> 6, ni = (row >> 4) & 3, rr = row & 15;
        const int n = blk * 64 + (rr >> 2) * 16 + ni * 4 + (rr & 3);      // channel held by packed row `row`
        if (n >= cout) continue;
        for (int t = 0; t < taps; ++t)
            for (int c = 0; c < cin; ++c) {
                const float v = W[((size_t)n * cin + c) * taps + t];
                const size_t o = (((size_t)(c / epb) * taps + t) * cp + row) * epb + (c % epb);
                if (p == PREC_F16) reinterpret_cast<f16*>(dst)[o] = (f16)v;
                else reinterpret_cast<float*>(dst)[o] = v;
            }
    }
    (void)chunks;
}

// second layer of a back-to-back pair: 1x1 weights with the input channels in the accumulator order of the first layer's kernel
void pack_weights_fused2(const float* W2, int cout2, int cin2, void* dst) {
    std::vector<float> perm((size_t)cout2 * cin2);
    for (int n = 0; n < cout2; ++n)
        for (int p = 0; p < cin2; ++p) {
            const int c = p >> 6, kk = (p >> 5) & 1, q = (p >> 3) & 3, j = p & 7;
            perm[(size_t)n * cin2 + p] = W2[(size_t)n * cin2 + 64 * c + 16 * q + 8 * kk + j];
        }
    pack_weights(PREC_F16, perm.data(), cout2, cin2, 1, dst);
}

// fp16x3 context.  Per output channel n the filter is scaled by 2^e(n) so that its largest weight lies in [2^13, 2^14): the low
// halves w_lo = fp16(w' - fp16(w')) of all but vanishing weights are then normal fp16 numbers (unscaled they would sit in the
// subnormal range and carry ~3e-6 relative error); oscale[n] = 2^-e(n) multiplies the accumulator in the epilogue (exact).
// K holds three passes over the (chunk-padded) input channels: w_hi, w_lo, w_hi -- against x_lo, x_hi, x_hi (see x3_chunk).
// TWO passes (round 4) when every weight of the layer is an fp16 value times its channel's scale, exactly: W[n] = fl32(w16[n] * scale[n])
// with w16 representable in fp16 -- what an ultralytics checkpoint is (its tensors are stored in fp16; Conv + BatchNorm are folded in
// fp32 at load time, so the folded filter of channel n is the fp16 filter times gamma / sqrt(var + eps)).  The layer is then
// scale[n] * sum_k (x_lo + x_hi) * w16: K holds [w16 | w16] against [x_lo | x_hi], oscale[n] = scale[n], and the weights carry no
// rounding at all.  x3_passes() decides from the numbers themselves (scale = null: all ones).
int x3_passes(const float* W, int cout, int cin, int k, const float* scale) {
    const size_t per = (size_t)cin * k * k;
    for (int n = 0; n < cout; ++n) {
        const float sc = scale ? scale[n] : 1.0f;
        if (!(sc != 0.0f) || !std::isfinite(sc)) return 3;
        for (size_t i = 0; i < per; ++i) {
            const float w = W[(size_t)n * per + i];
            const f16 h = (f16)(w / sc);
            if (!((float)h * sc == w)) return 3;
        }
    }
    return 2;
}

size_t packed_weight_bytes_x3(int cout, int cin, int k, int chunk_bytes, int passes) {
    const int epb = chunk_bytes / 2;
    return packed_weight_bytes(PREC_F16, cout, passes * ((cin + epb - 1) / epb * epb), k, chunk_bytes);
}

void pack_weights_x3(const float* W, int cout, int cin, int k, void* dst, float* oscale, int chunk_bytes, int passes, const float* scale) {
    const int taps = k * k, epb = chunk_bytes / 2, cinp = (cin + epb - 1) / epb * epb, cp = pad128(cout);
    memset(dst, 0, packed_weight_bytes_x3(cout, cin, k, chunk_bytes, passes));
    for (int i = 0; i < cp; ++i) oscale[i] = 1.0f;
    f16* o = reinterpret_cast<f16*>(dst);
    for (int row = 0; row < cp; ++row) {
        const int blk = row >> 6, ni = (row >> 4) & 3, rr = row & 15;
        const int n = blk * 64 + (rr >> 2) * 16 + ni * 4 + (rr & 3);      // channel held by packed row `row`
        if (n >= cout) continue;
        if (passes == 2) {                                   // exact fp16 filter, the channel's scale in the epilogue
            const float sc = scale ? scale[n] : 1.0f;
            oscale[n] = sc;
            for (int t = 0; t < taps; ++t)
                for (int c = 0; c < cin; ++c) {
                    const f16 h = (f16)(W[((size_t)n * cin + c) * taps + t] / sc);
                    for (int pass = 0; pass < 2; ++pass) {
                        const int cv = pass * cinp + c;
                        o[(((size_t)(cv / epb) * taps + t) * cp + row) * epb + (cv % epb)] = h;
                    }
                }
            continue;
        }
        float m = 0.0f;
        for (size_t i = 0; i < (size_t)cin * taps; ++i) m = fmaxf(m, fabsf(W[(size_t)n * cin * taps + i]));
        int e = 0;
        if (m > 0.0f && std::isfinite(m)) { int ex; frexpf(m, &ex); e = 14 - ex; }       // m = f * 2^ex, f in [0.5, 1): m * 2^e in [2^13, 2^14)
        if (e > 60) e = 60;
        if (e < -60) e = -60;
        const float up = ldexpf(1.0f, e);
        oscale[n] = ldexpf(1.0f, -e);
        for (int t = 0; t < taps; ++t)
            for (int c = 0; c < cin; ++c) {
                const float v = W[((size_t)n * cin + c) * taps + t] * up;
                const f16 hi = (f16)v, lo = (f16)(v - (float)hi);
                for (int pass = 0; pass < 3; ++pass) {
                    const int cv = pass * cinp + c;
                    o[(((size_t)(cv / epb) * taps + t) * cp + row) * epb + (cv % epb)] = pass == 1 ? lo : hi;
                }
            }
    }
}

// fp32 NHWC <-> high / low halves (kernel-level test entry and debug reads of the fp16x3 context)
__global__ __launch_bounds__(256) void x3_split_kernel(const float* __restrict__ in, f16* __restrict__ out, long n, int C) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long pix = i / C; const int c = (int)(i - pix * C);
        store_split1(out + pix * 2 * C + c, C, in[i]);
    }
}
__global__ __launch_bounds__(256) void x3_merge_kernel(const f16* __restrict__ in, float* __restrict__ out, long n, int C) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long pix = i / C; const int c = (int)(i - pix * C);
        out[i] = (float)in[pix * 2 * C + c] + (float)in[pix * 2 * C + C + c];
    }
}
hipError_t launch_x3_split(const float* in, void* out, long npix, int C, hipStream_t s) {
    const long n = npix * C;
    hipLaunchKernelGGL(x3_split_kernel, dim3((unsigned)((n + 255) / 256 < 65535 ? (n + 255) / 256 : 65535)), dim3(256), 0, s, in, reinterpret_cast<f16*>(out), n, C);
    return hipGetLastError();
}
hipError_t launch_x3_merge(const void* in, float* out, long npix, int C, hipStream_t s) {
    const long n = npix * C;
    hipLaunchKernelGGL(x3_merge_kernel, dim3((unsigned)((n + 255) / 256 < 65535 ? (n + 255) / 256 : 65535)), dim3(256), 0, s, reinterpret_cast<const f16*>(in), out, n, C);
    return hipGetLastError();
}

}  // namespace cy
