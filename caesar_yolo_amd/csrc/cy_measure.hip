// Catalog source measurement (cy_measure_sources): per source box, on the HBM-resident fp32 mosaic as cy_mosaic_prepare leaves it,
//   npix / nring   valid pixels (value != 0 and finite) of the box window / of the ring of `ring` pixels around it
//   bkg, rms       exact median of the ring's valid pixels and 1.4826 x the exact median of |v - bkg| (float64)
//   peak, x/y_peak largest valid pixel of the box window, first occurrence in row-major order
//   sum, sw, swx, swy   sum of (v - bkg), and the moments of the weights max(v - bkg, 0), float64
// One workgroup of 256 threads per source; the integer windows are solved on the host (launch_measure's caller) from the float64
// boxes.  Neither the box window nor the ring is assumed to fit LDS: every pass re-reads its pixels (a ring of a catalog source
// is a few KiB and stays in the vector cache / L2), 64-bit pixel offsets throughout (the 32k mosaic is one 4 GiB allocation).
// Medians are radix selections, 8 bits per pass over order-preserving 64-bit keys, 256-bin histograms in LDS:
//   pixels      fkey(v) in the high word                    -> 4 passes
//   deviations  bit pattern of the non-negative float64 d   -> 8 passes
// The selection finds the element of rank (n - 1) / 2 and how many elements are <= it; for an even n the upper middle element is
// the same value when that count exceeds n / 2, else the smallest larger key (one more pass).
// Sums: float64 per lane over increasing pixel index, __shfl_down tree per wave, the four waves added in order by thread 0:
// fixed association, so two runs give the same bits.  Nothing here is atomic outside LDS, and the LDS atomics are integer counts.
#include "cy_kernels.h"
#include <cfloat>
#include <climits>

#pragma clang fp contract(off)          // w * ix is rounded before it is added, as the float64 definition does

namespace cy {
namespace {

constexpr int MNT = 256, MNW = MNT / 64, MUNROLL = 4;

struct MSmem {
    unsigned hist[256];
    unsigned wsum[MNW];
    unsigned sel[4];                     // digit, rank inside the bin, elements below the bin, elements in the bin
    unsigned long long umin[MNW];
    double red[4][MNW];
    unsigned cnt[MNW];
    float pv[MNW]; long long pp[MNW];
};

__device__ __forceinline__ bool valid_px(float v) { return v != 0.0f && fabsf(v) <= FLT_MAX; }      // NaN fails the second test
__device__ __forceinline__ unsigned fkey32(float f) {                   // order-preserving float -> u32 (fkey of cy_preproc.hip)
    const unsigned b = __float_as_uint(f);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float fkey32_inv(unsigned k) { return __uint_as_float((k >> 31) ? (k & 0x7FFFFFFFu) : ~k); }

// The ring = grown window minus box window, as four rectangles walked one after the other with consecutive lanes on consecutive
// ix: top and bottom bands over the grown width, then the left and right flanks beside the box rows.
struct Ring {
    int bx0, bx1, by0, by1, gx0, gy0;
    unsigned gw, lw, rw, nT, nB, nL, n;
};
__device__ __forceinline__ float ring_value(const float* __restrict__ img, size_t MW, const Ring& r, unsigned i) {
    int ix, iy;
    if (i < r.nT) { iy = r.gy0 + (int)(i / r.gw); ix = r.gx0 + (int)(i % r.gw); }
    else if (i < r.nT + r.nB) { const unsigned j = i - r.nT; iy = r.by1 + 1 + (int)(j / r.gw); ix = r.gx0 + (int)(j % r.gw); }
    else if (i < r.nT + r.nB + r.nL) { const unsigned j = i - r.nT - r.nB; iy = r.by0 + (int)(j / r.lw); ix = r.gx0 + (int)(j % r.lw); }
    else { const unsigned j = i - r.nT - r.nB - r.nL; iy = r.by0 + (int)(j / r.rw); ix = r.bx1 + 1 + (int)(j % r.rw); }
    return img[(size_t)iy * MW + (size_t)ix];
}
template <int MODE> __device__ __forceinline__ unsigned long long ring_key(float v, double bkg) {
    if constexpr (MODE == 0) return (unsigned long long)fkey32(v) << 32;
    else return (unsigned long long)__double_as_longlong(fabs((double)v - bkg));      // d >= 0: orders like its bit pattern
}
template <int MODE> __device__ __forceinline__ double key_value(unsigned long long k) {
    if constexpr (MODE == 0) return (double)fkey32_inv((unsigned)(k >> 32));
    else return __longlong_as_double((long long)k);
}

// f(key) for every valid pixel of the ring; MUNROLL independent loads in flight per lane (an out-of-range slot reads as 0 = blank)
template <int MODE, typename F>
__device__ __forceinline__ void ring_for_each(const float* __restrict__ img, size_t MW, const Ring& r, double bkg, F f) {
    for (unsigned i0 = threadIdx.x; i0 < r.n; i0 += MUNROLL * MNT) {
        float v[MUNROLL];
#pragma unroll
        for (int u = 0; u < MUNROLL; ++u) { const unsigned i = i0 + u * MNT; v[u] = i < r.n ? ring_value(img, MW, r, i) : 0.0f; }
#pragma unroll
        for (int u = 0; u < MUNROLL; ++u) if (valid_px(v[u])) f(ring_key<MODE>(v[u], bkg));
    }
}

// Exact median of the keys of the ring's valid pixels; n = their count (0: returns 0).  Every thread gets the result.
template <int MODE>
__device__ double ring_median(MSmem& s, const float* __restrict__ img, size_t MW, const Ring& r, double bkg, unsigned& n) {
    constexpr int NP = MODE == 0 ? 4 : 8;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned long long prefix = 0;
    unsigned k = 0, below = 0, eq = 0;
    n = 0;
    for (int p = 0; p < NP; ++p) {
        const int shift = 56 - 8 * p;
        s.hist[tid] = 0;
        __syncthreads();
        const unsigned long long want = p ? prefix >> (shift + 8) : 0;
        ring_for_each<MODE>(img, MW, r, bkg, [&](unsigned long long key) {
            if (p == 0 || (key >> (shift + 8)) == want) atomicAdd(&s.hist[(unsigned)(key >> shift) & 255u], 1u);
        });
        __syncthreads();
        const unsigned h = s.hist[tid];
        unsigned incl = h;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        if (lane == 63) s.wsum[w] = incl;
        __syncthreads();
        unsigned off = 0, total = 0;
#pragma unroll
        for (int j = 0; j < MNW; ++j) { const unsigned t = s.wsum[j]; if (j < w) off += t; total += t; }
        if (p == 0) {
            n = total;
            if (n == 0) return 0.0;                         // uniform: `total` came from LDS
            k = (n - 1) / 2;
        }
        const unsigned excl = off + incl - h;
        if (k >= excl && k < excl + h) { s.sel[0] = (unsigned)tid; s.sel[1] = k - excl; s.sel[2] = excl; s.sel[3] = h; }
        __syncthreads();
        prefix |= (unsigned long long)s.sel[0] << shift;
        k = s.sel[1]; below += s.sel[2]; eq = s.sel[3];
    }
    const double a = key_value<MODE>(prefix);
    if ((n & 1u) || below + eq > n / 2) return a;           // odd count, or the upper middle element has the same value
    unsigned long long m = ~0ull;                           // smallest key above `prefix`
    ring_for_each<MODE>(img, MW, r, bkg, [&](unsigned long long key) { if (key > prefix && key < m) m = key; });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_down(m, o); m = t < m ? t : m; }
    if (lane == 0) s.umin[w] = m;
    __syncthreads();
    m = s.umin[0];
#pragma unroll
    for (int j = 1; j < MNW; ++j) m = s.umin[j] < m ? s.umin[j] : m;
    return (a + key_value<MODE>(m)) / 2.0;
}

__global__ __launch_bounds__(MNT) void measure_kernel(const MeasureArgs a) {
    __shared__ MSmem s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int* wn = a.win + (size_t)b * 8;
    // the host's windows are already inside the image; clamped again so that no index can leave it whatever arrives here
    const int bx0 = max(wn[0], 0), bx1 = min(wn[1], a.MW - 1), by0 = max(wn[2], 0), by1 = min(wn[3], a.MH - 1);
    const int gx0 = min(max(wn[4], 0), bx0), gx1 = max(min(wn[5], a.MW - 1), bx1), gy0 = min(max(wn[6], 0), by0), gy1 = max(min(wn[7], a.MH - 1), by1);
    double* out = a.out + (size_t)b * MEAS_FIELDS;
    if (bx1 < bx0 || by1 < by0) {                           // empty box window: nothing to measure, no ring either
        if (tid < MEAS_FIELDS) out[tid] = (tid == 5 || tid == 6) ? -1.0 : 0.0;
        return;
    }
    const size_t MW = (size_t)a.MW;
    const unsigned bw = (unsigned)(bx1 - bx0 + 1), bh = (unsigned)(by1 - by0 + 1);
    Ring r;
    r.bx0 = bx0; r.bx1 = bx1; r.by0 = by0; r.by1 = by1; r.gx0 = gx0; r.gy0 = gy0;
    r.gw = (unsigned)(gx1 - gx0 + 1); r.lw = (unsigned)(bx0 - gx0); r.rw = (unsigned)(gx1 - bx1);
    r.nT = (unsigned)(by0 - gy0) * r.gw; r.nB = (unsigned)(gy1 - by1) * r.gw; r.nL = r.lw * bh;
    r.n = r.nT + r.nB + r.nL + r.rw * bh;

    unsigned nring = 0, n2 = 0;
    double bkg = ring_median<0>(s, a.img, MW, r, 0.0, nring), rms = 0.0;
    if (nring) rms = 1.4826 * ring_median<1>(s, a.img, MW, r, bkg, n2);

    // ---- box window: counts, peak, moments
    double sum = 0.0, sw = 0.0, swx = 0.0, swy = 0.0;
    unsigned npix = 0;
    float pv = -INFINITY; long long pp = LLONG_MAX;
    const unsigned nb = bw * bh;
    for (unsigned i0 = tid; i0 < nb; i0 += MUNROLL * MNT) {
        float v[MUNROLL]; int ix[MUNROLL], iy[MUNROLL];
#pragma unroll
        for (int u = 0; u < MUNROLL; ++u) {
            const unsigned i = i0 + u * MNT;
            iy[u] = by0 + (int)(i / bw); ix[u] = bx0 + (int)(i % bw);
            v[u] = i < nb ? a.img[(size_t)iy[u] * MW + (size_t)ix[u]] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < MUNROLL; ++u) {
            if (!valid_px(v[u])) continue;
            ++npix;
            if (v[u] > pv) { pv = v[u]; pp = (long long)iy[u] * a.MW + ix[u]; }      // increasing index per lane: the first stays
            const double d = (double)v[u] - bkg;
            sum += d;
            if (d > 0.0) { sw += d; swx += d * (double)ix[u]; swy += d * (double)iy[u]; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_down(sum, o); sw += __shfl_down(sw, o); swx += __shfl_down(swx, o); swy += __shfl_down(swy, o);
        npix += __shfl_down(npix, o);
        const float v2 = __shfl_down(pv, o); const long long p2 = __shfl_down(pp, o);
        if (v2 > pv || (v2 == pv && p2 < pp)) { pv = v2; pp = p2; }
    }
    __syncthreads();
    if (lane == 0) { s.red[0][w] = sum; s.red[1][w] = sw; s.red[2][w] = swx; s.red[3][w] = swy; s.cnt[w] = npix; s.pv[w] = pv; s.pp[w] = pp; }
    __syncthreads();
    if (tid == 0) {
        for (int j = 1; j < MNW; ++j) {
            sum += s.red[0][j]; sw += s.red[1][j]; swx += s.red[2][j]; swy += s.red[3][j]; npix += s.cnt[j];
            if (s.pv[j] > pv || (s.pv[j] == pv && s.pp[j] < pp)) { pv = s.pv[j]; pp = s.pp[j]; }
        }
        out[0] = (double)npix; out[1] = (double)nring; out[2] = bkg; out[3] = rms;
        if (npix) {
            out[4] = (double)pv; out[5] = (double)(pp % a.MW); out[6] = (double)(pp / a.MW);
            out[7] = sum; out[8] = sw; out[9] = swx; out[10] = swy;
        } else {
            out[4] = 0.0; out[5] = -1.0; out[6] = -1.0; out[7] = 0.0; out[8] = 0.0; out[9] = 0.0; out[10] = 0.0;
        }
        out[11] = 0.0;
    }
}

}  // namespace

hipError_t launch_measure(const MeasureArgs& a, hipStream_t s) {
    if (a.n < 1 || a.MH < 1 || a.MW < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(measure_kernel, dim3(a.n), dim3(MNT), 0, s, a);
    return hipGetLastError();
}

}  // namespace cy
