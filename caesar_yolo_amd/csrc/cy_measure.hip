// Catalog source measurement (cy_measure_sources): per source box, on the HBM-resident fp32 mosaic as cy_mosaic_prepare leaves it,
//   npix / nring   valid pixels (value != 0 and finite) of the box window / of the ring of `ring` pixels around it
//   bkg, rms       exact median of the ring's valid pixels and 1.4826 x the exact median of |v - bkg| (float64)
//   peak, x/y_peak largest valid pixel of the box window, first occurrence in row-major order
//   sum, sw, swx, swy   sum of (v - bkg), and the moments of the weights max(v - bkg, 0), float64
// One workgroup of 256 threads per source; the integer windows are solved on the host (launch_measure's caller) from the float64
// boxes.  Neither the box window nor the ring is assumed to fit LDS: every pass re-reads its pixels (a ring of a catalog source
// is a few KiB and stays in the vector cache / L2), 64-bit pixel offsets throughout (the 32k mosaic is one 4 GiB allocation).
// Medians are the exact radix selections of cy_select.h (pixels: 4 passes, deviations: 8 passes, one more for the upper middle
// element of an even count when it is a different value); the ring hands its valid pixels to them.
// Sums: float64 per lane over increasing pixel index, then the block reduction of cy_reduce.h, finished by thread 0.  Nothing here
// is atomic outside LDS, and the LDS atomics are integer counts.
#include "cy_px.h"                      // valid_px
#include "cy_reduce.h"                  // RedSlots, reduction
#include "cy_select.h"                  // SelSmem, select_median
#include <climits>

#pragma clang fp contract(off)          // w * ix is rounded before it is added, as the float64 definition does

namespace cy {
namespace {

constexpr int MNT = 256, MUNROLL = 4;

struct MSmem {
    SelSmem<MNT> sel;
    RedSlots<MNT, 7> red;
};

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
// f(v) for every valid pixel of the ring; MUNROLL independent loads in flight per lane (an out-of-range slot reads as 0 = blank)
template <typename F>
__device__ __forceinline__ void ring_for_each(const float* __restrict__ img, size_t MW, const Ring& r, F f) {
    for (unsigned i0 = threadIdx.x; i0 < r.n; i0 += MUNROLL * MNT) {
        float v[MUNROLL];
#pragma unroll
        for (int u = 0; u < MUNROLL; ++u) { const unsigned i = i0 + u * MNT; v[u] = i < r.n ? ring_value(img, MW, r, i) : 0.0f; }
#pragma unroll
        for (int u = 0; u < MUNROLL; ++u) if (valid_px(v[u])) f(v[u]);
    }
}

__global__ __launch_bounds__(MNT) void measure_kernel(const MeasureArgs a) {
    __shared__ MSmem s;
    const int b = blockIdx.x, tid = threadIdx.x;
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
    const auto ring = [&](auto f) { ring_for_each(a.img, MW, r, f); };
    double bkg = select_median<0, MNT>(s.sel, ring, 0.0, 0xFFFFFFFFu, nring), rms = 0.0;
    if (nring) rms = 1.4826 * select_median<1, MNT>(s.sel, ring, bkg, 0xFFFFFFFFu, n2);

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
    const auto red = reduction(red_sum(sum), red_sum(sw), red_sum(swx), red_sum(swy), red_sum(npix), red_first_max(pv, pp, (long long)LLONG_MAX));
    red.wave();
    __syncthreads();
    red.park(s.red);
    __syncthreads();
    if (tid == 0) {
        red.total(s.red);
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

// cy_debug_reduce: cy_reduce.h on its own, one workgroup per row of `len` entries, thread t on entries t, t + 256, ..  Per row and
// finishing style (0: thread 0 after the barrier, 1: every thread, read back from the last one) eight 64-bit words: the float64 sum
// of val (bits), the entry count, the first maximum of the valid keys (float bits, index; none: -inf, 0xFFFFFFFF), the smallest
// and the largest index of a valid key (int; none: INT_MAX, -1), the first maximum again with a long long index (none:
// LLONG_MAX), and the smallest such index as unsigned long long (none: all ones)
__global__ __launch_bounds__(MNT) void reduce_probe_kernel(const double* __restrict__ val, const float* __restrict__ key, const int len,
                                                           unsigned long long* __restrict__ out) {
    __shared__ RedSlots<MNT, 9> s;
    const int tid = threadIdx.x;
    const size_t row = (size_t)blockIdx.x * (size_t)len;
    double sum = 0.0;
    unsigned n = 0, pi = 0xFFFFFFFFu;
    float pv = -INFINITY, qv = -INFINITY;
    int imin = INT_MAX, imax = -1;
    long long qi = LLONG_MAX;
    unsigned long long umin = ~0ull;
    for (int i = tid; i < len; i += MNT) {
        sum += val[row + i]; ++n;
        const float k = key[row + i];
        if (!valid_px(k)) continue;
        if (k > pv) { pv = k; pi = (unsigned)i; qv = k; qi = i; }                   // increasing index per lane: the first stays
        imin = min(imin, i); imax = max(imax, i);
        if ((unsigned long long)i < umin) umin = (unsigned long long)i;
    }
    const auto red = reduction(red_sum(sum), red_sum(n), red_first_max(pv, pi, 0xFFFFFFFFu), red_min(imin), red_max(imax),
                               red_first_max(qv, qi, (long long)LLONG_MAX), red_min(umin));
    red.wave();
    red.park(s);
    __syncthreads();
    for (int style = 0; style < 2; ++style) {                // thread 0 overwrites only its own registers in between
        if (tid != (style ? MNT - 1 : 0)) continue;
        red.total(s);
        unsigned long long* o = out + ((size_t)blockIdx.x * 2 + style) * 8;
        o[0] = (unsigned long long)__double_as_longlong(sum); o[1] = n; o[2] = __float_as_uint(pv); o[3] = pi;
        o[4] = (unsigned long long)(long long)imin; o[5] = (unsigned long long)(long long)imax; o[6] = (unsigned long long)qi; o[7] = umin;
    }
}

}  // namespace

void debug_reduce(const double* d_val, const float* d_key, int nrows, int len, unsigned long long* d_out) {
    hipLaunchKernelGGL(reduce_probe_kernel, dim3(nrows), dim3(MNT), 0, 0, d_val, d_key, len, d_out);
}

hipError_t launch_measure(const MeasureArgs& a, hipStream_t s) {
    if (a.n < 1 || a.MH < 1 || a.MW < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(measure_kernel, dim3(a.n), dim3(MNT), 0, s, a);
    return hipGetLastError();
}

}  // namespace cy
