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
// Sums: float64 per lane over increasing pixel index, __shfl_down tree per wave, the four waves added in order by thread 0:
// fixed association, so two runs give the same bits.  Nothing here is atomic outside LDS, and the LDS atomics are integer counts.
#include "cy_px.h"                      // valid_px
#include "cy_select.h"                  // SelSmem, select_median
#include <climits>

#pragma clang fp contract(off)          // w * ix is rounded before it is added, as the float64 definition does

namespace cy {
namespace {

constexpr int MNT = 256, MNW = MNT / 64, MUNROLL = 4;

struct MSmem {
    SelSmem<MNT> sel;
    double red[4][MNW];
    unsigned cnt[MNW];
    float pv[MNW]; long long pp[MNW];
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
