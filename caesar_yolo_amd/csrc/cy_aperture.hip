// Aperture sums at given positions (cy_aperture_sums); definitions: include/caesar_yolo_hip.h, DESIGN.md "Peak apertures".
//   aperture_kernel  per job K concentric rings around (cx, cy) on a map: counts, sum, sum of squares and variance sum of every
//                    ring, and the exact median and MAD of the outermost ring (the background annulus)
// One workgroup of 256 threads per job; the host (plan_apertures) decided the status, the squared radii and the window, which is
// inside the image.  A job that is not measured writes its row and returns before any barrier: the status comes from the job
// record, so the whole workgroup takes that branch together.
// Pass 1 walks the window once: pixel i = dy * W + dx on thread i mod 256, d2 = dx*dx + dy*dy (two products, one sum, not
// contracted), ring = the number of k < K with d2 > r2_k (the r2_k do not decrease, so that is the smallest k with d2 <= r2_k;
// ring == K: outside).  K is uniform and the comparisons are unrolled over APER_RINGS_MAX.  Per ring a thread keeps three float64
// accumulators and a count in registers and adds `ring == k ? x : 0.0` to each: indexing the arrays by `ring` would put them in
// scratch.  Adding +0.0 changes no bit: a sum starts at +0.0, a sum of non-zero terms that cancels is +0.0 under round-to-nearest,
// and no member is -0.0 (a valid v is non-zero, v*v and rms*rms of non-zero floats do not underflow in float64).
// Sums: sequential per thread in increasing i, then the block reduction of cy_reduce.h, finished by thread 0 after the medians.
// Then the two medians of the valid members of ring K by select_median (cy_select.h) with one walk over the window, the same in
// every pass, every thread taking part.  No global atomics, no inline assembly, nothing read that another workgroup wrote.
// Every loop has a bound fixed before it starts:
//   window   over the A <= 513 * 513 pixels of the window, 256 at a time (pass 1 once, the selection at most 4 + 1 + 8 + 1 times)
//   rings    APER_RINGS_MAX, unrolled; 6 shuffle steps and 4 waves
#include "cy_px.h"                      // valid_px, Win, window_of
#include "cy_reduce.h"                  // RedSlots, reduction
#include "cy_select.h"                  // SelSmem, select_median

#pragma clang fp contract(off)          // dx*dx + dy*dy: both products are rounded before the sum, as the float64 definition does

namespace cy {
namespace {

constexpr int APT = 256, APR = APER_RINGS_MAX;

struct ApSmem {
    SelSmem<APT> sel;
    RedSlots<APT, 4> red[APR];          // per ring: sum, sum of squares, variance sum, count
};

__global__ __launch_bounds__(APT) void aperture_kernel(const ApertureArgs a) {
    __shared__ ApSmem s;
    const int b = blockIdx.x, tid = threadIdx.x;
    const AperJob* __restrict__ job = a.jobs + b;
    double* out = a.out + (size_t)b * APER_FIELDS;
    const int K = a.K;
    const int win[4] = {job->x0, job->x1, job->y0, job->y1};
    Win wn;
    const long long area = window_of(win, a.MW, a.MH, wn);                        // held inside the image (cy_px.h)
    const int status = job->status ? job->status : (area == 0 || K < 1 || K > APR ? 2 : 0);
    if (status != 0) {                                        // uniform: the job record and the arguments only
        if (tid < APER_FIELDS) out[tid] = tid == 0 ? (double)status : (tid >= 1 && tid <= 4) ? -1.0 : 0.0;
        return;
    }
    const int bx0 = wn.x0, by0 = wn.y0;
    const unsigned W = wn.W, A = wn.A;
    const size_t MW = (size_t)a.MW, org = (size_t)by0 * MW + (size_t)bx0;
    const double cx = job->cx, cy = job->cy;
    double r2[APR];
#pragma unroll
    for (int k = 0; k < APR; ++k) r2[k] = k < K ? job->r2[k] : 0.0;
    const float* __restrict__ map = a.map;
    const float* __restrict__ rms = a.rms;

    // ring of window pixel i: 0 .. K - 1, K outside
    const auto ring_of = [&](const unsigned i, size_t& p) {
        const unsigned wy = i / W, wx = i - wy * W;
        p = org + (size_t)wy * MW + wx;
        const double dx = (double)(bx0 + (int)wx) - cx, dy = (double)(by0 + (int)wy) - cy;
        const double xx = dx * dx, yy = dy * dy;
        const double d2 = xx + yy;
        int ring = 0;
#pragma unroll
        for (int k = 0; k < APR; ++k) ring += (k < K && d2 > r2[k]) ? 1 : 0;
        return ring;
    };

    // ---- pass 1: counts and sums of every ring
    double S[APR], Q[APR], V[APR];
    unsigned N[APR];
#pragma unroll
    for (int k = 0; k < APR; ++k) { S[k] = 0.0; Q[k] = 0.0; V[k] = 0.0; N[k] = 0; }
    for (unsigned i = tid; i < A; i += APT) {
        size_t p;
        const int ring = ring_of(i, p);
        if (ring >= K) continue;
        const float px = map[p];
        if (!valid_px(px)) continue;
        const double v = (double)px, vv = v * v;
        double var = 0.0;
        if (rms) {
            const float rf = rms[p];
            if (rf > 0.0f && fabsf(rf) <= FLT_MAX) { const double r = (double)rf; var = r * r; }
        }
#pragma unroll
        for (int k = 0; k < APR; ++k) {
            const bool keep = ring == k;
            S[k] += keep ? v : 0.0; Q[k] += keep ? vv : 0.0; V[k] += keep ? var : 0.0;
            N[k] += keep ? 1u : 0u;
        }
    }
    // ring by ring, so that the compiler meets four quantities at a time (all 32 at once cost it twice the registers)
    const auto ring_red = [&](const int k) { return reduction(red_sum(S[k]), red_sum(Q[k]), red_sum(V[k]), red_sum(N[k])); };
#pragma unroll
    for (int k = 0; k < APR; ++k) { const auto red = ring_red(k); red.wave(); red.park(s.red[k]); }

    // ---- the background annulus: median and MAD of the valid pixels of ring K (the first barrier of select_median also orders
    // the parked values above before thread 0 reads them)
    const int last = K - 1;
    const auto annulus = [&](auto f) {
        for (unsigned i = tid; i < A; i += APT) {
            size_t p;
            if (ring_of(i, p) != last) continue;
            const float px = map[p];
            if (valid_px(px)) f(px);
        }
    };
    unsigned nann = 0, n2 = 0;
    const double med = select_median<0, APT>(s.sel, annulus, 0.0, 0xFFFFFFFFu, nann);
    double mad = 0.0;
    if (nann) mad = select_median<1, APT>(s.sel, annulus, med, 0xFFFFFFFFu, n2);

    if (tid == 0) {
        out[0] = 0.0;
        out[1] = (double)bx0; out[2] = (double)(bx0 + (int)W - 1); out[3] = (double)by0; out[4] = (double)(by0 + (int)wn.H - 1);
        out[5] = job->clipped ? 1.0 : 0.0;
        out[6] = nann ? med : 0.0; out[7] = mad;
#pragma unroll
        for (int k = 0; k < APR; ++k) {
            double* f = out + APER_HEAD + APER_RING_FIELDS * k;
            if (k < K) {
                ring_red(k).total(s.red[k]);
                f[0] = (double)N[k]; f[1] = S[k]; f[2] = Q[k]; f[3] = V[k];
            } else {
                f[0] = 0.0; f[1] = 0.0; f[2] = 0.0; f[3] = 0.0;
            }
        }
    }
}

}  // namespace

hipError_t launch_apertures(const ApertureArgs& a, hipStream_t s) {
    if (a.n < 1 || a.n > APER_JOBS_MAX || a.K < 1 || a.K > APER_RINGS_MAX || a.MH < 1 || a.MW < 1 || !a.map || !a.jobs || !a.out ||
        (long long)a.MH * a.MW >= (1LL << 31))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(aperture_kernel, dim3(a.n), dim3(APT), 0, s, a);
    return hipGetLastError();
}

}  // namespace cy
