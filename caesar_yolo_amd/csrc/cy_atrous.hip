// One level of the a trous (B3-spline, "starlet") decomposition (cy_atrous_step): the map smoothed by the separable five-tap kernel
// (1/16, 1/4, 3/8, 1/4, 1/16) with its taps `step` pixels apart, mirrored at the edges, and the detail plane in - smooth; definitions:
// include/caesar_yolo_hip.h, DESIGN.md "Residual scales".
// The row sum R(x, row) depends on (x, row) alone, and the output rows y, y +- step, y +- 2 step that use it lie in one residue class
// y mod step.  A thread owns a column and walks ATR_CHUNK consecutive output rows y = r + t * step of one class: it keeps the row
// sums of rows y - 2 step .. y + 2 step (folded into the image) as float64 in registers; the next output row shifts them by one and
// forms one new row sum from five loads, which the lanes of a wave make at consecutive addresses.  A chunk forms four row sums
// before its first output row; nothing else is computed twice.  Every pixel is read five times (the five column taps of its row),
// by the same workgroup at the same time: once from memory, four times from cache.  No LDS, no barrier, no atomics; no workgroup
// reads what another wrote.  fold() keeps every index inside the image, for any step; a thread at or beyond column MW does nothing.
// Work items (plan_atrous): item = (chunk * nres + r) * ncb + cb; a grid of at most ATR_GRID_MAX workgroups walks them with the
// grid's stride.  Every loop has a bound fixed before it starts:
//   items   item = blockIdx.x, += gridDim.x, below items < 2^31
//   rows    t = t0 .. min(t0 + ATR_CHUNK, rows of the class) - 1
#include "cy_px.h"
#include <cstdint>

#pragma clang fp contract(off)          // every product is rounded before it is added: one IEEE operation each, as the float64 definition has them

namespace cy {
namespace {

constexpr double H0 = 0.0625, H1 = 0.25, H2 = 0.375;         // the taps h0 = h4, h1 = h3, h2: exact in binary

// mirror without repeating the edge, for any i: period 2 (N - 1); an index inside [0, N) is itself
__device__ __forceinline__ int fold(const long long i, const int N) {
    if (i >= 0 && i < (long long)N) return (int)i;
    if (N == 1) return 0;
    const long long p = 2LL * ((long long)N - 1);
    long long m = i % p;
    if (m < 0) m += p;
    return (int)(m >= (long long)N ? p - m : m);
}

__device__ __forceinline__ double value(const float v) { return fabsf(v) <= FLT_MAX ? (double)v : 0.0; }      // NaN fails the test

// R(x, row) over the folded columns cx[0 .. 4] (cx[2] = x); *centre = a(x, row)
__device__ __forceinline__ double row_sum(const float* __restrict__ in, const size_t MW, const int row, const int* cx, double* centre) {
    const float* __restrict__ p = in + (size_t)row * MW;
    const float v0 = p[cx[0]], v1 = p[cx[1]], v2 = p[cx[2]], v3 = p[cx[3]], v4 = p[cx[4]];
    const double c = value(v2);
    double R = H0 * value(v0);
    R += H1 * value(v1);
    R += H2 * c;
    R += H1 * value(v3);
    R += H0 * value(v4);
    *centre = c;
    return R;
}

template <bool SMOOTH, bool DETAIL>
__global__ __launch_bounds__(ATR_COLS) void atrous_kernel(const AtrousArgs a) {
    const int MH = a.MH, MW = a.MW, s = a.step;
    const size_t W = (size_t)MW;
    for (int item = blockIdx.x; item < a.items; item += gridDim.x) {
        const int cb = item % a.ncb, q = item / a.ncb, r = q % a.nres, chunk = q / a.nres;
        const int nrow = (MH - r + s - 1) / s;                 // rows of class r: r < nres <= MH
        const int t0 = chunk * ATR_CHUNK, t1 = min(t0 + ATR_CHUNK, nrow);
        const long long xl = (long long)cb * ATR_COLS + threadIdx.x;
        if (t0 >= t1 || xl >= (long long)MW) continue;
        const int x = (int)xl;
        const int cx[5] = {fold(xl - 2 * s, MW), fold(xl - s, MW), x, fold(xl + s, MW), fold(xl + 2 * s, MW)};
        long long y = (long long)r + (long long)t0 * s;       // < MH
        double c0, c1, c2, c3, c4;                             // centres of the window's rows; c2 = a(x, y), c0 and c1 are not used
        double w0 = row_sum(a.in, W, fold(y - 2 * s, MH), cx, &c0);
        double w1 = row_sum(a.in, W, fold(y - s, MH), cx, &c1);
        double w2 = row_sum(a.in, W, (int)y, cx, &c2);
        double w3 = row_sum(a.in, W, fold(y + s, MH), cx, &c3);
        for (int t = t0; t < t1; ++t) {
            const double w4 = row_sum(a.in, W, fold(y + 2 * s, MH), cx, &c4);
            double C = H0 * w0;
            C += H1 * w1;
            C += H2 * w2;
            C += H1 * w3;
            C += H0 * w4;
            const float sm = (float)C;                          // one rounding to nearest even
            const size_t p = (size_t)y * W + (size_t)x;
            if (SMOOTH) a.smooth[p] = sm;
            if (DETAIL) a.detail[p] = (float)(c2 - (double)sm);
            w0 = w1; w1 = w2; w2 = w3; w3 = w4;
            c2 = c3; c3 = c4;
            y += s;
        }
    }
}

}  // namespace

hipError_t launch_atrous(const AtrousArgs& a, hipStream_t s) {
    // what the indexing rests on (plan_atrous): the item table matches the image and the step
    if (!a.in || (!a.smooth && !a.detail) || a.MH < 1 || a.MW < 1 || a.step < 1 || a.step > ATR_STEP_MAX || (long long)a.MH * a.MW >= (1LL << 31) ||
        (long long)a.ncb != ((long long)a.MW + ATR_COLS - 1) / ATR_COLS || a.nres != (a.step < a.MH ? a.step : a.MH) ||
        (long long)a.nchunk != (((long long)a.MH + a.step - 1) / a.step + ATR_CHUNK - 1) / ATR_CHUNK ||
        (long long)a.items != (long long)a.ncb * a.nres * a.nchunk || a.grid < 1 || a.grid > ATR_GRID_MAX || a.grid > a.items)
        return hipErrorInvalidValue;
    const dim3 grid(a.grid), block(ATR_COLS);
    if (a.smooth && a.detail) hipLaunchKernelGGL((atrous_kernel<true, true>), grid, block, 0, s, a);
    else if (a.smooth) hipLaunchKernelGGL((atrous_kernel<true, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((atrous_kernel<false, true>), grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace cy
