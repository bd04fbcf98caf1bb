// Residual peaks (cy_find_peaks): the local maxima of a map above k_sigma times a noise map, over the whole image; definitions:
// include/caesar_yolo_hip.h, DESIGN.md "Residual peaks".
// The image is cut into segments of PEAK_SEG = 1024 consecutive pixels of one row, segment s = iy * nsx + sx: their order is the
// row-major order of the pixels, so a peak's row is offset[s] + its rank inside s.  A workgroup of 256 threads takes a segment,
// thread t its pixels 4 t .. 4 t + 3; a grid of at most PK_GRID_MAX = 65536 workgroups walks the segments with the grid's stride.
//   peak_count_kernel  every thread tests `above` on its four pixels (8 bytes read per pixel: the only work on almost every pixel);
//                      a pixel that is above reads its neighbourhood (at most 17 x 17 values, from L2) and leaves at the first
//                      neighbour that outranks it.  Per wave and pixel slot j one ballot: word 4 w + j of the segment's bitmap, bit
//                      l = pixel 4 (64 w + l) + j; the popcounts of the four waves, added through LDS, are count[s]
//   peak_scan_kernel   one workgroup of 1024 threads walks the count table 1024 entries at a time: an inclusive shuffle scan per
//                      wave, the 16 wave totals through LDS, a running carry in a register -> offset[s] (exclusive) and the total
//   peak_fill_kernel   a segment with peaks and offset[s] < cap: every thread reads its wave's four bitmap words, the rank of its
//                      first pixel inside the wave is the popcount of the bits of the lanes below it, the waves before it are added
//                      through LDS; the thread that owns a peak computes its neighbourhood sums, row by row, and writes the row
// When MW % 4 == 0 and both maps are 16-byte aligned a thread's four pixels move as one 16-byte load (a quad is then inside the row or
// outside it); otherwise pixel by pixel.  A pixel at or beyond MW counts as 0: never above, never read.  Neighbourhoods are clipped
// to the image before they are walked.  No atomics, and no workgroup reads what another wrote in the same launch; the LDS words
// are double-buffered by the parity of the iteration, so that one barrier per segment orders them.
// Every loop has a bound fixed before it starts:
//   segments       seg = blockIdx.x, += gridDim.x, below nseg <= 2^24
//   neighbourhood  at most (2 radius + 1)^2 <= 289 pixels, inside the image
//   scan           ceil(nseg / 1024) rounds; 6 shuffle steps and 16 waves
#include "cy_px.h"                      // valid_px
#include <cstdint>

#pragma clang fp contract(off)          // every product is rounded before it is added or compared, as the float64 definition does

namespace cy {
namespace {

constexpr int PK_T = PEAK_SEG / 4, PK_W = PK_T / 64;
constexpr int PK_GRID_MAX = 1 << 16;    // 32 rounds of the 2048 workgroups a 256-CU chip holds at 8 waves per SIMD; a larger image is walked with the grid's stride
constexpr int SCAN_T = 1024, SCAN_W = SCAN_T / 64;
static_assert(PK_W * 4 == PEAK_SEG_WORDS, "one bitmap word per wave and pixel slot");

__device__ __forceinline__ bool above_px(float u, float r, double k) { return valid_px(u) && noisy_px(r) && (double)u >= k * (double)r; }

// the four values at p .. p + 3 of row-major map m, p being column ix of its row; 0 at and beyond column MW
template <bool VEC>
__device__ __forceinline__ void load_quad(const float* __restrict__ m, const size_t p, const int ix, const int MW, float* o) {
    o[0] = o[1] = o[2] = o[3] = 0.0f;
    if (VEC) {                                                // MW % 4 == 0: the quad is inside the row or outside it
        if (ix < MW) {
            const float4 q = *reinterpret_cast<const float4*>(m + p);
            o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
        }
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (ix + t < MW) o[t] = m[p + t];
    }
}

struct Hood { int x0, x1, y0, y1; };
__device__ __forceinline__ Hood hood_of(const PeakArgs& a, const int ix, const int iy) {
    return Hood{max(ix - a.radius, 0), min(ix + a.radius, a.MW - 1), max(iy - a.radius, 0), min(iy + a.radius, a.MH - 1)};
}

// (ix, iy) with u = fs * map there outranks every valid pixel of its neighbourhood
__device__ bool outranks_hood(const PeakArgs& a, const int ix, const int iy, const float u, const float fs) {
    const Hood h = hood_of(a, ix, iy);
    for (int qy = h.y0; qy <= h.y1; ++qy) {
        const float* __restrict__ row = a.map + (size_t)qy * (size_t)a.MW;
        for (int qx = h.x0; qx <= h.x1; ++qx) {
            const float uq = fs * row[qx];
            if (!valid_px(uq) || (qx == ix && qy == iy)) continue;
            if (uq > u || (uq == u && (qy < iy || (qy == iy && qx < ix)))) return false;
        }
    }
    return true;
}

template <bool VEC>
__global__ __launch_bounds__(PK_T) void peak_count_kernel(const PeakArgs a) {
    __shared__ unsigned wc[2][PK_W];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float fs = (float)a.sign;
    int it = 0;
    for (int seg = blockIdx.x; seg < a.nseg; seg += gridDim.x, it ^= 1) {
        const int iy = seg / a.nsx, ix = (seg - iy * a.nsx) * PEAK_SEG + 4 * tid;
        const size_t p = (size_t)iy * (size_t)a.MW + (size_t)ix;
        float v[4], r[4];
        load_quad<VEC>(a.map, p, ix, a.MW, v);
        load_quad<VEC>(a.rms, p, ix, a.MW, r);
        unsigned long long b[4];
        unsigned n = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float u = fs * v[t];
            const bool pk = above_px(u, r[t], a.k_sigma) && outranks_hood(a, ix + t, iy, u, fs);
            b[t] = __ballot(pk);
            n += (unsigned)__popcll(b[t]);
        }
        if (lane == 0) {
            unsigned long long* bw = a.bits + (size_t)seg * PEAK_SEG_WORDS + 4 * w;
#pragma unroll
            for (int t = 0; t < 4; ++t) bw[t] = b[t];
            wc[it][w] = n;
        }
        __syncthreads();
        if (tid == 0) {
            unsigned c = 0;
#pragma unroll
            for (int j = 0; j < PK_W; ++j) c += wc[it][j];
            a.count[seg] = c;
        }
    }
}

__global__ __launch_bounds__(SCAN_T) void peak_scan_kernel(const PeakArgs a) {
    __shared__ unsigned wt[2][SCAN_W];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned carry = 0;
    int it = 0;
    for (int base = 0; base < a.nseg; base += SCAN_T, it ^= 1) {
        const int i = base + tid;
        const unsigned c = i < a.nseg ? a.count[i] : 0u;
        unsigned inc = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wt[it][w] = inc;
        __syncthreads();
        unsigned before = 0, all = 0;
#pragma unroll
        for (int j = 0; j < SCAN_W; ++j) {
            const unsigned t = wt[it][j];
            all += t;
            if (j < w) before += t;
        }
        if (i < a.nseg) a.offset[i] = carry + before + (inc - c);
        carry += all;
    }
    if (tid == 0) *a.total = (long long)carry;
}

// the row of the peak at (ix, iy): plain sequential float64 sums over its neighbourhood, row by row
__device__ void peak_row(const PeakArgs& a, const int ix, const int iy, const float fs, double* __restrict__ out) {
    const Hood h = hood_of(a, ix, iy);
    const size_t MW = (size_t)a.MW, p = (size_t)iy * MW + (size_t)ix;
    double sum = 0.0, sw = 0.0, swx = 0.0, swy = 0.0;
    unsigned npix = 0, nabove = 0;
    for (int qy = h.y0; qy <= h.y1; ++qy) {
        const float* __restrict__ mrow = a.map + (size_t)qy * MW;
        const float* __restrict__ rrow = a.rms + (size_t)qy * MW;
        const double dy = (double)(qy - iy);
        for (int qx = h.x0; qx <= h.x1; ++qx) {
            const float uq = fs * mrow[qx];
            if (!valid_px(uq)) continue;
            const double du = (double)uq, wq = du > 0.0 ? du : 0.0;
            ++npix;
            sum += du; sw += wq; swx += wq * (double)(qx - ix); swy += wq * dy;
            if (above_px(uq, rrow[qx], a.k_sigma)) ++nabove;
        }
    }
    const float v = a.map[p], r = a.rms[p];
    out[0] = (double)ix; out[1] = (double)iy; out[2] = (double)v; out[3] = (double)r; out[4] = (double)(fs * v) / (double)r;
    out[5] = (double)npix; out[6] = (double)nabove; out[7] = sum; out[8] = sw; out[9] = swx; out[10] = swy; out[11] = 0.0;
}

__global__ __launch_bounds__(PK_T) void peak_fill_kernel(const PeakArgs a) {
    __shared__ unsigned wc[2][PK_W];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float fs = (float)a.sign;
    const unsigned cap = (unsigned)a.cap;
    const unsigned long long below = (1ULL << lane) - 1ULL;
    int it = 0;
    for (int seg = blockIdx.x; seg < a.nseg; seg += gridDim.x) {
        const unsigned off = a.offset[seg];
        if (a.count[seg] == 0u || off >= cap) continue;       // the same for every thread of the workgroup
        const unsigned long long* __restrict__ bw = a.bits + (size_t)seg * PEAK_SEG_WORDS + 4 * w;
        unsigned long long b[4];
        unsigned in_wave = 0, mine = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            b[t] = bw[t];
            in_wave += (unsigned)__popcll(b[t]);
            mine += (unsigned)__popcll(b[t] & below);
        }
        if (lane == 0) wc[it][w] = in_wave;
        __syncthreads();
        unsigned rank = off + mine;
#pragma unroll
        for (int j = 0; j < PK_W; ++j)
            if (j < w) rank += wc[it][j];
        it ^= 1;
        const int iy = seg / a.nsx, ix = (seg - iy * a.nsx) * PEAK_SEG + 4 * tid;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (!((b[t] >> lane) & 1ULL)) continue;
            if (rank < cap && ix + t < a.MW) peak_row(a, ix + t, iy, fs, a.rows + (size_t)rank * PEAK_FIELDS);
            ++rank;
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

hipError_t launch_peaks(const PeakArgs& a, hipStream_t s) {
    // what the indexing rests on: the tables match the image, columns plus the radius fit int (plan_peaks)
    if (a.MH < 1 || a.MW < 1 || a.radius < 1 || (long long)a.nsx != ((long long)a.MW + PEAK_SEG - 1) / PEAK_SEG ||
        (long long)a.nsx * PEAK_SEG + a.radius > 2147483647LL || (long long)a.nseg != (long long)a.MH * a.nsx || (long long)a.nseg > PEAK_MAX_SEG ||
        !a.map || !a.rms || !a.count || !a.offset || !a.bits || !a.total || a.cap < 0 || (a.cap > 0 && !a.rows))
        return hipErrorInvalidValue;
    const bool vec = a.MW % 4 == 0 && aligned16(a.map) && aligned16(a.rms);
    const dim3 grid(a.nseg < PK_GRID_MAX ? a.nseg : PK_GRID_MAX);
    if (vec) hipLaunchKernelGGL(peak_count_kernel<true>, grid, dim3(PK_T), 0, s, a);
    else hipLaunchKernelGGL(peak_count_kernel<false>, grid, dim3(PK_T), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(peak_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess || a.cap == 0) return e;
    hipLaunchKernelGGL(peak_fill_kernel, grid, dim3(PK_T), 0, s, a);
    return hipGetLastError();
}

}  // namespace cy
