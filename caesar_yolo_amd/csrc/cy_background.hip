// Background and noise mesh (cy_measure_background, cy_expand_background) on the HBM-resident fp32 mosaic as cy_mosaic_prepare
// leaves it.  The image is cut into cells of `cell` x `cell` pixels (edge cells may be partial); per cell
//   n0         valid pixels (value != 0 and finite)
//   bkg, rms   exact median and 1.4826 x the exact median of |v - bkg| (float64, the rule of measure_kernel) of the pixels that
//              survive `niter` clips at bkg +- k * rms; n their count, [L, H] the interval they were restricted to, rounds the
//              number of clips that removed a pixel
// background_kernel: one workgroup of 512 threads owns one cell from start to finish; no workgroup waits on another.  The clipped
// sets are nested, so every one of them is "the cell's valid pixels inside [L, H]" and no list of survivors is kept: each pass
// walks the whole cell and tests the interval.  Two forms of the walk:
//   LDS   cells of up to BKG_LDS_MAX = 128 x 128 pixels are copied once into dynamic LDS (4 bytes per pixel, blank = 0) and every
//         pass reads them from there;
//   L2    a larger cell (up to 4096 x 4096) is re-read from the image in every pass, 64-bit pixel offsets, four loads in flight
//         per lane.
// Medians are the exact radix selections of cy_select.h, the ones of measure_kernel: the cell hands them its valid pixels inside
// [L, H].  n == stop_at ends a selection after its counting pass: a clip that removed nothing needs no new median.
// Every loop is bounded before it starts: niter <= 32 clips, 4 or 8 passes, cell pixels / 512 steps per pass.  A clip that removes
// nothing ends the loop (the fixed point: the next clip would form the same lo and hi).  Counts, selections and single rounded
// operations only: nothing depends on the order in which pixels are visited.  The LDS atomics are integer counts.
// background_expand_kernel: the filled mesh [ncy][ncx][2] float64 sampled bilinearly at every pixel centre (the expression of
// measure.sample_mesh, float64, each operation rounded on its own), stored as fp32; consecutive lanes write consecutive ix.
#include "cy_px.h"                      // valid_px
#include "cy_select.h"                  // SelSmem, select_median

#pragma clang fp contract(off)          // m * (1 - f) is rounded before it is added, as the float64 definition does

namespace cy {
namespace {

constexpr int BNT = 512, BUNROLL = 4;

struct BSmem {
    SelSmem<BNT> sel;
};

struct Cell {
    const float* img;                   // first pixel of the cell in the image (L2 form)
    const float* lds;                   // the cell's pixels, row-major, cw per row (LDS form)
    size_t MW;
    unsigned cw, n;                     // width and pixel count of the cell
    double L, H;                        // current interval
};

// f(v) for every valid pixel of the cell inside [L, H]; an out-of-range slot reads as 0 = blank
template <bool LDS, typename F>
__device__ __forceinline__ void cell_for_each(const Cell& c, F f) {
    for (unsigned i0 = threadIdx.x; i0 < c.n; i0 += BUNROLL * BNT) {
        float v[BUNROLL];
#pragma unroll
        for (int u = 0; u < BUNROLL; ++u) {
            const unsigned i = i0 + u * BNT;
            if constexpr (LDS) v[u] = i < c.n ? c.lds[i] : 0.0f;
            else v[u] = i < c.n ? c.img[(size_t)(i / c.cw) * c.MW + (size_t)(i % c.cw)] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < BUNROLL; ++u) {
            const double d = (double)v[u];
            if (valid_px(v[u]) && d >= c.L && d <= c.H) f(v[u]);
        }
    }
}

template <bool LDS>
__global__ __launch_bounds__(BNT) void background_kernel(const BackgroundArgs a) {
    __shared__ BSmem s;
    extern __shared__ float cell_px[];                      // LDS form: cell * cell floats
    const int tid = threadIdx.x;
    const int cy_ = (int)(blockIdx.x / (unsigned)a.ncx), cx_ = (int)(blockIdx.x % (unsigned)a.ncx);
    if (cy_ >= a.ncy) return;                               // uniform; the grid is ncy * ncx
    // the cell's inclusive pixel range, clipped to the image: no index below can leave it
    const int x0 = cx_ * a.cell, y0 = cy_ * a.cell;
    const int x1 = min(a.MW, x0 + a.cell) - 1, y1 = min(a.MH, y0 + a.cell) - 1;
    double* out = a.out + (size_t)blockIdx.x * BKG_FIELDS;
    Cell c;
    c.MW = (size_t)a.MW;
    c.img = a.img + (size_t)y0 * c.MW + (size_t)x0;
    c.lds = cell_px;
    c.cw = (unsigned)(x1 - x0 + 1);
    c.n = c.cw * (unsigned)(y1 - y0 + 1);                   // <= 4096^2 = 2^24
    c.L = -INFINITY; c.H = INFINITY;
    if constexpr (LDS) {
        for (unsigned i = tid; i < c.n; i += BNT) cell_px[i] = c.img[(size_t)(i / c.cw) * c.MW + (size_t)(i % c.cw)];
        __syncthreads();
    }

    unsigned n0 = 0, n = 0, n2 = 0, rounds = 0;
    const auto cell = [&](auto f) { cell_for_each<LDS>(c, f); };       // c.L and c.H as they are at the call
    double med = select_median<0, BNT>(s.sel, cell, 0.0, 0xFFFFFFFFu, n0), sig = 0.0;
    n = n0;
    if (n) sig = 1.4826 * select_median<1, BNT>(s.sel, cell, med, 0xFFFFFFFFu, n2);
    for (int j = 0; j < a.niter && n; ++j) {                // n, and with it every branch below, is the same in every thread
        const double d = a.k * sig, lo = med - d, hi = med + d;
        c.L = fmax(c.L, lo); c.H = fmin(c.H, hi);
        const double m2 = select_median<0, BNT>(s.sel, cell, 0.0, n, n2);
        if (n2 == n) break;                                 // nothing removed: the fixed point
        ++rounds; n = n2; med = m2; sig = 0.0;
        if (n) sig = 1.4826 * select_median<1, BNT>(s.sel, cell, med, 0xFFFFFFFFu, n2);
    }
    if (tid == 0) {
        out[0] = (double)n0; out[1] = (double)n; out[2] = med; out[3] = sig;
        out[4] = c.L; out[5] = c.H; out[6] = (double)rounds; out[7] = 0.0;
    }
}

// t, clamped to [0, nc - 1] -> lower cell index and fraction (measure.sample_mesh)
__device__ __forceinline__ void mesh_coord(int i, int cell, int nc, int& i0, double& f) {
    if (nc == 1) { i0 = 0; f = 0.0; return; }
    double t = ((double)i - (double)(cell - 1) / 2.0) / (double)cell;
    t = t < 0.0 ? 0.0 : t;
    t = t > (double)(nc - 1) ? (double)(nc - 1) : t;
    i0 = min((int)floor(t), nc - 2);
    f = t - (double)i0;
}

__global__ __launch_bounds__(256) void background_expand_kernel(const BackgroundExpandArgs a) {
    const unsigned segs = (unsigned)((a.MW + 255) / 256);
    const int iy = (int)(blockIdx.x / segs), ix = (int)(blockIdx.x % segs) * 256 + (int)threadIdx.x;
    if (iy >= a.MH || ix >= a.MW) return;
    int cx0, cy0;
    double fx, fy;
    mesh_coord(ix, a.cell, a.ncx, cx0, fx);
    mesh_coord(iy, a.cell, a.ncy, cy0, fy);
    const int cx1 = min(cx0 + 1, a.ncx - 1), cy1 = min(cy0 + 1, a.ncy - 1);
    const double* m00 = a.mesh + ((size_t)cy0 * a.ncx + cx0) * 2;
    const double* m01 = a.mesh + ((size_t)cy0 * a.ncx + cx1) * 2;
    const double* m10 = a.mesh + ((size_t)cy1 * a.ncx + cx0) * 2;
    const double* m11 = a.mesh + ((size_t)cy1 * a.ncx + cx1) * 2;
    const double gx = 1.0 - fx, gy = 1.0 - fy;
    const size_t o = (size_t)iy * (size_t)a.MW + (size_t)ix;
    if (a.bkg) a.bkg[o] = (float)((m00[0] * gx + m01[0] * fx) * gy + (m10[0] * gx + m11[0] * fx) * fy);
    if (a.rms) a.rms[o] = (float)((m00[1] * gx + m01[1] * fx) * gy + (m10[1] * gx + m11[1] * fx) * fy);
}

}  // namespace

hipError_t launch_background(const BackgroundArgs& a, hipStream_t s) {
    if (a.MH < 1 || a.MW < 1 || a.cell < BKG_CELL_MIN || a.cell > BKG_CELL_MAX || a.ncx != (a.MW + a.cell - 1) / a.cell ||
        a.ncy != (a.MH + a.cell - 1) / a.cell || a.niter < 0 || a.niter > BKG_NITER_MAX)
        return hipErrorInvalidValue;
    const long long cells = (long long)a.ncy * a.ncx;       // < 2^31 / 16
    if ((long long)a.cell * a.cell <= BKG_LDS_MAX) {
        const size_t lds = (size_t)a.cell * a.cell * sizeof(float);
        return launch_lds<background_kernel<true>>(dim3((unsigned)cells), dim3(BNT), lds, BKG_LDS_MAX * sizeof(float), s, a);
    } else {
        hipLaunchKernelGGL(background_kernel<false>, dim3((unsigned)cells), dim3(BNT), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_background_expand(const BackgroundExpandArgs& a, hipStream_t s) {
    if (a.MH < 1 || a.MW < 1 || a.ncx < 1 || a.ncy < 1 || a.cell < BKG_CELL_MIN || a.cell > BKG_CELL_MAX || (!a.bkg && !a.rms))
        return hipErrorInvalidValue;
    const long long blocks = (long long)((a.MW + 255) / 256) * a.MH;       // <= MH * MW < 2^31
    hipLaunchKernelGGL(background_expand_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace cy
