// Model and residual maps (cy_render_gaussians) and the residual of every source (cy_measure_residuals); definitions:
// include/caesar_yolo_hip.h, DESIGN.md "Model and residual maps".
//   render_kernel          model(ix, iy) = sum over the contributing components k, in increasing k, of A_k exp(-q_k / 2) with
//                          q = (a*u)*u + ((2*b)*u)*v + (c*v)*v, u = ix - x0, v = iy - y0: the model and the expression of cy_fit.hip, in
//                          image pixels.  A component contributes inside its support rectangle, which the host decided, and nowhere else
//   residual_stats_kernel  counts, sums, largest |r| and model sum of r = (v - bkg) - model over a box window and over its island set
// render_kernel: one workgroup of 256 threads per 32 x 32 tile of the image, every tile (an empty one writes zeros), so that both maps
// are written in one pass; a grid of at most RND_GRID_MAX workgroups walks the tiles with the grid's stride.  Thread t owns the 4
// consecutive pixels 4 (t mod 8) .. 4 (t mod 8) + 3 of row t / 8.  The host's CSR table lists, per tile, the rendered components
// whose rectangle meets it, in increasing index; they pass through LDS in chunks of RND_CHUNK = 64 (thread j < 64 loads entry j: six
// float64 and the rectangle, 64 bytes), with a barrier on each side of the refill.  Every thread adds the chunk's components in list
// order to its four float64 accumulators and tests its own pixels against the rectangle: one plain sequential sum per pixel, so the
// bits do not depend on the tiling.  All lanes read the same LDS entry at a time (a broadcast).  No atomics, and no workgroup reads
// what another one wrote.  When MW % 4 == 0 and the pointers in use (the outputs; with a residual also the image and the background)
// are 16-byte aligned the four pixels move as one 16-byte access (a quad is then inside the row or outside it); otherwise pixel
// by pixel.  Partial edge tiles: a pixel at or beyond MW / MH is neither read nor written.
// residual_stats_kernel: one workgroup of 256 threads per source, modelled on the sums of cy_islands.hip: float64 per lane over
// increasing window index (pixel i on thread i mod 256), then the block reduction of cy_reduce.h, finished by thread 0.  The largest
// |r| travels with its window index as a first maximum: the smaller index wins a tie.
// Every loop has a bound fixed before it starts:
//   tiles       tile = blockIdx.x, += gridDim.x, below ntx * nty (< 2^27 for an image below 2^31 pixels)
//   chunks      over the tile's list entries, tile_off[t] .. tile_off[t + 1] (the whole table holds at most 2^27), 64 at a time
//   components  at most 64 per chunk, four pixels each
//   statistics  over the A <= 2^24 pixels of the window, 256 at a time; 6 shuffle steps and 4 waves
#include "cy_px.h"                      // valid_px, Win, window_of
#include "cy_reduce.h"                  // RedSlots, reduction
#include <cstdint>

#pragma clang fp contract(off)          // every product is rounded before it is added, as the float64 definition does

namespace cy {
namespace {

constexpr int RND_T = 256, RND_GRID_MAX = 1 << 20;
constexpr int RES_T = 256;
static_assert(RND_T == (RND_TILE / 4) * RND_TILE, "one thread per four pixels of a tile row");
static_assert(RND_CHUNK <= RND_T, "thread j loads entry j of a chunk");

struct RSmem {
    double par[RND_CHUNK][6];
    int rect[RND_CHUNK][4];
};

template <bool VEC>
__device__ __forceinline__ void render_tile(RSmem& s, const RenderArgs& a, const int tile) {
    const int tid = threadIdx.x;
    const int ty = tile / a.ntx, tx = tile - ty * a.ntx;
    const int iy = ty * RND_TILE + (tid >> 3), ix = tx * RND_TILE + (tid & 7) * 4;
    const int first = a.tile_off[tile], last = a.tile_off[tile + 1];
    const double v = (double)iy;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int base = first; base < last; base += RND_CHUNK) {
        const int cnt = min(RND_CHUNK, last - base);
        __syncthreads();                                      // the previous chunk has been read by everyone
        if (tid < cnt) {
            const int k = a.tile_list[base + tid];
#pragma unroll
            for (int f = 0; f < 6; ++f) s.par[tid][f] = a.comp[(size_t)k * 6 + f];
#pragma unroll
            for (int f = 0; f < 4; ++f) s.rect[tid][f] = a.rect[(size_t)k * 4 + f];
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const int sx0 = s.rect[j][0], sx1 = s.rect[j][1], sy0 = s.rect[j][2], sy1 = s.rect[j][3];
            if (iy < sy0 || iy > sy1 || ix + 3 < sx0 || ix > sx1) continue;
            const double A = s.par[j][0], x0 = s.par[j][1], y0 = s.par[j][2], pa = s.par[j][3], pb = s.par[j][4], pc = s.par[j][5];
            const double vv = v - y0, qv = (pc * vv) * vv;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (ix + t < sx0 || ix + t > sx1) continue;
                const double u = (double)(ix + t) - x0;
                const double q = (pa * u) * u + ((2.0 * pb) * u) * vv + qv;
                acc[t] += A * exp(-0.5 * q);
            }
        }
    }
    if (iy >= a.MH || ix >= a.MW) return;
    const size_t p = (size_t)iy * (size_t)a.MW + (size_t)ix;
    float mo[4], ro[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < 4; ++t) mo[t] = (float)acc[t];
    if (VEC) {                                                // MW % 4 == 0: the quad is inside the row
        if (a.resid) {
            const float4 pv = *reinterpret_cast<const float4*>(a.img + p);
            float4 bv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (a.bkg) bv = *reinterpret_cast<const float4*>(a.bkg + p);
            const float px[4] = {pv.x, pv.y, pv.z, pv.w}, bk[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (valid_px(px[t])) ro[t] = (float)(((double)px[t] - (a.bkg ? (double)bk[t] : 0.0)) - acc[t]);
            *reinterpret_cast<float4*>(a.resid + p) = make_float4(ro[0], ro[1], ro[2], ro[3]);
        }
        if (a.model) *reinterpret_cast<float4*>(a.model + p) = make_float4(mo[0], mo[1], mo[2], mo[3]);
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (ix + t >= a.MW) break;
            if (a.resid) {
                const float px = a.img[p + t];
                const double bk = a.bkg ? (double)a.bkg[p + t] : 0.0;
                a.resid[p + t] = valid_px(px) ? (float)(((double)px - bk) - acc[t]) : 0.0f;
            }
            if (a.model) a.model[p + t] = mo[t];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(RND_T) void render_kernel(const RenderArgs a) {
    __shared__ RSmem s;
    const int ntiles = a.ntx * a.nty;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) render_tile<VEC>(s, a, tile);
}

__global__ __launch_bounds__(RES_T) void residual_stats_kernel(const ResidualArgs a) {
    __shared__ RedSlots<RES_T, 9> s;
    const int b = blockIdx.x, tid = threadIdx.x;
    Win wn;
    const long long area = window_of(a.win + (size_t)b * 4, a.MW, a.MH, wn);      // held inside the image (cy_px.h)
    double* out = a.out + (size_t)b * RES_FIELDS;
    const bool large = area > ISL_MAX_AREA || a.off[(size_t)b * 2] == ISL_OFF_TOO_LARGE;
    if (area == 0 || large) {                                 // empty: nothing to measure.  Above the supported maximum: status 1
        if (tid < RES_FIELDS) out[tid] = tid == 0 ? (large && area ? 1.0 : 0.0) : (tid == 8 || tid == 9) ? -1.0 : 0.0;
        return;
    }
    const int bx0 = wn.x0, by0 = wn.y0;
    const unsigned W = wn.W, A = wn.A;
    const size_t MW = (size_t)a.MW, org = (size_t)by0 * MW + (size_t)bx0;
    const unsigned char* __restrict__ mask = a.mask + a.off[(size_t)b * 2 + 1];
    const double bkg = a.bkg[b];
    double Sw = 0.0, Qw = 0.0, Si = 0.0, Qi = 0.0, Mi = 0.0, best = -1.0;
    unsigned nw = 0, ni = 0, bi = 0xFFFFFFFFu;
    for (unsigned i = tid; i < A; i += RES_T) {
        const unsigned dy = i / W, dx = i - dy * W;
        const size_t p = org + (size_t)dy * MW + dx;
        const float px = a.img[p];
        if (!valid_px(px)) continue;
        const double md = (double)a.model[p], r = ((double)px - bkg) - md, rr = r * r;
        ++nw; Sw += r; Qw += rr;
        if (mask[i]) {
            ++ni; Si += r; Qi += rr; Mi += md;
            const double ar = fabs(r);
            if (ar > best) { best = ar; bi = i; }             // i increases: the first occurrence stays
        }
    }
    const auto red = reduction(red_sum(Sw), red_sum(Qw), red_sum(Si), red_sum(Qi), red_sum(Mi), red_sum(nw), red_sum(ni),
                               red_first_max(best, bi, 0xFFFFFFFFu));
    red.wave();
    red.park(s);
    __syncthreads();
    if (tid == 0) {
        red.total(s);
        const bool has = ni > 0 && bi < A;
        out[0] = 0.0; out[1] = (double)nw; out[2] = (double)ni; out[3] = Sw; out[4] = Qw; out[5] = Si; out[6] = Qi;
        out[7] = has ? best : 0.0;
        out[8] = has ? (double)(bx0 + (int)(bi % W)) : -1.0; out[9] = has ? (double)(by0 + (int)(bi / W)) : -1.0;
        out[10] = Mi; out[11] = 0.0;
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

hipError_t launch_render(const RenderArgs& a, hipStream_t s) {
    if (a.MH < 1 || a.MW < 1 || !a.img || (!a.model && !a.resid) || a.ntx != (a.MW + RND_TILE - 1) / RND_TILE ||
        a.nty != (a.MH + RND_TILE - 1) / RND_TILE || (long long)a.MH * a.MW >= (1LL << 31))
        return hipErrorInvalidValue;
    const int ntiles = a.ntx * a.nty;
    // the image and the background are read for the residual only; a null pointer counts as aligned
    const bool vec = a.MW % 4 == 0 && aligned16(a.model) && aligned16(a.resid) && (!a.resid || (aligned16(a.img) && aligned16(a.bkg)));
    const dim3 grid(ntiles < RND_GRID_MAX ? ntiles : RND_GRID_MAX);
    if (vec) hipLaunchKernelGGL(render_kernel<true>, grid, dim3(RND_T), 0, s, a);
    else hipLaunchKernelGGL(render_kernel<false>, grid, dim3(RND_T), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_residual_stats(const ResidualArgs& a, hipStream_t s) {
    if (a.n < 1 || a.MH < 1 || a.MW < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(residual_stats_kernel, dim3(a.n), dim3(RES_T), 0, s, a);
    return hipGetLastError();
}

}  // namespace cy
