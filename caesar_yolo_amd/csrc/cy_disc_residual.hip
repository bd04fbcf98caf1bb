// What a map holds on the discs of given jobs (cy_disc_residuals): count, sum, sum of squares and largest |r| of r = (double)v - bkg
// over the pixel set of every job, and the sum of a second map over the same pixels (definitions: include/caesar_yolo_hip.h,
// DESIGN.md "Second residual").  The chain runs it on the second residual with the jobs of the peak fits: the pixel set of a job
// is exactly the set its single fit used.
//   pixel set   that of cy_peakfit.hip, by the same code (member() of cy_disc.h): window pixel (qx, qy) is a member of job e when
//               d2_e <= R_e^2 and d2_f >= d2_e for each of the job's at most 8 kept neighbours f; a tie belongs to both
//   data        r = (double)v - bkg on a valid member (non-zero and finite v): one rounded operation, no sign applied
// One workgroup of 256 threads owns one job; the grid is the number of jobs the planner (plan_peak_fits) gave status 0, and
// workgroup t writes row t of a table of its own that the host deals out (disc_residual_row).  No workgroup reads what another
// one wrote; one sweep over the window, no LDS staging, no atomics, no inline assembly.
// Window pixel i = dy * W + dx sits on thread i mod 256; the sums run sequentially per thread over increasing i, the largest |r|
// keeps its first occurrence (`>`), then the block reduction of cy_reduce.h: red_sum for the three sums and the two counts,
// red_first_max for |r| with the window index.  Two calls give the same bytes.
// Every loop has a bound fixed before it starts:
//   window      over the A <= 513 x 513 pixels of the window, 256 at a time, once
//   neighbours  PFIT_NEIGH_MAX = 8 tests per pixel, unrolled;  reductions: 6 shuffle steps and 4 waves
// Every early return is uniform and comes before the barrier: it depends on the arguments and the job record alone.
#include "cy_px.h"                      // valid_px
#include "cy_reduce.h"                  // RedSlots, reduction
#include "cy_disc.h"                    // Disc, member: the membership test of the peak fits

#pragma clang fp contract(off)          // r * r is rounded before it is added, as the float64 definition does

namespace cy {
namespace {

constexpr int DR_T = 256, DR_NB = DISC_NB;
constexpr int DR_SIDE_MAX = 2 * PFIT_RADIUS_MAX + 1;
constexpr unsigned DR_NONE = 0xFFFFFFFFu;                     // no candidate for the largest |r|: a window index stays below 2^19

__global__ __launch_bounds__(DR_T) void disc_residual_kernel(const DiscResidualArgs a) {
    __shared__ RedSlots<DR_T, 7> slots;
    const int tid = threadIdx.x;
    const int t = blockIdx.x;
    if (t >= a.nrun) return;                                  // the row is inside the output: the grid is nrun
    double* out = a.out + (size_t)t * DRES_FIELDS;
    const int e = a.run[t];
    // the planner's jobs are measured ones, their windows inside the image and their neighbours inside the table; checked again so
    // that no index can leave a buffer whatever arrives here (as peakfit_kernel does).  cy_disc_residuals cannot produce such a
    // job; should it ever happen, nothing is read and the row is NaN throughout
    bool ok = e >= 0 && e < a.n;
    PeakFitJob j{};
    if (ok) {
        j = a.jobs[e];
        ok = j.status == 0 && j.x0 >= 0 && j.y0 >= 0 && j.x1 >= j.x0 && j.y1 >= j.y0 && j.x1 < a.MW && j.y1 < a.MH &&
             j.x1 - j.x0 < DR_SIDE_MAX && j.y1 - j.y0 < DR_SIDE_MAX && j.nneigh >= 0 && j.nneigh <= DR_NB;
        for (int k = 0; k < DR_NB; ++k) ok = ok && (k >= j.nneigh || (j.neigh[k] >= 0 && j.neigh[k] < a.n));
    }
    if (!ok) {                                                // uniform: the arguments and the job record only
        if (tid < DRES_FIELDS) out[tid] = __longlong_as_double(0x7FF8000000000000LL);
        return;
    }
    Disc d;
    d.bx0 = j.x0; d.by0 = j.y0; d.W = (unsigned)(j.x1 - j.x0 + 1);
    d.cx = j.cx; d.cy = j.cy; d.r2 = j.r2; d.nn = j.nneigh;
#pragma unroll
    for (int k = 0; k < DR_NB; ++k) {
        const bool has = k < j.nneigh;
        const PeakFitJob* f = a.jobs + (has ? j.neigh[k] : e);
        d.ncx[k] = f->cx; d.ncy[k] = f->cy;                  // beyond nneigh: the job's own centre, which member() does not look at
    }
    const unsigned A = d.W * (unsigned)(j.y1 - j.y0 + 1);
    const size_t MW = (size_t)a.MW;
    const float* __restrict__ map = a.map;
    const float* __restrict__ model = a.model;
    const double bkg = j.bkg;

    double acc[3] = {0.0, 0.0, 0.0};                          // sum r, sum r * r, sum of the model
    unsigned cnt[2] = {0u, 0u};                               // npix, nexcluded
    double best = 0.0;
    unsigned bi = DR_NONE;
    for (unsigned q = tid; q < A; q += DR_T) {
        unsigned wx, wy; bool in;
        const bool mine = member(d, q, wx, wy, in);
        if (!in) continue;
        const size_t p = ((size_t)d.by0 + wy) * MW + (size_t)d.bx0 + wx;
        const float fv = map[p];
        if (!valid_px(fv)) continue;
        if (!mine) { ++cnt[1]; continue; }
        const double r = (double)fv - bkg, rr = r * r, ar = fabs(r);
        acc[0] += r; acc[1] += rr;
        if (model) acc[2] += (double)model[p];
        ++cnt[0];
        if (bi == DR_NONE || ar > best) { best = ar; bi = q; }
    }
    const auto red = reduction(red_sum(acc), red_sum(cnt), red_first_max(best, bi, DR_NONE));
    red.wave();
    red.park(slots);
    __syncthreads();
    if (tid == 0) {
        red.total(slots);
        const bool any = bi != DR_NONE;
        const unsigned my = any ? bi / d.W : 0u, mx = any ? bi - my * d.W : 0u;
        out[0] = 0.0; out[1] = (double)cnt[0]; out[2] = (double)cnt[1];
        out[3] = acc[0]; out[4] = acc[1];
        out[5] = any ? best : 0.0;
        out[6] = any ? (double)(d.bx0 + (int)mx) : -1.0; out[7] = any ? (double)(d.by0 + (int)my) : -1.0;
        out[8] = acc[2]; out[9] = 0.0;
        out[10] = (double)j.x0; out[11] = (double)j.x1; out[12] = (double)j.y0; out[13] = (double)j.y1;
        out[14] = (double)j.clipped; out[15] = (double)j.nneigh;
    }
}

}  // namespace

hipError_t launch_disc_residuals(const DiscResidualArgs& a, hipStream_t s) {
    if (a.nrun < 1 || a.nrun > a.n || a.n > PFIT_JOBS_MAX || a.MH < 1 || a.MW < 1 || (long long)a.MH * a.MW >= (1LL << 31) || !a.map || !a.jobs ||
        !a.run || !a.out)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(disc_residual_kernel, dim3(a.nrun), dim3(DR_T), 0, s, a);
    return hipGetLastError();
}

}  // namespace cy
