// Gaussian fits at given positions (cy_fit_peaks): one elliptical Gaussian per job on the pixels of a disc around the job's centre,
// unweighted Levenberg-Marquardt in float64 (definitions: include/caesar_yolo_hip.h, DESIGN.md "Peak fits").
//   model, sums, step   those of the component fit (cy_fit.hip): gauss_terms, the 28 sums F, g, H, lm_solve and lm_iterate of cy_lm.h
//   data                y = sign * ((double)v - bkg): a hole is fitted as the peak of the negated map
//   pixel set           decided here, not on the host: window pixel (qx, qy) is a member of job e when d2_e = (qx - cx_e)^2 +
//                       (qy - cy_e)^2 <= R_e^2 and d2_f >= d2_e for each of the job's at most 8 kept neighbours f (a pixel goes to
//                       the nearest centre; a tie belongs to both).  Distances in image coordinates, two products and one sum,
//                       not contracted.  The neighbours' centres are read from the job table by their indices: the addresses
//                       depend on the job record alone, so they are uniform over the workgroup (scalar loads)
// One workgroup of 256 threads owns one fitted job from start to finish; the grid is the number of jobs the planner
// (plan_peak_fits) gave status 0, and workgroup t writes row t of a table of its own that the host deals out.  No workgroup reads
// what another one wrote; no atomics, no inline assembly, no list buffer and no mask.
// The job's list is every pixel of its window in increasing window index i = dy * W + dx, entry i on thread i mod 256; a pixel
// that is not a valid member (outside the disc, taken by a neighbour, 0 or not finite) keeps its position and contributes nothing.
// A window of at most PFIT_LDS_MAX = 8192 pixels (R <= 44: 89 x 89 = 7921) is staged once: one fp32 per window pixel in LDS, 0.0f
// for a pixel that is not a valid member, which valid_px rejects in every sweep.  A larger window evaluates membership again from
// the map in every sweep, served by L2 from the second sweep on.  The staging pass (a counting pass for the larger windows) counts
// npix, the valid members, and nexcluded, the valid pixels of the disc that a neighbour took.
// Registers and LDS, from the compiler's report for gfx950: 218 VGPRs, 102 SGPRs, no spill, 160 bytes of scratch (the job record,
// read once), 34 280 bytes of LDS (32 KiB of staged values, the reduction slots, the sums and the parameters).  fit_kernel is the
// yardstick at 176 VGPRs and 34 KiB of LDS: both leave two waves per SIMD, so two workgroups (67 KiB of LDS) are resident per CU.
// The 28 float64 accumulators are 56 VGPRs per lane; the membership test adds the pixel's and the centres' differences on top of
// the sweep of fit_kernel; the neighbours' centres are uniform and live in SGPRs.
// Every loop has a bound fixed before it starts:
//   iteration   it = 1 .. max_iter (<= FIT_MAX_ITER = 256); every lambda escalation is one iteration, so there is no inner loop
//   sweeps      at most max_iter + 1 per job, each over the A <= 513 x 513 pixels of the window, 256 at a time; one more walk counts
//   neighbours  PFIT_NEIGH_MAX = 8 tests per pixel, unrolled
//   reductions  6 shuffle steps and PF_T / 64 = 4 waves;  Cholesky and the two triangular solves: 6 x 6, fully unrolled
// Every early return is uniform: the ones that depend on the job record alone come before any barrier; the one that needs npix
// follows the staging barrier, after which every thread holds the same count.
// Sums: float64 per lane over increasing window index, then the block reduction of cy_reduce.h, finished by thread 0: two calls
// give the same bytes.
#include "cy_lm.h"                      // gauss_terms, hidx, lm_solve, lm_trial, lm_iterate
#include "cy_disc.h"                    // Disc, member: the membership test, shared with cy_peakgroup.hip

#pragma clang fp contract(off)          // every product is rounded before it is added, as the float64 definition does

namespace cy {
namespace {

constexpr int PF_T = 256, PF_NB = DISC_NB;
constexpr int PF_SIDE_MAX = 2 * PFIT_RADIUS_MAX + 1;

struct PSmem {
    float val[PFIT_LDS_MAX];
    RedSlots<PF_T, FIT_NSUM> red;       // sweep's
    double tot[FIT_NSUM];               // sums of the last sweep
    double cur[FIT_NSUM];               // sums at the accepted p
    double p[6], pt[6];                 // accepted and trial parameters
    RedSlots<PF_T, 2> cnt;              // the staging pass's: npix, nexcluded
    LmCtl ctl;
};

// F, g, H at pp (LDS, uniform) over the window; the totals land in s.tot (valid for thread 0 after the barrier inside)
template <bool LDS>
__device__ __forceinline__ void sweep(PSmem& s, const double* pp, const Disc& d, const unsigned A, const float* __restrict__ img, const size_t MW,
                                      const double bkg, const double sign) {
    const int tid = threadIdx.x;
    const double pA = pp[0], x0 = pp[1], y0 = pp[2], a = pp[3], b = pp[4], c = pp[5];
    double acc[FIT_NSUM];
#pragma unroll
    for (int k = 0; k < FIT_NSUM; ++k) acc[k] = 0.0;
    for (unsigned q = tid; q < A; q += PF_T) {
        unsigned wx, wy; float fv;
        if (LDS) { fv = s.val[q]; wy = q / d.W; wx = q - wy * d.W; }
        else {
            bool in;
            if (!member(d, q, wx, wy, in)) continue;
            fv = img[(size_t)wy * MW + wx];
        }
        if (!valid_px(fv)) continue;
        double J[6];
        const double y = sign * ((double)fv - bkg), r = y - gauss_terms(pA, x0, y0, a, b, c, (double)wx, (double)wy, J);
        acc[0] += r * r;
#pragma unroll
        for (int ii = 0; ii < 6; ++ii) {
            acc[1 + ii] += J[ii] * r;
#pragma unroll
            for (int jj = ii; jj < 6; ++jj) acc[hidx(ii, jj)] += J[ii] * J[jj];
        }
    }
    const auto red = reduction(red_sum(acc));
    red.wave();
    red.park(s.red);                                          // the slots of the sweep before: lm_iterate's barrier follows thread 0's read
    __syncthreads();
    if (tid == 0) {
        red.total(s.red);
#pragma unroll
        for (int k = 0; k < FIT_NSUM; ++k) s.tot[k] = acc[k];
    }
}

template <bool LDS>
__device__ void fit(PSmem& s, const PeakFitJob& j, const Disc& d, const unsigned A, const PeakFitArgs& a, double* __restrict__ out) {
    const int tid = threadIdx.x;
    const size_t MW = (size_t)a.MW;
    const float* __restrict__ img = a.map + (size_t)d.by0 * MW + (size_t)d.bx0;
    const double bkg = j.bkg, sign = j.sign;

    if (tid < 6) { s.p[tid] = j.p0[tid]; s.pt[tid] = j.p0[tid]; }
    if (tid == 0) { s.ctl.act = ACT_NONE; s.ctl.stop = 0; }
    // ---- the staging pass: the members' values (LDS), npix and nexcluded
    unsigned np = 0, nex = 0;
    for (unsigned q = tid; q < A; q += PF_T) {
        unsigned wx, wy; bool in;
        const bool mine = member(d, q, wx, wy, in);
        float fv = 0.0f;
        if (in) fv = img[(size_t)wy * MW + wx];
        const bool ok = valid_px(fv);
        if (LDS) s.val[q] = mine && ok ? fv : 0.0f;
        np += mine && ok; nex += in && !mine && ok;
    }
    {
        const auto red = reduction(red_sum(np), red_sum(nex));
        red.wave();
        red.park(s.cnt);
        __syncthreads();
        red.total(s.cnt);                                     // every thread; no later park in these slots
    }
    const auto tail = [&](double* o) {                        // the fields the job record decides
        o[32] = (double)j.x0; o[33] = (double)j.x1; o[34] = (double)j.y0; o[35] = (double)j.y1;
        o[36] = (double)j.clipped; o[37] = (double)j.nneigh; o[38] = (double)j.crowded; o[39] = (double)nex;
    };
    const int early = !admissible(j.p0) ? 4 : np < (unsigned)FIT_MIN_PIX ? 3 : 0;     // uniform
    if (early) {
        if (tid == 0) {
            for (int k = 0; k < PFIT_FIELDS; ++k) out[k] = 0.0;
            out[0] = (double)early; out[2] = (double)np;
            for (int k = 0; k < 6; ++k) out[5 + k] = j.p0[k];
            tail(out);
        }
        return;
    }

    // ---- sums at the start
    sweep<LDS>(s, s.pt, d, A, img, MW, bkg, sign);
    if (tid == 0)
        for (int k = 0; k < FIT_NSUM; ++k) s.cur[k] = s.tot[k];
    double lam;
    int status, niter;
    lm_iterate(s.ctl, a.max_iter, lam, status, niter,
               [&](const double lam, bool& small) {
                   double dd[6], pn[6];
                   if (!lm_solve(s.cur, lam, dd)) return false;
                   small = lm_trial(6, s.p, dd, pn);
                   if (!admissible(pn)) return false;
#pragma unroll
                   for (int k = 0; k < 6; ++k) s.pt[k] = pn[k];
                   return true;
               },
               [&] { sweep<LDS>(s, s.pt, d, A, img, MW, bkg, sign); },
               [&] { return s.cur[0]; }, [&] { return s.tot[0]; },
               [&] {
                   for (int k = 0; k < FIT_NSUM; ++k) s.cur[k] = s.tot[k];
#pragma unroll
                   for (int k = 0; k < 6; ++k) s.p[k] = s.pt[k];
               });
    if (tid == 0) {
        out[0] = (double)status; out[1] = (double)niter; out[2] = (double)np; out[3] = s.cur[0]; out[4] = lam;
        for (int k = 0; k < 6; ++k) out[5 + k] = s.p[k];
        for (int k = 0; k < 21; ++k) out[11 + k] = s.cur[7 + k];
        tail(out);
    }
}

__global__ __launch_bounds__(PF_T) void peakfit_kernel(const PeakFitArgs a) {
    __shared__ PSmem s;
    const int tid = threadIdx.x;
    const int t = blockIdx.x;
    if (t >= a.nrun) return;                                  // the row is inside the output: the grid is nrun
    double* out = a.out + (size_t)t * PFIT_FIELDS;
    const int e = a.run[t];
    // the planner's jobs are fitted ones, their windows inside the image and their neighbours inside the table; checked again so
    // that no index can leave a buffer whatever arrives here.  cy_fit_peaks cannot produce such a job; should it ever happen,
    // nothing is fitted and the row is NaN throughout
    bool ok = e >= 0 && e < a.n;
    PeakFitJob j{};
    if (ok) {
        j = a.jobs[e];
        ok = j.status == 0 && j.x0 >= 0 && j.y0 >= 0 && j.x1 >= j.x0 && j.y1 >= j.y0 && j.x1 < a.MW && j.y1 < a.MH &&
             j.x1 - j.x0 < PF_SIDE_MAX && j.y1 - j.y0 < PF_SIDE_MAX && j.nneigh >= 0 && j.nneigh <= PF_NB;
        for (int k = 0; k < PF_NB; ++k) ok = ok && (k >= j.nneigh || (j.neigh[k] >= 0 && j.neigh[k] < a.n));
    }
    if (!ok) {                                                // uniform: the arguments and the job record only
        if (tid < PFIT_FIELDS) out[tid] = __longlong_as_double(0x7FF8000000000000LL);
        return;
    }
    Disc d;
    d.bx0 = j.x0; d.by0 = j.y0; d.W = (unsigned)(j.x1 - j.x0 + 1);
    d.cx = j.cx; d.cy = j.cy; d.r2 = j.r2; d.nn = j.nneigh;
#pragma unroll
    for (int k = 0; k < PF_NB; ++k) {
        const bool has = k < j.nneigh;
        const PeakFitJob* f = a.jobs + (has ? j.neigh[k] : e);
        d.ncx[k] = f->cx; d.ncy[k] = f->cy;                  // beyond nneigh: the job's own centre, which member() does not look at
    }
    const unsigned A = d.W * (unsigned)(j.y1 - j.y0 + 1);
    if (A <= (unsigned)PFIT_LDS_MAX) fit<true>(s, j, d, A, a, out);
    else fit<false>(s, j, d, A, a, out);
}

}  // namespace

hipError_t launch_peak_fits(const PeakFitArgs& a, hipStream_t s) {
    if (a.nrun < 1 || a.nrun > a.n || a.n > PFIT_JOBS_MAX || a.MH < 1 || a.MW < 1 || (long long)a.MH * a.MW >= (1LL << 31) || a.max_iter < 1 ||
        a.max_iter > FIT_MAX_ITER || !a.map || !a.jobs || !a.run || !a.out)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(peakfit_kernel, dim3(a.nrun), dim3(PF_T), 0, s, a);
    return hipGetLastError();
}

}  // namespace cy
