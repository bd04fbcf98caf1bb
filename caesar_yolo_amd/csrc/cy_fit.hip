// Component fits (cy_fit_components): one elliptical Gaussian per deblended component, unweighted Levenberg-Marquardt in float64
// (definitions: include/caesar_yolo_hip.h, DESIGN.md "Component fits").
//   model    m = A exp(-(a u^2 + 2 b u v + c v^2) / 2), u = dx - x0, v = dy - y0; p = (A, x0, y0, a, b, c), x0 / y0 relative to the
//            window's first pixel in here (the runtime converts from and to image pixels)
//   sweep    F = sum r^2, g = J^T r, H = J^T J (upper triangle) at one p over the job's pixels: FIT_NSUM = 28 float64 sums
//   step     thread 0: 6 x 6 Cholesky of H + lambda diag(H), d, `small`, admissibility of p + d; everyone: sweep at the trial;
//            thread 0: accept / reject, lambda, convergence: lm_iterate of cy_lm.h, which states the rule and owns the loop
// The Gaussian and its Jacobian (gauss_terms), the staging of the list (list_pixel, stage_list), the place of H in the sums (hidx)
// and the 6 x 6 solve (lm_solve) are in cy_lm.h as well: the fit of a peak at a position (cy_peakfit.hip) uses them too.
// One workgroup of 256 threads owns one job of the job table from start to finish; no workgroup reads what another one wrote.
// The job's pixels arrive as a list of window indices i = dy * W + dx in increasing order, built by the runtime from the mask: the
// kernel never searches a window.  A list entry whose pixel is not valid (0 or non-finite) keeps its list position and contributes
// nothing.  A job of at most FIT_LDS_MAX list entries keeps {value, index} of every entry in LDS (8 bytes per pixel, 32 KiB; with
// the reduction scratch 34 KiB per workgroup: the 160 KiB of a CU would hold four); a larger one re-reads list and
// image, which L2 serves from the second sweep on.
// Registers: 28 float64 accumulators are 56 VGPRs per lane; with the six Jacobian entries, exp's temporaries and thread 0's 6 x 6
// factor the build reports 176 VGPRs and no spill (the 96 bytes of scratch hold the job record, read once).  Of the 512 registers
// per lane of a SIMD that leaves two waves per SIMD, so two workgroups (68 KiB of LDS) are resident per CU.  Holding the kernel
// to 128 VGPRs for four waves spills 25 registers and was not kept.
// Every loop has a bound fixed before it starts:
//   iteration   it = 1 .. max_iter (<= FIT_MAX_ITER = 256); every lambda escalation is one iteration, so there is no inner loop
//   sweeps      over the npos list entries of the job, npos <= 2^24; at most max_iter + 1 sweeps per job
//   reductions  6 shuffle steps and FIT_T / 64 = 4 waves;  Cholesky and the two triangular solves: 6 x 6, fully unrolled
// Sums: float64 per lane over increasing list position (entry q belongs to thread q mod 256), then the block reduction of
// cy_reduce.h, finished by thread 0.  No atomics.
#include "cy_lm.h"                      // gauss_terms, stage_list, hidx, lm_solve, lm_iterate

#pragma clang fp contract(off)          // every product is rounded before it is added, as the float64 definition does

namespace cy {
namespace {

constexpr int FIT_T = 256;

struct FSmem {
    float val[FIT_LDS_MAX];
    unsigned idx[FIT_LDS_MAX];
    RedSlots<FIT_T, FIT_NSUM> red;      // sweep's
    double tot[FIT_NSUM];               // sums of the last sweep
    double cur[FIT_NSUM];               // sums at the accepted p
    double p[6], pt[6];                 // accepted and trial parameters
    RedSlots<FIT_T, 1> cnt;             // stage_list's
    LmCtl ctl;
};

// F, g, H at pp (LDS, uniform) over the job's list; the totals land in s.tot (valid for thread 0 after the barrier inside)
template <bool LDS>
__device__ __forceinline__ void sweep(FSmem& s, const double* pp, const unsigned* __restrict__ list, const unsigned npos,
                                      const float* __restrict__ img, const size_t MW, const unsigned W, const unsigned A, const double bkg) {
    const int tid = threadIdx.x;
    const double pA = pp[0], x0 = pp[1], y0 = pp[2], a = pp[3], b = pp[4], c = pp[5];
    double acc[FIT_NSUM];
#pragma unroll
    for (int k = 0; k < FIT_NSUM; ++k) acc[k] = 0.0;
    for (unsigned q = tid; q < npos; q += FIT_T) {
        unsigned i; float fv;
        if (LDS) { i = s.idx[q]; fv = s.val[q]; }
        else i = list_pixel(list, q, img, MW, W, A, fv);
        if (i == LM_BAD) continue;
        const unsigned dy = i / W, dx = i - dy * W;
        double J[6];
        const double y = (double)fv - bkg, r = y - gauss_terms(pA, x0, y0, a, b, c, (double)dx, (double)dy, J);
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
__device__ void fit(FSmem& s, const FitJob& j, const FitArgs& a, double* __restrict__ out) {
    const int tid = threadIdx.x;
    const size_t MW = (size_t)a.MW;
    const float* __restrict__ img = a.img + (size_t)j.y0 * MW + (size_t)j.x0;
    const unsigned* __restrict__ list = a.list + j.list_off;
    const unsigned W = j.W, A = j.A, npos = j.npos;
    const double bkg = j.bkg;

    if (tid < 6) { s.p[tid] = j.p0[tid]; s.pt[tid] = j.p0[tid]; }
    if (tid == 0) { s.ctl.act = ACT_NONE; s.ctl.stop = 0; }
    const unsigned np = stage_list<FIT_T, LDS>(s.val, s.idx, s.cnt, list, npos, img, MW, W, A);      // the barrier is inside

    const int early = !admissible(j.p0) ? 4 : np < (unsigned)FIT_MIN_PIX ? 3 : 0;     // uniform
    if (early) {
        if (tid < FIT_FIELDS) out[tid] = tid == 0 ? (double)early : tid == 2 ? (double)np : tid >= 5 && tid < 11 ? s.p[tid - 5] : 0.0;
        return;
    }

    // ---- sums at the start
    sweep<LDS>(s, s.pt, list, npos, img, MW, W, A, bkg);
    if (tid == 0)
        for (int k = 0; k < FIT_NSUM; ++k) s.cur[k] = s.tot[k];
    double lam;
    int status, niter;
    lm_iterate(s.ctl, a.max_iter, lam, status, niter,
               [&](const double lam, bool& small) {
                   double d[6], pn[6];
                   if (!lm_solve(s.cur, lam, d)) return false;
                   small = lm_trial(6, s.p, d, pn);
                   if (!admissible(pn)) return false;
#pragma unroll
                   for (int k = 0; k < 6; ++k) s.pt[k] = pn[k];
                   return true;
               },
               [&] { sweep<LDS>(s, s.pt, list, npos, img, MW, W, A, bkg); },
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
    }
}

__global__ __launch_bounds__(FIT_T) void fit_kernel(const FitArgs a) {
    __shared__ FSmem s;
    const FitJob j = a.jobs[blockIdx.x];
    const int tid = threadIdx.x;
    // the runtime's jobs are inside the image, their rows inside the output and their lists inside the list buffer; checked again
    // so that no index can leave a buffer whatever arrives here.  cy_fit_components cannot produce such a job; should it ever
    // happen, nothing is fitted and, where the row itself is inside the output, it is NaN throughout
    const bool rowok = j.row >= 0 && j.row < a.nrows;
    const bool ok = rowok && j.x0 >= 0 && j.y0 >= 0 && j.W >= 1 && j.A >= j.W && j.A % j.W == 0 && (long long)j.A <= FIT_MAX_AREA &&
                    (long long)j.x0 + j.W <= a.MW && (long long)j.y0 + j.A / j.W <= a.MH && j.list_off >= 0 && j.npos <= j.A &&
                    j.list_off + (long long)j.npos <= a.nlist;
    if (!ok) {
        if (rowok && tid < FIT_FIELDS) a.out[(size_t)j.row * FIT_FIELDS + tid] = __longlong_as_double(0x7FF8000000000000LL);
        return;
    }
    double* out = a.out + (size_t)j.row * FIT_FIELDS;
    if (j.npos <= (unsigned)FIT_LDS_MAX) fit<true>(s, j, a, out);
    else fit<false>(s, j, a, out);
}

}  // namespace

hipError_t launch_fit(const FitArgs& a, hipStream_t s) {
    if (a.njobs < 1 || a.MH < 1 || a.MW < 1 || a.max_iter < 1 || a.max_iter > FIT_MAX_ITER) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fit_kernel, dim3(a.njobs), dim3(FIT_T), 0, s, a);
    return hipGetLastError();
}

}  // namespace cy
