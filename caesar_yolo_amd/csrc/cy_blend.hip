// Joint fits of blends (cy_fit_blends): the sum of M <= BLEND_MAX_MEMBERS elliptical Gaussians fitted to the union of the basins of
// a group of touching components, unweighted Levenberg-Marquardt in float64 (definitions: include/caesar_yolo_hip.h, DESIGN.md
// "Joint fits of blends").
// The model, the sums, the step, the ownership of the sums and the covariance blocks are those of cy_lm_multi.h, which the joint fit
// of a group of peaks (cy_peakgroup.hip) shares; this file states where the list comes from.
// One workgroup of 256 threads owns one job of the job table from start to finish; no workgroup reads what another one wrote.  The
// job's pixels arrive as a list of window indices in increasing order, built by the runtime from the mask: the kernel never searches
// a window.  A list entry whose pixel is not valid (0 or non-finite) keeps its list position and contributes nothing (its w is 0).
// A job of at most FIT_LDS_MAX list entries keeps {value, index} of every entry in LDS, a larger one re-reads list and image, which
// L2 serves from the second sweep on.
// Every loop has a bound fixed before it starts:
//   iteration   it = 1 .. max_iter (<= FIT_MAX_ITER = 256); every lambda escalation is one iteration, so there is no inner loop
//   sweeps      at most max_iter + 1 per job; chunks ceil(npos / 128), npos <= 2^24; per chunk <= 128 entries, M <= 4 members each
//   pair, thread 0's algebra   as cy_lm_multi.h lists them
#include "cy_lm_multi.h"                // the multi-Gaussian sweep, solve, loop and covariance blocks; cy_lm.h: stage_list

#pragma clang fp contract(off)          // every product is rounded before it is added, as the float64 definition does

namespace cy {
namespace {

constexpr int BL_T = ML_T;

struct BSmem {
    float val[FIT_LDS_MAX];
    unsigned idx[FIT_LDS_MAX];
    MultiSmem m;                        // the chunk rows, the sums, the factor and the parameters (cy_lm_multi.h)
    RedSlots<BL_T, 1> cnt;              // stage_list's
};

// a row of a job that was not fitted (status 3, 4): the start as given; the runtime restores the centres' exact bits
__device__ __forceinline__ void early_rows(const BlendJob& j, const BlendArgs& a, const int status, const unsigned np) {
    const int tid = threadIdx.x;
    if (tid >= j.M * BLEND_FIELDS) return;
    const int t = tid / BLEND_FIELDS, f = tid - t * BLEND_FIELDS;
    double v = 0.0;
    if (f == 0) v = (double)status;
    else if (f == 2) v = (double)np;
    else if (f == 5) v = (double)j.comp[0];
    else if (f == 6) v = (double)j.M;
    else if (f == 7) v = (double)t;
    else if (f >= 8 && f < 14) v = j.p0[6 * t + f - 8];
    a.out[((size_t)j.row0 + j.comp[t]) * BLEND_FIELDS + f] = v;
}

template <bool LDS>
__device__ void fit(BSmem& s, const BlendJob& j, const BlendArgs& a) {
    const int tid = threadIdx.x;
    const size_t MW = (size_t)a.MW;
    const float* __restrict__ img = a.img + (size_t)j.y0 * MW + (size_t)j.x0;
    const unsigned* __restrict__ list = a.list + j.list_off;
    const unsigned W = j.W, A = j.A, npos = j.npos;
    const int M = j.M, P = 6 * M;
    const double bkg = j.bkg;
    MultiSmem& m = s.m;

    if (tid < P) { m.p[tid] = j.p0[tid]; m.pt[tid] = j.p0[tid]; }
    if (tid == 0) { m.ctl.act = ACT_NONE; m.ctl.stop = 0; }
    const unsigned np = stage_list<BL_T, LDS>(s.val, s.idx, s.cnt, list, npos, img, MW, W, A);       // the barrier is inside

    const int early = !admissible_all(j.p0, M) ? 4 : np < (unsigned)(P + 1) ? 3 : 0;     // uniform
    if (early) { early_rows(j, a, early, np); return; }

    // list entry q -> its window index (or LM_BAD) and the datum
    const auto entry = [&](const unsigned q, double& y) {
        unsigned i; float fv;
        if (LDS) { i = s.idx[q]; fv = s.val[q]; }
        else i = list_pixel(list, q, img, MW, W, A, fv);
        y = (double)fv - bkg;
        return i;
    };
    const MultiSums u = multi_sums(P);
    double lam;
    int status, niter;
    multi_iterate(m, M, u.nsum, a.max_iter, lam, status, niter, [&](const double* pp) { multi_sweep(m, pp, M, npos, W, u, entry); });
    if (tid != 0) return;
    const bool cov = multi_inverse(m, P);
    for (int t = 0; t < M; ++t) multi_row(m, P, M, t, cov, status, niter, np, lam, j.comp[0], a.out + ((size_t)j.row0 + j.comp[t]) * BLEND_FIELDS);
}

__global__ __launch_bounds__(BL_T) void blend_kernel(const BlendArgs a) {
    __shared__ BSmem s;
    const BlendJob j = a.jobs[blockIdx.x];
    // the runtime's jobs are inside the image, their rows inside the output and their lists inside the list buffer; checked again
    // so that no index can leave a buffer whatever arrives here.  cy_fit_blends cannot produce such a job; should it ever happen,
    // nothing is fitted and nothing is written
    bool ok = j.M >= 2 && j.M <= BLEND_MAX_MEMBERS && j.row0 >= 0 && j.row0 % DBL_MAX_COMP == 0 && j.row0 + DBL_MAX_COMP <= a.nrows;
    for (int t = 0; ok && t < j.M; ++t) ok = j.comp[t] >= 0 && j.comp[t] < DBL_MAX_COMP && (t == 0 || j.comp[t] > j.comp[t - 1]);
    ok = ok && j.x0 >= 0 && j.y0 >= 0 && j.W >= 1 && j.A >= j.W && j.A % j.W == 0 && (long long)j.A <= FIT_MAX_AREA &&
         (long long)j.x0 + j.W <= a.MW && (long long)j.y0 + j.A / j.W <= a.MH && j.list_off >= 0 && j.npos <= j.A &&
         j.list_off + (long long)j.npos <= a.nlist;
    if (!ok) return;
    if (j.npos <= (unsigned)FIT_LDS_MAX) fit<true>(s, j, a);
    else fit<false>(s, j, a);
}

}  // namespace

hipError_t launch_blend(const BlendArgs& a, hipStream_t s) {
    if (a.njobs < 1 || a.MH < 1 || a.MW < 1 || a.max_iter < 1 || a.max_iter > FIT_MAX_ITER) return hipErrorInvalidValue;
    hipLaunchKernelGGL(blend_kernel, dim3(a.njobs), dim3(BL_T), 0, s, a);
    return hipGetLastError();
}

}  // namespace cy
