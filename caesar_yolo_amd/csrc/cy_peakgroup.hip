// Joint fits of groups of peaks (cy_fit_peak_groups): the sum of M <= BLEND_MAX_MEMBERS elliptical Gaussians fitted to the union of
// the discs of a group of linked peak-fit jobs, unweighted Levenberg-Marquardt in float64 (definitions: include/caesar_yolo_hip.h,
// DESIGN.md "Peak groups").
//   model, sums, step   those of the joint fit of a blend: cy_lm_multi.h (ownership by sum, the P x P algebra, the covariance blocks)
//   data                y = sign * ((double)v - bkg), bkg and sign those of the member in slot 0
//   pixel set           decided here by position (cy_disc.h): group-window pixel q belongs to the set when some member e has it inside
//                       its disc and no nearer to a kept neighbour of e that is NOT a member of the group.  Inside the group nothing
//                       is divided; jobs outside it keep their nearest-centre share
// One workgroup of 256 threads owns one group job from start to finish; the grid is the number of group jobs the planner
// (plan_peak_groups) made, and workgroup t writes the M member rows of block t of a table of its own that the host deals out.  No
// workgroup reads what another one wrote; no atomics, no inline assembly, no list buffer and no mask.
// The job's list is every pixel of the group window in increasing window index; a pixel that is not a valid member keeps its
// position and contributes nothing (its w is 0).  A window of at most PGRP_LDS_MAX = 8192 pixels is staged once: one fp32 per window
// pixel in LDS, 0.0f for a pixel that is not a valid member, which valid_px rejects in every sweep.  A larger window evaluates
// membership again from the map in every sweep.  The staging pass (a counting pass for the larger windows) counts npix, the valid
// members, and nexcluded, the valid pixels inside some member's disc that are in no member's share.
// The four discs with their eight outside neighbours each (centres as float64) live in LDS, not in registers: every lane reads the
// same word, a broadcast.  Thread e < 4 fills disc e from the job table before the first barrier.
// Every loop has a bound fixed before it starts:
//   iteration   it = 1 .. max_iter (<= FIT_MAX_ITER = 256); every lambda escalation is one iteration, so there is no inner loop
//   sweeps      at most max_iter + 1 per job, each over the A <= 2049 x 2049 pixels of the group window in chunks of 128; one more
//               walk, 256 pixels at a time, stages and counts
//   membership  M <= 4 discs per pixel, DISC_NB = 8 neighbour tests each, unrolled
//   checks      4 members x 8 neighbours of the job record
//   pair, thread 0's algebra   as cy_lm_multi.h lists them;  the counts' reduction: 6 shuffle steps and 4 waves
// Every early return is uniform: the ones that depend on the arguments and the job record alone come before any barrier; the one
// that needs npix follows the staging barrier, after which every thread holds the same count.
#include "cy_lm_multi.h"                // the multi-Gaussian sweep, solve, loop and covariance blocks
#include "cy_disc.h"                    // Disc, member

#pragma clang fp contract(off)          // every product is rounded before it is added, as the float64 definition does

namespace cy {
namespace {

constexpr int PG_T = ML_T, PG_M = BLEND_MAX_MEMBERS;
constexpr int PG_SIDE_MAX = (2 * PFIT_RADIUS_MAX + 1) + (PG_M - 1) * 2 * PFIT_RADIUS_MAX;     // a chain of four at link = 2: 2049

struct GSmem {
    float val[PGRP_LDS_MAX];
    MultiSmem m;
    Disc disc[PG_M];                    // slot e >= M: r2 = -1, a disc without a pixel
    RedSlots<PG_T, 2> cnt;              // the staging pass's: npix, nexcluded
};

// window pixel q: in some member's share (returned), inside some member's disc (in)
__device__ __forceinline__ bool group_member(const GSmem& s, const int M, const unsigned q, unsigned& wx, unsigned& wy, bool& in) {
    bool mine = false;
    in = false;
    for (int e = 0; e < M; ++e) {
        bool ie;
        const bool me = member(s.disc[e], q, wx, wy, ie);
        mine = mine || me; in = in || ie;
    }
    return mine;
}

template <bool LDS>
__device__ void fit(GSmem& s, const PeakGroupJob& g, const unsigned W, const unsigned A, const PeakGroupArgs& a, double* __restrict__ out) {
    const int tid = threadIdx.x;
    const size_t MW = (size_t)a.MW;
    const float* __restrict__ img = a.map + (size_t)g.y0 * MW + (size_t)g.x0;
    const int M = g.M, P = 6 * M;
    const double bkg = g.bkg, sign = g.sign;
    MultiSmem& m = s.m;

    if (tid < P) { m.p[tid] = g.p0[tid]; m.pt[tid] = g.p0[tid]; }
    if (tid == 0) { m.ctl.act = ACT_NONE; m.ctl.stop = 0; }
    // ---- the staging pass: the members' values (LDS), npix and nexcluded
    unsigned np = 0, nex = 0;
    for (unsigned q = tid; q < A; q += PG_T) {
        unsigned wx, wy; bool in;
        const bool mine = group_member(s, M, q, wx, wy, in);
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
    const int early = !admissible_all(g.p0, M) ? 4 : np < (unsigned)(P + 1) ? 3 : 0;     // uniform
    if (early) {                                              // the start as given; the runtime restores the centres' exact bits
        if (tid < M * PGRP_FIELDS) {
            const int t = tid / PGRP_FIELDS, f = tid - t * PGRP_FIELDS;
            double v = 0.0;
            if (f == 0) v = (double)early;
            else if (f == 2) v = (double)np;
            else if (f == 5) v = (double)g.member[0];
            else if (f == 6) v = (double)M;
            else if (f == 7) v = (double)t;
            else if (f >= 8 && f < 14) v = g.p0[6 * t + f - 8];
            else if (f == 41) v = (double)nex;
            out[tid] = v;
        }
        return;
    }

    // list entry q is window pixel q -> q (or LM_BAD) and the datum
    const auto entry = [&](const unsigned q, double& y) {
        float fv;
        if (LDS) fv = s.val[q];
        else {
            unsigned wx, wy; bool in;
            fv = 0.0f;
            if (group_member(s, M, q, wx, wy, in)) fv = img[(size_t)wy * MW + wx];
        }
        y = sign * ((double)fv - bkg);
        return valid_px(fv) ? q : LM_BAD;
    };
    const MultiSums u = multi_sums(P);
    double lam;
    int status, niter;
    multi_iterate(m, M, u.nsum, a.max_iter, lam, status, niter, [&](const double* pp) { multi_sweep(m, pp, M, A, W, u, entry); });
    if (tid != 0) return;
    const bool cov = multi_inverse(m, P);
    for (int t = 0; t < M; ++t) {
        double* o = out + (size_t)t * PGRP_FIELDS;
        multi_row(m, P, M, t, cov, status, niter, np, lam, g.member[0], o);
        o[41] = (double)nex;
    }
}

__global__ __launch_bounds__(PG_T) void peakgroup_kernel(const PeakGroupArgs a) {
    __shared__ GSmem s;
    const int tid = threadIdx.x;
    const int t = blockIdx.x;
    if (t >= a.ngroups) return;                               // the rows are inside the output: the grid is ngroups
    double* out = a.out + (size_t)t * PG_M * PGRP_FIELDS;
    const PeakGroupJob& g = a.groups[t];
    // the planner's groups name fitted jobs of the table, their windows lie inside the image and their neighbours inside the table;
    // checked again so that no index can leave a buffer whatever arrives here.  cy_fit_peak_groups cannot produce such a job; should
    // it ever happen, nothing is fitted and the rows are NaN throughout
    bool ok = g.M >= 2 && g.M <= PG_M && g.x0 >= 0 && g.y0 >= 0 && g.x1 >= g.x0 && g.y1 >= g.y0 && g.x1 < a.MW && g.y1 < a.MH &&
              g.x1 - g.x0 < PG_SIDE_MAX && g.y1 - g.y0 < PG_SIDE_MAX;
    for (int e = 0; e < PG_M; ++e) {
        if (!ok || e >= g.M) continue;
        ok = g.member[e] >= 0 && g.member[e] < a.n && (e == 0 || g.member[e] > g.member[e - 1]) && g.nout[e] >= 0 && g.nout[e] <= DISC_NB;
        for (int k = 0; k < DISC_NB; ++k) ok = ok && (k >= g.nout[e] || (g.out[e][k] >= 0 && g.out[e][k] < a.n));
    }
    if (!ok) {                                                // uniform: the arguments and the job record only
        if (tid < PG_M * PGRP_FIELDS) out[tid] = __longlong_as_double(0x7FF8000000000000LL);
        return;
    }
    const unsigned W = (unsigned)(g.x1 - g.x0 + 1), A = W * (unsigned)(g.y1 - g.y0 + 1);
    if (tid < PG_M) {
        Disc& d = s.disc[tid];
        const bool has = tid < g.M;
        const PeakFitJob* e = a.jobs + g.member[has ? tid : 0];
        d.bx0 = g.x0; d.by0 = g.y0; d.W = W;
        d.cx = e->cx; d.cy = e->cy; d.r2 = has ? e->r2 : -1.0; d.nn = has ? g.nout[tid] : 0;
        for (int k = 0; k < DISC_NB; ++k) {
            const bool hk = has && k < g.nout[tid];
            const PeakFitJob* f = hk ? a.jobs + g.out[tid][k] : e;
            d.ncx[k] = f->cx; d.ncy[k] = f->cy;              // beyond nn: the member's own centre, which member() does not look at
        }
    }
    __syncthreads();
    if (A <= (unsigned)PGRP_LDS_MAX) fit<true>(s, g, W, A, a, out);
    else fit<false>(s, g, W, A, a, out);
}

}  // namespace

hipError_t launch_peak_groups(const PeakGroupArgs& a, hipStream_t s) {
    if (a.ngroups < 1 || a.n < 2 || a.ngroups > a.n / 2 || a.n > PFIT_JOBS_MAX || a.MH < 1 || a.MW < 1 || (long long)a.MH * a.MW >= (1LL << 31) ||
        a.max_iter < 1 || a.max_iter > FIT_MAX_ITER || !a.map || !a.jobs || !a.groups || !a.out)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(peakgroup_kernel, dim3(a.ngroups), dim3(PG_T), 0, s, a);
    return hipGetLastError();
}

}  // namespace cy
