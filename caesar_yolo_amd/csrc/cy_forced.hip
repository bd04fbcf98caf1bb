// Forced photometry (cy_forced_fit): the amplitudes of Gaussians of FIXED position and shape on any map, one weighted linear
// least-squares problem per job (definitions: include/caesar_yolo_hip.h, DESIGN.md "Forced photometry").
//   unknowns    K = 1 + nneigh + fit_bkg <= 9: the job's amplitude, those of its at most FORCED_NEIGH_MAX = 7 kept neighbours (the
//               planner's list), and a local constant
//   pixel set   window pixel (ix, iy) of the job's support rectangle with q_0 <= nsigma^2, a valid v and, with an rms map, a usable
//               rms (noisy_px); q = (a*u)*u + ((2*b)*u)*v + (c*v)*v as the render kernel of cy_residual.hip forms it.  A pixel
//               inside the ellipse that fails the other two tests counts in nexcluded
//   per pixel   s = 1 / (double)rms (1 without a map); w = (((double)v - bkg) s, e_0 s, .., e_nneigh s, [s]), e_i = exp(-0.5 q_i); the
//               sums are the upper triangle of w^T w, every product rounded before it is added
// One workgroup of 256 threads owns one job; the grid is the number of jobs the planner (plan_forced) runs, and workgroup t
// writes row t of a table of its own that the host deals out (forced_row).  No workgroup reads what another one wrote; no atomics,
// no inline assembly.  The parameters of the job and its neighbours (8 x 5 float64) are loaded once into LDS.
// w lives in ten fixed slots: 0 the datum, 1 the job, 2 .. 8 the neighbours in kept order (0 beyond nneigh), 9 the constant (0
// without it), and every thread keeps the 55 sums of the 10 x 10 triangle in registers: a slot that is not in use adds exact zeros
// and its sums are never read.  Window pixel i = wy * W + wx sits on thread i mod 256; the sums run sequentially per thread over
// increasing i, then the block reduction of cy_reduce.h (red_sum).  Two calls give the same bytes.
// Thread 0 solves in LDS (Cholesky row by row as factor() of cy_lm_multi.h, a pivot t needs t > N_jj 2^-40 and a finite t), then
// everyone sweeps the same pixel set again for chi2 = sum (w_0 - sum_i x_i w_{1+i})^2 at the solution.
// Every loop has a bound fixed before it starts:
//   sweeps      twice over the A <= 514 x 514 pixels of the window, 256 at a time (the second has A = 0 when nothing was solved)
//   per pixel   FORCED_NEIGH_MAX = 7 neighbour terms and the 55 products, unrolled;  reductions: 6 shuffle steps and 4 waves
//   thread 0    Cholesky, the two triangular solves, inv(L) and the entries of inv(N): nested loops over K <= 9
// Every early return is uniform and comes before the first barrier: it depends on the arguments and the job record alone.
#include "cy_px.h"                      // valid_px, noisy_px
#include "cy_reduce.h"                  // RedSlots, reduction

#pragma clang fp contract(off)          // every product is rounded before it is added, as the float64 definition does

namespace cy {
namespace {

constexpr int FC_T = 256;
constexpr int FC_NB = FORCED_NEIGH_MAX, FC_W = FC_NB + 3, FC_KMAX = FC_NB + 2;     // 10 slots of w, at most 9 unknowns
constexpr int FC_NSUM = FC_W * (FC_W + 1) / 2;                                      // 55
constexpr int FC_BKG = FC_W - 1;                                                    // the slot of the constant

__host__ __device__ constexpr int fc_idx(int i, int j) { return i * FC_W - i * (i - 1) / 2 + (j - i); }    // sum (i, j), i <= j, row-major upper triangle
static_assert(fc_idx(FC_W - 1, FC_W - 1) == FC_NSUM - 1, "the triangle has FC_NSUM sums");

struct ForcedSmem {
    RedSlots<FC_T, FC_NSUM + 2> slots;
    double nb[FC_NB + 1][5];            // x0, y0, a, b, c of the job (row 0) and of its kept neighbours
    double tot[FC_NSUM];                // the sums
    double L[FC_KMAX][FC_KMAX], X[FC_KMAX][FC_KMAX];       // thread 0's Cholesky factor and its inverse
    double z[FC_KMAX], x[FC_KMAX];
    double xs[FC_W];                    // the solution by slot (xs[0] unused); zeros where no unknown lives
    int solved;
};

// what the sweeps share: the job's constants, uniform
struct ForcedCtx {
    const float* __restrict__ map; const float* __restrict__ rms;
    size_t MW;
    int bx0, by0; unsigned W;
    double bkg, ns2;
    int nn, fit_bkg;
};

// w of window pixel i.  -> 0 outside the ellipse, 1 a member (w filled), 2 inside the ellipse and excluded
__device__ __forceinline__ int forced_w(const ForcedSmem& s, const ForcedCtx& c, const unsigned i, double (&w)[FC_W]) {
    const unsigned wy = i / c.W, wx = i - wy * c.W;
    const double px = (double)(c.bx0 + (int)wx), py = (double)(c.by0 + (int)wy);
    double q[FC_NB + 1];
#pragma unroll
    for (int k = 0; k <= FC_NB; ++k) {
        q[k] = 0.0;
        if (k > c.nn) continue;                               // uniform
        const double u = px - s.nb[k][0], v = py - s.nb[k][1];
        q[k] = (s.nb[k][2] * u) * u + ((2.0 * s.nb[k][3]) * u) * v + (s.nb[k][4] * v) * v;
    }
    if (!(q[0] <= c.ns2)) return 0;
    const size_t p = ((size_t)c.by0 + wy) * c.MW + (size_t)c.bx0 + wx;
    const float fv = c.map[p];
    bool good = valid_px(fv);
    float fr = 1.0f;
    if (c.rms) { fr = c.rms[p]; good = good && noisy_px(fr); }
    if (!good) return 2;
    const double sc = c.rms ? 1.0 / (double)fr : 1.0;
    w[0] = ((double)fv - c.bkg) * sc;
#pragma unroll
    for (int k = 0; k <= FC_NB; ++k) w[1 + k] = k <= c.nn ? exp(-0.5 * q[k]) * sc : 0.0;
    w[FC_BKG] = c.fit_bkg ? sc : 0.0;
    return 1;
}

__device__ __forceinline__ bool fc_fin(double v) { return fabs(v) <= DBL_MAX; }
// the slot of unknown i (0 .. K - 1): the job and its neighbours sit in slots 1 .. 1 + nn, the constant in FC_BKG
__device__ __forceinline__ int fc_slot(int i, int nn) { return i <= nn ? 1 + i : FC_BKG; }

// thread 0: x = inv(N) b into s.x, inv(L) into s.X; false on a pivot that fails
__device__ bool forced_solve(ForcedSmem& s, const int K, const int nn) {
    for (int j = 0; j < K; ++j) {
        const int sj = fc_slot(j, nn);
        const double njj = s.tot[fc_idx(sj, sj)];
        double t = njj;
        for (int k = 0; k < j; ++k) t -= s.L[j][k] * s.L[j][k];
        if (!(t > njj * 0x1p-40) || !fc_fin(t)) return false;
        const double ljj = sqrt(t);
        s.L[j][j] = ljj;
        for (int i = j + 1; i < K; ++i) {
            double q = s.tot[fc_idx(sj, fc_slot(i, nn))];
            for (int k = 0; k < j; ++k) q -= s.L[i][k] * s.L[j][k];
            s.L[i][j] = q / ljj;
        }
    }
    for (int i = 0; i < K; ++i) {
        double q = s.tot[fc_idx(0, fc_slot(i, nn))];
        for (int k = 0; k < i; ++k) q -= s.L[i][k] * s.z[k];
        s.z[i] = q / s.L[i][i];
    }
    for (int i = K - 1; i >= 0; --i) {
        double q = s.z[i];
        for (int k = i + 1; k < K; ++k) q -= s.L[k][i] * s.x[k];
        s.x[i] = q / s.L[i][i];
    }
    for (int c = 0; c < K; ++c) {                             // inv(L) column by column, as multi_inverse of cy_lm_multi.h
        s.X[c][c] = 1.0 / s.L[c][c];
        for (int i = c + 1; i < K; ++i) {
            double q = 0.0;
            for (int k = c; k < i; ++k) q -= s.L[i][k] * s.X[k][c];
            s.X[i][c] = q / s.L[i][i];
        }
    }
    return true;
}
// thread 0: C_ij of C = inv(N) = inv(L)^T inv(L), i <= j
__device__ double forced_cov(const ForcedSmem& s, const int K, const int i, const int j) {
    double c = 0.0;
    for (int k = j; k < K; ++k) c += s.X[k][i] * s.X[k][j];
    return c;
}

__global__ __launch_bounds__(FC_T) void forced_kernel(const ForcedArgs a) {
    __shared__ ForcedSmem s;
    const int tid = threadIdx.x;
    const int t = blockIdx.x;
    if (t >= a.nrun) return;                                  // the row is inside the output: the grid is nrun
    double* out = a.out + (size_t)t * FORCED_FIELDS;
    const int e = a.run[t];
    // the planner's jobs are run ones, their rectangles inside the image and their neighbours inside the table; checked again so
    // that no index can leave a buffer whatever arrives here (as peakfit_kernel does).  cy_forced_fit cannot produce such a job;
    // should it ever happen, nothing is read and the row is NaN throughout
    bool ok = e >= 0 && e < a.n && (a.fit_bkg == 0 || a.fit_bkg == 1);
    ForcedJob j{};
    if (ok) {
        j = a.jobs[e];
        ok = (j.status == 0 || j.status == 2) && j.x0 >= 0 && j.y0 >= 0 && j.x1 >= j.x0 && j.y1 >= j.y0 && j.x1 < a.MW && j.y1 < a.MH &&
             j.x1 - j.x0 < FORCED_SIDE_MAX && j.y1 - j.y0 < FORCED_SIDE_MAX && j.nneigh >= 0 && j.nneigh <= FC_NB;
#pragma unroll
        for (int k = 0; k < FC_NB; ++k) ok = ok && (k >= j.nneigh || (j.neigh[k] >= 0 && j.neigh[k] < a.n));
    }
    if (!ok) {                                                // uniform: the arguments and the job record only
        if (tid < FORCED_FIELDS) out[tid] = __longlong_as_double(0x7FF8000000000000LL);
        return;
    }
    const int nn = j.nneigh, K = 1 + nn + a.fit_bkg;
    if (tid <= FC_NB) {                                       // thread k loads neighbour k - 1 (thread 0: the job); beyond nneigh: the job again
        const int f = tid >= 1 && tid <= nn ? a.jobs[e].neigh[tid - 1] : e;
        const ForcedJob* g = a.jobs + f;
        s.nb[tid][0] = g->cx; s.nb[tid][1] = g->cy; s.nb[tid][2] = g->a; s.nb[tid][3] = g->b; s.nb[tid][4] = g->c;
    }
    ForcedCtx c;
    c.map = a.map; c.rms = a.rms; c.MW = (size_t)a.MW;
    c.bx0 = j.x0; c.by0 = j.y0; c.W = (unsigned)(j.x1 - j.x0 + 1);
    c.bkg = j.bkg; c.ns2 = a.ns2; c.nn = nn; c.fit_bkg = a.fit_bkg;
    const unsigned A = c.W * (unsigned)(j.y1 - j.y0 + 1);
    __syncthreads();

    double acc[FC_NSUM];
#pragma unroll
    for (int k = 0; k < FC_NSUM; ++k) acc[k] = 0.0;
    unsigned cnt[2] = {0u, 0u};                               // npix, nexcluded
    for (unsigned i = tid; i < A; i += FC_T) {
        double w[FC_W];
        const int m = forced_w(s, c, i, w);
        if (m == 0) continue;
        if (m == 2) { ++cnt[1]; continue; }
        ++cnt[0];
#pragma unroll
        for (int r = 0; r < FC_W; ++r)
#pragma unroll
            for (int q = r; q < FC_W; ++q) acc[fc_idx(r, q)] += w[r] * w[q];
    }
    {
        const auto red = reduction(red_sum(acc), red_sum(cnt));
        red.wave();
        red.park(s.slots);
        __syncthreads();
        if (tid == 0) red.total(s.slots);
    }
    int status = 0;
    double amp = 0.0, amp_var = 0.0, bkg_off = 0.0, bkg_var = 0.0, cov_ab = 0.0, corr = 0.0;
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < FC_NSUM; ++k) s.tot[k] = acc[k];
        for (int k = 0; k < FC_W; ++k) s.xs[k] = 0.0;
        status = j.status;
        if (cnt[0] < (unsigned)K) status = 5;
        else if (!forced_solve(s, K, nn)) status = 4;
        else {
            amp = s.x[0]; amp_var = forced_cov(s, K, 0, 0);
            for (int i = 1; i <= nn; ++i) {
                const double r = fabs(forced_cov(s, K, 0, i)) / sqrt(amp_var * forced_cov(s, K, i, i));
                if (r > corr) corr = r;
            }
            if (a.fit_bkg) { bkg_off = s.x[K - 1]; bkg_var = forced_cov(s, K, K - 1, K - 1); cov_ab = forced_cov(s, K, 0, K - 1); }
            for (int i = 0; i < K; ++i) s.xs[fc_slot(i, nn)] = s.x[i];
        }
        s.solved = status == 0 || status == 2;
    }
    __syncthreads();
    const unsigned A2 = s.solved ? A : 0u;                    // uniform
    double xs[FC_W];
#pragma unroll
    for (int k = 0; k < FC_W; ++k) xs[k] = s.xs[k];
    double chi = 0.0;
    for (unsigned i = tid; i < A2; i += FC_T) {
        double w[FC_W];
        if (forced_w(s, c, i, w) != 1) continue;
        double m = xs[1] * w[1];
#pragma unroll
        for (int k = 2; k < FC_BKG; ++k)
            if (k <= 1 + nn) m += xs[k] * w[k];               // uniform
        if (a.fit_bkg) m += xs[FC_BKG] * w[FC_BKG];
        const double r = w[0] - m;
        chi += r * r;
    }
    const auto red2 = reduction(red_sum(chi));
    red2.wave();
    red2.park(s.slots);
    __syncthreads();
    if (tid == 0) {
        red2.total(s.slots);
        out[0] = (double)status; out[1] = (double)cnt[0]; out[2] = (double)cnt[1]; out[3] = (double)K; out[4] = (double)nn;
        out[5] = (double)j.crowded; out[6] = (double)j.ndup;
        out[7] = amp; out[8] = amp_var; out[9] = bkg_off; out[10] = bkg_var; out[11] = cov_ab; out[12] = chi;
        out[13] = s.tot[fc_idx(0, 0)]; out[14] = s.tot[fc_idx(1, 1)]; out[15] = s.tot[fc_idx(0, 1)];
        out[16] = corr;
        out[17] = (double)j.x0; out[18] = (double)j.x1; out[19] = (double)j.y0; out[20] = (double)j.y1;
        out[21] = j.status == 2 ? 1.0 : 0.0; out[22] = 0.0; out[23] = 0.0;
    }
}

}  // namespace

hipError_t launch_forced(const ForcedArgs& a, hipStream_t s) {
    if (a.nrun < 1 || a.nrun > a.n || a.n > FORCED_JOBS_MAX || a.MH < 1 || a.MW < 1 || (long long)a.MH * a.MW >= (1LL << 31) || !a.map || !a.jobs ||
        !a.run || !a.out || (a.fit_bkg != 0 && a.fit_bkg != 1))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(forced_kernel, dim3(a.nrun), dim3(FC_T), 0, s, a);
    return hipGetLastError();
}

}  // namespace cy
