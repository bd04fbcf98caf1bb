// What the component fit (cy_fit.hip), the joint fit of a blend (cy_blend.hip) and the fit of a peak at a position (cy_peakfit.hip)
// share: the elliptical Gaussian and its Jacobian, the staging of a job's pixel list, the 6 x 6 solve of the single-Gaussian fits
// and the Levenberg-Marquardt decision loop.  The rule of that loop is part of what a fitted
// number means and stands here once:
//   start     lambda = 1e-3, status 2, niter = max_iter
//   step      thread 0 solves (H + lambda diag(H)) d = g; `small`: every |d_k| <= 1e-10 (|p_k| + 1e-6); the trial is p + d
//   no trial  (no positive finite pivot, or p + d not admissible): converged (status 0) when small, else lambda *= 10
//   trial     everyone sweeps at p + d.  Fn < F: accepted, lambda = max(lambda / 10, 1e-12), converged when small or
//             F - Fn <= 1e-14 F.  Otherwise converged when small, else lambda *= 10
//   give up   lambda > 1e12: status 2
// Every lambda escalation is one iteration of it = 1 .. max_iter, so there is no inner loop.  Thread 0 decides; its decisions
// reach the other threads through the two LDS words of LmCtl, read after a barrier (uniform).
#pragma once
#include "cy_px.h"
#include "cy_reduce.h"                  // RedSlots, reduction
#include <cfloat>

#pragma clang fp contract(off)          // every product is rounded before it is added, as the float64 definition does

namespace cy {
namespace {

constexpr unsigned LM_BAD = 0xFFFFFFFFu;                    // a list entry that contributes nothing
constexpr int ACT_NONE = 0, ACT_SWEEP = 1, ACT_STOP = 2;
struct LmCtl { volatile int act, stop; };

__device__ __forceinline__ bool fin(double v) { return fabs(v) <= DBL_MAX; }
__device__ __forceinline__ bool admissible(const double* p) {
    return fin(p[0]) && fin(p[1]) && fin(p[2]) && fin(p[3]) && fin(p[4]) && fin(p[5]) && p[0] > 0.0 && p[3] > 0.0 && p[5] > 0.0 &&
           p[3] * p[5] - p[4] * p[4] > 0.0;
}

// One member at one pixel: m = A exp(-(a u^2 + 2 b u v + c v^2) / 2), u = dx - x0, v = dy - y0, and J = dm / d(A, x0, y0, a, b, c)
__device__ __forceinline__ double gauss_terms(const double A, const double x0, const double y0, const double a, const double b,
                                              const double c, const double dx, const double dy, double* J) {
    const double u = dx - x0, v = dy - y0;
    const double e = exp(-0.5 * ((a * u) * u + ((2.0 * b) * u) * v + (c * v) * v));
    const double m = A * e;
    J[0] = e; J[1] = m * (a * u + b * v); J[2] = m * (b * u + c * v);
    J[3] = ((-0.5 * m) * u) * u; J[4] = ((-m) * u) * v; J[5] = ((-0.5 * m) * v) * v;
    return m;
}

// Entry q of a job's list -> its window index i = dy * W + dx and the pixel's value, or LM_BAD when the index is outside the
// window or the pixel is not valid.  img: first pixel of the window, MW: row pitch of the image
__device__ __forceinline__ unsigned list_pixel(const unsigned* __restrict__ list, const unsigned q, const float* __restrict__ img,
                                               const size_t MW, const unsigned W, const unsigned A, float& fv) {
    const unsigned i = list[q];
    fv = 0.0f;
    if (i < A) { const unsigned yy = i / W; fv = img[(size_t)yy * MW + (i - yy * W)]; }
    return i >= A || !valid_px(fv) ? LM_BAD : i;
}

// The valid pixels of the list, counted (and, LDS, {value, index} of every entry parked in val / idx).  Ends with a barrier after
// which every thread holds the count: what the caller wrote to LDS before the call is visible to everyone after it.  No barrier
// follows the last read of cnt, so these slots are cnt's alone: a sweep that parked in them could overtake a slower wave's read
template <int NT, bool LDS>
__device__ __forceinline__ unsigned stage_list(float* val, unsigned* idx, RedSlots<NT, 1>& cnt, const unsigned* __restrict__ list, const unsigned npos,
                                               const float* __restrict__ img, const size_t MW, const unsigned W, const unsigned A) {
    const int tid = threadIdx.x;
    unsigned np = 0;
    for (unsigned q = tid; q < npos; q += NT) {
        float fv;
        const unsigned i = list_pixel(list, q, img, MW, W, A, fv);
        if (LDS) { idx[q] = i; val[q] = fv; }
        np += i != LM_BAD;
    }
    const auto red = reduction(red_sum(np));
    red.wave();
    red.park(cnt);
    __syncthreads();
    red.total(cnt);                                           // every thread
    return np;
}

// thread 0: pt = p + d -> `small`
__device__ __forceinline__ bool lm_trial(const int P, const double* p, const double* d, double* pt) {
    bool small = true;
    for (int k = 0; k < P; ++k) {
        small = small && fabs(d[k]) <= 1e-10 * (fabs(p[k]) + 1e-6);
        pt[k] = p[k] + d[k];
    }
    return small;
}

__host__ __device__ constexpr int hidx(int i, int j) { return 7 + i * 6 - i * (i - 1) / 2 + (j - i); }   // H(i, j), i <= j, in the 28 sums
static_assert(hidx(0, 0) == 7 && hidx(5, 5) == FIT_NSUM - 1, "F, g (6), H upper triangle row-major (21)");

// thread 0: d of (H + lam diag(H)) d = g by Cholesky (row by row, every inner sum subtracted term by term in increasing k); false
// on a pivot that is not positive and finite
__device__ __forceinline__ bool lm_solve(const double* cur, const double lam, double* d) {
    double L[6][6], z[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const double hjj = cur[hidx(j, j)];
        double t = hjj + lam * hjj;
#pragma unroll
        for (int k = 0; k < j; ++k) t -= L[j][k] * L[j][k];
        if (!(t > 0.0) || !fin(t)) return false;
        L[j][j] = sqrt(t);
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double q = cur[hidx(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) q -= L[i][k] * L[j][k];
            L[i][j] = q / L[j][j];
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double q = cur[1 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) q -= L[i][k] * z[k];
        z[i] = q / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double q = z[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) q -= L[k][i] * d[k];
        d[i] = q / L[i][i];
    }
    return true;
}

// The loop of the header comment, run by the whole workgroup after the sums at the start are in place and ctl is {ACT_NONE, 0}.
//   solve(lam, small)   thread 0: d at lam, small = lm_trial(..), the trial parameters; true when there is a trial to sweep
//   sweep()             everyone: the sums at the trial, visible to thread 0 when it returns
//   Fcur(), Fnew()      thread 0: F at the accepted parameters / at the trial
//   accept()            thread 0: the trial and its sums become the accepted ones
// lam, status and niter are thread 0's when it returns
template <typename Solve, typename Sweep, typename FCur, typename FNew, typename Accept>
__device__ __forceinline__ void lm_iterate(LmCtl& ctl, const int max_iter, double& lam, int& status, int& niter, Solve solve, Sweep sweep,
                                           FCur Fcur, FNew Fnew, Accept accept) {
    const int tid = threadIdx.x;
    bool small = false;
    lam = 1e-3; status = 2; niter = max_iter;
    for (int it = 1; it <= max_iter; ++it) {
        if (tid == 0) {
            small = false;
            int act = solve(lam, small) ? ACT_SWEEP : ACT_NONE;
            if (act == ACT_NONE) {                            // rejected without a sweep
                if (small) { status = 0; niter = it; act = ACT_STOP; }
                else {
                    lam *= 10.0;
                    if (lam > 1e12) { status = 2; niter = it; act = ACT_STOP; }
                }
            }
            ctl.act = act;
        }
        __syncthreads();
        const int act = ctl.act;                              // uniform (from LDS)
        if (act == ACT_STOP) break;
        if (act == ACT_SWEEP) {
            sweep();
            if (tid == 0) {
                const double F = Fcur(), Fn = Fnew();
                if (Fn < F) {
                    const bool conv = small || F - Fn <= 1e-14 * F;
                    accept();
                    lam = fmax(lam / 10.0, 1e-12);
                    if (conv) { status = 0; niter = it; ctl.stop = 1; }
                } else if (small) { status = 0; niter = it; ctl.stop = 1; }
                else {
                    lam *= 10.0;
                    if (lam > 1e12) { status = 2; niter = it; ctl.stop = 1; }
                }
            }
        }
        __syncthreads();
        if (ctl.stop) break;                                  // uniform (from LDS)
    }
}

}  // namespace
}  // namespace cy
