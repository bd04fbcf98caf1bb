// What the joint fit of a blend (cy_blend.hip) and the joint fit of a group of peaks (cy_peakgroup.hip) share: the sum of M <=
// BLEND_MAX_MEMBERS elliptical Gaussians fitted to one list of pixels, unweighted Levenberg-Marquardt in float64 (definitions:
// include/caesar_yolo_hip.h, DESIGN.md "Joint fits of blends").  The two kernels differ only in how list position q yields its
// pixel: `entry(q, y)` returns the window index i = dy * W + dx, or LM_BAD for an entry that contributes nothing, and the datum y.
//   model    m = sum_s A_s exp(-q_s / 2), every member as in cy_fit.hip; p = M x (A, x0, y0, a, b, c), P = 6 M parameters, x0 / y0
//            relative to the window's first pixel in here (the runtime converts from and to image pixels)
//   sweep    per list entry the vector w = (r, J_0 .. J_{P-1}), P + 1 numbers; the sums are the upper triangle of w^T w in row-major
//            order: F = w_0 w_0, g_i = w_0 w_{1+i}, H_ij = w_{1+i} w_{1+j}: NS = (P + 1)(P + 2) / 2 <= 325 float64 sums
//   step     thread 0: P x P Cholesky of H + lambda diag(H) in LDS, d, `small`, admissibility of p + d; everyone: sweep at the trial;
//            thread 0: accept / reject, lambda, convergence (lm_iterate of cy_lm.h, which states the rule and owns the loop), and
//            at the end inv(H)
// Ownership is by SUM, not by pixel: thread t of the 256 owns sums t and t + 256 and adds them over the whole list, so every sum is
// one plain sequential float64 sum in increasing list position: no reduction, no shuffle, no atomic, and two runs give the same
// bits.  The list is worked in chunks of BLEND_CHUNK = 128 entries: thread e < 128 computes w of chunk entry e (M exp) into LDS row
// e, 25 doubles apart (50 dwords: the 16 lanes of a 64-bit store group fall on 16 different bank pairs, and in the adding phase every
// lane reads row e at its own two columns: distinct banks or a broadcast); after a barrier every thread adds its two products per
// chunk entry.
// Every loop has a bound fixed before it starts:
//   sweep       chunks ceil(npos / 128); per chunk <= 128 entries, M <= 4 members each
//   pair        the (row, column) of a sum index: at most P + 1 = 25 steps, once per job
//   thread 0    Cholesky, the two triangular solves, the inverse of L and the members' blocks of inv(H): nested loops over P <= 24
#pragma once
#include "cy_lm.h"                      // gauss_terms, lm_trial, lm_iterate

#pragma clang fp contract(off)          // every product is rounded before it is added, as the float64 definition does

namespace cy {
namespace {

constexpr int ML_T = 256;
constexpr int ML_PMAX = 6 * BLEND_MAX_MEMBERS, ML_WMAX = ML_PMAX + 1;       // 24 parameters, 25 numbers per list entry
static_assert(BLEND_NSUM_MAX == ML_WMAX * (ML_WMAX + 1) / 2 && BLEND_NSUM_MAX <= 2 * ML_T, "two sums per thread cover every sum");
static_assert(ML_PMAX * ML_PMAX <= BLEND_CHUNK * ML_WMAX, "the inverse of L reuses the chunk rows");

struct MultiSmem {
    double ch[BLEND_CHUNK][ML_WMAX];    // w of the chunk's entries; after the fit: inv(L), row-major P x P
    double tot[BLEND_NSUM_MAX];         // sums of the last sweep
    double cur[BLEND_NSUM_MAX];         // sums at the accepted p
    double L[ML_PMAX][ML_PMAX];         // thread 0's Cholesky factor
    double p[ML_PMAX], pt[ML_PMAX], z[ML_PMAX], d[ML_PMAX];
    LmCtl ctl;
};

__device__ __forceinline__ bool admissible_all(const double* p, const int M) {
    bool ok = true;
    for (int s = 0; s < M; ++s) ok = ok && admissible(p + 6 * s);
    return ok;
}
__device__ __forceinline__ int hidx(const int P, const int i, const int j) { return 1 + P + i * P - i * (i - 1) / 2 + (j - i); }   // H(i, j), i <= j

// (row, column) of sum q in the row-major upper triangle of the n x n matrix w^T w; (0, 0) for q outside it
__device__ __forceinline__ void pair_of(int q, const int n, int* a, int* b) {
    *a = 0; *b = 0;
    if (q >= n * (n + 1) / 2) return;
    int r = 0;
    for (int k = 0; k < ML_WMAX; ++k) {
        if (q < n - r) break;
        q -= n - r; ++r;
    }
    *a = r; *b = r + q;
}

// the two sums of every thread, fixed for the job: sums tid and tid + 256 of the nsum = (P + 1)(P + 2) / 2
struct MultiSums { int a1, b1, a2, b2, nsum; };
__device__ __forceinline__ MultiSums multi_sums(const int P) {
    MultiSums u;
    pair_of(threadIdx.x, P + 1, &u.a1, &u.b1);
    pair_of(threadIdx.x + ML_T, P + 1, &u.a2, &u.b2);
    u.nsum = (P + 1) * (P + 2) / 2;
    return u;
}

// the sums at pp (LDS, uniform) over the job's list of npos entries in a window W wide; they land in s.tot (visible to everyone
// after the barrier at the end)
template <typename Entry>
__device__ __forceinline__ void multi_sweep(MultiSmem& s, const double* pp, const int M, const unsigned npos, const unsigned W, const MultiSums& u,
                                            Entry entry) {
    const int tid = threadIdx.x;
    double acc1 = 0.0, acc2 = 0.0;
    for (unsigned base = 0; base < npos; base += BLEND_CHUNK) {
        const unsigned cnt = npos - base < (unsigned)BLEND_CHUNK ? npos - base : (unsigned)BLEND_CHUNK;
        if ((unsigned)tid < cnt) {
            double y;
            const unsigned i = entry(base + tid, y);
            double* w = s.ch[tid];
            if (i == LM_BAD) {
                for (int k = 0; k <= 6 * M; ++k) w[k] = 0.0;
            } else {
                const unsigned dy = i / W, dx = i - dy * W;
                double mt = 0.0;
                for (int t = 0; t < M; ++t) {
                    const double* p = pp + 6 * t;
                    const double m = gauss_terms(p[0], p[1], p[2], p[3], p[4], p[5], (double)dx, (double)dy, w + 1 + 6 * t);
                    mt = t == 0 ? m : mt + m;
                }
                w[0] = y - mt;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (unsigned e = 0; e < cnt; ++e) {
            const double* w = s.ch[e];
            acc1 += w[u.a1] * w[u.b1];
            acc2 += w[u.a2] * w[u.b2];
        }
        __syncthreads();
    }
    if (tid < u.nsum) s.tot[tid] = acc1;
    if (tid + ML_T < u.nsum) s.tot[tid + ML_T] = acc2;
    __syncthreads();
}

// thread 0: the Cholesky factor of H + lam diag(H) into s.L (row by row, every inner sum subtracted term by term in increasing k);
// false on a pivot that is not positive and finite
__device__ bool factor(MultiSmem& s, const int P, const double lam) {
    for (int j = 0; j < P; ++j) {
        const double hjj = s.cur[hidx(P, j, j)];
        double t = hjj + lam * hjj;
        for (int k = 0; k < j; ++k) t -= s.L[j][k] * s.L[j][k];
        if (!(t > 0.0) || !fin(t)) return false;
        const double ljj = sqrt(t);
        s.L[j][j] = ljj;
        for (int i = j + 1; i < P; ++i) {
            double q = s.cur[hidx(P, j, i)];
            for (int k = 0; k < j; ++k) q -= s.L[i][k] * s.L[j][k];
            s.L[i][j] = q / ljj;
        }
    }
    return true;
}

// thread 0: d of (H + lam diag(H)) d = g into s.d
__device__ bool lm_solve(MultiSmem& s, const int P, const double lam) {
    if (!factor(s, P, lam)) return false;
    for (int i = 0; i < P; ++i) {
        double q = s.cur[1 + i];
        for (int k = 0; k < i; ++k) q -= s.L[i][k] * s.z[k];
        s.z[i] = q / s.L[i][i];
    }
    for (int i = P - 1; i >= 0; --i) {
        double q = s.z[i];
        for (int k = i + 1; k < P; ++k) q -= s.L[k][i] * s.d[k];
        s.d[i] = q / s.L[i][i];
    }
    return true;
}

// Everyone, with s.p = s.pt = the start and ctl = {ACT_NONE, 0} visible: the sums at the start, then the loop of cy_lm.h.
// sweep(pp): multi_sweep at pp over the job's list.  lam, status and niter are thread 0's when it returns, and so are s.p / s.cur
template <typename Sweep>
__device__ __forceinline__ void multi_iterate(MultiSmem& s, const int M, const int nsum, const int max_iter, double& lam, int& status, int& niter,
                                              Sweep sweep) {
    const int tid = threadIdx.x;
    const int P = 6 * M;
    sweep(s.pt);
    for (int k = tid; k < nsum; k += ML_T) s.cur[k] = s.tot[k];
    __syncthreads();
    lm_iterate(s.ctl, max_iter, lam, status, niter,
               [&](const double lam, bool& small) {
                   if (!lm_solve(s, P, lam)) return false;
                   small = lm_trial(P, s.p, s.d, s.pt);
                   return admissible_all(s.pt, M);
               },
               [&] { sweep(s.pt); },
               [&] { return s.cur[0]; }, [&] { return s.tot[0]; },
               [&] {
                   for (int k = 0; k < nsum; ++k) s.cur[k] = s.tot[k];
                   for (int k = 0; k < P; ++k) s.p[k] = s.pt[k];
               });
}

// thread 0: C = inv(H) at the reported p through H = L L^T, X = inv(L) column by column (into the chunk rows); false when H has
// no positive finite pivots
__device__ __forceinline__ bool multi_inverse(MultiSmem& s, const int P) {
    double* X = &s.ch[0][0];
    const bool cov = factor(s, P, 0.0);
    if (cov) {
        for (int c = 0; c < P; ++c) {
            X[c * P + c] = 1.0 / s.L[c][c];
            for (int i = c + 1; i < P; ++i) {
                double q = 0.0;
                for (int k = c; k < i; ++k) q -= s.L[i][k] * X[k * P + c];
                X[i * P + c] = q / s.L[i][i];
            }
        }
    }
    return cov;
}

// thread 0: the BLEND_FIELDS = 36 fields of member t's row at o; C_ij = sum_k>=j X_ki X_kj, only the member's own 6 x 6 block
__device__ __forceinline__ void multi_row(const MultiSmem& s, const int P, const int M, const int t, const bool cov, const int status, const int niter,
                                          const unsigned np, const double lam, const int group, double* o) {
    const double* X = &s.ch[0][0];
    o[0] = (double)status; o[1] = (double)niter; o[2] = (double)np; o[3] = s.cur[0]; o[4] = lam;
    o[5] = (double)group; o[6] = (double)M; o[7] = (double)t;
    for (int k = 0; k < 6; ++k) o[8 + k] = s.p[6 * t + k];
    o[14] = cov ? 1.0 : 0.0;
    int f = 15;
    for (int ii = 6 * t; ii < 6 * t + 6; ++ii)
        for (int jj = ii; jj < 6 * t + 6; ++jj) {
            double c = 0.0;
            if (cov)
                for (int k = jj; k < P; ++k) c += X[k * P + ii] * X[k * P + jj];
            o[f++] = c;
        }
}

}  // namespace
}  // namespace cy
