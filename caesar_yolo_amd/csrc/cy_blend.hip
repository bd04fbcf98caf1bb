// Joint fits of blends (cy_fit_blends): the sum of M <= BLEND_MAX_MEMBERS elliptical Gaussians fitted to the union of the basins of
// a group of touching components, unweighted Levenberg-Marquardt in float64 (definitions: include/caesar_yolo_hip.h, DESIGN.md
// "Joint fits of blends").
//   model    m = sum_s A_s exp(-q_s / 2), every member as in cy_fit.hip; p = M x (A, x0, y0, a, b, c), P = 6 M parameters, x0 / y0
//            relative to the window's first pixel in here (the runtime converts from and to image pixels)
//   sweep    per list entry the vector w = (r, J_0 .. J_{P-1}), P + 1 numbers; the sums are the upper triangle of w^T w in row-major
//            order: F = w_0 w_0, g_i = w_0 w_{1+i}, H_ij = w_{1+i} w_{1+j}: NS = (P + 1)(P + 2) / 2 <= 325 float64 sums
//   step     thread 0: P x P Cholesky of H + lambda diag(H) in LDS, d, `small`, admissibility of p + d; everyone: sweep at the trial;
//            thread 0: accept / reject, lambda, convergence (lm_iterate of cy_lm.h, which states the rule and owns the loop), and
//            at the end inv(H)
// One workgroup of 256 threads owns one job of the job table from start to finish; no workgroup reads what another one wrote.  The
// job's pixels arrive as a list of window indices in increasing order, built by the runtime from the mask: the kernel never searches
// a window.  A list entry whose pixel is not valid (0 or non-finite) keeps its list position and contributes nothing (its w is 0).
// Ownership is by SUM, not by pixel: thread t owns sums t and t + 256 and adds them over the whole list, so every sum is one plain
// sequential float64 sum in increasing list position: no reduction, no shuffle, no atomic, and two runs give the same bits.  The
// list is worked in chunks of BLEND_CHUNK = 128 entries: thread e < 128 computes w of chunk entry e (M exp) into LDS row e, 25
// doubles apart (50 dwords: the 16 lanes of a 64-bit store group fall on 16 different bank pairs, and in the adding phase every
// lane reads row e at its own two columns: distinct banks or a broadcast); after a barrier every thread adds its two products per
// chunk entry.  A job of at most FIT_LDS_MAX list entries keeps {value, index} of every entry in LDS, a larger one re-reads list and
// image, which L2 serves from the second sweep on.
// Every loop has a bound fixed before it starts:
//   iteration   it = 1 .. max_iter (<= FIT_MAX_ITER = 256); every lambda escalation is one iteration, so there is no inner loop
//   sweeps      at most max_iter + 1 per job; chunks ceil(npos / 128), npos <= 2^24; per chunk <= 128 entries, M <= 4 members each
//   pair        the (row, column) of a sum index: at most P + 1 = 25 steps, once per job
//   thread 0    Cholesky, the two triangular solves, the inverse of L and the members' blocks of inv(H): nested loops over P <= 24
#include "cy_lm.h"                      // gauss_terms, stage_list, lm_iterate

#pragma clang fp contract(off)          // every product is rounded before it is added, as the float64 definition does

namespace cy {
namespace {

constexpr int BL_T = 256;
constexpr int BL_PMAX = 6 * BLEND_MAX_MEMBERS, BL_WMAX = BL_PMAX + 1;       // 24 parameters, 25 numbers per list entry
static_assert(BLEND_NSUM_MAX == BL_WMAX * (BL_WMAX + 1) / 2 && BLEND_NSUM_MAX <= 2 * BL_T, "two sums per thread cover every sum");
static_assert(BL_PMAX * BL_PMAX <= BLEND_CHUNK * BL_WMAX, "the inverse of L reuses the chunk rows");

struct BSmem {
    float val[FIT_LDS_MAX];
    unsigned idx[FIT_LDS_MAX];
    double ch[BLEND_CHUNK][BL_WMAX];    // w of the chunk's entries; after the fit: inv(L), row-major P x P
    double tot[BLEND_NSUM_MAX];         // sums of the last sweep
    double cur[BLEND_NSUM_MAX];         // sums at the accepted p
    double L[BL_PMAX][BL_PMAX];         // thread 0's Cholesky factor
    double p[BL_PMAX], pt[BL_PMAX], z[BL_PMAX], d[BL_PMAX];
    RedSlots<BL_T, 1> cnt;              // stage_list's
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
    for (int k = 0; k < BL_WMAX; ++k) {
        if (q < n - r) break;
        q -= n - r; ++r;
    }
    *a = r; *b = r + q;
}

// the sums at pp (LDS, uniform) over the job's list; they land in s.tot (visible to everyone after the barrier at the end)
template <bool LDS>
__device__ __forceinline__ void sweep(BSmem& s, const double* pp, const int M, const unsigned* __restrict__ list, const unsigned npos,
                                      const float* __restrict__ img, const size_t MW, const unsigned W, const unsigned A, const double bkg,
                                      const int a1, const int b1, const int a2, const int b2, const int nsum) {
    const int tid = threadIdx.x;
    double acc1 = 0.0, acc2 = 0.0;
    for (unsigned base = 0; base < npos; base += BLEND_CHUNK) {
        const unsigned cnt = npos - base < (unsigned)BLEND_CHUNK ? npos - base : (unsigned)BLEND_CHUNK;
        if ((unsigned)tid < cnt) {
            const unsigned q = base + tid;
            unsigned i; float fv;
            if (LDS) { i = s.idx[q]; fv = s.val[q]; }
            else i = list_pixel(list, q, img, MW, W, A, fv);
            double* w = s.ch[tid];
            if (i == LM_BAD) {
                for (int k = 0; k <= 6 * M; ++k) w[k] = 0.0;
            } else {
                const unsigned dy = i / W, dx = i - dy * W;
                const double y = (double)fv - bkg;
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
            acc1 += w[a1] * w[b1];
            acc2 += w[a2] * w[b2];
        }
        __syncthreads();
    }
    if (tid < nsum) s.tot[tid] = acc1;
    if (tid + BL_T < nsum) s.tot[tid + BL_T] = acc2;
    __syncthreads();
}

// thread 0: the Cholesky factor of H + lam diag(H) into s.L (row by row, every inner sum subtracted term by term in increasing k);
// false on a pivot that is not positive and finite
__device__ bool factor(BSmem& s, const int P, const double lam) {
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
__device__ bool lm_solve(BSmem& s, const int P, const double lam) {
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
    const int M = j.M, P = 6 * M, nsum = (P + 1) * (P + 2) / 2;
    const double bkg = j.bkg;

    if (tid < P) { s.p[tid] = j.p0[tid]; s.pt[tid] = j.p0[tid]; }
    if (tid == 0) { s.ctl.act = ACT_NONE; s.ctl.stop = 0; }
    const unsigned np = stage_list<BL_T, LDS>(s.val, s.idx, s.cnt, list, npos, img, MW, W, A);       // the barrier is inside

    const int early = !admissible_all(j.p0, M) ? 4 : np < (unsigned)(P + 1) ? 3 : 0;     // uniform
    if (early) { early_rows(j, a, early, np); return; }

    int a1, b1, a2, b2;
    pair_of(tid, P + 1, &a1, &b1);
    pair_of(tid + BL_T, P + 1, &a2, &b2);

    // ---- sums at the start
    sweep<LDS>(s, s.pt, M, list, npos, img, MW, W, A, bkg, a1, b1, a2, b2, nsum);
    for (int k = tid; k < nsum; k += BL_T) s.cur[k] = s.tot[k];
    __syncthreads();
    double lam;
    int status, niter;
    lm_iterate(s.ctl, a.max_iter, lam, status, niter,
               [&](const double lam, bool& small) {
                   if (!lm_solve(s, P, lam)) return false;
                   small = lm_trial(P, s.p, s.d, s.pt);
                   return admissible_all(s.pt, M);
               },
               [&] { sweep<LDS>(s, s.pt, M, list, npos, img, MW, W, A, bkg, a1, b1, a2, b2, nsum); },
               [&] { return s.cur[0]; }, [&] { return s.tot[0]; },
               [&] {
                   for (int k = 0; k < nsum; ++k) s.cur[k] = s.tot[k];
                   for (int k = 0; k < P; ++k) s.p[k] = s.pt[k];
               });
    if (tid != 0) return;
    // ---- thread 0: C = inv(H) at the reported p through H = L L^T, X = inv(L) column by column, C_ij = sum_k>=j X_ki X_kj
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
    for (int t = 0; t < M; ++t) {
        double* o = a.out + ((size_t)j.row0 + j.comp[t]) * BLEND_FIELDS;
        o[0] = (double)status; o[1] = (double)niter; o[2] = (double)np; o[3] = s.cur[0]; o[4] = lam;
        o[5] = (double)j.comp[0]; o[6] = (double)M; o[7] = (double)t;
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
