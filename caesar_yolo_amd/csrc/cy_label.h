// Labelling of one box window, shared by the island step (cy_islands.hip) and the component step (cy_deblend.hip): sweeps 1-4 of
// the island step's header comment (init, link, flatten, seed flag).  One workgroup of 256 threads owns the window; labels are
// one u32 per pixel (index i = dy * W + dx) in LDS or in the workgroup's slice of the per-call workspace.  After label_window():
//   label(i) == NOLAB            i is no candidate
//   label(i) & ROOT              smallest pixel index of i's component (the component's root)
//   label(root) & SEEDED         the component holds a seed: it belongs to the island set
// Every loop has a bound fixed before it starts: sweeps run over the A pixels of the window, a walk to the root follows strictly
// decreasing labels (at most A steps), and unite() lowers the larger of its two roots with every retry (at most A retries).
// Workspace labels are read and written with agent-scope atomics (they go to L2, never to a stale line of the vector cache).
#pragma once
#include "cy_px.h"                      // valid_px, Win, window_of
#include "cy_reduce.h"                  // RedSlots, reduction
#include <climits>

#pragma clang fp contract(off)          // as in both files that include this one (Moments::add)

namespace cy {
namespace {

constexpr int INT = 256;
constexpr unsigned NOLAB = 0xFFFFFFFFu, SEEDED = 0x80000000u, ROOT = 0x7FFFFFFFu;
static_assert(ISL_MAX_AREA < (long long)SEEDED, "bit 31 of a label is the seed flag");

using LabRed = RedSlots<INT, 3>;        // reduction scratch of label_window: the seed count and the peak pixel

// The moments of the weights wt at window position (fx, fy), as islands and components carry them: S, Sx, Sy, Sxx, Syy, Sxy.  Every
// product is rounded before it is added, and fx * fx before it meets wt, as the float64 definition does
struct Moments {
    double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    __device__ __forceinline__ void add(const double wt, const double fx, const double fy) {
        m[0] += wt; m[1] += wt * fx; m[2] += wt * fy;
        m[3] += wt * (fx * fx); m[4] += wt * (fy * fy); m[5] += wt * (fx * fy);
    }
    __device__ __forceinline__ void store(double* out) const {
#pragma unroll
        for (int k = 0; k < 6; ++k) out[k] = m[k];
    }
};

// label accesses: LDS (workgroup scope) or this workgroup's slice of the global workspace (agent scope: served by L2)
template <bool LDS> struct Lab {
    static constexpr int SC = LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
    unsigned* p;
    __device__ __forceinline__ unsigned ld(unsigned i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, SC); }
    __device__ __forceinline__ void st(unsigned i, unsigned v) const { __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, SC); }
    __device__ __forceinline__ unsigned amin(unsigned i, unsigned v) const { return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, SC); }
    __device__ __forceinline__ void aor(unsigned i, unsigned v) const { __hip_atomic_fetch_or(p + i, v, __ATOMIC_RELAXED, SC); }
    __device__ __forceinline__ unsigned root(unsigned a, unsigned A) const {        // labels only decrease along the walk
        for (unsigned k = 0; k < A; ++k) { const unsigned q = ld(a); if (q == a) break; a = q; }
        return a;
    }
    __device__ __forceinline__ void unite(unsigned a, unsigned b, unsigned A) const {
        for (unsigned k = 0; k < A; ++k) {
            a = root(a, A); b = root(b, A);
            if (a == b) return;
            if (a < b) { const unsigned t = a; a = b; b = t; }
            const unsigned old = amin(a, b);            // a was a root when read: hang it under b
            if (old == a) return;
            a = old;                                    // somebody re-hung a under `old` first: old and b still have to meet
        }
    }
};

// Sweeps 1-4.  img: first pixel of the window, MW: row pitch of the image.  -> the number of seeds; pv / pi: the window's peak
// pixel (largest valid pixel, first in row-major order; pi == NOLAB when there is no valid pixel).  No seed: returns 0 right
// after sweep 1 (uniformly: the count comes from LDS) and the labels are not linked.  Otherwise it ends with a __syncthreads().
template <bool LDS>
__device__ __forceinline__ unsigned label_window(LabRed& s, const Lab<LDS> L, const float* __restrict__ img, const size_t MW, const bool c8,
                                                 const Win wn, const double seed, const double merge, float& pv, unsigned& pi) {
    const int tid = threadIdx.x, lane = tid & 63;
    const unsigned W = wn.W, A = wn.A;

    // ---- 1 init
    unsigned nseed = 0;
    pv = -INFINITY; pi = NOLAB;
    for (unsigned base = 0; base < A; base += INT) {          // uniform trip count: every lane takes part in the ballots
        const unsigned i = base + tid, dy = i / W, dx = i - dy * W;
        const float v = i < A ? img[(size_t)dy * MW + dx] : 0.0f;
        const bool ok = valid_px(v), cand = ok && (double)v >= merge;
        if (ok && v > pv) { pv = v; pi = i; }                  // increasing index per lane: the first stays
        nseed += cand && (double)v >= seed;
        const unsigned long long m = __ballot(cand);
        const bool joins = cand && lane > 0 && dx > 0 && ((m >> (lane - 1)) & 1ull);
        const unsigned long long starts = __ballot(cand && !joins);
        if (i < A) L.st(i, cand ? i - lane + (63u - (unsigned)__clzll((long long)(starts & (~0ull >> (63 - lane))))) : NOLAB);
    }
    const auto red = reduction(red_sum(nseed), red_first_max(pv, pi, NOLAB));
    red.wave();
    red.park(s);
    __syncthreads();                                          // also: the labels of sweep 1 are in place
    red.total(s);                                             // every thread
    if (nseed == 0) return 0;

    // ---- 2 link
    for (unsigned i = tid; i < A; i += INT) {
        if (L.ld(i) == NOLAB) continue;
        const unsigned dy = i / W, dx = i - dy * W;
        const bool left = dx > 0 && L.ld(i - 1) != NOLAB;
        if (left && (i & 63u) == 0) L.unite(i, i - 1, A);      // the run continues across the 64-pixel boundary of sweep 1
        if (dy == 0) continue;
        const unsigned u = i - W;
        const bool up = L.ld(u) != NOLAB, ul = dx > 0 && L.ld(u - 1) != NOLAB;
        if (up) {
            if (!(left && ul)) L.unite(i, u, A);               // left && ul: the left neighbour is linked to ul, which is in up's run
        } else if (c8) {
            if (ul && !left) L.unite(i, u - 1, A);             // left: ul is the left neighbour's `up`
            if (dx + 1 < W && L.ld(u + 1) != NOLAB) L.unite(i, u + 1, A);
        }
    }
    __syncthreads();

    // ---- 3 flatten
    for (unsigned i = tid; i < A; i += INT)
        if (L.ld(i) != NOLAB) L.st(i, L.root(i, A));
    __syncthreads();

    // ---- 4 seeds
    for (unsigned i = tid; i < A; i += INT) {
        const unsigned l = L.ld(i);
        if (l == NOLAB) continue;
        const unsigned dy = i / W, dx = i - dy * W;
        if ((double)img[(size_t)dy * MW + dx] >= seed && !(L.ld(l & ROOT) & SEEDED)) L.aor(l & ROOT, SEEDED);
    }
    __syncthreads();
    return nseed;
}

}  // namespace
}  // namespace cy
