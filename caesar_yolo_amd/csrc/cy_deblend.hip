// Source components (cy_deblend_islands): per source box, the island set of cy_measure_islands split into components by local
// peaks and steepest-ascent basins (definitions: include/caesar_yolo_hip.h, DESIGN.md "Source components").
//   rank     p outranks q when v(p) > v(q), or v(p) == v(q) and i(p) < i(q) (i = dy * W + dx): a total order on valid pixels
//   up(p)    the highest-ranked of p and its conn neighbours that are candidates inside the window;  summit  up(p) == p
//   basin    the pixels whose up-path ends at one summit
//   peak     a summit that outranks every island-set pixel of its own component within |dx|, |dy| <= radius and either has
//            (double)v >= peak_thr or is the top-ranked pixel of its component
//   kept     the first DBL_MAX_COMP peaks in rank order: components 0 .. ncomp - 1.  The basin of any other summit goes to the
//            kept peak of the same island at the smallest integer squared distance (ties: lower component); none: unassigned
// One workgroup of 256 threads owns one source from start to finish; no workgroup reads what another one wrote.  Two u32 per pixel
// of the window, both in LDS when the window has at most ISL_LDS_MAX pixels, else both in the workgroup's slices of the per-call
// workspace: the label of the island step (cy_label.h, sweeps 1-4) and the `up` word U.  An island-set pixel's U holds a pixel
// index in bits 0-23 (up(p), after sweep 6 p's summit); a summit's own U carries flags and, after sweep 11, its component in bits
// 24-30.  Every other pixel's U is NOLAB.  The root of a seeded component is known by bit 31 of its own label; bits 0-30 of that
// label carry the "holds a peak at or above peak_thr" flag and, in sweep 8, the payload of the top-of-component minimum.
// Sweeps after the labelling:
//   5 up       U = up(p) from the image and the labels
//   6 resolve  pointer doubling U(p) = U(U(p)) in place (every value ever stored at p is an ancestor of p on its path) until a
//              workgroup-wide "changed" flag stays clear: a pointer covers at least min(2^k, path length) steps after k rounds
//   7 local    summits that pass the radius test are flagged; those at or above peak_thr are peaks and flag their root
//   8 tops     only when a flagged summit below peak_thr sits in a component whose root has no flag (such a component has no
//              pixel at or above peak_thr, so its top-ranked pixel is its only peak): that pixel is found with two integer
//              minima per root, on the upper 30 bits of the inverted order key of v, then on {lower 2 bits, pixel index}
//   9 count    summits and peaks (integer reduction)
//  10 select   up to DBL_MAX_COMP workgroup arg-max reductions over the peaks, each "the highest rank below the previous pick"
//  11 assign   every summit's component: its own if kept, else the nearest kept peak of the same root, else unassigned
//  12 sums     one pass per component: counts, moments and mask bytes; the first pass also counts the island set and the
//              unassigned pixels
// Every loop has a bound fixed before it starts: the labelling as cy_label.h states; sweeps run over the A pixels of the window;
// sweep 5 looks at 8 neighbours; sweep 6 makes at most DBL_ROUNDS = 26 rounds (A <= 2^24: 24 rounds resolve every path, one more
// sees no change); sweep 7 looks at (2 radius + 1)^2 <= 289 pixels per summit; sweeps 10-12 make at most DBL_MAX_COMP passes with
// at most DBL_MAX_COMP kept peaks per summit.  There is no per-pixel walk along `up`.
// Sums: float64 per lane over increasing pixel index, then the block reduction of cy_reduce.h, finished by thread 0.  The atomics
// are integer minima / ors on labels only.
#include "cy_label.h"

#pragma clang fp contract(off)          // w * (dx * dx) is rounded before it is added, as the float64 definition does

namespace cy {
namespace {

constexpr int DBL_ROUNDS = 26;
constexpr unsigned IDX = 0x00FFFFFFu;                                   // pixel index of a U word
constexpr unsigned LOCAL = 1u << 28, CONT = 1u << 29, PEAK = 1u << 30;  // flags of a summit's own U word (sweeps 7-10)
constexpr unsigned CODE_SHIFT = 24, CODE_MASK = 0x1Fu, UNASSIGNED = 0x1Fu;   // from sweep 11: component + 1, or UNASSIGNED
constexpr unsigned HASPK = 1u << 30, PAY = 0x3FFFFFFFu;                 // a seeded root's own label: flag, payload of sweep 8
static_assert(ISL_MAX_AREA <= (long long)IDX + 1, "a pixel index has 24 bits");
static_assert(DBL_MAX_COMP < (int)UNASSIGNED, "component + 1 fits below UNASSIGNED");

struct DSmem {
    unsigned lab[ISL_LDS_MAX];
    unsigned up[ISL_LDS_MAX];
    LabRed lr;                          // the labelling, then the counts of sweep 9
    RedSlots<INT, 10> red[2];           // sweeps 10 and 12: buffer k & 1 of pass k
    unsigned kidx[DBL_MAX_COMP], kroot[DBL_MAX_COMP]; float kval[DBL_MAX_COMP];
    volatile unsigned chg[3], need;
};

__device__ __forceinline__ unsigned root_of(unsigned i, unsigned l) { return (l & SEEDED) ? i : l; }      // l: label of i, not NOLAB
// order-preserving map of a finite non-zero float to u32, inverted: the highest value has the smallest key
__device__ __forceinline__ unsigned inv_key(float v) {
    const unsigned u = __float_as_uint(v);
    return ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}

template <bool LDS>
__device__ void deblend(DSmem& s, const Lab<LDS> L, const Lab<LDS> U, const DeblendArgs& a, const Win wn, const double seed,
                        const double merge, const double bkg, const double pthr, unsigned char* __restrict__ mask,
                        double* __restrict__ out, double* __restrict__ comp) {
    const int tid = threadIdx.x;
    const size_t MW = (size_t)a.MW;
    const float* __restrict__ img = a.img + (size_t)wn.y0 * MW + (size_t)wn.x0;
    const unsigned W = wn.W, H = wn.H, A = wn.A;
    const bool c8 = a.conn == 8;
    const int R = a.radius;

    // ---- 1-4 init, link, flatten, seeds (cy_label.h)
    float pv; unsigned pi;
    const unsigned nseed = label_window<LDS>(s.lr, L, img, MW, c8, wn, seed, merge, pv, pi);
    if (nseed == 0) {                                         // uniform (from LDS): no island; mask and component rows are 0 already
        if (tid < DBL_FIELDS) out[tid] = 0.0;
        return;
    }

    // ---- 5 up
    for (unsigned i = tid; i < A; i += INT) {
        const unsigned l = L.ld(i);
        unsigned best = NOLAB;
        if (l != NOLAB && ((l & SEEDED) || (L.ld(l) & SEEDED))) {
            const unsigned dy = i / W, dx = i - dy * W;
            float bv = img[(size_t)dy * MW + dx];
            best = i;
#pragma unroll
            for (int ddy = -1; ddy <= 1; ++ddy)
#pragma unroll
                for (int ddx = -1; ddx <= 1; ++ddx) {
                    if ((ddx == 0 && ddy == 0) || (!c8 && ddx != 0 && ddy != 0)) continue;
                    const int yy = (int)dy + ddy, xx = (int)dx + ddx;
                    if (yy < 0 || xx < 0 || yy >= (int)H || xx >= (int)W) continue;
                    const unsigned j = (unsigned)yy * W + (unsigned)xx;
                    if (L.ld(j) == NOLAB) continue;
                    const float vj = img[(size_t)yy * MW + (unsigned)xx];
                    if (vj > bv || (vj == bv && j < best)) { bv = vj; best = j; }
                }
        }
        U.st(i, best);
    }
    if (tid < 3) s.chg[tid] = 0;
    if (tid == 3) s.need = 0;
    __syncthreads();

    // ---- 6 resolve
    for (int r = 0; r < DBL_ROUNDS; ++r) {
        bool ch = false;
        for (unsigned i = tid; i < A; i += INT) {
            const unsigned u = U.ld(i);
            if (u == NOLAB) continue;
            const unsigned uu = U.ld(u);
            if (uu != u) { U.st(i, uu); ch = true; }
        }
        if (ch) s.chg[r % 3] = 1;
        if (tid == 0) s.chg[(r + 1) % 3] = 0;                 // the next round's flag: last read before the previous barrier
        __syncthreads();
        if (!s.chg[r % 3]) break;                             // uniform (from LDS)
    }

    // ---- 7 local
    for (unsigned i = tid; i < A; i += INT) {
        if (U.ld(i) != i) continue;                           // summits only
        const unsigned dy = i / W, dx = i - dy * W;
        const float v = img[(size_t)dy * MW + dx];
        const unsigned rt = root_of(i, L.ld(i));
        const int ya = max((int)dy - R, 0), yb = min((int)dy + R, (int)H - 1), xa = max((int)dx - R, 0), xb = min((int)dx + R, (int)W - 1);
        bool top = true;
        for (int yy = ya; yy <= yb && top; ++yy)
            for (int xx = xa; xx <= xb; ++xx) {
                const unsigned q = (unsigned)yy * W + (unsigned)xx;
                const float vq = img[(size_t)yy * MW + (unsigned)xx];
                if (!(vq > v || (vq == v && q < i))) continue;
                const unsigned lq = L.ld(q);
                if (lq != NOLAB && root_of(q, lq) == rt) { top = false; break; }
            }
        if (!top) continue;
        if ((double)v >= pthr) {
            U.st(i, i | LOCAL | PEAK);
            if (!(L.ld(rt) & HASPK)) L.aor(rt, HASPK);
        } else {
            U.st(i, i | LOCAL);
        }
    }
    __syncthreads();

    // ---- 8 tops
    for (unsigned i = tid; i < A; i += INT) {
        const unsigned u = U.ld(i);
        if (u == NOLAB || (u & IDX) != i || !(u & LOCAL) || (u & PEAK)) continue;
        if (L.ld(root_of(i, L.ld(i))) & HASPK) continue;
        U.st(i, u | CONT);                                    // a contender for the top of its component
        s.need = 1;
    }
    __syncthreads();
    if (s.need) {                                             // uniform (from LDS)
        for (int pass = 0; pass < 2; ++pass) {
            for (unsigned i = tid; i < A; i += INT) {         // the roots without a flag hold the neutral payload
                const unsigned l = L.ld(i);
                if (l != NOLAB && (l & SEEDED) && !(l & HASPK)) L.st(i, SEEDED | PAY);
            }
            __syncthreads();
            for (unsigned i = tid; i < A; i += INT) {
                const unsigned u = U.ld(i);
                if (u == NOLAB || (u & IDX) != i || !(u & CONT)) continue;
                const unsigned dy = i / W, dx = i - dy * W;
                const unsigned key = inv_key(img[(size_t)dy * MW + dx]);
                L.amin(root_of(i, L.ld(i)), SEEDED | (pass == 0 ? key >> 2 : ((key & 3u) << 24) | i));
            }
            __syncthreads();
            for (unsigned i = tid; i < A; i += INT) {
                const unsigned u = U.ld(i);
                if (u == NOLAB || (u & IDX) != i || !(u & CONT)) continue;
                const unsigned dy = i / W, dx = i - dy * W;
                const unsigned key = inv_key(img[(size_t)dy * MW + dx]);
                const unsigned won = L.ld(root_of(i, L.ld(i)));
                if (pass == 0) { if ((won & PAY) != key >> 2) U.st(i, u & ~CONT); }      // a higher value exists: out
                else if ((won & IDX) == i) U.st(i, u | PEAK);
            }
            __syncthreads();
        }
    }

    // ---- 9 count
    unsigned nsum = 0, npk = 0;
    for (unsigned i = tid; i < A; i += INT) {
        const unsigned u = U.ld(i);
        if (u == NOLAB || (u & IDX) != i) continue;
        ++nsum; npk += (u & PEAK) != 0;
    }
    const auto count = reduction(red_sum(nsum), red_sum(npk));
    count.wave();
    count.park(s.lr);                                         // free since the barriers of the labelling; sweep 10 parks in s.red
    __syncthreads();
    count.total(s.lr);                                        // every thread
    const int ncomp = (int)min(npk, (unsigned)DBL_MAX_COMP);

    // ---- 10 select
    float qv = 0.0f; unsigned qi = 0;
    for (int k = 0; k < ncomp; ++k) {
        float bv = 0.0f; unsigned bi = NOLAB;
        for (unsigned i = tid; i < A; i += INT) {
            const unsigned u = U.ld(i);
            if (u == NOLAB || (u & IDX) != i || !(u & PEAK)) continue;
            const unsigned dy = i / W, dx = i - dy * W;
            const float v = img[(size_t)dy * MW + dx];
            if (k > 0 && !(v < qv || (v == qv && i > qi))) continue;       // below the previous pick only
            if (bi == NOLAB || v > bv) { bv = v; bi = i; }                  // increasing index per lane: the first stays
        }
        const auto pick = reduction(red_first_max(bv, bi, NOLAB));
        pick.wave();
        pick.park(s.red[k & 1]);                              // the slower waves may still read the other buffer: pick k - 1
        __syncthreads();
        pick.total(s.red[k & 1]);                             // every thread
        if (bi == NOLAB) bi = 0;                              // cannot happen (k < npeaks); keeps every index below inside the window
        qv = bv; qi = bi;
        if (tid == 0) { s.kidx[k] = bi; s.kval[k] = bv; s.kroot[k] = root_of(bi, L.ld(bi)); }
    }
    __syncthreads();

    // ---- 11 assign
    for (unsigned i = tid; i < A; i += INT) {
        const unsigned u = U.ld(i);
        if (u == NOLAB || (u & IDX) != i) continue;
        const unsigned rt = root_of(i, L.ld(i));
        const long long dy = i / W, dx = i - (unsigned)dy * W;
        unsigned code = UNASSIGNED;
        long long bd = LLONG_MAX;
        for (int t = 0; t < ncomp; ++t) {
            const unsigned kt = s.kidx[t];
            if (kt == i) { code = (unsigned)t + 1; break; }
            if (s.kroot[t] != rt) continue;
            const long long ky = kt / W, kx = kt - (unsigned)ky * W;
            const long long d2 = (dx - kx) * (dx - kx) + (dy - ky) * (dy - ky);
            if (d2 < bd) { bd = d2; code = (unsigned)t + 1; }
        }
        U.st(i, i | (code << CODE_SHIFT));
    }
    __syncthreads();

    // ---- 12 sums (the peak pixel is a seed, so its component is in the island set)
    const unsigned mainroot = root_of(pi, L.ld(pi));
    unsigned ntot = 0, nun = 0;
    for (int k = 0; k < ncomp; ++k) {
        Moments M;
        unsigned np = 0, ns = 0;
        for (unsigned i = tid; i < A; i += INT) {
            const unsigned u = U.ld(i);
            if (u == NOLAB) continue;
            const unsigned si = u & IDX;
            const unsigned code = ((si == i ? u : U.ld(si)) >> CODE_SHIFT) & CODE_MASK;
            if (k == 0) {
                ++ntot;
                if (code == UNASSIGNED) { ++nun; if (mask) mask[i] = 255; }
            }
            if (code != (unsigned)k + 1) continue;
            const unsigned dy = i / W, dx = i - dy * W;
            const double wt = (double)img[(size_t)dy * MW + dx] - bkg, fx = (double)dx, fy = (double)dy;
            M.add(wt, fx, fy);
            ++np; ns += si == i;
            if (mask) mask[i] = (unsigned char)(k + 1);
        }
        unsigned ct = ntot, cu = nun;                         // complete after pass 0; the later passes reduce copies nobody reads
        const auto red = reduction(red_sum(M.m), red_sum(np), red_sum(ns), red_sum(ct), red_sum(cu));
        red.wave();
        red.park(s.red[k & 1]);                               // thread 0 reads buffer k & 1 while the waves fill the other one
        __syncthreads();
        if (tid == 0) {
            red.total(s.red[k & 1]);
            if (k == 0) { ntot = ct; nun = cu; }
            const unsigned kt = s.kidx[k], ky = kt / W, kx = kt - ky * W;
            double* c = comp + (size_t)k * DBL_COMP_FIELDS;
            c[0] = (double)np; c[1] = (double)s.kval[k]; c[2] = (double)(wn.x0 + (int)kx); c[3] = (double)(wn.y0 + (int)ky);
            M.store(c + 4);
            c[10] = s.kroot[k] == mainroot ? 1.0 : 0.0; c[11] = (double)ns;
        }
    }
    if (tid == 0) {
        out[0] = npk > (unsigned)DBL_MAX_COMP ? 2.0 : 0.0; out[1] = (double)nsum; out[2] = (double)npk; out[3] = (double)ncomp;
        out[4] = (double)ntot; out[5] = (double)nun; out[6] = 0.0; out[7] = 0.0;
    }
}

__global__ __launch_bounds__(INT) void deblend_kernel(const DeblendArgs a) {
    __shared__ DSmem s;
    const int b = blockIdx.x, tid = threadIdx.x;
    Win w;
    const long long area = window_of(a.win + (size_t)b * 4, a.MW, a.MH, w);       // held inside the image (cy_px.h)
    double* out = a.out + (size_t)b * DBL_FIELDS;
    const long long wo = a.off[(size_t)b * 2], mo = a.off[(size_t)b * 2 + 1];
    const bool lds = wo < 0;
    if (area == 0 || area > ISL_MAX_AREA || wo == ISL_OFF_TOO_LARGE) {
        // empty window: nothing to measure.  Above the supported maximum: status 1, nothing measured
        if (tid < DBL_FIELDS) out[tid] = tid == 0 && area ? 1.0 : 0.0;
        return;
    }
    if (lds && area > ISL_LDS_MAX) {
        // the host gave no workspace to a window that needs one.  launch_deblend's caller cannot produce this; should it ever
        // happen, nothing is labelled (the LDS arrays would not hold it) and the row is NaN throughout
        if (tid < DBL_FIELDS) out[tid] = __longlong_as_double(0x7FF8000000000000LL);
        return;
    }
    const double* t = a.thr + (size_t)b * 4;
    unsigned char* mask = a.mask ? a.mask + mo : nullptr;
    double* comp = a.comp + (size_t)b * DBL_MAX_COMP * DBL_COMP_FIELDS;
    if (lds) deblend<true>(s, Lab<true>{s.lab}, Lab<true>{s.up}, a, w, t[0], t[1], t[2], t[3], mask, out, comp);
    else deblend<false>(s, Lab<false>{a.ws + wo}, Lab<false>{a.ws_up + wo}, a, w, t[0], t[1], t[2], t[3], mask, out, comp);
}

}  // namespace

hipError_t launch_deblend(const DeblendArgs& a, hipStream_t s) {
    if (a.n < 1 || a.MH < 1 || a.MW < 1 || (a.conn != 4 && a.conn != 8) || a.radius < 1 || a.radius > DBL_RADIUS_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(deblend_kernel, dim3(a.n), dim3(INT), 0, s, a);
    return hipGetLastError();
}

}  // namespace cy
