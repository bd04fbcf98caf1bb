// Exact median by radix selection, shared by the ring of cy_measure.hip and the cell of cy_background.hip.  The members are the
// floats a `walk` hands out; the selection orders them by a 64-bit key, 8 bits per pass, 256-bin histogram in LDS:
//   MODE 0  pixels      fkey32(v) in the high word                                  -> 4 passes
//   MODE 1  deviations  bit pattern of the non-negative float64 d = |v - centre|    -> 8 passes
// It finds the element of rank (n - 1) / 2 and how many elements are <= it; for an even n the upper middle element is the same
// value when that count exceeds n / 2, else the smallest larger key (one more pass), and the median is the float64 mean of the two.
// Counts and single rounded operations only: nothing depends on the order in which the walk visits the members.  The LDS atomics
// are integer counts.  A workgroup of NT >= 256 threads; the first 256 own one bin each.
#pragma once
#include "cy_reduce.h"                  // RedSlots, reduction: the minimum at the end

#pragma clang fp contract(off)          // as in every file that includes this one

namespace cy {
namespace {

__device__ __forceinline__ unsigned fkey32(float f) {                   // order-preserving float -> u32 (fkey of cy_preproc.hip)
    const unsigned b = __float_as_uint(f);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float fkey32_inv(unsigned k) { return __uint_as_float((k >> 31) ? (k & 0x7FFFFFFFu) : ~k); }

template <int MODE> __device__ __forceinline__ unsigned long long sel_key(float v, double centre) {
    if constexpr (MODE == 0) return (unsigned long long)fkey32(v) << 32;
    else return (unsigned long long)__double_as_longlong(fabs((double)v - centre));      // d >= 0: orders like its bit pattern
}
template <int MODE> __device__ __forceinline__ double key_value(unsigned long long k) {
    if constexpr (MODE == 0) return (double)fkey32_inv((unsigned)(k >> 32));
    else return __longlong_as_double((long long)k);
}

template <int NT> struct SelSmem {
    unsigned hist[256];
    unsigned wsum[4];
    unsigned sel[4];                     // digit, rank inside the bin, elements below the bin, elements in the bin
    RedSlots<NT, 1> umin;
};

// Exact median of the keys of the members; n = their count (0: returns 0).  n == stop_at: returns 0 after the counting pass (the
// caller keeps the median it has).  walk(f) calls f(v) for every member, the same members in every call, every thread of the
// workgroup taking part.  Every thread gets the same result.
template <int MODE, int NT, typename Walk>
__device__ double select_median(SelSmem<NT>& s, Walk walk, const double centre, const unsigned stop_at, unsigned& n) {
    static_assert(NT >= 256 && NT % 64 == 0, "one thread per bin, whole waves");
    constexpr int NP = MODE == 0 ? 4 : 8;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool bin = NT == 256 || tid < 256;                // this thread owns histogram bin `tid`
    unsigned long long prefix = 0;
    unsigned k = 0, below = 0, eq = 0;
    n = 0;
    for (int p = 0; p < NP; ++p) {
        const int shift = 56 - 8 * p;
        if (bin) s.hist[tid] = 0;
        __syncthreads();
        const unsigned long long want = p ? prefix >> (shift + 8) : 0;
        walk([&](float v) {
            const unsigned long long key = sel_key<MODE>(v, centre);
            if (p == 0 || (key >> (shift + 8)) == want) atomicAdd(&s.hist[(unsigned)(key >> shift) & 255u], 1u);
        });
        __syncthreads();
        const unsigned h = bin ? s.hist[tid] : 0u;
        unsigned incl = h;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        if (bin && lane == 63) s.wsum[w] = incl;
        __syncthreads();
        unsigned off = 0, total = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { const unsigned t = s.wsum[j]; if (j < w) off += t; total += t; }
        if (p == 0) {
            n = total;
            if (n == 0 || n == stop_at) return 0.0;         // uniform: `total` came from LDS
            k = (n - 1) / 2;
        }
        const unsigned excl = off + incl - h;
        if (bin && k >= excl && k < excl + h) { s.sel[0] = (unsigned)tid; s.sel[1] = k - excl; s.sel[2] = excl; s.sel[3] = h; }
        __syncthreads();
        prefix |= (unsigned long long)s.sel[0] << shift;
        k = s.sel[1]; below += s.sel[2]; eq = s.sel[3];
    }
    const double a = key_value<MODE>(prefix);
    if ((n & 1u) || below + eq > n / 2) return a;           // odd count, or the upper middle element has the same value
    unsigned long long m = ~0ull;                           // smallest key above `prefix`
    walk([&](float v) { const unsigned long long key = sel_key<MODE>(v, centre); if (key > prefix && key < m) m = key; });
    const auto red = reduction(red_min(m));
    red.wave();
    red.park(s.umin);
    __syncthreads();
    red.total(s.umin);                                      // every thread
    return (a + key_value<MODE>(m)) / 2.0;
}

}  // namespace
}  // namespace cy
