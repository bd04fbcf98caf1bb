// The block reduction of the measurement kernels (cy_measure, cy_islands, cy_deblend, cy_fit, cy_blend, cy_residual, cy_aperture,
// cy_label.h, cy_lm.h, cy_select.h).  Its association is part of what a catalog number means and stands here once:
//   lane    every thread brings one value per quantity, accumulated in its own fixed order (float64 sums: sequentially over
//           increasing index)
//   wave    six steps with offsets 32, 16, 8, 4, 2, 1: lane l takes lane l + o's value as the right operand, v = v (op) other; after
//           the last step lane 0 holds the wave's result (what the other lanes hold is not used)
//   block   lane 0 of wave w parks its value in slot w; the result is ((slot0 op slot1) op slot2) op slot3, read in that order
// A fixed association, so two runs give the same bits; tests/reduce_ref.py restates it in numpy and tests/test_gpu_reduce.py
// compares bit patterns (cy_debug_reduce).  Slot 0 holds exactly thread 0's register, so total() serves both finishing styles:
// `if (tid == 0) r.total(s)` where thread 0 writes the row, r.total(s) on every thread where all of them need the result.
// Operations: sum, minimum, maximum, and the first maximum, which carries an index.  Its rule, used everywhere: the other side wins
// when it has a candidate (index != none) and this side has none, or the other value is larger, or the values are equal and the
// other index is smaller.  A lane that walks increasing indices keeps its first maximum with `v > best`; none stays none.
// Barriers belong to the caller: wave() has none, park() writes LDS, and a __syncthreads() between park() and total() is the
// caller's (several callers let that barrier do other work too).  Slots are reused by the next park(): the caller also owns the
// barrier between the last total() of one use and the park() of the next (or uses two slot sets in turn).
// Only additions and comparisons in here: nothing that could be contracted, and no contraction pragma either way.
#pragma once
#include "cy_kernels.h"
#include <tuple>

namespace cy {
namespace {

// one 8-byte slot per quantity and wave, whatever the type (double, long long, unsigned long long; float, int, unsigned widened)
template <int NT, int NQ> struct RedSlots {
    static_assert(NT % 64 == 0, "whole waves");
    static constexpr int NW = NT / 64;
    unsigned long long q[NQ][NW];
    template <typename T> __device__ __forceinline__ void put(int i, int w, T v) {
        if constexpr (sizeof(T) == 8) q[i][w] = __builtin_bit_cast(unsigned long long, v);
        else q[i][w] = __builtin_bit_cast(unsigned, v);
    }
    template <typename T> __device__ __forceinline__ T get(int i, int w) const {
        if constexpr (sizeof(T) == 8) return __builtin_bit_cast(T, q[i][w]);
        else return __builtin_bit_cast(T, (unsigned)q[i][w]);
    }
};

struct RedAdd { template <typename T> static __device__ __forceinline__ T op(T a, T b) { return a + b; } };
struct RedMin { template <typename T> static __device__ __forceinline__ T op(T a, T b) { return b < a ? b : a; } };
struct RedMax { template <typename T> static __device__ __forceinline__ T op(T a, T b) { return b > a ? b : a; } };

// K quantities of one type under one operation; v lives in the caller's registers (only constant indices in here)
template <typename F, typename T, int K> struct RedFold {
    static constexpr int NQ = K;
    T* v;
    __device__ __forceinline__ void wave() const {
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v[k] = F::op(v[k], __shfl_down(v[k], o));
    }
    template <typename S> __device__ __forceinline__ void park(S& s, int i, int w) const {
#pragma unroll
        for (int k = 0; k < K; ++k) s.put(i + k, w, v[k]);
    }
    template <typename S> __device__ __forceinline__ void total(const S& s, int i) const {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            T t = s.template get<T>(i + k, 0);
#pragma unroll
            for (int j = 1; j < S::NW; ++j) t = F::op(t, s.template get<T>(i + k, j));
            v[k] = t;
        }
    }
};
template <typename T> __device__ __forceinline__ RedFold<RedAdd, T, 1> red_sum(T& v) { return {&v}; }
template <typename T, int K> __device__ __forceinline__ RedFold<RedAdd, T, K> red_sum(T (&v)[K]) { return {v}; }
template <typename T> __device__ __forceinline__ RedFold<RedMin, T, 1> red_min(T& v) { return {&v}; }
template <typename T> __device__ __forceinline__ RedFold<RedMax, T, 1> red_max(T& v) { return {&v}; }

// the first maximum: value v at index i, i == none when there is no candidate (v is then whatever the caller put there)
template <typename V, typename I> struct RedFirstMax {
    static constexpr int NQ = 2;
    V* v; I* i; I none;
    __device__ __forceinline__ void take(V v2, I i2) const {
        if (i2 != none && (*i == none || v2 > *v || (v2 == *v && i2 < *i))) { *v = v2; *i = i2; }
    }
    __device__ __forceinline__ void wave() const {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const V v2 = __shfl_down(*v, o); const I i2 = __shfl_down(*i, o); take(v2, i2); }
    }
    template <typename S> __device__ __forceinline__ void park(S& s, int k, int w) const { s.put(k, w, *v); s.put(k + 1, w, *i); }
    template <typename S> __device__ __forceinline__ void total(const S& s, int k) const {
        *v = s.template get<V>(k, 0); *i = s.template get<I>(k + 1, 0);
#pragma unroll
        for (int j = 1; j < S::NW; ++j) take(s.template get<V>(k, j), s.template get<I>(k + 1, j));
    }
};
template <typename V, typename I> __device__ __forceinline__ RedFirstMax<V, I> red_first_max(V& v, I& i, I none) { return {&v, &i, none}; }

// everything one place reduces, in one wave step, one park and one total: reduction(red_sum(a), red_min(b), ..)
template <typename... Ops> struct Reduction {
    static constexpr int NQ = (Ops::NQ + ... + 0);
    std::tuple<Ops...> ops;
    __device__ __forceinline__ void wave() const { std::apply([](const Ops&... op) { (op.wave(), ...); }, ops); }
    template <int NT, int N> __device__ __forceinline__ void park(RedSlots<NT, N>& s) const {       // lane 0 of every wave
        static_assert(NQ <= N, "one slot row per quantity");
        if ((threadIdx.x & 63) != 0) return;
        const int w = threadIdx.x >> 6;
        std::apply([&s, w](const Ops&... op) { int i = 0; ((op.park(s, i, w), i += Ops::NQ), ...); }, ops);
    }
    template <int NT, int N> __device__ __forceinline__ void total(const RedSlots<NT, N>& s) const {
        static_assert(NQ <= N, "one slot row per quantity");
        std::apply([&s](const Ops&... op) { int i = 0; ((op.total(s, i), i += Ops::NQ), ...); }, ops);
    }
};
template <typename... Ops> __device__ __forceinline__ Reduction<Ops...> reduction(Ops... ops) { return {std::tuple<Ops...>(ops...)}; }

}  // namespace
}  // namespace cy
