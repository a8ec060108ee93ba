// What the row-selection kernels share (decode_select.hip, decode_sample.hip): the workgroup shape, the mask bits of a column, the walk over
// a row's 16-byte vectors, and the unsigned order of the stored values.
#pragma once
#include "common_hip.h"
#include <math.h>

namespace {

constexpr int SEL_THREADS = 256, SEL_WAVES = SEL_THREADS / 64, SEL_UNROLL = 8;
constexpr float SEL_LOG2E = 1.44269504088896340736f;

// Is `b` (value, column) better than `a`?  A column of -1 is "none yet"; the lower column wins between equal values.
__device__ __forceinline__ bool sel_better(float av, int ai, float bv, int bi) {
    return bi >= 0 && (ai < 0 || bv > av || (bv == av && bi < ai));
}

// bits c % 32 .. c % 32 + n - 1 of word c / 32 (n <= 8 and c % n == 0: one word); NULL = every column
__device__ __forceinline__ uint32_t sel_mask_bits(const uint32_t* __restrict__ mask, int c) {
    return mask ? mask[c >> 5] >> (c & 31) : 0xffffffffu;
}

// One walk over the 16-byte vectors v = tid, tid + 256, ... < nvec of a row, SEL_UNROLL vectors per trip, each with the mask bits of its
// columns.  The loads of the NEXT trip are issued before the current one is worked on (one wave per SIMD: nothing else hides the latency),
// and they are UNCONDITIONAL, their index clamped to the last vector: behind a guard hipcc waits for every load in flight before the next
// use.  Whole trips run without a predicate; the last, partial one tests v < nvec around work that touches no memory.  f(first column,
// vector, mask bits from that column on) sees a thread's vectors in rising order.
template <typename T, bool MASKED, int UNROLL = SEL_UNROLL, typename F>
__device__ __forceinline__ void sel_walk(const T* __restrict__ x, const uint32_t* __restrict__ mask, int nvec, int tid, F&& f) {
    constexpr int VEC = Vec16<T>::N, TRIP = SEL_THREADS * UNROLL;
    if (nvec <= 0) return;
    Vec16<T> cur[UNROLL], nxt[UNROLL];
    uint32_t cur_bits[UNROLL], nxt_bits[UNROLL];
    auto fetch = [&](Vec16<T>* q, uint32_t* b, int v0) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int v = min(v0 + u * SEL_THREADS, nvec - 1);
            q[u] = load16<T>(x + (int64_t)v * VEC);
            b[u] = MASKED ? mask[(v * VEC) >> 5] >> ((v * VEC) & 31) : 0xffffffffu;
        }
    };
    fetch(cur, cur_bits, tid);
    int v0 = tid;
    for (int t = nvec / TRIP; t > 0; --t, v0 += TRIP) {
        fetch(nxt, nxt_bits, v0 + TRIP);
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) f((v0 + u * SEL_THREADS) * VEC, cur[u], cur_bits[u]);
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            cur[u] = nxt[u];
            cur_bits[u] = nxt_bits[u];
        }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
        const int v = v0 + u * SEL_THREADS;
        if (v < nvec) f(v * VEC, cur[u], cur_bits[u]);
    }
}

// The key of a value orders the stored numbers as unsigned integers: NaN below every number, -0 with +0, nothing at 0 (an empty place).
__device__ __forceinline__ uint32_t topk_key(float f) {
    const uint32_t b = __float_as_uint(f);
    uint32_t k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    k = f == 0.f ? 0x80000000u : k;
    return f != f ? 1u : k;
}

}  // namespace
