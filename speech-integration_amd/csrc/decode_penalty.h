// Repetition, frequency and presence penalties inside the row-selection kernels (ABI v22; decode_select.hip, decode_sample.hip).
// include/ssi_hip.h states the definition: with H the ids of the row's prompt and of its generated tokens and n_c the occurrences of c
// among the generated ones, the penalised value y_c = fma(x_c, a_c, -t_c) is formed in fp32 from the stored x_c where it is used and
// never stored; a column outside H keeps y_c = x_c without arithmetic.
//
// A workgroup (one row) builds the row's history in dynamic LDS before its first walk:
//   table  Hs (token + 1, count) pairs (first, so that a pair is one aligned 8-byte load), open addressing, slot = token mod Hs, linear probing; Hs = the smallest power of two >= 2 ld_gen,
//          at least 64, so at most half of it is ever taken and a probe ends at an empty slot.  Keys are claimed with atomicCAS, counts
//          added with atomicAdd: the sums are integers, the place a key lands in depends on the order of arrival, a lookup's result not.
//   seen   ceil(vocab / 32) words, bit c % 32 of word c / 32 = "c is in H" (LDS atomicOr);
// A walk reads the seen bits of a 16-byte vector with one LDS load; only where a bit is set does a lane look the column up (O(1) expected).
// An id outside [0, vocab) or a prompt line outside [0, n_prompts) is tested BEFORE any address is formed from it, skipped, and the row is
// counted once in *n_bad: ssi_attn_decode_beam's rule.
#pragma once
#include "decode_walk.h"

namespace {

constexpr int64_t PEN_LDS_MAX = 57344;                    // dynamic LDS of a penalised launch: 64 KB less 8 KB for the kernels' static LDS

static inline int64_t pen_table_slots(int64_t ld_gen) {
    int64_t hs = 64;
    while (hs < 2 * ld_gen) hs <<= 1;
    return hs;
}
static inline int64_t pen_lds_bytes(int64_t vocab, int64_t ld_gen) { return 4 * ((vocab + 31) / 32) + 8 * pen_table_slots(ld_gen); }

struct PenArgs {
    const int32_t* prompt_ids;
    int64_t ld_prompt;
    const int32_t* prompt_len;
    const int32_t* prompt_row;
    int64_t n_prompts;
    const int64_t* gen_ids;
    int64_t ld_gen;
    int32_t* n_bad;
    int hs;                                               // pen_table_slots(ld_gen)
    float inv_r, r, f, p;                                 // fl(1 / r) (from double), fl(r), fl(f), fl(p)
};

// The policy of the plain kernels: y = x, nothing read, nothing built.
struct PenNone {
    static constexpr bool ON = false;
    __device__ __forceinline__ float y(int, float x) const { return x; }
};

// What the walks hold of a row's history: the two LDS addresses and the table's size.  The four scalars are read from LDS where a column of
// the history is met (a load that goes out beside the probe's), so they cost the walks no registers.
struct PenOn {
    static constexpr bool ON = true;
    const uint32_t* seen;                                 // the bit mask
    const uint2* tab;                                     // the table: (token + 1, count) pairs, read with one 8-byte load
    uint32_t hmask;                                       // Hs - 1
    const float* par;                                     // {fl(1 / r), fl(r), fl(f), fl(p)}

    // the seen bits of column c and of those after it in its word
    __device__ __forceinline__ uint32_t bits(int c) const { return seen[c >> 5] >> (c & 31); }

    // n_c: the count stored under token c, 0 when the probe meets an empty slot first
    __device__ __forceinline__ uint32_t count(int c) const {
        const uint32_t k = (uint32_t)c + 1u;
        uint32_t h = (uint32_t)c & hmask;
        for (uint32_t n = 0; n <= hmask; ++n, h = (h + 1u) & hmask) {
            const uint2 at = tab[h];
            if (at.x == k) return at.y;
            if (at.x == 0u) break;
        }
        return 0u;
    }

    // y_c of a column of H (the header's definition, its two roundings)
    __device__ __forceinline__ float of_seen(int c, float x) const {
        const float4 q = *reinterpret_cast<const float4*>(par);
        const uint32_t n = (q.z != 0.f || q.w != 0.f) ? count(c) : 0u;      // (a repetition penalty alone needs no count: t is 0 either way)
        const float a = x > 0.f ? q.x : q.y;
        const float t = __builtin_fmaf(q.z, (float)n, n > 0u ? q.w : 0.f);
        return __builtin_fmaf(x, a, -t);
    }

    __device__ __forceinline__ float y(int c, float x) const { return (bits(c) & 1u) ? of_seen(c, x) : x; }
};

// y of the VEC columns of the vector at c0 (a multiple of VEC, so its bits lie in one word): get(e, x_e) with a compile-time e.  Without
// penalties it is empty and get hands x_e back, so the plain kernels keep their code.
template <typename T, typename Pen> struct PenVec;
template <typename T> struct PenVec<T, PenNone> {
    __device__ __forceinline__ PenVec(const PenNone&, int, const Vec16<T>&) {}
    __device__ __forceinline__ float get(int, float x) const { return x; }
};
template <typename T> struct PenVec<T, PenOn> {
    static constexpr int VEC = Vec16<T>::N;
    float y[VEC];
    __device__ __forceinline__ PenVec(const PenOn& pen, int c0, const Vec16<T>& xv) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) y[e] = xv.get(e);
        // Rare and divergent: a column of the history.  One lookup body per vector, run once per set bit; the element is read and written
        // through selects, so every register index stays a compile-time one.
        for (uint32_t sb = pen.bits(c0) & ((1u << VEC) - 1u); sb != 0u; sb &= sb - 1u) {
            const int at = __builtin_ctz(sb);
            float xe = y[0];
#pragma unroll
            for (int e = 1; e < VEC; ++e) xe = at == e ? y[e] : xe;
            const float ye = pen.of_seen(c0 + at, xe);
#pragma unroll
            for (int e = 0; e < VEC; ++e) y[e] = at == e ? ye : y[e];
        }
    }
    __device__ __forceinline__ float get(int e, float) const { return y[e]; }
};

// Builds row r's history in `lds` (pen_lds_bytes(vocab, ld_gen) bytes); ends with a barrier.
__device__ __forceinline__ PenOn pen_build(const PenArgs& a, const int32_t* __restrict__ n_generated, int64_t r, int vocab, int tid,
                                           uint32_t* lds) {
    __shared__ int s_bad;
    __shared__ __attribute__((aligned(16))) float s_par[4];
    const int words = (vocab + 31) >> 5;
    uint32_t* tab = lds;                                  // (first: the pairs stay 8-byte aligned whatever the vocabulary)
    uint32_t* seen = lds + 2 * a.hs;
    const uint32_t hmask = (uint32_t)a.hs - 1u;
    for (int i = tid; i < words + 2 * a.hs; i += SEL_THREADS) lds[i] = 0u;
    if (tid == 0) {
        s_bad = 0;
        s_par[0] = a.inv_r;
        s_par[1] = a.r;
        s_par[2] = a.f;
        s_par[3] = a.p;
    }
    __syncthreads();
    bool bad = false;
    const int64_t line = a.prompt_row ? (int64_t)a.prompt_row[r] : r;
    if (line < 0 || line >= a.n_prompts) {
        bad = true;
    } else {
        const int np = (int)min((int64_t)max(a.prompt_len[line], 0), a.ld_prompt);
        const int32_t* __restrict__ ids = a.prompt_ids + line * a.ld_prompt;
        for (int i = tid; i < np; i += SEL_THREADS) {
            const int32_t t = ids[i];
            if ((uint32_t)t >= (uint32_t)vocab) bad = true;
            else atomicOr(&seen[t >> 5], 1u << (t & 31));
        }
    }
    const int ng = (int)min((int64_t)max(n_generated[r], 0), a.ld_gen);
    const int64_t* __restrict__ gen = a.gen_ids + r * a.ld_gen;
    for (int i = tid; i < ng; i += SEL_THREADS) {
        const int64_t t64 = gen[i];
        if ((uint64_t)t64 >= (uint64_t)vocab) {
            bad = true;
            continue;
        }
        const uint32_t t = (uint32_t)t64, k = t + 1u;
        atomicOr(&seen[t >> 5], 1u << (t & 31));
        uint32_t h = t & hmask;
        for (uint32_t n = 0; n <= hmask; ++n, h = (h + 1u) & hmask) {      // (at most ld_gen <= Hs / 2 keys: an empty slot is always met)
            const uint32_t was = atomicCAS(&tab[2 * h], 0u, k);
            if (was == 0u || was == k) {
                atomicAdd(&tab[2 * h + 1], 1u);
                break;
            }
        }
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (tid == 0 && s_bad != 0 && a.n_bad) atomicAdd(a.n_bad, 1);
    PenOn pen;
    pen.seen = seen;
    pen.tab = reinterpret_cast<const uint2*>(tab);
    pen.hmask = hmask;
    pen.par = s_par;
    return pen;
}

// The host checks the two penalised entries share, after the plain entry's own: fills `a`.  0 or an SSI_ERR_* code.
static inline int pen_check(PenArgs& a, int64_t vocab, const int32_t* n_generated, const int32_t* prompt_ids, int64_t ld_prompt,
                            const int32_t* prompt_len, const int32_t* prompt_row, int64_t n_prompts, const int64_t* gen_ids, int64_t ld_gen,
                            double r, double f, double p, int32_t* n_bad) {
    SSI_CHECK_ARG(r > 0.0 && r < (double)INFINITY);
    SSI_CHECK_ARG(f >= -2.0 && f <= 2.0 && p >= -2.0 && p <= 2.0);
    SSI_CHECK_ARG(n_generated != nullptr && prompt_len != nullptr && n_prompts >= 1);
    SSI_CHECK_ARG(ld_gen >= 0 && ld_gen < (1LL << 30) && (gen_ids != nullptr || ld_gen == 0));
    SSI_CHECK_ARG(ld_prompt >= 0 && (prompt_ids != nullptr || ld_prompt == 0));
    if (pen_lds_bytes(vocab, ld_gen) > PEN_LDS_MAX) {
        ssi_set_error("decode penalties: vocab %lld with ld_gen %lld needs %lld bytes of LDS, more than %lld", (long long)vocab,
                      (long long)ld_gen, (long long)pen_lds_bytes(vocab, ld_gen), (long long)PEN_LDS_MAX);
        return SSI_ERR_UNSUPPORTED;
    }
    a.prompt_ids = prompt_ids;
    a.ld_prompt = ld_prompt;
    a.prompt_len = prompt_len;
    a.prompt_row = prompt_row;
    a.n_prompts = n_prompts;
    a.gen_ids = gen_ids;
    a.ld_gen = ld_gen;
    a.n_bad = n_bad;
    a.hs = (int)pen_table_slots(ld_gen);
    a.inv_r = (float)(1.0 / r);
    a.r = (float)r;
    a.f = (float)f;
    a.p = (float)p;
    return SSI_OK;
}

}  // namespace
