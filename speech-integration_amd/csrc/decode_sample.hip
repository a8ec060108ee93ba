// Sampled decoding (ABI v21): ssi_decode_sample draws a row's token from softmax(x / T) restricted by the allowed-token mask, top-k and
// top-p, and reports the token's log-probability under the row's unconstrained distribution at T = 1 and the size of the set drawn from.
// The definition (include/ssi_hip.h states it in full; DESIGN.md §3 derives the bounds):
//   A   the allowed columns below vocab (ssi_decode_select's masks), ordered by topk_key: NaN below every number;
//   K   top-k: the columns of A at or above the top_k-th largest value (ties at the threshold all stay); A when top_k <= 0 or >= |A|;
//   P   top-p: the fewest whole value classes of K, from the top, whose mass under softmax(x / T) over K reaches top_p; K when top_p >= 1;
//   token = argmax over P of x / T + G (Gumbel-max), the lowest column on a tie, G from Philox4x32-10 keyed by (seed; column, step, sequence).
//
// ssi_decode_select's shape: a workgroup of 4 waves per row, the row walked through sel_walk (it stays in L2 between the walks):
//   walk 1      the maximum over ALL real columns (for the log-normaliser) and the maximum over the allowed ones (for the masses);
//   select      only with top_k > 0 or top_p < 1: a radix select on the unsigned key of the stored values, 8 bits per pass (2 passes for bf16,
//               4 for fp32), first for the top-k threshold by COUNT, then for the top-p threshold by MASS among the keys at or above it.  A
//               pass fills a 256-bin LDS histogram of counts and of masses in integer fixed point (a term in [0, 1] scaled by 2^40, 64-bit
//               LDS adds: integer sums do not depend on the order of arrival), every thread then forms one suffix sum and a ballot finds
//               the digit at which the target is crossed;
//   last walk   the exp-sum over all real columns, term for term ssi_decode_select's, the draw among the kept columns and their count.
// No scratch, no workspace, no sort; a row's outputs depend on that row, the masks and the scalars only.
// ssi_decode_sample_pen (ABI v22) runs the same body with everything that selects on the penalised values of decode_penalty.h: fp32 numbers
// whatever the storage, so its radix select takes the 32-bit key (4 passes per threshold for bf16, too).
#include "decode_penalty.h"

namespace {

constexpr uint32_t SMP_TAG = 0x53414D50u;                 // "SAMP": the fourth counter word, apart from the optimizer's tensor numbers
constexpr float SMP_FIX = 0x1p40f;                        // the fixed point of a mass term

// The radix key of a stored value: topk_key's order in as many bits as the storage has (a bf16's low 16 bits of the fp32 pattern are empty).
template <typename T> struct SmpKey;
template <> struct SmpKey<float> {
    static constexpr int BITS = 32;
    static __device__ __forceinline__ uint32_t of(float f) { return topk_key(f); }
};
template <> struct SmpKey<bf16_t> {
    static constexpr int BITS = 16;
    static __device__ __forceinline__ uint32_t of(float f) { return topk_key(f) >> 16; }
};
// The key of what is selected on: a penalised value is an fp32 number whatever the storage, so its key has 32 bits.
template <typename T, typename Pen> struct SmpSel {
    static constexpr int BITS = Pen::ON ? 32 : SmpKey<T>::BITS;
    static __device__ __forceinline__ uint32_t of(float f) {
        if constexpr (Pen::ON) return topk_key(f);
        else return SmpKey<T>::of(f);
    }
};

// exp((x - m) / T) in fixed point: sc = fl(log2 e / T), nm = fl(-m sc).  A NaN (a NaN column, or inf - inf) and -inf count 0.
__device__ __forceinline__ unsigned long long smp_mass(float f, float sc, float nm) {
    const float w = __builtin_amdgcn_exp2f(__builtin_fmaf(f, sc, nm));
    return (unsigned long long)(fmaxf(w, 0.f) * SMP_FIX);      // (no clamp at 1: the factor 2^(m sc + nm) is common to all terms of a row)
}

// G = -ln(-ln u), u = (2 (w >> 9) + 1) 2^-24: an odd multiple of 2^-24 in (0, 1), exact in fp32, so G is finite.  -ln u for u >= 1/2 goes
// through log1p of the exact u - 1: what matters of a u just below 1 is its distance from 1.
__device__ __forceinline__ float smp_gumbel(uint32_t w) {
    const float u = (float)(2u * (w >> 9) + 1u) * 0x1p-24f;
    const float l = u < 0.5f ? -logf(u) : -log1pf(u - 1.f);
    return -logf(l);
}

// An upper bound of G from the leading ones of the word alone: with k of them u < 1 - 2^-(k + 1), and -ln(-ln(1 - e)) < -ln e = (k + 1) ln 2.
// The slack is a hundred times what the two logarithms of smp_gumbel can be off by, so the computed G never exceeds it.
__device__ __forceinline__ float smp_gumbel_bound(uint32_t w) {
    return (float)(__builtin_clz(~w | 1u) + 1) * 0.69314724f + 1e-3f;
}

// topk_key back to the value (key 0, "nothing yet", and the NaN key give a NaN: no comparison with it holds)
__device__ __forceinline__ float smp_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

struct SmpHist {
    uint32_t cnt[256];
    unsigned long long mass[256];
    uint32_t ccnt[257];                                   // suffix sums: c[d] = sum of the bins >= d; c[256] = 0
    unsigned long long cmass[257];
    int hi[SEL_WAVES];
};

// One radix pass: the histogram over the digit (key >> shift) & 255 of the allowed columns whose key is >= floor and whose higher digits
// equal prefix (0 in the first pass, where there are none), then the suffix sums.
template <typename T, typename Pen>
__device__ __forceinline__ void smp_pass(const T* __restrict__ x, const uint32_t* __restrict__ mask, int nvec, int vocab, int tid, int shift,
                                         uint32_t prefix, uint32_t floor, bool want_mass, float sc, float nm, SmpHist& h, const Pen& pen) {
    constexpr int VEC = Vec16<T>::N;
    __syncthreads();                                      // (the previous pass's reads of the suffix sums are over)
    h.cnt[tid] = 0u;
    h.mass[tid] = 0ull;
    __syncthreads();
    auto visit = [&](float f, bool allowed) {
        const uint32_t key = SmpSel<T, Pen>::of(f);
        if (allowed && key >= floor && ((key >> shift) >> 8) == prefix) {
            const uint32_t d = (key >> shift) & 255u;
            atomicAdd(&h.cnt[d], 1u);
            if (want_mass) atomicAdd(&h.mass[d], smp_mass(f, sc, nm));
        }
    };
    auto visit_vec = [&](int c0, const Vec16<T>& xv, uint32_t bits) {
        const PenVec<T, Pen> y(pen, c0, xv);
#pragma unroll
        for (int e = 0; e < VEC; ++e) visit(y.get(e, xv.get(e)), (bits & (1u << e)) != 0);
    };
    if (mask) sel_walk<T, true>(x, mask, nvec, tid, visit_vec);
    else sel_walk<T, false>(x, mask, nvec, tid, visit_vec);
    for (int c = nvec * VEC + tid; c < vocab; c += SEL_THREADS) visit(pen.y(c, to_f32<T>(x[c])), (sel_mask_bits(mask, c) & 1u) != 0);
    __syncthreads();
    uint32_t sc_ = 0u;
    unsigned long long sm_ = 0ull;
#pragma unroll 8
    for (int b = 255; b >= 0; --b) {                      // every lane reads the same bin: a broadcast
        const uint32_t hc = h.cnt[b];
        const unsigned long long hm = h.mass[b];
        sc_ += b >= tid ? hc : 0u;
        sm_ += b >= tid ? hm : 0ull;
    }
    h.ccnt[tid] = sc_;
    h.cmass[tid] = sm_;
    if (tid == 0) {
        h.ccnt[256] = 0u;
        h.cmass[256] = 0ull;
    }
    __syncthreads();
}

// The highest digit whose suffix sum reaches the target (0 when none does); uniform over the workgroup.
__device__ __forceinline__ int smp_find(bool ok, int tid, SmpHist& h) {
    const unsigned long long b = __ballot(ok);
    if ((tid & 63) == 0) h.hi[tid >> 6] = b ? (tid & ~63) + 63 - __builtin_clzll(b) : -1;
    __syncthreads();
    return max(max(max(h.hi[0], h.hi[1]), max(h.hi[2], h.hi[3])), 0);
}

// The row body of ssi_decode_sample and of ssi_decode_sample_pen: `pen` says what a column's value is wherever the token is DRAWN (the allowed
// maximum, the keys, the masses, the score; PenNone: the stored one); the row's maximum, the exp-sum and the log-probability stay on the
// stored values.
template <typename T, typename Pen>
__device__ __forceinline__ void sample_row(const T* logits, int64_t ld, int vocab, const uint32_t* allow,
                                           const uint32_t* allow_early, const int32_t* n_generated, int32_t min_new,
                                           float inv_t, float sc, int top_k, double top_p, uint32_t seed_lo, uint32_t seed_hi, uint32_t step,
                                           const uint32_t* sequence, int64_t* token, float* logprob,
                                           int32_t* n_kept, int vec_ok, const Pen& pen) {
    constexpr int VEC = Vec16<T>::N, BITS = SmpSel<T, Pen>::BITS;
    __shared__ float s_f[16];
    __shared__ int s_i[16];
    __shared__ SmpHist h;
    __shared__ uint32_t s_seen;                           // topk_key of the best score any thread has reached so far (the last walk)
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const T* __restrict__ x = logits + r * ld;
    const bool early = n_generated != nullptr && n_generated[r] < min_new;
    const uint32_t* __restrict__ mask = early ? allow_early : allow;
    const int nvec = vec_ok ? vocab / VEC : 0;
    const int tail0 = nvec * VEC;
    const uint32_t seq = sequence[r];

    // ---- walk 1: the maximum over all real columns and over the allowed ones (fmaxf passes a NaN by) -------------------------------
    float gm = -INFINITY, am = -INFINITY;
    auto maxima = [&](int c0, const Vec16<T>& xv, uint32_t bits) {
        const PenVec<T, Pen> y(pen, c0, xv);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float f = xv.get(e);
            gm = fmaxf(gm, f);
            am = fmaxf(am, (bits & (1u << e)) ? y.get(e, f) : -INFINITY);
        }
    };
    if (mask) sel_walk<T, true>(x, mask, nvec, tid, maxima);
    else sel_walk<T, false>(x, mask, nvec, tid, maxima);
    for (int c = tail0 + tid; c < vocab; c += SEL_THREADS) {
        const float f = to_f32<T>(x[c]);
        gm = fmaxf(gm, f);
        am = fmaxf(am, (sel_mask_bits(mask, c) & 1u) ? pen.y(c, f) : -INFINITY);
    }
    gm = wave_max(gm);
    am = wave_max(am);
    if (lane == 0) {
        s_f[wave] = gm;
        s_f[4 + wave] = am;
    }
    __syncthreads();
    gm = fmaxf(fmaxf(s_f[0], s_f[1]), fmaxf(s_f[2], s_f[3]));
    am = fmaxf(fmaxf(s_f[4], s_f[5]), fmaxf(s_f[6], s_f[7]));

    int bi = -1, kept = 0;
    float bv = -INFINITY;
    uint32_t tau = 0u;                                    // P = the allowed columns whose key is >= tau
    const bool drawn = am > -INFINITY;                    // (uniform over the workgroup)
    if (!drawn) {
        // No allowed column holds a value above -inf: ssi_decode_select's rule, the FIRST allowed column, and P is that column alone.
        int first = 0x7fffffff;
        if (!mask) {
            first = 0;
        } else {
            for (int w = tid; w < (vocab + 31) / 32; w += SEL_THREADS) {
                const uint32_t bits = mask[w];
                const int c = w * 32 + __builtin_ctz(bits | 0x80000000u);
                if (bits != 0 && c < vocab && c < first) first = c;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
        if (lane == 0) s_i[wave] = first;
        __syncthreads();
        first = min(min(s_i[0], s_i[1]), min(s_i[2], s_i[3]));
        if (first == 0x7fffffff) {                        // nothing allowed below vocab
            if (tid == 0) {
                token[r] = -1;
                if (logprob) logprob[r] = 0.f;
                if (n_kept) n_kept[r] = -1;
            }
            return;
        }
        bi = first;
        kept = 1;
    } else if (top_k > 0 || top_p < 1.0) {
        // ---- the thresholds ---------------------------------------------------------------------------------------------------------
        const float nm = -am * sc;
        const bool by_p = top_p < 1.0;
        unsigned long long z = 0ull;                      // the mass of K
        bool have_z = false;
        if (top_k > 0) {
            uint32_t prefix = 0u, target = (uint32_t)top_k;
            for (int shift = BITS - 8; shift >= 0; shift -= 8) {
                smp_pass<T>(x, mask, nvec, vocab, tid, shift, prefix, 0u, by_p, sc, nm, h, pen);
                if (shift == BITS - 8 && (uint32_t)top_k >= h.ccnt[0]) {      // top_k >= |A|: K = A
                    z = h.cmass[0];
                    prefix = 0u;
                    break;
                }
                const int d = smp_find(h.ccnt[tid] >= target, tid, h);
                target -= h.ccnt[d + 1];
                z += shift == 0 ? h.cmass[d] : h.cmass[d + 1];
                prefix = (prefix << 8) | (uint32_t)d;
            }
            tau = prefix;
            have_z = true;
        }
        if (by_p) {
            const uint32_t floor = tau;
            uint32_t prefix = 0u;
            unsigned long long target = 0ull;
            for (int shift = BITS - 8; shift >= 0; shift -= 8) {
                smp_pass<T>(x, mask, nvec, vocab, tid, shift, prefix, floor, true, sc, nm, h, pen);
                if (shift == BITS - 8) {
                    if (!have_z) z = h.cmass[0];
                    target = (unsigned long long)ceil(top_p * (double)z);
                    target = target > z ? z : target;
                    target = target < 1ull ? 1ull : target;
                }
                const int d = smp_find(h.cmass[tid] >= target, tid, h);
                target -= h.cmass[d + 1];
                prefix = (prefix << 8) | (uint32_t)d;
            }
            tau = prefix > floor ? prefix : floor;
        }
    }

    // ---- the last walk: the exp-sum over all real columns (ssi_decode_select's), the draw among the kept columns, their count ----------
    const float nm_all = -gm * SEL_LOG2E;
    float s = 0.f;
    // Pruning, which cannot change the result: a column whose score cannot exceed fma(x, 1/T, bound of G) — the fma is monotone in its addend —
    // is skipped without its logarithms when that is not above the thread's own best (an earlier, lower column: it would lose a tie, too) or
    // is below a score some column of the row has already reached (seen: shared through one LDS word, read racily — every value it ever
    // holds is a score that was reached; it starts at what the allowed maximum's column reaches at the least, G >= -2.83).
    float seen = __builtin_fmaf(am, inv_t, -2.83f);
    if (tid == 0) s_seen = topk_key(seen);
    __syncthreads();
    auto draw = [&](int c, float f, uint32_t word) {
        const float most = __builtin_fmaf(f, inv_t, smp_gumbel_bound(word));
        if (most > bv && !(most < seen)) {
            const float score = __builtin_fmaf(f, inv_t, smp_gumbel(word));
            const bool take = score > bv;
            bv = take ? score : bv;
            bi = take ? c : bi;
        }
    };
    auto last_vec = [&](int c0, const Vec16<T>& xv, uint32_t bits) {
        uint32_t kb = 0u;
        const PenVec<T, Pen> y(pen, c0, xv);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float f = xv.get(e);
            s += __builtin_amdgcn_exp2f(__builtin_fmaf(f, SEL_LOG2E, nm_all));
            kb |= (uint32_t)(drawn & ((bits & (1u << e)) != 0) & (SmpSel<T, Pen>::of(y.get(e, f)) >= tau)) << e;
        }
        kept += __builtin_popcount(kb);
        if (kb && ((c0 / (VEC * SEL_THREADS)) & 3) == 0)  // every fourth round, where something is kept: the best score reached so far, given and taken
            seen = fmaxf(seen, smp_unkey(max(atomicMax(&s_seen, topk_key(bv)), topk_key(bv))));
#pragma unroll
        for (int q = 0; q < VEC / 4; ++q) {               // one generator call per four columns, where one of them is kept
            if ((kb >> (4 * q)) & 15u) {
                const Philox4 p = philox4x32_10((uint32_t)(c0 >> 2) + q, step, seq, SMP_TAG, seed_lo, seed_hi);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (kb & (1u << (4 * q + j))) draw(c0 + 4 * q + j, y.get(4 * q + j, xv.get(4 * q + j)), p.w[j]);
            }
        }
    };
    constexpr int LAST_UNROLL = Pen::ON ? SEL_UNROLL / 2 : SEL_UNROLL;      // (the penalised draw holds y beside x: fewer vectors in flight, no spill)
    if (mask) sel_walk<T, true, LAST_UNROLL>(x, mask, nvec, tid, last_vec);
    else sel_walk<T, false, LAST_UNROLL>(x, mask, nvec, tid, last_vec);
    for (int c = tail0 + tid; c < vocab; c += SEL_THREADS) {
        const float f = to_f32<T>(x[c]);
        s += __builtin_amdgcn_exp2f(__builtin_fmaf(f, SEL_LOG2E, nm_all));
        const float yc = pen.y(c, f);
        if (drawn && (sel_mask_bits(mask, c) & 1u) && SmpSel<T, Pen>::of(yc) >= tau) {
            ++kept;
            const Philox4 p = philox4x32_10((uint32_t)(c >> 2), step, seq, SMP_TAG, seed_lo, seed_hi);
            const uint32_t word = (c & 3) == 0 ? p.w[0] : (c & 3) == 1 ? p.w[1] : (c & 3) == 2 ? p.w[2] : p.w[3];
            draw(c, yc, word);
        }
    }
    if (drawn) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {                // ssi_decode_select's fixed xor tree over (score, column) pairs
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (sel_better(bv, bi, ov, oi)) {
                bv = ov;
                bi = oi;
            }
        }
        __syncthreads();
        if (lane == 0) {
            s_f[wave] = bv;
            s_i[wave] = bi;
        }
        __syncthreads();
        bv = s_f[0];
        bi = s_i[0];
#pragma unroll
        for (int w = 1; w < SEL_WAVES; ++w) {
            if (sel_better(bv, bi, s_f[w], s_i[w])) {
                bv = s_f[w];
                bi = s_i[w];
            }
        }
        kept = block_sum_i32(kept, s_i + 8);
    }
    s = block_sum(s, s_f + 8);
    if (tid == 0) {
        token[r] = bi;
        if (logprob) logprob[r] = bi >= 0 ? to_f32<T>(x[bi]) - (gm + logf(s)) : 0.f;
        if (n_kept) n_kept[r] = bi >= 0 ? kept : -1;
    }
}

template <typename T>
__global__ __launch_bounds__(SEL_THREADS) void decode_sample_kernel(const T* __restrict__ logits, int64_t ld, int vocab,
                                                                    const uint32_t* __restrict__ allow, const uint32_t* __restrict__ allow_early,
                                                                    const int32_t* __restrict__ n_generated, int32_t min_new, float inv_t,
                                                                    float sc, int top_k, double top_p, uint32_t seed_lo, uint32_t seed_hi,
                                                                    uint32_t step, const uint32_t* __restrict__ sequence,
                                                                    int64_t* __restrict__ token, float* __restrict__ logprob,
                                                                    int32_t* __restrict__ n_kept, int vec_ok) {
    sample_row<T>(logits, ld, vocab, allow, allow_early, n_generated, min_new, inv_t, sc, top_k, top_p, seed_lo, seed_hi, step, sequence, token,
                  logprob, n_kept, vec_ok, PenNone{});
}

// ssi_decode_sample_pen (ABI v22): the row's history is built in dynamic LDS first (decode_penalty.h), then the same body draws on y.
template <typename T>
__global__ __launch_bounds__(SEL_THREADS) void sample_pen_kernel(const T* __restrict__ logits, int64_t ld, int vocab,
                                                                 const uint32_t* __restrict__ allow, const uint32_t* __restrict__ allow_early,
                                                                 const int32_t* __restrict__ n_generated, int32_t min_new, float inv_t, float sc,
                                                                 int top_k, double top_p, uint32_t seed_lo, uint32_t seed_hi, uint32_t step,
                                                                 const uint32_t* __restrict__ sequence, int64_t* __restrict__ token,
                                                                 float* __restrict__ logprob, int32_t* __restrict__ n_kept, int vec_ok,
                                                                 PenArgs pa) {
    extern __shared__ __attribute__((aligned(16))) uint32_t pen_lds[];
    const PenOn pen = pen_build(pa, n_generated, blockIdx.x, vocab, threadIdx.x, pen_lds);
    sample_row<T>(logits, ld, vocab, allow, allow_early, n_generated, min_new, inv_t, sc, top_k, top_p, seed_lo, seed_hi, step, sequence, token,
                  logprob, n_kept, vec_ok, pen);
}

// ssi_decode_sample_rows / ssi_decode_sample_pen_rows (ABI v28): the draw parameters and the step of row r come from device arrays (a NULL
// array: the launch's scalar).  One workgroup owns one row, so what it reads here is uniform over it, as the scalars are over a launch.
struct SmpRows {
    const uint32_t* step;
    const double* temperature;
    const int64_t* top_k;
    const double* top_p;
};

struct SmpDraw {
    float inv_t, sc;
    int top_k;
    double top_p;
    uint32_t step;
    bool ok;
};

// Row r's parameters, by the host expressions of the scalar entries: fl(1 / T) and fl(log2 e / T) are fp64 quotients rounded once to fp32
// (IEEE division and conversion on the device as on the host), top_k outside (0, vocab) is "off".  ok: T finite and > 0, top_p in (0, 1].
__device__ __forceinline__ SmpDraw smp_row_draw(const SmpRows& rw, int64_t r, int vocab, double temperature, int64_t top_k, double top_p) {
    const double t = rw.temperature ? rw.temperature[r] : temperature;
    const double p = rw.top_p ? rw.top_p[r] : top_p;
    const int64_t k = rw.top_k ? rw.top_k[r] : top_k;
    SmpDraw d;
    d.ok = t > 0.0 && t < (double)INFINITY && p > 0.0 && p <= 1.0;
    d.inv_t = (float)(1.0 / t);
    d.sc = (float)(1.44269504088896340736 / t);
    d.top_k = k <= 0 || k >= (int64_t)vocab ? 0 : (int)k;
    d.top_p = p;
    d.step = rw.step[r];
    return d;
}

// A row whose own parameters are refused fails alone: what a row with nothing allowed writes.
__device__ __forceinline__ void smp_row_refused(int64_t r, int64_t* token, float* logprob, int32_t* n_kept) {
    if (threadIdx.x == 0) {
        token[r] = -1;
        if (logprob) logprob[r] = 0.f;
        if (n_kept) n_kept[r] = -1;
    }
}

template <typename T>
__global__ __launch_bounds__(SEL_THREADS) void sample_rows_kernel(const T* __restrict__ logits, int64_t ld, int vocab,
                                                                  const uint32_t* __restrict__ allow, const uint32_t* __restrict__ allow_early,
                                                                  const int32_t* __restrict__ n_generated, int32_t min_new, double temperature,
                                                                  int64_t top_k, double top_p, uint32_t seed_lo, uint32_t seed_hi, SmpRows rw,
                                                                  const uint32_t* __restrict__ sequence, int64_t* __restrict__ token,
                                                                  float* __restrict__ logprob, int32_t* __restrict__ n_kept, int vec_ok) {
    const SmpDraw d = smp_row_draw(rw, blockIdx.x, vocab, temperature, top_k, top_p);
    if (!d.ok) {
        smp_row_refused(blockIdx.x, token, logprob, n_kept);
        return;
    }
    sample_row<T>(logits, ld, vocab, allow, allow_early, n_generated, min_new, d.inv_t, d.sc, d.top_k, d.top_p, seed_lo, seed_hi, d.step, sequence,
                  token, logprob, n_kept, vec_ok, PenNone{});
}

template <typename T>
__global__ __launch_bounds__(SEL_THREADS) void sample_rows_pen_kernel(const T* __restrict__ logits, int64_t ld, int vocab,
                                                                      const uint32_t* __restrict__ allow, const uint32_t* __restrict__ allow_early,
                                                                      const int32_t* __restrict__ n_generated, int32_t min_new, double temperature,
                                                                      int64_t top_k, double top_p, uint32_t seed_lo, uint32_t seed_hi, SmpRows rw,
                                                                      const uint32_t* __restrict__ sequence, int64_t* __restrict__ token,
                                                                      float* __restrict__ logprob, int32_t* __restrict__ n_kept, int vec_ok,
                                                                      PenArgs pa) {
    extern __shared__ __attribute__((aligned(16))) uint32_t pen_lds[];
    const SmpDraw d = smp_row_draw(rw, blockIdx.x, vocab, temperature, top_k, top_p);
    if (!d.ok) {                                          // (before the history is built: a refused row counts nothing into n_bad)
        smp_row_refused(blockIdx.x, token, logprob, n_kept);
        return;
    }
    const PenOn pen = pen_build(pa, n_generated, blockIdx.x, vocab, threadIdx.x, pen_lds);
    sample_row<T>(logits, ld, vocab, allow, allow_early, n_generated, min_new, d.inv_t, d.sc, d.top_k, d.top_p, seed_lo, seed_hi, d.step, sequence,
                  token, logprob, n_kept, vec_ok, pen);
}

// What the two _rows entries refuse before a launch: the plain entry's checks, with a scalar checked only where no array stands for it.
int smp_rows_check(const void* logits, int64_t ld, int64_t rows, int64_t vocab, int32_t min_new, double temperature, double top_p,
                   const uint32_t* step, const double* temperature_rows, const double* top_p_rows, const uint32_t* sequence,
                   const int64_t* token, int dtype) {
    SSI_CHECK_ARG(rows >= 0 && rows < (1LL << 31) && (dtype == SSI_F32 || dtype == SSI_BF16));
    SSI_CHECK_ARG(logits && token && vocab >= 1 && ld >= vocab && vocab < (1LL << 31) && min_new >= 0);
    SSI_CHECK_ARG(temperature_rows != nullptr || (temperature > 0.0 && temperature < (double)INFINITY));
    SSI_CHECK_ARG(top_p_rows != nullptr || (top_p > 0.0 && top_p <= 1.0));
    SSI_CHECK_ARG(sequence != nullptr && step != nullptr);
    return SSI_OK;
}

}  // namespace

extern "C" int ssi_decode_sample(const void* logits, int64_t ld, int64_t rows, int64_t vocab, const uint32_t* allow, const uint32_t* allow_early,
                                 const int32_t* n_generated, int32_t min_new, double temperature, int64_t top_k, double top_p, uint64_t seed,
                                 uint32_t step, const uint32_t* sequence, int64_t* token, float* logprob, int32_t* n_kept, int dtype,
                                 void* stream) {
    SSI_CHECK_ARG(rows >= 0 && rows < (1LL << 31) && (dtype == SSI_F32 || dtype == SSI_BF16));
    SSI_CHECK_ARG(logits && token && vocab >= 1 && ld >= vocab && vocab < (1LL << 31) && min_new >= 0);
    SSI_CHECK_ARG(temperature > 0.0 && temperature < (double)INFINITY);
    SSI_CHECK_ARG(top_p > 0.0 && top_p <= 1.0);
    SSI_CHECK_ARG(sequence != nullptr);
    if (rows == 0) return SSI_OK;
    const int64_t esize = dtype == SSI_BF16 ? 2 : 4;
    const int vec_ok = ((uintptr_t)logits & 15) == 0 && (ld * esize) % 16 == 0;
    const int k = top_k <= 0 || top_k >= vocab ? 0 : (int)top_k;      // |A| <= vocab: top_k >= vocab keeps all of A
    const float inv_t = (float)(1.0 / temperature), sc = (float)(1.44269504088896340736 / temperature);
    SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(decode_sample_kernel<T>, dim3((unsigned)rows), dim3(SEL_THREADS), 0, (hipStream_t)stream,
                                                 (const T*)logits, ld, (int)vocab, allow, allow_early, n_generated, min_new, inv_t, sc, k, top_p,
                                                 (uint32_t)seed, (uint32_t)(seed >> 32), step, sequence, token, logprob, n_kept, vec_ok));
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

extern "C" int ssi_decode_sample_pen(const void* logits, int64_t ld, int64_t rows, int64_t vocab, const uint32_t* allow, const uint32_t* allow_early,
                                     const int32_t* n_generated, int32_t min_new, double temperature, int64_t top_k, double top_p, uint64_t seed,
                                     uint32_t step, const uint32_t* sequence, int64_t* token, float* logprob, int32_t* n_kept,
                                     const int32_t* prompt_ids, int64_t ld_prompt, const int32_t* prompt_len, const int32_t* prompt_row,
                                     int64_t n_prompts, const int64_t* gen_ids, int64_t ld_gen, double repetition_penalty, double frequency_penalty,
                                     double presence_penalty, int32_t* n_bad, int dtype, void* stream) {
    SSI_CHECK_ARG(rows >= 0 && rows < (1LL << 31) && (dtype == SSI_F32 || dtype == SSI_BF16));
    SSI_CHECK_ARG(logits && token && vocab >= 1 && ld >= vocab && vocab < (1LL << 31) && min_new >= 0);
    SSI_CHECK_ARG(temperature > 0.0 && temperature < (double)INFINITY);
    SSI_CHECK_ARG(top_p > 0.0 && top_p <= 1.0);
    SSI_CHECK_ARG(sequence != nullptr);
    PenArgs pa;
    const int rc = pen_check(pa, vocab, n_generated, prompt_ids, ld_prompt, prompt_len, prompt_row, n_prompts, gen_ids, ld_gen,
                             repetition_penalty, frequency_penalty, presence_penalty, n_bad);
    if (rc != SSI_OK) return rc;
    if (rows == 0) return SSI_OK;
    const int64_t esize = dtype == SSI_BF16 ? 2 : 4;
    const int vec_ok = ((uintptr_t)logits & 15) == 0 && (ld * esize) % 16 == 0;
    const int k = top_k <= 0 || top_k >= vocab ? 0 : (int)top_k;
    const float inv_t = (float)(1.0 / temperature), sc = (float)(1.44269504088896340736 / temperature);
    SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(sample_pen_kernel<T>, dim3((unsigned)rows), dim3(SEL_THREADS),
                                                 (size_t)pen_lds_bytes(vocab, ld_gen), (hipStream_t)stream, (const T*)logits, ld, (int)vocab, allow,
                                                 allow_early, n_generated, min_new, inv_t, sc, k, top_p, (uint32_t)seed, (uint32_t)(seed >> 32), step,
                                                 sequence, token, logprob, n_kept, vec_ok, pa));
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

extern "C" int ssi_decode_sample_rows(const void* logits, int64_t ld, int64_t rows, int64_t vocab, const uint32_t* allow,
                                      const uint32_t* allow_early, const int32_t* n_generated, int32_t min_new, double temperature, int64_t top_k,
                                      double top_p, uint64_t seed, const uint32_t* step, const double* temperature_rows, const int64_t* top_k_rows,
                                      const double* top_p_rows, const uint32_t* sequence, int64_t* token, float* logprob, int32_t* n_kept,
                                      int dtype, void* stream) {
    const int rc = smp_rows_check(logits, ld, rows, vocab, min_new, temperature, top_p, step, temperature_rows, top_p_rows, sequence, token, dtype);
    if (rc != SSI_OK) return rc;
    if (rows == 0) return SSI_OK;
    const int64_t esize = dtype == SSI_BF16 ? 2 : 4;
    const int vec_ok = ((uintptr_t)logits & 15) == 0 && (ld * esize) % 16 == 0;
    const SmpRows rw{step, temperature_rows, top_k_rows, top_p_rows};
    SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(sample_rows_kernel<T>, dim3((unsigned)rows), dim3(SEL_THREADS), 0, (hipStream_t)stream,
                                                 (const T*)logits, ld, (int)vocab, allow, allow_early, n_generated, min_new, temperature, top_k,
                                                 top_p, (uint32_t)seed, (uint32_t)(seed >> 32), rw, sequence, token, logprob, n_kept, vec_ok));
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

extern "C" int ssi_decode_sample_pen_rows(const void* logits, int64_t ld, int64_t rows, int64_t vocab, const uint32_t* allow,
                                          const uint32_t* allow_early, const int32_t* n_generated, int32_t min_new, double temperature,
                                          int64_t top_k, double top_p, uint64_t seed, const uint32_t* step, const double* temperature_rows,
                                          const int64_t* top_k_rows, const double* top_p_rows, const uint32_t* sequence, int64_t* token,
                                          float* logprob, int32_t* n_kept, const int32_t* prompt_ids, int64_t ld_prompt, const int32_t* prompt_len,
                                          const int32_t* prompt_row, int64_t n_prompts, const int64_t* gen_ids, int64_t ld_gen,
                                          double repetition_penalty, double frequency_penalty, double presence_penalty, int32_t* n_bad, int dtype,
                                          void* stream) {
    int rc = smp_rows_check(logits, ld, rows, vocab, min_new, temperature, top_p, step, temperature_rows, top_p_rows, sequence, token, dtype);
    if (rc != SSI_OK) return rc;
    PenArgs pa;
    rc = pen_check(pa, vocab, n_generated, prompt_ids, ld_prompt, prompt_len, prompt_row, n_prompts, gen_ids, ld_gen, repetition_penalty,
                   frequency_penalty, presence_penalty, n_bad);
    if (rc != SSI_OK) return rc;
    if (rows == 0) return SSI_OK;
    const int64_t esize = dtype == SSI_BF16 ? 2 : 4;
    const int vec_ok = ((uintptr_t)logits & 15) == 0 && (ld * esize) % 16 == 0;
    const SmpRows rw{step, temperature_rows, top_k_rows, top_p_rows};
    SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(sample_rows_pen_kernel<T>, dim3((unsigned)rows), dim3(SEL_THREADS),
                                                 (size_t)pen_lds_bytes(vocab, ld_gen), (hipStream_t)stream, (const T*)logits, ld, (int)vocab, allow,
                                                 allow_early, n_generated, min_new, temperature, top_k, top_p, (uint32_t)seed,
                                                 (uint32_t)(seed >> 32), rw, sequence, token, logprob, n_kept, vec_ok, pa));
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}
