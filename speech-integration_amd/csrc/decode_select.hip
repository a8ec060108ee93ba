// Constrained greedy decoding (ABI v19): ssi_decode_select picks a row's token among the ALLOWED columns and reports, under the row's
// unconstrained distribution, that token's log-probability and its rank.  One launch per decode step, the logits read only.
//
// A workgroup of 4 waves takes one row and walks it twice (the 267 KB row of the flagship vocabulary stays in L2 between the walks):
//   walk 1  the maximum over ALL real columns, and the best (value, column) over the allowed ones;
//   walk 2  sum exp(x - max) over all real columns and the count of columns ranked before the chosen one.
// Both walks give a thread the same columns in the same order: 16-byte vectors v = tid, tid + 256, ... of the columns [0, vocab - vocab % VEC)
// when the row is 16-byte aligned, then single columns tid, tid + 256, ... of what is left (every column when it is not).  A thread meets
// its columns in rising order, so "take on >" keeps the first occurrence; threads are merged by a fixed xor tree and the four waves in the
// order 0, 1, 2, 3 with the lower column winning a tie.  A row's result depends on that row and the masks only.
// NaN: no comparison with a NaN holds, so a NaN column is neither the maximum nor chosen while any allowed column holds a number.
// ssi_decode_select_pen (ABI v22) runs the same body with the token chosen on the penalised values of decode_penalty.h.
#include "decode_penalty.h"

namespace {

// The row body of ssi_decode_select and of ssi_decode_select_pen: `pen` says what a column's value is where the token is CHOSEN (PenNone: the
// stored one); the maximum, the exp-sum and the rank stay on the stored values.
template <typename T, typename Pen>
__device__ __forceinline__ void select_row(const T* logits, int64_t ld, int vocab, const uint32_t* allow,
                                           const uint32_t* allow_early, const int32_t* n_generated, int32_t min_new,
                                           int64_t* token, float* logprob, int32_t* rank, int vec_ok,
                                           const Pen& pen) {
    constexpr int VEC = Vec16<T>::N;
    __shared__ float s_f[16];
    __shared__ int s_i[16];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const T* __restrict__ x = logits + r * ld;
    const bool early = n_generated != nullptr && n_generated[r] < min_new;
    const uint32_t* __restrict__ mask = early ? allow_early : allow;
    const int nvec = vec_ok ? vocab / VEC : 0;            // 16-byte vectors of the row; the columns from nvec * VEC on are walked singly
    const int tail0 = nvec * VEC;

    // ---- walk 1: the row's maximum, and the best allowed (value, column) ---------------------------------------------------------
    float gm = -INFINITY, bv = -INFINITY;
    int bi = -1;
    auto best = [&](int c0, const Vec16<T>& xv, uint32_t bits) {
        const PenVec<T, Pen> y(pen, c0, xv);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {                   // selects, no branches: the compiler otherwise jumps around every element
            const float f = xv.get(e);
            gm = fmaxf(gm, f);
            const float v = y.get(e, f);
            const bool take = ((bits & (1u << e)) != 0) & (v > bv);
            bv = take ? v : bv;
            bi = take ? c0 + e : bi;
        }
    };
    if (mask) sel_walk<T, true>(x, mask, nvec, tid, best);
    else sel_walk<T, false>(x, mask, nvec, tid, best);
    for (int c = tail0 + tid; c < vocab; c += SEL_THREADS) {
        const float xc = to_f32<T>(x[c]);
        gm = fmaxf(gm, xc);
        const float f = pen.y(c, xc);
        const bool take = ((sel_mask_bits(mask, c) & 1u) != 0) & (f > bv);
        bv = take ? f : bv;
        bi = take ? c : bi;
    }
    gm = wave_max(gm);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                    // the fixed xor tree over (value, column) pairs
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (sel_better(bv, bi, ov, oi)) {
            bv = ov;
            bi = oi;
        }
    }
    if (lane == 0) {
        s_f[wave] = gm;
        s_f[4 + wave] = bv;
        s_i[wave] = bi;
    }
    __syncthreads();
    gm = fmaxf(fmaxf(s_f[0], s_f[1]), fmaxf(s_f[2], s_f[3]));
    bv = s_f[4];
    bi = s_i[0];
#pragma unroll
    for (int w = 1; w < SEL_WAVES; ++w) {                 // the four waves, in order (every thread does the same: no broadcast needed)
        if (sel_better(bv, bi, s_f[4 + w], s_i[w])) {
            bv = s_f[4 + w];
            bi = s_i[w];
        }
    }
    if (bi < 0) {
        // No allowed column holds a value above -inf (uniform over the workgroup): every allowed one is -inf or NaN, or none is allowed.  The
        // token is then the FIRST allowed column, which is what "the first maximum" means on a row of -inf; a NaN is never chosen above.
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
        __syncthreads();
        if (lane == 0) s_i[wave] = first;
        __syncthreads();
        first = min(min(s_i[0], s_i[1]), min(s_i[2], s_i[3]));
        bi = first == 0x7fffffff ? -1 : first;
    }
    if (bi < 0) {                                         // nothing allowed below vocab (uniform over the workgroup)
        if (tid == 0) {
            token[r] = -1;
            if (logprob) logprob[r] = 0.f;
            if (rank) rank[r] = -1;
        }
        return;
    }
    if (tid == 0) token[r] = bi;
    if (!logprob && !rank) return;

    // ---- walk 2: the exp-sum over all real columns and the rank of the chosen one --------------------------------------------------
    // A term is exp2(fma(x, log2 e, nm)) with nm = fl(-max log2 e): one v_exp_f32 per column, as the register form of the cross-entropy does.
    const float xt = to_f32<T>(x[bi]);
    const float nm = -gm * SEL_LOG2E;
    float s = 0.f;
    int before = 0;
    sel_walk<T, false>(x, nullptr, nvec, tid, [&](int c0, const Vec16<T>& xv, uint32_t) {
        const int eb = bi - c0;                           // the elements e < eb of this vector lie before the chosen column
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float f = xv.get(e);
            s += __builtin_amdgcn_exp2f(__builtin_fmaf(f, SEL_LOG2E, nm));
            before += (int)((f > xt) | ((f == xt) & (e < eb)));      // (| and & on purpose: selects, no branches)
        }
    });
    for (int c = tail0 + tid; c < vocab; c += SEL_THREADS) {
        const float f = to_f32<T>(x[c]);
        s += __builtin_amdgcn_exp2f(__builtin_fmaf(f, SEL_LOG2E, nm));
        before += (int)((f > xt) | ((f == xt) & (c < bi)));
    }
    s = block_sum(s, s_f + 8);
    before = block_sum_i32(before, s_i + 8);
    if (tid == 0) {
        if (logprob) logprob[r] = xt - (gm + logf(s));
        if (rank) rank[r] = before;
    }
}

template <typename T>
__global__ __launch_bounds__(SEL_THREADS) void decode_select_kernel(const T* __restrict__ logits, int64_t ld, int vocab,
                                                                    const uint32_t* __restrict__ allow, const uint32_t* __restrict__ allow_early,
                                                                    const int32_t* __restrict__ n_generated, int32_t min_new,
                                                                    int64_t* __restrict__ token, float* __restrict__ logprob,
                                                                    int32_t* __restrict__ rank, int vec_ok) {
    select_row<T>(logits, ld, vocab, allow, allow_early, n_generated, min_new, token, logprob, rank, vec_ok, PenNone{});
}

// ssi_decode_select_pen (ABI v22): the row's history is built in dynamic LDS first (decode_penalty.h), then the same body chooses on y.
template <typename T>
__global__ __launch_bounds__(SEL_THREADS) void select_pen_kernel(const T* __restrict__ logits, int64_t ld, int vocab,
                                                                 const uint32_t* __restrict__ allow, const uint32_t* __restrict__ allow_early,
                                                                 const int32_t* __restrict__ n_generated, int32_t min_new,
                                                                 int64_t* __restrict__ token, float* __restrict__ logprob,
                                                                 int32_t* __restrict__ rank, int vec_ok, PenArgs pa) {
    extern __shared__ __attribute__((aligned(16))) uint32_t pen_lds[];
    const PenOn pen = pen_build(pa, n_generated, blockIdx.x, vocab, threadIdx.x, pen_lds);
    select_row<T>(logits, ld, vocab, allow, allow_early, n_generated, min_new, token, logprob, rank, vec_ok, pen);
}

// =====================================================================================================================
// ssi_topk_logprob (ABI v20, beam search): the k best allowed columns of a row with their log-probabilities, and the row's log-normaliser.
//
// The two walks of decode_select_kernel.  Walk 1 takes the maximum over all real columns and keeps, per thread, the K best allowed (key,
// column) pairs it met, sorted, in registers (compile-time indices only: no scratch).  The key of a value orders the stored numbers as
// unsigned integers: NaN below every number, -0 with +0, nothing at 0 (an empty place).  A thread meets its columns in rising order, so a
// new pair enters only above a strictly smaller key and the lower column stays ahead among equals.  Then k rounds pick the best head of
// the 256 lists — the xor tree and the wave order of decode_select_kernel, the lower column winning a tie — and the owner pops it.  Walk 2 is
// that kernel's exp-sum, term for term, so lse has its rounding points and lp = fl(x - lse) its bound.
// =====================================================================================================================

// is (bk, bi) ahead of (ak, ai)?  Key 0 is "none".
__device__ __forceinline__ bool topk_ahead(uint32_t ak, int ai, uint32_t bk, int bi) { return bk > ak || (bk == ak && bk != 0 && bi < ai); }

template <typename T, int K>
__global__ __launch_bounds__(SEL_THREADS) void topk_logprob_kernel(const T* __restrict__ logits, int64_t ld, int vocab, int k,
                                                                   const uint32_t* __restrict__ mask, int32_t* __restrict__ idx,
                                                                   float* __restrict__ lp, float* __restrict__ lse, int vec_ok) {
    constexpr int VEC = Vec16<T>::N;
    __shared__ float s_f[16];
    __shared__ int s_i[16];
    __shared__ uint32_t s_k[SEL_WAVES];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const T* __restrict__ x = logits + r * ld;
    const int nvec = vec_ok ? vocab / VEC : 0;
    const int tail0 = nvec * VEC;

    // ---- walk 1 ------------------------------------------------------------------------------------------------------------------
    float gm = -INFINITY;
    uint32_t key[K];
    int at[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        key[i] = 0u;
        at[i] = -1;
    }
    auto visit = [&](int c, float f, bool allowed) {
        gm = fmaxf(gm, f);
        const uint32_t nk = topk_key(f);
        if (allowed && nk > key[K - 1]) {                 // (rare once the lists have filled: a wave skips the insertion when no lane takes it)
#pragma unroll
            for (int i = K - 1; i > 0; --i) {             // every place the new pair passes takes what stood above it, the first one the pair
                const bool up = nk > key[i], up_prev = nk > key[i - 1];
                at[i] = up ? (up_prev ? at[i - 1] : c) : at[i];
                key[i] = up ? (up_prev ? key[i - 1] : nk) : key[i];
            }
            at[0] = nk > key[0] ? c : at[0];
            key[0] = nk > key[0] ? nk : key[0];
        }
    };
    auto visit_vec = [&](int c0, const Vec16<T>& xv, uint32_t bits) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) visit(c0 + e, xv.get(e), (bits & (1u << e)) != 0);
    };
    if (mask) sel_walk<T, true>(x, mask, nvec, tid, visit_vec);
    else sel_walk<T, false>(x, mask, nvec, tid, visit_vec);
    for (int c = tail0 + tid; c < vocab; c += SEL_THREADS) visit(c, to_f32<T>(x[c]), (sel_mask_bits(mask, c) & 1u) != 0);
    gm = wave_max(gm);
    if (lane == 0) s_f[wave] = gm;
    __syncthreads();
    gm = fmaxf(fmaxf(s_f[0], s_f[1]), fmaxf(s_f[2], s_f[3]));

    // ---- the k best heads, one per round ------------------------------------------------------------------------------------------
    int my_idx = -1;                                      // thread j < k keeps result j
    for (int j = 0; j < k; ++j) {
        uint32_t bk = key[0];
        int bi = at[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t ok = (uint32_t)__shfl_xor((int)bk, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (topk_ahead(bk, bi, ok, oi)) {
                bk = ok;
                bi = oi;
            }
        }
        __syncthreads();                                  // (the previous round's reads of s_k / s_i are over)
        if (lane == 0) {
            s_k[wave] = bk;
            s_i[wave] = bi;
        }
        __syncthreads();
        bk = s_k[0];
        bi = s_i[0];
#pragma unroll
        for (int w = 1; w < SEL_WAVES; ++w) {
            if (topk_ahead(bk, bi, s_k[w], s_i[w])) {
                bk = s_k[w];
                bi = s_i[w];
            }
        }
        if (bk == 0u) bi = -1;                            // nothing allowed is left (uniform over the workgroup)
        if (tid == j) my_idx = bi;
        if (bi >= 0 && at[0] == bi) {                     // the owner pops its head (columns are distinct)
#pragma unroll
            for (int i = 0; i + 1 < K; ++i) {
                key[i] = key[i + 1];
                at[i] = at[i + 1];
            }
            key[K - 1] = 0u;
            at[K - 1] = -1;
        }
    }

    // ---- walk 2: decode_select_kernel's exp-sum over all real columns --------------------------------------------------------------
    const float nm = -gm * SEL_LOG2E;
    float s = 0.f;
    sel_walk<T, false>(x, nullptr, nvec, tid, [&](int, const Vec16<T>& xv, uint32_t) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) s += __builtin_amdgcn_exp2f(__builtin_fmaf(xv.get(e), SEL_LOG2E, nm));
    });
    for (int c = tail0 + tid; c < vocab; c += SEL_THREADS) s += __builtin_amdgcn_exp2f(__builtin_fmaf(to_f32<T>(x[c]), SEL_LOG2E, nm));
    s = block_sum(s, s_f + 8);
    const float row_lse = gm + logf(s);
    if (tid == 0 && lse) lse[r] = row_lse;
    if (tid < k) {
        idx[r * k + tid] = my_idx;
        lp[r * k + tid] = my_idx >= 0 ? to_f32<T>(x[my_idx]) - row_lse : -INFINITY;
    }
}

}  // namespace

extern "C" int ssi_topk_logprob(const void* logits, int64_t ld, int64_t rows, int64_t vocab, int k, const uint32_t* mask, int64_t mask_words,
                                int32_t* idx, float* lp, float* lse, int dtype, void* stream) {
    SSI_CHECK_ARG(rows >= 0 && rows < (1LL << 31) && (dtype == SSI_F32 || dtype == SSI_BF16));
    SSI_CHECK_ARG(k >= 1 && k <= 8);
    SSI_CHECK_ARG(logits && idx && lp && vocab >= 1 && ld >= vocab && vocab < (1LL << 31));
    SSI_CHECK_ARG(mask ? mask_words == (vocab + 31) / 32 : mask_words == 0);
    if (rows == 0) return SSI_OK;
    const int64_t esize = dtype == SSI_BF16 ? 2 : 4;
    const int vec_ok = ((uintptr_t)logits & 15) == 0 && (ld * esize) % 16 == 0;
#define SSI_TOPK_K(KK)                                                                                                                        \
    hipLaunchKernelGGL((topk_logprob_kernel<T, KK>), dim3((unsigned)rows), dim3(SEL_THREADS), 0, (hipStream_t)stream, (const T*)logits, ld, \
                       (int)vocab, k, mask, idx, lp, lse, vec_ok)
    SSI_DISPATCH_DTYPE(dtype, {
        if (k == 1) SSI_TOPK_K(1);
        else if (k == 2) SSI_TOPK_K(2);
        else if (k <= 4) SSI_TOPK_K(4);
        else SSI_TOPK_K(8);
    });
#undef SSI_TOPK_K
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

extern "C" int ssi_decode_select(const void* logits, int64_t ld, int64_t rows, int64_t vocab, const uint32_t* allow, const uint32_t* allow_early,
                                 const int32_t* n_generated, int32_t min_new, int64_t* token, float* logprob, int32_t* rank, int dtype,
                                 void* stream) {
    SSI_CHECK_ARG(rows >= 0 && rows < (1LL << 31) && (dtype == SSI_F32 || dtype == SSI_BF16));
    SSI_CHECK_ARG(logits && token && vocab >= 1 && ld >= vocab && vocab < (1LL << 31) && min_new >= 0);
    if (rows == 0) return SSI_OK;
    const int64_t esize = dtype == SSI_BF16 ? 2 : 4;
    const int vec_ok = ((uintptr_t)logits & 15) == 0 && (ld * esize) % 16 == 0;
    SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(decode_select_kernel<T>, dim3((unsigned)rows), dim3(SEL_THREADS), 0, (hipStream_t)stream,
                                                 (const T*)logits, ld, (int)vocab, allow, allow_early, n_generated, min_new, token, logprob, rank,
                                                 vec_ok));
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

extern "C" int64_t ssi_decode_penalty_lds_bytes(int64_t vocab, int64_t ld_gen) {
    return vocab >= 1 && vocab < (1LL << 31) && ld_gen >= 0 && ld_gen < (1LL << 30) ? pen_lds_bytes(vocab, ld_gen) : -1;
}

extern "C" int ssi_decode_select_pen(const void* logits, int64_t ld, int64_t rows, int64_t vocab, const uint32_t* allow, const uint32_t* allow_early,
                                     const int32_t* n_generated, int32_t min_new, int64_t* token, float* logprob, int32_t* rank,
                                     const int32_t* prompt_ids, int64_t ld_prompt, const int32_t* prompt_len, const int32_t* prompt_row,
                                     int64_t n_prompts, const int64_t* gen_ids, int64_t ld_gen, double repetition_penalty, double frequency_penalty,
                                     double presence_penalty, int32_t* n_bad, int dtype, void* stream) {
    SSI_CHECK_ARG(rows >= 0 && rows < (1LL << 31) && (dtype == SSI_F32 || dtype == SSI_BF16));
    SSI_CHECK_ARG(logits && token && vocab >= 1 && ld >= vocab && vocab < (1LL << 31) && min_new >= 0);
    PenArgs pa;
    const int rc = pen_check(pa, vocab, n_generated, prompt_ids, ld_prompt, prompt_len, prompt_row, n_prompts, gen_ids, ld_gen,
                             repetition_penalty, frequency_penalty, presence_penalty, n_bad);
    if (rc != SSI_OK) return rc;
    if (rows == 0) return SSI_OK;
    const int64_t esize = dtype == SSI_BF16 ? 2 : 4;
    const int vec_ok = ((uintptr_t)logits & 15) == 0 && (ld * esize) % 16 == 0;
    SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(select_pen_kernel<T>, dim3((unsigned)rows), dim3(SEL_THREADS),
                                                 (size_t)pen_lds_bytes(vocab, ld_gen), (hipStream_t)stream, (const T*)logits, ld, (int)vocab, allow,
                                                 allow_early, n_generated, min_new, token, logprob, rank, vec_ok, pa));
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}
