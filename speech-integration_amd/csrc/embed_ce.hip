// K1 embedding gather / deterministic scatter-add, and K9 cross-entropy over the DSU-extended vocabulary.
#include "common_hip.h"

// =====================================================================================================================
// K1 forward: out[t,:] = table[tokens[t],:]   (coalesced 16-B row copies; one block of 256 lanes per 4 KiB of row)
// =====================================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void embed_fwd_kernel(const int64_t* __restrict__ tokens, const T* __restrict__ table,
                                                        T* __restrict__ out, int64_t n_tok, int dim, int64_t vocab) {
    constexpr int N = Vec16<T>::N;
    const int nvec = dim / N;
    for (int64_t t = blockIdx.x; t < n_tok; t += gridDim.x) {
        const int64_t tok = tokens[t];
        const bool ok = tok >= 0 && tok < vocab;
        for (int v = threadIdx.x; v < nvec; v += 256) {
            Vec16<T> a;
            if (ok) a = load16(table + tok * dim + v * N);
            else
#pragma unroll
                for (int i = 0; i < N; ++i) a.set(i, 0.f);
            store16(out + t * dim + v * N, a);
        }
    }
}

extern "C" int ssi_embed_fwd(const int64_t* tokens, const void* table, void* out, int64_t n_tok, int64_t dim,
                             int64_t vocab, int dtype, void* stream) {
    if (n_tok == 0) return SSI_OK;
    SSI_CHECK_ARG(tokens && table && out && n_tok > 0 && dim > 0 && dim % 8 == 0 && vocab > 0);
    const unsigned grid = (unsigned)(n_tok < 65536 ? n_tok : 65536);
    SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(embed_fwd_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, tokens,
                                                 (const T*)table, (T*)out, n_tok, (int)dim, vocab));
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

// =====================================================================================================================
// K1 backward: dtable[v,:] += sum over positions t with tokens[t]==v of dout[t,:]
//   pass 1: first[v] = min t, count[v] = #occurrences            (integer atomics: order-independent results)
//   pass 2: one wave per position t; only the wave with t == first[token] works: it scans the token array forward in
//           64-wide chunks (ballot), adds the matching rows in increasing t (fixed order => bitwise reproducible, no float
//           atomics), stops after count[v] matches, and does ONE read-modify-write of the table row.
// =====================================================================================================================
__global__ __launch_bounds__(256) void embed_index_kernel(const int64_t* __restrict__ tokens, int64_t n_tok, int64_t vocab,
                                                          int* __restrict__ first, int* __restrict__ count) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tok) return;
    const int64_t tok = tokens[t];
    if (tok < 0 || tok >= vocab) return;
    atomicMin(&first[tok], (int)t);
    atomicAdd(&count[tok], 1);
}

template <typename T, int MAXV>
__global__ __launch_bounds__(256) void embed_bwd_kernel(const int64_t* __restrict__ tokens, const T* __restrict__ dout,
                                                        T* __restrict__ dtable, int64_t n_tok, int dim, int64_t vocab,
                                                        const int* __restrict__ first, const int* __restrict__ count) {
    constexpr int N = Vec16<T>::N;
    const int lane = threadIdx.x & 63;
    const int64_t t0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t0 >= n_tok) return;
    const int64_t tok = tokens[t0];
    if (tok < 0 || tok >= vocab) return;
    if (first[tok] != (int)t0) return;  // wave-uniform
    const int need = count[tok];
    const int nvec = dim / N;
    float acc[MAXV][N];
#pragma unroll
    for (int k = 0; k < MAXV; ++k)
#pragma unroll
        for (int i = 0; i < N; ++i) acc[k][i] = 0.f;
    // A frequent token (hundreds of occurrences spread over the sequence) makes this wave the one the launch waits for, and a
    // scan that fetched one 64-position chunk of ids, then the matching row, then the next chunk ... was a chain of dependent
    // memory round trips (0.5 ms at 16 384 tokens).  So: the ids of SCAN chunks are requested together, the positions that match
    // are listed in LDS in increasing order, and their rows are requested ROWS at a time and added in list order.
    constexpr int SCAN = 8, ROWS = 8;
    __shared__ int hits_lds[4][64 * SCAN];
    int* hits = hits_lds[threadIdx.x >> 6];
    int found = 0;
    // every load below is unconditional on a clamped address and its result is masked afterwards: behind a branch hipcc waits for
    // each guarded load before it issues the next, which is the chain all over again
    for (int64_t base0 = (t0 / 64) * 64; base0 < n_tok && found < need; base0 += 64 * SCAN) {
        int64_t tk[SCAN];
#pragma unroll
        for (int u = 0; u < SCAN; ++u) {
            const int64_t idx = base0 + 64 * u + lane;
            tk[u] = tokens[idx < n_tok ? idx : n_tok - 1];
        }
        int n = 0;
#pragma unroll
        for (int u = 0; u < SCAN; ++u) {
            const int64_t idx = base0 + 64 * u + lane;
            const bool hit = idx < n_tok && idx >= t0 && tk[u] == tok;
            const unsigned long long mask = __ballot(hit);
            if (hit) hits[n + __popcll(mask & ((1ull << lane) - 1ull))] = (int)(idx - base0);
            n += __popcll(mask);
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the list is written before it is read back (same wave, no barrier needed)
        if (n == 1) {  // the common case (a token seen once in these 512 positions): one row, no padding requests
            const T* src = dout + (base0 + hits[0]) * dim;
#pragma unroll
            for (int k = 0; k < MAXV; ++k) {
                const int v = lane + k * 64;
                const Vec16<T> r = load16(src + (v < nvec ? v : nvec - 1) * N);
#pragma unroll
                for (int i = 0; i < N; ++i) acc[k][i] += v < nvec ? r.get(i) : 0.f;
            }
        } else
        for (int h0 = 0; h0 < n; h0 += ROWS) {
            int pos[ROWS];
#pragma unroll
            for (int u = 0; u < ROWS; ++u) pos[u] = hits[h0 + u < n ? h0 + u : n - 1];
            Vec16<T> a[ROWS][MAXV];
#pragma unroll
            for (int u = 0; u < ROWS; ++u) {
                const T* src = dout + (base0 + pos[u]) * dim;
#pragma unroll
                for (int k = 0; k < MAXV; ++k) {
                    const int v = lane + k * 64;
                    a[u][k] = load16(src + (v < nvec ? v : nvec - 1) * N);
                }
            }
            __builtin_amdgcn_sched_barrier(0);  // all ROWS x MAXV requests leave before the first is waited for (the scheduler sinks them otherwise)
#pragma unroll
            for (int u = 0; u < ROWS; ++u) {
                const bool row_ok = h0 + u < n;  // wave-uniform
#pragma unroll
                for (int k = 0; k < MAXV; ++k) {
                    const bool ok = row_ok && lane + k * 64 < nvec;
#pragma unroll
                    for (int i = 0; i < N; ++i) acc[k][i] += ok ? a[u][k].get(i) : 0.f;
                }
            }
        }
        found += n;
    }
    T* dst = dtable + tok * dim;
#pragma unroll
    for (int k = 0; k < MAXV; ++k) {
        const int v = lane + k * 64;
        if (v < nvec) {
            Vec16<T> a = load16(dst + v * N);
#pragma unroll
            for (int i = 0; i < N; ++i) a.set(i, a.get(i) + acc[k][i]);
            store16(dst + v * N, a);
        }
    }
}

static inline int64_t embed_ws_vocab_slots(int64_t vocab) { return ssi_align_up(vocab, 64); }
// the workspace holds first[] and count[] over the vocabulary; sized by vocab, reported through n_tok-independent API
extern "C" int64_t ssi_embed_bwd_workspace_bytes(int64_t vocab) { return 2 * embed_ws_vocab_slots(vocab) * (int64_t)sizeof(int); }

template <typename T>
static int launch_embed_bwd(const int64_t* tokens, const T* dout, T* dtable, int64_t n_tok, int dim, int64_t vocab,
                            const int* first, const int* count, hipStream_t st) {
    const int64_t vec_per_lane = ssi_cdiv(dim / Vec16<T>::N, 64);
    const dim3 grid((unsigned)ssi_cdiv(n_tok, 4));
    if (vec_per_lane <= 1) hipLaunchKernelGGL((embed_bwd_kernel<T, 1>), grid, dim3(256), 0, st, tokens, dout, dtable, n_tok, dim, vocab, first, count);
    else if (vec_per_lane <= 2) hipLaunchKernelGGL((embed_bwd_kernel<T, 2>), grid, dim3(256), 0, st, tokens, dout, dtable, n_tok, dim, vocab, first, count);
    else if (vec_per_lane <= 4) hipLaunchKernelGGL((embed_bwd_kernel<T, 4>), grid, dim3(256), 0, st, tokens, dout, dtable, n_tok, dim, vocab, first, count);
    else if (vec_per_lane <= 8) hipLaunchKernelGGL((embed_bwd_kernel<T, 8>), grid, dim3(256), 0, st, tokens, dout, dtable, n_tok, dim, vocab, first, count);
    else { ssi_set_error("embed_bwd: dim %d too large", dim); return SSI_ERR_UNSUPPORTED; }
    return SSI_OK;
}

extern "C" int ssi_embed_bwd(const int64_t* tokens, const void* dout, void* dtable, int64_t n_tok, int64_t dim,
                             int64_t vocab, int dtype, void* workspace, int64_t workspace_bytes, void* stream) {
    if (n_tok == 0) return SSI_OK;
    SSI_CHECK_ARG(tokens && dout && dtable && n_tok > 0 && n_tok < (1LL << 31) && dim > 0 && dim % 8 == 0 && vocab > 0);
    if (!workspace || workspace_bytes < ssi_embed_bwd_workspace_bytes(vocab)) { ssi_set_error("embed_bwd: workspace too small"); return SSI_ERR_WORKSPACE; }
    auto st = (hipStream_t)stream;
    int* first = (int*)workspace;
    int* count = first + embed_ws_vocab_slots(vocab);
    hipError_t e = hipMemsetAsync(first, 0x7f, embed_ws_vocab_slots(vocab) * sizeof(int), st);
    if (e == hipSuccess) e = hipMemsetAsync(count, 0, embed_ws_vocab_slots(vocab) * sizeof(int), st);
    if (e != hipSuccess) { ssi_set_error("embed_bwd: memset failed: %s", hipGetErrorString(e)); return SSI_ERR_HIP + (int)e; }
    hipLaunchKernelGGL(embed_index_kernel, dim3((unsigned)ssi_cdiv(n_tok, 256)), dim3(256), 0, st, tokens, n_tok, vocab, first, count);
    SSI_LAUNCH_CHECK();
    int rc = SSI_OK;
    SSI_DISPATCH_DTYPE(dtype, rc = launch_embed_bwd<T>(tokens, (const T*)dout, (T*)dtable, n_tok, (int)dim, vocab, first, count, st));
    if (rc) return rc;
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

// =====================================================================================================================
// K9 cross-entropy over rows of [rows, ld] logits, five entries:
//   ssi_ce_fwd(_weighted)  row_loss = w (lse - x[label]), row_lse; optional in-place gradient  w (softmax - onehot)
//   ssi_ce_fwd_z           + the auxiliary z-loss z * log^2 Z (opt-in, z_loss_coeff of the trainer).  With lse = log Z and p = softmax:
//                          row_z = w (lse lse)  (the coefficient is applied by the caller)
//                          grad[c] = w (f p[c] - [c == label]),  f = 1 + 2 z lse      (d/dx of lse - x[label] + z lse^2: d lse / dx = p)
//   ssi_ce_fwd_smooth      ssi_ce_fwd_z + label smoothing e (opt-in, label_smoothing of the trainer): the target is (1 - e) onehot + e / vocab.
//                          row_u = w (lse - mean_c x[c])  (the uniform part; the caller forms (1 - e) row_loss + e row_u)
//                          grad[c] = w (f p[c] - (1 - e) [c == label]) - w (e / vocab)
//   ssi_ce_fwd_metrics     forward only, + row_nll = lse - x[label] and the label's rank (the dev set's per-token-type loss, top-1, top-k):
//                          rank[r] = #{c < vocab : x[c] > x[label]} + #{c < label : x[c] == x[label]}  — the label's position in a stable
//                          descending sort of the row; rank == 0 <=> argmax(row) == label under the first-occurrence rule.  Compares on
//                          the stored values: an exact integer.
//   ssi_ce_fwd_kl          ssi_ce_fwd_weighted + b KL(teacher || student) against a frozen teacher's logits (opt-in, teacher_kl_coeff of the
//                          trainer).  With t the teacher row, tlse its lse (an input: a forward-only ssi_ce_fwd on the teacher buffer),
//                          q = exp(t - tlse), k the row's KL weight and bk = b k:
//                          row_kl = k sum_c q[c] ((t[c] - x[c]) - (tlse - lse))  (the coefficient is applied by the caller)
//                          grad[c] = (w + bk) p[c] - w [c == label] - bk q[c]
// Two forms — generic (any dtype and shape; one 512-thread block per row, fp32 online log-sum-exp, the gradient or the rank from a second
// read of the row out of L2 / Infinity Cache) and register-resident bf16 rows (the training step's form) — and in each form ONE body
// templated on the entry's CeMode, ce_generic_body and ce_row_bf16_body: what an entry adds sits behind `if constexpr`, so the max, the
// exp-sum and the lse are the same statements whatever the entry: row_loss and row_lse agree bit for bit across the five, and with z = 0
// (f = 1 exactly), e = 0 (times an exact 1, minus an exact 0) and b = 0 (minus an exact 0) so does the gradient.  The __global__ kernels are wrappers, one per entry
// and form, that pass nullptr / 0 for what is not theirs: the instantiations an entry launches do not depend on what the other entries
// need.  On the host the five entries share one launcher, ce_fwd_launch<MODE>; an entry keeps its own pointer and coefficient checks.
// =====================================================================================================================
enum CeMode { CE_PLAIN, CE_Z, CE_SMOOTH, CE_METRICS, CE_KL };

// what only CE_KL has (ssi_ce_fwd_kl): the frozen teacher's logits, their lse per row from a forward-only ssi_ce_fwd on that buffer, the
// per-row weight k of the KL term (nullptr: the row's w), the coefficient b, and where row_kl goes.  One struct, defaulted: the bodies take it
// last and the other four modes never name it.
struct CeKl {
    const void* teacher = nullptr; int64_t ld_teacher = 0; const float* teacher_lse = nullptr; const float* row_kl_weight = nullptr;
    float beta = 0.f; float* row_kl = nullptr;
};

// a row takes part iff its label is not ignored AND inside [0, vocab)
__device__ __forceinline__ bool ce_label_valid(int64_t label, int64_t vocab, int64_t ignore_index) {
    return label != ignore_index && label >= 0 && label < vocab;
}

// ---- generic form: the pieces (512 threads) ----------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ void ce_zero_row(T* lr, int64_t nvec) {
    constexpr int N = Vec16<T>::N;
    Vec16<T> z;
#pragma unroll
    for (int i = 0; i < N; ++i) z.set(i, 0.f);
    for (int64_t v = threadIdx.x; v < nvec; v += 512) store16(lr + v * N, z);
}

// online log-sum-exp over the columns [0, vocab) of one row
template <typename T> __device__ __forceinline__ float ce_row_lse(const T* lr, int64_t nvec, int64_t vocab, float* red) {
    constexpr int N = Vec16<T>::N;
    float m = -INFINITY, s = 0.f;
    for (int64_t v = threadIdx.x; v < nvec; v += 512) {
        Vec16<T> a = load16(lr + v * N);
        float lm = -INFINITY;
#pragma unroll
        for (int i = 0; i < N; ++i) if (v * N + i < vocab) lm = fmaxf(lm, a.get(i));
        if (lm > m) { s *= expf(m - lm); m = lm; }
#pragma unroll
        for (int i = 0; i < N; ++i) if (v * N + i < vocab) s += expf(a.get(i) - m);
    }
    const float gm = block_max(m, red);
    s = (m == -INFINITY) ? 0.f : s * expf(m - gm);
    const float gs = block_sum(s, red);
    return gm + logf(gs);
}

// plain fp32 sum over the columns [0, vocab) of one row, in a fixed order (per-thread stride, then the block's tree)
template <typename T> __device__ __forceinline__ float ce_row_sum(const T* lr, int64_t nvec, int64_t vocab, float* red) {
    constexpr int N = Vec16<T>::N;
    float s = 0.f;
    for (int64_t v = threadIdx.x; v < nvec; v += 512) {
        Vec16<T> a = load16(lr + v * N);
#pragma unroll
        for (int i = 0; i < N; ++i) if (v * N + i < vocab) s += a.get(i);
    }
    return block_sum(s, red);
}

// the label's rank in its row (see K9): pad columns [vocab, ld) never count
template <typename T> __device__ __forceinline__ int ce_rank_row(const T* lr, int64_t nvec, int64_t vocab, int64_t label, float xl, int* redi) {
    constexpr int N = Vec16<T>::N;
    int cnt = 0;
    for (int64_t v = threadIdx.x; v < nvec; v += 512) {
        Vec16<T> a = load16(lr + v * N);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int64_t c = v * N + i;
            const float x = a.get(i);
            cnt += (int)(c < vocab) & ((int)(x > xl) | ((int)(x == xl) & (int)(c < label)));  // bitwise: no branch per element
        }
    }
    return block_sum_i32(cnt, redi);
}

// in-place gradient of one row, pad columns 0:
//   CE_PLAIN   w (p - onehot): no multiply by 1
//   CE_Z       w (f p - onehot) with the z-loss factor f (ome = 1).  f may have any sign: lse < -1 / (2 z) makes it negative, and the plain
//              multiply carries that
//   CE_SMOOTH  w (f p - ome onehot) - wu on the real columns, ome = 1 - e and wu = w (e / vocab).  e = 0: ome = 1 and wu = 0 exactly — the
//              values of CE_Z
template <CeMode MODE, typename T>
__device__ __forceinline__ void ce_grad_row(T* lr, int64_t nvec, int64_t vocab, int64_t label, float lse, float w, float f, float ome, float wu) {
    constexpr int N = Vec16<T>::N;
    for (int64_t v = threadIdx.x; v < nvec; v += 512) {
        Vec16<T> a = load16(lr + v * N), o;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int64_t c = v * N + i;
            float g = 0.f;
            if (c < vocab) {
                if constexpr (MODE == CE_PLAIN) g = w * (expf(a.get(i) - lse) - (c == label ? 1.f : 0.f));
                else g = w * (f * expf(a.get(i) - lse) - (c == label ? ome : 0.f));
                if constexpr (MODE == CE_SMOOTH) {
                    asm volatile("" : "+v"(g));  // no fma across here: the product is rounded before wu leaves it, as in the register form
                    g -= wu;
                }
            }
            o.set(i, g);
        }
        store16(lr + v * N, o);
    }
}

// CE_KL: one pass over the student row and the teacher row (both from L2 / Infinity Cache after the lse passes) gives, if write_grad, the
// in-place gradient  w (p - onehot) + bk (p - q)  = (w + bk) p - w onehot - bk q,  bk = beta k, q = exp(t - tlse)  (bk = 0: plus an exact 0,
// the values of CE_PLAIN), and this thread's share of three sums in fp64:
//   acc[0] = sum_c Q[c] (t[c] - x[c]),   acc[1] = S = sum_c Q[c],  Q = exp(t - tlse),   acc[2] = SP = sum_c exp(x[c] - lse)
// S and SP are what the two fp32 lse leave of the rows' normalisers (1 up to the rounding of each lse, 2.4e-7 at an lse of 6): the caller forms
//   KL(q || p) = acc[0] / S - (tlse - lse) - log S + log SP
// which is  sum_c q[c] ((t[c] - x[c]) - (tlse - lse))  with the two roundings taken out — this form is not the step's, and a KL of 1e-3
// against a teacher close to the student is then good to 1e-8 where the plain sum stops at the lse's 3e-7.  The teacher row is read up to ITS
// OWN ld (nvec_t vectors; both lds cover the vocabulary) and never written.
template <typename T>
__device__ __forceinline__ void ce_kl_row(T* lr, const T* tr, int64_t nvec, int64_t nvec_t, int64_t vocab, int64_t label, float lse, float tlse,
                                          float w, float bk, int write_grad, double (&acc)[3]) {
    constexpr int N = Vec16<T>::N;
    acc[0] = acc[1] = acc[2] = 0.0;
    for (int64_t v = threadIdx.x; v < nvec; v += 512) {
        Vec16<T> a = load16(lr + v * N), o;
        Vec16<T> b = a;  // beyond the teacher's row: columns that are not vocabulary, never read below
        if (v < nvec_t) b = load16(tr + v * N);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int64_t c = v * N + i;
            float g = 0.f;
            if (c < vocab) {
                const float x = a.get(i), t = b.get(i);
                const float p = expf(x - lse), q = expf(t - tlse);
                const double Q = exp((double)t - (double)tlse);
                acc[0] += Q * ((double)t - (double)x);
                acc[1] += Q;
                acc[2] += exp((double)x - (double)lse);
                g = w * (p - (c == label ? 1.f : 0.f)) + bk * (p - q);
            }
            o.set(i, g);
        }
        if (write_grad) store16(lr + v * N, o);
    }
}

// The body of all five generic kernels, one block per row; the kernels pass nullptr / 0 for what is not theirs (ome = 1 for CE_Z).  A row
// without a valid label skips the passes and keeps lse = xl = sx = 0, w = 1, cnt = -1: every output below is then an exact 0, the rank -1.
template <typename T, CeMode MODE>
__device__ __forceinline__ void ce_generic_body(T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels, int64_t vocab,
                                                int64_t ignore_index, float two_z, float ome, float e_over_v, float* __restrict__ row_loss,
                                                float* __restrict__ row_lse, float* __restrict__ row_z, float* __restrict__ row_u,
                                                float* __restrict__ row_nll, int32_t* __restrict__ row_rank, int write_grad,
                                                const float* __restrict__ row_weight, float* red, int* redi, const CeKl& kl = CeKl{}) {
    const int64_t row = blockIdx.x;
    T* lr = logits + row * ld;
    const int64_t label = labels[row];
    const int64_t nvec = ld / Vec16<T>::N;
    const bool valid = ce_label_valid(label, vocab, ignore_index);  // block-uniform
    float lse = 0.f, sx = 0.f, w = 1.f, xl = 0.f;
    int cnt = -1;
    if (valid) {
        lse = ce_row_lse(lr, nvec, vocab, red);
        if constexpr (MODE == CE_SMOOTH) sx = ce_row_sum(lr, nvec, vocab, red);
        w = row_weight ? row_weight[row] : 1.f;  // weighted rows: loss and gradient of the row times w
        if (MODE == CE_METRICS || threadIdx.x == 0) xl = to_f32<T>(lr[label]);  // block-uniform address
        if constexpr (MODE == CE_METRICS) cnt = ce_rank_row(lr, nvec, vocab, label, xl, redi);  // a second pass over the row (from L2, as the gradient's)
    }
    if (threadIdx.x == 0) {
        row_loss[row] = w * (lse - xl);
        if (row_lse) row_lse[row] = lse;
        if constexpr (MODE == CE_Z) row_z[row] = w * (lse * lse);
        if constexpr (MODE == CE_SMOOTH) {
            if (row_z) row_z[row] = w * (lse * lse);
            row_u[row] = w * (lse - sx / (float)vocab);
        }
        if constexpr (MODE == CE_METRICS) { row_nll[row] = lse - xl; row_rank[row] = cnt; }
    }
    if constexpr (MODE == CE_KL) {  // its one pass runs forward-only too: row_kl comes from it
        if (!valid) {
            if (threadIdx.x == 0) kl.row_kl[row] = 0.f;
            if (write_grad) ce_zero_row(lr, nvec);
            return;
        }
        const float kw = kl.row_kl_weight ? kl.row_kl_weight[row] : w;
        __syncthreads();  // lr[label] read above must precede the overwrite below
        const float tlse = kl.teacher_lse[row];
        double acc[3];
        ce_kl_row<T>(lr, (const T*)kl.teacher + row * kl.ld_teacher, nvec, kl.ld_teacher / Vec16<T>::N, vocab, label, lse, tlse, w, kl.beta * kw,
                     write_grad, acc);
        __shared__ double redd[3][8];  // one slot per wave of the 512 threads; fixed order: the lanes' xor tree, then the waves in turn
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q] = wave_sum_f64(acc[q]);
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) redd[q][threadIdx.x >> 6] = acc[q];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double sum[3] = {0.0, 0.0, 0.0};
            for (int q = 0; q < 3; ++q)
                for (int i = 0; i < 8; ++i) sum[q] += redd[q][i];
            kl.row_kl[row] = kw * (float)(sum[0] / sum[1] - ((double)tlse - (double)lse) - log(sum[1]) + log(sum[2]));
        }
    } else if constexpr (MODE != CE_METRICS) {  // the metrics form is forward only: it never writes the row
        if (!write_grad) return;
        if (!valid) { ce_zero_row(lr, nvec); return; }
        const float f = fmaf(two_z, lse, 1.f);
        __syncthreads();  // lr[label] read above must precede the overwrite below
        ce_grad_row<MODE>(lr, nvec, vocab, label, lse, w, f, ome, w * e_over_v);
    }
}

template <typename T>
__global__ __launch_bounds__(512) void ce_fwd_kernel(T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                     int64_t vocab, int64_t ignore_index, float* __restrict__ row_loss,
                                                     float* __restrict__ row_lse, int write_grad, const float* __restrict__ row_weight) {
    __shared__ float red[16];
    ce_generic_body<T, CE_PLAIN>(logits, ld, labels, vocab, ignore_index, 0.f, 1.f, 0.f, row_loss, row_lse, nullptr, nullptr, nullptr, nullptr,
                                 write_grad, row_weight, red, nullptr);
}

template <typename T>
__global__ __launch_bounds__(512) void ce_fwd_z_kernel(T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                       int64_t vocab, int64_t ignore_index, float two_z, float* __restrict__ row_loss,
                                                       float* __restrict__ row_lse, float* __restrict__ row_z, int write_grad,
                                                       const float* __restrict__ row_weight) {
    __shared__ float red[16];
    ce_generic_body<T, CE_Z>(logits, ld, labels, vocab, ignore_index, two_z, 1.f, 0.f, row_loss, row_lse, row_z, nullptr, nullptr, nullptr,
                             write_grad, row_weight, red, nullptr);
}

template <typename T>
__global__ __launch_bounds__(512) void ce_fwd_smooth_kernel(T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                            int64_t vocab, int64_t ignore_index, float two_z, float ome, float e_over_v,
                                                            float* __restrict__ row_loss, float* __restrict__ row_lse,
                                                            float* __restrict__ row_z, float* __restrict__ row_u, int write_grad,
                                                            const float* __restrict__ row_weight) {
    __shared__ float red[16];
    ce_generic_body<T, CE_SMOOTH>(logits, ld, labels, vocab, ignore_index, two_z, ome, e_over_v, row_loss, row_lse, row_z, row_u, nullptr, nullptr,
                                  write_grad, row_weight, red, nullptr);
}

template <typename T>
__global__ __launch_bounds__(512) void ce_fwd_metrics_kernel(const T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                             int64_t vocab, int64_t ignore_index, float* __restrict__ row_loss,
                                                             float* __restrict__ row_lse, float* __restrict__ row_nll,
                                                             int32_t* __restrict__ row_rank, const float* __restrict__ row_weight) {
    __shared__ float red[16];
    __shared__ int redi[16];
    ce_generic_body<T, CE_METRICS>(const_cast<T*>(logits), ld, labels, vocab, ignore_index, 0.f, 1.f, 0.f, row_loss, row_lse, nullptr, nullptr,
                                   row_nll, row_rank, 0, row_weight, red, redi);
}

template <typename T>
__global__ __launch_bounds__(512) void ce_kl_generic_kernel(T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                            int64_t vocab, int64_t ignore_index, CeKl kl, float* __restrict__ row_loss,
                                                            float* __restrict__ row_lse, int write_grad,
                                                            const float* __restrict__ row_weight) {
    __shared__ float red[16];
    ce_generic_body<T, CE_KL>(logits, ld, labels, vocab, ignore_index, 0.f, 1.f, 0.f, row_loss, row_lse, nullptr, nullptr, nullptr, nullptr,
                              write_grad, row_weight, red, nullptr, kl);
}

// ---- bf16 rows held in registers (the training step's form) -------------------------------------------------------------------------------
// One 1024-thread workgroup per CU walks rows; a row of NCH x 8192 logits (NCH = 17: 139 264 >= 133 376) lives in NCH 16-byte registers
// per thread, so the log-sum-exp and the gradient both come from ONE read of the row: 2 passes over the logits (read + write back = 8.7 GB
// at T = 16 384, V = 133 258) instead of the 3 of ce_fwd_kernel above (13.1 GB).  A register's next-row load is issued as soon as its
// gradient has been stored, so the next row streams in under the stores and the exps of the current one.  NCH = ceil(ld / 8192) exactly
// and ld - vocab < 8192: only the last two chunks can hold columns that are not vocabulary.  Straight-line body (the only branches are
// workgroup-uniform and read-only on the row registers): with per-chunk branches hipcc spills the row.
//
// The body of all five row kernels; what an entry adds sits behind `if constexpr` on MODE, and the kernels pass nullptr / 0 for what is
// not theirs:
//   CE_Z        one scalar per row.  |f| rides in the exponent's additive term beside log2 w (f = 0: log2 0 = -inf, every exp2 gives 0 —
//               the row is -w on the label and 0 elsewhere).  The SIGN of f is applied to the packed result: the row computes
//               w |f| p - sign(f) w [c == label]  and, for f < 0, flips the sign bit of all eight bf16 of a register (4 XORs per chunk with
//               a per-row mask that is 0 otherwise; round-to-nearest-even is symmetric in the sign, so this IS the rounding of
//               w (f p - onehot)).  No branch per chunk.  (For f < 0 the columns whose gradient is 0 — pads, underflows — hold -0.)
//   CE_SMOOTH   CE_Z and two more scalars per row (every CE_Z statement runs; z = 0 makes them the exact no-ops they already are).  The
//               label column subtracts wl = sign(f) w (1 - e) and every REAL column sign(f) wu, wu = w (e / vocab), both before the
//               sign flip: the row computes  w |f| p - wl [c == label] - sign(f) wu.  Only the last two chunks can hold columns that are
//               not vocabulary; there the constant is selected per element with the `left` compare of the masking loop (a v_cndmask, no
//               branch), elsewhere it is subtracted unconditionally.  The same select keeps the -inf of the pads out of the plain sum of
//               the row (row_u), one more pass over the packed registers.  e = 0: minus an exact 0, times an exact 1 — CE_Z bit for bit.
//   CE_METRICS  no gradient (write_grad is false) and one more pass over the packed registers: compare with the label's logit and count.
//               Every lane needs that logit before the pass; the label is workgroup-uniform and nothing is overwritten here, so each
//               lane loads it itself from one address and nothing has to wait for it to land.  The pad columns are -inf in the
//               registers and lie above every valid label: they are neither greater than a logit nor tie below the label.
//   CE_KL       the teacher's row never lives in registers: with both lse known, the gradient loop reads the teacher's 16 bytes of this lane
//               and chunk (same buffer addressing; ld_teacher == ld), forms q = exp2(t log2e - tlse log2e) and adds q ((t - x) - (tlse - lse))
//               to the lane's share of row_kl; the gradient is  exp2(x log2e + nl) - w [c == label] - bk q  with log2 (w + bk) in nl beside
//               -lse log2e, bk = beta k.  TD teacher chunks are in flight ahead of the one in use, in a ring of TD registers.  The pads are
//               -inf in the row registers (t - x = inf, 0 inf = NaN) and 0 where the teacher's load lay beyond the row: in the last two
//               chunks q and the product are selected per element with the `left` compare.  bk = 0: minus an exact 0 — CE_PLAIN bit for
//               bit.  A row without a label: q = exp2(-inf) = 0 and bk = 0.  Forward-only the loop still runs, for row_kl, and stores nothing.

template <int NCH, CeMode MODE, bool write_grad>
__device__ __forceinline__ void ce_row_bf16_body(bf16_t* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels, int64_t rows,
                                                 int64_t vocab, int64_t ignore_index, float two_z, float ome, float e_over_v,
                                                 float* __restrict__ row_loss, float* __restrict__ row_lse, float* __restrict__ row_z,
                                                 float* __restrict__ row_u, float* __restrict__ row_nll, int32_t* __restrict__ row_rank,
                                                 const float* __restrict__ row_weight, float* red, int* redi, const CeKl& kl = CeKl{}) {
    static_assert(MODE != CE_METRICS || !write_grad, "the metrics form writes no gradient");
    constexpr bool KL = MODE == CE_KL;
    constexpr int TD = NCH < 3 ? NCH : 3;            // CE_KL: teacher chunks in flight
    constexpr bool WITH_F = MODE == CE_Z || MODE == CE_SMOOTH;  // the z-loss factor f and its sign flip
    constexpr bool SMOOTH = MODE == CE_SMOOTH;                  // ome = 1 - e, e_over_v = e / vocab (0 and unused otherwise)
    constexpr float LOG2E = 1.44269504088896340736f;
    constexpr int CHUNK = 8192;                      // columns per chunk: 1024 threads x 8 bf16
    const int tid = threadIdx.x;
    const int voff = tid * 16;                       // the one per-lane byte offset; the chunk rides in the scalar offset
    const int col0 = tid * 8;                        // this lane's first column inside a chunk
    const int row_bytes = (int)(ld * 2);             // buffer bound: loads beyond the row return 0, stores beyond it are dropped
    const int vocab_i = (int)vocab;
    u32x4 x[NCH];
    auto rsrc_of = [&](int64_t row) { return __builtin_amdgcn_make_buffer_rsrc(logits + row * ld, 0, row_bytes, 0x00020000u); };
    [[maybe_unused]] u32x4 tq[TD];                   // CE_KL: the ring of teacher chunks
    auto lo = [](unsigned u) { return __builtin_bit_cast(float, u << 16); };
    auto hi = [](unsigned u) { return __builtin_bit_cast(float, u & 0xffff0000u); };
    // the passes each re-derive the fp32 values from the packed registers: without this opaque touch the compiler keeps all
    // 8 x NCH converted floats alive across the passes and spills
    auto opaque = [&]() {
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int d = 0; d < 4; ++d) asm volatile("" : "+v"(x[c][d]));
    };
    int64_t row = blockIdx.x;
    if (row >= rows) return;
    {
        const __amdgpu_buffer_rsrc_t r0 = rsrc_of(row);
#pragma unroll
        for (int c = 0; c < NCH; ++c) x[c] = __builtin_amdgcn_raw_buffer_load_b128(r0, voff, c * CHUNK * 2, 0);
    }
    for (; row < rows; row += gridDim.x) {
        const int64_t next = row + gridDim.x;
        const int64_t label = labels[row];
        const bool valid = ce_label_valid(label, vocab, ignore_index);
        // a weighted row (ssi_ce_fwd_weighted): w * exp(x - lse) = exp2(x log2e - lse log2e + log2 w) — the weight rides in the exponent's
        // additive term at no cost per element; w = 1 (and no weights) adds an exact 0
        const float w = row_weight ? row_weight[row] : 1.f;
        float log2w = row_weight ? __log2f(w) : 0.f;
        const __amdgpu_buffer_rsrc_t rs = rsrc_of(row);
        // CE_KL: the row's k and bk = beta k; w + bk rides in the exponent where w does (beta = 0: w + 0 k = w)
        [[maybe_unused]] float kw = 0.f, bk = 0.f, dl = 0.f, nq = -INFINITY, klacc = 0.f;
        [[maybe_unused]] __amdgpu_buffer_rsrc_t rt = rs;
        if constexpr (KL) {
            kw = kl.row_kl_weight ? kl.row_kl_weight[row] : w;
            rt = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>((const bf16_t*)kl.teacher) + row * ld, 0, row_bytes, 0x00020000u);
        }
        // columns that are not vocabulary (the pad columns [vocab, ld), and beyond the row where the loads returned 0) become -inf
        // once, in the registers: max, exp-sum, gradient (exp2(-inf) = 0) and rank then need no column test at all
#pragma unroll
        for (int c = (NCH >= 2 ? NCH - 2 : 0); c < NCH; ++c) {
            const int left = vocab_i - c * CHUNK - col0;  // real columns from this lane's first one on
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                if (2 * d >= left) x[c][d] = (x[c][d] & 0xffff0000u) | 0x0000ff80u;
                if (2 * d + 1 >= left) x[c][d] = (x[c][d] & 0x0000ffffu) | 0xff800000u;
            }
        }
        float nl = -INFINITY;  // ignored / out-of-range label: every exp2 below gives 0 -> zero gradient row
        float wl = w;          // what the label column subtracts BEFORE the sign flip: sign(f) w  (CE_Z; w otherwise), times 1 - e (CE_SMOOTH)
        float wus = 0.f;       // what every real column subtracts BEFORE the sign flip: sign(f) w (e / vocab)  (CE_SMOOTH; 0 on a row without a label)
        unsigned flip = 0u;    // sign bits of the two bf16 of a packed dword, set iff f < 0  (CE_Z, CE_SMOOTH)
        if (valid) {           // workgroup-uniform; reads the row registers only
            float xl = 0.f;    // before this row's gradient is written (program order of one thread)
            if (MODE == CE_METRICS || tid == 0) xl = (float)logits[row * ld + label];
            float m = -INFINITY;
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int d = 0; d < 4; ++d) m = fmaxf(m, fmaxf(lo(x[c][d]), hi(x[c][d])));
            // thread 0's label logit must have LANDED before any wave may overwrite that address with the gradient: the barrier inside
            // block_max only orders issue.  Free here: the row registers the max just consumed were the only other loads in flight.
            if constexpr (MODE != CE_METRICS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const float gm = block_max(m, red);
            if constexpr (KL) {  // the first teacher chunks fly under the exp-sum pass (issued after the wait above, which they would lengthen)
#pragma unroll
                for (int i = 0; i < TD; ++i) tq[i] = __builtin_amdgcn_raw_buffer_load_b128(rt, voff, i * CHUNK * 2, 2 /* nt */);
            }
            opaque();
            const float nm = -gm * LOG2E;
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int d = 0; d < 4; ++d)
                    s += __builtin_amdgcn_exp2f(fmaf(lo(x[c][d]), LOG2E, nm)) + __builtin_amdgcn_exp2f(fmaf(hi(x[c][d]), LOG2E, nm));
            const float gs = block_sum(s, red);
            const float lse = gm + logf(gs);
            float gsx = 0.f;
            if constexpr (SMOOTH) {
                opaque();
                // ---- the plain sum of the real columns, a pass of its own (fused into the exp-sum pass, the row spilled): the pads are -inf
                // in the registers, select 0 for them
                float sx = 0.f;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const int left = vocab_i - c * CHUNK - col0;  // as in the masking loop; read in the last two chunks only
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        if (c < NCH - 2) sx += lo(x[c][d]) + hi(x[c][d]);
                        else sx += (2 * d < left ? lo(x[c][d]) : 0.f) + (2 * d + 1 < left ? hi(x[c][d]) : 0.f);
                    }
                }
                gsx = block_sum(sx, red);
            }
            int cnt = 0;
            if constexpr (MODE == CE_METRICS) {
                opaque();
                // ---- the rank pass: element e of chunk c is column c * CHUNK + col0 + e; it ties BELOW the label iff e < below - c * CHUNK
                const int below = (int)label - col0;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const int b = below - c * CHUNK;
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const float a0 = lo(x[c][d]), a1 = hi(x[c][d]);
                        // bitwise on purpose: || and && became a branch per element, and the row spilled
                        cnt += (int)(a0 > xl) | ((int)(a0 == xl) & (int)(2 * d < b));
                        cnt += (int)(a1 > xl) | ((int)(a1 == xl) & (int)(2 * d + 1 < b));
                    }
                }
                cnt = block_sum_i32(cnt, redi);
            }
            if (tid == 0) {
                row_loss[row] = w * (lse - xl);
                if (row_lse) row_lse[row] = lse;
                if constexpr (MODE == CE_Z) row_z[row] = w * (lse * lse);
                if constexpr (SMOOTH) {
                    if (row_z) row_z[row] = w * (lse * lse);
                    row_u[row] = w * (lse - gsx / (float)vocab_i);
                }
                if constexpr (MODE == CE_METRICS) { row_nll[row] = lse - xl; row_rank[row] = cnt; }
            }
            if constexpr (KL) {
                const float tlse = kl.teacher_lse[row];
                bk = kl.beta * kw;
                log2w = __log2f(w + bk);
                dl = tlse - lse;
                nq = -tlse * LOG2E;
            }
            nl = fmaf(-lse, LOG2E, log2w);  // (said as the fma it is compiled to: every mode forms the same nl, whatever else uses lse)
            if constexpr (WITH_F) {
                const float f = fmaf(two_z, lse, 1.f);
                nl += __log2f(fabsf(f));  // z = 0: f = 1 and this term an exact 0 — the nl of CE_PLAIN
                if constexpr (SMOOTH) { wl = w * ome; wus = w * e_over_v; }  // e = 0: w and 0, exactly
                if (f < 0.f) { wl = -wl; wus = -wus; flip = 0x80008000u; }
            }
        } else {
            if constexpr (KL) {  // no teacher loads for this row: defined values for the loop, whose q is exp2(-inf) = 0
#pragma unroll
                for (int i = 0; i < TD; ++i) tq[i] = u32x4{0u, 0u, 0u, 0u};
            }
            if (tid == 0) {
            row_loss[row] = 0.f;
            if (row_lse) row_lse[row] = 0.f;
            if constexpr (MODE == CE_Z) row_z[row] = 0.f;
            if constexpr (SMOOTH) { if (row_z) row_z[row] = 0.f; row_u[row] = 0.f; }
            if constexpr (MODE == CE_METRICS) { row_nll[row] = 0.f; row_rank[row] = -1; }
            }
        }
        opaque();
        // ---- gradient softmax - onehot, written over the logits; each register then takes the next row's chunk (past the last row:
        // this row again — a few wasted loads at the very end instead of a branch around every load)
        const int hot = valid ? (int)label - col0 : -(1 << 30);  // the label's column relative to this lane's first column of chunk 0
        const __amdgpu_buffer_rsrc_t rn = rsrc_of(next < rows ? next : row);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            if constexpr (KL) {
                const u32x4 tc = tq[c % TD];
                const int left = vocab_i - c * CHUNK - col0;  // as in the masking loop; read in the last two chunks only
                const int h = hot - c * CHUNK;
                float g[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float xe = (e & 1) ? hi(x[c][e >> 1]) : lo(x[c][e >> 1]);
                    const float te = (e & 1) ? hi(tc[e >> 1]) : lo(tc[e >> 1]);
                    float q = __builtin_amdgcn_exp2f(fmaf(te, LOG2E, nq));
                    float term = q * ((te - xe) - dl);
                    if (c >= NCH - 2) {  // a pad column or beyond the row: neither its q nor its NaN / inf product counts
                        q = e < left ? q : 0.f;
                        term = e < left ? term : 0.f;
                    }
                    klacc += term;
                    if (write_grad) {
                        const float pe = __builtin_amdgcn_exp2f(fmaf(xe, LOG2E, nl)) - (e == h ? wl : 0.f);
                        g[e] = pe - bk * q;
                    }
                }
                if (write_grad) {
                    bf16x8 ob;
#pragma unroll
                    for (int e = 0; e < 8; ++e) ob[e] = (bf16_t)g[e];
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, ob), rs, voff, c * CHUNK * 2, 2 /* nt: streamed once */);
                }
                // this ring register takes the teacher chunk TD ahead (valid or not: the loads of a row without a label are never used)
                if (c + TD < NCH) tq[c % TD] = __builtin_amdgcn_raw_buffer_load_b128(rt, voff, (c + TD) * CHUNK * 2, 2 /* nt */);
            } else if (write_grad) {
                float g[8];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    g[2 * d] = __builtin_amdgcn_exp2f(fmaf(lo(x[c][d]), LOG2E, nl));
                    g[2 * d + 1] = __builtin_amdgcn_exp2f(fmaf(hi(x[c][d]), LOG2E, nl));
                }
                const int h = hot - c * CHUNK;
                if ((unsigned)h < 8u) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) if (e == h) g[e] -= wl;
                }
                if constexpr (SMOOTH) {  // after the label's term: a column whose p underflowed holds the rounding of -wu
                    const int left = vocab_i - c * CHUNK - col0;
#pragma unroll
                    for (int e = 0; e < 8; ++e) g[e] -= (c < NCH - 2 || e < left) ? wus : 0.f;
                }
                bf16x8 ob;
#pragma unroll
                for (int e = 0; e < 8; ++e) ob[e] = (bf16_t)g[e];
                u32x4 o = __builtin_bit_cast(u32x4, ob);
                if constexpr (WITH_F) {
#pragma unroll
                    for (int d = 0; d < 4; ++d) o[d] ^= flip;
                }
                __builtin_amdgcn_raw_buffer_store_b128(o, rs, voff, c * CHUNK * 2, 2 /* nt: streamed once */);
            }
            x[c] = __builtin_amdgcn_raw_buffer_load_b128(rn, voff, c * CHUNK * 2, 2 /* nt */);
            __builtin_amdgcn_sched_barrier(0);  // one chunk at a time: a hoisted next-row load would need a register of its own
        }
        if constexpr (KL) {  // the lanes' shares of row_kl, summed under the next row's loads
            const float skl = block_sum(klacc, red);
            if (tid == 0) kl.row_kl[row] = valid ? kw * skl : 0.f;
        }
    }
}

template <int NCH, bool write_grad>
__global__ __launch_bounds__(1024, 4) void ce_row_bf16_kernel(bf16_t* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                              int64_t rows, int64_t vocab, int64_t ignore_index,
                                                              float* __restrict__ row_loss, float* __restrict__ row_lse,
                                                              const float* __restrict__ row_weight) {
    __shared__ float red[16];
    ce_row_bf16_body<NCH, CE_PLAIN, write_grad>(logits, ld, labels, rows, vocab, ignore_index, 0.f, 1.f, 0.f, row_loss, row_lse, nullptr, nullptr,
                                                nullptr, nullptr, row_weight, red, nullptr);
}

template <int NCH, bool write_grad>
__global__ __launch_bounds__(1024, 4) void ce_row_bf16_z_kernel(bf16_t* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                                int64_t rows, int64_t vocab, int64_t ignore_index, float two_z,
                                                                float* __restrict__ row_loss, float* __restrict__ row_lse,
                                                                float* __restrict__ row_z, const float* __restrict__ row_weight) {
    __shared__ float red[16];
    ce_row_bf16_body<NCH, CE_Z, write_grad>(logits, ld, labels, rows, vocab, ignore_index, two_z, 1.f, 0.f, row_loss, row_lse, row_z, nullptr,
                                            nullptr, nullptr, row_weight, red, nullptr);
}

template <int NCH, bool write_grad>
__global__ __launch_bounds__(1024, 4) void ce_row_bf16_smooth_kernel(bf16_t* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                                     int64_t rows, int64_t vocab, int64_t ignore_index, float two_z, float ome,
                                                                     float e_over_v, float* __restrict__ row_loss, float* __restrict__ row_lse,
                                                                     float* __restrict__ row_z, float* __restrict__ row_u,
                                                                     const float* __restrict__ row_weight) {
    __shared__ float red[16];
    ce_row_bf16_body<NCH, CE_SMOOTH, write_grad>(logits, ld, labels, rows, vocab, ignore_index, two_z, ome, e_over_v, row_loss, row_lse, row_z,
                                                 row_u, nullptr, nullptr, row_weight, red, nullptr);
}

template <int NCH, bool write_grad>
__global__ __launch_bounds__(1024, 4) void ce_kl_row_bf16_kernel(bf16_t* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                                 int64_t rows, int64_t vocab, int64_t ignore_index, CeKl kl,
                                                                 float* __restrict__ row_loss, float* __restrict__ row_lse,
                                                                 const float* __restrict__ row_weight) {
    __shared__ float red[16];
    ce_row_bf16_body<NCH, CE_KL, write_grad>(logits, ld, labels, rows, vocab, ignore_index, 0.f, 1.f, 0.f, row_loss, row_lse, nullptr, nullptr,
                                             nullptr, nullptr, row_weight, red, nullptr, kl);
}

template <int NCH>
__global__ __launch_bounds__(1024, 4) void ce_row_bf16_metrics_kernel(const bf16_t* __restrict__ logits, int64_t ld,
                                                                      const int64_t* __restrict__ labels, int64_t rows, int64_t vocab,
                                                                      int64_t ignore_index, float* __restrict__ row_loss,
                                                                      float* __restrict__ row_lse, float* __restrict__ row_nll,
                                                                      int32_t* __restrict__ row_rank, const float* __restrict__ row_weight) {
    __shared__ float red[16];
    __shared__ int redi[16];
    ce_row_bf16_body<NCH, CE_METRICS, false>(const_cast<bf16_t*>(logits), ld, labels, rows, vocab, ignore_index, 0.f, 1.f, 0.f, row_loss, row_lse,
                                             nullptr, nullptr, row_nll, row_rank, row_weight, red, redi);
}

// ---- host side: which form an input takes, and the chunk counts the row form is instantiated for --------------------------------------
static int ce_num_cus() {
    static const int n = [] {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        return cus;
    }();  // thread-safe one-time initialisation (C++11 magic static)
    return n;
}

// the one predicate of the five entries: the same inputs take the same form in each
static bool ce_row_form(int dtype, const void* logits, int64_t ld, int64_t vocab) {
    const int64_t chunks = ssi_cdiv(ld, 8192);
    return dtype == SSI_BF16 && ((uintptr_t)logits & 15) == 0 && ld - vocab < 8192 && ld * 2 < (1LL << 31) &&
           (chunks <= 4 || chunks == 8 || (chunks >= 16 && chunks <= 18));
}
static dim3 ce_row_grid(int64_t rows) { return dim3((unsigned)(rows < ce_num_cus() ? rows : ce_num_cus())); }

// runs the statement(s) with N = ceil(ld / 8192) as a constant, for the chunk counts ce_row_form admits (as SSI_DISPATCH_DTYPE does with T)
#define SSI_CE_CHUNKS_CASE(n, ...) case n: { constexpr int N = n; __VA_ARGS__; } break;
#define SSI_CE_DISPATCH_CHUNKS(ld, ...)                                                                                                 \
    switch ((int)ssi_cdiv(ld, 8192)) {                                                                                                  \
        SSI_CE_CHUNKS_CASE(1, __VA_ARGS__) SSI_CE_CHUNKS_CASE(2, __VA_ARGS__) SSI_CE_CHUNKS_CASE(3, __VA_ARGS__)                        \
        SSI_CE_CHUNKS_CASE(4, __VA_ARGS__) SSI_CE_CHUNKS_CASE(8, __VA_ARGS__) SSI_CE_CHUNKS_CASE(16, __VA_ARGS__)                       \
        SSI_CE_CHUNKS_CASE(17, __VA_ARGS__) SSI_CE_CHUNKS_CASE(18, __VA_ARGS__)                                                         \
    }

// what a launch needs, whatever the entry: the entries' common arguments first, then what only some of them have
struct CeArgs {
    void* logits; int64_t ld; const int64_t* labels; const float* row_weight; int64_t rows, vocab, ignore_index;
    float *row_loss, *row_lse; int write_grad, dtype; hipStream_t stream;
    float two_z = 0.f, ome = 1.f, e_over_v = 0.f;  // CE_Z, CE_SMOOTH: 2 z;  CE_SMOOTH: 1 - e, e / vocab
    float *row_z = nullptr, *row_u = nullptr;      // CE_Z, CE_SMOOTH;  CE_SMOOTH
    float* row_nll = nullptr; int32_t* row_rank = nullptr;  // CE_METRICS
    CeKl kl;                                                // CE_KL
};

// the row kernel of MODE with its own parameter list
template <CeMode MODE, int NCH, bool write_grad> static void ce_launch_row(const CeArgs& a) {
    const dim3 grid = ce_row_grid(a.rows), block(1024);
    bf16_t* logits = (bf16_t*)a.logits;
    if constexpr (MODE == CE_PLAIN)
        hipLaunchKernelGGL((ce_row_bf16_kernel<NCH, write_grad>), grid, block, 0, a.stream, logits, a.ld, a.labels, a.rows, a.vocab, a.ignore_index,
                           a.row_loss, a.row_lse, a.row_weight);
    else if constexpr (MODE == CE_Z)
        hipLaunchKernelGGL((ce_row_bf16_z_kernel<NCH, write_grad>), grid, block, 0, a.stream, logits, a.ld, a.labels, a.rows, a.vocab, a.ignore_index,
                           a.two_z, a.row_loss, a.row_lse, a.row_z, a.row_weight);
    else if constexpr (MODE == CE_KL)
        hipLaunchKernelGGL((ce_kl_row_bf16_kernel<NCH, write_grad>), grid, block, 0, a.stream, logits, a.ld, a.labels, a.rows, a.vocab, a.ignore_index,
                           a.kl, a.row_loss, a.row_lse, a.row_weight);
    else if constexpr (MODE == CE_SMOOTH)
        hipLaunchKernelGGL((ce_row_bf16_smooth_kernel<NCH, write_grad>), grid, block, 0, a.stream, logits, a.ld, a.labels, a.rows, a.vocab,
                           a.ignore_index, a.two_z, a.ome, a.e_over_v, a.row_loss, a.row_lse, a.row_z, a.row_u, a.row_weight);
    else
        hipLaunchKernelGGL((ce_row_bf16_metrics_kernel<NCH>), grid, block, 0, a.stream, (const bf16_t*)logits, a.ld, a.labels, a.rows, a.vocab,
                           a.ignore_index, a.row_loss, a.row_lse, a.row_nll, a.row_rank, a.row_weight);
}

// the generic kernel of MODE, likewise
template <CeMode MODE, typename T> static void ce_launch_generic(const CeArgs& a) {
    const dim3 grid((unsigned)a.rows), block(512);
    T* logits = (T*)a.logits;
    if constexpr (MODE == CE_PLAIN)
        hipLaunchKernelGGL(ce_fwd_kernel<T>, grid, block, 0, a.stream, logits, a.ld, a.labels, a.vocab, a.ignore_index, a.row_loss, a.row_lse,
                           a.write_grad, a.row_weight);
    else if constexpr (MODE == CE_Z)
        hipLaunchKernelGGL(ce_fwd_z_kernel<T>, grid, block, 0, a.stream, logits, a.ld, a.labels, a.vocab, a.ignore_index, a.two_z, a.row_loss,
                           a.row_lse, a.row_z, a.write_grad, a.row_weight);
    else if constexpr (MODE == CE_KL)
        hipLaunchKernelGGL(ce_kl_generic_kernel<T>, grid, block, 0, a.stream, logits, a.ld, a.labels, a.vocab, a.ignore_index, a.kl, a.row_loss,
                           a.row_lse, a.write_grad, a.row_weight);
    else if constexpr (MODE == CE_SMOOTH)
        hipLaunchKernelGGL(ce_fwd_smooth_kernel<T>, grid, block, 0, a.stream, logits, a.ld, a.labels, a.vocab, a.ignore_index, a.two_z, a.ome,
                           a.e_over_v, a.row_loss, a.row_lse, a.row_z, a.row_u, a.write_grad, a.row_weight);
    else
        hipLaunchKernelGGL(ce_fwd_metrics_kernel<T>, grid, block, 0, a.stream, (const T*)logits, a.ld, a.labels, a.vocab, a.ignore_index, a.row_loss,
                           a.row_lse, a.row_nll, a.row_rank, a.row_weight);
}

// what the five entries share: the common argument check, the form the input takes, the launch
template <CeMode MODE> static int ce_fwd_launch(const CeArgs& a) {
    SSI_CHECK_ARG(a.logits && a.labels && a.row_loss && a.rows >= 0 && a.vocab > 0 && a.ld >= a.vocab && a.ld % 8 == 0);
    // both forms read and write the rows 16 bytes at a time (the generic form too: load16 / store16): a base that is not 16-byte aligned is
    // refused here, before anything is launched.  With ld % 8 == 0 every row of an aligned base is aligned.
    SSI_CHECK_ARG(((uintptr_t)a.logits & 15) == 0);
    if constexpr (MODE == CE_KL) SSI_CHECK_ARG(((uintptr_t)a.kl.teacher & 15) == 0);
    if (a.rows == 0) return SSI_OK;
    bool row_form = ce_row_form(a.dtype, a.logits, a.ld, a.vocab);
    // CE_KL: the row form reads the teacher with the student's addressing; any other pair of buffers takes the generic form
    if constexpr (MODE == CE_KL) row_form = row_form && a.kl.ld_teacher == a.ld && ce_row_form(a.dtype, a.kl.teacher, a.kl.ld_teacher, a.vocab);
    if (row_form) {
        SSI_CE_DISPATCH_CHUNKS(a.ld,
            if (a.write_grad) ce_launch_row<MODE, N, true>(a);  // (never so for CE_METRICS, whose one kernel ignores the flag)
            else ce_launch_row<MODE, N, false>(a));
    } else {
        SSI_DISPATCH_DTYPE(a.dtype, ce_launch_generic<MODE, T>(a));
    }
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

static bool ce_z_coeff_ok(float z) { return z >= 0.f && z <= 3.0e38f; }  // NaN fails the first test, +inf the second

extern "C" int ssi_ce_fwd_weighted(void* logits, int64_t ld, const int64_t* labels, const float* row_weight, int64_t rows, int64_t vocab,
                                   int64_t ignore_index, float* row_loss, float* row_lse, int write_grad, int dtype, void* stream) {
    return ce_fwd_launch<CE_PLAIN>(CeArgs{logits, ld, labels, row_weight, rows, vocab, ignore_index, row_loss, row_lse, write_grad, dtype, (hipStream_t)stream});
}

extern "C" int ssi_ce_fwd(void* logits, int64_t ld, const int64_t* labels, int64_t rows, int64_t vocab,
                          int64_t ignore_index, float* row_loss, float* row_lse, int write_grad, int dtype, void* stream) {
    return ssi_ce_fwd_weighted(logits, ld, labels, nullptr, rows, vocab, ignore_index, row_loss, row_lse, write_grad, dtype, stream);
}

extern "C" int ssi_ce_fwd_z(void* logits, int64_t ld, const int64_t* labels, const float* row_weight, int64_t rows, int64_t vocab,
                            int64_t ignore_index, float z_coeff, float* row_loss, float* row_lse, float* row_z, int write_grad, int dtype,
                            void* stream) {
    SSI_CHECK_ARG(row_z);
    if (!ce_z_coeff_ok(z_coeff)) {
        ssi_set_error("ce_fwd_z: z_coeff must be finite and >= 0, got %g", (double)z_coeff);
        return SSI_ERR_ARG;
    }
    CeArgs a{logits, ld, labels, row_weight, rows, vocab, ignore_index, row_loss, row_lse, write_grad, dtype, (hipStream_t)stream};
    a.two_z = 2.f * z_coeff;
    a.row_z = row_z;
    return ce_fwd_launch<CE_Z>(a);
}

extern "C" int ssi_ce_fwd_smooth(void* logits, int64_t ld, const int64_t* labels, const float* row_weight, int64_t rows, int64_t vocab,
                                 int64_t ignore_index, float smoothing, float z_coeff, float* row_loss, float* row_lse, float* row_u,
                                 float* row_z, int write_grad, int dtype, void* stream) {
    SSI_CHECK_ARG(row_u);
    if (!(smoothing >= 0.f) || !(smoothing < 1.f)) {  // NaN fails the first test
        ssi_set_error("ce_fwd_smooth: smoothing must be finite and in [0, 1), got %g", (double)smoothing);
        return SSI_ERR_ARG;
    }
    if (!ce_z_coeff_ok(z_coeff)) {
        ssi_set_error("ce_fwd_smooth: z_coeff must be finite and >= 0, got %g", (double)z_coeff);
        return SSI_ERR_ARG;
    }
    SSI_CHECK_ARG(row_z || z_coeff == 0.f);
    CeArgs a{logits, ld, labels, row_weight, rows, vocab, ignore_index, row_loss, row_lse, write_grad, dtype, (hipStream_t)stream};
    a.two_z = 2.f * z_coeff;
    a.ome = 1.f - smoothing, a.e_over_v = smoothing / (float)vocab;  // fp32, in this order: the kernels form w * ome and w * e_over_v
    a.row_z = row_z, a.row_u = row_u;
    return ce_fwd_launch<CE_SMOOTH>(a);
}

extern "C" int ssi_ce_fwd_kl(void* logits, int64_t ld, const void* teacher, int64_t ld_teacher, const float* teacher_lse, const int64_t* labels,
                             const float* row_weight, const float* row_kl_weight, int64_t rows, int64_t vocab, int64_t ignore_index,
                             float kl_coeff, float* row_loss, float* row_lse, float* row_kl, int write_grad, int dtype, void* stream) {
    SSI_CHECK_ARG(teacher && teacher_lse && row_kl && teacher != logits && ld_teacher >= vocab && ld_teacher % 8 == 0);
    if (!ce_z_coeff_ok(kl_coeff)) {
        ssi_set_error("ce_fwd_kl: kl_coeff must be finite and >= 0, got %g", (double)kl_coeff);
        return SSI_ERR_ARG;
    }
    CeArgs a{logits, ld, labels, row_weight, rows, vocab, ignore_index, row_loss, row_lse, write_grad, dtype, (hipStream_t)stream};
    a.kl = CeKl{teacher, ld_teacher, teacher_lse, row_kl_weight, kl_coeff, row_kl};
    return ce_fwd_launch<CE_KL>(a);
}

extern "C" int ssi_ce_fwd_metrics(const void* logits, int64_t ld, const int64_t* labels, const float* row_weight, int64_t rows, int64_t vocab,
                                  int64_t ignore_index, float* row_loss, float* row_lse, float* row_nll, int32_t* row_rank, int dtype,
                                  void* stream) {
    SSI_CHECK_ARG(row_nll && row_rank);
    // the metrics kernels take the logits as const again: this form writes no gradient
    CeArgs a{const_cast<void*>(logits), ld, labels, row_weight, rows, vocab, ignore_index, row_loss, row_lse, 0, dtype, (hipStream_t)stream};
    a.row_nll = row_nll, a.row_rank = row_rank;
    return ce_fwd_launch<CE_METRICS>(a);
}

// The valid-label count uses the predicate of the row kernels; labels that are neither ignored nor in range are counted in out[3] so that
// the caller can raise on its next host read-back (torch would device-assert).
__global__ __launch_bounds__(1024) void ce_reduce_kernel(const float* __restrict__ row_loss, const int64_t* __restrict__ labels,
                                                         int64_t rows, int64_t vocab, int64_t ignore_index, float* __restrict__ out) {
    __shared__ float red[16];
    float s = 0.f, c = 0.f, bad = 0.f;
    for (int64_t r = threadIdx.x; r < rows; r += 1024) {
        const int64_t l = labels[r];
        if (ce_label_valid(l, vocab, ignore_index)) { s += row_loss[r]; c += 1.f; }
        else if (l != ignore_index) bad += 1.f;
    }
    s = block_sum(s, red);
    c = block_sum(c, red);
    bad = block_sum(bad, red);
    if (threadIdx.x == 0) { out[0] = s / c; out[1] = s; out[2] = c; out[3] = bad; }
}

extern "C" int ssi_ce_reduce(const float* row_loss, const int64_t* labels, int64_t rows, int64_t vocab, int64_t ignore_index,
                             float* out, void* stream) {
    SSI_CHECK_ARG(row_loss && labels && out && rows >= 0 && rows < (1LL << 24) && vocab > 0);
    hipLaunchKernelGGL(ce_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, row_loss, labels, rows, vocab, ignore_index, out);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

// =====================================================================================================================
// K9m the reductions over the rows ssi_ce_fwd_metrics wrote
// =====================================================================================================================
// The two reductions below sum the same four numbers over ranked rows (rank >= 0: the rows ssi_ce_fwd_metrics gave a valid label), in fp64;
// the counts ride as doubles (exact below 2^53).
__device__ __forceinline__ void ce_metrics_add(double (&acc)[4], int rank, float nll, int topk) {
    acc[0] += 1.0;
    acc[1] += (double)nll;
    acc[2] += rank == 0 ? 1.0 : 0.0;
    acc[3] += rank < topk ? 1.0 : 0.0;
}

// Per-type sums of the rows ssi_ce_fwd_metrics wrote.  One workgroup; output row j (a range, or j == n_ranges: every valid label) is one
// walk over the rows in thread-strided order and one fixed tree over the lanes and the 16 waves, in fp64: bitwise reproducible, no atomics.
#define SSI_CE_MAX_RANGES 8  // as ssi_count_tokens
__global__ __launch_bounds__(1024) void ce_metrics_reduce_kernel(const float* __restrict__ row_nll, const int32_t* __restrict__ row_rank,
                                                                 const int64_t* __restrict__ labels, int64_t rows,
                                                                 const int64_t* __restrict__ ranges, int n_ranges, int topk, int accumulate,
                                                                 double* __restrict__ out) {
    __shared__ double red[4][16];
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    for (int j = 0; j <= n_ranges; ++j) {
        const bool all = j == n_ranges;
        const int64_t lo = all ? 0 : ranges[2 * j], hi = all ? 0 : ranges[2 * j + 1];
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t r = threadIdx.x; r < rows; r += 1024) {
            const int rank = row_rank[r];
            const int64_t l = labels[r];
            if (rank >= 0 && (all || (l >= lo && l <= hi))) ce_metrics_add(acc, rank, row_nll[r], topk);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = wave_sum_f64(acc[q]);
        __syncthreads();  // the previous j's read of red is over
        if (ln == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) red[q][wv] = acc[q];
        }
        __syncthreads();
        if (threadIdx.x < 4) {
            double t = 0.0;
            for (int i = 0; i < 16; ++i) t += red[threadIdx.x][i];
            double* dst = out + 4 * j + threadIdx.x;
            *dst = accumulate ? *dst + t : t;
        }
    }
}

extern "C" int ssi_ce_metrics_reduce(const float* row_nll, const int32_t* row_rank, const int64_t* labels, int64_t rows, const int64_t* ranges,
                                     int n_ranges, int topk, int accumulate, double* out, void* stream) {
    SSI_CHECK_ARG(out && rows >= 0 && rows < (1LL << 31) && (rows == 0 || (row_nll && row_rank && labels)) && n_ranges >= 0 &&
                  n_ranges <= SSI_CE_MAX_RANGES && (ranges || n_ranges == 0) && topk >= 1);
    hipLaunchKernelGGL(ce_metrics_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, row_nll, row_rank, labels, rows, ranges, n_ranges,
                       topk, accumulate, out);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

// Per-sequence sums of the rows ssi_ce_fwd_metrics wrote (ssi_seq_score_reduce): sequence i is the flat positions [seq_start[i], seq_end[i]),
// clamped to [0, rows].  One wave per sequence, four per workgroup: the lanes stride over consecutive positions, each lane sums in fp64 in
// position order, then one fixed xor tree over the 64 lanes.  No atomics, no LDS: a sequence's four numbers depend on its own positions
// only — not on n_seq, not on which wave or workgroup took it.
__global__ __launch_bounds__(256) void seq_score_reduce_kernel(const float* __restrict__ row_nll, const int32_t* __restrict__ row_rank,
                                                               int64_t rows, const int64_t* __restrict__ seq_start,
                                                               const int64_t* __restrict__ seq_end, int64_t n_seq, int topk,
                                                               double* __restrict__ out) {
    const int ln = threadIdx.x & 63;
    const int64_t seq = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seq >= n_seq) return;  // wave-uniform
    int64_t end = seq_end[seq], start = seq_start[seq];
    end = end < 0 ? 0 : (end > rows ? rows : end);
    start = start < 0 ? 0 : (start > end ? end : start);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t r = start + ln; r < end; r += 64) {
        const int rank = row_rank[r];
        if (rank >= 0) ce_metrics_add(acc, rank, row_nll[r], topk);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = wave_sum_f64(acc[q]);
    if (ln == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) out[4 * seq + q] = acc[q];
    }
}

extern "C" int ssi_seq_score_reduce(const float* row_nll, const int32_t* row_rank, int64_t rows, const int64_t* seq_start,
                                    const int64_t* seq_end, int64_t n_seq, int topk, double* out, void* stream) {
    SSI_CHECK_ARG(rows >= 0 && rows < (1LL << 31) && n_seq >= 0 && n_seq < (1LL << 31) && topk >= 1 && (rows == 0 || (row_nll && row_rank)) &&
                  (n_seq == 0 || (seq_start && seq_end && out)));
    if (n_seq == 0) return SSI_OK;
    hipLaunchKernelGGL(seq_score_reduce_kernel, dim3((unsigned)ssi_cdiv(n_seq, 4)), dim3(256), 0, (hipStream_t)stream, row_nll, row_rank, rows,
                       seq_start, seq_end, n_seq, topk, out);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}
