// bf16 MFMA GEMM for gfx950 (MI355X): the dense contractions of the training step — QKV / output / gate-up / down
// projections, the tied LM head, and their data- and weight-gradients.
//
// One translation unit, kernels in this order (hipcc's output for a kernel depends on what precedes it in the module):
//   gemm_mfma.h  what both kernels share: tile constants, LDS swizzle and fragment reads, tile order, EpiArgs, the epilogue steps
//   gemm_wg8.h   the 8-wave kernel (every form, any K % 64 == 0), its split-K reduction and launcher
//   gemm_nt4.h   the persistent kernel (K % 128 == 0: the step's shapes), its scheduler, epilogues, split-K reduction and launcher
// This file: the host side only — which kernel takes a call (nt4_takes, the one rule), and the entry points declared in common_hip.h.
#include "gemm_mfma.h"
#include "gemm_wg8.h"
#include "gemm_nt4.h"

namespace {

// layout -> (A_COL, B_COL) as compile-time constants: f(std::bool_constant<A_COL>, std::bool_constant<B_COL>)
template <class F>
int with_layout(int layout, F&& f) {
    switch (layout) {
        case SSI_GEMM_NT: return f(std::false_type{}, std::false_type{});
        case SSI_GEMM_NN: return f(std::false_type{}, std::true_type{});
        case SSI_GEMM_TN: return f(std::true_type{}, std::true_type{});
    }
    return SSI_ERR_ARG;
}

// buffer-load offsets are 32-bit: a tile's rows (k-contiguous) or one K-step's k-rows (k-strided) must stay within 2 GiB
bool nt4_ld_ok(int64_t lda, int64_t ldb) { return 256 * lda * 2 < (1LL << 31) && 256 * ldb * 2 < (1LL << 31); }

// THE rule: does the persistent kernel take this call?  (a_col, b_col) = operand form, epi = epilogue, splits > 0 = split-K over that
// many K-slices, inter = I of the SwiGLU forward.  Everything else goes to the 8-wave kernel, which addresses with 64-bit arithmetic.
bool nt4_takes(bool a_col, bool b_col, int epi, const GemmCall& c, int splits = 0, int64_t inter = 0) {
    if (c.K % (2 * BK) || c.K < 4 * BK) return false;           // K-steps come in pairs (two LDS buffers), two of them in the prologue
    if (ssi_get_impl() == SSI_IMPL_MFMA_WG8) return false;      // the A/B switch for the 8-wave kernel
    if (c.accumulate && c.R) return false;                      // one previous value per output element (PREV)
    if (!nt4_ld_ok(c.lda, c.ldb)) return false;
    if (epi == EPI_SWIGLU_FWD) {
        // k-contiguous operands only; the up rows of W13 lie I rows behind the gate rows and that distance rides in the loader's 32-bit
        // scalar offset too (pieceB: up to I + 96 rows, + 31 rows of lane offset)
        if (a_col || b_col || (inter + 128) * c.ldb * 2 >= (1LL << 31)) return false;
    }
    if (splits > 0 && (c.K / BK / splits < 6 || c.ldc % 8)) return false;  // every K-slice at least 6 K-steps
    return true;
}

// one operand form of ssi_gemm: the persistent kernel where it applies (PREV = accumulate / residual / plain), else the 8-wave kernel
template <bool A_COL, bool B_COL>
int gemm_form(const GemmCall& c) {
    if (!nt4_takes(A_COL, B_COL, EPI_PLAIN, c)) return launch<A_COL, B_COL, false>(c);
    if (c.accumulate) return launch_nt4<A_COL, B_COL, EPI_PLAIN, 1>(c);
    if (c.R) return launch_nt4<A_COL, B_COL, EPI_PLAIN, 2>(c);
    return launch_nt4<A_COL, B_COL, EPI_PLAIN, 0>(c);
}

}  // namespace

void ssi_gemm_mfma_set_dynamic_tiles(int on) { g_nt4_dynamic.store(on ? 1 : 0, std::memory_order_relaxed); }

bool ssi_gemm_mfma_supported(int layout, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B,
                             int64_t ldb, const void* C, int64_t ldc, const void* R) {
    if (M <= 0 || N <= 0 || K <= 0) return false;
    if (M % BM || N % BN || K % BK) return false;
    if (lda % 8 || ldb % 8 || ldc % 8) return false;
    if (((uintptr_t)A | (uintptr_t)B | (uintptr_t)C | (uintptr_t)R) & 15) return false;
    if ((M / BM) * (N / BN) > (1LL << 30)) return false;
    (void)layout;
    return true;
}

int ssi_gemm_mfma_bf16(int layout, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B,
                       int64_t ldb, void* C, int64_t ldc, const void* R, float alpha, const float* alpha_dev,
                       int accumulate, void* stream) {
    const GemmCall c{(int)(M / BM), (int)(N / BN), K, A, lda, B, ldb, C, ldc, R, alpha, alpha_dev, accumulate, (hipStream_t)stream};
    return with_layout(layout, [&](auto ac, auto bc) { return gemm_form<decltype(ac)::value, decltype(bc)::value>(c); });
}

// `batch` problems of one shape in one launch of the persistent kernel: the weight-gradient form (TN), no residual;
// false = not taken, the caller loops over ssi_gemm
bool ssi_gemm_mfma_bf16_batched(int layout, int batch, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, int64_t bsA, const void* B,
                                int64_t ldb, int64_t bsB, void* C, int64_t ldc, int64_t bsC, float alpha, const float* alpha_dev, int accumulate,
                                void* stream, int* rc) {
    const GemmCall c{(int)(M / BM), (int)(N / BN), K, A, lda, B, ldb, C, ldc, nullptr, alpha, alpha_dev, accumulate, (hipStream_t)stream};
    if (layout != SSI_GEMM_TN || !nt4_takes(true, true, EPI_PLAIN, c) || (bsA | bsB | bsC) % 8 || (M / BM) * (N / BN) * batch > (1LL << 30))
        return false;
    EpiArgs ea{};
    ea.batch = batch; ea.bsA = bsA; ea.bsB = bsB; ea.bsC = bsC;
    *rc = accumulate ? launch_nt4<true, true, EPI_PLAIN, 1, false, true>(c, ea) : launch_nt4<true, true, EPI_PLAIN, 0, false, true>(c, ea);
    return true;
}

int ssi_gemm_mfma_bf16_splitk(int layout, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B,
                              int64_t ldb, void* C, int64_t ldc, const void* R, float alpha, const float* alpha_dev,
                              int accumulate, int splits, float* slabs, void* stream) {
    const GemmCall c{(int)(M / BM), (int)(N / BN), K, A, lda, B, ldb, C, ldc, R, alpha, alpha_dev, accumulate, (hipStream_t)stream};
    return with_layout(layout, [&](auto ac, auto bc) {
        constexpr bool AC = decltype(ac)::value, BC = decltype(bc)::value;
        if (!nt4_takes(AC, BC, EPI_PLAIN, c, splits)) return launch<AC, BC, true>(c, splits, slabs);
        // on the persistent kernel: units = tile x K-slice, every slice at least 6 K-steps.  Round 1-3: the weight-gradient form only; round 4: the
        // k-contiguous (NT) and data-gradient (NN) forms too, for output grids that leave CUs idle at small batches (T = 4096: W_o, W2 forward and the
        // data gradients of the N = 2048 projections have 128 tiles) or fill the last round badly (ragged T).  A residual is added by the reduction
        // pass (not together with accumulate, like the unsplit form).
        GemmCall part = c;  // the GEMM pass stores unscaled fp32 partials
        part.R = nullptr; part.alpha = 1.f; part.alpha_dev = nullptr;
        const int rc = launch_nt4<AC, BC, EPI_PLAIN, 0, true>(part, EpiArgs{}, splits, slabs);
        if (rc) return rc;
        hipLaunchKernelGGL(nt4_splitk_reduce_kernel, dim3((unsigned)ssi_cdiv((int64_t)c.tm * c.tn * 64, 4)), dim3(256), 0, c.stream, slabs, splits,
                           c.tm, c.tn, (bf16_t*)C, ldc, (const bf16_t*)R, alpha, alpha_dev, accumulate);
        SSI_LAUNCH_CHECK();
        return (int)SSI_OK;
    });
}

// QKV projection with the RoPE rotation of the q / k heads in the epilogue (head_dim 64, rot_cols % 256 == 0); false = not taken
bool ssi_gemm_rope_mfma(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                        const float* rope, const int32_t* positions, int64_t seq, int64_t rot_cols, void* stream, int* rc) {
    const GemmCall c{(int)(M / BM), (int)(N / BN), K, A, lda, B, ldb, C, ldc, nullptr, 1.f, nullptr, 0, (hipStream_t)stream};
    if (!nt4_takes(false, false, EPI_ROPE, c) || M % BM || N % BN || rot_cols % BN || rot_cols > N || lda % 8 || ldb % 8 || ldc % 8) return false;
    if (((uintptr_t)A | (uintptr_t)B | (uintptr_t)C) & 15) return false;
    EpiArgs ea{};
    ea.rope = rope; ea.pos = positions; ea.seq = seq; ea.rot_cols = rot_cols;
    *rc = launch_nt4<false, false, EPI_ROPE, 0, false>(c, ea);
    return true;
}

// ---- fused SwiGLU entries (MFMA path only; callers fall back to ssi_gemm + ssi_swiglu_* when this returns UNSUPPORTED) ----
bool ssi_gemm_swiglu_supported(int64_t M, int64_t inter, int64_t K, const void* p0, const void* p1, const void* p2, const void* p3,
                               int64_t ld0, int64_t ld1, int64_t ld2, int64_t ld3) {
    if (M <= 0 || M % BM || inter % BN || K % BK) return false;
    if ((ld0 | ld1 | ld2 | ld3) % 8) return false;
    if (((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2 | (uintptr_t)p3) & 15) return false;
    return true;
}

int ssi_gemm_swiglu_fwd_mfma(int64_t M, int64_t inter, int64_t K, const void* X, int64_t ldx, const void* W13, int64_t ldw,
                             void* GU, int64_t ldgu, void* ACT, int64_t ldact, void* stream) {
    // output tiles: 256 rows x (128 gate + 128 up) columns -> tiles_n = 2I / 256
    const GemmCall c{(int)(M / BM), (int)(2 * inter / BN), K, X, ldx, W13, ldw, GU, ldgu, nullptr, 1.f, nullptr, 0, (hipStream_t)stream};
    const EpiArgs ea{(bf16_t*)ACT, ldact, nullptr, 0, inter};
    if (nt4_takes(false, false, EPI_SWIGLU_FWD, c, 0, inter)) return launch_nt4<false, false, EPI_SWIGLU_FWD, 0, false>(c, ea);
    return launch<false, false, false, EPI_SWIGLU_FWD>(c, 1, nullptr, ea);
}

int ssi_gemm_swiglu_bwd_mfma(int layout, int64_t M, int64_t inter, int64_t K, const void* DY, int64_t lddy, const void* W2, int64_t ldw,
                             const void* GU, int64_t ldgu, void* DGU, int64_t lddgu, void* stream) {
    // d act [M, I] = DY [M, K] * W2 (NN: W2 [K, I]) or * W2T^T (NT: transposed copy [I, K]); the tile never reaches memory
    const GemmCall c{(int)(M / BM), (int)(inter / BN), K, DY, lddy, W2, ldw, DGU, lddgu, nullptr, 1.f, nullptr, 0, (hipStream_t)stream};
    const EpiArgs ea{(bf16_t*)DGU, lddgu, (const bf16_t*)GU, ldgu, inter};
    if (layout == SSI_GEMM_NN) {
        if (nt4_takes(false, true, EPI_SWIGLU_BWD, c)) return launch_nt4<false, true, EPI_SWIGLU_BWD, 0, false>(c, ea);
        return SSI_ERR_UNSUPPORTED;
    }
    if (nt4_takes(false, false, EPI_SWIGLU_BWD, c)) return launch_nt4<false, false, EPI_SWIGLU_BWD, 0, false>(c, ea);
    return launch<false, false, false, EPI_SWIGLU_BWD>(c, 1, nullptr, ea);
}

// NN form of the fused SwiGLU backward exists only on the persistent kernel
bool ssi_gemm_swiglu_bwd_nn_supported(int64_t K, int64_t lddy, int64_t ldw) {
    GemmCall c{};
    c.K = K; c.lda = lddy; c.ldb = ldw;
    return nt4_takes(false, true, EPI_SWIGLU_BWD, c);
}
