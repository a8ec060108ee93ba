// Skinny bf16 GEMM for gfx950 (MI355X): C[M, N] = A[M, K] W[N, K]^T for 1 <= M <= 64 — the projections and the tied head of a decode step
// of a few rows (one prompt, n samples, a handful of beams).  The 256-tile kernels of gemm_mfma.hip spend a whole m-tile on such a step;
// here the weight matrix is streamed once and the time is its HBM read.
//
// Lanes.  v_mfma_f32_16x16x32_bf16 takes, per lane l, 8 k-contiguous elements of row l & 15 of each operand at k = 8 (l >> 4) + j.  A
// contraction has no order across lane slots, so the k a slot stands for is free as long as both operands agree: a chunk of 64 k is given
// to the four lane groups g = l >> 4 as k = 16 g .. 16 g + 15 (two 16-byte loads per lane and row, two MFMAs: elements 0..7, then 8..15).
// The four groups of a weight row then cover one whole 128-byte line, and both operands are plain row reads: no transpose, no LDS staging.
// W is the B operand (accumulator column = lane & 15 = weight row n), A the A operand (accumulator row 4 (l >> 4) + reg = activation row).
//
// Tiles.  A workgroup owns NT n-tiles of 16 weight rows and all MT = ceil(M / 16) m-tiles; a weight fragment loaded once serves every
// m-tile and an activation fragment every n-tile.  Rows >= M of the last m-tile are never read (their fragments are zeros) and never stored.
//
// K split.  The waves of the workgroup share K: chunk c (64 k) belongs to wave c % WAVES, so neighbouring waves read neighbouring lines.
// The partial accumulators meet in LDS in a fixed order — with 8 waves, wave w + 4 is first folded into wave w, then the four sums are added
// in wave order by one thread per element: no atomics, the same bits in every launch.  NT, WAVES and with them the summation order are
// functions of N and the epilogue alone, never of M, and an output element depends on its own row of A only: row r of C has the same
// bits whatever M is and wherever r lies.  Every workgroup reads all of A from L2, so A's traffic is M / (16 NT) of W's:
//   N >= 8192: NT = 4, 4 waves  (the tied head: 2084 workgroups; A a quarter of W at M <= 16, equal at M = 64)
//   N <  8192: NT = 1, 8 waves  (N = 2048: 128 workgroups; A costs up to M / 16 of W's bytes, from L2.  A 64-row workgroup of 8 waves was
//                                measured for the down projection, N = 2048, K = 8192: 32 workgroups cannot keep enough requests in flight,
//                                41 us at one row and 67 at 64 against 13 and 40 for this form — without a split of K over workgroups, which
//                                needs a workspace the entry does not have, the workgroup count is worth more than the reuse of A)
//   SwiGLU:    NT = 4 = 2 gate tiles + the 2 matching up tiles of W13, 4 waves (I = 8192: 256 workgroups)
//
// Epilogues: the rounding points of the 256-tile kernels (gemm_mfma.h), element by element:
//   plain     bf16(sum);   with a residual  bf16(float(bf16(sum)) + R)
//   RoPE      ssi_rope_pair on the bf16-rounded pair of adjacent columns (adjacent lanes: one DPP exchange), rounded again
//   SwiGLU    gate, up = bf16(sum); ACT = bf16(float(bf16(silu(gate))) * up); GU = [gate | up] only where the caller wants it
// What a weight format does not change — the record, a lane's weight rows, the activation load, the merge and the epilogues (skinny_finish), the launch and
// the host frame — is gemm_skinny.h, shared with the FP8-weight kernel of gemm_wq8.hip; here are the bf16 weight load and the K loop.
#include "gemm_skinny.h"

namespace {

template <int MT, int NT, int WAVES, int EPI>
__global__ __launch_bounds__(WAVES * 64) void skinny_kernel(const SkinnyArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const bf16_t* wrow[NT];   // this lane's weight row of n-tile t at its 16 k of chunk 0
#pragma unroll
    for (int t = 0; t < NT; ++t) wrow[t] = a.w.W + skinny_weight_row<NT, EPI>(a, t) * a.w.ldw + 16 * g;
    const bf16_t* arow[MT];   // its activation row of m-tile i; rows at and beyond M are not alive: never read, their fragments are zeros
    bool alive[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        alive[i] = i * 16 + r16 < a.M;
        arow[i] = a.A + (int64_t)(alive[i] ? i * 16 + r16 : 0) * a.lda + 16 * g;
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto load = [&](int c, bf16x8 (&w)[NT][2], bf16x8 (&x)[MT][2]) {
        const int64_t k0 = (int64_t)c * 64;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            w[t][0] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(wrow[t] + k0));
            w[t][1] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(wrow[t] + k0 + 8));
        }
        skinny_load_act(arow, alive, k0, x);
    };
    auto multiply = [&](const bf16x8 (&w)[NT][2], const bf16x8 (&x)[MT][2]) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[i][h], w[t][h], acc[i][t], 0, 0, 0);
    };
    // a wave's chunks in rising order, one at a time (taking them four or two at a time with all loads ahead of the MFMAs was measured: no gain
    // at one row, and the 64-row forms lost a third at 64 rows to the registers it costs)
    const int chunks = (int)(a.K >> 6);
    for (int c = wave; c < chunks; c += WAVES) {
        bf16x8 w[NT][2], x[MT][2];
        load(c, w, x);
        multiply(w, x);
    }
    skinny_finish<MT, NT, WAVES, EPI>(a, acc);
}

struct Bf16Source {   // (gemm_skinny.h: what the host frame asks of a weight source)
    using Args = SkinnyArgs;
    static bool ok(const SkinnyBf16& w, int64_t K) { return w.W && w.ldw >= K && aligned16(w.W, w.ldw); }
    template <int MT, int NT, int WAVES, int EPI> static void launch(const Args& a, unsigned grid, hipStream_t stream) {
        hipLaunchKernelGGL((skinny_kernel<MT, NT, WAVES, EPI>), dim3(grid), dim3(WAVES * 64), 0, stream, a);
    }
};

}  // namespace

extern "C" int ssi_gemm_skinny(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
                               const void* R, int dtype, void* stream) {
    return skinny_plain<Bf16Source>("ssi_gemm_skinny", M, N, K, A, lda, SkinnyBf16{(const bf16_t*)W, ldw}, C, ldc, R, dtype, stream);
}

extern "C" int ssi_gemm_skinny_rope(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
                                    int n_heads_rot, int head_dim, const float* rope_table, int64_t table_len, const int32_t* positions,
                                    int dtype, void* stream) {
    return skinny_rope<Bf16Source>("ssi_gemm_skinny_rope", M, N, K, A, lda, SkinnyBf16{(const bf16_t*)W, ldw}, C, ldc, n_heads_rot, head_dim, rope_table,
                                   table_len, positions, dtype, stream);
}

extern "C" int ssi_gemm_skinny_swiglu(int64_t M, int64_t inter, int64_t K, const void* X, int64_t ldx, const void* W13, int64_t ldw, void* GU,
                                      int64_t ldgu, void* ACT, int64_t ldact, int dtype, void* stream) {
    return skinny_swiglu<Bf16Source>("ssi_gemm_skinny_swiglu", M, inter, K, X, ldx, SkinnyBf16{(const bf16_t*)W13, ldw}, GU, ldgu, ACT, ldact, dtype, stream);
}
