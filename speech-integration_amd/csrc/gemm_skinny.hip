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
#include "common_hip.h"

namespace {

enum { SK_PLAIN = 0, SK_ROPE = 1, SK_SWIGLU = 2 };
constexpr int SK_NT_WIDE_FROM = 8192;   // N from which a workgroup takes 4 n-tiles and 4 waves

struct SkinnyArgs {
    int M;
    int64_t N, K;              // SwiGLU: N = I (the width of ACT)
    const bf16_t* A; int64_t lda;
    const bf16_t* W; int64_t ldw;
    bf16_t* C; int64_t ldc;    // SwiGLU: GU (may be NULL), ldgu
    const bf16_t* R;           // plain: residual at ldc, or NULL
    bf16_t* act; int64_t ldact;
    const float* rope; int table_len; const int32_t* pos; int64_t rot_cols;
};

template <int MT, int NT, int WAVES, int EPI>
__global__ __launch_bounds__(WAVES * 64) void skinny_kernel(const SkinnyArgs a) {
    constexpr int T = MT * NT;
    __shared__ f32x4 part[4][T][64];   // 8 waves: the upper four fold into the lower four first
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;

    // weight row of this lane in n-tile t
    const bf16_t* wrow[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        int64_t n;
        if (EPI == SK_SWIGLU) n = (t >= NT / 2 ? a.N : 0) + (int64_t)blockIdx.x * (8 * NT) + (t % (NT / 2 > 0 ? NT / 2 : 1)) * 16 + r16;
        else n = ((int64_t)blockIdx.x * NT + t) * 16 + r16;
        wrow[t] = a.W + n * a.ldw + 16 * g;
    }
    const bf16_t* arow[MT];
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
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            x[i][0] = x[i][1] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (alive[i]) {
                x[i][0] = *reinterpret_cast<const bf16x8*>(arow[i] + k0);
                x[i][1] = *reinterpret_cast<const bf16x8*>(arow[i] + k0 + 8);
            }
        }
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

    if constexpr (WAVES == 8) {
        if (wave >= 4) {
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int t = 0; t < NT; ++t) part[wave - 4][i * NT + t][lane] = acc[i][t];
        }
        __syncthreads();
        if (wave < 4) {
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[i][t] += part[wave][i * NT + t][lane];
        }
        __syncthreads();
    }
    if (wave < 4) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int t = 0; t < NT; ++t) part[wave][i * NT + t][lane] = acc[i][t];
    }
    __syncthreads();

    // the sum of tile (i, t) in wave order; every lane of the calling wave gets its accumulator slot (column r16, rows 4 g .. 4 g + 3)
    auto total = [&](int tile) {
        f32x4 s = part[0][tile][lane];
#pragma unroll
        for (int w = 1; w < 4; ++w) s += part[w][tile][lane];
        return s;
    };

    if constexpr (EPI == SK_SWIGLU) {
        // items (i, tg): gate tile tg and up tile NT / 2 + tg of m-tile i
        constexpr int ITEMS = MT * (NT / 2);
#pragma unroll
        for (int it0 = 0; it0 < ITEMS; it0 += WAVES) {
            const int it = it0 + wave;
            if (it >= ITEMS) continue;   // (wave-uniform)
            const int i = it / (NT / 2), tg = it % (NT / 2);
            const f32x4 sg = total(i * NT + tg), su = total(i * NT + NT / 2 + tg);
            const int64_t col = (int64_t)blockIdx.x * (8 * NT) + tg * 16 + r16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = i * 16 + 4 * g + r;
                if (m >= a.M) continue;
                const bf16_t gv = (bf16_t)sg[r], uv = (bf16_t)su[r];
                const float sl = (float)(bf16_t)ssi_silu<bf16_t>((float)gv);
                a.act[m * a.ldact + col] = (bf16_t)(sl * (float)uv);
                if (a.C) {
                    a.C[m * a.ldc + col] = gv;
                    a.C[m * a.ldc + a.N + col] = uv;
                }
            }
        }
    } else {
#pragma unroll
        for (int tl0 = 0; tl0 < T; tl0 += WAVES) {
            const int tile = tl0 + wave;
            if (tile >= T) continue;     // (wave-uniform: every lane of a wave reaches the exchange below or none does)
            const int i = tile / NT, t = tile % NT;
            const f32x4 s = total(tile);
            const int64_t col = ((int64_t)blockIdx.x * NT + t) * 16 + r16;
            const bool rot = EPI == SK_ROPE && col < a.rot_cols;   // a pair (even column, odd column) lies on one side of rot_cols (a multiple of 64)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = i * 16 + 4 * g + r;
                bf16_t v = (bf16_t)s[r];
                if constexpr (EPI == SK_ROPE) {
                    // the neighbour lane's rounded value: lanes 2 p and 2 p + 1 hold the pair's x0 and x1 (every lane takes part in the exchange)
                    const float mine = (float)v;
                    const float other = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, mine), 0xB1 /* quad_perm [1,0,3,2] */, 0xF, 0xF, true));
                    if (rot && m < a.M) {
                        int p = a.pos[m];
                        p = p < 0 ? 0 : (p >= a.table_len ? a.table_len - 1 : p);
                        const f32x2 cs = *reinterpret_cast<const f32x2*>(a.rope + (int64_t)p * 64 + (col & 62));
                        float o0, o1;
                        if (lane & 1) ssi_rope_pair(other, mine, cs[0], cs[1], o0, o1);
                        else ssi_rope_pair(mine, other, cs[0], cs[1], o0, o1);
                        v = (bf16_t)((lane & 1) ? o1 : o0);
                    }
                }
                if (m >= a.M) continue;
                if (EPI == SK_PLAIN && a.R) v = (bf16_t)((float)v + (float)a.R[m * a.ldc + col]);
                a.C[m * a.ldc + col] = v;
            }
        }
    }
}

template <int NT, int WAVES, int EPI>
int skinny_launch(const SkinnyArgs& a, unsigned grid, hipStream_t stream) {
    const dim3 block(WAVES * 64);
    if (a.M <= 16) hipLaunchKernelGGL((skinny_kernel<1, NT, WAVES, EPI>), dim3(grid), block, 0, stream, a);
    else if (a.M <= 32) hipLaunchKernelGGL((skinny_kernel<2, NT, WAVES, EPI>), dim3(grid), block, 0, stream, a);
    else hipLaunchKernelGGL((skinny_kernel<4, NT, WAVES, EPI>), dim3(grid), block, 0, stream, a);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

bool aligned16(const void* p, int64_t ld) { return ((uintptr_t)p & 15) == 0 && ld % 8 == 0; }

// what the three entries refuse alike; 0 = go on
int skinny_common(const char* what, int64_t M, int64_t N, int64_t K, int dtype) {
    if (dtype != SSI_BF16 || M < 0 || M > SSI_GEMM_SKINNY_MAX_ROWS || N <= 0 || K <= 0 || N % 64 || K % 64) {
        ssi_set_error("%s: bf16, 1 <= M <= %d, N %% 64 == 0 and K %% 64 == 0 only (M=%lld N=%lld K=%lld dtype=%d)", what, SSI_GEMM_SKINNY_MAX_ROWS,
                      (long long)M, (long long)N, (long long)K, dtype);
        return SSI_ERR_UNSUPPORTED;
    }
    return SSI_OK;
}

}  // namespace

extern "C" int ssi_gemm_skinny(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
                               const void* R, int dtype, void* stream) {
    if (int rc = skinny_common("ssi_gemm_skinny", M, N, K, dtype)) return rc;
    SSI_CHECK_ARG(A && W && C && lda >= K && ldw >= K && ldc >= N);
    SSI_CHECK_ARG(aligned16(A, lda) && aligned16(W, ldw) && aligned16(C, ldc) && aligned16(R, ldc));
    if (M == 0) return SSI_OK;
    SkinnyArgs a{};
    a.M = (int)M; a.N = N; a.K = K;
    a.A = (const bf16_t*)A; a.lda = lda; a.W = (const bf16_t*)W; a.ldw = ldw; a.C = (bf16_t*)C; a.ldc = ldc; a.R = (const bf16_t*)R;
    if (N >= SK_NT_WIDE_FROM) return skinny_launch<4, 4, SK_PLAIN>(a, (unsigned)(N / 64), (hipStream_t)stream);
    return skinny_launch<1, 8, SK_PLAIN>(a, (unsigned)(N / 16), (hipStream_t)stream);
}

extern "C" int ssi_gemm_skinny_rope(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
                                    int n_heads_rot, int head_dim, const float* rope_table, int64_t table_len, const int32_t* positions,
                                    int dtype, void* stream) {
    if (int rc = skinny_common("ssi_gemm_skinny_rope", M, N, K, dtype)) return rc;
    if (head_dim != 64 || n_heads_rot < 0 || (int64_t)n_heads_rot * 64 > N) {
        ssi_set_error("ssi_gemm_skinny_rope: head_dim 64 and rotated columns within N only (head_dim=%d n_heads_rot=%d N=%lld)", head_dim, n_heads_rot,
                      (long long)N);
        return SSI_ERR_UNSUPPORTED;
    }
    SSI_CHECK_ARG(A && W && C && rope_table && positions && table_len > 0 && table_len < (1LL << 31) && lda >= K && ldw >= K && ldc >= N);
    SSI_CHECK_ARG(aligned16(A, lda) && aligned16(W, ldw) && aligned16(C, ldc) && ((uintptr_t)rope_table & 7) == 0);
    if (M == 0) return SSI_OK;
    SkinnyArgs a{};
    a.M = (int)M; a.N = N; a.K = K;
    a.A = (const bf16_t*)A; a.lda = lda; a.W = (const bf16_t*)W; a.ldw = ldw; a.C = (bf16_t*)C; a.ldc = ldc;
    a.rope = rope_table; a.table_len = (int)table_len; a.pos = positions; a.rot_cols = (int64_t)n_heads_rot * 64;
    return skinny_launch<1, 8, SK_ROPE>(a, (unsigned)(N / 16), (hipStream_t)stream);
}

extern "C" int ssi_gemm_skinny_swiglu(int64_t M, int64_t inter, int64_t K, const void* X, int64_t ldx, const void* W13, int64_t ldw, void* GU,
                                      int64_t ldgu, void* ACT, int64_t ldact, int dtype, void* stream) {
    if (int rc = skinny_common("ssi_gemm_skinny_swiglu", M, inter, K, dtype)) return rc;
    SSI_CHECK_ARG(X && W13 && ACT && ldx >= K && ldw >= K && ldact >= inter && (!GU || ldgu >= 2 * inter));
    SSI_CHECK_ARG(aligned16(X, ldx) && aligned16(W13, ldw) && aligned16(ACT, ldact) && (!GU || aligned16(GU, ldgu)));
    if (M == 0) return SSI_OK;
    SkinnyArgs a{};
    a.M = (int)M; a.N = inter; a.K = K;
    a.A = (const bf16_t*)X; a.lda = ldx; a.W = (const bf16_t*)W13; a.ldw = ldw; a.C = (bf16_t*)GU; a.ldc = ldgu; a.act = (bf16_t*)ACT; a.ldact = ldact;
    return skinny_launch<4, 4, SK_SWIGLU>(a, (unsigned)(inter / 32), (hipStream_t)stream);
}
