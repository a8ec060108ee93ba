// What the skinny GEMMs share whatever their weight matrix is stored as (gemm_skinny.hip: bf16 rows; gemm_wq8.hip: e4m3 codes and one exponent byte
// per row): the epilogue names, the argument record, a lane's weight rows, the activation load, the LDS merge with the three epilogues
// (skinny_finish), the launch by m-tile count and the host side of the entries.  The design notes are gemm_skinny.hip's header.  A translation unit
// adds its kernel <MT, NT, WAVES, EPI> over the record — where a lane's 16 k of a weight row come from, and how many chunks the K loop keeps in
// flight — and names it to the host frame in a SOURCE struct: Args (the record its kernel takes), ok(weights, K) (pointers, pitch and alignment of
// the weight matrix) and launch<MT, NT, WAVES, EPI>(args, grid, stream).
// Every rounding point, the RoPE clamp, the merge order and every refusal are written here once: on equal accumulators the two kernels store the same
// bits by construction.  Three short steps of the kernels are written out in both all the same: the activation row pointers (arow, alive), the zeroing
// of the accumulators and the MFMA order h, i, t.  As functions of this file, in every form tried (taking values, the record or the arrays; inlined by
// force or not; called directly or from a closure), each gave some forms another K loop or other registers (wq8_gemm_kernel: the row pointers all
// twelve, the MFMAs two; skinny_kernel: the zeroing all twelve, the MFMAs called directly six), and the loops that were measured are kept
// (tools/kernel_lint.py --against tells).  Those lines are what tests/test_gemm_wq8_gpu.py still holds together.
#pragma once
#include "common_hip.h"

namespace {

enum { SK_PLAIN = 0, SK_ROPE = 1, SK_SWIGLU = 2 };
constexpr int SK_NT_WIDE_FROM = 8192;   // N from which a workgroup takes 4 n-tiles and 4 waves
struct SkinnyBf16 { const bf16_t* W; int64_t ldw; };                                  // rows of K bf16
struct SkinnyFp8 { const uint8_t* codes; int64_t ld_codes; const uint8_t* exps; };    // rows of K e4m3 codes, one exponent byte per row

template <class WEIGHTS>
struct SkinnyRecord {
    int M;
    int64_t N, K;              // SwiGLU: N = I (the width of ACT)
    const bf16_t* A; int64_t lda;
    WEIGHTS w;
    bf16_t* C; int64_t ldc;    // SwiGLU: GU (may be NULL), ldgu
    const bf16_t* R;           // plain: residual at ldc, or NULL
    bf16_t* act; int64_t ldact;
    const float* rope; int table_len; const int32_t* pos; int64_t rot_cols;
};
struct SkinnyArgs : SkinnyRecord<SkinnyBf16> {};   // (types of their own, not aliases: a kernel's symbol carries the name of its argument type)
struct Wq8Args : SkinnyRecord<SkinnyFp8> {};

// ---- device: a lane is row r16 = lane & 15 of its operand fragments and k group g = lane >> 4 of a chunk
// the weight row of this lane in n-tile t of its workgroup (SwiGLU: the first NT / 2 tiles are gate rows, the others the matching up rows, N = I below)
template <int NT, int EPI, class WEIGHTS>
__device__ __forceinline__ int64_t skinny_weight_row(const SkinnyRecord<WEIGHTS>& a, int t) {
    const int lane = threadIdx.x & 63, r16 = lane & 15;
    if (EPI == SK_SWIGLU) return (t >= NT / 2 ? a.N : 0) + (int64_t)blockIdx.x * (8 * NT) + (t % (NT / 2 > 0 ? NT / 2 : 1)) * 16 + r16;
    return ((int64_t)blockIdx.x * NT + t) * 16 + r16;
}

// the activation half of a chunk's load: the lane's 16 k at k0 of its row arow[i] of every m-tile, zeros where the row is not alive (>= M)
template <int MT>
__device__ __forceinline__ void skinny_load_act(const bf16_t* const (&arow)[MT], const bool (&alive)[MT], int64_t k0, bf16x8 (&x)[MT][2]) {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        x[i][0] = x[i][1] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (alive[i]) {
            x[i][0] = *reinterpret_cast<const bf16x8*>(arow[i] + k0);
            x[i][1] = *reinterpret_cast<const bf16x8*>(arow[i] + k0 + 8);
        }
    }
}

// After the K loop: the partial accumulators of the workgroup's waves meet in LDS in a fixed order, then every tile is finished by one wave with the
// rounding points and stores of epilogue EPI.  Called by every thread of the workgroup.
template <int MT, int NT, int WAVES, int EPI, class WEIGHTS>
__device__ __forceinline__ void skinny_finish(const SkinnyRecord<WEIGHTS>& a, f32x4 (&acc)[MT][NT]) {
    constexpr int T = MT * NT;
    __shared__ f32x4 part[4][T][64];   // 8 waves: the upper four fold into the lower four first
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;

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

// ---- host
// the m-tile count is M's alone: NT, WAVES and with them the summation order never depend on it
template <class SOURCE, int NT, int WAVES, int EPI>
int skinny_launch(const typename SOURCE::Args& a, unsigned grid, void* stream) {
    if (a.M <= 16) SOURCE::template launch<1, NT, WAVES, EPI>(a, grid, (hipStream_t)stream);
    else if (a.M <= 32) SOURCE::template launch<2, NT, WAVES, EPI>(a, grid, (hipStream_t)stream);
    else SOURCE::template launch<4, NT, WAVES, EPI>(a, grid, (hipStream_t)stream);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

bool aligned16(const void* p, int64_t ld) { return ((uintptr_t)p & 15) == 0 && ld % 8 == 0; }

// what every entry refuses alike, under the entry's own name; 0 = go on
int skinny_common(const char* what, int64_t M, int64_t N, int64_t K, int dtype) {
    if (dtype != SSI_BF16 || M < 0 || M > SSI_GEMM_SKINNY_MAX_ROWS || N <= 0 || K <= 0 || N % 64 || K % 64) {
        ssi_set_error("%s: bf16, 1 <= M <= %d, N %% 64 == 0 and K %% 64 == 0 only (M=%lld N=%lld K=%lld dtype=%d)", what, SSI_GEMM_SKINNY_MAX_ROWS,
                      (long long)M, (long long)N, (long long)K, dtype);
        return SSI_ERR_UNSUPPORTED;
    }
    return SSI_OK;
}

// the part of the record that every epilogue fills (SwiGLU: N = I, C = GU)
template <class SOURCE, class WEIGHTS>
typename SOURCE::Args skinny_record(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const WEIGHTS& w, void* C, int64_t ldc) {
    typename SOURCE::Args a{};
    a.M = (int)M; a.N = N; a.K = K; a.A = (const bf16_t*)A; a.lda = lda; a.w = w; a.C = (bf16_t*)C; a.ldc = ldc;
    return a;
}

// The three entry bodies: the refusals in the order the entries have always made them, the record, the grid.
template <class SOURCE, class WEIGHTS>
int skinny_plain(const char* what, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const WEIGHTS& w, void* C, int64_t ldc, const void* R,
                 int dtype, void* stream) {
    if (int rc = skinny_common(what, M, N, K, dtype)) return rc;
    SSI_CHECK_ARG(A && C && lda >= K && ldc >= N && SOURCE::ok(w, K));
    SSI_CHECK_ARG(aligned16(A, lda) && aligned16(C, ldc) && aligned16(R, ldc));
    if (M == 0) return SSI_OK;
    auto a = skinny_record<SOURCE>(M, N, K, A, lda, w, C, ldc);
    a.R = (const bf16_t*)R;
    if (N >= SK_NT_WIDE_FROM) return skinny_launch<SOURCE, 4, 4, SK_PLAIN>(a, (unsigned)(N / 64), stream);
    return skinny_launch<SOURCE, 1, 8, SK_PLAIN>(a, (unsigned)(N / 16), stream);
}

template <class SOURCE, class WEIGHTS>
int skinny_rope(const char* what, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const WEIGHTS& w, void* C, int64_t ldc, int n_heads_rot,
                int head_dim, const float* rope_table, int64_t table_len, const int32_t* positions, int dtype, void* stream) {
    if (int rc = skinny_common(what, M, N, K, dtype)) return rc;
    if (head_dim != 64 || n_heads_rot < 0 || (int64_t)n_heads_rot * 64 > N) {
        ssi_set_error("%s: head_dim 64 and rotated columns within N only (head_dim=%d n_heads_rot=%d N=%lld)", what, head_dim, n_heads_rot, (long long)N);
        return SSI_ERR_UNSUPPORTED;
    }
    SSI_CHECK_ARG(A && C && rope_table && positions && table_len > 0 && table_len < (1LL << 31) && lda >= K && ldc >= N && SOURCE::ok(w, K));
    SSI_CHECK_ARG(aligned16(A, lda) && aligned16(C, ldc) && ((uintptr_t)rope_table & 7) == 0);
    if (M == 0) return SSI_OK;
    auto a = skinny_record<SOURCE>(M, N, K, A, lda, w, C, ldc);
    a.rope = rope_table; a.table_len = (int)table_len; a.pos = positions; a.rot_cols = (int64_t)n_heads_rot * 64;
    return skinny_launch<SOURCE, 1, 8, SK_ROPE>(a, (unsigned)(N / 16), stream);
}

template <class SOURCE, class WEIGHTS>
int skinny_swiglu(const char* what, int64_t M, int64_t inter, int64_t K, const void* X, int64_t ldx, const WEIGHTS& w13, void* GU, int64_t ldgu,
                  void* ACT, int64_t ldact, int dtype, void* stream) {
    if (int rc = skinny_common(what, M, inter, K, dtype)) return rc;
    SSI_CHECK_ARG(X && ACT && ldx >= K && ldact >= inter && (!GU || ldgu >= 2 * inter) && SOURCE::ok(w13, K));
    SSI_CHECK_ARG(aligned16(X, ldx) && aligned16(ACT, ldact) && (!GU || aligned16(GU, ldgu)));
    if (M == 0) return SSI_OK;
    auto a = skinny_record<SOURCE>(M, inter, K, X, ldx, w13, GU, ldgu);
    a.act = (bf16_t*)ACT; a.ldact = ldact;
    return skinny_launch<SOURCE, 4, 4, SK_SWIGLU>(a, (unsigned)(inter / 32), stream);
}

}  // namespace
