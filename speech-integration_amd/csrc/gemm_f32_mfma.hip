// fp32 GEMM on the fp32-input matrix instruction of gfx950 (v_mfma_f32_32x32x2_f32): exact fp32, and bit for bit what
// gemm_generic_kernel<float> returns.  The instruction computes D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)) per element: a k-ordered
// fmaf chain with one rounding per product.  This kernel keeps ONE accumulator per output element, starts it at 0 and walks
// k = 0, 1, 2, ... in ascending pairs, which is the chain of the generic kernel.  Nothing here may change that order: no split-K,
// no second accumulator for an element, no k permutation inside a tile (lane half h of k-step s reads k = 2 s + h, nothing wider).
//
// 256 threads, 128 x 128 output tile, BK = 32.  Wave w owns the 64 x 64 block (w >> 1, w & 1) as 2 x 2 accumulators of 32 x 32,
// so four independent chains cover the 64-cycle dependent latency of the instruction.  Both operands sit k-major in LDS
// ([k][row], row stride 132 floats), whatever their layout in memory: a lane's operand is one ds_read_b32, lanes 0-31 on 32
// consecutive floats of row k, lanes 32-63 on row k + 1.  The next tile is fetched into registers while the current one is
// multiplied (one LDS buffer, two barriers per tile; the other workgroups of the CU fill the gaps).  The full-tile loop is one
// basic block: its loads are clamped, not predicated (rows past M only feed outputs that are never stored), and the K tail
// (zero-filled, fma(0, 0, acc) = acc) is code of its own.
#include "common_hip.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 32, LDS_LD = 132, THREADS = 256;
constexpr int PER_THREAD = BM * BK / THREADS;  // 16 floats of each operand per thread and tile

typedef float LdsTile[BK][LDS_LD];

// One operand tile: rows [row0, row0 + 128) x k [k0, k0 + 32) of X, element (row, k) at X[row * ld + k] (KCONTIG) or
// X[k * ld + row].  VEC: 16-byte loads along the contiguous dimension (needs 16-byte aligned rows; row-contiguous operands need
// rows % 4 == 0 so that a group of four is inside or outside as a whole).  The k range must be inside the matrix; rows are clamped.
template <bool KCONTIG, bool VEC>
__device__ __forceinline__ void fetch_tile(float (&r)[PER_THREAD], const float* __restrict__ X, int64_t ld, int64_t row0, int64_t rows,
                                           int64_t k0, int tid) {
    if constexpr (VEC) {
#pragma unroll
        for (int it = 0; it < PER_THREAD / 4; ++it) {
            const int e = tid + it * THREADS;
            const float* p;
            if constexpr (KCONTIG) {
                const int64_t gr = min(row0 + (e >> 3), rows - 1);
                p = X + gr * ld + k0 + (e & 7) * 4;
            } else {
                const int64_t gr = min(row0 + (e & 31) * 4, rows - 4);
                p = X + (k0 + (e >> 5)) * ld + gr;
            }
            const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
            for (int j = 0; j < 4; ++j) r[it * 4 + j] = v[j];
        }
    } else {
#pragma unroll
        for (int it = 0; it < PER_THREAD; ++it) {
            const int e = tid + it * THREADS;
            if constexpr (KCONTIG) r[it] = X[min(row0 + (e >> 5), rows - 1) * ld + k0 + (e & 31)];
            else                   r[it] = X[(k0 + (e >> 7)) * ld + min(row0 + (e & 127), rows - 1)];
        }
    }
}

template <bool KCONTIG, bool VEC>
__device__ __forceinline__ void stash_tile(const float (&r)[PER_THREAD], LdsTile& Xs, int tid) {
    if constexpr (VEC) {
#pragma unroll
        for (int it = 0; it < PER_THREAD / 4; ++it) {
            const int e = tid + it * THREADS;
            if constexpr (KCONTIG) {
#pragma unroll
                for (int j = 0; j < 4; ++j) Xs[(e & 7) * 4 + j][e >> 3] = r[it * 4 + j];
            } else {
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = r[it * 4 + j];
                *reinterpret_cast<f32x4*>(&Xs[e >> 5][(e & 31) * 4]) = v;
            }
        }
    } else {
#pragma unroll
        for (int it = 0; it < PER_THREAD; ++it) {
            const int e = tid + it * THREADS;
            if constexpr (KCONTIG) Xs[e & 31][e >> 5] = r[it];
            else                   Xs[e >> 7][e & 127] = r[it];
        }
    }
}

// The last, partial tile: element loads, zero past K and past the last row.
template <bool KCONTIG>
__device__ __forceinline__ void tail_tile(LdsTile& Xs, const float* __restrict__ X, int64_t ld, int64_t row0, int64_t rows, int64_t k0,
                                          int64_t K, int tid) {
#pragma unroll
    for (int it = 0; it < PER_THREAD; ++it) {
        const int e = tid + it * THREADS;
        const int kk = KCONTIG ? (e & 31) : (e >> 7), rr = KCONTIG ? (e >> 5) : (e & 127);
        const int64_t gr = row0 + rr, gk = k0 + kk;
        float v = 0.f;
        if (gr < rows && gk < K) v = KCONTIG ? X[gr * ld + gk] : X[gk * ld + gr];
        Xs[kk][rr] = v;
    }
}

// 16 k-steps of the four accumulators of a wave; lane half kh supplies k = 2 s + kh of step s.  The operands of step s + 1 are
// read while step s multiplies.
__device__ __forceinline__ void mma_tile(f32x16 (&acc)[2][2], const LdsTile& As, const LdsTile& Bs, int am, int bn, int kh) {
    float a[2][2], b[2][2];
    a[0][0] = As[kh][am]; a[0][1] = As[kh][am + 32]; b[0][0] = Bs[kh][bn]; b[0][1] = Bs[kh][bn + 32];
#pragma unroll
    for (int s = 0; s < BK / 2; ++s) {
        const int c = s & 1, n = c ^ 1;
        if (s + 1 < BK / 2) {
            const int k = 2 * (s + 1) + kh;
            a[n][0] = As[k][am]; a[n][1] = As[k][am + 32]; b[n][0] = Bs[k][bn]; b[n][1] = Bs[k][bn + 32];
        }
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c][0], b[c][0], acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c][0], b[c][1], acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c][1], b[c][0], acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c][1], b[c][1], acc[1][1], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Workgroups per CU: three for the NT / NN forms with 16-byte loads (measured + 6 % / + 1.5 % over two: the third wave of a SIMD
// fills the stash-and-barrier gaps of the other two), two for TN, which lost 3 - 9 % on the weight-gradient shapes under the tighter
// register budget, and for the element-load forms.
template <int LAYOUT, bool VEC>
__global__ __launch_bounds__(THREADS, (VEC && LAYOUT != SSI_GEMM_TN) ? 3 : 2) void gemm_f32_mfma_kernel(int64_t M, int64_t N, int64_t K, const float* __restrict__ A, int64_t lda,
                                                                   const float* __restrict__ B, int64_t ldb, float* __restrict__ C,
                                                                   int64_t ldc, const float* __restrict__ R, float alpha,
                                                                   const float* __restrict__ alpha_dev, int accumulate, int tiles_m,
                                                                   int tiles_n) {
    constexpr bool A_KCONTIG = LAYOUT != SSI_GEMM_TN;  // op(A)[m][k]: NT, NN read A[m * lda + k]; TN reads A[k * lda + m]
    constexpr bool B_KCONTIG = LAYOUT == SSI_GEMM_NT;  // op(B)[k][n]: NT reads B[n * ldb + k]; NN, TN read B[k * ldb + n]
    __shared__ __attribute__((aligned(16))) LdsTile As;
    __shared__ __attribute__((aligned(16))) LdsTile Bs;

    // Workgroups go round-robin over the 8 XCDs: give each XCD a contiguous run of tile numbers (bijective for any count), and
    // walk the tiles in groups of 8 tile rows so that the workgroups an XCD runs together share operand panels in its L2.
    const int nwg = gridDim.x, orig = blockIdx.x, xcd = orig & 7, q = nwg >> 3, rem = nwg & 7;
    const int wg = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (orig >> 3);
    constexpr int GROUP = 8;
    const int per_group = GROUP * tiles_n, first_m = wg / per_group * GROUP, in_group = wg % per_group;
    const int group_m = min(tiles_m - first_m, GROUP);
    const int64_t m0 = (int64_t)(first_m + in_group % group_m) * BM, n0 = (int64_t)(in_group / group_m) * BN;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kh = lane >> 5, am = (wave >> 1) * 64 + (lane & 31), bn = (wave & 1) * 64 + (lane & 31);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int64_t full = K / BK;
    if (full > 0) {
        float ra[PER_THREAD], rb[PER_THREAD];
        fetch_tile<A_KCONTIG, VEC>(ra, A, lda, m0, M, 0, tid);
        fetch_tile<B_KCONTIG, VEC>(rb, B, ldb, n0, N, 0, tid);
        for (int64_t t = 0; t < full; ++t) {
            stash_tile<A_KCONTIG, VEC>(ra, As, tid);
            stash_tile<B_KCONTIG, VEC>(rb, Bs, tid);
            __syncthreads();
            const int64_t next = min(t + 1, full - 1) * BK;  // the last trip fetches its own tile again rather than branch
            fetch_tile<A_KCONTIG, VEC>(ra, A, lda, m0, M, next, tid);
            fetch_tile<B_KCONTIG, VEC>(rb, B, ldb, n0, N, next, tid);
            __builtin_amdgcn_sched_barrier(0);  // the loads go out before the matrix instructions, not after them
            mma_tile(acc, As, Bs, am, bn, kh);
            __syncthreads();
        }
    }
    if (full * BK < K) {
        tail_tile<A_KCONTIG>(As, A, lda, m0, M, full * BK, K, tid);
        tail_tile<B_KCONTIG>(Bs, B, ldb, n0, N, full * BK, K, tid);
        __syncthreads();
        mma_tile(acc, As, Bs, am, bn, kh);
    }

    // the epilogue of gemm_generic_kernel, expression for expression.  C/D map of the 32 x 32 forms: column = lane & 31,
    // row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
    const float al = alpha * (alpha_dev ? *alpha_dev : 1.f);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t gm = m0 + (wave >> 1) * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (gm >= M) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int64_t gn = n0 + bn + j * 32;
                float v = al * acc[i][j][r];
                if (accumulate) v += C[gm * ldc + gn];
                if (R) v += R[gm * ldc + gn];
                C[gm * ldc + gn] = v;
            }
        }
}

template <int LAYOUT>
void launch(bool vec, dim3 grid, hipStream_t stream, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B, int64_t ldb,
            float* C, int64_t ldc, const float* R, float alpha, const float* alpha_dev, int accumulate, int tiles_m, int tiles_n) {
    if (vec)
        hipLaunchKernelGGL((gemm_f32_mfma_kernel<LAYOUT, true>), grid, dim3(THREADS), 0, stream, M, N, K, A, lda, B, ldb, C, ldc, R, alpha,
                           alpha_dev, accumulate, tiles_m, tiles_n);
    else
        hipLaunchKernelGGL((gemm_f32_mfma_kernel<LAYOUT, false>), grid, dim3(THREADS), 0, stream, M, N, K, A, lda, B, ldb, C, ldc, R, alpha,
                           alpha_dev, accumulate, tiles_m, tiles_n);
}

}  // namespace

// The shapes the fp32 MFMA kernel takes: N a multiple of the tile width; M and K are arbitrary (tails are handled in the kernel).
// Operands whose rows are not 16-byte aligned run the same kernel with element loads.
bool ssi_gemm_f32_mfma_supported(int layout, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B, int64_t ldb,
                                 const void* C, int64_t ldc, const void* R) {
    if (layout != SSI_GEMM_NT && layout != SSI_GEMM_NN && layout != SSI_GEMM_TN) return false;
    if (M <= 0 || N <= 0 || K <= 0 || N % BN) return false;
    if (ssi_cdiv(M, BM) * (N / BN) > (1LL << 30)) return false;
    if (((uintptr_t)A | (uintptr_t)B | (uintptr_t)C | (uintptr_t)R) & 3) return false;
    (void)lda; (void)ldb; (void)ldc;
    return true;
}

int ssi_gemm_f32_mfma(int layout, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B, int64_t ldb, void* C,
                      int64_t ldc, const void* R, float alpha, const float* alpha_dev, int accumulate, void* stream) {
    const int tiles_m = (int)ssi_cdiv(M, BM), tiles_n = (int)(N / BN);
    const bool vec = ((((uintptr_t)A | (uintptr_t)B) & 15) == 0) && lda % 4 == 0 && ldb % 4 == 0 && (layout != SSI_GEMM_TN || M % 4 == 0);
    const dim3 grid((unsigned)(tiles_m * tiles_n));
    const float *a = (const float*)A, *b = (const float*)B, *r = (const float*)R;
    if (layout == SSI_GEMM_NT)
        launch<SSI_GEMM_NT>(vec, grid, (hipStream_t)stream, M, N, K, a, lda, b, ldb, (float*)C, ldc, r, alpha, alpha_dev, accumulate, tiles_m, tiles_n);
    else if (layout == SSI_GEMM_NN)
        launch<SSI_GEMM_NN>(vec, grid, (hipStream_t)stream, M, N, K, a, lda, b, ldb, (float*)C, ldc, r, alpha, alpha_dev, accumulate, tiles_m, tiles_n);
    else
        launch<SSI_GEMM_TN>(vec, grid, (hipStream_t)stream, M, N, K, a, lda, b, ldb, (float*)C, ldc, r, alpha, alpha_dev, accumulate, tiles_m, tiles_n);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}
