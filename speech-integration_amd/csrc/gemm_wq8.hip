// FP8 weights for small-batch decoding (ABI v27; the header's "FP8 weights"): ssi_weight_quant_fp8 turns a bf16 matrix W[N, K] into K e4m3 codes and
// one power-of-two exponent byte per ROW (the rule and the device code of the FP8 K/V cache, q8_codes.h, a row standing where a cached line
// stands there), and the three ssi_gemm_skinny*_w8 entries are the skinny GEMMs of gemm_skinny.hip on such a matrix: half the weight bytes.
//
// The GEMM kernel is skinny_kernel with another K loop.  Which k a lane slot stands for, which 64-wide chunk belongs to which wave (chunk c to wave
// c % WAVES, taken in rising order), the order of the MFMAs within a chunk (h, then m-tile, then n-tile), the LDS merge and the epilogues
// (wq8_finish) are that kernel's, so the output is BIT-EQUAL to the plain entry's on the dequantised matrix stored
// as bf16.  What differs:
//   - a lane's 16 k of a chunk and weight row are 16 codes in ONE 16-byte load where skinny_kernel makes two;
//   - they become the two bf16x8 operands of the chunk's two MFMAs by v_cvt_pk_f32_fp8 (exact), v_ldexp_f32 by the row's exponent (exact) and
//     v_cvt_pk_bf16_f32 (exact: four significant bits; see the header for the rows below the bf16 normal range).  The exponent is applied AT THE
//     CONVERSION, not to the fp32 sums: the matrix cores then see the very operands the plain kernel loads, whatever the magnitudes — a factor on
//     the sums would round differently where a partial sum of unscaled codes overflows or the scaled one goes subnormal.  32 vector
//     instructions per 16 codes, beside the 16 bytes they arrive in: the kernel stays bound by the weight stream;
//   - DEPTH of a wave's chunks are in flight: chunk c + DEPTH * WAVES is requested into the registers chunk c has just left, so a lane keeps
//     DEPTH * NT 16-byte weight loads outstanding — with DEPTH = 2 the bytes per lane that skinny_kernel has in flight with one chunk (the FP8 K/V
//     cache halved the bytes in flight with the bytes and came out slower).  Every register index is a compile-time constant: no scratch.
#include "common_hip.h"
#include "q8_codes.h"

namespace {

#ifndef WQ8_DEPTH
#define WQ8_DEPTH 2   // chunks of a wave in flight (1, 2 and 4 were measured: profiles/LAB_NOTES.md)
#endif

enum { SK_PLAIN = 0, SK_ROPE = 1, SK_SWIGLU = 2 };
constexpr int SK_NT_WIDE_FROM = 8192;   // N from which a workgroup takes 4 n-tiles and 4 waves

struct Wq8Args {               // gemm_skinny.hip's SkinnyArgs with (codes, ld_codes, exps) for (W, ldw)
    int M;
    int64_t N, K;              // SwiGLU: N = I (the width of ACT)
    const bf16_t* A; int64_t lda;
    const uint8_t* codes; int64_t ld_codes;
    const uint8_t* exps;
    bf16_t* C; int64_t ldc;    // SwiGLU: GU (may be NULL), ldgu
    const bf16_t* R;           // plain: residual at ldc, or NULL
    bf16_t* act; int64_t ldact;
    const float* rope; int table_len; const int32_t* pos; int64_t rot_cols;
};

// =====================================================================================================================
// ssi_weight_quant_fp8: one wave per row, 8 elements (16 bytes) per lane and trip.  First pass: the bits of the largest finite |x| (an xor-shuffle
// maximum over the wave); second pass (the row comes from L2): every lane writes its 8 codes at once, lane 0 the exponent byte.
// =====================================================================================================================
__global__ __launch_bounds__(256) void wq8_quant_kernel(const bf16_t* __restrict__ W, int64_t ldw, int64_t N, int K, uint8_t* __restrict__ codes,
                                                        int64_t ld_codes, uint8_t* __restrict__ exps) {
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;                                   // (whole waves: every shuffle below meets live lanes only)
    const bf16_t* row = W + n * ldw;
    uint32_t a = 0;
    for (int k = lane * 8; k < K; k += 512) {
        const Vec16<bf16_t> x = load16<bf16_t>(row + k);
#pragma unroll
        for (int v = 0; v < 8; ++v) a = q8_absmax_bits(a, x.get(v));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)a, o, 64);
        a = other > a ? other : a;
    }
    const int b = q8_exponent_byte(a);
    for (int k = lane * 8; k < K; k += 512) {
        const Vec16<bf16_t> x = load16<bf16_t>(row + k);
        float f[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) f[v] = x.get(v);
        u32x2 w;
        w[0] = q8_encode4(f[0], f[1], f[2], f[3], b);
        w[1] = q8_encode4(f[4], f[5], f[6], f[7], b);
        *reinterpret_cast<u32x2*>(codes + n * ld_codes + k) = w;
    }
    if (lane == 0) exps[n] = (uint8_t)b;
}

// the two MFMA operands (elements 0..7 and 8..15 of the lane's 16 k) of 16 codes under e = b - 127
__device__ __forceinline__ void wq8_operands(const u32x4 q, int e, bf16x8& lo, bf16x8& hi) {
    float f[16];
#pragma unroll
    for (int w = 0; w < 4; ++w) q8_decode4(q[w], e, f + 4 * w);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        lo[j] = (bf16_t)f[j];
        hi[j] = (bf16_t)f[8 + j];
    }
}

// skinny_kernel's merge and epilogues, statement for statement (that kernel's source stays as it is, so that its code objects do; the bit-equality
// tests hold the two copies together): the partial accumulators of the workgroup's waves meet in LDS in a fixed order, then every tile is
// finished by one wave with the rounding points and stores of epilogue EPI.  Called by every thread of the workgroup.
template <int MT, int NT, int WAVES, int EPI>
__device__ __forceinline__ void wq8_finish(const Wq8Args& a, f32x4 (&acc)[MT][NT]) {
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

template <int MT, int NT, int WAVES, int EPI>
__global__ __launch_bounds__(WAVES * 64) void wq8_gemm_kernel(const Wq8Args a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;

    // code row and exponent of this lane's weight row in n-tile t (n < N: nothing behind exps[N - 1] is read)
    const uint8_t* wrow[NT];
    int we[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        int64_t n;
        if (EPI == SK_SWIGLU) n = (t >= NT / 2 ? a.N : 0) + (int64_t)blockIdx.x * (8 * NT) + (t % (NT / 2 > 0 ? NT / 2 : 1)) * 16 + r16;
        else n = ((int64_t)blockIdx.x * NT + t) * 16 + r16;
        wrow[t] = a.codes + n * a.ld_codes + 16 * g;
        we[t] = (int)a.exps[n] - 127;
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

    auto load = [&](int c, u32x4 (&w)[NT], bf16x8 (&x)[MT][2]) {
        const int64_t k0 = (int64_t)c * 64;
#pragma unroll
        for (int t = 0; t < NT; ++t) w[t] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow[t] + k0));
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            x[i][0] = x[i][1] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (alive[i]) {
                x[i][0] = *reinterpret_cast<const bf16x8*>(arow[i] + k0);
                x[i][1] = *reinterpret_cast<const bf16x8*>(arow[i] + k0 + 8);
            }
        }
    };
    auto multiply = [&](const u32x4 (&w)[NT], const bf16x8 (&x)[MT][2]) {
        bf16x8 b[NT][2];
#pragma unroll
        for (int t = 0; t < NT; ++t) wq8_operands(w[t], we[t], b[t][0], b[t][1]);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[i][h], b[t][h], acc[i][t], 0, 0, 0);
    };
    // a wave's chunks in rising order, WQ8_DEPTH of them in flight (all conditions are wave-uniform)
    const int chunks = (int)(a.K >> 6);
    u32x4 w[WQ8_DEPTH][NT];
    bf16x8 x[WQ8_DEPTH][MT][2];
#pragma unroll
    for (int d = 0; d < WQ8_DEPTH; ++d)
        if (wave + d * WAVES < chunks) load(wave + d * WAVES, w[d], x[d]);
    for (int c = wave; c < chunks; c += WQ8_DEPTH * WAVES) {
#pragma unroll
        for (int d = 0; d < WQ8_DEPTH; ++d) {
            const int cd = c + d * WAVES;
            if (cd < chunks) {
                multiply(w[d], x[d]);
                if (cd + WQ8_DEPTH * WAVES < chunks) load(cd + WQ8_DEPTH * WAVES, w[d], x[d]);
            }
        }
    }

    wq8_finish<MT, NT, WAVES, EPI>(a, acc);
}

template <int NT, int WAVES, int EPI>
int wq8_launch(const Wq8Args& a, unsigned grid, hipStream_t stream) {
    const dim3 block(WAVES * 64);
    if (a.M <= 16) hipLaunchKernelGGL((wq8_gemm_kernel<1, NT, WAVES, EPI>), dim3(grid), block, 0, stream, a);
    else if (a.M <= 32) hipLaunchKernelGGL((wq8_gemm_kernel<2, NT, WAVES, EPI>), dim3(grid), block, 0, stream, a);
    else hipLaunchKernelGGL((wq8_gemm_kernel<4, NT, WAVES, EPI>), dim3(grid), block, 0, stream, a);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

// a code matrix as the entries take it: rows of K codes on 16-byte boundaries
bool codes_ok(const void* codes, int64_t ld_codes, const void* exps, int64_t K) {
    return codes && exps && ld_codes >= K && ((uintptr_t)codes & 15) == 0 && ld_codes % 16 == 0;
}

}  // namespace

extern "C" int ssi_weight_quant_fp8(const void* W, int64_t ldw, int64_t N, int64_t K, void* codes, int64_t ld_codes, void* exps, int dtype,
                                    void* stream) {
    if (dtype != SSI_BF16 || N < 0 || K <= 0 || K % 64 || K >= (1LL << 31)) {
        ssi_set_error("ssi_weight_quant_fp8: bf16 and K %% 64 == 0 only (N=%lld K=%lld dtype=%d)", (long long)N, (long long)K, dtype);
        return SSI_ERR_UNSUPPORTED;
    }
    SSI_CHECK_ARG(W && ldw >= K && aligned16(W, ldw) && codes_ok(codes, ld_codes, exps, K) && ssi_cdiv(N, 4) < (1LL << 31));
    if (N == 0) return SSI_OK;
    hipLaunchKernelGGL(wq8_quant_kernel, dim3((unsigned)ssi_cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)W, ldw, N, (int)K,
                       (uint8_t*)codes, ld_codes, (uint8_t*)exps);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

extern "C" int ssi_gemm_skinny_w8(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* codes, int64_t ld_codes,
                                  const void* exps, void* C, int64_t ldc, const void* R, int dtype, void* stream) {
    if (int rc = skinny_common("ssi_gemm_skinny_w8", M, N, K, dtype)) return rc;
    SSI_CHECK_ARG(A && C && lda >= K && ldc >= N && codes_ok(codes, ld_codes, exps, K));
    SSI_CHECK_ARG(aligned16(A, lda) && aligned16(C, ldc) && aligned16(R, ldc));
    if (M == 0) return SSI_OK;
    Wq8Args a{};
    a.M = (int)M; a.N = N; a.K = K;
    a.A = (const bf16_t*)A; a.lda = lda; a.C = (bf16_t*)C; a.ldc = ldc; a.R = (const bf16_t*)R;
    a.codes = (const uint8_t*)codes; a.ld_codes = ld_codes; a.exps = (const uint8_t*)exps;
    if (N >= SK_NT_WIDE_FROM) return wq8_launch<4, 4, SK_PLAIN>(a, (unsigned)(N / 64), (hipStream_t)stream);
    return wq8_launch<1, 8, SK_PLAIN>(a, (unsigned)(N / 16), (hipStream_t)stream);
}

extern "C" int ssi_gemm_skinny_rope_w8(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* codes, int64_t ld_codes,
                                       const void* exps, void* C, int64_t ldc, int n_heads_rot, int head_dim, const float* rope_table,
                                       int64_t table_len, const int32_t* positions, int dtype, void* stream) {
    if (int rc = skinny_common("ssi_gemm_skinny_rope_w8", M, N, K, dtype)) return rc;
    if (head_dim != 64 || n_heads_rot < 0 || (int64_t)n_heads_rot * 64 > N) {
        ssi_set_error("ssi_gemm_skinny_rope_w8: head_dim 64 and rotated columns within N only (head_dim=%d n_heads_rot=%d N=%lld)", head_dim,
                      n_heads_rot, (long long)N);
        return SSI_ERR_UNSUPPORTED;
    }
    SSI_CHECK_ARG(A && C && rope_table && positions && table_len > 0 && table_len < (1LL << 31) && lda >= K && ldc >= N);
    SSI_CHECK_ARG(codes_ok(codes, ld_codes, exps, K) && aligned16(A, lda) && aligned16(C, ldc) && ((uintptr_t)rope_table & 7) == 0);
    if (M == 0) return SSI_OK;
    Wq8Args a{};
    a.M = (int)M; a.N = N; a.K = K;
    a.A = (const bf16_t*)A; a.lda = lda; a.C = (bf16_t*)C; a.ldc = ldc;
    a.rope = rope_table; a.table_len = (int)table_len; a.pos = positions; a.rot_cols = (int64_t)n_heads_rot * 64;
    a.codes = (const uint8_t*)codes; a.ld_codes = ld_codes; a.exps = (const uint8_t*)exps;
    return wq8_launch<1, 8, SK_ROPE>(a, (unsigned)(N / 16), (hipStream_t)stream);
}

extern "C" int ssi_gemm_skinny_swiglu_w8(int64_t M, int64_t inter, int64_t K, const void* X, int64_t ldx, const void* codes13, int64_t ld_codes,
                                         const void* exps13, void* GU, int64_t ldgu, void* ACT, int64_t ldact, int dtype, void* stream) {
    if (int rc = skinny_common("ssi_gemm_skinny_swiglu_w8", M, inter, K, dtype)) return rc;
    SSI_CHECK_ARG(X && ACT && ldx >= K && ldact >= inter && (!GU || ldgu >= 2 * inter) && codes_ok(codes13, ld_codes, exps13, K));
    SSI_CHECK_ARG(aligned16(X, ldx) && aligned16(ACT, ldact) && (!GU || aligned16(GU, ldgu)));
    if (M == 0) return SSI_OK;
    Wq8Args a{};
    a.M = (int)M; a.N = inter; a.K = K;
    a.A = (const bf16_t*)X; a.lda = ldx; a.C = (bf16_t*)GU; a.ldc = ldgu; a.act = (bf16_t*)ACT; a.ldact = ldact;
    a.codes = (const uint8_t*)codes13; a.ld_codes = ld_codes; a.exps = (const uint8_t*)exps13;
    return wq8_launch<4, 4, SK_SWIGLU>(a, (unsigned)(inter / 32), (hipStream_t)stream);
}
