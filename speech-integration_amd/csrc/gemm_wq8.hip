// FP8 weights for small-batch decoding (ABI v27; the header's "FP8 weights"): ssi_weight_quant_fp8 turns a bf16 matrix W[N, K] into K e4m3 codes and
// one power-of-two exponent byte per ROW (the rule and the device code of the FP8 K/V cache, q8_codes.h, a row standing where a cached line
// stands there), and the three ssi_gemm_skinny*_w8 entries are the skinny GEMMs of gemm_skinny.hip on such a matrix: half the weight bytes.
//
// The GEMM kernel is skinny_kernel with another weight load and another K loop.  The weight and activation rows of a lane, the activation load, the LDS
// merge and the epilogues are the same code (gemm_skinny.h); chunk c goes to wave c % WAVES in rising order and the MFMAs of a chunk run h, then m-tile,
// then n-tile, as there: the output is BIT-EQUAL to the plain entry's on the dequantised matrix stored as bf16.  What differs:
//   - a lane's 16 k of a chunk and weight row are 16 codes in ONE 16-byte load where skinny_kernel makes two;
//   - they become the two bf16x8 operands of the chunk's two MFMAs by v_cvt_pk_f32_fp8 (exact), v_ldexp_f32 by the row's exponent (exact) and
//     v_cvt_pk_bf16_f32 (exact: four significant bits; see the header for the rows below the bf16 normal range).  The exponent is applied AT THE
//     CONVERSION, not to the fp32 sums: the matrix cores then see the very operands the plain kernel loads, whatever the magnitudes — a factor on
//     the sums would round differently where a partial sum of unscaled codes overflows or the scaled one goes subnormal.  32 vector
//     instructions per 16 codes, beside the 16 bytes they arrive in: the kernel stays bound by the weight stream;
//   - DEPTH of a wave's chunks are in flight: chunk c + DEPTH * WAVES is requested into the registers chunk c has just left, so a lane keeps
//     DEPTH * NT 16-byte weight loads outstanding — with DEPTH = 2 the bytes per lane that skinny_kernel has in flight with one chunk (the FP8 K/V
//     cache halved the bytes in flight with the bytes and came out slower).  Every register index is a compile-time constant: no scratch.
#include "gemm_skinny.h"
#include "q8_codes.h"

namespace {

#ifndef WQ8_DEPTH
#define WQ8_DEPTH 2   // chunks of a wave in flight (1, 2 and 4 were measured: profiles/LAB_NOTES.md)
#endif

// ssi_weight_quant_fp8: one wave per row, 8 elements (16 bytes) per lane and trip.  First pass: the bits of the largest finite |x| (an xor-shuffle
// maximum over the wave); second pass (the row comes from L2): every lane writes its 8 codes at once, lane 0 the exponent byte.
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

template <int MT, int NT, int WAVES, int EPI>
__global__ __launch_bounds__(WAVES * 64) void wq8_gemm_kernel(const Wq8Args a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    // code row (at this lane's 16 k of chunk 0) and exponent of this lane's weight row in n-tile t (n < N: nothing behind exps[N - 1] is read)
    const uint8_t* wrow[NT];
    int we[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int64_t n = skinny_weight_row<NT, EPI>(a, t);
        wrow[t] = a.w.codes + n * a.w.ld_codes + 16 * g;
        we[t] = (int)a.w.exps[n] - 127;
    }
    const bf16_t* arow[MT];   // (these two, the zeroing and the MFMA order are skinny_kernel's lines: see gemm_skinny.h for why they are not its functions)
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
        skinny_load_act(arow, alive, k0, x);
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
    skinny_finish<MT, NT, WAVES, EPI>(a, acc);
}

// a code matrix as the entries take it: rows of K codes on 16-byte boundaries
bool codes_ok(const void* codes, int64_t ld_codes, const void* exps, int64_t K) {
    return codes && exps && ld_codes >= K && ((uintptr_t)codes & 15) == 0 && ld_codes % 16 == 0;
}

struct Fp8Source {   // (gemm_skinny.h: what the host frame asks of a weight source)
    using Args = Wq8Args;
    static bool ok(const SkinnyFp8& w, int64_t K) { return codes_ok(w.codes, w.ld_codes, w.exps, K); }
    template <int MT, int NT, int WAVES, int EPI> static void launch(const Args& a, unsigned grid, hipStream_t stream) {
        hipLaunchKernelGGL((wq8_gemm_kernel<MT, NT, WAVES, EPI>), dim3(grid), dim3(WAVES * 64), 0, stream, a);
    }
};

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
    return skinny_plain<Fp8Source>("ssi_gemm_skinny_w8", M, N, K, A, lda, SkinnyFp8{(const uint8_t*)codes, ld_codes, (const uint8_t*)exps}, C, ldc, R,
                                   dtype, stream);
}

extern "C" int ssi_gemm_skinny_rope_w8(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* codes, int64_t ld_codes,
                                       const void* exps, void* C, int64_t ldc, int n_heads_rot, int head_dim, const float* rope_table,
                                       int64_t table_len, const int32_t* positions, int dtype, void* stream) {
    return skinny_rope<Fp8Source>("ssi_gemm_skinny_rope_w8", M, N, K, A, lda, SkinnyFp8{(const uint8_t*)codes, ld_codes, (const uint8_t*)exps}, C, ldc,
                                  n_heads_rot, head_dim, rope_table, table_len, positions, dtype, stream);
}

extern "C" int ssi_gemm_skinny_swiglu_w8(int64_t M, int64_t inter, int64_t K, const void* X, int64_t ldx, const void* codes13, int64_t ld_codes,
                                         const void* exps13, void* GU, int64_t ldgu, void* ACT, int64_t ldact, int dtype, void* stream) {
    return skinny_swiglu<Fp8Source>("ssi_gemm_skinny_swiglu_w8", M, inter, K, X, ldx, SkinnyFp8{(const uint8_t*)codes13, ld_codes, (const uint8_t*)exps13},
                                    GU, ldgu, ACT, ldact, dtype, stream);
}
