// bf16 MFMA GEMM, shared by the 8-wave kernel (gemm_wg8.h) and the persistent kernel (gemm_nt4.h): tile constants, LDS swizzle and
// fragment reads, the tile order, the epilogue arguments and the epilogue steps that both kernels and both split-K reduction passes
// perform.  Included by gemm_mfma.hip only (one translation unit, kernels in a fixed order).
#pragma once
#include "common_hip.h"
#include <type_traits>

namespace {

constexpr int BM = 256, BN = 256, BK = 64;
constexpr int TILE_BYTES = BM * BK * 2;                      // 32 KiB per operand tile
constexpr int PIPE_BYTES = 2 * 2 * TILE_BYTES;               // 128 KiB

// one GEMM call as the host side passes it along: tile counts, operands as ssi_gemm takes them, stream
struct GemmCall {
    int tm, tn;  // M / BM, N / BN
    int64_t K;
    const void* A;
    int64_t lda;
    const void* B;
    int64_t ldb;
    void* C;
    int64_t ldc;
    const void* R;
    float alpha;
    const float* alpha_dev;
    int accumulate;
    hipStream_t stream;
};

// Operand forms (all three layouts of ssi_gemm use the same main loop):
//   ROW  tile [rows][64 k]  (k contiguous in memory): fragments by ds_read_b128, 16-B chunk c of row r stored at
//        chunk c ^ ((r >> 1) & 7)  -> conflict-free for the 16-lane ds_read_b128 groups.
//   COL  tile [64 k][cols]  (k strided in memory: NN's B, TN's A and B): fragments by 2 x ds_read_b64_tr_b16 (the
//        hardware transpose read), 16-B chunk c of k-row r stored at chunk c ^ (g(r) << 1),
//        g(r) = (r & 3) | (((r >> 3) & 1) << 2)  -> the 8 k-rows one half-wave touches land on 8 distinct 32-B slots.
__device__ __forceinline__ int col_swz(int krow) { return ((krow & 3) | (((krow >> 3) & 1) << 2)) << 1; }

// ---- LDS -> MFMA fragment --------------------------------------------------------------------------------------------
// fragment of 16 "outer" indices (rows of A / columns of B) x 32 k: lane l holds outer = base + (l & 15), k = kh*32 + 8*(l>>4) + j
template <bool COL>
__device__ __forceinline__ bf16x8 read_frag(const char* lds_tile, int outer_base, int kh, int lane) {
    if (!COL) {
        const int row = outer_base + (lane & 15);
        const int chunk = (kh * 4 + (lane >> 4)) ^ ((row >> 1) & 7);
        return *reinterpret_cast<const bf16x8*>(lds_tile + row * 128 + chunk * 16);
    } else {
        // two transposed reads of 4 k-rows x 16 columns each; in a 16-lane group lane 4q+p addresses k-row q, cols 4p..4p+3
        const int i = lane & 15, q = i >> 2, p = i & 3;
        const int kbase = kh * 32 + 8 * (lane >> 4);
        const int chunk = (outer_base >> 3) + (p >> 1);
        const int k0 = kbase + q, k1 = kbase + 4 + q;
        const char* a0 = lds_tile + k0 * 512 + ((chunk ^ col_swz(k0)) * 16) + 8 * (p & 1);
        const char* a1 = lds_tile + k1 * 512 + ((chunk ^ col_swz(k1)) * 16) + 8 * (p & 1);
        s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a0);
        s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a1);
        typedef __attribute__((ext_vector_type(8))) short s16x8;
        s16x8 r = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        return __builtin_bit_cast(bf16x8, r);
    }
}

// ---- tile order --------------------------------------------------------------------------------------------------------
// grouped order of the tile sequence: GM m-tiles x all n-tiles per group
__device__ __forceinline__ void tile_from_t(int t, int tiles_m, int tiles_n, int& tm, int& tn) {
    constexpr int GM = 4;
    const int per_group = GM * tiles_n;
    const int group = t / per_group, in_group = t % per_group;
    const int gm = (tiles_m - group * GM) < GM ? (tiles_m - group * GM) : GM;
    tm = group * GM + in_group % gm;
    tn = in_group / gm;
}

__device__ __forceinline__ void tile_coords(int bid, int tiles_m, int tiles_n, int& tm, int& tn) {
    // XCD-aware remap (bijective for any grid size): blocks b and b+8 share an XCD, give each XCD a contiguous span
    const int nwg = tiles_m * tiles_n;
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    const int t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    tile_from_t(t, tiles_m, tiles_n, tm, tn);
}

// ---- epilogue forms ----------------------------------------------------------------------------------------------------
// EPI: 0 plain epilogue; 1 SwiGLU forward (the 256 output columns of a tile are 128 gate + the matching 128 up columns of
// W13; writes GU = [gate | up] and ACT = silu(gate) * up); 2 SwiGLU backward (C tile = d act, never stored: reads gate/up
// from GU and writes d gate / d up into DGU).  Same rounding points as the separate swiglu kernels (bf16 GEMM result first).
enum { EPI_PLAIN = 0, EPI_SWIGLU_FWD = 1, EPI_SWIGLU_BWD = 2, EPI_ROPE = 3 };
struct EpiArgs {
    bf16_t* out2 = nullptr;        // FWD: ACT [M, I]      BWD: DGU [M, 2I]
    int64_t ld_out2 = 0;
    const bf16_t* in2 = nullptr;   // BWD: GU [M, 2I]
    int64_t ld_in2 = 0;
    int64_t inter = 0;             // I
    // EPI_ROPE (QKV projection): interleaved RoPE on output columns [0, rot_cols) (the q and k heads, 64 wide), applied to the
    // bf16-rounded GEMM result and rounded again = ssi_rope_inplace on the stored tensor
    const float* rope = nullptr;    // [table_len, 32, 2] (cos, sin)
    const int32_t* pos = nullptr;   // [M] positions, or NULL: position = row % seq
    int64_t seq = 1;
    int64_t rot_cols = 0;
    // batched form (EPI_PLAIN, no split-K): `batch` problems of one shape in one launch; tile t belongs to problem t / (tiles_m * tiles_n),
    // whose operands start bsA / bsB / bsC elements after those of the problem before (C's stride also applies to R)
    int batch = 1;
    int64_t bsA = 0, bsB = 0, bsC = 0;
};

// ---- epilogue steps, one copy each ---------------------------------------------------------------------------------------
// previous values (accumulate) or the residual are added to the ROUNDED product (F.linear then `+`: two roundings)
__device__ __forceinline__ bf16x8 add_prev8(bf16x8 x, const bf16x8 prev) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = (bf16_t)((float)x[e] + (float)prev[e]);
    return x;
}


// Lane exchange of the register epilogues (accumulator layout: lane (r = lane & 15, g = lane >> 4) owns row r, columns 4g .. 4g+3 of a
// 16 x 16 tile).  pair_swap: x, y = the lane's 4 rounded columns of two neighbouring tiles -> after the swaps lane (r, g) owns 8
// consecutive columns of ONE of them: even 16-lane groups the first tile, odd groups the second, columns (g >> 1) * 8 .. + 7 of that tile
__device__ __forceinline__ u32x4 pair_swap(const bf16x4 x, const bf16x4 y) {
    const u32x2 xu = __builtin_bit_cast(u32x2, x), yu = __builtin_bit_cast(u32x2, y);
    const auto s0 = __builtin_amdgcn_permlane16_swap(xu[0], yu[0], false, false);
    const auto s1 = __builtin_amdgcn_permlane16_swap(xu[1], yu[1], false, false);
    u32x4 o;
    o[0] = s0[0]; o[1] = s1[0]; o[2] = s0[1]; o[3] = s1[1];
    return o;
}
// duo_rows: oa, ob = pair_swap of tiles (j0, j0+1) and (j0+2, j0+3): 64 columns = one 128-B line per row, as two 16-B vectors per lane
// arranged for FULL-LINE stores: a store whose 16-lane groups each cover 64 B of 16 different rows costs ~7x a store of
// whole 128-B lines (measured), so lanes 8..15 of every group trade rows with lanes 0..7 (two DPP row shifts):
//   lo: rows 0..7  — lanes r < 8 keep (row r, columns 0..31),  lanes r >= 8 take (row r-8, columns 32..63)
//   hi: rows 8..15 — lanes r < 8 take (row r+8, columns 0..31), lanes r >= 8 keep (row r, columns 32..63)
__device__ __forceinline__ void duo_rows(const u32x4 oa, const u32x4 ob, u32x4& lo, u32x4& hi) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        lo[d] = (unsigned)__builtin_amdgcn_update_dpp((int)oa[d], (int)ob[d], 0x118 /* row_shr:8 */, 0xF, 0xC, false);
        hi[d] = (unsigned)__builtin_amdgcn_update_dpp((int)ob[d], (int)oa[d], 0x108 /* row_shl:8 */, 0xF, 0x3, false);
    }
}

// ACT = silu(gate).to(bf16) * up on 8 elements (same rounding points as ssi_swiglu_fwd)
__device__ __forceinline__ bf16x8 swiglu_fwd8(const bf16x8 gv, const bf16x8 uv) {
    bf16x8 av;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float gf = (float)gv[e];
        const float sl = (float)(bf16_t)ssi_silu<bf16_t>(gf);
        av[e] = (bf16_t)(sl * (float)uv[e]);
    }
    return av;
}

// d gate = d act * up * silu'(gate), d up = d act * silu(gate) on 8 elements (same formulas as ssi_swiglu_bwd)
__device__ __forceinline__ void swiglu_bwd8(const bf16x8 gv, const bf16x8 uv, const bf16x8 dv, bf16x8& og, bf16x8& ou) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float dg, du;
        ssi_swiglu_bwd_elem<bf16_t>((float)gv[e], (float)uv[e], (float)dv[e], dg, du);
        ou[e] = (bf16_t)du;
        og[e] = (bf16_t)dg;
    }
}

}  // namespace
