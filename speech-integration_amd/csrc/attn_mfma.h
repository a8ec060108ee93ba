// Causal GQA flash attention on the gfx950 matrix cores (bf16, head_dim 64) — forward, dQ and dK/dV.
// Replaces F.scaled_dot_product_attention(is_causal=True) inside torchtune's MultiHeadAttention and its autograd
// (SURVEY.md §2.3 K5/K10).  qkv is the fused projection output [B*S, (H + 2 KV) * 64] after RoPE.
//
// Orientation (all three kernels): scores are produced TRANSPOSED or with the reduction index on the accumulator's ROW
// axis, so that the 32x32 accumulator of one v_mfma_f32_32x32x16_bf16 is directly the B operand of the next product
// (no LDS round trip, no lane shuffles for P):
//   forward : S^T[key][q] = K Q^T      -> P^T -> O^T[d][q]  += V^T[d][key] P^T[key][q]      (row statistics per LANE)
//   dQ      : S^T, dP^T[key][q] = V dO^T -> dS^T -> dQ^T[d][q] += K^T[d][key] dS^T[key][q]
//   dK/dV   : S[q][key] = Q K^T, dP[q][key] = dO V^T -> P, dS -> dV^T[d][key] += dO^T[d][q] P[q][key],
//             dK^T[d][key] += Q^T[d][q] dS[q][key]                                          (key on the lane, sums in regs)
// k-contiguous operands come from LDS by ds_read_b128, k-strided ones by ds_read_b64_tr_b16 (hardware transpose); tiles
// are [rows][64] bf16 (128-B rows) with a 16-B-chunk XOR swizzle chosen per tile for the way it is read.
// Workgroup = 4 waves; the waves of a workgroup share one kv head (K/V tiles staged once for the 4 query heads of a GQA
// group).  No atomics anywhere: dQ gets its own pass (recomputing S and dP) so every output has exactly one writer and
// results are bitwise reproducible.
//
// This header: what the kernel files attn_fwd.h, attn_bwd_dq.h and attn_bwd_dkv.h share — operand types, tile swizzles, fragment readers, the
// LDS-DMA tile movers, the workgroup -> work map and the -DATTN_TRACE macros.  The three kernel files are the parts of ONE translation unit,
// attention_mfma.hip, which includes them in that order and holds the host side (support rule, mode switches, work plan, backward dispatcher).
// They are not compiled apart: hipcc's code for a kernel depends on what stands in front of it in the module (attn_bwd_dkv_kernel compiled
// without the forward and dQ kernels ahead of it comes out with another register allocation and five instructions fewer), and these
// kernels are held to their listings (tools/kernel_lint.py).
#pragma once
#include <type_traits>
#include "common_hip.h"

namespace {

// Backward of the interleaved RoPE on the 4 consecutive head dimensions d0 .. d0+3 of one row (two adjacent pairs), applied to
// the gradient AFTER its rounding to bf16 and rounded again, i.e. exactly what ssi_rope_inplace(inverse) does to the stored
// tensor (torchtune applies RoPE as a separate bf16 -> fp32 -> bf16 op).  tb = table row of the position: [hd/2][cos, sin].
__device__ __forceinline__ bf16x4 unrope4(bf16x4 v, f32x4 cs) {  // cs = (cos, sin) of pairs d0/2 and d0/2 + 1
    const float x0 = (float)v[0], x1 = (float)v[1], x2 = (float)v[2], x3 = (float)v[3];
    bf16x4 o;
    o[0] = (bf16_t)(x0 * cs[0] + x1 * cs[1]);
    o[1] = (bf16_t)(x1 * cs[0] - x0 * cs[1]);
    o[2] = (bf16_t)(x2 * cs[2] + x3 * cs[3]);
    o[3] = (bf16_t)(x3 * cs[2] - x2 * cs[3]);
    return o;
}
__device__ __forceinline__ bf16x4 unrope4(bf16x4 v, const float* __restrict__ tb, int d0) {
    return unrope4(v, *reinterpret_cast<const f32x4*>(tb + d0));
}

// Workgroup -> (rank of the block inside its (batch, kv head) pair, pair).  Workgroups go to the 8 XCDs round-robin by
// blockIdx, and under the causal mask a block's work is proportional to its rank, so a plain "block = blockIdx % n" map hands
// XCD x only the blocks of rank x, x + 8, ...: 2.4x the work for XCD 0 as for XCD 7 at 16 blocks per pair, and the kernel lasts
// as long as XCD 0.  Here every XCD gets whole pairs (n_pairs / 8 of them: equal work, and a pair's K / V or Q / dO stay in one
// L2) and meets their blocks in rank order — with `rank` counting from the heaviest block, longest first across its pairs.
__device__ __forceinline__ void block_to_work(int n_blocks, int n_pairs, int& rank, int& pair) {
    const int i = (int)blockIdx.x;
    if (n_pairs % 8 == 0) {
        const int ppx = n_pairs / 8, xcd = i & 7, j = i >> 3;
        rank = j / ppx;
        pair = xcd * ppx + j % ppx;
    } else {
        rank = i % n_blocks;
        pair = i / n_blocks;
    }
}

// Workgroup barrier for the LDS-DMA rings.  __syncthreads() would do, except that hipcc puts `s_waitcnt vmcnt(0)` in front of
// its s_barrier: that waits for the prefetches of the NEXT steps as well and exposes their whole memory latency every step.
// Here the counted vmcnt wait for this step's pieces is written out by the caller; only LDS traffic is drained.
__device__ __forceinline__ void ring_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// -DATTN_TRACE (debug build, tools/attn_trace.py): every workgroup leaves its start, the start and end of its tile loop and its end on the
// 100 MHz constant clock, where it ran (XCC, SE, CU) and its work (tiles / steps) in a device-side table: the occupancy timeline of a launch —
// per-workgroup cost against its tile count, idle slots, the tail.  Never part of the product build (the extra export would also fail
// tests/test_abi.py).
#ifdef ATTN_TRACE
constexpr int TRACE_MAX = 8192;
__device__ unsigned long long g_attn_trace[3][TRACE_MAX][6];
#define TRACE_BEGIN() const unsigned long long tr_t0_ = __builtin_amdgcn_s_memrealtime(); unsigned long long tr_ta_ = 0, tr_tb_ = 0
#define TRACE_LOOP_BEGIN() tr_ta_ = __builtin_amdgcn_s_memrealtime()   /* prologue issued (loads in flight), tile loop starts */
#define TRACE_LOOP_END() tr_tb_ = __builtin_amdgcn_s_memrealtime()     /* tile loop done, epilogue starts */
#define TRACE_END(k, work)                                                                                                        \
    if (threadIdx.x == 0 && blockIdx.x < TRACE_MAX) {                                                                             \
        unsigned hw_, xcc_;                                                                                                       \
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_));                                                        \
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));                                                      \
        g_attn_trace[k][blockIdx.x][0] = tr_t0_;                                                                                  \
        g_attn_trace[k][blockIdx.x][1] = __builtin_amdgcn_s_memrealtime();                                                        \
        g_attn_trace[k][blockIdx.x][2] = ((unsigned long long)xcc_ << 32) | hw_;                                                  \
        g_attn_trace[k][blockIdx.x][3] = (unsigned long long)(work);                                                              \
        g_attn_trace[k][blockIdx.x][4] = tr_ta_;                                                                                  \
        g_attn_trace[k][blockIdx.x][5] = tr_tb_;                                                                                  \
    }
#else
#define TRACE_BEGIN()
#define TRACE_LOOP_BEGIN()
#define TRACE_LOOP_END()
#define TRACE_END(k, work)
#endif

constexpr int HD = 64;
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ int rowmap(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// 16-B-chunk XOR swizzles of a [rows][64] bf16 tile (two 128-B rows per 256-B bank row):
//   SWZ_ROW  f = (row >> 1) & 7: the 8 same-parity rows of a ds_read_b128 lane group land on 8 different chunks   (row reads only)
//   SWZ_TR   f = 4 * bit 1 of row: rows r and r + 2 of a transposed 4-row block land on opposite halves of the row (transposed reads only)
//   SWZ_DUAL both at once: the three bits of (row >> 1) rotated so that bit 1 of the row becomes bit 2 of f — still 8 different values on
//            the row-read groups, and r / r + 2 differ in bit 2.  With SWZ_ROW a tile that is ALSO read transposed (K in dQ, Q and dO in
//            dK/dV) cost every ds_read_b64_tr_b16 a 2-way conflict (SQ_LDS_BANK_CONFLICT = one extra cycle per LDS instruction).
enum { SWZ_ROW = 0, SWZ_TR = 1, SWZ_DUAL = 2 };
template <int SWZ> __device__ __forceinline__ int swz(int row) {
    if (SWZ == SWZ_ROW) return (row >> 1) & 7;
    if (SWZ == SWZ_TR) return ((row >> 1) & 1) << 2;
    return (((row >> 1) & 1) << 2) | ((row >> 2) & 3);
}

// 32 rows x 16 k fragment of a [rows][64] tile: lane l holds row = row_base + (l & 31), k = 16 ks + 8 (l >> 5) + j
template <int SWZ> __device__ __forceinline__ bf16x8 frag_row(const char* tile, int row_base, int ks, int lane) {
    const int row = row_base + (lane & 31);
    const int chunk = (2 * ks + (lane >> 5)) ^ swz<SWZ>(row);
    return *reinterpret_cast<const bf16x8*>(tile + row * 128 + chunk * 16);
}

// transposed fragment: lane l holds column c = cbase + (l & 31) of tile rows kbase + {8 (j >> 2) + 4 (l >> 5) + (j & 3)}, j = 0..7
// (the k order in which a 32x32 accumulator, converted to bf16, presents itself as an MFMA operand)
template <int SWZ> __device__ __forceinline__ bf16x8 frag_tr(const char* tile, int kbase, int cbase, int lane) {
    const int G = lane >> 4, h = G >> 1, i = lane & 15, q = i >> 2, p = i & 3;
    const int chunk = ((cbase + 16 * (G & 1)) >> 3) + (p >> 1);
    const int r0 = kbase + 4 * h + q, r1 = r0 + 8;
    const char* a0 = tile + r0 * 128 + ((chunk ^ swz<SWZ>(r0)) * 16) + 8 * (p & 1);
    const char* a1 = tile + r1 * 128 + ((chunk ^ swz<SWZ>(r1)) * 16) + 8 * (p & 1);
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a0);
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a1);
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    s16x8 r = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, r);
}

// one half (4 of the 8 k rows: half 0 = rows kbase + 4 (l >> 5) + 0..3, half 1 = those + 8) of frag_tr: one ds_read_b64_tr_b16
template <int SWZ> __device__ __forceinline__ s16x4 frag_tr_half(const char* tile, int kbase, int cbase, int lane, int half) {
    const int G = lane >> 4, h = G >> 1, i = lane & 15, q = i >> 2, p = i & 3;
    const int chunk = ((cbase + 16 * (G & 1)) >> 3) + (p >> 1);
    const int r = kbase + 4 * h + q + 8 * half;
    const char* a = tile + r * 128 + ((chunk ^ swz<SWZ>(r)) * 16) + 8 * (p & 1);
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a);
}

// registers 8 s .. 8 s + 7 of a 32x32 accumulator as a bf16 operand fragment (k-step s)
__device__ __forceinline__ bf16x8 acc_frag(const f32x16& a, int s) {
    bf16x8 f;
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (bf16_t)a[8 * s + j];
    return f;
}

__device__ __forceinline__ bf16x8 scale_frag(bf16x8 v, float s) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (bf16_t)((float)v[j] * s);
    return v;
}

// stage a [ROWS][64] bf16 tile global -> registers -> LDS (swizzled), split so the loads fly under compute (T14)
template <int ROWS, int NTHR> struct TileStage {
    static constexpr int N = ROWS * 8 / NTHR;  // 16-B chunks per thread
    u32x4 r[N];
    __device__ __forceinline__ void load(const bf16_t* g, int64_t ld, int tid) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int c = tid + i * NTHR;
            r[i] = *reinterpret_cast<const u32x4*>(g + (int64_t)(c >> 3) * ld + (c & 7) * 8);
        }
    }
    template <int SWZ> __device__ __forceinline__ void store(char* tile, int tid) const {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int c = tid + i * NTHR, row = c >> 3, chunk = (c & 7) ^ swz<SWZ>(row);
            *reinterpret_cast<u32x4*>(tile + row * 128 + chunk * 16) = r[i];
        }
    }
};

// LDS-DMA requests are written as inline asm, not as __builtin_amdgcn_global_load_lds: the compiler knows that the builtin writes
// LDS and puts `s_waitcnt vmcnt(0)` in front of the next LDS read it cannot prove disjoint (every ds_read_b64_tr_b16 here), which
// waits for the prefetches of the LATER tiles as well and turns a ring of N tiles into a ring of one.  With the asm form the only
// waits are the counted ones written out next to the ring barriers.  A request = one wave-instruction: lane l's 16 (or 4) bytes at
// rsrc base + voff(l) + soff go to LDS byte M0 + 16 l (4 l); the bank swizzle of a tile image is therefore applied on the per-lane
// SOURCE offset.  The buffer form keeps the per-lane part of the address a constant 32-bit VGPR and the moving part a scalar
// (resource: buffer_rsrc in common_hip.h).
typedef __attribute__((address_space(3))) char lds_c;
__device__ __forceinline__ void dma16(unsigned lds_dst, unsigned voff, u32x4 rs, unsigned soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lds_dst), "v"(voff), "s"(rs), "s"(soff) : "memory");
}
__device__ __forceinline__ void dma4(unsigned lds_dst, unsigned voff, u32x4 rs, unsigned soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %3 offen lds" ::"s"(lds_dst), "v"(voff), "s"(rs), "s"(soff) : "memory");
}

// K and V tiles (64 keys x 64 d each, 8 KiB + 8 KiB) of one (batch, kv head) into ring slots: each of the 4 waves moves two 1-KiB
// pieces (8 rows x 128 B) of K and two of V = 4 requests per wave per tile.
// Waves per workgroup of the forward and dQ kernels: 4 (one 32-query block x the 4 heads of a GQA group, two such workgroups per CU).  With 8
// (-DATTN_NW=8: two query blocks share each K / V tile, every wave issues 2 LDS-DMA requests per tile instead of 4, one workgroup per CU) the
// forward took 197-201 us against 179 and the backward 553-561 against 549: what the halved request count saves, the 8-wave barrier and the
// loss of the second, unsynchronised workgroup cost again.
#ifndef ATTN_NW
#define ATTN_NW 4
#endif
constexpr int ANW = ATTN_NW, ANP = 8 / ATTN_NW;  // waves per workgroup, K (and V) pieces per wave and tile
template <int SWZ_K, int SWZ_V> struct KvTileDma {
    u32x4 rs;             // base = K rows of the batch, column block of the kv head
    unsigned vk[ANP], vv[ANP];  // per-lane source byte offsets of this wave's K and V pieces inside a tile
    unsigned lds_piece;   // LDS byte address of this wave's first piece in slot 0
    unsigned tile_bytes;  // source bytes from one tile to the next
    __device__ __forceinline__ void init(const bf16_t* kbase, int64_t ld, int kv_cols, const char* smem, int wave, int lane) {
        rs = buffer_rsrc(kbase);
#pragma unroll
        for (int p = 0; p < ANP; ++p) {
            const int row = (p * ANW + wave) * 8 + (lane >> 3);
            vk[p] = (unsigned)((row * ld + ((lane & 7) ^ swz<SWZ_K>(row)) * 8) * 2);
            vv[p] = (unsigned)((row * ld + kv_cols + ((lane & 7) ^ swz<SWZ_V>(row)) * 8) * 2);
        }
        lds_piece = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_c*)smem + (unsigned)wave * 1024u);
        tile_bytes = (unsigned)(64 * ld * 2);
    }
    __device__ __forceinline__ void tile(int t, unsigned slot_bytes) const {
        const unsigned soff = (unsigned)t * tile_bytes;
#pragma unroll
        for (int p = 0; p < ANP; ++p) {
            dma16(lds_piece + slot_bytes + p * ANW * 1024, vk[p], rs, soff);
            dma16(lds_piece + slot_bytes + 8192 + p * ANW * 1024, vv[p], rs, soff);
        }
    }
    // request i (0 .. 2 ANP - 1) of a tile alone: K piece i >> 1 (even i) or V piece i >> 1 (odd i)
    __device__ __forceinline__ void piece(int t, unsigned slot_bytes, int i) const {
        const unsigned soff = (unsigned)t * tile_bytes;
        const int p = i >> 1;
        if (i & 1) dma16(lds_piece + slot_bytes + 8192 + p * ANW * 1024, vv[p], rs, soff);
        else dma16(lds_piece + slot_bytes + p * ANW * 1024, vk[p], rs, soff);
    }
};

// A [64 rows][64] bf16 tile (64 consecutive rows of one head's column block) into LDS by ONE wave, SWZ_ROW image: 8 requests of 8 rows x
// 128 B — whole 128-B lines, where a fragment load straight from global memory (lane = row) touches 32 rows x 32 B per instruction.
struct RowTileDma {
    u32x4 rs;
    unsigned voff[2];  // per-lane source byte offset inside a request, for even / odd requests (the swizzle's bit 2 follows the request)
    unsigned step;     // source bytes from one request to the next
    __device__ __forceinline__ void init(const bf16_t* base, int64_t ld, int lane) {
        rs = buffer_rsrc(base);
#pragma unroll
        for (int par = 0; par < 2; ++par)  // swz<SWZ_ROW>(8 i + (l >> 3)) = (l >> 4) ^ 4 (i & 1)
            voff[par] = (unsigned)(((lane >> 3) * ld + ((lane & 7) ^ (lane >> 4) ^ (4 * par)) * 8) * 2);
        step = (unsigned)(8 * ld * 2);
    }
    __device__ __forceinline__ void request(int i, unsigned lds_tile) const { dma16(lds_tile + i * 1024, voff[i & 1], rs, (unsigned)i * step); }
};

__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_;
    bf16x2_ v;
    v[0] = (bf16_t)a;
    v[1] = (bf16_t)b;
    return __builtin_bit_cast(unsigned, v);
}

}  // namespace

// What ssi_attn_bwd_mfma hands its two passes, attn_bwd_dq_launch (attn_bwd_dq.h) and attn_bwd_dkv_launch (attn_bwd_dkv.h).  Each launches its
// kernels, ORs the SSI_ATTN_USED_* bits of its choice into *used and returns SSI_OK or an error code (the codes and the bits share the
// positive range, hence the out-parameter).
struct AttnBwdArgs {
    const void* qkv; int64_t ld; const void *out, *dout; const float* lse; void* dqkv; float* delta;
    const int32_t *doc_start, *doc_end; const float* rope; int64_t table_len; const int32_t* positions;
    int64_t batch, seq; int n_heads, n_kv; void* workspace; int64_t workspace_bytes;
    const int32_t *plan_dev, *plan_header;  // plan_header: the plan's header on the host, validated; NULL = no plan
    hipStream_t stream;
};
