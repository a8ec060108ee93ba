// bf16 MFMA GEMM, the persistent kernel.  Included by gemm_mfma.hip only, after gemm_wg8.h.
// =====================================================================================================================
// NT4: the k-contiguous (NT) form as a persistent kernel with one wave per SIMD — the shape the chip's own library picks
// for these sizes (256 x 256 x 64 tile, 4 waves), written for this step's epilogues.
//   * 256 threads = 4 waves as 2 x 2, 128 x 128 outputs per wave: all 256 AGPRs hold accumulators, LDS fragment traffic is
//     2/3 of the 8-wave kernel's.  The MFMAs are inline asm with the accumulator tied in place: with the whole AGPR file in
//     use the builtin form makes the allocator rotate accumulators through copies (hundreds of v_accvgpr moves per K-tile).
//   * gridDim.x (= CUs) workgroups draw output tiles from a scheduler (per-XCD spans, see below) until none is left; the
//     order in which tiles are handed out is the XCD-aware grouped order.  The HBM -> LDS operand stream (LDS-DMA, see the
//     main loop below) runs two K-steps ahead of the MFMAs and does not stop at tile boundaries: a tile's first operands
//     arrive while the previous tile is still being multiplied.
//   * One K-step = two phases of 64 MFMAs, each on one k-half's fragments held in registers; the ds_reads of the next phase
//     and the DMA issues ride at fixed MFMA slots (NT4_* below); two raw s_barriers per K-step.
//   * Epilogue straight from registers: two v_permlane16_swap per tile pair give each lane 8 consecutive bf16 columns
//     (16-B stores, 64 B per row per instruction); no LDS, so the operand stream keeps running underneath it.
// Requires K % 128 == 0 and not both `accumulate` and R; other NT calls use the 8-wave kernel above.
// =====================================================================================================================
#pragma once
#include "gemm_mfma.h"
#include <atomic>

namespace {

// cache-policy bits of the epilogue stores (2 = nt, 16 = sc1): measured neutral on the step's shapes, left at the default
constexpr int NT4_ST_AUX = 0;
constexpr int NT4_ST_AUX_BIG = 2;  // outputs far larger than the 256 MiB Infinity Cache (gate/up/act of the fused SwiGLU forward, 0.8 GB)
// schedule of the main loop (slots = MFMA indices inside a 64-MFMA phase): F1 reads every NT4_RS MFMAs from slot 0, barrier at NT4_BAR,
// NT4_NA pieces in phase A at NT4_A0 + i * NT4_SA, the other pieces in phase B at 3 + 5 i
constexpr int NT4_RS = 2, NT4_BAR = 40, NT4_A0 = 44, NT4_SA = 6, NT4_NA = 4;
constexpr int NT4_THREADS = 256;
constexpr int NT4_LDS_BYTES = PIPE_BYTES + 16;  // operand pipeline + the scheduler's broadcast word
constexpr int NT4_WM = 128, NT4_WN = 128;

// Tile scheduler state of the persistent kernel: per launch slot, 8 per-XCD "next tile of my span" counters + a count of
// finished workgroups (the last one to finish clears the slot for its next use).  Static device memory, no allocation.
__device__ int g_nt4_sched[16][16];
std::atomic<int> g_nt4_dynamic{0};
inline unsigned nt4_next_slot() {
    static std::atomic<unsigned> n{0};
    return n.fetch_add(1, std::memory_order_relaxed);
}

// A_COL / B_COL: false = the operand is k-contiguous in memory, true = k-strided (its tile is a [64 k][256 columns] image read
//      back with ds_read_b64_tr_b16, as in the 8-wave kernel).  NT = (false, false), NN = (false, true: data gradients against
//      the untransposed weights), TN = (true, true: weight gradients)
// PREV: 0 = C is overwritten, 1 = C += result (accumulate), 2 = C = R + result (residual)
// SPLITK: a unit of work is (output tile, K-slice); the fp32 partial tile goes to the workspace in the accumulator's own layout
//      (unit, wave, 16x16 tile, lane: every store is one contiguous KiB) and nt4_splitk_reduce_kernel finishes the tile
template <bool A_COL, bool B_COL, int EPI, int PREV, bool SPLITK, bool BATCHED>
__device__ __forceinline__ void nt4_body(char* smem, int tiles_m, int tiles_n, int64_t K, const bf16_t* __restrict__ A,
                                         int64_t lda, const bf16_t* __restrict__ B, int64_t ldb,
                                         bf16_t* __restrict__ C, int64_t ldc, const bf16_t* __restrict__ R,
                                         float alpha, const float* __restrict__ alpha_dev, EpiArgs ea, int slot,  // slot < 0: static tile order
                                         int splits, float* __restrict__ slabs) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int per_prob = tiles_m * tiles_n;        // output tiles of one problem
    const int ntiles_out = BATCHED ? per_prob * ea.batch : per_prob;  // output tiles of the launch (BATCHED: ssi_gemm_batched)
    const int ntiles = SPLITK ? ntiles_out * splits : ntiles_out;  // units of work
    // unit -> (problem, tile coordinates inside it)
    auto locate = [&](int t, int& tm, int& tn) {
        int tt = SPLITK ? t % ntiles_out : t, pb = 0;
        if constexpr (BATCHED) { pb = tt / per_prob; tt -= pb * per_prob; }
        tile_from_t(tt, tiles_m, tiles_n, tm, tn);
        return pb;
    };
    const int G = (int)gridDim.x;
    const int nk_total = (int)(K / BK);  // even, >= 4 (per K-slice when SPLITK)
    // K-steps [k_lo, k_hi) of unit t (slice boundaries rounded to even step counts)
    auto k_lo = [&](int t) { return SPLITK ? (int)(((int64_t)nk_total * (t / ntiles_out) / splits) & ~1LL) : 0; };
    auto k_hi = [&](int t) { return SPLITK ? ((t / ntiles_out) + 1 == splits ? nk_total : (int)(((int64_t)nk_total * (t / ntiles_out + 1) / splits) & ~1LL)) : nk_total; };

    // ---- tile scheduler: workgroups draw tiles from the contiguous span of their XCD (operand panels stay in that XCD's L2) and,
    // once it is empty, from the other spans.  Dynamic rather than "tile b, b+G, ...": a workgroup that starts late, or not at all,
    // because another kernel (RCCL during the gradient exchange) holds its CU, then costs its share of tiles, not a whole round.
    // The first tile of a workgroup is fixed (index b/8 of its XCD's span), later ones come from the span's atomic counter; the
    // request for the tile after next is issued at the start of a tile and read at its end, so its round trip is never waited for.
    int* sched = g_nt4_sched[slot < 0 ? 0 : slot];
    volatile int* lds_next = reinterpret_cast<volatile int*>(smem + PIPE_BYTES);
    const int xcd = (int)blockIdx.x & 7, span_q = ntiles >> 3, span_r = ntiles & 7;
    auto span_len = [&](int x) { return span_q + (x < span_r ? 1 : 0); };
    auto span_lo = [&](int x) { return x < span_r ? x * (span_q + 1) : span_r * (span_q + 1) + (x - span_r) * span_q; };
    // the first two tiles of every workgroup are fixed (no atomic in the prologue; shapes of up to two rounds never use the counters)
    auto span_wgs = [&](int x) { return (G - x + 7) >> 3; };  // workgroups whose blockIdx maps to XCD x
    auto span_fixed = [&](int x) { const int n = 2 * span_wgs(x); return n < span_len(x) ? n : span_len(x); };
    // slot < 0 = static order (tile index += G/8 within the span): optimal when every workgroup has its CU from the start, since
    // equal tiles then need no balancing and a greedy scheduler can only hurt (a workgroup that is a little early takes a third
    // tile where everybody should do two: measured -3..-12 % on the 2-3-round shapes).  The trainer switches to the dynamic
    // order when the gradient exchange shares the GPU with the backward GEMMs (world size > 1).
    const bool dynamic = slot >= 0;
    int my_idx = (int)blockIdx.x >> 3;  // static order: position inside the span
    int pending = 0;
    auto request_tile = [&]() {
        if (dynamic && tid == 0) pending = atomicAdd(&sched[xcd], 1);
    };
    auto receive_tile = [&]() -> int {
        if (!dynamic) {
            my_idx += G >> 3;
            return ((G & 7) == 0 && my_idx < span_len(xcd)) ? span_lo(xcd) + my_idx : -1;
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // everybody has read the previous answer
        if (tid == 0) {
            int t = -1;
            const int i = pending + span_fixed(xcd);
            if (i < span_len(xcd)) t = span_lo(xcd) + i;
            if (t < 0) {  // own span empty: take from the others (only at the very end of a launch); one look at all the counters
                int seen[8];  // first, so that a finished launch costs one load instead of seven atomic round trips
#pragma unroll
                for (int x = 0; x < 8; ++x) seen[x] = __hip_atomic_load(&sched[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                for (int k = 1; k < 8 && t < 0; ++k) {
                    const int x = (xcd + k) & 7;
                    if (seen[x] + span_fixed(x) >= span_len(x)) continue;
                    const int j = atomicAdd(&sched[x], 1) + span_fixed(x);
                    if (j < span_len(x)) t = span_lo(x) + j;
                }
            }
            *lds_next = t;
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        return __builtin_amdgcn_readfirstlane(*lds_next);
    };
    int cur = ((int)blockIdx.x >> 3) < span_len(xcd) ? span_lo(xcd) + ((int)blockIdx.x >> 3) : -1;
    int nxt = -1;
    if (dynamic) {
        const int second = ((int)blockIdx.x >> 3) + span_wgs(xcd);
        nxt = (cur >= 0 && second < span_len(xcd)) ? span_lo(xcd) + second : -1;
    }

    f32x4 acc[8][8];  // [j (n-tile)][i (m-tile)], defined by the zero-C MFMAs of each tile's first K-step
    // LDS: [A buf 0 | A buf 1 | B buf 0 | B buf 1]; with the buffer index a compile-time constant every fragment address is one
    // per-lane base register plus a 16-bit immediate
    auto tileA = [&](int buf) { return smem + buf * TILE_BYTES; };
    auto tileB = [&](int buf) { return smem + 2 * TILE_BYTES + buf * TILE_BYTES; };

    // ---- load side: (lv, lkt) = output tile and K-tile of the next fetch ------------------------------------------------
    int lkt = 0, lnk = nk_total;  // K-step of the next fetch inside its unit, K-steps of that unit
    const bf16_t* baseA = A;
    const bf16_t* baseB = B;
    const int64_t kstepA_ = A_COL ? BK * lda : BK, kstepB_ = B_COL ? BK * ldb : BK;
    auto set_load_tile = [&](int t) {
        int tm, tn;
        const int pb = locate(t, tm, tn);
        const bf16_t* Ap = BATCHED ? A + pb * ea.bsA : A;
        const bf16_t* Bp = BATCHED ? B + pb * ea.bsB : B;
        baseA = (A_COL ? Ap + (int64_t)tm * BM : Ap + (int64_t)tm * BM * lda) + k_lo(t) * kstepA_;
        // SwiGLU forward: the 256 tile columns are [gate 0..63 | up 0..63 | gate 64..127 | up 64..127] of 128 W13 column pairs
        baseB = (B_COL ? Bp + (int64_t)tn * BN : Bp + (int64_t)tn * (EPI == EPI_SWIGLU_FWD ? BN / 2 : BN) * ldb) + k_lo(t) * kstepB_;
        lnk = k_hi(t) - k_lo(t);
    };
    auto advance = [&]() {
        if (++lkt == lnk) {  // the fetches run at most 2 K-steps ahead of the MFMAs: this is always the switch to tile `nxt`
            lkt = 0;
            if (nxt >= 0) set_load_tile(nxt);  // after the last tile: keep re-fetching valid memory, never consumed
        }
    };
    // staging, ROW tiles: piece p = rows p*32 + (tid >> 3), 16-B chunk (tid & 7), swizzled on the LDS side.  COL tiles: piece p =
    // k-rows p*8 + (tid >> 5), chunk (tid & 31) swizzled on the SOURCE side (LDS image lane-linear); the swizzle term
    // col_swz(k-row) only depends on p through its parity.  One VGPR byte offset per operand (two for COL); the (piece,
    // K-tile) part rides in the scalar offset of the buffer load.
    auto lane_off = [&](bool col, int64_t ld, int odd) {
        if (col) return (int)(((tid >> 5) * ld + (((tid & 31) ^ col_swz(odd * 8 + (tid >> 5))) * 8)) * 2);
        return (int)(((tid >> 3) * ld + (tid & 7) * 8) * 2);
    };
    const int offA0 = lane_off(A_COL, lda, 0), offA1 = A_COL ? lane_off(true, lda, 1) : offA0;
    const int offB0 = lane_off(B_COL, ldb, 0), offB1 = B_COL ? lane_off(true, ldb, 1) : offB0;
    const int64_t kstepA = kstepA_, kstepB = kstepB_;  // elements per K-step: added to the (64-bit) buffer base
    auto pieceA = [&](int p) { return A_COL ? (int)(p * 8 * lda * 2) : (int)(p * 32 * lda * 2); };
    auto pieceB = [&](int p) {
        if (B_COL) return (int)(p * 8 * ldb * 2);
        if (EPI == EPI_SWIGLU_FWD) {
            const int blk64 = p >> 1;  // 64-row block of the tile: 0 gate lo, 1 up lo, 2 gate hi, 3 up hi
            return (int)((((blk64 & 1) ? ea.inter : 0) + (blk64 >> 1) * 64 + (p & 1) * 32) * ldb * 2);
        }
        return (int)(p * 32 * ldb * 2);
    };
    // COL fragments: the address of 16-column group t (0..7) of a wave's operand is (group-0 address) XOR (t << 5) — the
    // swizzle only touches the three chunk bits that t occupies — so one per-lane base per operand serves all 8 groups; the
    // XOR is redone per read (kept from being hoisted into 16 live registers by the asm in dma_body).
    int trA = 0, trB = 0;
    if (A_COL || B_COL) {
        const int i16 = lane & 15, q = i16 >> 2, pp = i16 & 3, k0l = 8 * (lane >> 4) + q;
        const int common = k0l * 512 + (pp >> 1) * 16 + 8 * (pp & 1) + (col_swz(k0l) << 4);
        trA = common + wm * 256;
        trB = common + wn * 256;
    }
    auto rd_tr = [&](const char* tile, int base, int t8, int kh) {
        typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
        const char* a0 = tile + (base ^ (t8 << 5)) + kh * 16384;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a0);
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + 2048));
        typedef __attribute__((ext_vector_type(8))) short s16x8;
        const s16x8 r = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        return __builtin_bit_cast(bf16x8, r);
    };
    using F_ = std::false_type;
    // ---- main loop ---------------------------------------------------------------------------------------------------------
    // LDS: two [A | B] buffers filled by LDS-DMA (buffer_load ... lds: no staging registers, no ds_write).  k-contiguous operand: a
    // piece = one wave-instruction = 8 rows x 128 B, lane-linear in LDS, the 16-byte-chunk swizzle applied to the per-lane SOURCE
    // address.  Per K-step and wave: 128 MFMAs, 32 ds_read_b128, 16 DMA issues, two barriers; nothing else touches a VGPR.
    //   registers : F0 = the 8 A + 8 B fragments of the k-half 0 of this K-step, F1 = those of k-half 1 (128 VGPRs)
    //   phase A   : 64 MFMAs on F0.  Under them F1 is read from this K-step's LDS buffer; once every wave has done so (barrier) the
    //               buffer is free and the DMA of K-step +2 starts into it
    //   phase B   : 64 MFMAs on F1.  The DMA of K-step +1 (issued one K-step ago) is waited for (counted vmcnt: this K-step's 16
    //               pieces stay in flight) + barrier, then F0 of the next K-step is read from the other buffer
    bf16x8 F0A[8], F0B[8], F1A[8], F1B[8];
    const int dofA = (int)(((tid >> 3) * lda + (((tid & 7) ^ ((tid >> 4) & 7)) * 8)) * 2);
    const int dofB = (int)(((tid >> 3) * ldb + (((tid & 7) ^ ((tid >> 4) & 7)) * 8)) * 2);
    // One piece = buffer_load_dwordx4 ... lds: LDS destination = M0 + lane * 16.  M0 is written one MFMA AHEAD of the load (dma_m0 then
    // dma_go): written right in front of it, as the builtin form does, every piece stalls the wave's issue for ~50 cycles (measured:
    // SQ_WAIT_INST_ANY +25 %, the loop 18 % longer); with an MFMA in between the wait disappears under the matrix pipe.
    typedef __attribute__((address_space(3))) char lds_c;
    const unsigned lds_wave = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_c*)smem + (unsigned)wave * 1024u);  // one cast, then integers
    auto dma_m0 = [&](int buf, int d) {  // piece d: 0..7 = A rows d*32 .. +31, 8..15 = B
        const unsigned dst = lds_wave + (unsigned)((d < 8 ? buf * TILE_BYTES : 2 * TILE_BYTES + buf * TILE_BYTES) + (d & 7) * 4096);  // tileA / tileB
        asm volatile("s_mov_b32 m0, %0" ::"s"(dst) : "memory");
    };
    u32x4 rsA, rsB;  // buffer resources of the K-step being fetched (set once per K-step by dma_src)
    auto dma_src = [&]() { rsA = buffer_rsrc(baseA + lkt * kstepA); rsB = buffer_rsrc(baseB + lkt * kstepB); };
    // k-contiguous operand: 8 rows x 128 B per piece, swizzled source chunk (dofA / dofB); k-strided operand: 2 k-rows x 512 B per piece with
    // the offA* / offB* source offsets (its LDS image is lane-linear already)
    auto dma_go = [&](int d) {
        if (d < 8) asm volatile("buffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(A_COL ? ((d & 1) ? offA1 : offA0) : dofA), "s"(rsA), "s"(pieceA(d)) : "memory");
        else asm volatile("buffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(B_COL ? ((d & 1) ? offB1 : offB0) : dofB), "s"(rsB), "s"(pieceB(d - 8)) : "memory");
    };
    auto dma = [&](int buf, int d) {  // prologue form: no MFMA to hide behind
        dma_m0(buf, d);
        asm volatile("s_nop 1" ::: "memory");
        dma_go(d);
    };
    auto fragA = [&](const char* t, int i, int kh) {
        if constexpr (A_COL) return rd_tr(t, trA, i, kh);
        else return read_frag<false>(t, wm * NT4_WM + i * 16, kh, lane);
    };
    auto fragB = [&](const char* t, int j, int kh) {
        if constexpr (B_COL) return rd_tr(t, trB, j, kh);
        else return read_frag<false>(t, wn * NT4_WN + j * 16, kh, lane);
    };
    // 64 MFMAs: every accumulator tile once, A fragment outer; extra(m) is issued right after MFMA m and pinned there
    auto phase = [&](const bf16x8 (&fa)[8], const bf16x8 (&fb)[8], auto zero_c, auto extra) {
#pragma unroll
        for (int m = 0; m < 64; ++m) {
            const int i = m >> 3, j = m & 7;
            if (decltype(zero_c)::value)
                asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=a"(acc[j][i]) : "v"(fb[j]), "v"(fa[i]));
            else
                asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[j][i]) : "v"(fb[j]), "v"(fa[i]));
            extra(m);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto dma_body = [&](auto cur_c, auto first) {
        constexpr int cur = decltype(cur_c)::value;
        if (A_COL) asm volatile("" : "+v"(trA));  // keep the per-read XOR of the transposed-read addresses from being hoisted into 16 registers
        if (B_COL) asm volatile("" : "+v"(trB));
        const char* la = tileA(cur);
        const char* lb = tileB(cur);
        const char* na = tileA(cur ^ 1);
        const char* nb = tileB(cur ^ 1);
        // DMA pieces are spread over the rest of the K-step (4 waves x 1 KiB every ~5 MFMAs keeps the CU's load path about half busy; bunched
        // right behind the barrier the pieces queue up and every issue stalls the wave): pieces 0..NA-1 in phase A, the rest in phase B
        constexpr int RS = NT4_RS, BAR = NT4_BAR, A0 = NT4_A0, SA = NT4_SA, NA = NT4_NA;
        static_assert(15 * RS + 4 <= BAR && BAR + 2 <= A0 - 1 && A0 + (NA - 1) * SA <= 63 && 3 + 5 * (15 - NA) <= 58, "DMA schedule");
        phase(F0A, F0B, first, [&](int m) {
            if (m < 16 * RS && m % RS == 0) {
                const int r = m / RS;
                if (r < 8) F1B[r] = fragB(lb, r, 1); else F1A[r - 8] = fragA(la, r - 8, 1);
            }
            if (m == BAR) {
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // every wave holds its F1: this buffer may be overwritten
                dma_src();
            }
            if (m >= A0 - 1 && m < A0 - 1 + NA * SA && (m - (A0 - 1)) % SA == 0) dma_m0(cur, (m - (A0 - 1)) / SA);
            if (m >= A0 && m < A0 + NA * SA && (m - A0) % SA == 0) dma_go((m - A0) / SA);
        });
        // the fetch cursor moves on BETWEEN the phases (this K-step's buffer resources were taken at the barrier above).  Not inside the
        // unrolled MFMA loops: with the split-K unit arithmetic (integer divisions) inlined there, the 64-iteration loop passes hipcc's
        // size limit for `#pragma unroll`, stays a runtime loop, and the accumulator array it then indexes dynamically lands in scratch
        advance();
        phase(F1A, F1B, F_{}, [&](int m) {
            if (m >= 2 && m < 2 + 5 * (16 - NA) && (m - 2) % 5 == 0) dma_m0(cur, NA + (m - 2) / 5);  // 2, 7, ...
            if (m >= 3 && m < 3 + 5 * (16 - NA) && (m - 3) % 5 == 0) dma_go(NA + (m - 3) / 5);       // 3, 8, ...
            if (m == 11) {
                // K-step +1 (16 pieces issued during the last K-step) has landed for this wave — the NA + 2 pieces of this K-step issued so
                // far may still be in flight — and, with the barrier, for every wave
                static_assert(NA == 4, "the counted wait below leaves NA + 2 = 6 pieces in flight");
                asm volatile("s_waitcnt vmcnt(6)\n\ts_barrier" ::: "memory");
            }
            // next K-step's F0 from the other buffer: 16 reads on the even slots 12..50 that carry no DMA issue (18, 28, 38, 48 do)
            if (m >= 12 && m <= 50 && !(m & 1) && m % 10 != 8) {
                const int r = (m - 12) / 2 - (m - 8) / 10;
                if (r < 8) F0B[r] = fragB(nb, r, 0); else F0A[r - 8] = fragA(na, r - 8, 0);
            }
        });
    };
    set_load_tile(cur >= 0 ? cur : 0);
    if (nk_total == 0) return;  // (never: keeps the scheduler state below out of a degenerate launch)
    dma_src();
#pragma unroll
    for (int d = 0; d < 16; ++d) dma(0, d);
    advance();
    dma_src();
#pragma unroll
    for (int d = 0; d < 16; ++d) dma(1, d);
    advance();
    asm volatile("s_waitcnt vmcnt(16)\n\ts_barrier" ::: "memory");  // K-step 0 is in LDS
#pragma unroll
    for (int r = 0; r < 8; ++r) F0B[r] = fragB(tileB(0), r, 0);
#pragma unroll
    for (int r = 0; r < 8; ++r) F0A[r] = fragA(tileA(0), r, 0);
    if (cur >= 0 && !dynamic) nxt = receive_tile();
    const float al = alpha * (alpha_dev ? *alpha_dev : 1.f);
    const int g = lane >> 4;
    while (cur >= 0) {
        int tm, tn;
        const int pb = locate(cur, tm, tn);
        const int nk = k_hi(cur) - k_lo(cur);
        using B0_ = std::integral_constant<int, 0>;
        using B1_ = std::integral_constant<int, 1>;
        // the tile after next is requested now and read after the epilogue: the answer is the oldest vector-memory operation in
        // flight, so the counted waits of the K-steps below retire it (asking later would mean waiting for the epilogue's stores)
        if (nxt >= 0) request_tile();
        dma_body(B0_{}, std::true_type{});
        dma_body(B1_{}, F_{});
        for (int kt = 2; kt < nk; kt += 2) {
            dma_body(B0_{}, F_{});
            dma_body(B1_{}, F_{});
        }
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");  // the asm MFMAs are opaque to the hazard recogniser: let the last results land
        // ---- epilogue: acc[j][i] holds C[m = wm*128 + i*16 + (lane&15)][n = wn*128 + j*16 + (lane>>4)*4 + r] -------------
        // pair(i, ja, jb): tiles ja, jb of m-tile i, scaled, rounded and exchanged (pair_swap): even 16-lane groups end up with 8
        // consecutive columns of tile ja, odd groups of tile jb
        auto pair = [&](int i, int ja, int jb, auto scale_c) {
            bf16x4 x, y;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float fx, fy;  // explicit reads, in program order: left to the allocator these become long-range AGPR shuffles
                asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(fx) : "a"(acc[ja][i][r]));
                asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(fy) : "a"(acc[jb][i][r]));
                x[r] = (bf16_t)(decltype(scale_c)::value ? fx * al : fx);
                y[r] = (bf16_t)(decltype(scale_c)::value ? fy * al : fy);
            }
            return pair_swap(x, y);
        };
        // duo(i, j0): the four tiles j0 .. j0+3 (64 columns = one 128-B line per row) of m-tile i as two 16-B vectors per lane
        // arranged for full-line stores (duo_rows)
        auto duo = [&](int i, int j0, auto scale_c, u32x4& lo, u32x4& hi) {
            const u32x4 oa = pair(i, j0, j0 + 1, scale_c), ob = pair(i, j0 + 2, j0 + 3, scale_c);
            duo_rows(oa, ob, lo, hi);
        };
        if constexpr (SPLITK) {
            // fp32 partial tile, accumulator layout: [unit][wave][i*8 + j][lane] x f32x4, one contiguous KiB per store
            const __amdgpu_buffer_rsrc_t rsS = buffer_rsrc_of(slabs + ((int64_t)cur * 4 + wave) * (64 * 64 * 4));
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    u32x4 v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float f;
                        asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(f) : "a"(acc[j][i][r]));
                        v[r] = __builtin_bit_cast(unsigned, f);
                    }
                    __builtin_amdgcn_raw_buffer_store_b128(v, rsS, lane * 16, (i * 8 + j) * 1024, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
        } else {
        const int64_t row0 = (int64_t)tm * BM + wm * NT4_WM;
        // lane -> (row within an 8-row group, column within a 64-column duo)
        const int lane_row = lane & 7, lane_col = ((lane >> 3) & 1) * 32 + (g & 1) * 16 + (g >> 1) * 8;
        auto epilogue = [&](auto scale_c) {
        if constexpr (EPI == EPI_PLAIN) {
            const int64_t tile_off = (BATCHED ? pb * ea.bsC : 0) + row0 * ldc + (int64_t)tn * BN + wn * NT4_WN;
            const __amdgpu_buffer_rsrc_t rsC = buffer_rsrc_of(C + tile_off);
            const __amdgpu_buffer_rsrc_t rsP = buffer_rsrc_of(PREV == 2 ? R + tile_off : C + tile_off);
            const int voff = (int)((lane_row * ldc + lane_col) * 2);
            auto soff = [&](int i, int h, int jd) { return (int)(((i * 16 + h * 8) * ldc + jd * 64) * 2); };
            u32x4 pv[2][4];  // [m-tile parity][(duo, half)]
            auto ldprev = [&](int i) {
#pragma unroll
                for (int q = 0; q < 4; ++q) pv[i & 1][q] = __builtin_amdgcn_raw_buffer_load_b128(rsP, voff, soff(i, q & 1, q >> 1), 0);
            };
            auto add_prev = [&](u32x4& o, const u32x4& p) {
                o = __builtin_bit_cast(u32x4, add_prev8(__builtin_bit_cast(bf16x8, o), __builtin_bit_cast(bf16x8, p)));
            };
            if (PREV) ldprev(0);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (PREV && i + 1 < 8) ldprev(i + 1);
#pragma unroll
                for (int jd = 0; jd < 2; ++jd) {
                    u32x4 lo, hi;
                    duo(i, jd * 4, scale_c, lo, hi);
                    if (PREV) { add_prev(lo, pv[i & 1][jd * 2]); add_prev(hi, pv[i & 1][jd * 2 + 1]); }
                    __builtin_amdgcn_raw_buffer_store_b128(lo, rsC, voff, soff(i, 0, jd), NT4_ST_AUX);
                    __builtin_amdgcn_raw_buffer_store_b128(hi, rsC, voff, soff(i, 1, jd), NT4_ST_AUX);
                    __builtin_amdgcn_sched_barrier(0);  // one duo at a time: bounded register pressure
                }
            }
        } else if constexpr (EPI == EPI_ROPE) {
            const int64_t tile_off = row0 * ldc + (int64_t)tn * BN + wn * NT4_WN;
            const __amdgpu_buffer_rsrc_t rsC = buffer_rsrc_of(C + tile_off);
            const int voff = (int)((lane_row * ldc + lane_col) * 2);
            auto soff = [&](int i, int hh, int jd) { return (int)(((i * 16 + hh * 8) * ldc + jd * 64) * 2); };
            const bool rot = (int64_t)tn * BN < ea.rot_cols;  // tile-uniform: the v heads are not rotated (rot_cols is a multiple of 256)
            // a lane's 8 columns start at a multiple of 8 inside a 64-wide head, the same one for every vector it stores: the
            // (cos, sin) it needs depend on the row only.  Positions of its 16 rows first, then the table rows one m-tile ahead.
            int prow[8][2];
            f32x4 cs[2][2][2];  // [m-tile parity][row half][pairs 0-1 | pairs 2-3]
            if (rot) {
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh) {
                        const int64_t r = row0 + i * 16 + hh * 8 + lane_row;
                        prow[i][hh] = ea.pos ? ea.pos[r] : (int)(r % ea.seq);
                    }
            }
            auto ldcs = [&](int i) {
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const float* tb = ea.rope + (int64_t)prow[i][hh] * 64 + (lane_col & 63);
                    cs[i & 1][hh][0] = *reinterpret_cast<const f32x4*>(tb);
                    cs[i & 1][hh][1] = *reinterpret_cast<const f32x4*>(tb + 4);
                }
            };
            auto rotate = [&](u32x4& o, const f32x4& c01, const f32x4& c23) {
                bf16x8 v = __builtin_bit_cast(bf16x8, o);
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const f32x4& c = p < 2 ? c01 : c23;
                    float o0, o1;
                    ssi_rope_pair((float)v[2 * p], (float)v[2 * p + 1], c[(p & 1) * 2], c[(p & 1) * 2 + 1], o0, o1);
                    v[2 * p] = (bf16_t)o0;
                    v[2 * p + 1] = (bf16_t)o1;
                }
                o = __builtin_bit_cast(u32x4, v);
            };
            if (rot) ldcs(0);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (rot && i + 1 < 8) ldcs(i + 1);
#pragma unroll
                for (int jd = 0; jd < 2; ++jd) {
                    u32x4 lo, hi;
                    duo(i, jd * 4, scale_c, lo, hi);
                    if (rot) { rotate(lo, cs[i & 1][0][0], cs[i & 1][0][1]); rotate(hi, cs[i & 1][1][0], cs[i & 1][1][1]); }
                    __builtin_amdgcn_raw_buffer_store_b128(lo, rsC, voff, soff(i, 0, jd), NT4_ST_AUX);
                    __builtin_amdgcn_raw_buffer_store_b128(hi, rsC, voff, soff(i, 1, jd), NT4_ST_AUX);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        } else if constexpr (EPI == EPI_SWIGLU_FWD) {
            // n-tiles 0..3 = gate columns c0 .. c0+63, n-tiles 4..7 = the matching up columns, c0 = tn*128 + wn*64:
            // GU = [gate | up], ACT = silu(gate).to(bf16) * up   (same rounding points as ssi_swiglu_fwd)
            const int64_t c0 = (int64_t)tn * (BN / 2) + wn * 64;
            const __amdgpu_buffer_rsrc_t rsGU = buffer_rsrc_of(C + row0 * ldc + c0);
            const __amdgpu_buffer_rsrc_t rsACT = buffer_rsrc_of(ea.out2 + row0 * ea.ld_out2 + c0);
            const int voff = (int)((lane_row * ldc + lane_col) * 2), voff2 = (int)((lane_row * ea.ld_out2 + lane_col) * 2);
            const int up_off = (int)(ea.inter * 2);
            auto act_of = [&](const u32x4& gq, const u32x4& uq) {
                return __builtin_bit_cast(u32x4, swiglu_fwd8(__builtin_bit_cast(bf16x8, gq), __builtin_bit_cast(bf16x8, uq)));
            };
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                u32x4 glo, ghi, ulo, uhi;
                duo(i, 0, scale_c, glo, ghi);
                duo(i, 4, scale_c, ulo, uhi);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const u32x4& gq = h ? ghi : glo;
                    const u32x4& uq = h ? uhi : ulo;
                    const int so = (int)(((i * 16 + h * 8) * ldc) * 2), so2 = (int)(((i * 16 + h * 8) * ea.ld_out2) * 2);
                    __builtin_amdgcn_raw_buffer_store_b128(gq, rsGU, voff, so, NT4_ST_AUX_BIG);
                    __builtin_amdgcn_raw_buffer_store_b128(uq, rsGU, voff, so + up_off, NT4_ST_AUX_BIG);
                    __builtin_amdgcn_raw_buffer_store_b128(act_of(gq, uq), rsACT, voff2, so2, NT4_ST_AUX_BIG);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            // SwiGLU backward: the tile is d act [256 rows, 256 columns of I], never stored: d gate = d act * up * silu'(gate),
            // d up = d act * silu(gate), gate/up read from GU, written to DGU (same formulas as ssi_swiglu_bwd)
            const int64_t c0 = (int64_t)tn * BN + wn * NT4_WN;
            const __amdgpu_buffer_rsrc_t rsGU = buffer_rsrc_of(ea.in2 + row0 * ea.ld_in2 + c0);
            const __amdgpu_buffer_rsrc_t rsDGU = buffer_rsrc_of(ea.out2 + row0 * ea.ld_out2 + c0);
            const int voff = (int)((lane_row * ea.ld_in2 + lane_col) * 2), voff2 = (int)((lane_row * ea.ld_out2 + lane_col) * 2);
            const int up_off = (int)(ea.inter * 2);
            u32x4 pg[2][2], pu[2][2];  // [unit parity][half]; unit = (m-tile i, duo jd), fetched one unit ahead
            auto ldprev = [&](int u) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int so = (int)((((u >> 1) * 16 + h * 8) * ea.ld_in2 + (u & 1) * 64) * 2);
                    pg[u & 1][h] = __builtin_amdgcn_raw_buffer_load_b128(rsGU, voff, so, 0);
                    pu[u & 1][h] = __builtin_amdgcn_raw_buffer_load_b128(rsGU, voff, so + up_off, 0);
                }
            };
            auto grads = [&](const u32x4& dq, const u32x4& gq, const u32x4& uq, u32x4& og_out, u32x4& ou_out) {
                bf16x8 og, ou;
                swiglu_bwd8(__builtin_bit_cast(bf16x8, gq), __builtin_bit_cast(bf16x8, uq), __builtin_bit_cast(bf16x8, dq), og, ou);
                og_out = __builtin_bit_cast(u32x4, og);
                ou_out = __builtin_bit_cast(u32x4, ou);
            };
            ldprev(0);
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                if (u + 1 < 16) ldprev(u + 1);
                const int i = u >> 1, jd = u & 1;
                u32x4 lo, hi;
                duo(i, jd * 4, scale_c, lo, hi);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    u32x4 og, ou;
                    grads(h ? hi : lo, pg[u & 1][h], pu[u & 1][h], og, ou);
                    const int so2 = (int)(((i * 16 + h * 8) * ea.ld_out2 + jd * 64) * 2);
                    __builtin_amdgcn_raw_buffer_store_b128(og, rsDGU, voff2, so2, NT4_ST_AUX);
                    __builtin_amdgcn_raw_buffer_store_b128(ou, rsDGU, voff2, so2 + up_off, NT4_ST_AUX);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        };
        if (al == 1.f) epilogue(std::false_type{});
        else epilogue(std::true_type{});
        }
        cur = nxt;
        if (cur >= 0) nxt = receive_tile();  // F0 of the next tile's K-step 0 (read in the last phase B) stays live across the epilogue
    }
    // Behind its last tile the fetch cursor kept requesting (valid memory, never consumed): those LDS-DMA requests must have landed before
    // the workgroup ends — its LDS goes to whichever workgroup the CU runs next.  (Also waits for the last epilogue's stores: the kernel's
    // end waits for them anyway.)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // the last workgroup to get here clears the scheduler slot for the launch that uses it next
    if (dynamic && tid == 0 && atomicAdd(&sched[8], 1) == G - 1) {  // plain stores: nobody reads the slot before this kernel has ended
        volatile int* vs = sched;
#pragma unroll
        for (int i = 0; i < 9; ++i) vs[i] = 0;
    }
}

// BATCHED: several problems of one shape in one launch (EpiArgs::batch)
template <bool A_COL, bool B_COL, int EPI, int PREV, bool SPLITK = false, bool BATCHED = false>
__global__ __launch_bounds__(NT4_THREADS, 1) void gemm_nt4dma_kernel(int tiles_m, int tiles_n, int64_t K, const bf16_t* __restrict__ A,
                                                                     int64_t lda, const bf16_t* __restrict__ B, int64_t ldb,
                                                                     bf16_t* __restrict__ C, int64_t ldc, const bf16_t* __restrict__ R,
                                                                     float alpha, const float* __restrict__ alpha_dev, EpiArgs ea, int slot,
                                                                     int splits, float* __restrict__ slabs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    nt4_body<A_COL, B_COL, EPI, PREV, SPLITK, BATCHED>(smem, tiles_m, tiles_n, K, A, lda, B, ldb, C, ldc, R, alpha, alpha_dev, ea, slot, splits, slabs);
}

// Finishes split-K tiles: one wave per (output tile, wave of the GEMM workgroup, m-tile i, 64-column duo).  Sums the K-slices'
// partials (contiguous KiB reads), then the same rounding points and the same full-line stores as the direct epilogue:
// C = (accumulate ? C : 0) + bf16(alpha * sum).
__global__ __launch_bounds__(256) void nt4_splitk_reduce_kernel(const float* __restrict__ slabs, int splits, int tiles_m, int tiles_n,
                                                                bf16_t* __restrict__ C, int64_t ldc, const bf16_t* __restrict__ R, float alpha,
                                                                const float* __restrict__ alpha_dev, int accumulate) {
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // (tile, wave, i, jd)
    const int ntiles = tiles_m * tiles_n;
    if (u >= (int64_t)ntiles * 64) return;
    const int jd = (int)(u & 1), i = (int)((u >> 1) & 7), wave = (int)((u >> 4) & 3), t = (int)(u >> 6);
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 4;
    int tm, tn;
    tile_from_t(t, tiles_m, tiles_n, tm, tn);
    const float al = alpha * (alpha_dev ? *alpha_dev : 1.f);
    f32x4 sum[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sum[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < splits; ++s) {
        const float* p = slabs + (((int64_t)s * ntiles + t) * 4 + wave) * (64 * 64 * 4) + (int64_t)(i * 8 + jd * 4) * 256 + lane * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(p + j * 256);
#pragma unroll
            for (int r = 0; r < 4; ++r) sum[j][r] += v[r];
        }
    }
    auto pair = [&](const f32x4& a, const f32x4& b) {
        bf16x4 x, y;
#pragma unroll
        for (int r = 0; r < 4; ++r) { x[r] = (bf16_t)(a[r] * al); y[r] = (bf16_t)(b[r] * al); }
        return pair_swap(x, y);
    };
    u32x4 lo, hi;
    duo_rows(pair(sum[0], sum[1]), pair(sum[2], sum[3]), lo, hi);
    const int lane_row = lane & 7, lane_col = ((lane >> 3) & 1) * 32 + (g & 1) * 16 + (g >> 1) * 8;
    bf16_t* base = C + ((int64_t)tm * BM + wm * NT4_WM + i * 16 + lane_row) * ldc + (int64_t)tn * BN + wn * NT4_WN + jd * 64 + lane_col;
    // previous values (accumulate) or the residual (same rows, same leading dimension as C) are added to the ROUNDED product, as the
    // unsplit epilogue does (F.linear then `+`: two roundings)
    const int64_t r_off = R ? (R - C) : 0;
    auto finish = [&](u32x4 o, bf16_t* dst) {
        if (accumulate || R)
            o = __builtin_bit_cast(u32x4, add_prev8(__builtin_bit_cast(bf16x8, o), *reinterpret_cast<const bf16x8*>(dst + r_off)));
        *reinterpret_cast<u32x4*>(dst) = o;
    };
    finish(lo, base);
    finish(hi, base + 8 * ldc);
}

template <bool A_COL, bool B_COL, int EPI, int PREV, bool SPLITK = false, bool BATCHED = false>
int launch_nt4(const GemmCall& c, EpiArgs ea = EpiArgs{}, int splits = 1, float* slabs = nullptr) {
    static_assert(!BATCHED || (!SPLITK && EPI == EPI_PLAIN), "batched form: plain epilogue, no split-K");
    auto kern = gemm_nt4dma_kernel<A_COL, B_COL, EPI, PREV, SPLITK, BATCHED>;
    // one-time set-up per instantiation as C++11 thread-safe statics: the forward thread and autograd's backward thread may both be the
    // first to launch a given form
    static const hipError_t attr_rc = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, NT4_LDS_BYTES);
    if (attr_rc != hipSuccess) { ssi_set_error("gemm_nt4: cannot reserve %d B of LDS: %s", NT4_LDS_BYTES, hipGetErrorString(attr_rc)); return SSI_ERR_HIP + (int)attr_rc; }
    static const int num_cu = [] {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        return cus;
    }();
    const int ntiles = c.tm * c.tn * (SPLITK ? splits : 1) * (BATCHED ? ea.batch : 1);
    int grid = ntiles < num_cu ? ntiles : num_cu;
    const int slot = g_nt4_dynamic.load(std::memory_order_relaxed) ? (int)(nt4_next_slot() & 15) : -1;  // consecutive launches: different slots
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(NT4_THREADS), NT4_LDS_BYTES, c.stream, c.tm, c.tn, c.K, (const bf16_t*)c.A, c.lda,
                       (const bf16_t*)c.B, c.ldb, (bf16_t*)c.C, c.ldc, (const bf16_t*)c.R, c.alpha, c.alpha_dev, ea, slot, splits, slabs);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

}  // namespace
