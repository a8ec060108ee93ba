// dK / dV of the MFMA flash attention (attn_mfma.h: orientation and shared helpers): attn_bwd_dkv_kernel (128-key workgroups, two per CU, optionally
// split over the query heads), attn_bwd_dkv2_kernel (one wave per SIMD, hand-placed software pipeline; plain rows or a work plan), the two
// reductions of the split forms and the rule that picks between them.  Part of the translation unit attention_mfma.hip, which includes it once.
#pragma once
#include "attn_mfma.h"
#include "attn_plan.h"

#ifndef DKV_RING
#define DKV_RING 6
#endif
#ifndef DKV_WAVES
#define DKV_WAVES 2
#endif

namespace {

// =====================================================================================================================
// backward: dK, dV
// =====================================================================================================================
// Workgroup = (b, kv head, 128-key group); wave w owns keys [key0 + 32 w, +32) and keeps their dK^T / dV^T in accumulators
// while the workgroup sweeps, for each of the `rep` query heads of the kv head in turn, the Q / dO tiles (32 queries) from
// the diagonal to the end of the sequence.  The tile of a step is staged ONCE for all four waves (LDS-DMA, double
// buffered, one step ahead), so Q and dO cross the L2 -> CU path once per 128 keys instead of once per 32, and the sum
// over the query heads of the group happens in registers: no cross-wave reduction, no partial buffers, one writer per
// output element.
// HSPLIT (round 4): a workgroup sweeps `heads_per_wg` of the group's query heads instead of all `rep` of them; its dK / dV sums leave as fp32
// partial rows in `partial` ([slot = head / heads_per_wg][B * S][KV][dK 64 | dV 64]) and attn_dkv_head_reduce_kernel adds the slots in a fixed order.  For
// launches whose workgroups cannot fill the chip: the longest workgroup IS the launch (B = 2, S = 2048: 256 workgroups, the heaviest with
// 256 steps: 176 us per layer where 65 is the launch's share of the chip), and a workgroup's steps are queries x heads.
template <bool HSPLIT>
__global__ __launch_bounds__(256, DKV_WAVES) void attn_bwd_dkv_kernel(const bf16_t* __restrict__ qkv, int64_t ld,
                                                           const bf16_t* __restrict__ dout, const float* __restrict__ lse,
                                                           const float* __restrict__ delta, bf16_t* __restrict__ dqkv,
                                                           const int32_t* __restrict__ doc_end, const float* __restrict__ rope,
                                                           const int32_t* __restrict__ positions, int S, int H, int KV,
                                                           float* __restrict__ partial, int heads_per_wg) {
    // ring of RING step buffers: [Q tile 4 KiB | dO tile 4 KiB | lse 128 B | delta 128 B]; requests run RING-1 steps ahead
    constexpr int SB = 8192 + 256;
    constexpr int RING = DKV_RING;
    __shared__ __attribute__((aligned(16))) char smem[RING * SB];
    TRACE_BEGIN();
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rep_all = H / KV;
    const int rep = HSPLIT ? heads_per_wg : rep_all;  // query heads this workgroup sweeps
    const int n_slots = rep_all / rep;                 // workgroups (and partial rows) per key group
    const int ngrp = S / 128;
    int kgrp, pair_, head0 = 0, slot = 0;  // low key groups (most work) are dispatched first
    if (HSPLIT) {
        int r;
        block_to_work(ngrp * n_slots, (int)(gridDim.x / (ngrp * n_slots)), r, pair_);
        kgrp = r / n_slots;
        slot = r % n_slots;
        head0 = slot * rep;
    } else {
        block_to_work(ngrp, (int)(gridDim.x / ngrp), kgrp, pair_);
    }
    const int kvh = pair_ % KV;
    const int b = pair_ / KV;
    const int h = lane >> 5;
    const int64_t row0 = (int64_t)b * S;
    const int64_t ldo = (int64_t)H * HD;
    const int key0 = kgrp * 128 + wave * 32;
    const int kg = key0 + (lane & 31);

    // -K * 2^-3 and -V as B operands (lane holds row key0 + (l & 31), d = 16 ks + 8 h + j).  With the operands negated and
    // +lse / +delta as the initial accumulators, the chains deliver  lse - S  and  delta - dP,  so that
    // P = exp2(-(lse - S) log2 e) needs one multiply (by a negative constant) and -dS = P (delta - dP) one more: no
    // subtractions, no zero-initialisation.  dK accumulates with the opposite sign and is flipped by the final scale.
    bf16x8 kf[4], vf[4];
    {
        const bf16_t* krow = qkv + (row0 + kg) * ld + (int64_t)H * HD + (int64_t)kvh * HD + 8 * h;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            kf[ks] = scale_frag(*reinterpret_cast<const bf16x8*>(krow + 16 * ks), -0.125f);
            vf[ks] = scale_frag(*reinterpret_cast<const bf16x8*>(krow + (int64_t)KV * HD + 16 * ks), -1.0f);
        }
    }
    f32x16 dk[2], dv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[i][r] = 0.f; dv[i][r] = 0.f; }

    // packed rows: key k is seen by the queries k <= q < doc_end[k] (doc_end is non-decreasing along a row): the tile loop stops
    // at the end of the document of the group's last key, a tile needs the document mask iff it reaches past the end of the
    // document of the wave's first key, and is dead for the wave from the end of the document of its last key on.
    const int de = doc_end ? doc_end[row0 + kg] : S;                      // this lane's key
    const int de_lo = doc_end ? doc_end[row0 + key0] : S;                 // first key of the wave
    const int de_hi = doc_end ? doc_end[row0 + key0 + 31] : S;            // last key of the wave
    const int q_end = doc_end ? doc_end[row0 + kgrp * 128 + 127] : S;     // last key of the group
    const int qb_first = kgrp * 4;                       // first 32-query tile that sees any key of the group
    const int per_head = (q_end + 31) / 32 - qb_first;   // tiles per query head
    const int n_steps = per_head * rep;
    // step -> (head of the group, query tile); each wave moves one 1-KiB piece of Q and one of dO per step.  Steps are issued in
    // order, so (head, tile) and the three source addresses advance incrementally: the per-step `step / per_head`, `step % per_head` and
    // 64-bit address arithmetic cost 67 scalar instructions per step and wave before (SQ_INSTS_SALU), a fifth of the step's issue
    int iss_qt = 0;                                  // query tile of the next request inside its head
    const int irow = wave * 8 + (lane >> 3), ichunk = (lane & 7) ^ swz<SWZ_DUAL>(wave * 8 + (lane >> 3));
    const u32x4 rs_q = buffer_rsrc(qkv + row0 * ld + (int64_t)(kvh * rep_all + head0) * HD);    // Q columns of the group's first head, this batch
    const u32x4 rs_do = buffer_rsrc(dout + row0 * ldo + (int64_t)(kvh * rep_all + head0) * HD);
    const unsigned voff_q = (unsigned)((irow * ld + ichunk * 8) * 2), voff_do = (unsigned)((irow * ldo + ichunk * 8) * 2);
    unsigned soff_q = (unsigned)(qb_first * 32 * ld * 2), soff_do = (unsigned)(qb_first * 32 * ldo * 2);  // scalar, advanced per request
    const float* iss_rc = (lane < 32 ? lse : delta) + ((int64_t)b * H + kvh * rep_all + head0) * S + qb_first * 32 + (lane & 31);
    const unsigned lds_piece = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_c*)smem + (unsigned)wave * 1024u);
    const unsigned lds_rc = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_c*)smem + 8192u);
    auto issue = [&](int step) {
        const unsigned buf = (unsigned)(step % RING) * SB;
        dma16(lds_piece + buf, voff_q, rs_q, soff_q);
        dma16(lds_piece + buf + 4096, voff_do, rs_do, soff_do);
        // row constants of the tile: lanes 0-31 fetch lse[q0 + l], lanes 32-63 delta[q0 + l - 32] (every wave issues the same
        // 256-B request so that all waves count 3 requests per step); two arrays, hence per-lane 64-bit addresses
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, off" ::"s"(lds_rc + buf), "v"(iss_rc) : "memory");
        if (++iss_qt == per_head) {  // next head of the group: back to the first query tile, one head further
            iss_qt = 0;
            soff_q += (unsigned)(HD * 2) - (unsigned)((per_head - 1) * 32 * ld * 2);
            soff_do += (unsigned)(HD * 2) - (unsigned)((per_head - 1) * 32 * ldo * 2);
            iss_rc += (int64_t)S - (int64_t)(per_head - 1) * 32;
        } else {
            soff_q += (unsigned)(32 * ld * 2);
            soff_do += (unsigned)(32 * ldo * 2);
            iss_rc += 32;
        }
    };
    int cur_qt = 0;  // query tile of the step being computed (steps run in order too)
    // -DDKV_STAMP (debug build, tools/dkv_stamps.py): cycle totals of wave 0 per phase of a step, left in the workgroup's first dq row
#ifdef DKV_STAMP
    PhaseStamps<true, 6> st;
    int st_steps = 0;
#else
    PhaseStamps<false, 6> st;
#endif
    // one step on ring buffer BUF (compile-time, so every LDS address is a hoisted per-lane base + an immediate)
    auto do_step = [&](int step, auto buf_c) {
        constexpr int BUF = decltype(buf_c)::value;
        const int q0 = (qb_first + cur_qt) * 32;
        if (++cur_qt == per_head) cur_qt = 0;
        const char* qt = smem + BUF * SB;
        const char* dt = qt + 4096;
        const float* rcs = reinterpret_cast<const float*>(qt + 8192);
        if constexpr (BUF % 2 == 0) {
            // one barrier per TWO steps: own requests of this step and the next have landed (later ones may stay in flight) ...
            if (step + RING - 3 < n_steps) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * (RING - 4)) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // tail: fewer requests are in flight than the constant assumes
            ring_barrier();  // ... and everybody else's; the buffers of steps -1 and -2 are free again
            if (step + RING - 2 < n_steps) issue(step + RING - 2);
            if (step + RING - 1 < n_steps) issue(step + RING - 1);
        }
        st.tick(0);  // wait + barrier + the two requests the barrier made room for
        if (q0 + 31 < key0 || q0 >= de_hi) return;  // wave-uniform: no query of the tile sees any key of this wave
#ifdef DKV_STAMP
        ++st_steps;
#endif
        f32x16 sacc, pacc;  // rows = queries q0 + rowmap(r, h): row constants come in runs of 4
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 l4 = *reinterpret_cast<const f32x4*>(rcs + 4 * h + 8 * g);
            const f32x4 d4 = *reinterpret_cast<const f32x4*>(rcs + 32 + 4 * h + 8 * g);
#pragma unroll
            for (int e = 0; e < 4; ++e) { sacc[4 * g + e] = l4[e]; pacc[4 * g + e] = d4[e]; }
        }
        // fragment reads ahead of the products that use them (see attn_fwd_kernel)
        bf16x8 qfr[4], dfr[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qfr[ks] = frag_row<SWZ_DUAL>(qt, 0, ks, lane);
            dfr[ks] = frag_row<SWZ_DUAL>(dt, 0, ks, lane);
        }
        __builtin_amdgcn_sched_barrier(0);
#ifdef DKV_STAMP
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
        st.tick(1);  // row constants + fragment reads landed
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qfr[ks], kf[ks], sacc, 0, 0, 0);
            pacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dfr[ks], vf[ks], pacc, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        st.tick(2);  // S / dP MFMAs issued
        bf16x8 dtr[2][2], qtr[2][2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int db = 0; db < 2; ++db) {
                dtr[s2][db] = frag_tr<SWZ_DUAL>(dt, s2 * 16, db * 32, lane);
                qtr[s2][db] = frag_tr<SWZ_DUAL>(qt, s2 * 16, db * 32, lane);
            }
        __builtin_amdgcn_sched_barrier(0);
        st.tick(3);  // transposed reads issued
        if (q0 < key0 + 32 || q0 + 31 >= de_lo) {  // edge tile: keys beyond the query or of an earlier document contribute nothing
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float p = __builtin_amdgcn_exp2f(sacc[r] * -LOG2E);
                const int q = q0 + rowmap(r, h);
                if (kg > q || q >= de) p = 0.f;
                sacc[r] = p;
                pacc[r] *= p;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(sacc[r] * -LOG2E);
                sacc[r] = p;
                pacc[r] *= p;
            }
        }
        st.tick(4);  // exponentials (includes waiting for S / dP)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const bf16x8 pf = acc_frag(sacc, s2), dsf = acc_frag(pacc, s2);
#pragma unroll
            for (int db = 0; db < 2; ++db) {
                dv[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dtr[s2][db], pf, dv[db], 0, 0, 0);
                dk[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtr[s2][db], dsf, dk[db], 0, 0, 0);
            }
        }
        st.tick(5);  // conversions + dV / dK MFMAs issued
    };
#pragma unroll
    for (int i = 0; i < RING - 2; ++i)
        if (i < n_steps) issue(i);
    static_assert(RING % 2 == 0 && RING >= 4 && RING <= 10, "the barrier cadence (one per two steps) needs an even ring");
    TRACE_LOOP_BEGIN();
    for (int step = 0; step < n_steps; step += RING) {
        do_step(step, std::integral_constant<int, 0>{});
        if (step + 1 < n_steps) do_step(step + 1, std::integral_constant<int, 1>{});
        if (step + 2 < n_steps) do_step(step + 2, std::integral_constant<int, 2>{});
        if (step + 3 < n_steps) do_step(step + 3, std::integral_constant<int, 3>{});
        if constexpr (RING > 4) {
            if (step + 4 < n_steps) do_step(step + 4, std::integral_constant<int, 4>{});
            if (step + 5 < n_steps) do_step(step + 5, std::integral_constant<int, 5>{});
        }
        if constexpr (RING > 6) {
            if (step + 6 < n_steps) do_step(step + 6, std::integral_constant<int, 6>{});
            if (step + 7 < n_steps) do_step(step + 7, std::integral_constant<int, 7>{});
        }
        if constexpr (RING > 8) {
            if (step + 8 < n_steps) do_step(step + 8, std::integral_constant<int, 8>{});
            if (step + 9 < n_steps) do_step(step + 9, std::integral_constant<int, 9>{});
        }
    }
    TRACE_LOOP_END();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (see attn_fwd_kernel)
#ifdef DKV_STAMP
    if (lane == 0 && wave == 0) {  // DEBUG BUILD ONLY: overwrites the first floats of the workgroup's first dq row
        float* dbg = reinterpret_cast<float*>(dqkv + (row0 + kgrp * 128) * ld);
        for (int i = 0; i < 6; ++i) dbg[i] = (float)st.total[i];
        dbg[6] = (float)(__builtin_readcyclecounter() - st.begin);
        dbg[7] = (float)st_steps;
        dbg[8] = (float)n_steps;
    }
#endif
    if constexpr (HSPLIT) {  // raw fp32 sums of this head: [head][row][kv head][dK 64 | dV 64]; scale, RoPE backward and rounding happen after the heads are added
        const int64_t t_rows = (int64_t)(gridDim.x / (ngrp * n_slots)) / KV * S;  // B * S
        float* prow = partial + (((int64_t)slot * t_rows + row0 + kg) * KV + kvh) * 128;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 vk, vv;
#pragma unroll
                for (int e = 0; e < 4; ++e) { vk[e] = dk[db][4 * g + e]; vv[e] = dv[db][4 * g + e]; }
                *reinterpret_cast<f32x4*>(prow + db * 32 + 8 * g + 4 * h) = vk;
                *reinterpret_cast<f32x4*>(prow + 64 + db * 32 + 8 * g + 4 * h) = vv;
            }
        TRACE_END(2, n_steps);
        return;
    }
    // lane = key, registers = d (runs of 4): 8-byte stores into the k and v column blocks of dqkv
    bf16_t* krow_out = dqkv + (row0 + kg) * ld + (int64_t)H * HD + (int64_t)kvh * HD;
    bf16_t* vrow_out = krow_out + (int64_t)KV * HD;
    const float* tb = rope ? rope + (int64_t)(positions ? positions[row0 + kg] : kg) * HD : nullptr;  // dK leaves in pre-RoPE space
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bf16x4 vk, vv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                vk[e] = (bf16_t)(dk[db][4 * g + e] * -0.125f);  // dk holds -sum dS Q
                vv[e] = (bf16_t)dv[db][4 * g + e];
            }
            if (tb) vk = unrope4(vk, tb, db * 32 + 8 * g + 4 * h);
            *reinterpret_cast<bf16x4*>(krow_out + db * 32 + 8 * g + 4 * h) = vk;
            *reinterpret_cast<bf16x4*>(vrow_out + db * 32 + 8 * g + 4 * h) = vv;
        }
    TRACE_END(2, n_steps);
}


// =====================================================================================================================
// backward: dK, dV — round 4: one wave per SIMD, hand-placed software pipeline
// =====================================================================================================================
// Same algebra, same operand images and the same summation order as attn_bwd_dkv_kernel (results are bit-identical), rebuilt around what
// its trace said (profiles/LAB_NOTES.md, round 3): a wave was bound by its own chain  fragment reads -> S / dP -> exponentials -> dV / dK,
// which two unsynchronised waves per SIMD overlapped only by chance (matrix pipe 41 % busy).  Here a wave has the SIMD to itself
// (__launch_bounds__(256, 1): the whole 512-entry register file) and overlaps the chain with itself:
//   * a wave owns 64 keys = two 32-key blocks kb; a workgroup = 256 keys of one (batch, kv head).  A UNIT = (query tile t, kb) is what a
//     step of the old kernel was: 8 S / dP products (SP), the exponentials (SM), 8 dV / dK products (DKV).  Q / dO row and transposed
//     fragments are read once per TILE and serve both units: half the LDS reads per product;
//   * a PERIOD = 16 MFMAs carries three units at once: SP of unit u+1, SM of unit u spread over the 16 MFMA gaps (per gap: one scale, one
//     exponential, one multiply, one packed conversion = 20 issue cycles beside the MFMA's 8, MI355X_MICROARCH.md "vector-instruction ISSUE cost"),
//     DKV of unit u-1.  Units alternate kb, so S / dP need one register set per kb and no double buffer;
//   * every MFMA is inline asm with its register class pinned (S / dP results in arch VGPRs where the vector ALU reads them, dK / dV sums and
//     the K / V operand fragments in accumulation registers) and every gap is closed by sched_barrier(0): hipcc allocates, the order is ours;
//   * the vector issue port is the scarce unit (8 + 20 of a gap's 32 cycles are taken), so the 32 LDS reads of a tile are SPREAD: one per gap
//     (two in 8 of the 32 gaps), each a register's last use behind and >= 8 gaps ahead of its first use; the LDS-DMA requests (ring of 12
//     tiles, one barrier and nine requests per wave per four tiles, counted vmcnt) go one per gap into the one half-period per tile that carries no LDS reads.  Bunched two
//     per gap in half of the gaps (first build) the reads cost 6-11 cycles each (in-kernel stamps).
// A wave does not skip the tiles in front of its keys (the old kernel's `return`): with one wave per SIMD nothing else could use the slot,
// and wave 0 of the workgroup needs every tile anyway — they run masked (p = 0 adds exact zeros).
constexpr int DKV2_RING = 12;
constexpr int DKV2_SB = 8192 + 256;

// VARLEN (round 5): packed rows.  The work comes from a host-built PLAN (ssi_attn_plan_build): an item = (row b, first key k0 — a multiple of
// 32 —, document [dstart, dend)) = the up to 256 keys k0 .. k0 + 255 of ONE document, items sorted by work, heaviest first; a workgroup =
// (item, kv head).  Because an item never leaves its document, everything that made packed rows expensive in the 128-key kernel is uniform
// here: the query tiles are those from k0 to the END OF THE DOCUMENT (tiles of other documents are skipped, not masked — they are simply
// not in the tile table), and the masked tiles are the 8 on the diagonal, with the plain rows' mask  key <= query.  The document's last tile,
// when the document does not end on a 32-row boundary, holds queries of the NEXT document: they are taken out by their row constant, not by
// a mask — the lanes that fetch lse[q] for q >= dend fetch 1e30 instead (one word of the plan's header), so P = exp2((S - lse) log2 e) = 0
// exactly and dS = P (dP - delta) = 0 for those rows at no cost in the loops (first build: a second condition in the mask, 1.5 compares and
// a scalar instruction per element more in every masked tile).  Lanes whose key lies outside [dstart, dend) — the head of the first item
// of a document that does not start on a 32-row boundary, the tail of its last item — compute on clamped rows and store nothing (key = lane:
// whatever they accumulate stays in their own columns).
template <bool VARLEN>
__global__ __launch_bounds__(256, 1) void attn_bwd_dkv2_kernel(const bf16_t* __restrict__ qkv, int64_t ld, const bf16_t* __restrict__ dout,
                                                               const float* __restrict__ lse, const float* __restrict__ delta,
                                                               bf16_t* __restrict__ dqkv, const float* __restrict__ rope,
                                                               const int32_t* __restrict__ positions, int S, int H, int KV,
                                                               const int4* __restrict__ items, const float* __restrict__ lse_beyond,
                                                               float* __restrict__ partial) {
    constexpr int SB = DKV2_SB, RING = DKV2_RING;
    __shared__ __attribute__((aligned(16))) char smem[RING * SB + DKV2_MAX_STEPS * 4];  // ring of [Q tile 4 KiB | dO tile 4 KiB | lse 128 B | delta 128 B], tile table
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rep_all = H / KV;
    // query heads this workgroup sweeps: all of the kv head's, or (VARLEN) the item's share of them — a heavy item of the plan is split over
    // the query heads (2 or 4 workgroups whose fp32 sums meet in attn_dkv_plan_reduce_kernel), so that a launch is not as long as its longest document
    int rep = rep_all, head0 = 0, pslot = -1;
    int kvh, b, k0, dstart = 0, dend = S;
    if constexpr (VARLEN) {  // workgroup -> (item, kv head): consecutive workgroups = the kv heads of one item, i.e. (KV = 8) one per XCD
        const int id = (int)blockIdx.x;
        kvh = id % KV;
        const int4 it = items[2 * (id / KV)], ih = items[2 * (id / KV) + 1];  // (uniform address: scalar loads)
        b = it.x, k0 = it.y, dstart = it.z, dend = it.w;
        head0 = ih.x, rep = ih.y, pslot = ih.z;
    } else {
        const int ngrp = S / 256;
        int kgrp, pair_;  // low key groups (most work) are dispatched first
        block_to_work(ngrp, (int)(gridDim.x / ngrp), kgrp, pair_);
        kvh = pair_ % KV;
        b = pair_ / KV;
        k0 = kgrp * 256;
    }
    const int h = lane >> 5;
    const int64_t row0 = (int64_t)b * S;
    const int64_t ldo = (int64_t)H * HD;
    const int key0 = k0 + wave * 64;

    // operands and row constants exactly as in attn_bwd_dkv_kernel: -K * 2^-3 and -V as B operands, +lse / +delta as initial accumulators
    bf16x8 kf[2][4], vf[2][4];
    int kg[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        kg[kb] = key0 + 32 * kb + (lane & 31);
        const int krow_i = VARLEN ? (kg[kb] < S ? kg[kb] : S - 1) : kg[kb];  // (an item's last keys may lie beyond the row: not stored)
        const bf16_t* krow = qkv + (row0 + krow_i) * ld + (int64_t)H * HD + (int64_t)kvh * HD + 8 * h;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            kf[kb][ks] = scale_frag(*reinterpret_cast<const bf16x8*>(krow + 16 * ks), -0.125f);
            vf[kb][ks] = scale_frag(*reinterpret_cast<const bf16x8*>(krow + (int64_t)KV * HD + 16 * ks), -1.0f);
            // from here on the fragments LIVE in accumulation registers: an "a" input alone makes hipcc keep them in arch VGPRs and copy
            // them over (4 v_accvgpr_write) in front of every MFMA that names them
            asm volatile("" : "=a"(kf[kb][ks]) : "0"(kf[kb][ks]));
            asm volatile("" : "=a"(vf[kb][ks]) : "0"(vf[kb][ks]));
        }
    }
    f32x16 dk[2][2], dv[2][2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) { dk[kb][i][r] = 0.f; dv[kb][i][r] = 0.f; }

    const int qb_first = k0 / 32;                                        // first 32-query tile that sees any key of the group
    const int per_head = (VARLEN ? (dend + 31) / 32 : S / 32) - qb_first;  // tiles per query head (plain rows: >= 8)
    // tiles of the two loops, each a multiple of 4 (a trip): plain rows come with rep % 4 == 0; an item of the plan that sweeps 1 or 2 heads
    // is padded with DUMMY tiles — any tile's Q / dO under lse = 1e30 for all its rows, i.e. P = 0, dS = 0: exact zeros added

    // ---- LDS-DMA requests: as in attn_bwd_dkv_kernel, three per tile and wave, issued part by part ----------------------------------------
    // Tile order: the MASKED tiles of every head first (the 8 tiles on the group's diagonal), then the rest of every head.  Two plain loops, one per form of the exponentials — not an if / else per period and not two inner loops taking turns:
    // wherever register tuples defined in different places meet (a diamond, a loop nest), hipcc's phi elimination splits them into scalars in
    // arch VGPRs and copies them into the accumulation registers in front of every MFMA (1 500 v_accvgpr moves and 400 scratch accesses in
    // the loop of the first build).  The order of the sums over the tiles differs from attn_bwd_dkv_kernel's, so the two kernels agree to
    // rounding, not bit for bit; each is reproducible run to run.
    // masked tiles per head: the group's diagonal (8 tiles; with VARLEN fewer when the document ends inside it)
    const int n_edge = VARLEN ? (per_head < 8 ? per_head : 8) : 8;
    const int n_masked_real = n_edge * rep, n_rest_real = (per_head - n_edge) * rep;
    const int n_masked = VARLEN ? (n_masked_real + 3) & ~3 : n_masked_real;          // tiles of the first loop
    const int n_steps = n_masked + (VARLEN ? (n_rest_real + 3) & ~3 : n_rest_real);
    // tile i of the sequence -> (head << 16) | tile of the head, looked up in a table in LDS behind the ring (built once per workgroup): the
    // requests run 6-7 tiles ahead of the products and cross heads and loops at other times, and a cursor kept in scalar registers by selects
    // cost ~50 scalar instructions per trip, all in front of its first MFMA
    int* seq_tab = reinterpret_cast<int*>(smem + RING * SB);
    for (int i = tid; i < n_steps; i += 256) {
        const int j = i < n_masked ? i : i - n_masked, len = i < n_masked ? n_edge : per_head - n_edge;
        int w = 0x8000;  // dummy: tile 0 of the first head, bit 15 = "its rows see nothing"
        if (!VARLEN || j < (i < n_masked ? n_masked_real : n_rest_real)) w = ((j / len) << 16) | ((i < n_masked ? 0 : n_edge) + j % len);
        seq_tab[i] = w;
    }
    const int irow = wave * 8 + (lane >> 3), ichunk = (lane & 7) ^ swz<SWZ_DUAL>(wave * 8 + (lane >> 3));
    const u32x4 rs_q = buffer_rsrc(qkv + row0 * ld + (int64_t)(kvh * rep_all + head0) * HD);
    const u32x4 rs_do = buffer_rsrc(dout + row0 * ldo + (int64_t)(kvh * rep_all + head0) * HD);
    const unsigned voff_q = (unsigned)((irow * ld + ichunk * 8) * 2), voff_do = (unsigned)((irow * ldo + ichunk * 8) * 2);
    const float* rc_base = (lane < 32 ? lse : delta) + ((int64_t)b * H + kvh * rep_all + head0) * S + (lane & 31);
    const unsigned lds_piece = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_c*)smem + (unsigned)wave * 1024u);
    const unsigned lds_rc = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_c*)smem + 8192u);
    // Requests are issued for EVERY ring position, also behind the last tile (the last tile again; the bytes go to a slot nobody reads): the
    // counted vmcnt waits hold without a tail case, and there is no branch inside a trip — hipcc sinks the pure vector instructions of a gap
    // across any basic-block boundary towards their users, which undoes the placement.
    // One request = M0 (LDS destination) written one gap AHEAD of the load that uses it (issue_m0 then issue_go, as in gemm_nt4dma: written
    // right in front of the load, every request stalls the wave's issue).
    auto seq_at = [&](int step) __attribute__((always_inline)) { return seq_tab[step < n_steps ? step : n_steps - 1]; };  // every lane reads the same word
    // Per trip of 4 tiles a wave issues 9 requests: the row constants of ONE of the four tiles (tile + wave: 256 B, lse | delta) FIRST, then its
    // Q and dO pieces of the four tiles (every wave used to fetch every tile's constants: 12 requests; a request costs its wave ~40 cycles)
    auto issue_m0 = [&](unsigned buf, int part) __attribute__((always_inline)) {  // buf = byte offset of the tile's ring slot
        const unsigned dst = part == 0 ? lds_piece + buf : part == 1 ? lds_piece + buf + 4096 : lds_rc + buf;
        asm volatile("s_mov_b32 m0, %0" ::"s"(dst) : "memory");
    };
    auto issue_go = [&](int w, int part) __attribute__((always_inline)) {  // w = table word of the tile
        const int qrow = (qb_first + (w & 0x7fff)) * 32, hoff = (w >> 16) * (HD * 2);
        if (part == 0) asm volatile("buffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(voff_q), "s"(rs_q), "s"((unsigned)(qrow * (int)ld * 2 + hoff)) : "memory");
        else if (part == 1) asm volatile("buffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(voff_do), "s"(rs_do), "s"((unsigned)(qrow * (int)ldo * 2 + hoff)) : "memory");
        else {
            const float* src = rc_base + ((w >> 16) * S + qrow);
            if constexpr (VARLEN) {  // queries of the next document (the document's last tile): lse = 1e30 -> P = 0, dS = 0
                const int seen_until = (w & 0x8000) ? 0 : dend;  // (a scalar select, no branch: a trip stays one basic block)
                if (lane < 32 && qrow + lane >= seen_until) src = lse_beyond;
            }
            asm volatile("global_load_lds_dword %0, off" ::"v"(src) : "memory");
        }
    };

    // ---- per-tile register state ------------------------------------------------------------------------------------------------------------
    f32x16 sacc[2], pacc[2];          // S' = lse - S and dP' = delta - dP of the unit in flight per key block
    f32x16 rcl, rcd;                  // lse / delta of the tile whose S / dP products come next (rows = queries rowmap(r, h))
    bf16x8 qfr[4], dfr[4];            // Q / dO row fragments of that tile
    s16x4 dtrh[2][2][2], qtrh[2][2][2];  // [s2][db][half]: dO / Q transposed fragments of the tile whose dV / dK products come next
    u32x4 pfu[2][2], dsu[2][2];       // [kb][s2]: P and -dS of a unit as bf16 operand fragments
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            pfu[i][j] = u32x4{0u, 0u, 0u, 0u};
            dsu[i][j] = u32x4{0u, 0u, 0u, 0u};
            dtrh[i][j][0] = dtrh[i][j][1] = s16x4{0, 0, 0, 0};  // the first period's dV / dK products add 0 * 0
            qtrh[i][j][0] = qtrh[i][j][1] = s16x4{0, 0, 0, 0};
        }

    // Ring offsets of a trip as three scalars (RING = 12 is not a power of two and a trip's 4 tiles never wrap: t % 4 == 0): bytes of the slot of
    // tile t (trip start), of tile t+4 (next trip's first) and of tile t+8 (first requested); tile t+i of the trip sits i * SB further on.
    unsigned ring_cur = 0, ring_nxt = 4 * SB, ring_req = 8 * SB;
    auto tile_base = [&](int i) __attribute__((always_inline)) { return smem + (i < 4 ? ring_cur + i * SB : ring_nxt); };  // i = tile - trip start, 0..4
    // read i (0..15) of the 16 row reads of a tile: 0-3 lse (rows 4h + 8i ..+3), 4-7 delta, 8-11 Q row fragments, 12-15 dO row fragments
    auto read_rows = [&](const char* qt, int i) __attribute__((always_inline)) {
        const float* rcs = reinterpret_cast<const float*>(qt + 8192);
        if (i < 4) {
            const f32x4 l4 = *reinterpret_cast<const f32x4*>(rcs + 4 * h + 8 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) rcl[4 * i + e] = l4[e];
        } else if (i < 8) {
            const f32x4 d4 = *reinterpret_cast<const f32x4*>(rcs + 32 + 4 * h + 8 * (i - 4));
#pragma unroll
            for (int e = 0; e < 4; ++e) rcd[4 * (i - 4) + e] = d4[e];
        } else if (i < 12) qfr[i - 8] = frag_row<SWZ_DUAL>(qt, 0, i - 8, lane);
        else dfr[i - 12] = frag_row<SWZ_DUAL>(qt + 4096, 0, i - 12, lane);
    };
    // read i (0..15) of the 16 transposed reads of a tile, in the order the dV / dK products use them: fragment i >> 1, half i & 1
    auto read_tr = [&](const char* qt, int i) __attribute__((always_inline)) {
        const int j = i >> 1, s2 = j >> 2, db = (j >> 1) & 1;
        if (j & 1) qtrh[s2][db][i & 1] = frag_tr_half<SWZ_DUAL>(qt, s2 * 16, db * 32, lane, i & 1);
        else dtrh[s2][db][i & 1] = frag_tr_half<SWZ_DUAL>(qt + 4096, s2 * 16, db * 32, lane, i & 1);
    };
    auto tr_frag = [&](const s16x4 (&hv)[2]) {
        typedef __attribute__((ext_vector_type(8))) short s16x8;
        return __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(hv[0], hv[1], 0, 1, 2, 3, 4, 5, 6, 7));
    };
    // S / dP product m (0..7) of key block kb: the S chain first (m = 0..3 = k-slices), then the dP chain; the first of a chain takes the row
    // constants as C.  S first because the exponentials of the next period start with S: its last product is 4 MFMAs (128 cycles) old when the
    // first scale reads it, dP's last product >= 52 cycles when the first multiply does (asm MFMAs are invisible to hipcc's hazard
    // recogniser; an MFMA result needs 44).
    auto sp_mfma = [&](int kb, int m) __attribute__((always_inline)) {
        const int ks = m & 3;
        if (m == 0) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(sacc[kb]) : "v"(qfr[0]), "a"(kf[kb][0]), "v"(rcl));
        else if (m == 4) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(pacc[kb]) : "v"(dfr[0]), "a"(vf[kb][0]), "v"(rcd));
        else if (m > 4) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(pacc[kb]) : "v"(dfr[ks]), "a"(vf[kb][ks]));
        else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(sacc[kb]) : "v"(qfr[ks]), "a"(kf[kb][ks]));
    };
    // dV / dK product j (0..7) of key block kb, in attn_bwd_dkv_kernel's order: for s2: for db: dV, dK
    auto dkv_mfma = [&](int kb, int j) __attribute__((always_inline)) {
        const int s2 = j >> 2, db = (j >> 1) & 1;
        if (j & 1) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(dk[kb][db]) : "v"(tr_frag(qtrh[s2][db])), "v"(dsu[kb][s2]));
        else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(dv[kb][db]) : "v"(tr_frag(dtrh[s2][db])), "v"(pfu[kb][s2]));
    };
    // exponentials of unit (tile at q0, kb), gap g of 16: scale + exponential of element g, -dS of element g - 1, one packed conversion
    float pv[16], dsv[16];
    auto sm_gap = [&](auto edge_c, int kb, int q0, int g) __attribute__((always_inline)) {
        constexpr bool EDGE = decltype(edge_c)::value;
        {
            float p = __builtin_amdgcn_exp2f(sacc[kb][g] * -LOG2E);
            if (EDGE) {
                const int q = q0 + rowmap(g, h);
                if (kg[kb] > q) p = 0.f;  // keys beyond the query contribute nothing
            }
            pv[g] = p;
        }
        if (g >= 1) dsv[g - 1] = pacc[kb][g - 1] * pv[g - 1];
        if (g >= 2 && !(g & 1)) { const int j = (g - 2) >> 1; pfu[kb][j >> 2][j & 3] = pack_bf16(pv[g - 2], pv[g - 1]); }
        if (g >= 3 && (g & 1)) { const int j = (g - 3) >> 1; dsu[kb][j >> 2][j & 3] = pack_bf16(dsv[g - 3], dsv[g - 2]); }
        if (g == 15) {
            dsv[15] = pacc[kb][15] * pv[15];
            pfu[kb][1][3] = pack_bf16(pv[14], pv[15]);
            dsu[kb][1][3] = pack_bf16(dsv[14], dsv[15]);
        }
    };

    // -DDKV2_STAMP (debug build, tools/attn_dkv_check.py stamps): cycle totals of wave 0 per half-period, by kind of tile (with / without the
    // barrier), left in the first floats of the workgroup's first dq row.  The stamp waits for the LDS reads in flight: read shares, not lengths.
#ifdef DKV2_STAMP
    PhaseStamps<true, 8, true> st2;
#else
    PhaseStamps<false, 8, true> st2;
#endif
#ifdef DKV2_STAMP_GAPS  // debug build: cycles per GAP of the periods of a tile without barrier / requests (wave 0), 32 totals
    PhaseStamps<true, 32, true> sg;
#else
    PhaseStamps<false, 32, true> sg;
#endif
    // period A of tile t: SM of unit (t, 0);  MFMAs 0-7 = dV / dK of (t-1, 1), 8-15 = S / dP of (t, 1) — the products whose results the vector
    // ALU needs come LAST, so that at most ~1.4 S / dP register sets are live at any time (first-half S / dP put 296 registers in flight and the
    // fragments into scratch).  Behind MFMA 7: the ring barrier (every second tile).  LDS reads: one transposed read of tile t per gap (fragment
    // j right behind the last use of tile t-1's fragment j), and from gap 10 on also the row constants of tile t+1
    auto period_a = [&](auto edge_c, auto sync_c, auto pos_c, int t, int q0) __attribute__((always_inline)) {
        constexpr int POS = decltype(pos_c)::value;  // position of tile t in its trip
        const char* ct_ = tile_base(POS);
        const char* nt_ = tile_base(POS + 1);
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            if (m < 8) dkv_mfma(1, m);
            else sp_mfma(1, m - 8);
            sm_gap(edge_c, 0, q0, m);
            if (m == 7 && decltype(sync_c)::value) {
                __builtin_amdgcn_sched_barrier(0);
                // own requests of tiles t+1 .. t+4 have landed — the Q / dO pieces of t+5, t+6, t+7 stay in flight; the row constants of
                // t+4 .. t+7 were this wave's FIRST request of the last trip ...
                asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                ring_barrier();  // ... and everybody's; every wave is done with tiles t-4 .. t-1: their slots are free
            }
            read_tr(ct_, m);                      // fragment m >> 1 of tile t-1 had its last use in MFMA m >> 1
            if (m >= 10) read_rows(nt_, m - 10);  // lse 0-3, delta 0-1 of tile t+1
            // An MFMA reads its C operand over its whole run and hipcc does not know the asm is one: left to itself it handed the registers of
            // lse / delta (dead to it behind MFMA 8 / 12) to the very next vector instruction, and the products ran on a half-overwritten C.
            // Keep them alive for two more gaps (64 cycles).
            if (m == 9) asm volatile("" ::"v"(rcl));
            if (m == 13) asm volatile("" ::"v"(rcd));
            __builtin_amdgcn_sched_barrier(0);
            if (m == 7) st2.tick(decltype(sync_c)::value ? 0 : 4);
            if (!decltype(sync_c)::value && t % 4 == 3) sg.tick(m);
        }
        st2.tick(decltype(sync_c)::value ? 1 : 5);
    };
    // period B of tile t: SM of unit (t, 1);  MFMAs 0-7 = dV / dK of (t, 0), 8-15 = S / dP of (t+1, 0);  row constants and row fragments of tile
    // t+1 under the first half (constants first: they are the C operands of MFMAs 8 and 9), the LDS-DMA requests of tiles t+RING-2, t+RING-1
    // (every second tile) under the second, which carries no LDS reads
    auto period_b = [&](auto edge_c, auto issue_c, int t, int q0) __attribute__((always_inline)) {
        const char* nt_ = tile_base(decltype(issue_c)::value + 1);
        int wv0 = 0, wv1 = 0, w0 = 0, w1 = 0;
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            if (m < 8) dkv_mfma(0, m);
            else sp_mfma(0, m - 8);
            sm_gap(edge_c, 1, q0, m);
            if (m < 2) read_rows(nt_, 6 + m);  // delta 2-3
            if (m < 8) read_rows(nt_, 8 + m);  // Q / dO row fragments, each 8 gaps ahead of its product
            {   // requests for tile t + RING - 4 (its slot was freed by this trip's barrier); in the trip's first tile also the row constants
                constexpr int KIND = decltype(issue_c)::value;  // position of tile t in its trip
                const int rt = t + RING - 4;
                if (m == 0) { wv0 = seq_at(rt); if (KIND == 0) wv1 = seq_at(rt + wave); }
                if (m == 6) { w0 = __builtin_amdgcn_readfirstlane(wv0); if (KIND == 0) w1 = __builtin_amdgcn_readfirstlane(wv1); }
                if (KIND == 0) {
                    if (m == 8) issue_go(w1, 2);
                    if (m == 9 || m == 10) issue_go(w0, m - 9);
                    if (m == 7) issue_m0(ring_req + (unsigned)wave * SB, 2);
                    if (m == 8 || m == 9) issue_m0(ring_req, m - 8);
                } else {
                    if (m == 9 || m == 10) issue_go(w0, m - 9);
                    if (m == 8 || m == 9) issue_m0(ring_req + KIND * SB, m - 8);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (m == 7) st2.tick(decltype(issue_c)::value == 0 ? 2 : 6);
            if (decltype(issue_c)::value == 3) sg.tick(16 + m);
        }
        st2.tick(decltype(issue_c)::value == 0 ? 3 : 7);
        if (decltype(issue_c)::value == 2) sg.reset();
    };

    // ---- prologue ---------------------------------------------------------------------------------------------------------------------------
    // Everything this wave has loaded from global memory is consumed HERE: hipcc does not see the LDS-DMA requests below, and its wait for a
    // value first used inside the loops (packed rows' document ends, when this kernel still took them) was `s_waitcnt vmcnt(0)` in every trip.
    asm volatile("" ::"v"(kg[0]), "v"(kg[1]) : "memory");
    __syncthreads();  // the table is complete (nothing is in flight yet that a vmcnt(0) could drain)
    // tiles 0 .. RING-5: this wave's two row-constant requests first (tiles wave and wave + 4), then its Q / dO pieces
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int w = __builtin_amdgcn_readfirstlane(seq_at(wave + 4 * i));
        issue_m0((unsigned)(wave + 4 * i) * SB, 2);
        asm volatile("s_nop 0" ::: "memory");
        issue_go(w, 2);
    }
#pragma unroll
    for (int i = 0; i < RING - 4; ++i) {
        const int w = __builtin_amdgcn_readfirstlane(seq_at(i));
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            issue_m0((unsigned)i * SB, part);
            asm volatile("s_nop 0" ::: "memory");
            issue_go(w, part);
        }
    }
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (RING - 4) - 2) : "memory");  // this wave's constants and its pieces of tile 0 have landed
    ring_barrier();
#pragma unroll
    for (int i = 0; i < 16; ++i) read_rows(smem, i);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 7" ::: "memory");  // the K / V fragments reach the asm MFMAs through v_accvgpr_write: let the last one land
#pragma unroll
    for (int m = 0; m < 8; ++m) sp_mfma(0, m);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");  // asm MFMAs are opaque to the hazard recogniser: S / dP of unit (0, 0) must have landed

    // ---- main loops: four tiles per trip (one barrier, nine requests per wave); a trip is ONE basic block ------------------------------------
    using T_ = std::true_type;
    using F_ = std::false_type;
    int cur_qt = 0;  // tile of the head in the masked loop (the other loop needs no query positions)
    auto trip = [&](auto edge_c, int t) __attribute__((always_inline)) {
        int q0[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            q0[i] = (qb_first + cur_qt) * 32;
            cur_qt = cur_qt + 1 == n_edge ? 0 : cur_qt + 1;
        }
        using P0 = std::integral_constant<int, 0>;
        using P1 = std::integral_constant<int, 1>;
        using P2 = std::integral_constant<int, 2>;
        using P3 = std::integral_constant<int, 3>;
        period_a(edge_c, T_{}, P0{}, t, q0[0]);
        period_b(edge_c, P0{}, t, q0[0]);
        period_a(edge_c, F_{}, P1{}, t + 1, q0[1]);
        period_b(edge_c, P1{}, t + 1, q0[1]);
        period_a(edge_c, F_{}, P2{}, t + 2, q0[2]);
        period_b(edge_c, P2{}, t + 2, q0[2]);
        period_a(edge_c, F_{}, P3{}, t + 3, q0[3]);
        period_b(edge_c, P3{}, t + 3, q0[3]);
        ring_cur = ring_nxt;
        ring_nxt = ring_req;
        ring_req = ring_req == 8 * SB ? 0u : ring_req + 4 * SB;
    };
    int t = 0;
    for (; t < n_masked; t += 4) trip(T_{}, t);
    for (; t < n_steps; t += 4) trip(F_{}, t);
    // ---- drain: dV / dK of the last unit ----------------------------------------------------------------------------------------------------
#pragma unroll
    for (int j = 0; j < 8; ++j) dkv_mfma(1, j);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_waitcnt vmcnt(0)" ::: "memory");  // results landed; no request of this wave is left in flight towards LDS
#ifdef DKV2_STAMP
    const unsigned long long st2_total = __builtin_readcyclecounter() - st2.begin;
#endif

    if constexpr (VARLEN) {
        if (pslot >= 0) {  // an item split over the query heads: raw fp32 sums [slot][kv head][key of the item][dK 64 | dV 64]; scale, RoPE backward
#pragma unroll             // and rounding happen after the heads are added (attn_dkv_plan_reduce_kernel)
            for (int kb = 0; kb < 2; ++kb) {
                float* prow = partial + (((int64_t)pslot * KV + kvh) * 256 + (kg[kb] - k0)) * 128;
#pragma unroll
                for (int db = 0; db < 2; ++db)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        f32x4 vk, vv;
#pragma unroll
                        for (int e = 0; e < 4; ++e) { vk[e] = dk[kb][db][4 * g + e]; vv[e] = dv[kb][db][4 * g + e]; }
                        *reinterpret_cast<f32x4*>(prow + db * 32 + 8 * g + 4 * h) = vk;
                        *reinterpret_cast<f32x4*>(prow + 64 + db * 32 + 8 * g + 4 * h) = vv;
                    }
            }
            return;
        }
    }
    const float* tb0 = rope ? rope : nullptr;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
        if (VARLEN && (kg[kb] < dstart || kg[kb] >= dend)) continue;  // another item's key (or none)
        bf16_t* krow_out = dqkv + (row0 + kg[kb]) * ld + (int64_t)H * HD + (int64_t)kvh * HD;
        bf16_t* vrow_out = krow_out + (int64_t)KV * HD;
        const float* tb = tb0 ? tb0 + (int64_t)(positions ? positions[row0 + kg[kb]] : kg[kb]) * HD : nullptr;  // dK leaves in pre-RoPE space
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                bf16x4 vk, vv;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    vk[e] = (bf16_t)(dk[kb][db][4 * g + e] * -0.125f);  // dk holds -sum dS Q
                    vv[e] = (bf16_t)dv[kb][db][4 * g + e];
                }
                if (tb) vk = unrope4(vk, tb, db * 32 + 8 * g + 4 * h);
                *reinterpret_cast<bf16x4*>(krow_out + db * 32 + 8 * g + 4 * h) = vk;
                *reinterpret_cast<bf16x4*>(vrow_out + db * 32 + 8 * g + 4 * h) = vv;
            }
    }
#ifdef DKV2_STAMP
    if (wave == 0 && lane == 0) {  // DEBUG BUILD ONLY: overwrites the first floats of the workgroup's first dq row
        float* dbg = reinterpret_cast<float*>(dqkv + (row0 + k0) * ld);
        for (int i = 0; i < 8; ++i) dbg[i] = (float)st2.total[i];
        dbg[8] = (float)st2_total;
        dbg[9] = (float)n_steps;
        dbg[10] = (float)(k0 / 256);
    }
#endif
#ifdef DKV2_STAMP_GAPS
    if (wave == 0 && lane == 0) {  // DEBUG BUILD ONLY
        float* dbg = reinterpret_cast<float*>(dqkv + (row0 + k0) * ld);
        for (int i = 0; i < 32; ++i) dbg[i] = (float)sg.total[i];
        dbg[32] = (float)n_steps;
    }
#endif
}

}  // namespace

// Adds the per-head partial rows of the HSPLIT form in head order (fixed: reproducible), then does what the unsplit kernel's epilogue does:
// dK * -2^-3 (the sums carry the opposite sign), optional RoPE backward, rounding, stores.  One thread per (row, kv head, 4 columns).
__global__ __launch_bounds__(256) void attn_dkv_head_reduce_kernel(const float* __restrict__ partial, int rep, int64_t t_rows, int KV,
                                                                   bf16_t* __restrict__ dqkv, int64_t ld, int H, const float* __restrict__ rope,
                                                                   const int32_t* __restrict__ positions, int S) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (row, kvh, c4) with c4 = 0..31: dK columns 4 c4 .. (c4 < 16), dV columns (c4 - 16) * 4 ..
    if (i >= t_rows * KV * 32) return;
    const int c4 = (int)(i & 31), kvh = (int)((i >> 5) % KV);
    const int64_t row = (i >> 5) / KV;
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
    for (int hd = 0; hd < rep; ++hd) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(partial + (((int64_t)hd * t_rows + row) * KV + kvh) * 128 + c4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) sum[e] += v[e];
    }
    bf16x4 o;
    bf16_t* dst;
    if (c4 < 16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (bf16_t)(sum[e] * -0.125f);
        if (rope) o = unrope4(o, rope + (int64_t)(positions ? positions[row] : (int)(row % S)) * HD, c4 * 4);
        dst = dqkv + row * ld + (int64_t)H * HD + (int64_t)kvh * HD + c4 * 4;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (bf16_t)sum[e];
        dst = dqkv + row * ld + (int64_t)(H + KV) * HD + (int64_t)kvh * HD + (c4 - 16) * 4;
    }
    *reinterpret_cast<bf16x4*>(dst) = o;
}

// The items of a plan that were split over the query heads: adds their slots' fp32 rows in slot order (fixed: reproducible), then the epilogue of
// attn_bwd_dkv2_kernel.  red = {b, k0, dstart, dend}, {first slot, slots, 0, 0} per split 256-key chunk; one thread per (key, 4 columns).
__global__ __launch_bounds__(256) void attn_dkv_plan_reduce_kernel(const float* __restrict__ partial, const int4* __restrict__ red, int KV,
                                                                   bf16_t* __restrict__ dqkv, int64_t ld, int H, const float* __restrict__ rope,
                                                                   const int32_t* __restrict__ positions, int S) {
    const int chunk = (int)blockIdx.x / (KV * 32), kvh = ((int)blockIdx.x / 32) % KV;
    const int4 it = red[2 * chunk], is = red[2 * chunk + 1];
    const int i = ((int)blockIdx.x % 32) * 256 + (int)threadIdx.x;  // (key of the chunk, c4): dK columns 4 c4 .. (c4 < 16), dV columns 4 (c4 - 16) ..
    const int key = i >> 5, c4 = i & 31, kg = it.y + key;
    if (kg < it.z || kg >= it.w) return;
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
    for (int sl = 0; sl < is.y; ++sl) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(partial + (((int64_t)(is.x + sl) * KV + kvh) * 256 + key) * 128 + c4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) sum[e] += v[e];
    }
    const int64_t row = (int64_t)it.x * S + kg;
    bf16x4 o;
    bf16_t* dst;
    if (c4 < 16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (bf16_t)(sum[e] * -0.125f);
        if (rope) o = unrope4(o, rope + (int64_t)(positions ? positions[row] : kg) * HD, c4 * 4);
        dst = dqkv + row * ld + (int64_t)H * HD + (int64_t)kvh * HD + c4 * 4;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (bf16_t)sum[e];
        dst = dqkv + row * ld + (int64_t)(H + KV) * HD + (int64_t)kvh * HD + (c4 - 16) * 4;
    }
    *reinterpret_cast<bf16x4*>(dst) = o;
}

// fp32 workspace the head-split dK / dV form wants for this shape (0: the launch fills the chip without it, or a single head per kv head)
// Workgroups per key group of the split form: all `rep` heads apart below 512 workgroups (two fit a CU: 512 fill the chip once, and the heaviest
// of them — queries x heads steps — is as long as the launch), two halves below 1024 (one long packed row: B = 1, S = 11 520 gives 720 workgroups
// whose heaviest sweeps a whole document x 4 heads = 256 steps where the chip's share per slot is 127); 1 = unsplit.
static int dkv_head_slots(int64_t batch, int64_t seq, int n_heads, int n_kv) {
    const int rep = n_heads / n_kv;
    const int64_t wgs = batch * n_kv * (seq / 128);
    if (rep <= 1 || seq % 128) return 1;
    if (wgs < 512) return rep;
    if (wgs < 1024 && rep % 2 == 0) return 2;
    return 1;
}
int64_t ssi_attn_mfma_bwd_workspace_bytes(int64_t batch, int64_t seq, int n_heads, int n_kv) {
    const int slots = dkv_head_slots(batch, seq, n_heads, n_kv);
    return slots <= 1 ? 0 : (int64_t)slots * batch * seq * n_kv * 128 * (int64_t)sizeof(float);
}

// The dK / dV pass of ssi_attn_bwd_mfma (delta comes from the dQ pass in front of it): ORs the SSI_ATTN_USED_* bits of its choice into *used.
// sel = the mode of ssi_set_attn_impl(SSI_ATTN_KERNEL_DKV)
static int attn_bwd_dkv_launch(const AttnBwdArgs& a, int sel, int* used) {
    const auto& [qkv, ld, out, dout, lse, dqkv, delta, doc_start, doc_end, rope, table_len, positions, batch, seq, n_heads, n_kv, workspace,
                 workspace_bytes, plan_dev, ph, st] = a;  // (ph: the plan's header on the host, validated by ssi_attn_bwd_mfma; NULL: no plan)
    const int rep = n_heads / n_kv;
    // dK / dV: the pipelined one-wave-per-SIMD kernel where its shape assumptions hold (256-key groups, an even number of tiles per group);
    // ssi_set_attn_impl(DKV, OLD) keeps the round-1..3 kernel
    // (plain causal rows, or packed rows with a plan; packed rows without one keep the 128-key kernel, whose waves skip the tiles outside
    //  their keys' documents — at B = 2, S = 8192 with documents of 440-1100 tokens the fixed 256-key groups of the plain form, masking
    //  instead of skipping, took 409 us against 329)
    // ... and only where its 256-key workgroups (one per CU at a time) can be balanced over the 256 CUs: the heaviest one walks (S / 32) * rep
    // tiles, the chip's share per CU is the total over 256.  B = 8, S = 2048: 256 against 288; B = 2, S = 2048: 256 against 72 — there the
    // 128-key kernel (two workgroups per CU, half the granularity) is faster.  Mode NEW forces this kernel whatever the balance.
    const int64_t ngrp2 = seq / 256, per0 = seq / 32;
    const int64_t total_tiles = batch * n_kv * rep * (ngrp2 * per0 - 8 * ngrp2 * (ngrp2 - 1) / 2);
    const bool balanced = per0 * rep * 256 <= total_tiles * 23 / 20 || sel == SSI_ATTN_MODE_NEW;
    const bool v2 = !doc_end && seq % 256 == 0 && rep % 4 == 0 && (seq / 32) * rep <= DKV2_MAX_STEPS && balanced && sel != SSI_ATTN_MODE_OLD;
    if (ph && sel != SSI_ATTN_MODE_OLD) {
        const int64_t want = ssi_attn_plan_workspace_bytes(ph);
        if (want > 0 && (!workspace || workspace_bytes < want || ((uintptr_t)workspace & 15))) {
            ssi_set_error("ssi_attn_varlen_bwd_plan: the plan splits %d chunks over the query heads and needs %lld bytes of workspace (got %lld)", ph[PLAN_W_N_REDUCE],
                          (long long)want, (long long)workspace_bytes);
            return SSI_ERR_WORKSPACE;
        }
        hipLaunchKernelGGL(attn_bwd_dkv2_kernel<true>, dim3((unsigned)(ph[PLAN_W_N_DKV_ITEMS] * n_kv)), dim3(256), 0, st, (const bf16_t*)qkv, ld, (const bf16_t*)dout, lse,
                           delta, (bf16_t*)dqkv, rope, positions, (int)seq, n_heads, n_kv, reinterpret_cast<const int4*>(plan_dev + ph[PLAN_W_DKV_OFF]),
                           reinterpret_cast<const float*>(plan_dev + PLAN_W_LSE_BEYOND), (float*)workspace);
        *used |= SSI_ATTN_USED_DKV2 | SSI_ATTN_USED_PLAN;
        if (ph[PLAN_W_N_REDUCE] > 0) {
            SSI_LAUNCH_CHECK();
            hipLaunchKernelGGL(attn_dkv_plan_reduce_kernel, dim3((unsigned)(ph[PLAN_W_N_REDUCE] * n_kv * 32)), dim3(256), 0, st, (const float*)workspace,
                               reinterpret_cast<const int4*>(plan_dev + ph[PLAN_W_REDUCE_OFF]), n_kv, (bf16_t*)dqkv, ld, n_heads, rope, positions, (int)seq);
            *used |= SSI_ATTN_USED_HEAD_SPLIT;
        }
    } else if (v2) {
        hipLaunchKernelGGL(attn_bwd_dkv2_kernel<false>, dim3((unsigned)(batch * n_kv * (seq / 256))), dim3(256), 0, st, (const bf16_t*)qkv, ld,
                           (const bf16_t*)dout, lse, delta, (bf16_t*)dqkv, rope, positions, (int)seq, n_heads, n_kv, (const int4*)nullptr,
                           (const float*)nullptr, (float*)nullptr);
        *used |= SSI_ATTN_USED_DKV2;
    } else {
        // small launches: one workgroup per query head + a reduction, when the caller brought the workspace (mode NO_HEAD_SPLIT: never)
        const int64_t want = ssi_attn_mfma_bwd_workspace_bytes(batch, seq, n_heads, n_kv);
        if (want > 0 && workspace && workspace_bytes >= want && ((uintptr_t)workspace & 15) == 0 && sel != SSI_ATTN_MODE_NO_HEAD_SPLIT) {
            const int slots = dkv_head_slots(batch, seq, n_heads, n_kv);
            hipLaunchKernelGGL(attn_bwd_dkv_kernel<true>, dim3((unsigned)(batch * n_kv * (seq / 128) * slots)), dim3(256), 0, st, (const bf16_t*)qkv, ld,
                               (const bf16_t*)dout, lse, delta, (bf16_t*)dqkv, doc_end, rope, positions, (int)seq, n_heads, n_kv, (float*)workspace,
                               rep / slots);
            SSI_LAUNCH_CHECK();
            hipLaunchKernelGGL(attn_dkv_head_reduce_kernel, dim3((unsigned)ssi_cdiv(batch * seq * n_kv * 32, 256)), dim3(256), 0, st,
                               (const float*)workspace, slots, batch * seq, n_kv, (bf16_t*)dqkv, ld, n_heads, rope, positions, (int)seq);
            *used |= SSI_ATTN_USED_HEAD_SPLIT;
        } else {
            hipLaunchKernelGGL(attn_bwd_dkv_kernel<false>, dim3((unsigned)(batch * n_kv * (seq / 128))), dim3(256), 0, st, (const bf16_t*)qkv, ld,
                               (const bf16_t*)dout, lse, delta, (bf16_t*)dqkv, doc_end, rope, positions, (int)seq, n_heads, n_kv, (float*)nullptr, rep);
        }
    }
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}
