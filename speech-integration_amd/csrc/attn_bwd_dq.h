// dQ of the MFMA flash attention (attn_mfma.h: orientation and shared helpers): attn_bwd_dq_kernel (one 32-query block per wave, two workgroups
// per CU), attn_bwd_dq2_kernel (one wave per SIMD, hand-placed software pipeline, persistent workgroups; plain rows or a work plan) and the
// rule that picks between them.  Part of the translation unit attention_mfma.hip, which includes it once.
#pragma once
#include "attn_mfma.h"
#include "attn_plan.h"

namespace {

// =====================================================================================================================
// backward: dQ   (same decomposition as the forward)
// =====================================================================================================================
__global__ __launch_bounds__(64 * ANW, ANW == 8 ? 1 : 2) void attn_bwd_dq_kernel(const bf16_t* __restrict__ qkv, int64_t ld, const bf16_t* __restrict__ out,
                                                          const bf16_t* __restrict__ dout, const float* __restrict__ lse,
                                                          float* __restrict__ delta, bf16_t* __restrict__ dqkv,
                                                          const int32_t* __restrict__ doc_start, const float* __restrict__ rope,
                                                          const int32_t* __restrict__ positions, int S, int H, int KV) {
    __shared__ __attribute__((aligned(16))) char smem[3 * 2 * 8192];  // ring of 3 x [K | V][64][64] bf16
    TRACE_BEGIN();
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rep = H / KV, qpw = ANW / rep;
    const int nqb = S / (32 * qpw);
    int rank_, pair_;
    block_to_work(nqb, (int)(gridDim.x / nqb), rank_, pair_);
    const int qgrp = nqb - 1 - rank_;
    const int kvh = pair_ % KV;
    const int b = pair_ / KV;
    const int head = kvh * rep + wave % rep;
    const int q0 = (qgrp * qpw + wave / rep) * 32;
    const int nt = ((qgrp * qpw + qpw - 1) * 32 + 31) / 64 + 1;
    const int h = lane >> 5;
    const int64_t row0 = (int64_t)b * S;
    const bf16_t* kbase = qkv + row0 * ld + (int64_t)H * HD + (int64_t)kvh * HD;
    const int qg = q0 + (lane & 31);
    // packed rows: see attn_fwd_kernel
    const int ds = doc_start ? doc_start[row0 + qg] : 0;
    const int ds_lo = doc_start ? doc_start[row0 + q0] : 0;
    const int ds_hi = doc_start ? doc_start[row0 + q0 + 31] : 0;
    const int t_first = doc_start ? doc_start[row0 + qgrp * qpw * 32] / 64 : 0;

    bf16x8 qf[4], dof[4];
    {
        const bf16_t* qrow = qkv + (row0 + qg) * ld + (int64_t)head * HD + 8 * h;
        const bf16_t* drow = dout + (row0 + qg) * ((int64_t)H * HD) + (int64_t)head * HD + 8 * h;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qf[ks] = scale_frag(*reinterpret_cast<const bf16x8*>(qrow + 16 * ks), 0.125f);
            dof[ks] = *reinterpret_cast<const bf16x8*>(drow + 16 * ks);
        }
    }
    const float lq = lse[((int64_t)b * H + head) * S + qg];
    // delta = rowsum(dO * O) of this lane's query row: each half-wave holds half of the row (the dO fragments are already here);
    // written out for the dK/dV kernel, which runs after this one (every (row, head) belongs to exactly one wave)
    float dl = 0.f;
    {
        const bf16_t* orow = out + (row0 + qg) * ((int64_t)H * HD) + (int64_t)head * HD + 8 * h;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 of = *reinterpret_cast<const bf16x8*>(orow + 16 * ks);
#pragma unroll
            for (int j = 0; j < 8; ++j) dl += (float)of[j] * (float)dof[ks][j];
        }
        dl += __shfl_xor(dl, 32, 64);
        if (h == 0) delta[((int64_t)b * H + head) * S + qg] = dl;
    }
    f32x16 dq[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[i][r] = 0.f;

    // -DDQ_STAMP (debug build, tools/dkv_stamps.py dq): cycle totals of wave 0 per phase of a tile, left in the wave's first dq row
#ifdef DQ_STAMP
    PhaseStamps<true, 6> qs;
    int qs_tiles = 0;
#else
    PhaseStamps<false, 6> qs;
#endif
    KvTileDma<SWZ_DUAL, SWZ_ROW> kvdma;
    kvdma.init(kbase, ld, KV * HD, smem, wave, lane);
    kvdma.tile(t_first, 0);
    if (t_first + 1 < nt) kvdma.tile(t_first + 1, 16384);
    auto tile_step = [&](int t, auto buf_c) {
        constexpr int BUF = decltype(buf_c)::value;
        const char* kt = smem + BUF * 16384;
        const char* vt = kt + 8192;
        if (t + 1 < nt) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * ANP) : "memory");  // own pieces of tile t landed (tile t+1 may fly)
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ring_barrier();  // everybody's pieces landed; the slot of tile t-1 is free again
        if (t + 2 < nt) kvdma.tile(t + 2, ((BUF + 2) % 3) * 16384);
        qs.tick(0);  // wait + barrier + the 4 requests of tile t+2
        const int k0 = t * 64;
        if (k0 <= q0 + 31 && k0 + 63 >= ds_lo) {
#ifdef DQ_STAMP
            ++qs_tiles;
#endif
            // fragment reads ahead of the products that use them (see attn_fwd_kernel)
            bf16x8 kfr[2][4], vfr[2][4];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    kfr[kb][ks] = frag_row<SWZ_DUAL>(kt, kb * 32, ks, lane);
                    vfr[kb][ks] = frag_row<SWZ_ROW>(vt, kb * 32, ks, lane);
                }
            __builtin_amdgcn_sched_barrier(0);
#ifdef DQ_STAMP
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
            qs.tick(1);  // 16 row-fragment reads landed
            f32x16 sacc[2], pacc[2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) { sacc[kb][r] = -lq; pacc[kb][r] = -dl; }  // S'^T = K Q^T - lse, dP'^T = V dO^T - delta
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[kb][ks], qf[ks], sacc[kb], 0, 0, 0);
                    pacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[kb][ks], dof[ks], pacc[kb], 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
            qs.tick(2);  // 16 S / dP MFMAs issued
            bf16x8 ktr[4][2];
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int db = 0; db < 2; ++db) ktr[s][db] = frag_tr<SWZ_DUAL>(kt, s * 16, db * 32, lane);
            __builtin_amdgcn_sched_barrier(0);
            qs.tick(3);  // 16 transposed reads issued
            if (k0 + 63 > q0 || k0 < ds_hi) {  // edge tile: keys beyond the query or before its document contribute nothing
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float p = __builtin_amdgcn_exp2f(sacc[kb][r] * LOG2E);
                        const int key = k0 + kb * 32 + rowmap(r, h);
                        if (key > qg || key < ds) p = 0.f;
                        sacc[kb][r] = p * pacc[kb][r];  // dS^T (the 1/sqrt(d) factor is applied once at the end)
                    }
            } else {
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) sacc[kb][r] = __builtin_amdgcn_exp2f(sacc[kb][r] * LOG2E) * pacc[kb][r];
            }
            qs.tick(4);  // exponentials (includes waiting for S / dP)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const bf16x8 dsf = acc_frag(sacc[s >> 1], s & 1);
#pragma unroll
                for (int db = 0; db < 2; ++db)
                    dq[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktr[s][db], dsf, dq[db], 0, 0, 0);
            }
            qs.tick(5);  // conversions + 8 dQ MFMAs issued
        }
    };
    TRACE_LOOP_BEGIN();
    for (int t = t_first; t < nt; t += 3) {
        tile_step(t, std::integral_constant<int, 0>{});
        if (t + 1 < nt) tile_step(t + 1, std::integral_constant<int, 1>{});
        if (t + 2 < nt) tile_step(t + 2, std::integral_constant<int, 2>{});
    }
    TRACE_LOOP_END();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (see attn_fwd_kernel)
    bf16_t* drow = dqkv + (row0 + qg) * ld + (int64_t)head * HD;
#ifdef DQ_STAMP
    unsigned long long qs_total = __builtin_readcyclecounter() - qs.begin;
#endif
    // rope != NULL: the gradient leaves in pre-RoPE space (backward of the rotation fused here, saves a pass over dqkv)
    const float* tb = rope ? rope + (int64_t)(positions ? positions[row0 + qg] : qg) * HD : nullptr;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bf16x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (bf16_t)(dq[db][4 * g + e] * 0.125f);
            if (tb) v = unrope4(v, tb, db * 32 + 8 * g + 4 * h);
            *reinterpret_cast<bf16x4*>(drow + db * 32 + 8 * g + 4 * h) = v;
        }
#ifdef DQ_STAMP
    if (wave == 0) {  // DEBUG BUILD ONLY: lane 0's row of head `head` carries the totals (overwrites the gradient there)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) {
            float* dbg = reinterpret_cast<float*>(drow);
            for (int i = 0; i < 6; ++i) dbg[i] = (float)qs.total[i];
            dbg[6] = (float)qs_total;
            dbg[7] = (float)qs_tiles;
            dbg[8] = (float)(nt - t_first);
        }
    }
#endif
    TRACE_END(1, nt - t_first);
}

// =====================================================================================================================
// backward: dQ — round 4: one wave per SIMD, hand-placed software pipeline, persistent workgroups
// (4 query heads per kv head; plain causal rows: S a multiple of 128, i.e. of 64 x 2, 4 or 8 query blocks per workgroup — the host takes the
//  largest count that divides S / 64 and fills the chip; packed rows: round 5, from a work plan, see VARLEN below)
// =====================================================================================================================
// The recipe of attn_bwd_dkv2_kernel (further down: read its header first) applied to dQ.  An ITEM = 64 queries x the 4 query heads of a kv
// head (wave w = head w), sweeping the 64-key tiles 0 .. its own; a UNIT = (32-key block kb, 32-query block qb) of a tile: 8 S^T / dP^T
// MFMAs (SP), 16 x { fma, exponential, multiply } + 8 packed conversions (SM), 4 dQ^T MFMAs (DQ).  A PERIOD = 12 MFMAs: DQ of unit u-1
// (MFMAs 0-3), SP of unit u+1 (4-11, S first), SM of unit u spread over the 12 gaps; four periods = one tile = one trip of the loop (one basic
// block, one barrier, four LDS-DMA requests per wave, 32 LDS reads: 8 per period, each >= 8 gaps ahead of its first use).  K / V row fragments
// and K transposed fragments of a key block serve both query blocks.  Q / dO operand fragments and the dQ sums live in accumulation
// registers; delta rides in as the C operand of the dP chain (a replicated register set that is never dead), lse as the addend of the
// exponent's fma (which also carries the 1/sqrt(d): the Q fragments stay as loaded).  Only the last tile of an item (its diagonal) needs the
// causal mask: a second, masked loop of one trip behind the first.
//
// With 400 registers per wave a CU holds ONE workgroup, so whatever an item does before and behind its tiles — waiting for its operands,
// converting them, storing dQ — is time the matrix pipe stands still: ~19 000 cycles per item against ~2 350 per tile and 16.5 tiles per item
// when every item was a workgroup (profiles/r04_dq2_stamps.txt).  Hence the workgroups are PERSISTENT: a workgroup walks DQ2_ITEMS = 8 (4, 2 for
// small launches) query blocks of one (batch, kv head) — blocks g, 2W-1-g, 2W+g, 4W-1-g, ... of the S/64, W = S/64/DQ2_ITEMS workgroups per
// pair, every workgroup the same number of tiles — and the Q, dO and O rows of the NEXT item are requested (LDS-DMA, whole 128-B lines, into per-wave images: no barrier)
// while the current item computes; its lse one item ahead into registers; the RoPE table rows for the store into LDS as well.
constexpr int DQ2_RING = 3;
constexpr int DQ2_STAGE = DQ2_RING * 16384;            // per wave: [Q | dO | O][64][64] bf16 images of the item's rows of its head
constexpr int DQ2_ROPE = DQ2_STAGE + 4 * 3 * 8192;     // [64 queries][64] fp32 table rows, 16-B chunks XOR (row & 15)
constexpr int DQ2_LDS = DQ2_ROPE + 64 * 256;           // 160 KiB: all of a CU's LDS

// The vector instructions of a dQ unit beside its 12 MFMAs: per pair j of accumulator elements two fmas (kind 0: 2 issue slots), two
// exponentials (kinds 1, 2: 2 slots each), two multiplies (kind 3) and a packed conversion (kind 4: 1 slot): 72 slots, dealt to the 12 gaps
// by their running slot count in an order that never lets an instruction read its predecessor's result: fma j+1, exp j, exp j, multiply
// j-1, conversion j-2.  (Packed fp32 — v_pk_fma_f32, v_pk_mul_f32 — would halve the fma / multiply slots, but beside a running MFMA one
// packed instruction costs ~14 cycles against ~4.5 for a scalar one: tools/micro/mfma_gap.hip, 63 cycles per gap for 4 of them.)
struct Dq2Plan {
    int n, kind[40], pair[40], gap[40];
};
constexpr Dq2Plan dq2_make_plan() {
    Dq2Plan p{};
    int n = 0;
    auto push = [&](int kind, int j) {
        if (j < 0 || j > 7) return;
        p.kind[n] = kind;
        p.pair[n] = j;
        ++n;
    };
    push(0, 0);
    for (int j = 0; j < 10; ++j) {
        push(0, j + 1);
        push(1, j);
        push(2, j);
        push(3, j - 1);
        push(4, j - 2);
    }
    p.n = n;
    int slots = 0;
    for (int i = 0; i < n; ++i) {
        const int g = slots * 12 / 72;
        p.gap[i] = g > 11 ? 11 : g;
        slots += p.kind[i] == 4 ? 1 : 2;
    }
    return p;
}
constexpr Dq2Plan DQ2_PLAN = dq2_make_plan();

// VARLEN (round 5; DQ2_ITEMS = 0): packed rows.  The items come from a host-built PLAN (ssi_attn_plan_build): an item = (row b, 64-query block
// q0 — a multiple of 64 —, document [dstart, dend)); a block that straddles a document boundary is two items.  A workgroup walks the items of
// one GROUP of the plan (groups of equal total work: longest-processing-time assignment on the host, an item's work = its key tiles + its
// fixed cost), heaviest first, for one kv head.  An item sweeps the key tiles dstart / 64 .. q0 / 64 of ITS document (tiles of other
// documents are skipped); masked are its diagonal tile and, when the document does not start on a 64-row boundary, its first tile (keys
// < dstart) — both by the one mask  dstart <= key <= query  in a masked loop of its own in front of / behind the plain loop.  Lanes whose query
// lies outside [dstart, dend) compute on whatever their row holds and store nothing (query = lane: their columns stay their own).  RoPE
// positions are query - dstart (the plan builder checks that input_pos runs 0, 1, 2, ... inside every document).
template <int DQ2_ITEMS, bool VARLEN = false>  // query blocks per workgroup: 8, 4 or 2 (the host takes the largest that fills the chip in whole rounds)
__global__ __launch_bounds__(256, 1) void attn_bwd_dq2_kernel(const bf16_t* __restrict__ qkv, int64_t ld, const bf16_t* __restrict__ out,
                                                              const bf16_t* __restrict__ dout, const float* __restrict__ lse,
                                                              float* __restrict__ delta, bf16_t* __restrict__ dqkv,
                                                              const float* __restrict__ rope, int S, int H, int KV, int W,
                                                              const int4* __restrict__ groups, int group_stride, int table_len) {
    __shared__ __attribute__((aligned(16))) char smem[DQ2_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5;
    // workgroup -> ((batch, kv head) pair, group g of its query blocks); an XCD gets whole pairs (their K / V stay in one L2)
    int pair, g;
    const int4* gp = nullptr;  // VARLEN: this workgroup's group of the plan: [0].x = its item count, [1 ..] = the items
    if constexpr (VARLEN) {
        const int id = (int)blockIdx.x;
        pair = id % KV;  // consecutive workgroups = the kv heads of one group, i.e. (KV = 8) kv head = XCD
        g = id / KV;
        gp = groups + (int64_t)g * group_stride;
    } else {
        const int n_pairs = (int)gridDim.x / W, id = (int)blockIdx.x;
        if (n_pairs % 8 == 0) {
            const int ppx = n_pairs / 8, k = id >> 3;
            pair = (id & 7) * ppx + k / W;
            g = k % W;
        } else {
            pair = id / W;
            g = id % W;
        }
    }
    const int n_items = VARLEN ? gp[0].x : DQ2_ITEMS;
    const int kvh = pair % KV, b = VARLEN ? 0 : pair / KV;   // VARLEN: the row is the item's
    const int head = kvh * 4 + wave;
    const int64_t row0 = (int64_t)b * S, ldo = (int64_t)H * HD;
    const bf16_t* kbase = qkv + row0 * ld + (int64_t)H * HD + (int64_t)kvh * HD;
    // item i (heaviest first) -> query block: the pairs (2W-1-g, g) of the four 2W-blocks, from the top
    auto item_block = [&](int i) __attribute__((always_inline)) {
        const int u = (DQ2_ITEMS / 2 - 1) - (i >> 1);
        return u * 2 * W + ((i & 1) ? g : 2 * W - 1 - g);
    };
    // item i as (row offset of its batch row, query block, first key tile, document)
    struct Item { int64_t r0; int jq, t0, ds, de; };
    auto item_at = [&](int i) __attribute__((always_inline)) {
        Item it;
        if constexpr (VARLEN) {
            const int4 v = gp[1 + i];  // (uniform address: a scalar load)
            it.r0 = (int64_t)v.x * S, it.jq = v.y >> 6, it.t0 = v.z >> 6, it.ds = v.z, it.de = v.w;
        } else {
            it.r0 = row0, it.jq = item_block(i), it.t0 = 0, it.ds = 0, it.de = S;
        }
        return it;
    };

    KvTileDma<SWZ_DUAL, SWZ_ROW> kvdma;
    kvdma.init(kbase, ld, KV * HD, smem, wave, lane);
    // requests of a [64][64] image by one wave (see RowTileDma): per-lane source offsets for rows of stride ld (Q) and ldo (dO, O)
    unsigned vq[2], vo[2];
#pragma unroll
    for (int par = 0; par < 2; ++par) {
        const int chunk = (lane & 7) ^ (lane >> 4) ^ (4 * par);
        vq[par] = (unsigned)(((lane >> 3) * ld + chunk * 8) * 2);
        vo[par] = (unsigned)(((lane >> 3) * ldo + chunk * 8) * 2);
    }
    const char* stage = smem + DQ2_STAGE + wave * (3 * 8192);
    const unsigned stage_lds = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_c*)stage);
    // Q, dO and O rows of item block jq of this wave's head: 24 requests
    auto request_stage = [&](int64_t r0_, int jq) __attribute__((always_inline)) {
        const int64_t r = r0_ + jq * 64;
        const u32x4 rq = buffer_rsrc(qkv + r * ld + (int64_t)head * HD), rd = buffer_rsrc(dout + r * ldo + (int64_t)head * HD),
                    ro = buffer_rsrc(out + r * ldo + (int64_t)head * HD);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            dma16(stage_lds + i * 1024, vq[i & 1], rq, (unsigned)(i * 8 * ld * 2));
            dma16(stage_lds + 8192 + i * 1024, vo[i & 1], rd, (unsigned)(i * 8 * ldo * 2));
            dma16(stage_lds + 16384 + i * 1024, vo[i & 1], ro, (unsigned)(i * 8 * ldo * 2));
        }
    };
    // RoPE table rows q0 .. q0 + 63 (256 B each) of an item: 16 pieces of 4 rows, wave w the pieces w, w + 4, w + 8, w + 12; the 16-B chunk c
    // of row r lies at chunk c ^ (r & 15).  Without a table the requests read the head of qkv instead (and the store ignores them).
    const unsigned rope_lds = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_c*)(smem + DQ2_ROPE));
    const unsigned vrope = (unsigned)((lane >> 4) * 256 + (((lane & 15) ^ ((4 * wave + (lane >> 4)) & 15)) * 16));
    const u32x4 rope_rs = buffer_rsrc(rope ? (const void*)rope : (const void*)qkv);
    auto lse_of = [&](int64_t r0_, int jq, int qb) __attribute__((always_inline)) {  // lse is [B][H][S]: r0_ = b S
        return lse[(r0_ * H + (int64_t)head * S) + jq * 64 + 32 * qb + (lane & 31)];
    };

    // ---- per-tile register state ------------------------------------------------------------------------------------------------------------
    bf16x8 qf[2][4], dof[2][4];    // B operands: lane = query q0 + 32 qb + (l & 31), d = 16 ks + 8 h + j
    f32x16 pdl[2];                 // -delta of the lane's query in all 16 registers: C operand of the dP^T chain
    float nlq[2];                  // -lse * log2(e): p = exp2(S^T * log2(e) / 8 + nlq)
    int qg[2];
    f32x16 dq[2][2];
    f32x16 sacc[2], pacc[2];       // [unit parity]: S^T and dP'^T of the unit in flight
    bf16x8 rowK[2][4], rowV[2][4]; // [kb]: K / V row fragments (A operands of the S^T / dP^T products)
    s16x4 ktrh[4][2][2];           // [k-step s][db][half]: K transposed fragments (A operands of the dQ^T products); s = 2 kb, 2 kb + 1
    u32x4 dsu[2][2];               // [unit parity][s2]: dS^T of a unit as bf16 operand fragments
    unsigned ring_cur, ring_nxt, ring_n2;  // byte offsets of the slots of tiles t, t+1, t+2
    constexpr float SCALE2 = LOG2E * 0.125f;  // log2(e) / sqrt(d)

    auto tr_frag = [&](const s16x4 (&hv)[2]) __attribute__((always_inline)) {
        typedef __attribute__((ext_vector_type(8))) short s16x8;
        return __builtin_bit_cast(bf16x8, (s16x8)__builtin_shufflevector(hv[0], hv[1], 0, 1, 2, 3, 4, 5, 6, 7));
    };
    // read i (0..7) of the row fragments of key block kb of the tile at `slot`: 0-3 K, 4-7 V
    auto read_rows = [&](unsigned slot, int kb, int i) __attribute__((always_inline)) {
        const char* kt = smem + slot;
        if (i < 4) rowK[kb][i] = frag_row<SWZ_DUAL>(kt, kb * 32, i, lane);
        else rowV[kb][i - 4] = frag_row<SWZ_ROW>(kt + 8192, kb * 32, i - 4, lane);
    };
    // read i (0..7) of the transposed fragments of key block kb: k-step 2 kb + (i >> 2), db (i >> 1) & 1, half i & 1 — the order of their use
    auto read_tr = [&](unsigned slot, int kb, int i) __attribute__((always_inline)) {
        const int sI = 2 * kb + (i >> 2), db = (i >> 1) & 1;
        ktrh[sI][db][i & 1] = frag_tr_half<SWZ_DUAL>(smem + slot, sI * 16, db * 32, lane, i & 1);
    };
    // S^T / dP^T product m (0..7) of unit (kb, qb) into register set `par`: the S chain first (see sp_mfma of attn_bwd_dkv2_kernel)
    auto sp_mfma = [&](int par, int kb, int qb, int m) __attribute__((always_inline)) {
        const int ks = m & 3;
        if (m == 0) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=v"(sacc[par]) : "v"(rowK[kb][0]), "a"(qf[qb][0]));
        else if (m == 4) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %3" : "=&v"(pacc[par]) : "v"(rowV[kb][0]), "a"(dof[qb][0]), "v"(pdl[qb]));
        else if (m > 4) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(pacc[par]) : "v"(rowV[kb][ks]), "a"(dof[qb][ks]));
        else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(sacc[par]) : "v"(rowK[kb][ks]), "a"(qf[qb][ks]));
    };
    // dQ^T product i (0..3) of unit (kb, qb) whose dS^T sits in dsu[par]: k-step s2 = i >> 1 of the key block, d block i & 1
    auto dq_mfma = [&](int par, int kb, int qb, int i) __attribute__((always_inline)) {
        const int s2 = i >> 1, db = i & 1;
        asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(dq[qb][db]) : "v"(tr_frag(ktrh[2 * kb + s2][db])), "v"(dsu[par][s2]));
    };
    // exponentials of unit (kb, qb) in register set `par`, gap g of 12: the instructions DQ2_PLAN puts there
    f32x2 ev[8], dsv[8];
    float pv[16];
    // the causal mask inside a DIAGONAL 32 x 32 block (kb == qb of the diagonal tile): key row rowmap(r, h) against query column l & 31 —
    // the same 16 lane masks for every item.  Of the other two blocks of that tile, (kb 0, qb 1) is all visible and (kb 1, qb 0) all masked.
    bool beyond[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) beyond[r] = rowmap(r, h) > (lane & 31);
    int ds_item = 0;  // VARLEN: first key of the item's document
    auto sm_gap = [&](auto edge_c, int par, int kb, int qb, int k0, int gap) __attribute__((always_inline)) {
        constexpr bool EDGE = decltype(edge_c)::value;
        if (!VARLEN && EDGE && kb == 1 && qb == 0) {  // nothing visible: dS^T = 0
            if (gap == 0) dsu[par][0] = dsu[par][1] = u32x4{0u, 0u, 0u, 0u};
            return;
        }
#pragma unroll
        for (int i = 0; i < DQ2_PLAN.n; ++i) {
            if (DQ2_PLAN.gap[i] != gap) continue;
            const int j = DQ2_PLAN.pair[i], kind = DQ2_PLAN.kind[i];
            if (kind == 0) {
                ev[j][0] = fmaf(sacc[par][2 * j], SCALE2, nlq[qb]);
                ev[j][1] = fmaf(sacc[par][2 * j + 1], SCALE2, nlq[qb]);
            } else if (kind == 1 || kind == 2) {
                const int r = 2 * j + kind - 1;
                float p = __builtin_amdgcn_exp2f(ev[j][kind - 1]);
                if constexpr (VARLEN) {  // a masked tile of a packed row (the document's first or the item's diagonal): dstart <= key <= query
                    if (EDGE) {
                        const int key = k0 + 32 * kb + rowmap(r, h);
                        if (key > qg[qb] || key < ds_item) p = 0.f;
                    }
                } else if (EDGE && kb == qb && beyond[r]) p = 0.f;  // keys beyond the query contribute nothing
                pv[r] = p;
            } else if (kind == 3) {
                dsv[j][0] = pv[2 * j] * pacc[par][2 * j];  // dS^T (the 1/sqrt(d) factor is applied once at the end)
                dsv[j][1] = pv[2 * j + 1] * pacc[par][2 * j + 1];
            } else {
                dsu[par][j >> 2][j & 3] = pack_bf16(dsv[j][0], dsv[j][1]);
            }
        }
    };
    // one period: SM of unit `cur`, DQ of the unit before it, SP of the unit behind it; 8 LDS reads; optionally the ring barrier in front and
    // four LDS-DMA requests behind.  Units are (kb, qb, register set); k0 = first key of `cur`'s tile.
    struct Unit { int kb, qb, par; };
    auto period = [&](auto edge_c, auto sync_c, auto sp_c, Unit prev, Unit cur, Unit next, int k0, auto reads, auto tail, auto landed) __attribute__((always_inline)) {
        if (decltype(sync_c)::value) {
            // own requests of tile t+1 have landed (those of t+2 stay in flight) ... and everybody's; every wave is done with tile t
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            ring_barrier();
        }
#pragma unroll
        for (int m = 0; m < 12; ++m) {
            if (m < 4) dq_mfma(prev.par, prev.kb, prev.qb, m);
            else if (decltype(sp_c)::value) sp_mfma(next.par, next.kb, next.qb, m - 4);
            __builtin_amdgcn_sched_barrier(0);  // the MFMA first: the first multiply of a period reads the dP^T chain finished one MFMA ago
            sm_gap(edge_c, cur.par, cur.kb, cur.qb, k0, m);
            reads(m);
            tail(m);
            if (m == 11) landed();  // the period's 8 LDS reads (issued in gaps 0-7): ONE wait here instead of hipcc's one per first use
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // "these registers have been read": hipcc puts its s_waitcnt lgkmcnt in front, and none at the uses behind
    auto rows_landed = [&](int kb) __attribute__((always_inline)) {
        asm volatile("" ::"v"(rowK[kb][0]), "v"(rowK[kb][1]), "v"(rowK[kb][2]), "v"(rowK[kb][3]), "v"(rowV[kb][0]), "v"(rowV[kb][1]), "v"(rowV[kb][2]),
                     "v"(rowV[kb][3]));
    };
    auto tr_landed = [&](int kb) __attribute__((always_inline)) {
        asm volatile("" ::"v"(ktrh[2 * kb][0][0]), "v"(ktrh[2 * kb][0][1]), "v"(ktrh[2 * kb][1][0]), "v"(ktrh[2 * kb][1][1]), "v"(ktrh[2 * kb + 1][0][0]),
                     "v"(ktrh[2 * kb + 1][0][1]), "v"(ktrh[2 * kb + 1][1][0]), "v"(ktrh[2 * kb + 1][1][1]));
    };
    auto none = [&](int) __attribute__((always_inline)) {};
    using T_ = std::true_type;
    using F_ = std::false_type;
    const Unit U0{0, 0, 0}, U1{0, 1, 1}, U2{1, 0, 0}, U3{1, 1, 1};
    // hipcc does not know the asm statements above to be MFMAs.  Where it moves their registers itself — at the ends of the loops below — its
    // copies get no wait states: a copy reading a result still in the pipe, or an MFMA reading an accumulator register written just before it
    // (that one cost element 0 of a dQ block).  MFMA_DRAIN / MFMA_GUARD at every such place.
#define MFMA_DRAIN() asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory")
#define MFMA_GUARD() asm volatile("s_nop 7" ::: "memory")

    // -DDQ2_STAMP (debug build, tools/attn_dq_check.py stamps): cycles of wave 0 per phase of an item, summed over the workgroup's items, left
    // in the first floats of its LAST item's first dq row (the lightest block of the group) together with the 100 MHz clock's count
#ifdef DQ2_STAMP
    PhaseStamps<true, 7, true> stq;
    const unsigned long long stq_rt0 = __builtin_amdgcn_s_memrealtime();
#else
    PhaseStamps<false, 7, true> stq;
#endif
    // ---- before the first item: its rows, its lse -------------------------------------------------------------------------------------------
    // the first three key tiles of an item of nt tiles; behind the last tile the last tile is requested again (into a slot nobody reads), so
    // that the counted vmcnt waits hold without a tail case and a trip has no branch
    auto request_first_tiles = [&](int t0, int nt) __attribute__((always_inline)) {  // tiles t0 .. nt - 1
        kvdma.tile(t0, 0);
        kvdma.tile(t0 + 1 < nt ? t0 + 1 : t0, 16384);
        kvdma.tile(t0 + 2 < nt ? t0 + 2 : nt - 1, 32768);
    };
    // K / V rows of the item's batch row (VARLEN: items of one group may lie in different rows)
    auto kv_rows = [&](int64_t r0_) __attribute__((always_inline)) {
        if constexpr (VARLEN) kvdma.rs = buffer_rsrc(qkv + r0_ * ld + (int64_t)H * HD + (int64_t)kvh * HD);
    };
    float lqn[2];
    {
        const Item i0 = item_at(0);
        kv_rows(i0.r0);
        request_first_tiles(i0.t0, i0.jq + 1);
        request_stage(i0.r0, i0.jq);
        lqn[0] = lse_of(i0.r0, i0.jq, 0);
        lqn[1] = lse_of(i0.r0, i0.jq, 1);
    }

    for (int it = 0; it < n_items; ++it) {
        const Item icur = item_at(it), inxt = item_at(it + 1 < n_items ? it + 1 : it);
        const int jq = icur.jq, jn = inxt.jq;
        const int q0 = jq * 64, nt = jq + 1;  // key tiles t0 .. jq; the last one holds the diagonal
        const int64_t rw0 = icur.r0;          // row offset of the item's batch row
        if constexpr (VARLEN) ds_item = icur.ds;
        const float lq0 = lqn[0], lq1 = lqn[1];
        // everything this wave has asked for is there: the item's rows (asked for an item ago), its first three tiles (asked for in front of
        // the store of the item before), that store
        asm volatile("s_waitcnt vmcnt(0)" ::"v"(lq0), "v"(lq1) : "memory");
        stq.tick(0);
        bf16x8 oraw[2][4];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                qf[qb][ks] = frag_row<SWZ_ROW>(stage, 32 * qb, ks, lane);
                dof[qb][ks] = frag_row<SWZ_ROW>(stage + 8192, 32 * qb, ks, lane);
                oraw[qb][ks] = frag_row<SWZ_ROW>(stage + 16384, 32 * qb, ks, lane);
            }
        // in registers: the images are free for the next item's rows (this wave's own images: no barrier)
        asm volatile("s_waitcnt lgkmcnt(0)" ::"v"(oraw[1][3]), "v"(dof[1][3]), "v"(qf[1][3]) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        lqn[0] = lse_of(inxt.r0, jn, 0);
        lqn[1] = lse_of(inxt.r0, jn, 1);
        // 28 requests — the table rows of THIS item (nobody reads the old ones any more: barrier at the end of the item before) and the next
        // item's rows — dealt over the 8 steps of the delta sums: back to back, four waves' requests queue up in front of the CU's one
        // address unit (~150 cycles each where a request inside the tile loop costs 40)
        const int64_t rn = inxt.r0 + jn * 64;
        const u32x4 rq = buffer_rsrc(qkv + rn * ld + (int64_t)head * HD), rd = buffer_rsrc(dout + rn * ldo + (int64_t)head * HD),
                    ro = buffer_rsrc(out + rn * ldo + (int64_t)head * HD);
        auto request = [&](int i) __attribute__((always_inline)) {
            if (i < 4) {
                if constexpr (VARLEN) {  // table row of query q = its position q - dstart, kept inside the table for the lanes outside the document
                    const int pr = q0 - icur.ds + 4 * (wave + 4 * i) + (lane >> 4);
                    const int prc = pr < 0 ? 0 : (pr < table_len ? pr : table_len - 1);
                    dma16(rope_lds + (wave + 4 * i) * 1024, (rope ? (unsigned)prc * 256u : 0u) + (vrope & 255u), rope_rs, 0u);
                } else
                dma16(rope_lds + (wave + 4 * i) * 1024, vrope, rope_rs, (unsigned)((rope ? q0 * 256 : 0) + (wave + 4 * i) * 1024));
            } else {
                const int j = (i - 4) / 3, which = (i - 4) % 3;
                if (which == 0) dma16(stage_lds + j * 1024, vq[j & 1], rq, (unsigned)(j * 8 * ld * 2));
                else if (which == 1) dma16(stage_lds + 8192 + j * 1024, vo[j & 1], rd, (unsigned)(j * 8 * ldo * 2));
                else dma16(stage_lds + 16384 + j * 1024, vo[j & 1], ro, (unsigned)(j * 8 * ldo * 2));
            }
        };
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            qg[qb] = q0 + 32 * qb + (lane & 31);
            float dl = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
                for (int e = 0; e < 8; ++e) dl += (float)oraw[qb][ks][e] * (float)dof[qb][ks][e];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = (4 * qb + ks) * 28 / 8; i < (4 * qb + ks + 1) * 28 / 8; ++i) request(i);
                __builtin_amdgcn_sched_barrier(0);
            }
            dl += __shfl_xor(dl, 32, 64);
            // for the dK / dV kernel, which runs after this one (every (row, head) belongs to exactly one wave)
            if (h == 0) delta[(rw0 * H + (int64_t)head * S) + qg[qb]] = dl;  // (a straddled block's two items write the same values)
            nlq[qb] = -(qb ? lq1 : lq0) * LOG2E;
#pragma unroll
            for (int r = 0; r < 16; ++r) pdl[qb][r] = -dl;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {  // from here on the fragments LIVE in accumulation registers (see attn_bwd_dkv2_kernel)
                asm volatile("" : "=a"(qf[qb][ks]) : "0"(qf[qb][ks]));
                asm volatile("" : "=a"(dof[qb][ks]) : "0"(dof[qb][ks]));
            }
        }
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int db = 0; db < 2; ++db)
#pragma unroll
                for (int r = 0; r < 16; ++r) dq[qb][db][r] = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int k2 = 0; k2 < 2; ++k2) dsu[i][k2] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int sI = 0; sI < 4; ++sI)
#pragma unroll
            for (int db = 0; db < 2; ++db) ktrh[sI][db][0] = ktrh[sI][db][1] = s16x4{0, 0, 0, 0};  // the first period's dQ products add 0 * 0
        ring_cur = 0, ring_nxt = 16384, ring_n2 = 32768;
        stq.tick(1);

        // ---- tile 0 is there for everybody (each wave waited for its own pieces above): row fragments of its first key block, transposed
        // fragments of the same, S^T / dP^T of unit 0
        ring_barrier();
#pragma unroll
        for (int i = 0; i < 8; ++i) read_rows(0, 0, i);
#pragma unroll
        for (int i = 0; i < 8; ++i) read_tr(0, 0, i);
        __builtin_amdgcn_sched_barrier(0);
        MFMA_GUARD();
#pragma unroll
        for (int m = 0; m < 8; ++m) sp_mfma(0, 0, 0, m);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");

        stq.tick(2);
        int t = icur.t0;
        if constexpr (VARLEN) {
            // ---- packed rows: the document's first tile when it holds keys of the document before (dstart off the 64-row grid) and is not
            // the diagonal tile: the masked form of a full trip.  A loop of zero or one trip (see below why a loop)
            const int t_head = ((icur.ds & 63) && t + 1 < nt) ? t + 1 : t;
            for (; t < t_head; ++t) {
                const int k0 = t * 64;
                const int t3 = t + 3 < nt ? t + 3 : nt - 1;
                MFMA_GUARD();
                period(T_{}, F_{}, T_{}, U3, U0, U1, k0, [&](int m) __attribute__((always_inline)) { if (m < 8) read_rows(ring_cur, 1, m); }, none, [&]() __attribute__((always_inline)) { rows_landed(1); });
                period(T_{}, F_{}, T_{}, U0, U1, U2, k0, [&](int m) __attribute__((always_inline)) { if (m < 8) read_tr(ring_cur, 1, m); }, none, [&]() __attribute__((always_inline)) { tr_landed(1); });
                period(T_{}, T_{}, T_{}, U1, U2, U3, k0, [&](int m) __attribute__((always_inline)) { if (m < 8) read_rows(ring_nxt, 0, m); },
                       [&](int m) __attribute__((always_inline)) { if (m >= 8) kvdma.piece(t3, ring_cur, m - 8); }, [&]() __attribute__((always_inline)) { rows_landed(0); });
                period(T_{}, F_{}, T_{}, U2, U3, U0, k0, [&](int m) __attribute__((always_inline)) { if (m < 8) read_tr(ring_nxt, 0, m); }, none, [&]() __attribute__((always_inline)) { tr_landed(0); });
                const unsigned c = ring_cur;
                ring_cur = ring_nxt;
                ring_nxt = ring_n2;
                ring_n2 = c;
            }
            MFMA_DRAIN();
        }
        // ---- the unmasked tiles: t0 .. nt - 2 -----------------------------------------------------------------------------------------------
        for (; t + 1 < nt; ++t) {
            const int k0 = t * 64;
            const int t3 = t + 3 < nt ? t + 3 : nt - 1;  // (a select)
            MFMA_GUARD();
            period(F_{}, F_{}, T_{}, U3, U0, U1, k0, [&](int m) __attribute__((always_inline)) { if (m < 8) read_rows(ring_cur, 1, m); }, none, [&]() __attribute__((always_inline)) { rows_landed(1); });
            period(F_{}, F_{}, T_{}, U0, U1, U2, k0, [&](int m) __attribute__((always_inline)) { if (m < 8) read_tr(ring_cur, 1, m); }, none, [&]() __attribute__((always_inline)) { tr_landed(1); });
            period(F_{}, T_{}, T_{}, U1, U2, U3, k0, [&](int m) __attribute__((always_inline)) { if (m < 8) read_rows(ring_nxt, 0, m); },
                   [&](int m) __attribute__((always_inline)) { if (m >= 8) kvdma.piece(t3, ring_cur, m - 8); }, [&]() __attribute__((always_inline)) { rows_landed(0); });
            period(F_{}, F_{}, T_{}, U2, U3, U0, k0, [&](int m) __attribute__((always_inline)) { if (m < 8) read_tr(ring_nxt, 0, m); }, none, [&]() __attribute__((always_inline)) { tr_landed(0); });
            const unsigned c = ring_cur;
            ring_cur = ring_nxt;
            ring_nxt = ring_n2;
            ring_n2 = c;
        }
        MFMA_DRAIN();
        stq.tick(3);
        // ---- the diagonal tile, masked; no tile behind it.  Written as a second LOOP (of one trip): straight-line code here would be entered
        // from the loop above or around it, the accumulation registers of the two ways in would meet at its entry, and hipcc moves them there.
        // Two loops in sequence keep their registers (as in attn_bwd_dkv2_kernel).
        for (; t < nt; ++t) {
            const int k0 = t * 64;
            MFMA_GUARD();
            period(T_{}, F_{}, T_{}, U3, U0, U1, k0, [&](int m) __attribute__((always_inline)) { if (m < 8) read_rows(ring_cur, 1, m); }, none, [&]() __attribute__((always_inline)) { rows_landed(1); });
            period(T_{}, F_{}, F_{}, U0, U1, U2, k0, [&](int m) __attribute__((always_inline)) { if (m < 8) read_tr(ring_cur, 1, m); }, none, [&]() __attribute__((always_inline)) { tr_landed(1); });
            period(T_{}, F_{}, T_{}, U1, U2, U3, k0, none, none, [&]() __attribute__((always_inline)) {});
            period(T_{}, F_{}, F_{}, U2, U3, U0, k0, none, none, [&]() __attribute__((always_inline)) {});
        }
        MFMA_DRAIN();
#pragma unroll
        for (int i = 0; i < 4; ++i) dq_mfma(U3.par, U3.kb, U3.qb, i);
        __builtin_amdgcn_sched_barrier(0);
        MFMA_DRAIN();
        stq.tick(4);
        // ---- the store.  Every request of this wave has landed (table rows; the next item's rows; the tiles asked for beyond the last) ...
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ring_barrier();  // ... and every other wave's pieces of the table rows
        f32x4 rcs[2][2][4];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            const int q = 32 * qb + (lane & 31);
#pragma unroll
            for (int db = 0; db < 2; ++db)
#pragma unroll
                for (int gg = 0; gg < 4; ++gg)
                    rcs[qb][db][gg] = *reinterpret_cast<const f32x4*>(smem + DQ2_ROPE + q * 256 + (((8 * db + 2 * gg + h) ^ (q & 15)) * 16));
        }
        // everybody has its table rows in registers and is done with the ring: the next item's requests may overwrite both
        ring_barrier();
        kv_rows(inxt.r0);
        request_first_tiles(inxt.t0, jn + 1);  // (behind the last item: its own once more — waited for at the end of the kernel)
        stq.tick(5);
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            bf16_t* drow = dqkv + (rw0 + qg[qb]) * ld + (int64_t)head * HD;
            const bool mine = !VARLEN || (qg[qb] >= icur.ds && qg[qb] < icur.de);  // packed rows: queries of other documents are other items'
#pragma unroll
            for (int db = 0; db < 2; ++db)
#pragma unroll
                for (int gg = 0; gg < 4; ++gg) {
                    bf16x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (bf16_t)(dq[qb][db][4 * gg + e] * 0.125f);
                    // rope != NULL: the gradient leaves in pre-RoPE space (backward of the rotation fused here, saves a pass over dqkv)
                    if (rope) v = unrope4(v, rcs[qb][db][gg]);
                    if (mine) *reinterpret_cast<bf16x4*>(drow + db * 32 + 8 * gg + 4 * h) = v;
                }
        }
        stq.tick(6);
#ifdef DQ2_STAMP
        if (it == n_items - 1 && wave == 0) {  // DEBUG BUILD ONLY: overwrites the first floats of the item's first dq row
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0) {
                float* dbg = reinterpret_cast<float*>(dqkv + (rw0 + q0) * ld + (int64_t)head * HD);
                for (int i = 0; i < 7; ++i) dbg[i] = (float)stq.total[i];
                dbg[7] = (float)(__builtin_readcyclecounter() - stq.begin);
                dbg[8] = (float)(__builtin_amdgcn_s_memrealtime() - stq_rt0);
                dbg[9] = (float)g;
            }
        }
#endif
    }
    // The last item asked for its own rows once more (landed before its store) — and for its first three tiles once more, in front of its
    // store: nothing of this workgroup may be in flight towards LDS when it ends (the LDS goes to the next workgroup on this CU).
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace

// The dQ pass of ssi_attn_bwd_mfma: ORs the SSI_ATTN_USED_* bits of its choice into *used.  selq = the mode of ssi_set_attn_impl(SSI_ATTN_KERNEL_DQ)
static int attn_bwd_dq_launch(const AttnBwdArgs& a, int selq, int* used) {
    const auto& [qkv, ld, out, dout, lse, dqkv, delta, doc_start, doc_end, rope, table_len, positions, batch, seq, n_heads, n_kv, workspace,
                 workspace_bytes, plan_dev, ph, st] = a;  // (ph: the plan's header on the host, validated by ssi_attn_bwd_mfma; NULL: no plan)
    const int rep = n_heads / n_kv, qpw = ANW / rep;
    // dQ: the pipelined one-wave-per-SIMD kernel (persistent workgroups of 8, 4 or 2 query blocks: the largest count whose workgroups fill
    // the chip in whole rounds of 256, or in many rounds) for plain causal rows of 4 query heads per kv head; ssi_set_attn_impl(DQ, OLD)
    // keeps the round-1..3 kernel, NEW forces this one (8 blocks per workgroup if S allows, else 4, 2) whatever the fill
    int dq2_items = 0;
    if (!doc_start && !positions && rep == 4 && seq % 128 == 0 && selq != SSI_ATTN_MODE_OLD) {
        const int64_t nqb = seq / 64;
        for (int it = 8; it >= 2 && !dq2_items; it >>= 1) {
            if (nqb % it) continue;
            const int64_t grid = batch * n_kv * (nqb / it);
            if (grid % 256 == 0 || grid >= 1024) dq2_items = it;
        }
        if (!dq2_items && selq == SSI_ATTN_MODE_NEW) dq2_items = nqb % 8 == 0 ? 8 : nqb % 4 == 0 ? 4 : 2;
    }
    if (ph && selq != SSI_ATTN_MODE_OLD) {
        hipLaunchKernelGGL((attn_bwd_dq2_kernel<0, true>), dim3((unsigned)(ph[PLAN_W_N_DQ_GROUPS] * n_kv)), dim3(256), 0, st, (const bf16_t*)qkv, ld, (const bf16_t*)out,
                           (const bf16_t*)dout, lse, delta, (bf16_t*)dqkv, rope, (int)seq, n_heads, n_kv, 0,
                           reinterpret_cast<const int4*>(plan_dev + ph[PLAN_W_DQ_OFF]), ph[PLAN_W_DQ_GROUP_WORDS] / PLAN_DQ_ITEM_WORDS, (int)std::min<int64_t>(table_len, 1 << 30));
        *used |= SSI_ATTN_USED_DQ2 | SSI_ATTN_USED_PLAN;
    } else if (dq2_items) {
        const int w = (int)(seq / 64 / dq2_items);
        const dim3 grid((unsigned)(batch * n_kv * w));
        auto kern = dq2_items == 8 ? attn_bwd_dq2_kernel<8> : dq2_items == 4 ? attn_bwd_dq2_kernel<4> : attn_bwd_dq2_kernel<2>;
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, (const bf16_t*)qkv, ld, (const bf16_t*)out, (const bf16_t*)dout, lse, delta, (bf16_t*)dqkv,
                           rope, (int)seq, n_heads, n_kv, w, (const int4*)nullptr, 0, 0);
        *used |= SSI_ATTN_USED_DQ2 | (dq2_items << 8);
    }
    else
        hipLaunchKernelGGL(attn_bwd_dq_kernel, dim3((unsigned)(batch * n_kv * (seq / (32 * qpw)))), dim3(64 * ANW), 0, st, (const bf16_t*)qkv,
                           ld, (const bf16_t*)out, (const bf16_t*)dout, lse, delta, (bf16_t*)dqkv, doc_start, rope, positions, (int)seq, n_heads, n_kv);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}
