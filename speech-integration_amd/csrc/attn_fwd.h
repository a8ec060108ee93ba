// Forward of the MFMA flash attention (attn_mfma.h: orientation and shared helpers): attn_fwd_kernel and its launch.
// Part of the translation unit attention_mfma.hip, which includes it once.
#pragma once
#include "attn_mfma.h"

namespace {

constexpr float RESCALE_TAU = 5.545177444479562f;  // 8 ln 2

// =====================================================================================================================
// forward
// =====================================================================================================================
// grid.x = B * KV * (S / (32 * QPW)),  QPW = ANW / rep q-blocks per workgroup; wave w: head kvh*rep + w % rep, q-block w / rep
__global__ __launch_bounds__(64 * ANW, ANW == 8 ? 1 : 2) void attn_fwd_kernel(const bf16_t* __restrict__ qkv, int64_t ld, bf16_t* __restrict__ out,
                                                       float* __restrict__ lse, const int32_t* __restrict__ doc_start, int S, int H,
                                                       int KV) {
    __shared__ __attribute__((aligned(16))) char smem[3 * 2 * 8192];  // ring of 3 x [K | V][64][64] bf16
    TRACE_BEGIN();
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rep = H / KV, qpw = ANW / rep;
    const int nqb = S / (32 * qpw);
    // heavy q-blocks first
    int rank_, pair_;
    block_to_work(nqb, (int)(gridDim.x / nqb), rank_, pair_);
    const int qgrp = nqb - 1 - rank_;
    const int kvh = pair_ % KV;
    const int b = pair_ / KV;
    const int head = kvh * rep + wave % rep;
    const int q0 = (qgrp * qpw + wave / rep) * 32;
    const int q_last_wg = (qgrp * qpw + qpw - 1) * 32 + 31;
    const int nt = q_last_wg / 64 + 1;
    const int h = lane >> 5;
    const int64_t row0 = (int64_t)b * S;
    const bf16_t* kbase = qkv + row0 * ld + (int64_t)H * HD + (int64_t)kvh * HD;
    // packed rows: a query sees keys doc_start <= key <= query.  doc_start is non-decreasing along a row, so the first key
    // tile any row of the workgroup / wave needs, and whether a tile needs the document mask, follow from the end rows.
    const int qg_ = q0 + (lane & 31);
    const int ds = doc_start ? doc_start[row0 + qg_] : 0;                       // this lane's query
    const int ds_lo = doc_start ? doc_start[row0 + q0] : 0;                     // first row of the wave
    const int ds_hi = doc_start ? doc_start[row0 + q0 + 31] : 0;                // last row of the wave
    const int t_first = doc_start ? doc_start[row0 + qgrp * qpw * 32] / 64 : 0;  // first tile of the workgroup

    // Q as the B operand of S^T = K Q^T, pre-scaled by 1/sqrt(64) = 2^-3 (exact in bf16)
    bf16x8 qf[4];
    {
        const bf16_t* qrow = qkv + (row0 + q0 + (lane & 31)) * ld + (int64_t)head * HD + 8 * h;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = scale_frag(*reinterpret_cast<const bf16x8*>(qrow + 16 * ks), 0.125f);
    }
    f32x16 oacc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
    float m = -INFINITY, lsum = 0.f;  // reference max (scaled-score units) and this half-wave's partial row sum
    float mb = 0.f;                   // m in exp2 units (0 while the row has seen no key)
    const int qg = q0 + (lane & 31);

    // ring of 3 tile slots filled by LDS-DMA two tiles ahead (4 requests per wave per tile)
    KvTileDma<SWZ_ROW, SWZ_TR> kvdma;
    kvdma.init(kbase, ld, KV * HD, smem, wave, lane);
    kvdma.tile(t_first, 0);
    if (t_first + 1 < nt) kvdma.tile(t_first + 1, 16384);
    auto tile_step = [&](int t, auto buf_c) {
        constexpr int BUF = decltype(buf_c)::value;  // compile-time ring slot: LDS addresses = hoisted lane base + immediate
        const char* kt = smem + BUF * 16384;
        const char* vt = kt + 8192;
        if (t + 1 < nt) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * ANP) : "memory");  // own pieces of tile t landed (tile t+1 may fly)
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ring_barrier();  // everybody's pieces landed; the slot of tile t-1 is free again
        if (t + 2 < nt) kvdma.tile(t + 2, ((BUF + 2) % 3) * 16384);
        const int k0 = t * 64;
        if (k0 <= q0 + 31 && k0 + 63 >= ds_lo) {  // wave-uniform: this tile intersects the visible range of the wave's rows
            // All 8 K fragments are requested before the first product and all 16 V fragments right behind the S^T products (they land
            // under the softmax).  Left to itself the compiler reads each fragment into the same registers right in front of its MFMA
            // (read, lgkmcnt(0), MFMA, read, ...), which exposes the LDS latency once per MFMA.
            bf16x8 kfr[2][4];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) kfr[kb][ks] = frag_row<SWZ_ROW>(kt, kb * 32, ks, lane);
            __builtin_amdgcn_sched_barrier(0);
            f32x16 sacc[2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) sacc[kb][r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[kb][ks], qf[ks], sacc[kb], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            bf16x8 vfr[4][2];
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int db = 0; db < 2; ++db) vfr[s][db] = frag_tr<SWZ_TR>(vt, s * 16, db * 32, lane);
            __builtin_amdgcn_sched_barrier(0);
            if (k0 + 63 > q0 || k0 < ds_hi) {  // edge tile: mask keys beyond the query or before its document
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = k0 + kb * 32 + rowmap(r, h);
                        if (key > qg || key < ds) sacc[kb][r] = -INFINITY;
                    }
            }
            float mx = sacc[0][0];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[kb][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            // Deferred rescale: the reference maximum m of a row moves only when the tile's maximum exceeds it by more than
            // RESCALE_TAU, and then for the whole wave at once (wave-uniform branch), so most tiles skip the 32 multiplies of O^T and the
            // extra exponential.  With a stale m the probabilities of a tile are at most e^TAU = 256 instead of 1: same relative precision in
            // bf16, sums and O^T in fp32, and out = O / l, lse = m + log l do not depend on which m was used.
            if (__builtin_amdgcn_ballot_w64(mx > m + RESCALE_TAU) != 0) {
                const float mn = fmaxf(m, mx);
                // a row whose document starts after this tile has seen no key yet (m = mn = -inf): keep its state finite
                const float mref = mn == -INFINITY ? 0.f : mn;
                const float alpha = __builtin_amdgcn_exp2f((m - mref) * LOG2E);
                mb = mref * LOG2E;
                lsum *= alpha;
                m = mn;
#pragma unroll
                for (int db = 0; db < 2; ++db)
#pragma unroll
                    for (int r = 0; r < 16; ++r) oacc[db][r] *= alpha;
            }
            float rs = 0.f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = __builtin_amdgcn_exp2f(sacc[kb][r] * LOG2E - mb);
                    sacc[kb][r] = p;
                    rs += p;
                }
            lsum += rs;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const bf16x8 pf = acc_frag(sacc[s >> 1], s & 1);
#pragma unroll
                for (int db = 0; db < 2; ++db)
                    oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfr[s][db], pf, oacc[db], 0, 0, 0);
            }
        }
    };
    TRACE_LOOP_BEGIN();
    for (int t = t_first; t < nt; t += 3) {
        tile_step(t, std::integral_constant<int, 0>{});
        if (t + 1 < nt) tile_step(t + 1, std::integral_constant<int, 1>{});
        if (t + 2 < nt) tile_step(t + 2, std::integral_constant<int, 2>{});
    }
    TRACE_LOOP_END();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the last tile's wait left nothing in flight towards LDS; once more on every path: kernel_lint R3)
    const float ltot = lsum + __shfl_xor(lsum, 32, 64);
    const float inv = 1.f / ltot;
    bf16_t* orow = out + (row0 + qg) * ((int64_t)H * HD) + (int64_t)head * HD;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bf16x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (bf16_t)(oacc[db][4 * g + e] * inv);
            *reinterpret_cast<bf16x4*>(orow + db * 32 + 8 * g + 4 * h) = v;
        }
    if (h == 0) lse[((int64_t)b * H + head) * S + qg] = m + logf(ltot);
    TRACE_END(0, nt - t_first);
}

}  // namespace

int ssi_attn_fwd_mfma(const void* qkv, int64_t ld, void* out, float* lse, const int32_t* doc_start, int64_t batch, int64_t seq,
                      int n_heads, int n_kv, void* stream) {
    const int rep = n_heads / n_kv, qpw = ANW / rep;
    const unsigned grid = (unsigned)(batch * n_kv * (seq / (32 * qpw)));
    hipLaunchKernelGGL(attn_fwd_kernel, dim3(grid), dim3(64 * ANW), 0, (hipStream_t)stream, (const bf16_t*)qkv, ld, (bf16_t*)out, lse,
                       doc_start, (int)seq, n_heads, n_kv);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}
