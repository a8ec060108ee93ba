// Edit distance with substitution / deletion / insertion counts between spans of int32 ids (ssi_edit_distance; the definition is in
// include/ssi_hip.h).  One wave per pair, four waves per workgroup (as seq_score_reduce_kernel).
//
// Layout.  The hypothesis columns are dealt to the 64 lanes in strips of C = SSI_EDIT_COLS columns: lane l of column block b owns the columns
// 64 C b + C l + 1 .. + C, the current row of them in C registers indexed at compile time only.  The reference rows move through the lanes
// as a wavefront: at step t lane l works on row t - l.  What it needs from its left neighbour — the cell (row, last column of lane l - 1),
// which that lane finished at step t - 1 — arrives by one cross-lane move per step; the same cell of the step before is the diagonal of
// the strip's first column.  The reference id of the row travels down the lanes the same way, so only lane 0 reads ids: 64 at a time,
// one coalesced load per 64 steps, issued one chunk ahead.  A hypothesis longer than 64 C columns runs in column blocks; the last column
// of a block (one cell per row, written by lane 63) stays in LDS for lane 0 of the next block, in place: a row's slot is read (a chunk
// of 64 rows ahead of use) before the new block's lane 63 reaches it 63 steps later, and LDS operations of one wave complete in order.
//
// A cell is ONE register: cost << 16 | S (both <= SSI_EDIT_MAX_LEN = 4096).  D and I are not carried: every cell (i, j) is the end of
// an alignment path with i = hits + S + D and j = hits + S + I, so D - I = i - j and D + I = cost - S give both at the end.  "Strictly
// lower cost" on packed cells a, b is (a | 0xffff) < b: true iff cost(a) < cost(b), whatever the S fields hold.  Integer arithmetic only,
// no atomics, no scratch; the cell update is compares and selects.  A pair's result depends on its two spans alone.
#include "common_hip.h"

namespace {

constexpr int C = SSI_EDIT_COLS;
constexpr int BLOCK_COLS = 64 * C;

// MULTI: hypotheses of more than one column block (the boundary column in LDS, 16 KiB per wave).  The host launches the other form
// whenever max_len <= 64 C, so that the common short case holds no LDS and runs at full occupancy.
template <bool MULTI>
__global__ __launch_bounds__(256) void edit_distance_kernel(const int32_t* __restrict__ tokens, int64_t n_tokens,
                                                            const int64_t* __restrict__ ref_start, const int32_t* __restrict__ ref_len,
                                                            const int64_t* __restrict__ hyp_start, const int32_t* __restrict__ hyp_len,
                                                            int64_t n_pairs, int max_len, int32_t* __restrict__ out) {
    __shared__ int boundary[MULTI ? 4 : 1][MULTI ? SSI_EDIT_MAX_LEN : 1];
    const int ln = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // the pair and its loop bounds in SGPRs
    const int64_t pair = (int64_t)blockIdx.x * 4 + wv;
    if (pair >= n_pairs) return;  // wave-uniform
    const int64_t rs = ref_start[pair], hs = hyp_start[pair];
    const int m = ref_len[pair], n = hyp_len[pair];
    int32_t* o = out + 4 * pair;
    // the span check comes before any address is formed from a span (all of it wave-uniform)
    const bool bad = m < 0 || n < 0 || m > max_len || n > max_len || rs < 0 || hs < 0 || rs > n_tokens - m || hs > n_tokens - n;
    if (bad) {
        if (ln < 4) o[ln] = -1;
        return;
    }
    if (m == 0 || n == 0) {  // row 0 is (j, 0, 0, j), column 0 is (i, 0, i, 0)
        if (ln == 0) {
            o[0] = m + n; o[1] = 0; o[2] = m; o[3] = n;
        }
        return;
    }
    const int32_t* ref = tokens + rs;
    const int32_t* hyp = tokens + hs;
    int* bnd = boundary[MULTI ? wv : 0];

    const int n_blocks = MULTI ? (n + BLOCK_COLS - 1) / BLOCK_COLS : 1;
    int row[C];
    for (int blk = 0; blk < n_blocks; ++blk) {
        const int j0 = blk * BLOCK_COLS;                                    // the column left of the block
        const int cols = min(n - j0, BLOCK_COLS);                           // 1 .. 64 C
        const int lanes = (cols + C - 1) / C;                               // lanes that hold a live column
        const bool store_boundary = MULTI && blk + 1 < n_blocks;            // then cols == 64 C and lane 63 is live
        int h[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int j = j0 + ln * C + c;                                  // 0-based hypothesis index of the column
            h[c] = j < n ? hyp[j] : 0;
            row[c] = (j + 1) << 16;                                         // row 0: cost j, S 0
        }
        int prev_in = j0 << 16;                                             // lane 0's diagonal of row 1; lanes > 0 receive theirs
        int tok = 0;
        const int steps = m + lanes - 1;
        // 64 reference ids (and boundary cells) per chunk, lane l holding the one of row chunk + l + 1; the next chunk is asked for now
        int ids_next = ln < m ? ref[ln] : 0;
        int cells_next = (MULTI && blk > 0 && ln < m) ? bnd[ln] : 0;
        for (int chunk = 0; chunk < steps; chunk += 64) {
            const int ids = ids_next, cells = cells_next;
            const int ahead = chunk + 64 + ln;
            ids_next = ahead < m ? ref[ahead] : 0;
            cells_next = (MULTI && blk > 0 && ahead < m) ? bnd[ahead] : 0;
            const int k_end = min(64, steps - chunk);
            for (int k = 0; k < k_end; ++k) {
                const int t = chunk + k + 1;                                // step; lane l is on row t - l
                const int i = t - ln;
                // lane 0: column j0 of row t — (t, 0, t, 0) in the first block, the stored boundary otherwise — and the id of row t
                const int id0 = __builtin_amdgcn_readlane(ids, k);
                const int cell0 = (MULTI && blk > 0) ? __builtin_amdgcn_readlane(cells, k) : (t << 16);
                const int from_left = __shfl_up(row[C - 1], 1, 64);
                const int tok_left = __shfl_up(tok, 1, 64);
                const int in = ln == 0 ? cell0 : from_left;
                tok = ln == 0 ? id0 : tok_left;
                if (i >= 1 && i <= m) {
                    int diag = prev_in, left = in;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const int up = row[c];
                        int best = diag + (tok != h[c] ? 0x10001 : 0);      // 1. the diagonal: + 0 on a hit, else + 1 cost and + 1 S
                        const int u = up + 0x10000;                         // 2. up: + 1 cost (a deletion)
                        best = (u | 0xffff) < best ? u : best;
                        const int l = left + 0x10000;                       // 3. left: + 1 cost (an insertion)
                        best = (l | 0xffff) < best ? l : best;
                        row[c] = best;
                        diag = up;
                        left = best;
                    }
                    if (store_boundary && ln == 63) bnd[i - 1] = row[C - 1];
                }
                prev_in = in;
            }
        }
    }
    // the cell (m, n): in the last block, column n - j0 of the block
    const int last = n - (n_blocks - 1) * BLOCK_COLS - 1;                    // 0-based column inside the last block
    int cell = row[0];
#pragma unroll
    for (int c = 1; c < C; ++c) cell = (last % C == c) ? row[c] : cell;
    if (ln == last / C) {
        const int dist = cell >> 16, s = cell & 0xffff;
        const int d = (dist - s + m - n) / 2;                               // D - I = m - n, D + I = dist - S
        o[0] = dist; o[1] = s; o[2] = d; o[3] = dist - s - d;
    }
}

}  // namespace

extern "C" size_t ssi_edit_distance_workspace_bytes(int64_t n_pairs, int32_t max_len) {
    (void)n_pairs; (void)max_len;
    return 0;  // the boundary column between two column blocks lives in LDS
}

extern "C" int ssi_edit_distance(const int32_t* tokens, int64_t n_tokens, const int64_t* ref_start, const int32_t* ref_len,
                                 const int64_t* hyp_start, const int32_t* hyp_len, int64_t n_pairs, int32_t max_len, int32_t* out,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace;
    SSI_CHECK_ARG(n_tokens >= 0 && n_pairs >= 0 && n_pairs < (1LL << 31) && max_len >= 0 && (n_tokens == 0 || tokens) &&
                  (n_pairs == 0 || (ref_start && ref_len && hyp_start && hyp_len && out)));
    if (max_len > SSI_EDIT_MAX_LEN) {
        ssi_set_error("ssi_edit_distance: max_len %d above SSI_EDIT_MAX_LEN %d", (int)max_len, SSI_EDIT_MAX_LEN);
        return SSI_ERR_UNSUPPORTED;
    }
    if (workspace_bytes < ssi_edit_distance_workspace_bytes(n_pairs, max_len)) {
        ssi_set_error("ssi_edit_distance: workspace of %zu bytes is too small", workspace_bytes);
        return SSI_ERR_WORKSPACE;
    }
    if (n_pairs == 0) return SSI_OK;
    const dim3 grid((unsigned)ssi_cdiv(n_pairs, 4)), block(256);
    if (max_len <= BLOCK_COLS)
        hipLaunchKernelGGL(edit_distance_kernel<false>, grid, block, 0, (hipStream_t)stream, tokens, n_tokens, ref_start, ref_len, hyp_start,
                           hyp_len, n_pairs, (int)max_len, out);
    else
        hipLaunchKernelGGL(edit_distance_kernel<true>, grid, block, 0, (hipStream_t)stream, tokens, n_tokens, ref_start, ref_len, hyp_start,
                           hyp_len, n_pairs, (int)max_len, out);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}
