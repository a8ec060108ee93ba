// Byte-pair encoding over discrete speech units: the trainer's kernels and the encoder (ssi_bpe_*; the definition is in include/ssi_hip.h).
//
// Trainer.  Everything a merge needs lives on the device: the ids in two buffers that swap roles per merge, the dense pair-count table
// uint32[v_cap x v_cap], the merge list, and the state words (done, merges made, the current pair, n_bad, the two lengths).  One merge m is
// five launches, and the kernel boundary is the only synchronisation between workgroups:
//   bpe_best_partial_kernel   the 64-bit maximum of count << 32 | ~(a v_cap + b) over the (n_base + m)^2 live entries, one partial per workgroup
//   bpe_best_final_kernel     the maximum of the partials; stop (done = 1) or record (a, b, count) in the state and the merge list
//   bpe_mark_kernel           per tile of SSI_BPE_TILE ids: the last break of a run of a (for a == b), the positions dropped under either parity
//   bpe_scan_kernel           one workgroup: prefix maximum of the breaks and, with the parity that gives, prefix sum of the kept positions
//   bpe_apply_kernel          per tile: close up into the other buffer and update the counts of the pairs beside a merged window
// After done every kernel returns at once, so the host may launch ahead and read the state back at a cadence.
//
// Which positions merge.  d(i) ("dropped") says that position i is the second id of a merged pair; position i starts a merge iff d(i + 1).
//   a != b: d(i) = x[i-1] == a && x[i] == b                                   (two such windows cannot overlap)
//   a == b: d(i) = x[i-1] == a && x[i] == a && (i - r(i)) odd,  r(i) = the start of the run of a that holds i
// r(i) is the inclusive prefix maximum of p(j) = (x[j] != a ? j + 1 : 0): a tile knows it for every position behind its first break and
// takes the carry of the tiles before it (0: the run began at position 0) for the rest.  Only the parity of the carry decides what the
// leading run of a tile drops, so the mark kernel counts both cases and the scan kernel picks.
//
// Counts.  A pair is owned by its right-hand position.  A kept position i (new value v = d(i+1) ? z : x[i], new left neighbour
// L = d(i-1) ? z : x[i-1]) changes its pair iff d(i-1) or d(i+1): then (x[i-1], x[i]) loses one and (L, v) gains one.  Dropped positions own
// occurrences of (a, b) only, and after the merge no (a, b) is left, so that one entry is set to zero by the scan kernel and never
// subtracted from: the hottest address of the table gets no atomic at all.  Adds to equal addresses are combined within the wave first.
// Integer adds commute: the table is exact and the same bytes in every run.
#include "common_hip.h"

namespace {

constexpr int TILE = SSI_BPE_TILE;
constexpr int TPB = 256;
constexpr int IPT = TILE / TPB;  // ids per thread, contiguous
constexpr int SEP = SSI_BPE_SEP;
constexpr int NONE = 0x7fffffff;  // "no merge here" among ranks
constexpr int MAX_PARTIALS = 2048;
constexpr int SCAN_THREADS = 1024;
static_assert(IPT == 16, "the LDS padding below is one word per 16");

// LDS index of tile element j: one pad word per 16, so that 64 lanes reading elements 16 apart hit 64 banks' worth of distinct words
__device__ __forceinline__ int P(int j) { return j + (j >> 4); }

__device__ __forceinline__ bool is_id(int s, int below) { return (unsigned)s < (unsigned)below; }

// table[idx] += delta for the active lanes, equal addresses of the wave combined into one atomic.  Call from converged code.
__device__ __forceinline__ void bpe_wave_add(uint32_t* table, uint32_t idx, uint32_t delta, bool active) {
    unsigned long long todo = __ballot(active);
    const int ln = threadIdx.x & 63;
    while (todo) {  // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t lidx = (uint32_t)__shfl((int)idx, leader, 64);
        const unsigned long long same = __ballot(active && idx == lidx);  // holds the leader
        if (ln == leader) atomicAdd(table + lidx, delta * (uint32_t)__popcll(same));
        todo &= ~same;
    }
}

// exclusive block scan of non-negative ints (0 is the identity of both forms); `red` holds one int per wave; every thread gets the total
template <bool MAX> __device__ __forceinline__ int bpe_op(int a, int b) { return MAX ? max(a, b) : a + b; }
template <bool MAX> __device__ __forceinline__ int bpe_block_scan(int v, int* red, int& total) {
    const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (ln >= o) inc = bpe_op<MAX>(inc, t);
    }
    __syncthreads();  // `red` may still be read by a scan before this one
    if (ln == 63) red[wv] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < nw; ++w) {
        const int t = red[w];
        if (w < wv) base = bpe_op<MAX>(base, t);
        tot = bpe_op<MAX>(tot, t);
    }
    total = tot;
    int exc = __shfl_up(inc, 1, 64);
    if (ln == 0) exc = 0;
    return bpe_op<MAX>(base, exc);
}

__device__ __forceinline__ unsigned long long bpe_wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}

// the length of the buffer that merge m reads, never above the buffers' capacity
__device__ __forceinline__ int64_t bpe_len(const int32_t* state, int m, int64_t n_cap) {
    const int64_t n = state[SSI_BPE_ST_LEN + (m & 1)];
    return n < 0 ? 0 : (n > n_cap ? n_cap : n);
}

// ---- full count ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void bpe_pair_count_kernel(const int32_t* __restrict__ ids, int64_t n, int V, int stride,
                                                            uint32_t* __restrict__ table, int32_t* __restrict__ n_bad) {
    const int64_t threads = (int64_t)gridDim.x * TPB;
    const int64_t rounds = (n + threads - 1) / threads;  // the same for every lane: the ballots below are converged
    const int ln = threadIdx.x & 63;
    for (int64_t r = 0; r < rounds; ++r) {
        const int64_t i = r * threads + (int64_t)blockIdx.x * TPB + threadIdx.x;
        const bool in = i < n;
        const int s = in ? ids[i] : SEP;
        const int p = (in && i > 0) ? ids[i - 1] : SEP;
        const bool pair = is_id(s, V) && is_id(p, V);  // checked before the address is formed
        bpe_wave_add(table, pair ? (uint32_t)p * (uint32_t)stride + (uint32_t)s : 0u, 1u, pair);
        if (n_bad) {
            const unsigned long long bad = __ballot(in && s != SEP && !is_id(s, V));
            if (bad && ln == 0) atomicAdd(n_bad, (int)__popcll(bad));
        }
    }
}

// copy with every id outside [0, V) replaced by the separator; the replaced ones that were not separators are counted
__global__ __launch_bounds__(TPB) void bpe_sanitise_kernel(const int32_t* __restrict__ ids, int64_t n, int V, int32_t* __restrict__ dst,
                                                          int32_t* __restrict__ n_bad) {
    const int64_t threads = (int64_t)gridDim.x * TPB;
    const int64_t rounds = (n + threads - 1) / threads;
    const int ln = threadIdx.x & 63;
    for (int64_t r = 0; r < rounds; ++r) {
        const int64_t i = r * threads + (int64_t)blockIdx.x * TPB + threadIdx.x;
        const bool in = i < n;
        const int s = in ? ids[i] : SEP;
        if (in) dst[i] = is_id(s, V) ? s : SEP;
        const unsigned long long bad = __ballot(in && s != SEP && !is_id(s, V));
        if (bad && ln == 0) atomicAdd(n_bad, (int)__popcll(bad));
    }
}

__global__ void bpe_state_init_kernel(int32_t* state, int32_t n) {
    if (threadIdx.x < SSI_BPE_STATE_WORDS) state[threadIdx.x] = (threadIdx.x == SSI_BPE_ST_LEN) ? n : 0;
}

// ---- best pair -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void bpe_best_partial_kernel(const uint32_t* __restrict__ table, int v_cur, int stride,
                                                              const int32_t* __restrict__ state, unsigned long long* __restrict__ partial) {
    __shared__ unsigned long long red[TPB / 64];
    if (state[SSI_BPE_ST_DONE]) return;
    unsigned long long best = 0;
    for (int a = blockIdx.x; a < v_cur; a += gridDim.x) {
        const uint32_t* row = table + (size_t)a * stride;
        const uint32_t base = (uint32_t)a * (uint32_t)stride;
        for (int b = threadIdx.x; b < v_cur; b += TPB) {
            const unsigned long long key = ((unsigned long long)row[b] << 32) | (uint32_t)~(base + (uint32_t)b);
            best = key > best ? key : best;
        }
    }
    best = bpe_wave_max_u64(best);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < TPB / 64; ++w) best = red[w] > best ? red[w] : best;
        partial[blockIdx.x] = best;
    }
}

__global__ __launch_bounds__(TPB) void bpe_best_final_kernel(const unsigned long long* __restrict__ partial, int n_partial, int stride, int m,
                                                            int min_frequency, int32_t* __restrict__ state, int32_t* __restrict__ merges) {
    __shared__ unsigned long long red[TPB / 64];
    if (state[SSI_BPE_ST_DONE]) return;
    unsigned long long best = 0;
    for (int i = threadIdx.x; i < n_partial; i += TPB) best = partial[i] > best ? partial[i] : best;
    best = bpe_wave_max_u64(best);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < TPB / 64; ++w) best = red[w] > best ? red[w] : best;
        const uint32_t count = (uint32_t)(best >> 32), idx = ~(uint32_t)best;
        if (count < (uint32_t)min_frequency) {
            state[SSI_BPE_ST_DONE] = 1;
        } else {
            const int a = (int)(idx / (uint32_t)stride), b = (int)(idx % (uint32_t)stride);
            state[SSI_BPE_ST_A] = a;
            state[SSI_BPE_ST_B] = b;
            state[SSI_BPE_ST_COUNT] = (int32_t)count;
            state[SSI_BPE_ST_M] = m + 1;
            merges[3 * m] = a;
            merges[3 * m + 1] = b;
            merges[3 * m + 2] = (int32_t)count;
        }
    }
}

// ---- one tile of a merge ---------------------------------------------------------------------------------------------------------------
// The tile in LDS: s_ids[P(j)] = x[t0 + j] (SEP at and beyond n), s_halo = {x[t0-2], x[t0-1], x[t0+TILE]} (SEP outside the buffer).
__device__ __forceinline__ void bpe_load_tile(const int32_t* __restrict__ src, int64_t n, int64_t t0, int* s_ids, int* s_halo) {
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        const int j = k * TPB + threadIdx.x;
        const int64_t i = t0 + j;
        s_ids[P(j)] = i < n ? src[i] : SEP;
    }
    if (threadIdx.x < 3) {
        const int64_t i = threadIdx.x == 2 ? t0 + TILE : t0 - 2 + threadIdx.x;
        s_halo[threadIdx.x] = (i >= 0 && i < n) ? src[i] : SEP;
    }
    __syncthreads();
}

// what one thread sees of it: its IPT ids, the two before and the one behind
struct BpeWindow {
    int l2, l1, rt;
};
__device__ __forceinline__ BpeWindow bpe_read_window(const int* s_ids, const int* s_halo, int (&c)[IPT]) {
    const int j0 = threadIdx.x * IPT;
#pragma unroll
    for (int k = 0; k < IPT; ++k) c[k] = s_ids[P(j0 + k)];
    BpeWindow w;
    w.l1 = j0 > 0 ? s_ids[P(j0 - 1)] : s_halo[1];
    w.l2 = j0 > 0 ? s_ids[P(j0 - 2)] : s_halo[0];
    w.rt = j0 + IPT < TILE ? s_ids[P(j0 + IPT)] : s_halo[2];
    return w;
}

// the thread's last break of a run of a: max of p(j) over its ids (0: none); positions at and beyond n are left out, so p <= n < 2^31
__device__ __forceinline__ int bpe_last_break(const int (&c)[IPT], int a, int64_t i0, int64_t n) {
    int last = 0;
#pragma unroll
    for (int k = 0; k < IPT; ++k)
        if (i0 + k < n && c[k] != a) last = (int)(i0 + k + 1);
    return last;
}

// bit k + 1 of the result is d(i0 + k) for k = -1 .. IPT.  `before`: the run start that holds for position i0 - 1 (the tile's last break in
// front of this thread, or the carry of the tiles before); used for a == b only.
__device__ __forceinline__ uint32_t bpe_dropped(const int (&c)[IPT], const BpeWindow& w, int a, int b, int64_t i0, int before) {
    uint32_t d = 0;
    const int lo = (int)i0;  // parities only: the low bit of a difference is the xor of the low bits
    if (a != b) {
        d |= (w.l2 == a && w.l1 == b) ? 1u : 0u;
#pragma unroll
        for (int k = 0; k < IPT; ++k) d |= ((k ? c[k - 1] : w.l1) == a && c[k] == b) ? (2u << k) : 0u;
        d |= (c[IPT - 1] == a && w.rt == b) ? (2u << IPT) : 0u;
    } else {
        int r = before;
        d |= (w.l1 == a && w.l2 == a && (((lo - 1) ^ r) & 1)) ? 1u : 0u;
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
            if (c[k] != a) r = lo + k + 1;
            d |= (c[k] == a && (k ? c[k - 1] : w.l1) == a && (((lo + k) ^ r) & 1)) ? (2u << k) : 0u;
        }
        d |= (w.rt == a && c[IPT - 1] == a && (((lo + IPT) ^ r) & 1)) ? (2u << IPT) : 0u;
    }
    return d;
}

constexpr uint32_t OWN_BITS = ((1u << IPT) - 1) << 1;  // d(i0) .. d(i0 + IPT - 1)

__global__ __launch_bounds__(TPB) void bpe_mark_kernel(const int32_t* __restrict__ src, int64_t n_cap, int m, const int32_t* __restrict__ state,
                                                      int32_t* __restrict__ tile_max, int32_t* __restrict__ tile_drop) {
    __shared__ int s_ids[TILE + TILE / 16], s_halo[4], red[TPB / 64];
    if (state[SSI_BPE_ST_DONE]) return;
    const int64_t n = bpe_len(state, m, n_cap), t0 = (int64_t)blockIdx.x * TILE;
    if (t0 >= n) return;
    const int a = state[SSI_BPE_ST_A], b = state[SSI_BPE_ST_B];
    bpe_load_tile(src, n, t0, s_ids, s_halo);
    int c[IPT];
    const BpeWindow w = bpe_read_window(s_ids, s_halo, c);
    const int64_t i0 = t0 + threadIdx.x * IPT;
    int before = 0, last = 0;
    if (a == b) before = bpe_block_scan<true>(bpe_last_break(c, a, i0, n), red, last);
    // a dropped position holds b, so it lies below n.  before == 0: no break in the tile so far, the carry decides; its parity is tried both ways
    const int even = __popc(bpe_dropped(c, w, a, b, i0, before ? before : 0) & OWN_BITS);
    const int odd = __popc(bpe_dropped(c, w, a, b, i0, before ? before : 1) & OWN_BITS);
    int n_even, n_odd;
    bpe_block_scan<false>(even, red, n_even);
    bpe_block_scan<false>(odd, red, n_odd);
    if (threadIdx.x == 0) {
        tile_max[blockIdx.x] = last;
        tile_drop[2 * blockIdx.x] = n_even;
        tile_drop[2 * blockIdx.x + 1] = n_odd;
    }
}

// One workgroup.  In: tile_max, tile_drop.  Out, in place: tile_max[t] = the carry of tile t (the run start that holds in front of it),
// tile_drop[2 t] = where the tile's kept ids begin in the other buffer.  Also: the new length, and the merged pair's count set to zero.
__global__ __launch_bounds__(SCAN_THREADS) void bpe_scan_kernel(int64_t n_cap, int m, int stride, int32_t* __restrict__ state,
                                                               uint32_t* __restrict__ table, int32_t* __restrict__ tile_max,
                                                               int32_t* __restrict__ tile_drop) {
    __shared__ int red[SCAN_THREADS / 64];
    if (state[SSI_BPE_ST_DONE]) return;
    const int64_t n = bpe_len(state, m, n_cap);
    const int64_t n_tiles = (n + TILE - 1) / TILE;
    int carry = 0, offset = 0;
    for (int64_t base = 0; base < n_tiles; base += SCAN_THREADS) {  // uniform
        const int64_t t = base + threadIdx.x;
        const bool in = t < n_tiles;
        int chunk_max, chunk_kept;
        const int own_max = in ? tile_max[t] : 0;
        const int before = max(carry, bpe_block_scan<true>(own_max, red, chunk_max));
        const int len = !in ? 0 : (n - t * TILE < TILE ? (int)(n - t * TILE) : TILE);
        const int kept = in ? len - tile_drop[2 * t + (before & 1)] : 0;
        const int at = offset + bpe_block_scan<false>(kept, red, chunk_kept);
        if (in) {
            tile_max[t] = before;
            tile_drop[2 * t] = at;
        }
        carry = max(carry, chunk_max);
        offset += chunk_kept;
    }
    if (threadIdx.x == 0) {
        state[SSI_BPE_ST_LEN + ((m + 1) & 1)] = offset;
        table[(size_t)state[SSI_BPE_ST_A] * stride + state[SSI_BPE_ST_B]] = 0;  // a, b < n_base + m: written by bpe_best_final_kernel from an index of the table
    }
}

__global__ __launch_bounds__(TPB) void bpe_apply_kernel(const int32_t* __restrict__ src, int32_t* __restrict__ dst, int64_t n_cap, int m, int z,
                                                       int stride, const int32_t* __restrict__ state, uint32_t* __restrict__ table,
                                                       const int32_t* __restrict__ tile_max, const int32_t* __restrict__ tile_drop) {
    __shared__ int s_ids[TILE + TILE / 16], s_halo[4], red[TPB / 64];
    if (state[SSI_BPE_ST_DONE]) return;
    const int64_t n = bpe_len(state, m, n_cap), t0 = (int64_t)blockIdx.x * TILE;
    if (t0 >= n) return;
    const int a = state[SSI_BPE_ST_A], b = state[SSI_BPE_ST_B];
    bpe_load_tile(src, n, t0, s_ids, s_halo);
    int c[IPT];
    const BpeWindow w = bpe_read_window(s_ids, s_halo, c);
    const int64_t i0 = t0 + threadIdx.x * IPT;
    int before = 0, unused;
    if (a == b) {
        before = bpe_block_scan<true>(bpe_last_break(c, a, i0, n), red, unused);
        if (before == 0) before = tile_max[blockIdx.x];
    }
    const uint32_t d = bpe_dropped(c, w, a, b, i0, before);
    uint32_t keep = 0;  // bit k: position i0 + k is written to the other buffer
#pragma unroll
    for (int k = 0; k < IPT; ++k) keep |= (i0 + k < n && !(d >> (k + 1) & 1)) ? (1u << k) : 0u;
    int tile_kept;
    int at = bpe_block_scan<false>(__popc(keep), red, tile_kept);  // its barriers also end every thread's reads of s_ids

    // counts first (they need the old ids), then the kept ids go back into s_ids, closed up
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
        const bool dl = d >> k & 1, dr = d >> (k + 2) & 1;          // d(i - 1), d(i + 1)
        const bool changed = (keep >> k & 1) && (dl || dr);
        const int old_l = k ? c[k - 1] : w.l1, old_r = c[k];
        const int new_l = dl ? z : old_l, new_r = dr ? z : old_r;
        // every id is checked against z (< v_cap, the host's check) before an address is formed from it
        const bool sub = changed && is_id(old_l, z) && is_id(old_r, z) && !(old_l == a && old_r == b);
        const bool add = changed && is_id(new_l, z + 1) && is_id(new_r, z + 1);
        bpe_wave_add(table, sub ? (uint32_t)old_l * (uint32_t)stride + (uint32_t)old_r : 0u, ~0u, sub);
        bpe_wave_add(table, add ? (uint32_t)new_l * (uint32_t)stride + (uint32_t)new_r : 0u, 1u, add);
    }
#pragma unroll
    for (int k = 0; k < IPT; ++k)
        if (keep >> k & 1) s_ids[P(at++)] = (d >> (k + 2) & 1) ? z : c[k];
    __syncthreads();
    const int64_t out0 = tile_drop[2 * blockIdx.x];
    for (int q = threadIdx.x; q < tile_kept; q += TPB)
        if (out0 + q < n_cap) dst[out0 + q] = s_ids[P(q)];
}

// ---- encoder ---------------------------------------------------------------------------------------------------------------------------
// One workgroup per sequence, the sequence and the rank of every adjacent pair in LDS, ITEMS contiguous ids per thread.  Per round: the
// workgroup's lowest rank q; the positions that hold it start a merge where their offset in a run of such positions is even (a run longer
// than one only arises for a pair of equal ids), found by the same prefix maximum as in the trainer; close up; ranks are looked up again
// only for a kept position whose own id or right neighbour is new.
template <int ITEMS> __device__ __forceinline__ int PE(int j) { return ITEMS == 16 ? j + (j >> 4) : j + (j >> 5); }

template <int ITEMS>
__global__ __launch_bounds__(TPB) void bpe_encode_kernel(const int32_t* __restrict__ tokens, int64_t n_tokens, const int64_t* __restrict__ seq_start,
                                                        const int32_t* __restrict__ seq_len, int max_len, const int32_t* __restrict__ rank_table,
                                                        int V, int n_base, int32_t* __restrict__ out, int32_t* __restrict__ out_len) {
    constexpr int LMAX = TPB * ITEMS;
    constexpr int LDS_N = LMAX + LMAX / 16 + 1;
    __shared__ int s_x[LDS_N], s_rank[LDS_N], s_start[LDS_N], red[TPB / 64];
    const int64_t seq = blockIdx.x;
    const int64_t st = seq_start[seq];
    int len = seq_len[seq];
    // the span check comes before any address is formed from the span (uniform over the workgroup)
    if (len < 0 || len > max_len || len > LMAX || st < 0 || st > n_tokens - len) {
        if (threadIdx.x == 0) out_len[seq] = -1;
        return;
    }
    const int n_merges = V - n_base;
    for (int k = 0; k < ITEMS; ++k) {
        const int j = k * TPB + threadIdx.x;
        s_x[PE<ITEMS>(j)] = j < len ? tokens[st + j] : SEP;
    }
    __syncthreads();
    const int j0 = threadIdx.x * ITEMS;
    auto x_at = [&](int j) { return j < LMAX ? s_x[PE<ITEMS>(j)] : SEP; };
    auto rank_of = [&](int l, int r) {  // ids outside [0, V) have no rank and act as separators: checked before the address is formed
        if (!is_id(l, V) || !is_id(r, V)) return NONE;
        const int q = rank_table[(size_t)l * V + r];
        return is_id(q, n_merges) ? q : NONE;
    };
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) s_rank[PE<ITEMS>(j0 + k)] = rank_of(x_at(j0 + k), x_at(j0 + k + 1));
    __syncthreads();

    for (;;) {
        int rk[ITEMS], lowest = NONE;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            rk[k] = s_rank[PE<ITEMS>(j0 + k)];
            lowest = min(lowest, rk[k]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lowest = min(lowest, __shfl_xor(lowest, o, 64));
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = lowest;
        __syncthreads();
        int q = red[0];
        for (int wv = 1; wv < TPB / 64; ++wv) q = min(q, red[wv]);
        if (q == NONE) break;  // uniform
        const int z = n_base + q;

        // starts: position j holds rank q and lies an even number of places behind the first of its run of such positions
        int last = 0, unused;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k)
            if (rk[k] != q) last = j0 + k + 1;
        int r = bpe_block_scan<true>(last, red, unused);
        uint32_t starts = 0;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            if (rk[k] != q) r = j0 + k + 1;
            const bool s = rk[k] == q && !(((j0 + k) ^ r) & 1);
            starts |= s ? (1u << k) : 0u;
            s_start[PE<ITEMS>(j0 + k)] = s;
        }
        __syncthreads();
        auto start_at = [&](int j) { return j >= 0 && j < LMAX ? s_start[PE<ITEMS>(j)] : 0; };
        // bit k + 1: start(j0 + k), k = -1 .. ITEMS + 1
        const uint32_t sb = (starts << 1) | (start_at(j0 - 1) ? 1u : 0u) | (start_at(j0 + ITEMS) ? (2u << ITEMS) : 0u) |
                            (start_at(j0 + ITEMS + 1) ? (4u << ITEMS) : 0u);
        int xs[ITEMS + 2];
#pragma unroll
        for (int k = 0; k < ITEMS + 2; ++k) xs[k] = x_at(j0 + k);
        int v[ITEMS], nr[ITEMS];
        uint32_t keep = 0;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const bool s0 = sb >> (k + 1) & 1, s1 = sb >> (k + 2) & 1, s2 = sb >> (k + 3) & 1, dropped = sb >> k & 1;
            keep |= (j0 + k < len && !dropped) ? (1u << k) : 0u;
            v[k] = s0 ? z : xs[k];
            // the right neighbour in the closed-up sequence: j + 2 behind a start (j + 1 is dropped), else j + 1
            const int nv = s0 ? (s2 ? z : xs[k + 2]) : (s1 ? z : xs[k + 1]);
            nr[k] = (s0 || s1) ? rank_of(v[k], nv) : rk[k];
        }
        int new_len;
        int at = bpe_block_scan<false>(__popc(keep), red, new_len);  // its barriers also end every thread's reads of s_x and s_rank
#pragma unroll
        for (int k = 0; k < ITEMS; ++k)
            if (keep >> k & 1) {
                s_x[PE<ITEMS>(at)] = v[k];
                s_rank[PE<ITEMS>(at)] = nr[k];
                ++at;
            }
        for (int j = new_len + threadIdx.x; j < len; j += TPB) {
            s_x[PE<ITEMS>(j)] = SEP;
            s_rank[PE<ITEMS>(j)] = NONE;
        }
        len = new_len;
        __syncthreads();
    }
    if (threadIdx.x == 0) out_len[seq] = len;
    for (int j = threadIdx.x; j < len; j += TPB) out[st + j] = s_x[PE<ITEMS>(j)];
}

constexpr int ENCODE_SHORT = TPB * 4;

int bpe_stream_grid(int64_t n) { return ssi_cdiv(n, TPB) < 4096 ? (int)ssi_cdiv(n, TPB) : 4096; }

}  // namespace

extern "C" int ssi_bpe_pair_count(const int32_t* ids, int64_t n, int32_t V, int32_t stride, uint32_t* table, int32_t* n_bad, void* stream) {
    SSI_CHECK_ARG(n >= 0 && n < (1LL << 31) && V > 0 && stride >= V && (n == 0 || ids) && table);
    if (stride > SSI_BPE_MAX_VOCAB) {
        ssi_set_error("ssi_bpe_pair_count: table of %d columns, above SSI_BPE_MAX_VOCAB %d", (int)stride, SSI_BPE_MAX_VOCAB);
        return SSI_ERR_UNSUPPORTED;
    }
    if (n == 0) return SSI_OK;
    hipLaunchKernelGGL(bpe_pair_count_kernel, dim3(bpe_stream_grid(n)), dim3(TPB), 0, (hipStream_t)stream, ids, n, (int)V, (int)stride, table, n_bad);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

extern "C" size_t ssi_bpe_train_workspace_bytes(int64_t n) {
    const int64_t tiles = ssi_cdiv(n < 0 ? 0 : n, TILE) + 1;
    return (size_t)MAX_PARTIALS * sizeof(unsigned long long) + (size_t)tiles * 3 * sizeof(int32_t);
}

extern "C" int ssi_bpe_train_begin(const int32_t* ids, int64_t n, int32_t n_base, int32_t v_cap, int32_t* buf0, uint32_t* table, int32_t* state,
                                   void* stream) {
    SSI_CHECK_ARG(n >= 0 && n < (1LL << 31) && n_base > 0 && v_cap >= n_base && (n == 0 || (ids && buf0)) && table && state);
    if (v_cap > SSI_BPE_MAX_VOCAB) {
        ssi_set_error("ssi_bpe_train_begin: n_base + n_merges = %d above SSI_BPE_MAX_VOCAB %d", (int)v_cap, SSI_BPE_MAX_VOCAB);
        return SSI_ERR_UNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(table, 0, (size_t)v_cap * v_cap * sizeof(uint32_t), s) != hipSuccess) {
        ssi_set_error("ssi_bpe_train_begin: clearing the table failed");
        return SSI_ERR_HIP;
    }
    hipLaunchKernelGGL(bpe_state_init_kernel, dim3(1), dim3(64), 0, s, state, (int32_t)n);
    SSI_LAUNCH_CHECK();
    if (n == 0) return SSI_OK;
    hipLaunchKernelGGL(bpe_sanitise_kernel, dim3(bpe_stream_grid(n)), dim3(TPB), 0, s, ids, n, (int)n_base, buf0, state + SSI_BPE_ST_NBAD);
    SSI_LAUNCH_CHECK();
    return ssi_bpe_pair_count(buf0, n, n_base, v_cap, table, nullptr, stream);
}

extern "C" int ssi_bpe_merge(int32_t* buf0, int32_t* buf1, int64_t n_cap, int64_t n_upper, int32_t n_base, int32_t v_cap, int32_t m,
                             int32_t min_frequency, uint32_t* table, int32_t* merges, int32_t* state, void* workspace, size_t workspace_bytes,
                             void* stream) {
    SSI_CHECK_ARG(n_cap >= 0 && n_cap < (1LL << 31) && n_upper >= 0 && n_upper <= n_cap && n_base > 0 && m >= 0 && v_cap > n_base &&
                  m < v_cap - n_base && min_frequency >= 1 && (n_cap == 0 || (buf0 && buf1)) && table && merges && state && workspace);
    if (v_cap > SSI_BPE_MAX_VOCAB) {
        ssi_set_error("ssi_bpe_merge: n_base + n_merges = %d above SSI_BPE_MAX_VOCAB %d", (int)v_cap, SSI_BPE_MAX_VOCAB);
        return SSI_ERR_UNSUPPORTED;
    }
    if (workspace_bytes < ssi_bpe_train_workspace_bytes(n_upper)) {
        ssi_set_error("ssi_bpe_merge: workspace of %zu bytes is too small", workspace_bytes);
        return SSI_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* partial = (unsigned long long*)workspace;
    int32_t* tile_max = (int32_t*)(partial + MAX_PARTIALS);
    const int64_t tiles = ssi_cdiv(n_upper, TILE);
    int32_t* tile_drop = tile_max + tiles + 1;
    const int32_t* src = (m & 1) ? buf1 : buf0;
    int32_t* dst = (m & 1) ? buf0 : buf1;
    const int v_cur = n_base + m, z = v_cur;
    const int n_partial = v_cur < MAX_PARTIALS ? v_cur : MAX_PARTIALS;
    hipLaunchKernelGGL(bpe_best_partial_kernel, dim3(n_partial), dim3(TPB), 0, s, table, v_cur, (int)v_cap, state, partial);
    hipLaunchKernelGGL(bpe_best_final_kernel, dim3(1), dim3(TPB), 0, s, partial, n_partial, (int)v_cap, (int)m, (int)min_frequency, state, merges);
    if (tiles > 0) {
        hipLaunchKernelGGL(bpe_mark_kernel, dim3((unsigned)tiles), dim3(TPB), 0, s, src, n_upper, (int)m, state, tile_max, tile_drop);
        hipLaunchKernelGGL(bpe_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, n_upper, (int)m, (int)v_cap, state, table, tile_max, tile_drop);
        hipLaunchKernelGGL(bpe_apply_kernel, dim3((unsigned)tiles), dim3(TPB), 0, s, src, dst, n_upper, (int)m, z, (int)v_cap, state, table, tile_max,
                           tile_drop);
    }
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

extern "C" int ssi_bpe_encode(const int32_t* tokens, int64_t n_tokens, const int64_t* seq_start, const int32_t* seq_len, int64_t n_seq,
                              int32_t max_len, const int32_t* rank_table, int32_t V, int32_t n_base, int32_t* out, int32_t* out_len, void* stream) {
    SSI_CHECK_ARG(n_tokens >= 0 && n_seq >= 0 && n_seq < (1LL << 31) && max_len >= 0 && n_base > 0 && V >= n_base && (n_tokens == 0 || (tokens && out)) &&
                  (n_seq == 0 || (seq_start && seq_len && out_len)) && rank_table);
    if (max_len > SSI_BPE_ENCODE_MAX_LEN || V > SSI_BPE_MAX_VOCAB) {
        ssi_set_error("ssi_bpe_encode: max_len %d above SSI_BPE_ENCODE_MAX_LEN %d, or V %d above SSI_BPE_MAX_VOCAB %d", (int)max_len,
                      SSI_BPE_ENCODE_MAX_LEN, (int)V, SSI_BPE_MAX_VOCAB);
        return SSI_ERR_UNSUPPORTED;
    }
    if (n_seq == 0) return SSI_OK;
    const dim3 grid((unsigned)n_seq), block(TPB);
    if (max_len <= ENCODE_SHORT)
        hipLaunchKernelGGL(bpe_encode_kernel<4>, grid, block, 0, (hipStream_t)stream, tokens, n_tokens, seq_start, seq_len, (int)max_len, rank_table,
                           (int)V, (int)n_base, out, out_len);
    else
        hipLaunchKernelGGL(bpe_encode_kernel<16>, grid, block, 0, (hipStream_t)stream, tokens, n_tokens, seq_start, seq_len, (int)max_len, rank_table,
                           (int)V, (int)n_base, out, out_len);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}
