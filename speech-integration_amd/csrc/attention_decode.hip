// Generation (ABI v18): the K/V cache of a decode step.  ssi_kv_store scatters the k / v columns of qkv rows into the cache,
// ssi_attn_decode is single-query attention of one new token per sequence over that sequence's cached keys.  ssi_attn_decode_beam (ABI v20)
// reads the generated keys through an ancestry table; ssi_attn_decode_split / ssi_attn_decode_beam_split (ABI v25) split a row's keys over
// workgroups and merge the partial softmax states in a second launch.  All of them share one walk (dec_walk, dec_merged) and one finish (dec_finish).
//
// The cache of one layer: k_cache and v_cache, each [n_slots, cap, n_kv * head_dim] in the model's dtype, K after RoPE (as it sits in qkv).
#include "common_hip.h"
#include <math.h>

namespace {

// =====================================================================================================================
// ssi_kv_store: one 16-byte vector per lane.  A row of qkv holds its k heads and, right behind them, its v heads: vector c of the
// row's 2 * n_kv * head_dim cache elements goes to k_cache for c < half and to v_cache otherwise.
// =====================================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void kv_store_kernel(const T* __restrict__ qkv, int64_t ld, const int64_t* __restrict__ dest, int64_t rows,
                                                       int64_t n_dest, T* __restrict__ kc, T* __restrict__ vc, int q_cols, int kv_cols,
                                                       int32_t* __restrict__ n_bad) {
    constexpr int VEC = Vec16<T>::N;
    const int half = kv_cols / VEC;                       // vectors of one row of one cache
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = i / (2 * half);
    if (r >= rows) return;
    const int c = (int)(i - r * (2 * half));
    const int64_t d = dest[r];
    if (d == -1) return;
    if (d < 0 || d >= n_dest) {
        if (c == 0 && n_bad) atomicAdd(n_bad, 1);         // integer: exact whatever the order
        return;
    }
    const Vec16<T> x = load16<T>(qkv + r * ld + q_cols + (int64_t)c * VEC);
    T* dst = (c < half ? kc : vc) + d * kv_cols + (int64_t)(c < half ? c : c - half) * VEC;
    store16<T>(dst, x);
}

// =====================================================================================================================
// ssi_attn_decode: one workgroup per (row, kv head), 4 waves.  The G query heads of the group share every K / V line.
//
// Lanes: a key's head_dim elements are spread over LPK = 2^lpk_log2 lanes, 16 bytes each (lanes whose columns lie past head_dim idle:
// head_dim / VEC need not be a power of two), so a wave holds KPW = 64 / LPK keys per load.  A wave takes key CHUNKS of U * KPW keys,
// chunk c going to wave c % 4; inside a chunk key slot s of load u holds key  base + u * KPW + s.  Every lane keeps the running
// (max, exp-sum, P.V) of its key slot in fp32 — scores in base 2: q is scaled by log2(e) / sqrt(head_dim) once —
// and the states are merged in a FIXED order: the key slots of a wave by an xor tree (the lower slot's state first), the four waves
// through LDS in the order 0, 1, 2, 3.  P is never rounded to the storage type.  A row's result depends on that row's inputs only.
// =====================================================================================================================
constexpr int DEC_WAVES = 4, DEC_U = 2, DEC_MAX_HD = 128;

__device__ __forceinline__ float dec_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
// weight of a partial state with maximum m in a merged state with maximum mn >= m (an empty state has m = -inf, also when mn is -inf)
__device__ __forceinline__ float dec_weight(float m, float mn) { return m == -INFINITY ? 0.f : dec_exp2(m - mn); }

// Where a lane stands in its wave: the key slot it serves and the 16 bytes (columns col .. col + VEC - 1) of that key's lines it holds.
struct DecLane {
    int lpk, kpw, sub, kslot, col;
};
template <typename T>
__device__ __forceinline__ DecLane dec_lane(int lpk_log2, int hd) {
    const int lane = threadIdx.x & 63, lpk = 1 << lpk_log2;
    const int sub = lane & (lpk - 1);
    return {lpk, 64 >> lpk_log2, sub, lane >> lpk_log2, sub * Vec16<T>::N};
}

// The per-wave states of a workgroup on their way through LDS
template <int G>
struct DecLds {
    float (&m)[DEC_WAVES][G], (&l)[DEC_WAVES][G];
    float (&acc)[DEC_WAVES][G][DEC_MAX_HD];
};
#define DEC_LDS(G, lds)                                      \
    __shared__ float s_m[DEC_WAVES][G], s_l[DEC_WAVES][G];   \
    __shared__ float s_acc[DEC_WAVES][G][DEC_MAX_HD];        \
    const DecLds<G> lds{s_m, s_l, s_acc}

// THE WALK of one (row, kv head) of single-query attention over the keys k0 .. n - 1, the body every decode kernel shares: the key walk, the
// per-key update and the xor tree over a wave's key slots, up to the four waves' states in ``lds`` (behind a barrier); ``dec_merged`` then merges
// them.  Waves and chunks are placed relative to k0.  ``keys.exists(j)`` says whether key j is there — one that is not is skipped and leaves the
// state as it was — and ``keys.lines(j, kp, vp)`` names the lane's 16 bytes of its K and V lines.  Without CAN_SKIP the caller promises
// n > k0 keys that all exist.  ``qrow``: the row's first query head of this kv head.
template <typename T, int G, bool CAN_SKIP, typename Keys>
__device__ __forceinline__ void dec_walk(const T* __restrict__ qrow, int k0, int n, int hd, int g, const DecLane& at, float qscale, const Keys& keys,
                                         const DecLds<G>& lds) {
    constexpr int VEC = Vec16<T>::N;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lpk = at.lpk, kpw = at.kpw, sub = at.sub, kslot = at.kslot, col = at.col;
    const bool active = col < hd;

    float q[G][VEC], acc[G][VEC], m[G], l[G];
#pragma unroll
    for (int h = 0; h < G; ++h) {
        const int hh = h < g ? h : g - 1;                 // heads past g repeat the last one and are not stored
        Vec16<T> x = {};
        if (active) x = load16<T>(qrow + (int64_t)hh * hd + col);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            q[h][v] = active ? x.get(v) * qscale : 0.f;
            acc[h][v] = 0.f;
        }
        m[h] = -INFINITY;
        l[h] = 0.f;
    }

    const int chunk = kpw * DEC_U;
    for (int base = k0 + wave * chunk; base < n; base += DEC_WAVES * chunk) {
        Vec16<T> kx[DEC_U] = {}, vx[DEC_U] = {};
        bool have[DEC_U];
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {                 // every load of the chunk is issued before the first use
            const int j = base + u * kpw + kslot;
            have[u] = j < n;
            if (CAN_SKIP) have[u] = have[u] && keys.exists(j);
            if (have[u] && active) {
                const T *kp, *vp;
                keys.lines(j, kp, vp);
                kx[u] = load16_nt<T>(kp);
                vx[u] = load16_nt<T>(vp);
            }
        }
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const bool ld_ok = have[u] && active;
            float kf[VEC], vf[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                kf[v] = ld_ok ? kx[u].get(v) : 0.f;
                vf[v] = ld_ok ? vx[u].get(v) : 0.f;
            }
            float s[G];
#pragma unroll
            for (int h = 0; h < G; ++h) {
                float d = 0.f;
#pragma unroll
                for (int v = 0; v < VEC; ++v) d = __builtin_fmaf(q[h][v], kf[v], d);
                s[h] = d;
            }
            for (int o = lpk >> 1; o > 0; o >>= 1) {      // (every lane of the wave takes part: the trip count is uniform)
#pragma unroll
                for (int h = 0; h < G; ++h) s[h] += __shfl_xor(s[h], o, 64);
            }
            if (have[u]) {
#pragma unroll
                for (int h = 0; h < G; ++h) {
                    const float mn = fmaxf(m[h], s[h]);
                    const float a = dec_exp2(m[h] - mn);  // (-inf - finite = -inf: 0)
                    const float p = dec_exp2(s[h] - mn);
                    l[h] = __builtin_fmaf(l[h], a, p);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[h][v] = __builtin_fmaf(p, vf[v], acc[h][v] * a);
                    m[h] = mn;
                }
            }
        }
    }

    // the key slots of the wave: xor tree, the state of the lower slot first in every sum (all lanes then hold the same bits)
    for (int o = lpk; o < 64; o <<= 1) {
        const bool low = (lane & o) == 0;
#pragma unroll
        for (int h = 0; h < G; ++h) {
            const float mo = __shfl_xor(m[h], o, 64), lo = __shfl_xor(l[h], o, 64);
            const float m0 = low ? m[h] : mo, m1 = low ? mo : m[h];
            const float mn = fmaxf(m0, m1);
            const float e0 = dec_weight(m0, mn), e1 = dec_weight(m1, mn);
            l[h] = __builtin_fmaf(low ? lo : l[h], e1, (low ? l[h] : lo) * e0);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float ao = __shfl_xor(acc[h][v], o, 64);
                acc[h][v] = __builtin_fmaf(low ? ao : acc[h][v], e1, (low ? acc[h][v] : ao) * e0);
            }
            m[h] = mn;
        }
    }
    if (kslot == 0 && active) {
#pragma unroll
        for (int h = 0; h < G; ++h) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) lds.acc[wave][h][col + v] = acc[h][v];
            if (sub == 0) {
                lds.m[wave][h] = m[h];
                lds.l[wave][h] = l[h];
            }
        }
    }
    __syncthreads();
}

// the four waves, in order: the merged, unnormalised state (M, L, O) of head h, column d
template <int G>
__device__ __forceinline__ void dec_merged(const DecLds<G>& lds, int h, int d, float& M, float& L, float& O) {
    float mn = lds.m[0][h];
#pragma unroll
    for (int w = 1; w < DEC_WAVES; ++w) mn = fmaxf(mn, lds.m[w][h]);
    L = 0.f, O = 0.f;
#pragma unroll
    for (int w = 0; w < DEC_WAVES; ++w) {
        const float e = dec_weight(lds.m[w][h], mn);
        L = __builtin_fmaf(lds.l[w][h], e, L);
        O = __builtin_fmaf(lds.acc[w][h][d], e, O);
    }
    M = mn;
}

// THE FINISH of one element: the division, the one rounding on the store and the head's lse (written by the lane of column 0; ``lse`` may be
// null).  ``can_skip``: a row all of whose keys were skipped is zeros with lse -inf.
template <typename T>
__device__ __forceinline__ void dec_finish(float M, float L, float O, bool can_skip, T* __restrict__ o, float* __restrict__ lse, bool first) {
    const bool none = can_skip && !(L > 0.f);             // every key was skipped
    *o = from_f32<T>(none ? 0.f : O / L);
    if (lse && first) *lse = none ? -INFINITY : (M + log2f(L)) * 0.69314718055994531f;
}

// walk and finish of one (row, kv head) over the keys 0 .. n - 1 in one workgroup; ``lse`` (may be null) takes the heads' values from ``lse[lse_at]`` on
template <typename T, int G, bool CAN_SKIP, typename Keys>
__device__ __forceinline__ void dec_row(const T* __restrict__ qrow, int n, T* __restrict__ orow, float* __restrict__ lse, int64_t lse_at, int hd,
                                        int g, const DecLane& at, float qscale, const Keys& keys) {
    DEC_LDS(G, lds);
    dec_walk<T, G, CAN_SKIP>(qrow, 0, n, hd, g, at, qscale, keys, lds);
    for (int i = threadIdx.x; i < g * hd; i += 256) {
        const int h = i / hd, d = i - h * hd;
        float M, L, O;
        dec_merged<G>(lds, h, d, M, L, O);
        dec_finish<T>(M, L, O, CAN_SKIP, orow + i, lse ? lse + lse_at + h : nullptr, d == 0);
    }
}

// walk of the keys k0 .. n - 1 in one workgroup, its merged state to the split's place in the workspace: per query head head_dim + 2 floats,
// O[head_dim], M, L (``part``: the first head's; a head's lines lie ``head_stride`` floats apart)
template <typename T, int G, bool CAN_SKIP, typename Keys>
__device__ __forceinline__ void dec_part(const T* __restrict__ qrow, int k0, int n, float* __restrict__ part, int64_t head_stride, int hd, int g,
                                         const DecLane& at, float qscale, const Keys& keys) {
    DEC_LDS(G, lds);
    dec_walk<T, G, CAN_SKIP>(qrow, k0, n, hd, g, at, qscale, keys, lds);
    for (int i = threadIdx.x; i < g * hd; i += 256) {
        const int h = i / hd, d = i - h * hd;
        float M, L, O;
        dec_merged<G>(lds, h, d, M, L, O);
        float* p = part + h * head_stride;
        p[d] = O;
        if (d == 0) {
            p[hd] = M;
            p[hd + 1] = L;
        }
    }
}

// the keys of one cache slot, one behind the other
template <typename T>
struct SlotKeys {
    const T *kbase, *vbase;                               // key 0, the lane's columns
    int64_t kv_cols;
    __device__ __forceinline__ bool exists(int) const { return true; }
    __device__ __forceinline__ void lines(int j, const T*& kp, const T*& vp) const {
        kp = kbase + (int64_t)j * kv_cols;
        vp = vbase + (int64_t)j * kv_cols;
    }
};

template <typename T, int G>
__global__ __launch_bounds__(256) void kv_decode_kernel(const T* __restrict__ qkv, int64_t ld, const T* __restrict__ kc, const T* __restrict__ vc,
                                                        int64_t n_slots, int cap, const int32_t* __restrict__ slot,
                                                        const int32_t* __restrict__ kv_len, T* __restrict__ out, float* __restrict__ lse,
                                                        int n_heads, int n_kv, int hd, int g, int lpk_log2, float qscale,
                                                        int32_t* __restrict__ n_bad) {
    const int64_t r = blockIdx.x;
    const int kvh = blockIdx.y, tid = threadIdx.x;
    const int h0 = kvh * g;
    const int sl = slot[r];
    int n = kv_len[r];
    n = n < cap ? n : cap;
    T* orow = out + (r * n_heads + h0) * hd;
    if (sl < 0 || sl >= n_slots || n <= 0) {              // (uniform over the workgroup)
        for (int i = tid; i < g * hd; i += 256) orow[i] = from_f32<T>(0.f);
        if (lse && tid < g) lse[r * n_heads + h0 + tid] = -INFINITY;
        if (sl >= n_slots && kvh == 0 && tid == 0 && n_bad) atomicAdd(n_bad, 1);
        return;
    }
    const DecLane at = dec_lane<T>(lpk_log2, hd);
    const int64_t kv_cols = (int64_t)n_kv * hd;
    const T* kbase = kc + ((int64_t)sl * cap * n_kv + kvh) * hd + at.col;
    const T* vbase = vc + ((int64_t)sl * cap * n_kv + kvh) * hd + at.col;
    dec_row<T, G, false>(qkv + r * ld + (int64_t)h0 * hd, n, orow, lse, r * n_heads + h0, hd, g, at, qscale, SlotKeys<T>{kbase, vbase, kv_cols});
}

// =====================================================================================================================
// ssi_attn_decode_beam (ABI v20): the same row over the concatenation of two key ranges — the np keys of a PROMPT cache slot, then ng keys of a
// BEAM cache read through an ancestry table: generated position i of row r lies in beam slot anc[r, i], at position i.  Key j of the walk
// is prompt key j for j < np and generated key j - np otherwise, so chunks, waves and merges are those of kv_decode_kernel on a cache that
// holds the row's keys one behind the other, and so are the bits.  An index outside its cache is never turned into an address: the key is
// skipped, and the row is counted once.
// =====================================================================================================================
// prompt keys 0 .. np - 1 of one prompt cache slot, then generated keys: position i of the beam cache slot the ancestry names
template <typename T>
struct BeamKeys {
    const T *pk, *pv;                                     // prompt key 0, the lane's columns (never used when !p_ok)
    const T *bk, *bv;                                     // the beam cache
    const int32_t* arow;                                  // the row's ancestry
    int64_t kv_cols, head_at;                             // elements per cached position; the lane's columns within one
    int np, cap_b, n_bslots;
    bool p_ok;
    __device__ __forceinline__ bool exists(int j) const {
        if (j < np) return p_ok;
        const int a = arow[j - np];
        return a >= 0 && a < n_bslots;                    // checked before any address is formed from it
    }
    __device__ __forceinline__ void lines(int j, const T*& kp, const T*& vp) const {   // (only for a key that exists)
        if (j < np) {
            kp = pk + (int64_t)j * kv_cols;
            vp = pv + (int64_t)j * kv_cols;
        } else {
            const int i = j - np;
            const int64_t off = ((int64_t)arow[i] * cap_b + i) * kv_cols + head_at;
            kp = bk + off;
            vp = bv + off;
        }
    }
};

template <typename T, int G>
__global__ __launch_bounds__(256) void beam_decode_kernel(const T* __restrict__ qkv, int64_t ld, const T* __restrict__ pk, const T* __restrict__ pv,
                                                          int64_t n_pslots, int cap_p, const T* __restrict__ bk, const T* __restrict__ bv,
                                                          int64_t n_bslots, int cap_b, const int32_t* __restrict__ prompt_slot,
                                                          const int32_t* __restrict__ prompt_len, const int32_t* __restrict__ gen_len,
                                                          const int32_t* __restrict__ anc, int64_t ld_anc, T* __restrict__ out,
                                                          float* __restrict__ lse, int n_heads, int n_kv, int hd, int g, int lpk_log2, float qscale,
                                                          int32_t* __restrict__ n_bad) {
    const int64_t r = blockIdx.x;
    const int kvh = blockIdx.y, tid = threadIdx.x;
    const int h0 = kvh * g;
    const int sl = prompt_slot[r];
    int np = prompt_len[r], ng = gen_len[r];
    np = np < cap_p ? np : cap_p;
    np = np > 0 ? np : 0;
    ng = ng < cap_b ? ng : cap_b;
    ng = (int64_t)ng < ld_anc ? ng : (int)ld_anc;
    ng = ng > 0 ? ng : 0;
    T* orow = out + (r * n_heads + h0) * hd;
    if (sl < 0 || np + ng <= 0) {                         // (uniform over the workgroup)
        for (int i = tid; i < g * hd; i += 256) orow[i] = from_f32<T>(0.f);
        if (lse && tid < g) lse[r * n_heads + h0 + tid] = -INFINITY;
        return;
    }
    const bool p_ok = sl < n_pslots;
    const int64_t kv_cols = (int64_t)n_kv * hd;
    const DecLane at = dec_lane<T>(lpk_log2, hd);
    const int64_t pbase = ((int64_t)(p_ok ? sl : 0) * cap_p * n_kv + kvh) * hd + at.col;
    const BeamKeys<T> keys{pk + pbase, pv + pbase, bk, bv, anc + r * ld_anc, kv_cols, (int64_t)kvh * hd + at.col, np, cap_b, (int)n_bslots, p_ok};
    dec_row<T, G, true>(qkv + r * ld + (int64_t)h0 * hd, np + ng, orow, lse, r * n_heads + h0, hd, g, at, qscale, keys);
    if (kvh == 0 && n_bad) {                              // once per row (every kv head meets the same indices): the ancestry alone once more
        bool bad = !p_ok && np > 0;
        for (int i = tid; i < ng; i += 256) bad |= !keys.exists(np + i);
        const int any = __syncthreads_or(bad ? 1 : 0);
        if (tid == 0 && any) atomicAdd(n_bad, 1);
    }
}

// =====================================================================================================================
// ssi_attn_decode_split / ssi_attn_decode_beam_split (ABI v25): the keys of a (row, kv head) over several workgroups.  Workgroup z of a row
// with n keys walks the keys [z * span, min((z + 1) * span, n)) as the plain kernel walks a cache that starts there, and writes its merged,
// unnormalised state to the workspace [rows, n_heads, n_splits, head_dim + 2]; a merge kernel behind it on the stream applies the four-wave
// merge's formula over the row's ceil(n / span) partials in the order z = 0, 1, ... and finishes.  No atomics but the error count, no flag,
// no ticket: the kernel boundary is the only synchronisation.
// =====================================================================================================================
template <typename T, int G>
__global__ __launch_bounds__(256) void split_kv_walk_kernel(const T* __restrict__ qkv, int64_t ld, const T* __restrict__ kc, const T* __restrict__ vc,
                                                            int64_t n_slots, int cap, const int32_t* __restrict__ slot,
                                                            const int32_t* __restrict__ kv_len, float* __restrict__ ws, int64_t span, int n_heads,
                                                            int n_kv, int hd, int g, int lpk_log2, float qscale) {
    const int64_t r = blockIdx.x, k0 = (int64_t)blockIdx.z * span;
    const int kvh = blockIdx.y, h0 = kvh * g;
    const int sl = slot[r];
    int n = kv_len[r];
    n = n < cap ? n : cap;
    if (sl < 0 || sl >= n_slots || k0 >= n) return;       // (uniform over the workgroup; n <= 0 is among them: the merge writes such a row)
    const int n_end = k0 + span < n ? (int)(k0 + span) : n;
    const DecLane at = dec_lane<T>(lpk_log2, hd);
    const int64_t kv_cols = (int64_t)n_kv * hd;
    const T* kbase = kc + ((int64_t)sl * cap * n_kv + kvh) * hd + at.col;
    const T* vbase = vc + ((int64_t)sl * cap * n_kv + kvh) * hd + at.col;
    float* part = ws + (((r * n_heads + h0) * gridDim.z) + blockIdx.z) * (hd + 2);
    dec_part<T, G, false>(qkv + r * ld + (int64_t)h0 * hd, (int)k0, n_end, part, (int64_t)gridDim.z * (hd + 2), hd, g, at, qscale,
                          SlotKeys<T>{kbase, vbase, kv_cols});
}

template <typename T, int G>
__global__ __launch_bounds__(256) void split_beam_walk_kernel(const T* __restrict__ qkv, int64_t ld, const T* __restrict__ pk, const T* __restrict__ pv,
                                                              int64_t n_pslots, int cap_p, const T* __restrict__ bk, const T* __restrict__ bv,
                                                              int64_t n_bslots, int cap_b, const int32_t* __restrict__ prompt_slot,
                                                              const int32_t* __restrict__ prompt_len, const int32_t* __restrict__ gen_len,
                                                              const int32_t* __restrict__ anc, int64_t ld_anc, float* __restrict__ ws, int64_t span,
                                                              int n_heads, int n_kv, int hd, int g, int lpk_log2, float qscale,
                                                              int32_t* __restrict__ n_bad) {
    const int64_t r = blockIdx.x, k0 = (int64_t)blockIdx.z * span;
    const int kvh = blockIdx.y, tid = threadIdx.x, h0 = kvh * g;
    const int sl = prompt_slot[r];
    int np = prompt_len[r], ng = gen_len[r];
    np = np < cap_p ? np : cap_p;
    np = np > 0 ? np : 0;
    ng = ng < cap_b ? ng : cap_b;
    ng = (int64_t)ng < ld_anc ? ng : (int)ld_anc;
    ng = ng > 0 ? ng : 0;
    const int n = np + ng;
    if (sl < 0 || k0 >= n) return;                        // (uniform over the workgroup)
    const int n_end = k0 + span < n ? (int)(k0 + span) : n;
    const bool p_ok = sl < n_pslots;
    const int64_t kv_cols = (int64_t)n_kv * hd;
    const DecLane at = dec_lane<T>(lpk_log2, hd);
    const int64_t pbase = ((int64_t)(p_ok ? sl : 0) * cap_p * n_kv + kvh) * hd + at.col;
    const BeamKeys<T> keys{pk + pbase, pv + pbase, bk, bv, anc + r * ld_anc, kv_cols, (int64_t)kvh * hd + at.col, np, cap_b, (int)n_bslots, p_ok};
    float* part = ws + (((r * n_heads + h0) * gridDim.z) + blockIdx.z) * (hd + 2);
    dec_part<T, G, true>(qkv + r * ld + (int64_t)h0 * hd, (int)k0, n_end, part, (int64_t)gridDim.z * (hd + 2), hd, g, at, qscale, keys);
    if (kvh == 0 && blockIdx.z == 0 && n_bad) {           // once per row, over the whole ancestry: beam_decode_kernel's count
        bool bad = !p_ok && np > 0;
        for (int i = tid; i < ng; i += 256) bad |= !keys.exists(np + i);
        const int any = __syncthreads_or(bad ? 1 : 0);
        if (tid == 0 && any) atomicAdd(n_bad, 1);
    }
}

// The merge of both forms, one workgroup per (row, kv head), one thread per (head, column).  A row has ``len_a`` keys clamped to [0, cap_a]
// and, with ``len_b`` (the beam form), ``len_b`` more clamped to [0, cap_b]; ``slot >= slot_limit`` is a dead row that is counted (the slot form's
// slot outside the cache; the beam form passes no limit: its walk skips and counts).  Only the splits the walk wrote are read.
template <typename T>
__global__ __launch_bounds__(256) void split_kv_merge_kernel(const float* __restrict__ ws, int64_t span, int64_t n_splits, const int32_t* __restrict__ slot,
                                                             int64_t slot_limit, const int32_t* __restrict__ len_a, int cap_a,
                                                             const int32_t* __restrict__ len_b, int cap_b, T* __restrict__ out,
                                                             float* __restrict__ lse, int n_heads, int hd, int g, int32_t* __restrict__ n_bad) {
    const int64_t r = blockIdx.x;
    const int kvh = blockIdx.y, tid = threadIdx.x, h0 = kvh * g;
    const int sl = slot[r];
    int n = len_a[r];
    n = n < cap_a ? n : cap_a;
    n = (len_b && n < 0) ? 0 : n;
    if (len_b) {
        int nb = len_b[r];
        nb = nb < cap_b ? nb : cap_b;
        n += nb > 0 ? nb : 0;
    }
    T* orow = out + (r * n_heads + h0) * hd;
    if (sl < 0 || sl >= slot_limit || n <= 0) {           // (uniform over the workgroup)
        for (int i = tid; i < g * hd; i += 256) orow[i] = from_f32<T>(0.f);
        if (lse && tid < g) lse[r * n_heads + h0 + tid] = -INFINITY;
        if (sl >= slot_limit && kvh == 0 && tid == 0 && n_bad) atomicAdd(n_bad, 1);
        return;
    }
    const int S = (int)((n + span - 1) / span);
    const int64_t line = hd + 2;
    for (int i = tid; i < g * hd; i += 256) {
        const int h = i / hd, d = i - h * hd;
        const float* p = ws + (r * n_heads + h0 + h) * n_splits * line;
        float M = p[hd];
        for (int z = 1; z < S; ++z) M = fmaxf(M, p[z * line + hd]);
        float L = 0.f, O = 0.f;
        for (int z = 0; z < S; ++z) {
            const float e = dec_weight(p[z * line + hd], M);
            L = __builtin_fmaf(p[z * line + hd + 1], e, L);
            O = __builtin_fmaf(p[z * line + d], e, O);
        }
        dec_finish<T>(M, L, O, len_b != nullptr, orow + i, lse ? lse + r * n_heads + h0 + h : nullptr, d == 0);
    }
}

template <typename T, int G>
void launch_decode(const void* qkv, int64_t ld, const void* kc, const void* vc, int64_t n_slots, int64_t cap, const int32_t* slot,
                   const int32_t* kv_len, void* out, float* lse, int64_t rows, int n_heads, int n_kv, int hd, int32_t* n_bad, void* stream) {
    const int lanes = hd / Vec16<T>::N;
    int lpk_log2 = 0;
    while ((1 << lpk_log2) < lanes) ++lpk_log2;
    const float qscale = (float)(1.4426950408889634 / sqrt((double)hd));
    hipLaunchKernelGGL((kv_decode_kernel<T, G>), dim3((unsigned)rows, (unsigned)n_kv), dim3(256), 0, (hipStream_t)stream, (const T*)qkv, ld,
                       (const T*)kc, (const T*)vc, n_slots, (int)cap, slot, kv_len, (T*)out, lse, n_heads, n_kv, hd, n_heads / n_kv, lpk_log2,
                       qscale, n_bad);
}

template <typename T, int G>
void launch_decode_beam(const void* qkv, int64_t ld, const void* pk, const void* pv, int64_t n_pslots, int64_t cap_p, const void* bk, const void* bv,
                        int64_t n_bslots, int64_t cap_b, const int32_t* prompt_slot, const int32_t* prompt_len, const int32_t* gen_len,
                        const int32_t* anc, int64_t ld_anc, void* out, float* lse, int64_t rows, int n_heads, int n_kv, int hd, int32_t* n_bad,
                        void* stream) {
    const int lanes = hd / Vec16<T>::N;
    int lpk_log2 = 0;
    while ((1 << lpk_log2) < lanes) ++lpk_log2;
    const float qscale = (float)(1.4426950408889634 / sqrt((double)hd));
    hipLaunchKernelGGL((beam_decode_kernel<T, G>), dim3((unsigned)rows, (unsigned)n_kv), dim3(256), 0, (hipStream_t)stream, (const T*)qkv, ld,
                       (const T*)pk, (const T*)pv, n_pslots, (int)cap_p, (const T*)bk, (const T*)bv, n_bslots, (int)cap_b, prompt_slot, prompt_len,
                       gen_len, anc, ld_anc, (T*)out, lse, n_heads, n_kv, hd, n_heads / n_kv, lpk_log2, qscale, n_bad);
}

template <typename T, int G>
void launch_split(const void* qkv, int64_t ld, const void* kc, const void* vc, int64_t n_slots, int64_t cap, const int32_t* slot,
                  const int32_t* kv_len, float* ws, int64_t span, int64_t n_splits, int64_t rows, int n_heads, int n_kv, int hd, void* stream) {
    const int lanes = hd / Vec16<T>::N;
    int lpk_log2 = 0;
    while ((1 << lpk_log2) < lanes) ++lpk_log2;
    const float qscale = (float)(1.4426950408889634 / sqrt((double)hd));
    hipLaunchKernelGGL((split_kv_walk_kernel<T, G>), dim3((unsigned)rows, (unsigned)n_kv, (unsigned)n_splits), dim3(256), 0, (hipStream_t)stream,
                       (const T*)qkv, ld, (const T*)kc, (const T*)vc, n_slots, (int)cap, slot, kv_len, ws, span, n_heads, n_kv, hd, n_heads / n_kv,
                       lpk_log2, qscale);
}

template <typename T, int G>
void launch_split_beam(const void* qkv, int64_t ld, const void* pk, const void* pv, int64_t n_pslots, int64_t cap_p, const void* bk, const void* bv,
                       int64_t n_bslots, int64_t cap_b, const int32_t* prompt_slot, const int32_t* prompt_len, const int32_t* gen_len,
                       const int32_t* anc, int64_t ld_anc, float* ws, int64_t span, int64_t n_splits, int64_t rows, int n_heads, int n_kv, int hd,
                       int32_t* n_bad, void* stream) {
    const int lanes = hd / Vec16<T>::N;
    int lpk_log2 = 0;
    while ((1 << lpk_log2) < lanes) ++lpk_log2;
    const float qscale = (float)(1.4426950408889634 / sqrt((double)hd));
    hipLaunchKernelGGL((split_beam_walk_kernel<T, G>), dim3((unsigned)rows, (unsigned)n_kv, (unsigned)n_splits), dim3(256), 0, (hipStream_t)stream,
                       (const T*)qkv, ld, (const T*)pk, (const T*)pv, n_pslots, (int)cap_p, (const T*)bk, (const T*)bv, n_bslots, (int)cap_b,
                       prompt_slot, prompt_len, gen_len, anc, ld_anc, ws, span, n_heads, n_kv, hd, n_heads / n_kv, lpk_log2, qscale, n_bad);
}

template <typename T>
void launch_split_merge(const float* ws, int64_t span, int64_t n_splits, const int32_t* slot, int64_t slot_limit, const int32_t* len_a, int64_t cap_a,
                        const int32_t* len_b, int64_t cap_b, void* out, float* lse, int64_t rows, int n_heads, int n_kv, int hd, int32_t* n_bad,
                        void* stream) {
    hipLaunchKernelGGL(split_kv_merge_kernel<T>, dim3((unsigned)rows, (unsigned)n_kv), dim3(256), 0, (hipStream_t)stream, ws, span, n_splits, slot,
                       slot_limit, len_a, (int)cap_a, len_b, (int)cap_b, (T*)out, lse, n_heads, hd, n_heads / n_kv, n_bad);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// head geometry both entries accept
int check_geometry(const char* who, int n_heads, int n_kv, int head_dim) {
    if (n_heads < 1 || n_kv < 1 || head_dim < 1) { ssi_set_error("%s: n_heads, n_kv and head_dim must be positive", who); return SSI_ERR_ARG; }
    if (n_heads % n_kv || n_heads / n_kv > 8 || head_dim % 8 || head_dim > DEC_MAX_HD || n_kv > 65535) {
        ssi_set_error("%s: unsupported head geometry (n_heads %d, n_kv %d, head_dim %d): head_dim a multiple of 8 up to %d, 1 to 8 query heads "
                      "per kv head", who, n_heads, n_kv, head_dim, DEC_MAX_HD);
        return SSI_ERR_UNSUPPORTED;
    }
    return SSI_OK;
}

// what ssi_attn_decode and its split form check alike (rows > 0)
int check_decode_args(const void* qkv, int64_t ld, const void* k_cache, const void* v_cache, int64_t n_slots, int64_t cap, const int32_t* slot,
                      const int32_t* kv_len, const void* out, int64_t rows, int n_heads, int head_dim, int dtype) {
    const int64_t esize = dtype == SSI_BF16 ? 2 : 4;
    SSI_CHECK_ARG(qkv && slot && kv_len && out && rows < (1LL << 31) && ld >= (int64_t)n_heads * head_dim);
    SSI_CHECK_ARG((k_cache && v_cache) || n_slots * cap == 0);
    SSI_CHECK_ARG(aligned16(qkv) && aligned16(k_cache) && aligned16(v_cache) && (ld * esize) % 16 == 0);
    return SSI_OK;
}

// what ssi_attn_decode_beam and its split form check alike (rows > 0)
int check_beam_args(const void* qkv, int64_t ld, const void* pk_cache, const void* pv_cache, int64_t n_pslots, int64_t cap_p, const void* bk_cache,
                    const void* bv_cache, int64_t n_bslots, int64_t cap_b, const int32_t* prompt_slot, const int32_t* prompt_len,
                    const int32_t* gen_len, const int32_t* anc, int64_t ld_anc, const void* out, int64_t rows, int n_heads, int head_dim, int dtype) {
    const int64_t esize = dtype == SSI_BF16 ? 2 : 4;
    SSI_CHECK_ARG(qkv && prompt_slot && prompt_len && gen_len && out && rows < (1LL << 31) && ld >= (int64_t)n_heads * head_dim);
    SSI_CHECK_ARG((pk_cache && pv_cache) || n_pslots * cap_p == 0);
    SSI_CHECK_ARG((bk_cache && bv_cache && anc) || n_bslots * cap_b * ld_anc == 0);
    SSI_CHECK_ARG(aligned16(qkv) && aligned16(pk_cache) && aligned16(pv_cache) && aligned16(bk_cache) && aligned16(bv_cache) && (ld * esize) % 16 == 0);
    return SSI_OK;
}

// keys per round of the four waves (8 loads of 64 / LPK keys) of a form, the unit of a split's span; 0: no such form
int decode_round(int head_dim, int dtype) {
    if ((dtype != SSI_F32 && dtype != SSI_BF16) || head_dim < 1 || head_dim % 8 || head_dim > DEC_MAX_HD) return 0;
    const int lanes = head_dim * (dtype == SSI_BF16 ? 2 : 4) / 16;
    int lpk = 1;
    while (lpk < lanes) lpk *= 2;
    return 8 * (64 / lpk);
}

// the default span in keys where a form's round is not larger: tools/generate_bench.py --part split_kv (README, "Split-KV decode attention")
constexpr int DEC_SPLIT_SPAN = 128;

// what the two split entries check alike: the span, the number of splits against the ``keys`` a row can have, the workspace
int check_split_args(int64_t span, int64_t n_splits, int64_t keys, const void* workspace, int64_t workspace_bytes, int64_t rows, int n_heads,
                     int head_dim, int dtype) {
    const int round = decode_round(head_dim, dtype);
    SSI_CHECK_ARG(round > 0 && span > 0 && span % round == 0 && span < (1LL << 31));
    SSI_CHECK_ARG(n_splits >= 1 && n_splits <= 65535 && n_splits * span >= keys);
    SSI_CHECK_ARG(workspace && aligned16(workspace) && workspace_bytes >= ssi_attn_decode_split_workspace(rows, n_heads, head_dim, n_splits));
    return SSI_OK;
}

#define SSI_DECODE_FORMS(g, LAUNCH)  \
    do {                             \
        if ((g) == 1) LAUNCH(1);     \
        else if ((g) == 2) LAUNCH(2); \
        else if ((g) <= 4) LAUNCH(4); \
        else LAUNCH(8);              \
    } while (0)

}  // namespace

extern "C" int ssi_kv_store(const void* qkv, int64_t ld, const int64_t* dest, int64_t rows, int64_t n_dest, void* k_cache, void* v_cache,
                            int n_heads, int n_kv, int head_dim, int32_t* n_bad, int dtype, void* stream) {
    SSI_CHECK_ARG(rows >= 0 && n_dest >= 0 && (dtype == SSI_F32 || dtype == SSI_BF16));
    if (int rc = check_geometry("ssi_kv_store", n_heads, n_kv, head_dim)) return rc;
    if (rows == 0) return SSI_OK;
    const int64_t esize = dtype == SSI_BF16 ? 2 : 4, q_cols = (int64_t)n_heads * head_dim, kv_cols = (int64_t)n_kv * head_dim;
    SSI_CHECK_ARG(qkv && dest && k_cache && v_cache && ld >= q_cols + 2 * kv_cols && rows < (1LL << 31));
    SSI_CHECK_ARG(aligned16(qkv) && aligned16(k_cache) && aligned16(v_cache) && (ld * esize) % 16 == 0);
    const int64_t vecs = rows * (2 * kv_cols / (16 / esize));
    SSI_CHECK_ARG(ssi_cdiv(vecs, 256) < (1LL << 31));
    SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(kv_store_kernel<T>, dim3((unsigned)ssi_cdiv(vecs, 256)), dim3(256), 0, (hipStream_t)stream,
                                                 (const T*)qkv, ld, dest, rows, n_dest, (T*)k_cache, (T*)v_cache, (int)q_cols, (int)kv_cols, n_bad));
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

extern "C" int ssi_attn_decode(const void* qkv, int64_t ld, const void* k_cache, const void* v_cache, int64_t n_slots, int64_t cap,
                               const int32_t* slot, const int32_t* kv_len, void* out, float* lse, int64_t rows, int n_heads, int n_kv,
                               int head_dim, int32_t* n_bad, int dtype, void* stream) {
    SSI_CHECK_ARG(rows >= 0 && n_slots >= 0 && cap >= 0 && cap < (1LL << 31) && (dtype == SSI_F32 || dtype == SSI_BF16));
    if (int rc = check_geometry("ssi_attn_decode", n_heads, n_kv, head_dim)) return rc;
    if (rows == 0) return SSI_OK;
    if (int rc = check_decode_args(qkv, ld, k_cache, v_cache, n_slots, cap, slot, kv_len, out, rows, n_heads, head_dim, dtype)) return rc;
#define SSI_DECODE_G(GG) launch_decode<T, GG>(qkv, ld, k_cache, v_cache, n_slots, cap, slot, kv_len, out, lse, rows, n_heads, n_kv, head_dim, n_bad, stream)
    SSI_DISPATCH_DTYPE(dtype, SSI_DECODE_FORMS(n_heads / n_kv, SSI_DECODE_G));
#undef SSI_DECODE_G
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

extern "C" int ssi_attn_decode_beam(const void* qkv, int64_t ld, const void* pk_cache, const void* pv_cache, int64_t n_pslots, int64_t cap_p,
                                    const void* bk_cache, const void* bv_cache, int64_t n_bslots, int64_t cap_b, const int32_t* prompt_slot,
                                    const int32_t* prompt_len, const int32_t* gen_len, const int32_t* anc, int64_t ld_anc, void* out, float* lse,
                                    int64_t rows, int n_heads, int n_kv, int head_dim, int32_t* n_bad, int dtype, void* stream) {
    SSI_CHECK_ARG(rows >= 0 && n_pslots >= 0 && cap_p >= 0 && n_bslots >= 0 && cap_b >= 0 && ld_anc >= 0 && (dtype == SSI_F32 || dtype == SSI_BF16));
    SSI_CHECK_ARG(cap_p + cap_b < (1LL << 31) && n_bslots < (1LL << 31));
    if (int rc = check_geometry("ssi_attn_decode_beam", n_heads, n_kv, head_dim)) return rc;
    if (rows == 0) return SSI_OK;
    if (int rc = check_beam_args(qkv, ld, pk_cache, pv_cache, n_pslots, cap_p, bk_cache, bv_cache, n_bslots, cap_b, prompt_slot, prompt_len, gen_len,
                                 anc, ld_anc, out, rows, n_heads, head_dim, dtype)) return rc;
    const int64_t cap_b_eff = (bk_cache && bv_cache && anc) ? cap_b : 0, n_ps_eff = (pk_cache && pv_cache) ? n_pslots : 0;
#define SSI_DECODE_G(GG)                                                                                                                          \
    launch_decode_beam<T, GG>(qkv, ld, pk_cache, pv_cache, n_ps_eff, cap_p, bk_cache, bv_cache, n_bslots, cap_b_eff, prompt_slot, prompt_len, gen_len, \
                              anc, ld_anc, out, lse, rows, n_heads, n_kv, head_dim, n_bad, stream)
    SSI_DISPATCH_DTYPE(dtype, SSI_DECODE_FORMS(n_heads / n_kv, SSI_DECODE_G));
#undef SSI_DECODE_G
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

extern "C" int ssi_attn_decode_split_span(int head_dim, int dtype) {
    const int round = decode_round(head_dim, dtype);
    return round > DEC_SPLIT_SPAN ? round : round ? DEC_SPLIT_SPAN : 0;
}

extern "C" int64_t ssi_attn_decode_split_workspace(int64_t rows, int n_heads, int head_dim, int64_t n_splits) {
    if (rows < 0 || n_heads < 1 || head_dim < 1 || n_splits < 1) return 0;
    return rows * n_heads * n_splits * (head_dim + 2) * (int64_t)sizeof(float);
}

extern "C" int ssi_attn_decode_split(const void* qkv, int64_t ld, const void* k_cache, const void* v_cache, int64_t n_slots, int64_t cap,
                                     const int32_t* slot, const int32_t* kv_len, void* out, float* lse, int64_t rows, int n_heads, int n_kv,
                                     int head_dim, int32_t* n_bad, int64_t span, int64_t n_splits, void* workspace, int64_t workspace_bytes,
                                     int dtype, void* stream) {
    SSI_CHECK_ARG(rows >= 0 && n_slots >= 0 && cap >= 0 && cap < (1LL << 31) && (dtype == SSI_F32 || dtype == SSI_BF16));
    if (int rc = check_geometry("ssi_attn_decode_split", n_heads, n_kv, head_dim)) return rc;
    if (int rc = check_split_args(span, n_splits, cap, workspace, workspace_bytes, rows, n_heads, head_dim, dtype)) return rc;
    if (rows == 0) return SSI_OK;
    if (int rc = check_decode_args(qkv, ld, k_cache, v_cache, n_slots, cap, slot, kv_len, out, rows, n_heads, head_dim, dtype)) return rc;
#define SSI_DECODE_G(GG)                                                                                                                           \
    launch_split<T, GG>(qkv, ld, k_cache, v_cache, n_slots, cap, slot, kv_len, (float*)workspace, span, n_splits, rows, n_heads, n_kv, head_dim, stream)
    SSI_DISPATCH_DTYPE(dtype, {
        SSI_DECODE_FORMS(n_heads / n_kv, SSI_DECODE_G);
        launch_split_merge<T>((const float*)workspace, span, n_splits, slot, n_slots, kv_len, cap, nullptr, 0, out, lse, rows, n_heads, n_kv, head_dim,
                              n_bad, stream);
    });
#undef SSI_DECODE_G
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

extern "C" int ssi_attn_decode_beam_split(const void* qkv, int64_t ld, const void* pk_cache, const void* pv_cache, int64_t n_pslots, int64_t cap_p,
                                          const void* bk_cache, const void* bv_cache, int64_t n_bslots, int64_t cap_b, const int32_t* prompt_slot,
                                          const int32_t* prompt_len, const int32_t* gen_len, const int32_t* anc, int64_t ld_anc, void* out,
                                          float* lse, int64_t rows, int n_heads, int n_kv, int head_dim, int32_t* n_bad, int64_t span,
                                          int64_t n_splits, void* workspace, int64_t workspace_bytes, int dtype, void* stream) {
    SSI_CHECK_ARG(rows >= 0 && n_pslots >= 0 && cap_p >= 0 && n_bslots >= 0 && cap_b >= 0 && ld_anc >= 0 && (dtype == SSI_F32 || dtype == SSI_BF16));
    SSI_CHECK_ARG(cap_p + cap_b < (1LL << 31) && n_bslots < (1LL << 31));
    if (int rc = check_geometry("ssi_attn_decode_beam_split", n_heads, n_kv, head_dim)) return rc;
    if (int rc = check_split_args(span, n_splits, cap_p + (cap_b < ld_anc ? cap_b : ld_anc), workspace, workspace_bytes, rows, n_heads, head_dim, dtype))
        return rc;
    if (rows == 0) return SSI_OK;
    if (int rc = check_beam_args(qkv, ld, pk_cache, pv_cache, n_pslots, cap_p, bk_cache, bv_cache, n_bslots, cap_b, prompt_slot, prompt_len, gen_len,
                                 anc, ld_anc, out, rows, n_heads, head_dim, dtype)) return rc;
    const int64_t cap_b_eff = (bk_cache && bv_cache && anc) ? cap_b : 0, n_ps_eff = (pk_cache && pv_cache) ? n_pslots : 0;
    const int64_t gen_cap = cap_b_eff < ld_anc ? cap_b_eff : ld_anc;
#define SSI_DECODE_G(GG)                                                                                                                          \
    launch_split_beam<T, GG>(qkv, ld, pk_cache, pv_cache, n_ps_eff, cap_p, bk_cache, bv_cache, n_bslots, cap_b_eff, prompt_slot, prompt_len, gen_len, \
                             anc, ld_anc, (float*)workspace, span, n_splits, rows, n_heads, n_kv, head_dim, n_bad, stream)
    SSI_DISPATCH_DTYPE(dtype, {
        SSI_DECODE_FORMS(n_heads / n_kv, SSI_DECODE_G);
        launch_split_merge<T>((const float*)workspace, span, n_splits, prompt_slot, INT64_MAX, prompt_len, cap_p, gen_len, gen_cap, out, lse, rows,
                              n_heads, n_kv, head_dim, nullptr, stream);
    });
#undef SSI_DECODE_G
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}
