// Generation (ABI v18): the K/V cache of a decode step.  ssi_kv_store scatters the k / v columns of qkv rows into the cache,
// ssi_attn_decode is single-query attention of one new token per sequence over that sequence's cached keys.  ssi_attn_decode_beam (ABI v20)
// reads the generated keys through an ancestry table; ssi_attn_decode_split / ssi_attn_decode_beam_split (ABI v25) split a row's keys over
// workgroups and merge the partial softmax states in a second launch.  All of them share one walk (dec_walk, dec_merged) and one finish (dec_finish).
//
// The cache of one layer: k_cache and v_cache, each [n_slots, cap, n_kv * head_dim] in the model's dtype, K after RoPE (as it sits in qkv).
// The *_fp8 entries (ABI v26) keep it as e4m3 codes with one power-of-two exponent byte per (position, kv head) instead (the header's "FP8 K/V
// cache"): ssi_kv_store_fp8 quantises, and the four attention entries run the same walk with a storage policy that hands it dequantised values.
#include "common_hip.h"
#include "q8_codes.h"
#include <math.h>

namespace {

typedef uint32_t q8_u32x2 __attribute__((ext_vector_type(2)));   // the 8 codes of a bf16 lane

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
// ssi_kv_store_fp8 (ABI v26): the same scatter, every line quantised on its way (the header's "FP8 K/V cache").  A line (one kv head of k or
// of v of one row) lies on LPK = 2^lpk_log2 >= head_dim / VEC lanes of one wave, 16 bytes of qkv each (lanes whose columns lie past head_dim
// idle, as in the decode kernels); its absmax is an xor-shuffle maximum of the lanes' |x| bit patterns (finite magnitudes order as unsigned
// integers), every lane then scales (v_ldexp_f32: exact), converts (v_cvt_pk_fp8_f32: RNE) and writes its VEC codes at once, and the line's first
// lane writes the exponent byte.  What leaves the kernel early does so for whole lines, so every shuffle meets live lanes only.
// =====================================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void q8_store_kernel(const T* __restrict__ qkv, int64_t ld, const int64_t* __restrict__ dest, int64_t rows,
                                                       int64_t n_dest, uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, uint8_t* __restrict__ ke,
                                                       uint8_t* __restrict__ ve, int q_cols, int n_kv, int hd, int lpk_log2,
                                                       int32_t* __restrict__ n_bad) {
    constexpr int VEC = Vec16<T>::N, WORDS = VEC / 4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t line = i >> lpk_log2;                   // of rows * 2 * n_kv lines: a row's k heads, then its v heads
    const int sub = (int)(i & ((1 << lpk_log2) - 1)), col = sub * VEC;
    const int64_t r = line / (2 * n_kv);
    if (r >= rows) return;
    const int c = (int)(line - r * (2 * n_kv));
    const int64_t d = dest[r];
    if (d == -1) return;
    if (d < 0 || d >= n_dest) {
        if (c == 0 && sub == 0 && n_bad) atomicAdd(n_bad, 1);
        return;
    }
    const bool active = col < hd;
    Vec16<T> x = {};
    if (active) x = load16<T>(qkv + r * ld + q_cols + (int64_t)c * hd + col);
    float f[VEC];
    uint32_t a = 0;                                       // the bits of the largest finite |x|
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        f[v] = x.get(v);
        a = q8_absmax_bits(a, f[v]);
    }
    for (int o = 1 << lpk_log2 >> 1; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)a, o, 64);
        a = other > a ? other : a;
    }
    const int b = q8_exponent_byte(a);
    if (!active) return;
    uint32_t w[WORDS];
#pragma unroll
    for (int k = 0; k < WORDS; ++k) w[k] = q8_encode4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3], b);
    const bool is_k = c < n_kv;
    const int64_t at = d * n_kv + (is_k ? c : c - n_kv);
    uint8_t* dst = (is_k ? kc : vc) + at * hd + col;
    if constexpr (WORDS == 2) {
        q8_u32x2 o2;
        o2[0] = w[0];
        o2[1] = w[1];
        *reinterpret_cast<q8_u32x2*>(dst) = o2;
    } else {
        *reinterpret_cast<uint32_t*>(dst) = w[0];
    }
    if (sub == 0) (is_k ? ke : ve)[at] = (uint8_t)b;
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
// state as it was — and ``keys.load(j, kx, vx)`` loads the lane's VEC elements of its K and V lines as they are stored (``Keys::Raw``);
// ``Keys::unpack`` turns them into the fp32 values the walk computes with.  Without CAN_SKIP the caller promises n > k0 keys that all exist.
// ``qrow``: the row's first query head of this kv head.
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
        typename Keys::Raw kx[DEC_U] = {}, vx[DEC_U] = {};
        bool have[DEC_U];
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {                 // every load of the chunk is issued before the first use
            const int j = base + u * kpw + kslot;
            have[u] = j < n;
            if (CAN_SKIP) have[u] = have[u] && keys.exists(j);
            if (have[u] && active) keys.load(j, kx[u], vx[u]);
        }
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const bool ld_ok = have[u] && active;
            float kf[VEC], vf[VEC];
            Keys::unpack(kx[u], kf);
            Keys::unpack(vx[u], vf);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                kf[v] = ld_ok ? kf[v] : 0.f;
                vf[v] = ld_ok ? vf[v] : 0.f;
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

// =====================================================================================================================
// HOW A CACHE IS STORED.  A kernel is handed a cache (PlainCache, Q8Cache); ``lines`` gives one lane its view of one kv head from cached
// position ``first`` on (position p of slot s is cached position s * cap + p): ``load(p, kx, vx)`` loads the lane's VEC elements of the K and
// V lines of cached position p as they are stored, ``unpack`` makes them the fp32 values of the walk.
// =====================================================================================================================
template <typename T>
struct PlainLines {
    using Raw = Vec16<T>;
    const T *k, *v;                                       // the cache
    int64_t at, kv_cols;                                  // cached position 0 of the view, the kv head, the lane's columns; elements per position
    __device__ __forceinline__ void load(int64_t p, Raw& kx, Raw& vx) const {
        const int64_t off = p * kv_cols + at;
        kx = load16_nt<T>(k + off);
        vx = load16_nt<T>(v + off);
    }
    static __device__ __forceinline__ void unpack(const Raw& x, float (&f)[Vec16<T>::N]) {
#pragma unroll
        for (int i = 0; i < Vec16<T>::N; ++i) f[i] = x.get(i);
    }
};
template <typename T>
struct PlainCache {
    using Lines = PlainLines<T>;
    const T *k, *v;
    __device__ __forceinline__ Lines lines(int64_t first, int n_kv, int kvh, int hd, int col) const {
        return {k, v, (first * n_kv + kvh) * hd + col, (int64_t)n_kv * hd};
    }
};

// The fp8 cache (ABI v26): a lane's VEC codes are VEC / 4 words, loaded at once (8 bytes for bf16, 4 for fp32: the plain form's lane layout),
// and the line's exponent byte b.  The value of a code is float(code) * 2^(b - 127), made ELEMENT BY ELEMENT here (v_cvt_pk_f32_fp8, then
// v_ldexp_f32: both exact), so the walk sees the very fp32 values it sees on a plain cache that holds the dequantised lines, whatever their
// magnitude — a scale applied to the score and to p instead would round differently where a product overflows or goes subnormal, and would
// save only 2 * VEC v_ldexp_f32 a key beside the 2 * G * VEC v_fma_f32 the walk spends on it.
template <typename T>
struct Q8Lines {
    static constexpr int VEC = Vec16<T>::N, WORDS = VEC / 4;
    struct Raw {
        uint32_t c[WORDS];
        uint32_t b;
    };
    const uint8_t *k, *v;                                 // codes: cached position 0 of the view, the kv head, the lane's columns
    const uint8_t *ke, *ve;                               // exponent bytes: cached position 0 of the view, the kv head
    int64_t kv_cols;
    int n_kv;
    static __device__ __forceinline__ void codes(const uint8_t* p, uint32_t (&c)[WORDS]) {
        if constexpr (WORDS == 2) {
            const q8_u32x2 x = __builtin_nontemporal_load(reinterpret_cast<const q8_u32x2*>(p));
            c[0] = x[0];
            c[1] = x[1];
        } else {
            c[0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
        }
    }
    __device__ __forceinline__ void load(int64_t p, Raw& kx, Raw& vx) const {
        codes(k + p * kv_cols, kx.c);
        codes(v + p * kv_cols, vx.c);
        kx.b = ke[p * n_kv];
        vx.b = ve[p * n_kv];
    }
    static __device__ __forceinline__ void unpack(const Raw& x, float (&f)[VEC]) {
        const int e = (int)x.b - 127;
#pragma unroll
        for (int w = 0; w < WORDS; ++w) q8_decode4(x.c[w], e, f + 4 * w);
    }
};
template <typename T>
struct Q8Cache {
    using Lines = Q8Lines<T>;
    const uint8_t *k, *v, *ke, *ve;
    __device__ __forceinline__ Lines lines(int64_t first, int n_kv, int kvh, int hd, int col) const {
        const int64_t line = first * n_kv + kvh;
        return {k + line * hd + col, v + line * hd + col, ke + line, ve + line, (int64_t)n_kv * hd, n_kv};
    }
};

// the keys of one cache slot, one behind the other (``at``: the slot's position 0)
template <typename L>
struct SlotKeys {
    using Raw = typename L::Raw;
    L at;
    __device__ __forceinline__ bool exists(int) const { return true; }
    __device__ __forceinline__ void load(int j, Raw& kx, Raw& vx) const { at.load(j, kx, vx); }
    template <int N>
    static __device__ __forceinline__ void unpack(const Raw& x, float (&f)[N]) { L::unpack(x, f); }
};

// one (row, kv head) of ssi_attn_decode on a cache stored as ``C``
template <typename T, int G, typename C>
__device__ __forceinline__ void slot_decode(const T* __restrict__ qkv, int64_t ld, const C& cache, int64_t n_slots, int cap,
                                            const int32_t* __restrict__ slot, const int32_t* __restrict__ kv_len, T* __restrict__ out,
                                            float* __restrict__ lse, int n_heads, int n_kv, int hd, int g, int lpk_log2, float qscale,
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
    const SlotKeys<typename C::Lines> keys{cache.lines((int64_t)sl * cap, n_kv, kvh, hd, at.col)};
    dec_row<T, G, false>(qkv + r * ld + (int64_t)h0 * hd, n, orow, lse, r * n_heads + h0, hd, g, at, qscale, keys);
}

template <typename T, int G>
__global__ __launch_bounds__(256) void kv_decode_kernel(const T* __restrict__ qkv, int64_t ld, const T* __restrict__ kc, const T* __restrict__ vc,
                                                        int64_t n_slots, int cap, const int32_t* __restrict__ slot,
                                                        const int32_t* __restrict__ kv_len, T* __restrict__ out, float* __restrict__ lse,
                                                        int n_heads, int n_kv, int hd, int g, int lpk_log2, float qscale,
                                                        int32_t* __restrict__ n_bad) {
    slot_decode<T, G>(qkv, ld, PlainCache<T>{kc, vc}, n_slots, cap, slot, kv_len, out, lse, n_heads, n_kv, hd, g, lpk_log2, qscale, n_bad);
}

template <typename T, int G>
__global__ __launch_bounds__(256) void q8_decode_kernel(const T* __restrict__ qkv, int64_t ld, Q8Cache<T> cache, int64_t n_slots, int cap,
                                                        const int32_t* __restrict__ slot, const int32_t* __restrict__ kv_len,
                                                        T* __restrict__ out, float* __restrict__ lse, int n_heads, int n_kv, int hd, int g,
                                                        int lpk_log2, float qscale, int32_t* __restrict__ n_bad) {
    slot_decode<T, G>(qkv, ld, cache, n_slots, cap, slot, kv_len, out, lse, n_heads, n_kv, hd, g, lpk_log2, qscale, n_bad);
}

// =====================================================================================================================
// ssi_attn_decode_beam (ABI v20): the same row over the concatenation of two key ranges — the np keys of a PROMPT cache slot, then ng keys of a
// BEAM cache read through an ancestry table: generated position i of row r lies in beam slot anc[r, i], at position i.  Key j of the walk
// is prompt key j for j < np and generated key j - np otherwise, so chunks, waves and merges are those of kv_decode_kernel on a cache that
// holds the row's keys one behind the other, and so are the bits.  An index outside its cache is never turned into an address: the key is
// skipped, and the row is counted once.
// =====================================================================================================================
// prompt keys 0 .. np - 1 of one prompt cache slot, then generated keys: position i of the beam cache slot the ancestry names
template <typename L>
struct BeamKeys {
    using Raw = typename L::Raw;
    L prompt;                                             // the prompt slot's position 0 (never used when !p_ok)
    L beam;                                               // the beam cache's position 0
    const int32_t* arow;                                  // the row's ancestry
    int np, cap_b, n_bslots;
    bool p_ok;
    __device__ __forceinline__ bool exists(int j) const {
        if (j < np) return p_ok;
        const int a = arow[j - np];
        return a >= 0 && a < n_bslots;                    // checked before any address is formed from it
    }
    __device__ __forceinline__ void load(int j, Raw& kx, Raw& vx) const {   // (only for a key that exists)
        if (j < np) {
            prompt.load(j, kx, vx);
        } else {
            const int i = j - np;
            beam.load((int64_t)arow[i] * cap_b + i, kx, vx);
        }
    }
    template <int N>
    static __device__ __forceinline__ void unpack(const Raw& x, float (&f)[N]) { L::unpack(x, f); }
};

// one (row, kv head) of ssi_attn_decode_beam on a prompt cache and a beam cache stored as ``C``
template <typename T, int G, typename C>
__device__ __forceinline__ void beam_decode(const T* __restrict__ qkv, int64_t ld, const C& pcache, int64_t n_pslots, int cap_p, const C& bcache,
                                            int64_t n_bslots, int cap_b, const int32_t* __restrict__ prompt_slot,
                                            const int32_t* __restrict__ prompt_len, const int32_t* __restrict__ gen_len,
                                            const int32_t* __restrict__ anc, int64_t ld_anc, T* __restrict__ out, float* __restrict__ lse,
                                            int n_heads, int n_kv, int hd, int g, int lpk_log2, float qscale, int32_t* __restrict__ n_bad) {
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
    const DecLane at = dec_lane<T>(lpk_log2, hd);
    const BeamKeys<typename C::Lines> keys{pcache.lines((int64_t)(p_ok ? sl : 0) * cap_p, n_kv, kvh, hd, at.col),
                                           bcache.lines(0, n_kv, kvh, hd, at.col), anc + r * ld_anc, np, cap_b, (int)n_bslots, p_ok};
    dec_row<T, G, true>(qkv + r * ld + (int64_t)h0 * hd, np + ng, orow, lse, r * n_heads + h0, hd, g, at, qscale, keys);
    if (kvh == 0 && n_bad) {                              // once per row (every kv head meets the same indices): the ancestry alone once more
        bool bad = !p_ok && np > 0;
        for (int i = tid; i < ng; i += 256) bad |= !keys.exists(np + i);
        const int any = __syncthreads_or(bad ? 1 : 0);
        if (tid == 0 && any) atomicAdd(n_bad, 1);
    }
}

template <typename T, int G>
__global__ __launch_bounds__(256) void beam_decode_kernel(const T* __restrict__ qkv, int64_t ld, const T* __restrict__ pk, const T* __restrict__ pv,
                                                          int64_t n_pslots, int cap_p, const T* __restrict__ bk, const T* __restrict__ bv,
                                                          int64_t n_bslots, int cap_b, const int32_t* __restrict__ prompt_slot,
                                                          const int32_t* __restrict__ prompt_len, const int32_t* __restrict__ gen_len,
                                                          const int32_t* __restrict__ anc, int64_t ld_anc, T* __restrict__ out,
                                                          float* __restrict__ lse, int n_heads, int n_kv, int hd, int g, int lpk_log2, float qscale,
                                                          int32_t* __restrict__ n_bad) {
    beam_decode<T, G>(qkv, ld, PlainCache<T>{pk, pv}, n_pslots, cap_p, PlainCache<T>{bk, bv}, n_bslots, cap_b, prompt_slot, prompt_len, gen_len, anc,
                      ld_anc, out, lse, n_heads, n_kv, hd, g, lpk_log2, qscale, n_bad);
}

template <typename T, int G>
__global__ __launch_bounds__(256) void q8_beam_kernel(const T* __restrict__ qkv, int64_t ld, Q8Cache<T> pcache, int64_t n_pslots, int cap_p,
                                                      Q8Cache<T> bcache, int64_t n_bslots, int cap_b, const int32_t* __restrict__ prompt_slot,
                                                      const int32_t* __restrict__ prompt_len, const int32_t* __restrict__ gen_len,
                                                      const int32_t* __restrict__ anc, int64_t ld_anc, T* __restrict__ out, float* __restrict__ lse,
                                                      int n_heads, int n_kv, int hd, int g, int lpk_log2, float qscale,
                                                      int32_t* __restrict__ n_bad) {
    beam_decode<T, G>(qkv, ld, pcache, n_pslots, cap_p, bcache, n_bslots, cap_b, prompt_slot, prompt_len, gen_len, anc, ld_anc, out, lse, n_heads,
                      n_kv, hd, g, lpk_log2, qscale, n_bad);
}

// =====================================================================================================================
// ssi_attn_decode_split / ssi_attn_decode_beam_split (ABI v25): the keys of a (row, kv head) over several workgroups.  Workgroup z of a row
// with n keys walks the keys [z * span, min((z + 1) * span, n)) as the plain kernel walks a cache that starts there, and writes its merged,
// unnormalised state to the workspace [rows, n_heads, n_splits, head_dim + 2]; a merge kernel behind it on the stream applies the four-wave
// merge's formula over the row's ceil(n / span) partials in the order z = 0, 1, ... and finishes.  No atomics but the error count, no flag,
// no ticket: the kernel boundary is the only synchronisation.
// =====================================================================================================================
template <typename T, int G, typename C>
__device__ __forceinline__ void split_slot_walk(const T* __restrict__ qkv, int64_t ld, const C& cache, int64_t n_slots, int cap,
                                                const int32_t* __restrict__ slot, const int32_t* __restrict__ kv_len, float* __restrict__ ws,
                                                int64_t span, int n_heads, int n_kv, int hd, int g, int lpk_log2, float qscale) {
    const int64_t r = blockIdx.x, k0 = (int64_t)blockIdx.z * span;
    const int kvh = blockIdx.y, h0 = kvh * g;
    const int sl = slot[r];
    int n = kv_len[r];
    n = n < cap ? n : cap;
    if (sl < 0 || sl >= n_slots || k0 >= n) return;       // (uniform over the workgroup; n <= 0 is among them: the merge writes such a row)
    const int n_end = k0 + span < n ? (int)(k0 + span) : n;
    const DecLane at = dec_lane<T>(lpk_log2, hd);
    const SlotKeys<typename C::Lines> keys{cache.lines((int64_t)sl * cap, n_kv, kvh, hd, at.col)};
    float* part = ws + (((r * n_heads + h0) * gridDim.z) + blockIdx.z) * (hd + 2);
    dec_part<T, G, false>(qkv + r * ld + (int64_t)h0 * hd, (int)k0, n_end, part, (int64_t)gridDim.z * (hd + 2), hd, g, at, qscale, keys);
}

template <typename T, int G>
__global__ __launch_bounds__(256) void split_kv_walk_kernel(const T* __restrict__ qkv, int64_t ld, const T* __restrict__ kc, const T* __restrict__ vc,
                                                            int64_t n_slots, int cap, const int32_t* __restrict__ slot,
                                                            const int32_t* __restrict__ kv_len, float* __restrict__ ws, int64_t span, int n_heads,
                                                            int n_kv, int hd, int g, int lpk_log2, float qscale) {
    split_slot_walk<T, G>(qkv, ld, PlainCache<T>{kc, vc}, n_slots, cap, slot, kv_len, ws, span, n_heads, n_kv, hd, g, lpk_log2, qscale);
}

template <typename T, int G>
__global__ __launch_bounds__(256) void q8_split_walk_kernel(const T* __restrict__ qkv, int64_t ld, Q8Cache<T> cache, int64_t n_slots, int cap,
                                                            const int32_t* __restrict__ slot, const int32_t* __restrict__ kv_len,
                                                            float* __restrict__ ws, int64_t span, int n_heads, int n_kv, int hd, int g,
                                                            int lpk_log2, float qscale) {
    split_slot_walk<T, G>(qkv, ld, cache, n_slots, cap, slot, kv_len, ws, span, n_heads, n_kv, hd, g, lpk_log2, qscale);
}

template <typename T, int G, typename C>
__device__ __forceinline__ void split_beam_walk(const T* __restrict__ qkv, int64_t ld, const C& pcache, int64_t n_pslots, int cap_p, const C& bcache,
                                                int64_t n_bslots, int cap_b, const int32_t* __restrict__ prompt_slot,
                                                const int32_t* __restrict__ prompt_len, const int32_t* __restrict__ gen_len,
                                                const int32_t* __restrict__ anc, int64_t ld_anc, float* __restrict__ ws, int64_t span, int n_heads,
                                                int n_kv, int hd, int g, int lpk_log2, float qscale, int32_t* __restrict__ n_bad) {
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
    const DecLane at = dec_lane<T>(lpk_log2, hd);
    const BeamKeys<typename C::Lines> keys{pcache.lines((int64_t)(p_ok ? sl : 0) * cap_p, n_kv, kvh, hd, at.col),
                                           bcache.lines(0, n_kv, kvh, hd, at.col), anc + r * ld_anc, np, cap_b, (int)n_bslots, p_ok};
    float* part = ws + (((r * n_heads + h0) * gridDim.z) + blockIdx.z) * (hd + 2);
    dec_part<T, G, true>(qkv + r * ld + (int64_t)h0 * hd, (int)k0, n_end, part, (int64_t)gridDim.z * (hd + 2), hd, g, at, qscale, keys);
    if (kvh == 0 && blockIdx.z == 0 && n_bad) {           // once per row, over the whole ancestry: beam_decode_kernel's count
        bool bad = !p_ok && np > 0;
        for (int i = tid; i < ng; i += 256) bad |= !keys.exists(np + i);
        const int any = __syncthreads_or(bad ? 1 : 0);
        if (tid == 0 && any) atomicAdd(n_bad, 1);
    }
}

template <typename T, int G>
__global__ __launch_bounds__(256) void split_beam_walk_kernel(const T* __restrict__ qkv, int64_t ld, const T* __restrict__ pk, const T* __restrict__ pv,
                                                              int64_t n_pslots, int cap_p, const T* __restrict__ bk, const T* __restrict__ bv,
                                                              int64_t n_bslots, int cap_b, const int32_t* __restrict__ prompt_slot,
                                                              const int32_t* __restrict__ prompt_len, const int32_t* __restrict__ gen_len,
                                                              const int32_t* __restrict__ anc, int64_t ld_anc, float* __restrict__ ws, int64_t span,
                                                              int n_heads, int n_kv, int hd, int g, int lpk_log2, float qscale,
                                                              int32_t* __restrict__ n_bad) {
    split_beam_walk<T, G>(qkv, ld, PlainCache<T>{pk, pv}, n_pslots, cap_p, PlainCache<T>{bk, bv}, n_bslots, cap_b, prompt_slot, prompt_len, gen_len,
                          anc, ld_anc, ws, span, n_heads, n_kv, hd, g, lpk_log2, qscale, n_bad);
}

template <typename T, int G>
__global__ __launch_bounds__(256) void q8_split_beam_kernel(const T* __restrict__ qkv, int64_t ld, Q8Cache<T> pcache, int64_t n_pslots, int cap_p,
                                                            Q8Cache<T> bcache, int64_t n_bslots, int cap_b,
                                                            const int32_t* __restrict__ prompt_slot, const int32_t* __restrict__ prompt_len,
                                                            const int32_t* __restrict__ gen_len, const int32_t* __restrict__ anc, int64_t ld_anc,
                                                            float* __restrict__ ws, int64_t span, int n_heads, int n_kv, int hd, int g,
                                                            int lpk_log2, float qscale, int32_t* __restrict__ n_bad) {
    split_beam_walk<T, G>(qkv, ld, pcache, n_pslots, cap_p, bcache, n_bslots, cap_b, prompt_slot, prompt_len, gen_len, anc, ld_anc, ws, span, n_heads,
                          n_kv, hd, g, lpk_log2, qscale, n_bad);
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

// A cache as an entry hands it to a launcher: the model-dtype form (k, v), or with ``q8`` codes (k, v) and exponent bytes (ke, ve).
struct CacheArg {
    const void *k, *v, *ke, *ve;
    bool q8;
    bool there() const { return k && v && (!q8 || (ke && ve)); }
};
template <typename T>
Q8Cache<T> q8_cache(const CacheArg& c) {
    return {(const uint8_t*)c.k, (const uint8_t*)c.v, (const uint8_t*)c.ke, (const uint8_t*)c.ve};
}

// lanes of a key (a power of two) and the scale of q: the same for both storage forms
template <typename T>
int lanes_log2(int hd) {
    int lpk_log2 = 0;
    while ((1 << lpk_log2) < hd / Vec16<T>::N) ++lpk_log2;
    return lpk_log2;
}
float decode_qscale(int hd) { return (float)(1.4426950408889634 / sqrt((double)hd)); }

template <typename T, int G>
void launch_decode(const void* qkv, int64_t ld, const CacheArg& c, int64_t n_slots, int64_t cap, const int32_t* slot, const int32_t* kv_len, void* out,
                   float* lse, int64_t rows, int n_heads, int n_kv, int hd, int32_t* n_bad, void* stream) {
    const dim3 grid((unsigned)rows, (unsigned)n_kv);
    if (c.q8)
        hipLaunchKernelGGL((q8_decode_kernel<T, G>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)qkv, ld, q8_cache<T>(c), n_slots, (int)cap, slot,
                           kv_len, (T*)out, lse, n_heads, n_kv, hd, n_heads / n_kv, lanes_log2<T>(hd), decode_qscale(hd), n_bad);
    else
        hipLaunchKernelGGL((kv_decode_kernel<T, G>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)qkv, ld, (const T*)c.k, (const T*)c.v, n_slots,
                           (int)cap, slot, kv_len, (T*)out, lse, n_heads, n_kv, hd, n_heads / n_kv, lanes_log2<T>(hd), decode_qscale(hd), n_bad);
}

template <typename T, int G>
void launch_decode_beam(const void* qkv, int64_t ld, const CacheArg& p, int64_t n_pslots, int64_t cap_p, const CacheArg& b, int64_t n_bslots,
                        int64_t cap_b, const int32_t* prompt_slot, const int32_t* prompt_len, const int32_t* gen_len, const int32_t* anc,
                        int64_t ld_anc, void* out, float* lse, int64_t rows, int n_heads, int n_kv, int hd, int32_t* n_bad, void* stream) {
    const dim3 grid((unsigned)rows, (unsigned)n_kv);
    if (p.q8)
        hipLaunchKernelGGL((q8_beam_kernel<T, G>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)qkv, ld, q8_cache<T>(p), n_pslots, (int)cap_p,
                           q8_cache<T>(b), n_bslots, (int)cap_b, prompt_slot, prompt_len, gen_len, anc, ld_anc, (T*)out, lse, n_heads, n_kv, hd,
                           n_heads / n_kv, lanes_log2<T>(hd), decode_qscale(hd), n_bad);
    else
        hipLaunchKernelGGL((beam_decode_kernel<T, G>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)qkv, ld, (const T*)p.k, (const T*)p.v, n_pslots,
                           (int)cap_p, (const T*)b.k, (const T*)b.v, n_bslots, (int)cap_b, prompt_slot, prompt_len, gen_len, anc, ld_anc, (T*)out, lse,
                           n_heads, n_kv, hd, n_heads / n_kv, lanes_log2<T>(hd), decode_qscale(hd), n_bad);
}

template <typename T, int G>
void launch_split(const void* qkv, int64_t ld, const CacheArg& c, int64_t n_slots, int64_t cap, const int32_t* slot, const int32_t* kv_len, float* ws,
                  int64_t span, int64_t n_splits, int64_t rows, int n_heads, int n_kv, int hd, void* stream) {
    const dim3 grid((unsigned)rows, (unsigned)n_kv, (unsigned)n_splits);
    if (c.q8)
        hipLaunchKernelGGL((q8_split_walk_kernel<T, G>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)qkv, ld, q8_cache<T>(c), n_slots, (int)cap,
                           slot, kv_len, ws, span, n_heads, n_kv, hd, n_heads / n_kv, lanes_log2<T>(hd), decode_qscale(hd));
    else
        hipLaunchKernelGGL((split_kv_walk_kernel<T, G>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)qkv, ld, (const T*)c.k, (const T*)c.v,
                           n_slots, (int)cap, slot, kv_len, ws, span, n_heads, n_kv, hd, n_heads / n_kv, lanes_log2<T>(hd), decode_qscale(hd));
}

template <typename T, int G>
void launch_split_beam(const void* qkv, int64_t ld, const CacheArg& p, int64_t n_pslots, int64_t cap_p, const CacheArg& b, int64_t n_bslots,
                       int64_t cap_b, const int32_t* prompt_slot, const int32_t* prompt_len, const int32_t* gen_len, const int32_t* anc, int64_t ld_anc,
                       float* ws, int64_t span, int64_t n_splits, int64_t rows, int n_heads, int n_kv, int hd, int32_t* n_bad, void* stream) {
    const dim3 grid((unsigned)rows, (unsigned)n_kv, (unsigned)n_splits);
    if (p.q8)
        hipLaunchKernelGGL((q8_split_beam_kernel<T, G>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)qkv, ld, q8_cache<T>(p), n_pslots,
                           (int)cap_p, q8_cache<T>(b), n_bslots, (int)cap_b, prompt_slot, prompt_len, gen_len, anc, ld_anc, ws, span, n_heads, n_kv, hd,
                           n_heads / n_kv, lanes_log2<T>(hd), decode_qscale(hd), n_bad);
    else
        hipLaunchKernelGGL((split_beam_walk_kernel<T, G>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)qkv, ld, (const T*)p.k, (const T*)p.v,
                           n_pslots, (int)cap_p, (const T*)b.k, (const T*)b.v, n_bslots, (int)cap_b, prompt_slot, prompt_len, gen_len, anc, ld_anc, ws,
                           span, n_heads, n_kv, hd, n_heads / n_kv, lanes_log2<T>(hd), decode_qscale(hd), n_bad);
}

template <typename T>
void launch_split_merge(const float* ws, int64_t span, int64_t n_splits, const int32_t* slot, int64_t slot_limit, const int32_t* len_a, int64_t cap_a,
                        const int32_t* len_b, int64_t cap_b, void* out, float* lse, int64_t rows, int n_heads, int n_kv, int hd, int32_t* n_bad,
                        void* stream) {
    hipLaunchKernelGGL(split_kv_merge_kernel<T>, dim3((unsigned)rows, (unsigned)n_kv), dim3(256), 0, (hipStream_t)stream, ws, span, n_splits, slot,
                       slot_limit, len_a, (int)cap_a, len_b, (int)cap_b, (T*)out, lse, n_heads, hd, n_heads / n_kv, n_bad);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// head geometry every entry accepts
int check_geometry(const char* who, int n_heads, int n_kv, int head_dim) {
    if (n_heads < 1 || n_kv < 1 || head_dim < 1) { ssi_set_error("%s: n_heads, n_kv and head_dim must be positive", who); return SSI_ERR_ARG; }
    if (n_heads % n_kv || n_heads / n_kv > 8 || head_dim % 8 || head_dim > DEC_MAX_HD || n_kv > 65535) {
        ssi_set_error("%s: unsupported head geometry (n_heads %d, n_kv %d, head_dim %d): head_dim a multiple of 8 up to %d, 1 to 8 query heads "
                      "per kv head", who, n_heads, n_kv, head_dim, DEC_MAX_HD);
        return SSI_ERR_UNSUPPORTED;
    }
    return SSI_OK;
}

// what ssi_attn_decode and its split form check alike (rows > 0); the exponent bytes of an fp8 cache need no alignment
int check_decode_args(const void* qkv, int64_t ld, const CacheArg& c, int64_t n_slots, int64_t cap, const int32_t* slot, const int32_t* kv_len,
                      const void* out, int64_t rows, int n_heads, int head_dim, int dtype) {
    const int64_t esize = dtype == SSI_BF16 ? 2 : 4;
    SSI_CHECK_ARG(qkv && slot && kv_len && out && rows < (1LL << 31) && ld >= (int64_t)n_heads * head_dim);
    SSI_CHECK_ARG(c.there() || n_slots * cap == 0);
    SSI_CHECK_ARG(aligned16(qkv) && aligned16(c.k) && aligned16(c.v) && (ld * esize) % 16 == 0);
    return SSI_OK;
}

// what ssi_attn_decode_beam and its split form check alike (rows > 0)
int check_beam_args(const void* qkv, int64_t ld, const CacheArg& p, int64_t n_pslots, int64_t cap_p, const CacheArg& b, int64_t n_bslots, int64_t cap_b,
                    const int32_t* prompt_slot, const int32_t* prompt_len, const int32_t* gen_len, const int32_t* anc, int64_t ld_anc, const void* out,
                    int64_t rows, int n_heads, int head_dim, int dtype) {
    const int64_t esize = dtype == SSI_BF16 ? 2 : 4;
    SSI_CHECK_ARG(qkv && prompt_slot && prompt_len && gen_len && out && rows < (1LL << 31) && ld >= (int64_t)n_heads * head_dim);
    SSI_CHECK_ARG(p.there() || n_pslots * cap_p == 0);
    SSI_CHECK_ARG((b.there() && anc) || n_bslots * cap_b * ld_anc == 0);
    SSI_CHECK_ARG(aligned16(qkv) && aligned16(p.k) && aligned16(p.v) && aligned16(b.k) && aligned16(b.v) && (ld * esize) % 16 == 0);
    return SSI_OK;
}

// keys per round of the four waves (8 loads of 64 / LPK keys) of a form, the unit of a split's span; 0: no such form.  (The fp8 forms keep the
// lane layout of the model's dtype: theirs is the same.)
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

// ---- the entries' bodies: an entry and its _fp8 form differ in the CacheArg they make of their arguments --------------------------------------
int decode_entry(const char* who, const void* qkv, int64_t ld, const CacheArg& c, int64_t n_slots, int64_t cap, const int32_t* slot,
                 const int32_t* kv_len, void* out, float* lse, int64_t rows, int n_heads, int n_kv, int head_dim, int32_t* n_bad, int dtype,
                 void* stream) {
    SSI_CHECK_ARG(rows >= 0 && n_slots >= 0 && cap >= 0 && cap < (1LL << 31) && (dtype == SSI_F32 || dtype == SSI_BF16));
    if (int rc = check_geometry(who, n_heads, n_kv, head_dim)) return rc;
    if (rows == 0) return SSI_OK;
    if (int rc = check_decode_args(qkv, ld, c, n_slots, cap, slot, kv_len, out, rows, n_heads, head_dim, dtype)) return rc;
#define SSI_DECODE_G(GG) launch_decode<T, GG>(qkv, ld, c, n_slots, cap, slot, kv_len, out, lse, rows, n_heads, n_kv, head_dim, n_bad, stream)
    SSI_DISPATCH_DTYPE(dtype, SSI_DECODE_FORMS(n_heads / n_kv, SSI_DECODE_G));
#undef SSI_DECODE_G
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

int beam_entry(const char* who, const void* qkv, int64_t ld, const CacheArg& p, int64_t n_pslots, int64_t cap_p, const CacheArg& b, int64_t n_bslots,
               int64_t cap_b, const int32_t* prompt_slot, const int32_t* prompt_len, const int32_t* gen_len, const int32_t* anc, int64_t ld_anc,
               void* out, float* lse, int64_t rows, int n_heads, int n_kv, int head_dim, int32_t* n_bad, int dtype, void* stream) {
    SSI_CHECK_ARG(rows >= 0 && n_pslots >= 0 && cap_p >= 0 && n_bslots >= 0 && cap_b >= 0 && ld_anc >= 0 && (dtype == SSI_F32 || dtype == SSI_BF16));
    SSI_CHECK_ARG(cap_p + cap_b < (1LL << 31) && n_bslots < (1LL << 31));
    if (int rc = check_geometry(who, n_heads, n_kv, head_dim)) return rc;
    if (rows == 0) return SSI_OK;
    if (int rc = check_beam_args(qkv, ld, p, n_pslots, cap_p, b, n_bslots, cap_b, prompt_slot, prompt_len, gen_len, anc, ld_anc, out, rows, n_heads,
                                 head_dim, dtype)) return rc;
    const int64_t cap_b_eff = (b.there() && anc) ? cap_b : 0, n_ps_eff = p.there() ? n_pslots : 0;
#define SSI_DECODE_G(GG)                                                                                                                          \
    launch_decode_beam<T, GG>(qkv, ld, p, n_ps_eff, cap_p, b, n_bslots, cap_b_eff, prompt_slot, prompt_len, gen_len, anc, ld_anc, out, lse, rows, \
                              n_heads, n_kv, head_dim, n_bad, stream)
    SSI_DISPATCH_DTYPE(dtype, SSI_DECODE_FORMS(n_heads / n_kv, SSI_DECODE_G));
#undef SSI_DECODE_G
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

int split_entry(const char* who, const void* qkv, int64_t ld, const CacheArg& c, int64_t n_slots, int64_t cap, const int32_t* slot,
                const int32_t* kv_len, void* out, float* lse, int64_t rows, int n_heads, int n_kv, int head_dim, int32_t* n_bad, int64_t span,
                int64_t n_splits, void* workspace, int64_t workspace_bytes, int dtype, void* stream) {
    SSI_CHECK_ARG(rows >= 0 && n_slots >= 0 && cap >= 0 && cap < (1LL << 31) && (dtype == SSI_F32 || dtype == SSI_BF16));
    if (int rc = check_geometry(who, n_heads, n_kv, head_dim)) return rc;
    if (int rc = check_split_args(span, n_splits, cap, workspace, workspace_bytes, rows, n_heads, head_dim, dtype)) return rc;
    if (rows == 0) return SSI_OK;
    if (int rc = check_decode_args(qkv, ld, c, n_slots, cap, slot, kv_len, out, rows, n_heads, head_dim, dtype)) return rc;
#define SSI_DECODE_G(GG) \
    launch_split<T, GG>(qkv, ld, c, n_slots, cap, slot, kv_len, (float*)workspace, span, n_splits, rows, n_heads, n_kv, head_dim, stream)
    SSI_DISPATCH_DTYPE(dtype, {
        SSI_DECODE_FORMS(n_heads / n_kv, SSI_DECODE_G);
        launch_split_merge<T>((const float*)workspace, span, n_splits, slot, n_slots, kv_len, cap, nullptr, 0, out, lse, rows, n_heads, n_kv, head_dim,
                              n_bad, stream);
    });
#undef SSI_DECODE_G
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

int beam_split_entry(const char* who, const void* qkv, int64_t ld, const CacheArg& p, int64_t n_pslots, int64_t cap_p, const CacheArg& b,
                     int64_t n_bslots, int64_t cap_b, const int32_t* prompt_slot, const int32_t* prompt_len, const int32_t* gen_len,
                     const int32_t* anc, int64_t ld_anc, void* out, float* lse, int64_t rows, int n_heads, int n_kv, int head_dim, int32_t* n_bad,
                     int64_t span, int64_t n_splits, void* workspace, int64_t workspace_bytes, int dtype, void* stream) {
    SSI_CHECK_ARG(rows >= 0 && n_pslots >= 0 && cap_p >= 0 && n_bslots >= 0 && cap_b >= 0 && ld_anc >= 0 && (dtype == SSI_F32 || dtype == SSI_BF16));
    SSI_CHECK_ARG(cap_p + cap_b < (1LL << 31) && n_bslots < (1LL << 31));
    if (int rc = check_geometry(who, n_heads, n_kv, head_dim)) return rc;
    if (int rc = check_split_args(span, n_splits, cap_p + (cap_b < ld_anc ? cap_b : ld_anc), workspace, workspace_bytes, rows, n_heads, head_dim, dtype))
        return rc;
    if (rows == 0) return SSI_OK;
    if (int rc = check_beam_args(qkv, ld, p, n_pslots, cap_p, b, n_bslots, cap_b, prompt_slot, prompt_len, gen_len, anc, ld_anc, out, rows, n_heads,
                                 head_dim, dtype)) return rc;
    const int64_t cap_b_eff = (b.there() && anc) ? cap_b : 0, n_ps_eff = p.there() ? n_pslots : 0;
    const int64_t gen_cap = cap_b_eff < ld_anc ? cap_b_eff : ld_anc;
#define SSI_DECODE_G(GG)                                                                                                                       \
    launch_split_beam<T, GG>(qkv, ld, p, n_ps_eff, cap_p, b, n_bslots, cap_b_eff, prompt_slot, prompt_len, gen_len, anc, ld_anc, (float*)workspace, \
                             span, n_splits, rows, n_heads, n_kv, head_dim, n_bad, stream)
    SSI_DISPATCH_DTYPE(dtype, {
        SSI_DECODE_FORMS(n_heads / n_kv, SSI_DECODE_G);
        launch_split_merge<T>((const float*)workspace, span, n_splits, prompt_slot, INT64_MAX, prompt_len, cap_p, gen_len, gen_cap, out, lse, rows,
                              n_heads, n_kv, head_dim, nullptr, stream);
    });
#undef SSI_DECODE_G
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

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

extern "C" int ssi_kv_store_fp8(const void* qkv, int64_t ld, const int64_t* dest, int64_t rows, int64_t n_dest, void* k_codes, void* v_codes,
                                void* k_exp, void* v_exp, int n_heads, int n_kv, int head_dim, int32_t* n_bad, int dtype, void* stream) {
    SSI_CHECK_ARG(rows >= 0 && n_dest >= 0 && (dtype == SSI_F32 || dtype == SSI_BF16));
    if (int rc = check_geometry("ssi_kv_store_fp8", n_heads, n_kv, head_dim)) return rc;
    if (rows == 0) return SSI_OK;
    const int64_t esize = dtype == SSI_BF16 ? 2 : 4, q_cols = (int64_t)n_heads * head_dim, kv_cols = (int64_t)n_kv * head_dim;
    SSI_CHECK_ARG(qkv && dest && k_codes && v_codes && k_exp && v_exp && ld >= q_cols + 2 * kv_cols && rows < (1LL << 31));
    SSI_CHECK_ARG(aligned16(qkv) && aligned16(k_codes) && aligned16(v_codes) && (ld * esize) % 16 == 0);
    SSI_DISPATCH_DTYPE(dtype, {
        const int lpk_log2 = lanes_log2<T>(head_dim);
        const int64_t lanes = (rows * 2 * n_kv) << lpk_log2;
        SSI_CHECK_ARG(ssi_cdiv(lanes, 256) < (1LL << 31));
        hipLaunchKernelGGL(q8_store_kernel<T>, dim3((unsigned)ssi_cdiv(lanes, 256)), dim3(256), 0, (hipStream_t)stream, (const T*)qkv, ld, dest, rows,
                           n_dest, (uint8_t*)k_codes, (uint8_t*)v_codes, (uint8_t*)k_exp, (uint8_t*)v_exp, (int)q_cols, n_kv, head_dim, lpk_log2, n_bad);
    });
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

extern "C" int ssi_attn_decode(const void* qkv, int64_t ld, const void* k_cache, const void* v_cache, int64_t n_slots, int64_t cap,
                               const int32_t* slot, const int32_t* kv_len, void* out, float* lse, int64_t rows, int n_heads, int n_kv,
                               int head_dim, int32_t* n_bad, int dtype, void* stream) {
    return decode_entry("ssi_attn_decode", qkv, ld, {k_cache, v_cache, nullptr, nullptr, false}, n_slots, cap, slot, kv_len, out, lse, rows, n_heads,
                        n_kv, head_dim, n_bad, dtype, stream);
}

extern "C" int ssi_attn_decode_fp8(const void* qkv, int64_t ld, const void* k_codes, const void* v_codes, const void* k_exp, const void* v_exp,
                                   int64_t n_slots, int64_t cap, const int32_t* slot, const int32_t* kv_len, void* out, float* lse, int64_t rows,
                                   int n_heads, int n_kv, int head_dim, int32_t* n_bad, int dtype, void* stream) {
    return decode_entry("ssi_attn_decode_fp8", qkv, ld, {k_codes, v_codes, k_exp, v_exp, true}, n_slots, cap, slot, kv_len, out, lse, rows, n_heads,
                        n_kv, head_dim, n_bad, dtype, stream);
}

extern "C" int ssi_attn_decode_beam(const void* qkv, int64_t ld, const void* pk_cache, const void* pv_cache, int64_t n_pslots, int64_t cap_p,
                                    const void* bk_cache, const void* bv_cache, int64_t n_bslots, int64_t cap_b, const int32_t* prompt_slot,
                                    const int32_t* prompt_len, const int32_t* gen_len, const int32_t* anc, int64_t ld_anc, void* out, float* lse,
                                    int64_t rows, int n_heads, int n_kv, int head_dim, int32_t* n_bad, int dtype, void* stream) {
    return beam_entry("ssi_attn_decode_beam", qkv, ld, {pk_cache, pv_cache, nullptr, nullptr, false}, n_pslots, cap_p,
                      {bk_cache, bv_cache, nullptr, nullptr, false}, n_bslots, cap_b, prompt_slot, prompt_len, gen_len, anc, ld_anc, out, lse, rows,
                      n_heads, n_kv, head_dim, n_bad, dtype, stream);
}

extern "C" int ssi_attn_decode_beam_fp8(const void* qkv, int64_t ld, const void* pk_codes, const void* pv_codes, const void* pk_exp,
                                        const void* pv_exp, int64_t n_pslots, int64_t cap_p, const void* bk_codes, const void* bv_codes,
                                        const void* bk_exp, const void* bv_exp, int64_t n_bslots, int64_t cap_b, const int32_t* prompt_slot,
                                        const int32_t* prompt_len, const int32_t* gen_len, const int32_t* anc, int64_t ld_anc, void* out, float* lse,
                                        int64_t rows, int n_heads, int n_kv, int head_dim, int32_t* n_bad, int dtype, void* stream) {
    return beam_entry("ssi_attn_decode_beam_fp8", qkv, ld, {pk_codes, pv_codes, pk_exp, pv_exp, true}, n_pslots, cap_p,
                      {bk_codes, bv_codes, bk_exp, bv_exp, true}, n_bslots, cap_b, prompt_slot, prompt_len, gen_len, anc, ld_anc, out, lse, rows,
                      n_heads, n_kv, head_dim, n_bad, dtype, stream);
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
    return split_entry("ssi_attn_decode_split", qkv, ld, {k_cache, v_cache, nullptr, nullptr, false}, n_slots, cap, slot, kv_len, out, lse, rows,
                       n_heads, n_kv, head_dim, n_bad, span, n_splits, workspace, workspace_bytes, dtype, stream);
}

extern "C" int ssi_attn_decode_split_fp8(const void* qkv, int64_t ld, const void* k_codes, const void* v_codes, const void* k_exp, const void* v_exp,
                                         int64_t n_slots, int64_t cap, const int32_t* slot, const int32_t* kv_len, void* out, float* lse,
                                         int64_t rows, int n_heads, int n_kv, int head_dim, int32_t* n_bad, int64_t span, int64_t n_splits,
                                         void* workspace, int64_t workspace_bytes, int dtype, void* stream) {
    return split_entry("ssi_attn_decode_split_fp8", qkv, ld, {k_codes, v_codes, k_exp, v_exp, true}, n_slots, cap, slot, kv_len, out, lse, rows,
                       n_heads, n_kv, head_dim, n_bad, span, n_splits, workspace, workspace_bytes, dtype, stream);
}

extern "C" int ssi_attn_decode_beam_split(const void* qkv, int64_t ld, const void* pk_cache, const void* pv_cache, int64_t n_pslots, int64_t cap_p,
                                          const void* bk_cache, const void* bv_cache, int64_t n_bslots, int64_t cap_b, const int32_t* prompt_slot,
                                          const int32_t* prompt_len, const int32_t* gen_len, const int32_t* anc, int64_t ld_anc, void* out,
                                          float* lse, int64_t rows, int n_heads, int n_kv, int head_dim, int32_t* n_bad, int64_t span,
                                          int64_t n_splits, void* workspace, int64_t workspace_bytes, int dtype, void* stream) {
    return beam_split_entry("ssi_attn_decode_beam_split", qkv, ld, {pk_cache, pv_cache, nullptr, nullptr, false}, n_pslots, cap_p,
                            {bk_cache, bv_cache, nullptr, nullptr, false}, n_bslots, cap_b, prompt_slot, prompt_len, gen_len, anc, ld_anc, out, lse,
                            rows, n_heads, n_kv, head_dim, n_bad, span, n_splits, workspace, workspace_bytes, dtype, stream);
}

extern "C" int ssi_attn_decode_beam_split_fp8(const void* qkv, int64_t ld, const void* pk_codes, const void* pv_codes, const void* pk_exp,
                                              const void* pv_exp, int64_t n_pslots, int64_t cap_p, const void* bk_codes, const void* bv_codes,
                                              const void* bk_exp, const void* bv_exp, int64_t n_bslots, int64_t cap_b,
                                              const int32_t* prompt_slot, const int32_t* prompt_len, const int32_t* gen_len, const int32_t* anc,
                                              int64_t ld_anc, void* out, float* lse, int64_t rows, int n_heads, int n_kv, int head_dim,
                                              int32_t* n_bad, int64_t span, int64_t n_splits, void* workspace, int64_t workspace_bytes, int dtype,
                                              void* stream) {
    return beam_split_entry("ssi_attn_decode_beam_split_fp8", qkv, ld, {pk_codes, pv_codes, pk_exp, pv_exp, true}, n_pslots, cap_p,
                            {bk_codes, bv_codes, bk_exp, bv_exp, true}, n_bslots, cap_b, prompt_slot, prompt_len, gen_len, anc, ld_anc, out, lse, rows,
                            n_heads, n_kv, head_dim, n_bad, span, n_splits, workspace, workspace_bytes, dtype, stream);
}
