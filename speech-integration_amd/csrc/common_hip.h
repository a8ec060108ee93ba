// Shared device/host helpers for libssi_hip.so (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/ssi_hip.h"

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

#define SSI_WAVE 64

// thread-local error text (defined in api.hip)
void ssi_set_error(const char* fmt, ...);

#define SSI_CHECK_ARG(cond)                                                                  \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            ssi_set_error("%s:%d: argument check failed: %s", __FILE__, __LINE__, #cond);    \
            return SSI_ERR_ARG;                                                              \
        }                                                                                    \
    } while (0)

#define SSI_LAUNCH_CHECK()                                                                   \
    do {                                                                                     \
        hipError_t e_ = hipGetLastError();                                                   \
        if (e_ != hipSuccess) {                                                              \
            ssi_set_error("%s:%d: launch failed: %s", __FILE__, __LINE__, hipGetErrorString(e_)); \
            return SSI_ERR_HIP + (int)e_;                                                    \
        }                                                                                    \
    } while (0)

static inline int64_t ssi_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int64_t ssi_align_up(int64_t a, int64_t b) { return ssi_cdiv(a, b) * b; }

// ---- storage <-> fp32 ------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ float to_f32(T v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<bf16_t>(bf16_t v) { return (float)v; }
template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t from_f32<bf16_t>(float v) { return (bf16_t)v; }  // RNE, NaN-preserving (v_cvt_pk_bf16_f32)

// logistic function used by every SwiGLU site (elementwise kernels and the fused GEMM epilogues must agree bit for bit).
// bf16 storage: v_exp_f32 / v_rcp_f32 (about 1 ulp each, far below the bf16 rounding that follows); f32 storage: libm.
template <typename T> __device__ __forceinline__ float ssi_sigmoid(float x);
template <> __device__ __forceinline__ float ssi_sigmoid<float>(float x) { return 1.f / (1.f + expf(-x)); }
template <> __device__ __forceinline__ float ssi_sigmoid<bf16_t>(float x) {
    return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * -1.44269504088896f));
}
template <typename T> __device__ __forceinline__ float ssi_silu(float x);
template <> __device__ __forceinline__ float ssi_silu<float>(float x) { return x / (1.f + expf(-x)); }
template <> __device__ __forceinline__ float ssi_silu<bf16_t>(float x) { return x * ssi_sigmoid<bf16_t>(x); }
// SwiGLU backward per element, shared by ssi_swiglu_bwd and the fused GEMM epilogues: contraction is switched off here so
// that every call site rounds identically whatever surrounds it (the fused and unfused paths are tested bit for bit).
template <typename T> __device__ __forceinline__ void ssi_swiglu_bwd_elem(float gf, float uf, float df, float& dgate, float& dup) {
#pragma clang fp contract(off)
    const float sig = ssi_sigmoid<T>(gf);
    const float one_minus = 1.f - sig;
    const float t = 1.f + gf * one_minus;
    dup = df * (gf * sig);
    dgate = (df * uf) * (sig * t);
}

// One RoPE pair, shared by ssi_rope_inplace and the QKV GEMM epilogue, which must agree bit for bit.  The library is built with
// -ffp-contract=fast, under which the backend fuses a multiply into an add whatever the pragma says, and WHICH of the two products it
// fuses depended on the surrounding code: the row kernel rounded x0 s and fused x1 c, the GEMM epilogue rounded x1 c and fused x0 s, and
// o1 differed by one bf16 ulp in a few elements per million.  The fusion is therefore written out, in the form the GEMM epilogue has
// always been compiled to (the training step runs that kernel; its results are unchanged bit for bit): both products with x1 are rounded,
// both products with x0 are fused.
__device__ __forceinline__ void ssi_rope_pair(float x0, float x1, float c, float s, float& o0, float& o1) {
#pragma clang fp contract(off)
    const float x1s = x1 * s, x1c = x1 * c;
    o0 = __builtin_fmaf(x0, c, -x1s);
    o1 = __builtin_fmaf(x0, s, x1c);
}

// 16-byte vector of storage elements: 4 floats or 8 bf16
template <typename T> struct Vec16;
template <> struct Vec16<float> {
    static constexpr int N = 4;
    f32x4 v;
    __device__ __forceinline__ float get(int i) const { return v[i]; }
    __device__ __forceinline__ void set(int i, float x) { v[i] = x; }
};
template <> struct Vec16<bf16_t> {
    static constexpr int N = 8;
    bf16x8 v;
    __device__ __forceinline__ float get(int i) const { return (float)v[i]; }
    __device__ __forceinline__ void set(int i, float x) { v[i] = (bf16_t)x; }
};
template <typename T> __device__ __forceinline__ Vec16<T> load16(const T* p) {
    Vec16<T> r;
    r.v = *reinterpret_cast<const decltype(r.v)*>(p);
    return r;
}
template <typename T> __device__ __forceinline__ void store16(T* p, const Vec16<T>& r) {
    *reinterpret_cast<decltype(r.v)*>(p) = r.v;
}

// streaming forms (touched once per launch: keep them out of the way of what the caches could hold)
template <typename T> __device__ __forceinline__ Vec16<T> load16_nt(const T* p) {
    Vec16<T> r;
    r.v = __builtin_nontemporal_load(reinterpret_cast<const decltype(r.v)*>(p));
    return r;
}
template <typename T> __device__ __forceinline__ void store16_nt(T* p, const Vec16<T>& r) {
    __builtin_nontemporal_store(r.v, reinterpret_cast<decltype(r.v)*>(p));
}

// ---- reductions ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {  // the same fixed xor tree in fp64
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// block-wide sum for blockDim.x <= 1024; `red` is >= 16 floats of LDS; result broadcast to all threads
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (l == 0) red[w] = v;
    __syncthreads();
    float t = (l < nw) ? red[l] : 0.f;
    t = wave_sum(t);
    return t;
}
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (l == 0) red[w] = v;
    __syncthreads();
    float t = (l < nw) ? red[l] : -INFINITY;
    t = wave_max(t);
    return t;
}
// block-wide integer sum for blockDim.x <= 1024; `red` is >= 16 ints of LDS; result broadcast to all threads
__device__ __forceinline__ int block_sum_i32(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (l == 0) red[w] = v;
    __syncthreads();
    int t = (l < nw) ? red[l] : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    return t;
}

// ---- counter-based random bits ---------------------------------------------------------------------------------------------
struct Philox4 { uint32_t w[4]; };

// Philox4x32-10 (Salmon et al., SC'11): ten rounds of two 32x32->64 multiplies, the key bumped by the Weyl constants between rounds
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// ---- buffer resources ----------------------------------------------------------------------------------------------------
// Raw buffer over `base`: stride 0, 2 GiB window, 32-bit data format (gfx9 family).  buffer_rsrc: the four words in SGPRs, for the inline-asm
// LDS-DMA requests (attn_mfma.h, gemm_nt4.h); buffer_rsrc_of: the compiler's resource type, for the raw_buffer_load / _store builtins.
constexpr unsigned BUF_RSRC_WORD3 = 0x00020000u;
__device__ __forceinline__ u32x4 buffer_rsrc(const void* base) {
    const uint64_t a = (uint64_t)(uintptr_t)base;
    u32x4 r;
    r[0] = __builtin_amdgcn_readfirstlane((unsigned)a);
    r[1] = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32) & 0xffffu);
    r[2] = 0x7fffffffu;
    r[3] = BUF_RSRC_WORD3;
    return r;
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc_of(const void* p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, BUF_RSRC_WORD3);
}

// ---- debug-build cycle stamps ------------------------------------------------------------------------------------------
// Cycle counter per phase of a kernel: tick(i) adds the cycles since the previous tick (or reset) to total[i].  A kernel declares
// PhaseStamps<true, ...> under its own -D flag and PhaseStamps<false, ...> otherwise: that form is empty, the calls compile to nothing.
// FENCED: scheduling barriers around each counter read, for the software-pipelined kernels (the read stays in the gap it is written in).
template <bool ENABLED, int N, bool FENCED = false> struct PhaseStamps {
    unsigned long long begin = __builtin_readcyclecounter(), last = begin, total[N] = {};
    __device__ __forceinline__ void reset() {
        if (FENCED) __builtin_amdgcn_sched_barrier(0);
        last = __builtin_readcyclecounter();
        if (FENCED) __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ void tick(int i) {
        const unsigned long long prev = last;
        reset();
        total[i] += last - prev;
    }
};
template <int N, bool FENCED> struct PhaseStamps<false, N, FENCED> {
    __device__ __forceinline__ void reset() {}
    __device__ __forceinline__ void tick(int) {}
};

// ---- internal functions: defined in one .hip file, called from another ------------------------------------------------
// Declared here ONCE; the defining file includes this header too, so the compiler holds the definition to the declaration.
// (C++ linkage: none of these is part of the ABI in include/ssi_hip.h.)
int ssi_get_impl();  // gemm_generic.hip: the value of ssi_set_impl

// gemm_mfma.hip: bf16 GEMMs on the matrix cores.  The bool forms return false when the shape is not theirs (the caller falls back to the
// unfused path); *rc then carries nothing.
bool ssi_gemm_mfma_supported(int layout, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B,
                             int64_t ldb, const void* C, int64_t ldc, const void* R);
int ssi_gemm_mfma_bf16(int layout, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B,
                       int64_t ldb, void* C, int64_t ldc, const void* R, float alpha, const float* alpha_dev,
                       int accumulate, void* stream);
int ssi_gemm_mfma_bf16_splitk(int layout, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B,
                              int64_t ldb, void* C, int64_t ldc, const void* R, float alpha, const float* alpha_dev,
                              int accumulate, int splits, float* slabs, void* stream);
bool ssi_gemm_mfma_bf16_batched(int layout, int batch, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, int64_t bsA, const void* B,
                                int64_t ldb, int64_t bsB, void* C, int64_t ldc, int64_t bsC, float alpha, const float* alpha_dev, int accumulate,
                                void* stream, int* rc);
void ssi_gemm_mfma_set_dynamic_tiles(int on);
bool ssi_gemm_rope_mfma(int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                        const float* rope, const int32_t* positions, int64_t seq, int64_t rot_cols, void* stream, int* rc);
bool ssi_gemm_swiglu_supported(int64_t M, int64_t inter, int64_t K, const void* p0, const void* p1, const void* p2, const void* p3,
                               int64_t ld0, int64_t ld1, int64_t ld2, int64_t ld3);
int ssi_gemm_swiglu_fwd_mfma(int64_t M, int64_t inter, int64_t K, const void* X, int64_t ldx, const void* W13, int64_t ldw,
                             void* GU, int64_t ldgu, void* ACT, int64_t ldact, void* stream);
int ssi_gemm_swiglu_bwd_mfma(int layout, int64_t M, int64_t inter, int64_t K, const void* DY, int64_t lddy, const void* W2, int64_t ldw,
                             const void* GU, int64_t ldgu, void* DGU, int64_t lddgu, void* stream);
bool ssi_gemm_swiglu_bwd_nn_supported(int64_t K, int64_t lddy, int64_t ldw);

// gemm_f32_mfma.hip: fp32 GEMMs on the fp32-input matrix instructions
bool ssi_gemm_f32_mfma_supported(int layout, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B,
                                 int64_t ldb, const void* C, int64_t ldc, const void* R);
int ssi_gemm_f32_mfma(int layout, int64_t M, int64_t N, int64_t K, const void* A, int64_t lda, const void* B, int64_t ldb,
                      void* C, int64_t ldc, const void* R, float alpha, const float* alpha_dev, int accumulate,
                      void* stream);

// attention_mfma.hip and the kernel files it includes
bool ssi_attn_mfma_supported(int64_t ld, int64_t batch, int64_t seq, int n_heads, int n_kv, int head_dim, int dtype);
void ssi_attn_note_dispatch(int v);
int ssi_attn_bwd_mfma(const void* qkv, int64_t ld, const void* out, const void* dout, const float* lse, void* dqkv,
                      float* delta, const int32_t* doc_start, const int32_t* doc_end, const float* rope, int64_t table_len,
                      const int32_t* positions, int64_t batch, int64_t seq, int n_heads, int n_kv, void* workspace, int64_t workspace_bytes,
                      const int32_t* plan_dev, const int32_t* host_plan_header, void* stream);
int ssi_attn_fwd_mfma(const void* qkv, int64_t ld, void* out, float* lse, const int32_t* doc_start, int64_t batch, int64_t seq,
                      int n_heads, int n_kv, void* stream);                                              // attn_fwd.h
int64_t ssi_attn_mfma_bwd_workspace_bytes(int64_t batch, int64_t seq, int n_heads, int n_kv);            // attn_bwd_dkv.h

#define SSI_DISPATCH_DTYPE(dtype, ...)                           \
    do {                                                         \
        if ((dtype) == SSI_F32) {                                \
            using T = float;                                     \
            __VA_ARGS__;                                         \
        } else if ((dtype) == SSI_BF16) {                        \
            using T = bf16_t;                                    \
            __VA_ARGS__;                                         \
        } else {                                                 \
            ssi_set_error("unsupported dtype %d", (int)(dtype)); \
            return SSI_ERR_ARG;                                  \
        }                                                        \
    } while (0)
