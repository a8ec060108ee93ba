// Bandwidth-bound kernels of the training step: RMSNorm, RoPE, SwiGLU, token counting, grad scaling, sum of squares,
// AdamW.  All are HBM-roofline kernels: 16-byte per-lane accesses, one wave (64 lanes) per row for the row reductions,
// shuffles for the reductions, fp32 math with the reference's rounding points.
#include "common_hip.h"

// =====================================================================================================================
// K2 RMSNorm forward: one wave per row (torchtune.modules.RMSNorm.forward)
// =====================================================================================================================
template <typename T, int MAXV>
__global__ __launch_bounds__(256) void rmsnorm_fwd_kernel(const T* __restrict__ x, const T* __restrict__ scale,
                                                          T* __restrict__ y, float* __restrict__ rstd_out,
                                                          int64_t rows, int dim, float eps) {
    constexpr int N = Vec16<T>::N;
    const int lane = threadIdx.x & 63;
    const int nvec = dim / N;
    const int64_t wave_global = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), wave_stride = (int64_t)gridDim.x * 4;
    // each row is read once, into registers; the next row of the wave is in flight while this one is reduced and written
    Vec16<T> w[MAXV];
#pragma unroll
    for (int k = 0; k < MAXV; ++k) {
        const int v = lane + k * 64;
        if (v < nvec) w[k] = load16(scale + v * N);
    }
    auto fetch = [&](int64_t row, Vec16<T>* a) {
        if (row >= rows) return;
#pragma unroll
        for (int k = 0; k < MAXV; ++k) {
            const int v = lane + k * 64;
            if (v < nvec) a[k] = load16(x + row * dim + v * N);
        }
    };
    auto finish = [&](int64_t row, const Vec16<T>* a) {
        float ss = 0.f;
#pragma unroll
        for (int k = 0; k < MAXV; ++k) {
            const int v = lane + k * 64;
            if (v < nvec) {
#pragma unroll
                for (int i = 0; i < N; ++i) { float f = a[k].get(i); ss += f * f; }
            }
        }
        ss = wave_sum(ss);
        const float rstd = rsqrtf(ss / (float)dim + eps);
        if (lane == 0 && rstd_out) rstd_out[row] = rstd;
#pragma unroll
        for (int k = 0; k < MAXV; ++k) {
            const int v = lane + k * 64;
            if (v < nvec) {
                Vec16<T> o;
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    // (x32 * rstd).type_as(x) * scale : round to storage type before the scale multiply
                    float xn = to_f32<T>(from_f32<T>(a[k].get(i) * rstd));
                    o.set(i, xn * w[k].get(i));
                }
                store16(y + row * dim + v * N, o);
            }
        }
    };
    Vec16<T> a0[MAXV], a1[MAXV];
    fetch(wave_global, a0);
    for (int64_t row = wave_global; row < rows; row += 2 * wave_stride) {
        fetch(row + wave_stride, a1);
        finish(row, a0);
        if (row + wave_stride >= rows) break;
        fetch(row + 2 * wave_stride, a0);
        finish(row + wave_stride, a1);
    }
}

// K2 RMSNorm backward.  Per wave: a strided set of rows; dscale partial sums kept per lane-column in registers and
// reduced over the block's 4 waves through LDS, then written as one partial row per block.
template <typename T, int MAXV>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                          const T* __restrict__ scale, const float* __restrict__ rstd,
                                                          const T* __restrict__ dres, T* __restrict__ dx,
                                                          float* __restrict__ partials, int64_t rows, int dim) {
    constexpr int N = Vec16<T>::N;
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [4][WS]
    constexpr int WS = MAXV * N * 64;  // floats per wave in the staging buffer (>= dim)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nvec = dim / N;
    float dw[MAXV][N];
#pragma unroll
    for (int k = 0; k < MAXV; ++k)
#pragma unroll
        for (int i = 0; i < N; ++i) dw[k][i] = 0.f;

    const int64_t wave_global = (int64_t)blockIdx.x * 4 + wave, wave_stride = (int64_t)gridDim.x * 4;
    // A wave walks rows/waves rows one after the other (the dscale sums stay in its registers), so it alone would pay the whole
    // memory latency twice per row: each row is read ONCE, into registers, and the next row's loads are in flight while this
    // one is reduced and written (two register sets, alternating).
    struct RowRegs { Vec16<T> a[MAXV], g[MAXV], r[MAXV]; float rs; };
    Vec16<T> w[MAXV];
#pragma unroll
    for (int k = 0; k < MAXV; ++k) {
        const int v = lane + k * 64;
        if (v < nvec) w[k] = load16(scale + v * N);
    }
    auto fetch = [&](int64_t row, RowRegs& q) {
        if (row >= rows) return;
        q.rs = rstd[row];
#pragma unroll
        for (int k = 0; k < MAXV; ++k) {
            const int v = lane + k * 64;
            if (v < nvec) {
                q.a[k] = load16(x + row * dim + v * N);
                q.g[k] = load16(dy + row * dim + v * N);
                if (dres) q.r[k] = load16(dres + row * dim + v * N);
            }
        }
    };
    auto finish = [&](int64_t row, const RowRegs& q) {
        const float rs = q.rs;
        float c = 0.f;
#pragma unroll
        for (int k = 0; k < MAXV; ++k) {
            const int v = lane + k * 64;
            if (v < nvec) {
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    const float xhat = q.a[k].get(i) * rs;
                    c += q.g[k].get(i) * w[k].get(i) * xhat;
                    dw[k][i] += q.g[k].get(i) * xhat;
                }
            }
        }
        c = wave_sum(c) / (float)dim;
#pragma unroll
        for (int k = 0; k < MAXV; ++k) {
            const int v = lane + k * 64;
            if (v < nvec) {
                Vec16<T> o;
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    const float xhat = q.a[k].get(i) * rs;
                    float d = rs * (q.g[k].get(i) * w[k].get(i) - xhat * c);
                    if (dres) d += q.r[k].get(i);
                    o.set(i, d);
                }
                store16(dx + row * dim + v * N, o);
            }
        }
    };
    RowRegs q0, q1;
    fetch(wave_global, q0);
    for (int64_t row = wave_global; row < rows; row += 2 * wave_stride) {
        fetch(row + wave_stride, q1);
        finish(row, q0);
        if (row + wave_stride >= rows) break;
        fetch(row + 2 * wave_stride, q0);
        finish(row + wave_stride, q1);
    }
    // block reduce of dscale partials.  Staged [wave][k][i][lane]: consecutive lanes on consecutive banks.  The column-major form
    // [wave][column] (a lane's N consecutive floats = a 32-byte stride between lanes) was the one kernel of the step with LDS bank
    // conflicts (SQ_LDS_BANK_CONFLICT 14.4 % of its LDS cycles, profiles/r03_pmc_kernels.md); same sums in the same order.
#pragma unroll
    for (int k = 0; k < MAXV; ++k) {
        const int v = lane + k * 64;
        if (v < nvec)
#pragma unroll
            for (int i = 0; i < N; ++i) lds[wave * WS + (k * N + i) * 64 + lane] = dw[k][i];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < WS; idx += 256) {
        const int l = idx & 63, ki = idx >> 6, v = l + (ki / N) * 64;
        if (v < nvec)
            partials[(int64_t)blockIdx.x * dim + v * N + ki % N] = lds[idx] + lds[WS + idx] + lds[2 * WS + idx] + lds[3 * WS + idx];
    }
}

// dscale[c] += sum_b partials[b][c]   (fixed order -> deterministic).  64 columns x 16 row groups per 1024-thread block: every
// thread has nblocks/16 independent loads in flight (with 4 row groups the 128-deep dependent chain made this launch cost as
// much as the 60x larger rmsnorm_bwd pass in front of it).
template <typename T>
__global__ __launch_bounds__(1024) void colsum_accum_kernel(const float* __restrict__ partials, T* __restrict__ dscale,
                                                            int nblocks, int dim, int accumulate) {
    __shared__ float red[16][64];
    const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + cx;
    float s = 0.f;
    if (col < dim) {
        float part[4] = {0.f, 0.f, 0.f, 0.f};
        int b = ry;
        for (; b + 48 < nblocks; b += 64) {
#pragma unroll
            for (int u = 0; u < 4; ++u) part[u] += partials[(int64_t)(b + 16 * u) * dim + col];
        }
        for (; b < nblocks; b += 16) part[0] += partials[(int64_t)b * dim + col];
        s = (part[0] + part[1]) + (part[2] + part[3]);
    }
    red[ry][cx] = s;
    __syncthreads();
    if (ry == 0 && col < dim) {
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) t += red[r][cx];
        dscale[col] = from_f32<T>(accumulate ? to_f32<T>(dscale[col]) + t : t);
    }
}

static inline int rmsnorm_bwd_blocks(int64_t rows) {
    // one 4-wave block per CU: with the row prefetch a wave hides its own latency, and fewer blocks mean fewer partial rows for the
    // column sum (measured at 16384 x 2048 bf16: 256 blocks 45.7 us, 512 50.3, 1024 60.3; before the prefetch 512 was best at 54.4)
    int64_t b = ssi_cdiv(rows, 4);
    return (int)(b < 256 ? b : 256);
}

extern "C" int64_t ssi_rmsnorm_bwd_workspace_bytes(int64_t rows, int64_t dim) {
    return (int64_t)rmsnorm_bwd_blocks(rows) * dim * (int64_t)sizeof(float);
}

extern "C" int ssi_rmsnorm_fwd(const void* x, const void* scale, void* y, float* rstd, int64_t rows, int64_t dim,
                               float eps, int dtype, void* stream) {
    SSI_CHECK_ARG(x && scale && y && rows >= 0 && dim > 0 && dim % 8 == 0);
    if (rows == 0) return SSI_OK;
    const int64_t nb = ssi_cdiv(rows, 4) < 1024 ? ssi_cdiv(rows, 4) : 1024;  // 16384 x 2048 bf16: 1024 blocks 20.7 us, 256 23.7, 4096 21.2
    const int64_t vec_per_lane = ssi_cdiv(dim / (dtype == SSI_BF16 ? 8 : 4), 64);
    if (vec_per_lane > 8) { ssi_set_error("rmsnorm_fwd: dim %d too large", (int)dim); return SSI_ERR_UNSUPPORTED; }
#define SSI_RMS_FWD(MV)                                                                                                              \
    SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((rmsnorm_fwd_kernel<T, MV>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, \
                                                 (const T*)x, (const T*)scale, (T*)y, rstd, rows, (int)dim, eps))
    if (vec_per_lane <= 1) { SSI_RMS_FWD(1); }
    else if (vec_per_lane <= 2) { SSI_RMS_FWD(2); }
    else if (vec_per_lane <= 4) { SSI_RMS_FWD(4); }
    else { SSI_RMS_FWD(8); }
#undef SSI_RMS_FWD
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

template <typename T>
static int launch_rmsnorm_bwd(const T* dy, const T* x, const T* scale, const float* rstd, const T* dres, T* dx, T* dscale,
                              int64_t rows, int dim, int nb, size_t lds_bytes, float* workspace, hipStream_t st, int accumulate) {
    const int64_t vec_per_lane = ssi_cdiv(dim / Vec16<T>::N, 64);
    const int maxv = vec_per_lane <= 1 ? 1 : vec_per_lane <= 2 ? 2 : vec_per_lane <= 4 ? 4 : 8;
    lds_bytes = (size_t)4 * maxv * Vec16<T>::N * 64 * sizeof(float);  // [4 waves][MAXV * N * 64]
    if (vec_per_lane <= 1)
        hipLaunchKernelGGL((rmsnorm_bwd_kernel<T, 1>), dim3(nb), dim3(256), lds_bytes, st, dy, x, scale, rstd, dres, dx, workspace, rows, dim);
    else if (vec_per_lane <= 2)
        hipLaunchKernelGGL((rmsnorm_bwd_kernel<T, 2>), dim3(nb), dim3(256), lds_bytes, st, dy, x, scale, rstd, dres, dx, workspace, rows, dim);
    else if (vec_per_lane <= 4)
        hipLaunchKernelGGL((rmsnorm_bwd_kernel<T, 4>), dim3(nb), dim3(256), lds_bytes, st, dy, x, scale, rstd, dres, dx, workspace, rows, dim);
    else if (vec_per_lane <= 8)
        hipLaunchKernelGGL((rmsnorm_bwd_kernel<T, 8>), dim3(nb), dim3(256), lds_bytes, st, dy, x, scale, rstd, dres, dx, workspace, rows, dim);
    else { ssi_set_error("rmsnorm_bwd: dim %d too large", dim); return SSI_ERR_UNSUPPORTED; }
    SSI_LAUNCH_CHECK();
    hipLaunchKernelGGL(colsum_accum_kernel<T>, dim3((unsigned)ssi_cdiv(dim, 64)), dim3(1024), 0, st, (const float*)workspace, dscale, nb, dim, accumulate);
    return SSI_OK;
}

extern "C" int ssi_rmsnorm_bwd(const void* dy, const void* x, const void* scale, const float* rstd, const void* dres,
                               void* dx, void* dscale, int accumulate_dscale, int64_t rows, int64_t dim, int dtype, void* workspace,
                               int64_t workspace_bytes, void* stream) {
    SSI_CHECK_ARG(dy && x && scale && rstd && dx && dscale && rows >= 0 && dim > 0 && dim % 8 == 0);
    if (rows == 0) return SSI_OK;
    const int nb = rmsnorm_bwd_blocks(rows);
    if (!workspace || workspace_bytes < ssi_rmsnorm_bwd_workspace_bytes(rows, dim)) {
        ssi_set_error("rmsnorm_bwd: workspace too small");
        return SSI_ERR_WORKSPACE;
    }
    const size_t lds_bytes = 4 * ssi_align_up(dim, 512) * sizeof(float);  // upper bound of what launch_rmsnorm_bwd asks for
    SSI_CHECK_ARG(dim <= 8 * 8 * 64 && 2 * lds_bytes <= 160 * 1024);
    int rc = SSI_OK;
    SSI_DISPATCH_DTYPE(dtype, rc = launch_rmsnorm_bwd<T>((const T*)dy, (const T*)x, (const T*)scale, rstd, (const T*)dres,
                                                         (T*)dx, (T*)dscale, rows, (int)dim, nb, lds_bytes,
                                                         (float*)workspace, (hipStream_t)stream, accumulate_dscale));
    if (rc) return rc;
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

// =====================================================================================================================
// K4 RoPE (Llama3ScaledRoPE.forward): adjacent pairs, fp32 math, in place.  One 16-byte vector per thread.
// =====================================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void rope_kernel(T* __restrict__ x, int64_t ld, int64_t rows, int64_t seq_len,
                                                   int rot_width, int head_dim, const float* __restrict__ table,
                                                   const int32_t* __restrict__ positions, float sign) {
    constexpr int N = Vec16<T>::N;
    const int vec_per_row = rot_width / N;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= rows * vec_per_row) return;
    const int64_t row = gid / vec_per_row;
    const int col = (int)(gid % vec_per_row) * N;
    const int64_t pos = positions ? (int64_t)positions[row] : (row % seq_len);
    const int pair0 = (col % head_dim) >> 1;
    const float* tb = table + (pos * (head_dim >> 1) + pair0) * 2;
    T* p = x + row * ld + col;
    Vec16<T> a = load16(p), o;
#pragma unroll
    for (int i = 0; i < N; i += 2) {
        const float c = tb[i], s = tb[i + 1] * sign;
        const float x0 = a.get(i), x1 = a.get(i + 1);
        float o0, o1;
        ssi_rope_pair(x0, x1, c, s, o0, o1);
        o.set(i, o0);
        o.set(i + 1, o1);
    }
    store16(p, o);
}

extern "C" int ssi_rope_inplace(void* x, int64_t ld, int64_t rows, int64_t seq_len, int n_heads_rot, int head_dim,
                                const float* table, int64_t table_len, const int32_t* positions, int inverse, int dtype,
                                void* stream) {
    SSI_CHECK_ARG(x && table && rows >= 0 && seq_len > 0 && n_heads_rot > 0 && head_dim > 0 && head_dim % 8 == 0);
    SSI_CHECK_ARG(ld % 8 == 0 && (int64_t)n_heads_rot * head_dim <= ld);
    SSI_CHECK_ARG(positions != nullptr || table_len >= seq_len);
    if (rows == 0) return SSI_OK;
    const int rot_width = n_heads_rot * head_dim;
    SSI_DISPATCH_DTYPE(dtype, {
        const int64_t total = rows * (rot_width / Vec16<T>::N);
        hipLaunchKernelGGL(rope_kernel<T>, dim3((unsigned)ssi_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (T*)x,
                           ld, rows, seq_len, rot_width, head_dim, table, positions, inverse ? -1.f : 1.f);
    });
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

// =====================================================================================================================
// K7 SwiGLU elementwise (torchtune FeedForward middle): act = silu(gate) * up ; gu = [gate | up]
// =====================================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const T* __restrict__ gu, T* __restrict__ act, int64_t rows,
                                                         int64_t inter) {
    constexpr int N = Vec16<T>::N;
    const int64_t vpr = inter / N;
    for (int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x; gid < rows * vpr; gid += (int64_t)gridDim.x * 256) {
        const int64_t row = gid / vpr, col = (gid % vpr) * N;
        Vec16<T> g = load16(gu + row * 2 * inter + col), u = load16(gu + row * 2 * inter + inter + col), o;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const float gf = g.get(i);
            const float s = to_f32<T>(from_f32<T>(ssi_silu<T>(gf)));  // F.silu result rounded to storage type
            o.set(i, s * u.get(i));
        }
        store16(act + row * inter + col, o);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const T* __restrict__ dact, const T* __restrict__ gu,
                                                         T* __restrict__ dgu, int64_t rows, int64_t inter) {
    constexpr int N = Vec16<T>::N;
    const int64_t vpr = inter / N;
    for (int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x; gid < rows * vpr; gid += (int64_t)gridDim.x * 256) {
        const int64_t row = gid / vpr, col = (gid % vpr) * N;
        Vec16<T> g = load16(gu + row * 2 * inter + col), u = load16(gu + row * 2 * inter + inter + col);
        Vec16<T> d = load16(dact + row * inter + col), og, ou;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            float dg, du;
            ssi_swiglu_bwd_elem<T>(g.get(i), u.get(i), d.get(i), dg, du);
            ou.set(i, du);
            og.set(i, dg);
        }
        store16(dgu + row * 2 * inter + col, og);
        store16(dgu + row * 2 * inter + inter + col, ou);
    }
}

static inline unsigned stream_grid(int64_t work_items, int64_t cap = 8192) {
    int64_t b = ssi_cdiv(work_items, 256);
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

extern "C" int ssi_swiglu_fwd(const void* gu, void* act, int64_t rows, int64_t inter, int dtype, void* stream) {
    SSI_CHECK_ARG(gu && act && rows >= 0 && inter > 0 && inter % 8 == 0);
    if (rows == 0) return SSI_OK;
    SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(swiglu_fwd_kernel<T>, dim3(stream_grid(rows * inter / Vec16<T>::N)),
                                                 dim3(256), 0, (hipStream_t)stream, (const T*)gu, (T*)act, rows, inter));
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

extern "C" int ssi_swiglu_bwd(const void* dact, const void* gu, void* dgu, int64_t rows, int64_t inter, int dtype,
                              void* stream) {
    SSI_CHECK_ARG(dact && gu && dgu && rows >= 0 && inter > 0 && inter % 8 == 0);
    if (rows == 0) return SSI_OK;
    SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(swiglu_bwd_kernel<T>, dim3(stream_grid(rows * inter / Vec16<T>::N)),
                                                 dim3(256), 0, (hipStream_t)stream, (const T*)dact, (const T*)gu,
                                                 (T*)dgu, rows, inter));
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

// =====================================================================================================================
// K14 token-type counts + valid-label count in ONE launch (replaces 6-7 .sum().item() syncs, trainer.py:388,391)
// =====================================================================================================================
#define SSI_MAX_RANGES 8
__global__ __launch_bounds__(256) void count_tokens_kernel(const int64_t* __restrict__ tokens,
                                                           const int64_t* __restrict__ labels, int64_t n,
                                                           const int64_t* __restrict__ ranges, int n_ranges,
                                                           int64_t pad_id, int64_t ignore_index,
                                                           unsigned long long* __restrict__ out) {
    __shared__ unsigned int blk[SSI_MAX_RANGES + 2];
    if (threadIdx.x < SSI_MAX_RANGES + 2) blk[threadIdx.x] = 0;
    __syncthreads();
    int64_t lo[SSI_MAX_RANGES], hi[SSI_MAX_RANGES];
    unsigned int cnt[SSI_MAX_RANGES + 2];
#pragma unroll
    for (int r = 0; r < SSI_MAX_RANGES; ++r) {
        lo[r] = r < n_ranges ? ranges[2 * r] : 1;
        hi[r] = r < n_ranges ? ranges[2 * r + 1] : 0;
    }
#pragma unroll
    for (int r = 0; r < SSI_MAX_RANGES + 2; ++r) cnt[r] = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t t = tokens[i];
#pragma unroll
        for (int r = 0; r < SSI_MAX_RANGES; ++r) cnt[r] += (t >= lo[r] && t <= hi[r]) ? 1u : 0u;
        cnt[SSI_MAX_RANGES] += (t != pad_id) ? 1u : 0u;
        if (labels) cnt[SSI_MAX_RANGES + 1] += (labels[i] != ignore_index) ? 1u : 0u;
    }
#pragma unroll
    for (int r = 0; r < SSI_MAX_RANGES + 2; ++r) {
        unsigned int v = cnt[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&blk[r], v);
    }
    __syncthreads();
    if (threadIdx.x < SSI_MAX_RANGES + 2) {
        const int r = threadIdx.x;
        const int dst = r < SSI_MAX_RANGES ? r : n_ranges + (r - SSI_MAX_RANGES);
        if ((r >= SSI_MAX_RANGES || r < n_ranges) && blk[r]) atomicAdd(&out[dst], (unsigned long long)blk[r]);
    }
}

extern "C" int ssi_count_tokens(const int64_t* tokens, const int64_t* labels, int64_t n, const int64_t* ranges,
                                int n_ranges, int64_t pad_id, int64_t ignore_index, int64_t* out, void* stream) {
    SSI_CHECK_ARG((tokens || n == 0) && out && n >= 0 && n_ranges >= 0 && n_ranges <= SSI_MAX_RANGES && (ranges || n_ranges == 0));
    hipError_t e = hipMemsetAsync(out, 0, sizeof(int64_t) * (n_ranges + 2), (hipStream_t)stream);
    if (e != hipSuccess) { ssi_set_error("count_tokens: memset failed: %s", hipGetErrorString(e)); return SSI_ERR_HIP + (int)e; }
    if (n == 0) return SSI_OK;
    int64_t b = ssi_cdiv(n, 256);
    if (b > 256) b = 256;
    hipLaunchKernelGGL(count_tokens_kernel, dim3((unsigned)b), dim3(256), 0, (hipStream_t)stream, tokens, labels, n, ranges,
                       n_ranges, pad_id, ignore_index, (unsigned long long*)out);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

// =====================================================================================================================
// Packed rows: positions + document bounds from input_pos in ONE launch (the model did this with ~10 torch ops per step).
// One 256-thread workgroup per row; a document starts where input_pos == 0 (and at position 0 of the row).  Each thread owns a
// contiguous span: last start at or before it (forward) and first start after it (backward) come from two LDS scans over the
// per-thread summaries, then the span is filled.  Integer work: results are exact.
// =====================================================================================================================
__global__ __launch_bounds__(256) void doc_ranges_kernel(const int64_t* __restrict__ input_pos, int64_t seq, int max_pos,
                                                         int32_t* __restrict__ pos, int32_t* __restrict__ doc_start,
                                                         int32_t* __restrict__ doc_end, int32_t* __restrict__ n_clamped) {
    __shared__ int last_start[256], first_start[256];
    const int64_t row = blockIdx.x;
    const int64_t* ip = input_pos + row * seq;
    const int t = threadIdx.x;
    const int span = (int)((seq + 255) / 256);
    const int lo = t * span, hi = (int)(lo + span < seq ? lo + span : seq);
    int ls = -1, fs = (int)seq;  // last start inside my span, first start inside my span
    for (int s = lo; s < hi; ++s) {
        const bool st = s == 0 || ip[s] == 0;
        if (st) { ls = s; if (fs == (int)seq) fs = s; }
    }
    last_start[t] = ls;
    first_start[t] = fs;
    __syncthreads();
    int before = -1;             // last start in the spans before mine
    for (int u = t - 1; u >= 0 && before < 0; --u) before = last_start[u];
    int after = (int)seq;        // first start in the spans after mine
    for (int u = t + 1; u < 256 && after == (int)seq; ++u) after = first_start[u];
    // forward: document start of every position of my span
    int cur = before, clamped = 0;
    for (int s = lo; s < hi; ++s) {
        if (s == 0 || ip[s] == 0) cur = s;
        doc_start[row * seq + s] = cur;
        const int64_t p = ip[s];
        clamped += (p < 0 || p > max_pos) ? 1 : 0;
        pos[row * seq + s] = (int32_t)(p < 0 ? 0 : (p > max_pos ? max_pos : p));
    }
    if (n_clamped && clamped) atomicAdd(n_clamped, clamped);  // integer: exact whatever the order
    // backward: one past the last position of the document = the first start strictly after s
    int nxt = after;
    for (int s = hi - 1; s >= lo; --s) {
        doc_end[row * seq + s] = nxt;
        if (s == 0 || ip[s] == 0) nxt = s;
    }
}

extern "C" int ssi_doc_ranges(const int64_t* input_pos, int64_t batch, int64_t seq, int64_t max_pos, int32_t* positions,
                              int32_t* doc_start, int32_t* doc_end, int32_t* n_clamped, void* stream) {
    SSI_CHECK_ARG(input_pos && positions && doc_start && doc_end && batch >= 0 && seq >= 0 && seq < (1LL << 31) && max_pos >= 0 && max_pos < (1LL << 31));
    if (batch == 0 || seq == 0) return SSI_OK;
    hipLaunchKernelGGL(doc_ranges_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, input_pos, seq, (int)max_pos, positions,
                       doc_start, doc_end, n_clamped);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

// =====================================================================================================================
// K11 scale_grads, K12 sum of squares (for clip_grad_norm_) — flat-buffer streaming kernels (K13 AdamW follows its rounding and its table)
// =====================================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void scale_kernel(T* __restrict__ x, int64_t n, float scale, const float* scale_dev) {
    constexpr int N = Vec16<T>::N;
    const float s = scale * (scale_dev ? *scale_dev : 1.f);
    const int64_t nvec = n / N;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * 256) {
        Vec16<T> a = load16(x + v * N);
#pragma unroll
        for (int i = 0; i < N; ++i) a.set(i, a.get(i) * s);
        store16(x + v * N, a);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n - nvec * N)) {
        const int64_t i = nvec * N + threadIdx.x;
        x[i] = from_f32<T>(to_f32<T>(x[i]) * s);
    }
}

extern "C" int ssi_scale_inplace(void* x, int64_t n, float scale, const float* scale_dev, int dtype, void* stream) {
    SSI_CHECK_ARG(x && n >= 0 && ((uintptr_t)x % 16) == 0);
    if (n == 0) return SSI_OK;
    SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(scale_kernel<T>, dim3(stream_grid(n / Vec16<T>::N + 1)), dim3(256), 0,
                                                 (hipStream_t)stream, (T*)x, n, scale, scale_dev));
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

#define SSI_SUMSQ_BLOCKS 1024
template <typename T>
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const T* __restrict__ x, int64_t n, float* __restrict__ part) {
    constexpr int N = Vec16<T>::N;
    __shared__ float red[16];
    const int64_t nvec = n / N;
    float s = 0.f;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * 256) {
        Vec16<T> a = load16(x + v * N);
#pragma unroll
        for (int i = 0; i < N; ++i) { const float f = a.get(i); s += f * f; }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n - nvec * N)) {
        const float f = to_f32<T>(x[nvec * N + threadIdx.x]);
        s += f * f;
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(1024) void sumsq_final_kernel(const float* __restrict__ part, int nb, float* __restrict__ out) {
    __shared__ float red[16];
    float s = (int)threadIdx.x < nb ? part[threadIdx.x] : 0.f;
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = s;
}
extern "C" int64_t ssi_sumsq_workspace_bytes(int64_t) { return SSI_SUMSQ_BLOCKS * sizeof(float); }
extern "C" int ssi_sumsq(const void* x, int64_t n, int dtype, float* out, void* workspace, int64_t workspace_bytes,
                         void* stream) {
    SSI_CHECK_ARG(x && out && n >= 0 && ((uintptr_t)x % 16) == 0);
    if (!workspace || workspace_bytes < ssi_sumsq_workspace_bytes(n)) { ssi_set_error("sumsq: workspace too small"); return SSI_ERR_WORKSPACE; }
    SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(sumsq_partial_kernel<T>, dim3(SSI_SUMSQ_BLOCKS), dim3(256), 0,
                                                 (hipStream_t)stream, (const T*)x, n, (float*)workspace));
    SSI_LAUNCH_CHECK();
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const float*)workspace,
                       SSI_SUMSQ_BLOCKS, out);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

// =====================================================================================================================
// K12g sums of squares per GROUP of segments of a flat buffer (ABI v23; opt-in, HipAdamW(grad_groups=...)): one read of the buffer gives
// every group's sum.  The table travels by value in the kernel arguments, in units of 8 elements like AdamwSegTable.  A block owns a
// CONTIGUOUS run of 256-vector tiles; it finds the segment of its first unit ONCE with wave-uniform indices only (15 coarse ends, then the
// 16 ends of one chunk) and walks forward from there, so a tile that lies inside one segment touches no table (a lookup per tile put two
// dependent rounds of scalar loads in front of every vector load: 0.71 ms against ssi_sumsq's 0.44 on 1.246 G bf16 elements; the walk:
// 0.42); a tile that segments end in walks those segments, the lanes only select.  ONE running sum per thread, that of the block's current
// group.  When the group changes (a block-uniform event: at most once per segment of the block's run) the sum is reduced over the block by
// the fixed xor tree and added, by thread 0, to the group's slot in LDS.  A lane of a skipped segment (group -1) issues no load.  No float
// atomics anywhere: the per-block slots go to the workspace and the final kernel adds them in a fixed order, so the bits are the same in
// every launch, and a group's sum is built from its own elements and exact zeros only.
// =====================================================================================================================
#define SSI_SUMSQ_GROUPS_BLOCKS 2048
struct SumsqGroupTable {
    uint32_t end8[SSI_SUMSQ_MAX_SEGS];         // exclusive end of segment s in units of 8 elements (the last: rounded up); unused: 0xFFFFFFFF
    int32_t group[SSI_SUMSQ_MAX_SEGS];         // group of segment s, -1: not read
    uint32_t coarse[SSI_SUMSQ_MAX_SEGS / 16];  // end8[16 k + 15]
    int n_segs;
};

template <typename T>
__global__ __launch_bounds__(256) void sumsq_groups_partial_kernel(const T* __restrict__ x, int64_t n, const SumsqGroupTable tab,
                                                                   int tiles_per_block, int n_groups, int tail_group,
                                                                   float* __restrict__ part) {
    constexpr int N = Vec16<T>::N;
    __shared__ float red[16];
    __shared__ float acc[SSI_SUMSQ_MAX_GROUPS];
    if (threadIdx.x < SSI_SUMSQ_MAX_GROUPS) acc[threadIdx.x] = 0.f;   // (block_sum's barriers lie between this and thread 0's first add)
    const int64_t nvec = n / N;
    float s = 0.f;
    int cur = -1;   // the group s belongs to; block-uniform
    auto flush = [&]() {
        if (cur >= 0) {
            const float t = block_sum(s, red);
            if (threadIdx.x == 0) acc[cur] += t;
            s = 0.f;
        }
    };
    const int64_t t0 = (int64_t)blockIdx.x * tiles_per_block;
    // the segment of the block's first unit: one lookup per block; the tiles that follow walk forward from it
    int sg = 0;
    uint32_t seg_start = 0u, seg_end = 0xFFFFFFFFu;
    int seg_g = -1;
    if (t0 * 256 < nvec) {
        const uint32_t ub = (uint32_t)((t0 * 256 * N) >> 3);
        int c = 0;
#pragma unroll
        for (int j = 0; j < SSI_SUMSQ_MAX_SEGS / 16 - 1; ++j) c += ub >= tab.coarse[j] ? 1 : 0;
        sg = 16 * c;
#pragma unroll
        for (int j = 0; j < 16; ++j) sg += ub >= tab.end8[16 * c + j] ? 1 : 0;
        seg_start = sg ? tab.end8[sg - 1] : 0u;
        seg_end = tab.end8[sg];
        seg_g = tab.group[sg];
    }
    auto add = [&](int64_t i) {
        const Vec16<T> a = load16(x + i * N);
#pragma unroll
        for (int e = 0; e < N; ++e) { const float f = a.get(e); s += f * f; }
    };
    for (int k = 0; k < tiles_per_block; ++k) {
        const int64_t b = (t0 + k) * 256;   // the tile's first vector
        if (b >= nvec) break;
        const int64_t i = b + threadIdx.x;
        const uint32_t ub0 = (uint32_t)((b * N) >> 3), ub1 = (uint32_t)(((b + 255) * N) >> 3), u = (uint32_t)((i * N) >> 3);
        while (ub0 >= seg_end && sg + 1 < tab.n_segs) {   // (every index here is wave-uniform: scalar loads, and only at a segment's end)
            seg_start = seg_end;
            ++sg;
            seg_end = tab.end8[sg];
            seg_g = tab.group[sg];
        }
        if (ub1 < seg_end) {   // the whole tile lies in one segment: no table access
            if (seg_g >= 0) {
                if (seg_g != cur) { flush(); cur = seg_g; }
                if (i < nvec) add(i);
            }
            continue;
        }
        uint32_t start = seg_start;
        for (int q = sg; q < tab.n_segs && start <= ub1; ++q) {   // the segments that reach into the tile: the lanes only select
            const uint32_t end = tab.end8[q];
            const int g = tab.group[q];
            if (g >= 0) {
                if (g != cur) { flush(); cur = g; }
                if (u >= start && u < end && i < nvec) add(i);
            }
            start = end;
        }
    }
    if (blockIdx.x == gridDim.x - 1 && tail_group >= 0) {   // the ragged tail belongs to the last segment
        if (tail_group != cur) { flush(); cur = tail_group; }
        if (threadIdx.x < (n - nvec * N)) {
            const float f = to_f32<T>(x[nvec * N + threadIdx.x]);
            s += f * f;
        }
    }
    flush();
    __syncthreads();
    if ((int)threadIdx.x < n_groups) part[(int64_t)blockIdx.x * n_groups + threadIdx.x] = acc[threadIdx.x];
}

// one block per group: the per-block slots in ascending block order, two per thread, then the fixed tree; nb == 0 writes the zeros
__global__ __launch_bounds__(1024) void sumsq_groups_final_kernel(const float* __restrict__ part, int nb, int n_groups, float* __restrict__ out) {
    __shared__ float red[16];
    const int g = blockIdx.x, t = threadIdx.x;
    float s = t < nb ? part[(int64_t)t * n_groups + g] : 0.f;
    if (t + 1024 < nb) s += part[(int64_t)(t + 1024) * n_groups + g];
    s = block_sum(s, red);
    if (t == 0) out[g] = s;
}

extern "C" int64_t ssi_sumsq_groups_workspace_bytes(int64_t, int, int n_groups) {
    return (int64_t)SSI_SUMSQ_GROUPS_BLOCKS * (n_groups < 1 ? 1 : n_groups) * (int64_t)sizeof(float);
}

extern "C" int ssi_sumsq_groups(const void* x, int64_t n, int dtype, const int64_t* seg_end, const int32_t* seg_group, int n_segs,
                                int n_groups, float* out, void* workspace, int64_t workspace_bytes, void* stream) {
    SSI_CHECK_ARG(out && n >= 0 && (x || n == 0) && ((uintptr_t)x % 16) == 0 && seg_end && seg_group && n_segs >= 1 && n_groups >= 1);
    SSI_CHECK_ARG(dtype == SSI_F32 || dtype == SSI_BF16);
    if (n_segs > SSI_SUMSQ_MAX_SEGS) { ssi_set_error("sumsq_groups: %d segments, at most %d", n_segs, SSI_SUMSQ_MAX_SEGS); return SSI_ERR_UNSUPPORTED; }
    if (n_groups > SSI_SUMSQ_MAX_GROUPS) { ssi_set_error("sumsq_groups: %d groups, at most %d", n_groups, SSI_SUMSQ_MAX_GROUPS); return SSI_ERR_UNSUPPORTED; }
    SSI_CHECK_ARG(seg_end[n_segs - 1] == n);
    if (n == 0) SSI_CHECK_ARG(n_segs == 1);
    for (int s = 0; s < n_segs; ++s) {
        SSI_CHECK_ARG(n == 0 || seg_end[s] > (s ? seg_end[s - 1] : 0));   // strictly ascending
        SSI_CHECK_ARG(s == n_segs - 1 || seg_end[s] % 8 == 0);            // a 16-byte vector lies in ONE segment
        SSI_CHECK_ARG(seg_group[s] >= -1 && seg_group[s] < n_groups);
    }
    if (n >= ((int64_t)1 << 35) - 8) { ssi_set_error("sumsq_groups: n = %lld is beyond the 32-bit unit index", (long long)n); return SSI_ERR_UNSUPPORTED; }
    if (!workspace || workspace_bytes < ssi_sumsq_groups_workspace_bytes(n, n_segs, n_groups)) { ssi_set_error("sumsq_groups: workspace too small"); return SSI_ERR_WORKSPACE; }
    // skipped segments at either end are not launched over: the launch covers [first read start, last read end)
    int s0 = 0, s1 = n_segs;
    while (s0 < n_segs && seg_group[s0] < 0) ++s0;
    int nb = 0;
    if (n > 0 && s0 < n_segs) {
        while (seg_group[s1 - 1] < 0) --s1;
        const int64_t lo = s0 ? seg_end[s0 - 1] : 0, nn = seg_end[s1 - 1] - lo;
        SumsqGroupTable tab;
        for (int s = 0; s < SSI_SUMSQ_MAX_SEGS; ++s) { tab.end8[s] = 0xFFFFFFFFu; tab.group[s] = -1; }
        tab.n_segs = s1 - s0;
        for (int s = s0; s < s1; ++s) {
            tab.end8[s - s0] = (uint32_t)((seg_end[s] - lo + 7) / 8);
            tab.group[s - s0] = seg_group[s];
        }
        for (int k = 0; k < SSI_SUMSQ_MAX_SEGS / 16; ++k) tab.coarse[k] = tab.end8[16 * k + 15];
        const size_t esz = dtype == SSI_BF16 ? 2 : 4;   // lo is a multiple of 8 elements: the 16-byte alignment holds
        const char* xp = (const char*)x + lo * esz;
        const int per = dtype == SSI_BF16 ? 8 : 4;
        const int64_t tiles = ssi_cdiv(nn / per, 256);
        int64_t tpb = ssi_cdiv(tiles, SSI_SUMSQ_GROUPS_BLOCKS);
        if (tpb < 1) tpb = 1;
        nb = (int)ssi_cdiv(tiles, tpb);
        if (nb < 1) nb = 1;
        const int tail_group = (nn % per) ? seg_group[s1 - 1] : -1;   // (a tail exists only when the last segment is read: skipped ends are cut at multiples of 8)
        SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(sumsq_groups_partial_kernel<T>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream,
                                                     (const T*)xp, nn, tab, (int)tpb, n_groups, tail_group, (float*)workspace));
        SSI_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sumsq_groups_final_kernel, dim3((unsigned)n_groups), dim3(1024), 0, (hipStream_t)stream, (const float*)workspace, nb,
                       n_groups, out);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

// =====================================================================================================================
// K13s AdamW with stochastic rounding of the three bf16 stores (ABI v11; opt-in, HipAdamW(stochastic_rounding=True)).  Round-to-nearest
// drops every update below half a bf16 step: v * 0.999 rounds back to v for every bf16 v, and a weight at 1.0 never moves at lr 2e-4
// (profiles/LAB_NOTES.md).  The rounding is defined on the bit pattern and the random bits come from a counter-based generator keyed by
// (seed, step, global element index, tensor): no state, the same bits in every launch, on every rank and after every resume.
// =====================================================================================================================
// (Philox4x32-10 itself is in common_hip.h: the sampler of decode_sample.hip draws from it, too.)
// the 64 random bits of tensor `tensor` for the 8-element vector j (= global element index >> 3) at optimizer step `step`
__device__ __forceinline__ Philox4 sr_bits(int64_t j, uint32_t step, uint32_t tensor, uint64_t seed) {
    return philox4x32_10((uint32_t)j, (uint32_t)((uint64_t)j >> 32), step, tensor, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// fp32 -> bf16 bit pattern, element k of its vector: add 16 random bits below the bf16 mantissa and truncate, so the neighbour away from zero
// is taken with probability (low 16 bits) / 65536 and a value bf16 holds is never changed.  inf / NaN: the round-to-nearest conversion; a
// finite value is never carried into inf.
__device__ __forceinline__ unsigned short sr_bf16(float x, const Philox4& b, int k) {
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7F800000u) == 0x7F800000u) return __builtin_bit_cast(unsigned short, (bf16_t)x);
    const uint32_t t = u + ((b.w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu);
    return (unsigned short)(((t & 0x7F800000u) == 0x7F800000u ? u : t) >> 16);
}
__device__ __forceinline__ bf16_t sr_bf16_value(float x, const Philox4& b, int k) { return __builtin_bit_cast(bf16_t, sr_bf16(x, b, k)); }

// =====================================================================================================================
// K13g AdamW over SEGMENTS of the flat buffers (ABI v16; opt-in, HipAdamW(param_segments=...)): consecutive element ranges with their own
// lr, weight decay and frozen flag in ONE launch.  The table travels by value in the kernel arguments (no device allocation, no copy
// enqueued).  Segment ends are multiples of 8 elements (all but the last), so a 16-byte vector never straddles one: the table is kept in
// UNITS of 8 elements, 32 bits per end.  A block finds the segment of its first unit with wave-uniform indices only (scalar loads, two
// dependent rounds: 8 coarse ends, then the 16 ends of one chunk), walks the segments that reach into its 256 vectors (one, almost always)
// and lets every lane keep the coefficients of the segment its vector lies in.  A lane of a frozen segment issues no load and no store.  The
// random bits are a function of the global element index, so a segment is bit-equal to the plain kernel run on it alone.
// =====================================================================================================================
struct AdamwSegTable {
    uint32_t end8[SSI_ADAMW_MAX_SEGS];        // exclusive end of segment s in units of 8 elements (the last: rounded up); unused: 0xFFFFFFFF
    float decay[SSI_ADAMW_MAX_SEGS];          // (float)(1 - lr * weight_decay)
    float step_size[SSI_ADAMW_MAX_SEGS];      // (float)(lr / bc1)
    uint32_t coarse[SSI_ADAMW_MAX_SEGS / 16]; // end8[16 k + 15]
    uint32_t frozen[SSI_ADAMW_MAX_SEGS / 32]; // bit s: segment s is frozen
    int n_segs;
};

// the gradient factor of segment s under GS: one correctly rounded product of the launch's scale and the segment's DEVICE scale (a scalar load:
// s is wave-uniform), or the segment's scale alone when the launch has none
__device__ __forceinline__ float adamw_seg_gscale(const float* __restrict__ grad_scale_dev, float gs_launch, const float* __restrict__ seg_scale_dev, int s) {
    const float ss = seg_scale_dev[s];
    return grad_scale_dev ? gs_launch * ss : ss;
}

// coefficients of the segment unit `u` lies in, for a block whose vectors cover the units [ub0, ub1]; false: frozen (or past the last end).
// GS: gs becomes the segment's gradient factor, and a segment whose factor is not finite counts as frozen
template <bool GS>
__device__ __forceinline__ bool adamw_seg_lookup(const AdamwSegTable& t, uint32_t ub0, uint32_t ub1, uint32_t u, float& decay, float& step_size,
                                                 const float* __restrict__ grad_scale_dev, float gs_launch, const float* __restrict__ seg_scale_dev, float& gs) {
    int c = 0;
#pragma unroll
    for (int k = 0; k < SSI_ADAMW_MAX_SEGS / 16 - 1; ++k) c += ub0 >= t.coarse[k] ? 1 : 0;
    int s = 16 * c;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += ub0 >= t.end8[16 * c + k] ? 1 : 0;
    uint32_t start = s ? t.end8[s - 1] : 0u;
    bool active = false;
    for (; s < t.n_segs && start <= ub1; ++s) {   // every index here is wave-uniform: the lanes only select
        const uint32_t end = t.end8[s];
        [[maybe_unused]] float gs_s = 0.f;
        if constexpr (GS) gs_s = adamw_seg_gscale(grad_scale_dev, gs_launch, seg_scale_dev, s);
        if (u >= start && u < end) {
            decay = t.decay[s];
            step_size = t.step_size[s];
            active = !((t.frozen[s >> 5] >> (s & 31)) & 1u);
            if constexpr (GS) { gs = gs_s; active = active && fabsf(gs_s) < INFINITY; }
        }
        start = end;
    }
    return active;
}

// =====================================================================================================================
// K13 AdamW: ONE element function and ONE body behind the seven kernels.  SR: the three stores round stochastically; SEG: decay and step_size
// come per segment from the table; GS (ABI v23, with SEG): the gradient factor too, from a per-segment DEVICE scale.  Built with -ffp-contract=fast, the variants agree bit for bit because the arithmetic is written once.
// =====================================================================================================================
struct AdamwCoef { float w1, beta2, w2, eps, inv_bc2_sqrt; };           // what every element of a launch shares
struct AdamwSr { uint64_t seed; uint32_t step; int64_t vec_offset; };   // SR: the generator's key and the slice's first vector in the global index

// fp32 -> storage, element k of its vector: to nearest, or (SR) by the vector's random bits b
template <typename T, bool SR> __device__ __forceinline__ T adamw_rounded(float x, const Philox4& b, int k) {
    if constexpr (SR) return sr_bf16_value(x, b, k);
    else return from_f32<T>(x);
}

__device__ __forceinline__ void adamw_elem(float& pf, float& mf, float& vf, float gr, float decay, float step_size, const AdamwCoef& c) {
    pf *= decay;
    mf = mf + c.w1 * (gr - mf);
    vf = c.beta2 * vf + c.w2 * gr * gr;
    const float denom = sqrtf(vf) * c.inv_bc2_sqrt + c.eps;
    pf -= step_size * mf / denom;
}

template <typename T, bool SEG, bool SR, bool GS = false>
__device__ __forceinline__ void adamw_body(T* __restrict__ p, T* __restrict__ g, T* __restrict__ m, T* __restrict__ v, int64_t n,
                                           const AdamwSegTable* tab, float decay, float step_size, const AdamwCoef c,
                                           const float* __restrict__ grad_scale_dev, int zero_grad, const AdamwSr sr,
                                           const float* __restrict__ seg_scale_dev = nullptr) {
    constexpr int N = Vec16<T>::N;
    static_assert(!SR || N == 8, "one Philox call per tensor covers the 8 elements of a 16-byte vector");
    static_assert(!GS || SEG, "the device scale is per segment");
    const float gs = grad_scale_dev ? *grad_scale_dev : 1.f;
    [[maybe_unused]] float gs_seg = gs;   // GS: the factor of the segment the lane's vector lies in, set by the lookup
    if ((zero_grad & 2) && !(fabsf(gs) < INFINITY)) return;  // bit 1: a non-finite scale (an accumulation window without a label) changes nothing
    zero_grad &= 1;
    const int64_t nvec = n / N;
    // one vector per thread and trip.  Plain: b is the thread's vector.  SEG: b is the block's first vector, which the lookup needs wave-uniform
    for (int64_t b = (int64_t)blockIdx.x * 256 + (SEG ? 0 : threadIdx.x); b < nvec; b += (int64_t)gridDim.x * 256) {
        const int64_t i = SEG ? b + threadIdx.x : b;
        if constexpr (SEG) {
            const bool active = adamw_seg_lookup<GS>(*tab, (uint32_t)((b * N) >> 3), (uint32_t)(((b + 255) * N) >> 3), (uint32_t)((i * N) >> 3), decay,
                                                     step_size, grad_scale_dev, gs, seg_scale_dev, gs_seg);
            if (!active || i >= nvec) continue;
        }
        Vec16<T> pp = load16_nt(p + i * N), gg = load16_nt(g + i * N), mm = load16_nt(m + i * N), vv = load16_nt(v + i * N);
        // one generator call per tensor and vector; only the SR stores read the bits, so without SR none is compiled
        const Philox4 rp = sr_bits(sr.vec_offset + i, sr.step, 0, sr.seed), rm = sr_bits(sr.vec_offset + i, sr.step, 1, sr.seed),
                      rv = sr_bits(sr.vec_offset + i, sr.step, 2, sr.seed);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            float pf = pp.get(k), mf = mm.get(k), vf = vv.get(k);
            adamw_elem(pf, mf, vf, gg.get(k) * (GS ? gs_seg : gs), decay, step_size, c);
            pp.v[k] = adamw_rounded<T, SR>(pf, rp, k); mm.v[k] = adamw_rounded<T, SR>(mf, rm, k); vv.v[k] = adamw_rounded<T, SR>(vf, rv, k);
            if (zero_grad) gg.set(k, 0.f);
        }
        store16_nt(p + i * N, pp); store16_nt(m + i * N, mm); store16_nt(v + i * N, vv);
        if (zero_grad) store16_nt(g + i * N, gg);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n - nvec * N)) {
        if constexpr (SEG) {
            const int last = tab->n_segs - 1;   // the ragged tail belongs to the last segment
            if ((tab->frozen[last >> 5] >> (last & 31)) & 1u) return;
            decay = tab->decay[last];
            step_size = tab->step_size[last];
            if constexpr (GS) {
                gs_seg = adamw_seg_gscale(grad_scale_dev, gs, seg_scale_dev, last);
                if (!(fabsf(gs_seg) < INFINITY)) return;
            }
        }
        const int k = threadIdx.x;   // SR: the slice starts on a vector boundary of the global index, so the tail is the head of vector vec_offset + nvec
        const int64_t i = nvec * N + k;
        float pf = to_f32<T>(p[i]), mf = to_f32<T>(m[i]), vf = to_f32<T>(v[i]);
        adamw_elem(pf, mf, vf, to_f32<T>(g[i]) * (GS ? gs_seg : gs), decay, step_size, c);
        p[i] = adamw_rounded<T, SR>(pf, sr_bits(sr.vec_offset + nvec, sr.step, 0, sr.seed), k);
        m[i] = adamw_rounded<T, SR>(mf, sr_bits(sr.vec_offset + nvec, sr.step, 1, sr.seed), k);
        v[i] = adamw_rounded<T, SR>(vf, sr_bits(sr.vec_offset + nvec, sr.step, 2, sr.seed), k);
        if (zero_grad) g[i] = from_f32<T>(0.f);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void adamw_kernel(T* __restrict__ p, T* __restrict__ g, T* __restrict__ m,
                                                    T* __restrict__ v, int64_t n, float decay, float w1, float beta2,
                                                    float w2, float eps, float step_size, float inv_bc2_sqrt,
                                                    const float* __restrict__ grad_scale_dev, int zero_grad) {
    adamw_body<T, false, false>(p, g, m, v, n, nullptr, decay, step_size, AdamwCoef{w1, beta2, w2, eps, inv_bc2_sqrt}, grad_scale_dev, zero_grad, AdamwSr{});
}

__global__ __launch_bounds__(256) void adamw_sr_kernel(bf16_t* __restrict__ p, bf16_t* __restrict__ g, bf16_t* __restrict__ m,
                                                       bf16_t* __restrict__ v, int64_t n, float decay, float w1, float beta2, float w2,
                                                       float eps, float step_size, float inv_bc2_sqrt,
                                                       const float* __restrict__ grad_scale_dev, int zero_grad, uint64_t seed,
                                                       uint32_t step, int64_t vec_offset) {
    adamw_body<bf16_t, false, true>(p, g, m, v, n, nullptr, decay, step_size, AdamwCoef{w1, beta2, w2, eps, inv_bc2_sqrt}, grad_scale_dev, zero_grad,
                                    AdamwSr{seed, step, vec_offset});
}

template <typename T>
__global__ __launch_bounds__(256) void adamw_seg_kernel(T* __restrict__ p, T* __restrict__ g, T* __restrict__ m, T* __restrict__ v, int64_t n,
                                                        const AdamwSegTable tab, float w1, float beta2, float w2, float eps, float inv_bc2_sqrt,
                                                        const float* __restrict__ grad_scale_dev, int zero_grad) {
    adamw_body<T, true, false>(p, g, m, v, n, &tab, 0.f, 0.f, AdamwCoef{w1, beta2, w2, eps, inv_bc2_sqrt}, grad_scale_dev, zero_grad, AdamwSr{});
}

__global__ __launch_bounds__(256) void adamw_seg_sr_kernel(bf16_t* __restrict__ p, bf16_t* __restrict__ g, bf16_t* __restrict__ m,
                                                           bf16_t* __restrict__ v, int64_t n, const AdamwSegTable tab, float w1, float beta2,
                                                           float w2, float eps, float inv_bc2_sqrt, const float* __restrict__ grad_scale_dev,
                                                           int zero_grad, uint64_t seed, uint32_t step, int64_t vec_offset) {
    adamw_body<bf16_t, true, true>(p, g, m, v, n, &tab, 0.f, 0.f, AdamwCoef{w1, beta2, w2, eps, inv_bc2_sqrt}, grad_scale_dev, zero_grad,
                                   AdamwSr{seed, step, vec_offset});
}

template <typename T>
__global__ __launch_bounds__(256) void adamw_gscale_kernel(T* __restrict__ p, T* __restrict__ g, T* __restrict__ m, T* __restrict__ v, int64_t n,
                                                           const AdamwSegTable tab, float w1, float beta2, float w2, float eps, float inv_bc2_sqrt,
                                                           const float* __restrict__ grad_scale_dev, int zero_grad,
                                                           const float* __restrict__ seg_scale_dev) {
    adamw_body<T, true, false, true>(p, g, m, v, n, &tab, 0.f, 0.f, AdamwCoef{w1, beta2, w2, eps, inv_bc2_sqrt}, grad_scale_dev, zero_grad, AdamwSr{},
                                     seg_scale_dev);
}

__global__ __launch_bounds__(256) void adamw_gscale_sr_kernel(bf16_t* __restrict__ p, bf16_t* __restrict__ g, bf16_t* __restrict__ m,
                                                              bf16_t* __restrict__ v, int64_t n, const AdamwSegTable tab, float w1, float beta2,
                                                              float w2, float eps, float inv_bc2_sqrt, const float* __restrict__ grad_scale_dev,
                                                              int zero_grad, uint64_t seed, uint32_t step, int64_t vec_offset,
                                                              const float* __restrict__ seg_scale_dev) {
    adamw_body<bf16_t, true, true, true>(p, g, m, v, n, &tab, 0.f, 0.f, AdamwCoef{w1, beta2, w2, eps, inv_bc2_sqrt}, grad_scale_dev, zero_grad,
                                         AdamwSr{seed, step, vec_offset}, seg_scale_dev);
}

static int adamw_check_buffers(const void* param, const void* grad, const void* exp_avg, const void* exp_avg_sq, int64_t n, int64_t step) {
    SSI_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && n >= 0 && step >= 1);
    SSI_CHECK_ARG(((uintptr_t)param % 16) == 0 && ((uintptr_t)grad % 16) == 0 && ((uintptr_t)exp_avg % 16) == 0 &&
                  ((uintptr_t)exp_avg_sq % 16) == 0);
    return SSI_OK;
}

// A step's coefficients: every one in double from the double hyper-parameters, then rounded once to fp32, as torch's fused AdamW does:
// 1 - (float)0.999 is 1.3e-5 away from (float)(1 - 0.999), which moved ~0.5 % of the bf16 exp_avg_sq (and, through the cancellations of m,
// ~4 % of the exp_avg) a bf16 step away from the reference's within 7 steps
struct AdamwStep {
    double bc1;   // 1 - beta1^step, kept in double for step_size
    AdamwCoef c;
    AdamwStep(double beta1, double beta2, double eps, int64_t step)
        : bc1(1.0 - pow(beta1, (double)step)),
          c{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)(1.0 / sqrt(1.0 - pow(beta2, (double)step)))} {}
    float decay(double lr, double weight_decay) const { return (float)(1.0 - lr * weight_decay); }
    float step_size(double lr) const { return (float)(lr / bc1); }
};

// 17 GB touched once: non-temporal accesses and as many short blocks as there are 16-byte vectors (no grid-stride loop at the model's
// size: 608 k blocks).  tools/adamw_bench.py, 1.246 G bf16 parameters: 8192 long-lived blocks 5.5 TB/s, 32768 6.2, 131072 6.3, one vector
// per thread 6.47 TB/s (2.70 ms); two vectors per thread with all eight loads in flight first: 6.1
template <typename T> static dim3 adamw_grid(int64_t n) { return dim3(stream_grid(n / Vec16<T>::N + 1, 1 << 20)); }

extern "C" int ssi_adamw_step(void* param, void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, double lr, double beta1,
                              double beta2, double eps, double weight_decay, int64_t step, const float* grad_scale_dev,
                              int zero_grad, int dtype, void* stream) {
    if (const int rc = adamw_check_buffers(param, grad, exp_avg, exp_avg_sq, n, step)) return rc;
    if (n == 0) return SSI_OK;
    const AdamwStep s(beta1, beta2, eps, step);
    SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(adamw_kernel<T>, adamw_grid<T>(n), dim3(256), 0, (hipStream_t)stream, (T*)param, (T*)grad,
                                                 (T*)exp_avg, (T*)exp_avg_sq, n, s.decay(lr, weight_decay), s.c.w1, s.c.beta2, s.c.w2, s.c.eps,
                                                 s.step_size(lr), s.c.inv_bc2_sqrt, grad_scale_dev, zero_grad));
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

extern "C" int ssi_adamw_step_sr(void* param, void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, double lr, double beta1,
                                 double beta2, double eps, double weight_decay, int64_t step, const float* grad_scale_dev,
                                 int zero_grad, int dtype, uint64_t seed, int64_t elem_offset, void* stream) {
    if (const int rc = adamw_check_buffers(param, grad, exp_avg, exp_avg_sq, n, step)) return rc;
    SSI_CHECK_ARG(dtype == SSI_BF16);   // fp32 storage has nothing to round
    SSI_CHECK_ARG(step < ((int64_t)1 << 32) && elem_offset >= 0 && elem_offset % 8 == 0);
    if (n == 0) return SSI_OK;
    const AdamwStep s(beta1, beta2, eps, step);
    hipLaunchKernelGGL(adamw_sr_kernel, adamw_grid<bf16_t>(n), dim3(256), 0, (hipStream_t)stream, (bf16_t*)param, (bf16_t*)grad,
                       (bf16_t*)exp_avg, (bf16_t*)exp_avg_sq, n, s.decay(lr, weight_decay), s.c.w1, s.c.beta2, s.c.w2, s.c.eps, s.step_size(lr),
                       s.c.inv_bc2_sqrt, grad_scale_dev, zero_grad, seed, (uint32_t)step, elem_offset / 8);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

// the segmented launch; seg_scale_dev: NULL (ssi_adamw_step_seg) or the per-segment device scales (ssi_adamw_step_seg_gscale)
static int adamw_step_seg_launch(void* param, void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, const int64_t* seg_end,
                                 const double* seg_lr, const double* seg_weight_decay, const int32_t* seg_frozen, int n_segs,
                                 double beta1, double beta2, double eps, int64_t step, const float* grad_scale_dev, int zero_grad,
                                 int dtype, int stochastic, uint64_t seed, int64_t elem_offset, const float* seg_scale_dev, void* stream) {
    if (const int rc = adamw_check_buffers(param, grad, exp_avg, exp_avg_sq, n, step)) return rc;
    SSI_CHECK_ARG(seg_end && seg_lr && seg_weight_decay && seg_frozen && n_segs >= 1);
    SSI_CHECK_ARG(dtype == SSI_F32 || dtype == SSI_BF16);
    if (stochastic) SSI_CHECK_ARG(dtype == SSI_BF16 && step < ((int64_t)1 << 32) && elem_offset >= 0 && elem_offset % 8 == 0);
    if (n_segs > SSI_ADAMW_MAX_SEGS) { ssi_set_error("adamw_step_seg: %d segments, at most %d per launch", n_segs, SSI_ADAMW_MAX_SEGS); return SSI_ERR_UNSUPPORTED; }
    SSI_CHECK_ARG(seg_end[n_segs - 1] == n);
    if (n == 0) { SSI_CHECK_ARG(n_segs == 1); return SSI_OK; }
    for (int s = 0; s < n_segs; ++s) {
        SSI_CHECK_ARG(seg_end[s] > (s ? seg_end[s - 1] : 0));            // strictly ascending
        SSI_CHECK_ARG(s == n_segs - 1 || seg_end[s] % 8 == 0);           // a 16-byte vector lies in ONE segment
    }
    if (n >= ((int64_t)1 << 35) - 8) { ssi_set_error("adamw_step_seg: n = %lld is beyond the 32-bit unit index", (long long)n); return SSI_ERR_UNSUPPORTED; }
    // frozen segments at either end are not launched over at all: the launch covers [first trainable start, last trainable end)
    int s0 = 0, s1 = n_segs;
    while (s0 < n_segs && seg_frozen[s0]) ++s0;
    if (s0 == n_segs) return SSI_OK;
    while (seg_frozen[s1 - 1]) --s1;
    const int64_t lo = s0 ? seg_end[s0 - 1] : 0, nn = seg_end[s1 - 1] - lo;
    const AdamwStep st(beta1, beta2, eps, step);
    AdamwSegTable tab;
    for (int s = 0; s < SSI_ADAMW_MAX_SEGS; ++s) { tab.end8[s] = 0xFFFFFFFFu; tab.decay[s] = 1.f; tab.step_size[s] = 0.f; }
    for (int k = 0; k < SSI_ADAMW_MAX_SEGS / 32; ++k) tab.frozen[k] = 0u;
    tab.n_segs = s1 - s0;
    for (int s = s0; s < s1; ++s) {
        const int j = s - s0;
        tab.end8[j] = (uint32_t)((seg_end[s] - lo + 7) / 8);
        tab.decay[j] = st.decay(seg_lr[s], seg_weight_decay[s]);
        tab.step_size[j] = st.step_size(seg_lr[s]);
        if (seg_frozen[s]) tab.frozen[j >> 5] |= 1u << (j & 31);
    }
    for (int k = 0; k < SSI_ADAMW_MAX_SEGS / 16; ++k) tab.coarse[k] = tab.end8[16 * k + 15];
    const size_t esz = dtype == SSI_BF16 ? 2 : 4;   // lo is a multiple of 8 elements: the 16-byte alignment holds
    char *pp = (char*)param + lo * esz, *gp = (char*)grad + lo * esz, *mp = (char*)exp_avg + lo * esz, *vp = (char*)exp_avg_sq + lo * esz;
    if (seg_scale_dev) {   // the scales of the segments the launch covers
        const float* ssd = seg_scale_dev + s0;
        if (stochastic) {
            hipLaunchKernelGGL(adamw_gscale_sr_kernel, adamw_grid<bf16_t>(nn), dim3(256), 0, (hipStream_t)stream, (bf16_t*)pp, (bf16_t*)gp, (bf16_t*)mp,
                               (bf16_t*)vp, nn, tab, st.c.w1, st.c.beta2, st.c.w2, st.c.eps, st.c.inv_bc2_sqrt, grad_scale_dev, zero_grad, seed,
                               (uint32_t)step, (elem_offset + lo) / 8, ssd);
        } else {
            SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(adamw_gscale_kernel<T>, adamw_grid<T>(nn), dim3(256), 0, (hipStream_t)stream, (T*)pp, (T*)gp,
                                                         (T*)mp, (T*)vp, nn, tab, st.c.w1, st.c.beta2, st.c.w2, st.c.eps, st.c.inv_bc2_sqrt,
                                                         grad_scale_dev, zero_grad, ssd));
        }
    } else if (stochastic) {
        hipLaunchKernelGGL(adamw_seg_sr_kernel, adamw_grid<bf16_t>(nn), dim3(256), 0, (hipStream_t)stream, (bf16_t*)pp, (bf16_t*)gp, (bf16_t*)mp,
                           (bf16_t*)vp, nn, tab, st.c.w1, st.c.beta2, st.c.w2, st.c.eps, st.c.inv_bc2_sqrt, grad_scale_dev, zero_grad, seed,
                           (uint32_t)step, (elem_offset + lo) / 8);
    } else {
        SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(adamw_seg_kernel<T>, adamw_grid<T>(nn), dim3(256), 0, (hipStream_t)stream, (T*)pp, (T*)gp,
                                                     (T*)mp, (T*)vp, nn, tab, st.c.w1, st.c.beta2, st.c.w2, st.c.eps, st.c.inv_bc2_sqrt,
                                                     grad_scale_dev, zero_grad));
    }
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

extern "C" int ssi_adamw_step_seg(void* param, void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, const int64_t* seg_end,
                                  const double* seg_lr, const double* seg_weight_decay, const int32_t* seg_frozen, int n_segs,
                                  double beta1, double beta2, double eps, int64_t step, const float* grad_scale_dev, int zero_grad,
                                  int dtype, int stochastic, uint64_t seed, int64_t elem_offset, void* stream) {
    return adamw_step_seg_launch(param, grad, exp_avg, exp_avg_sq, n, seg_end, seg_lr, seg_weight_decay, seg_frozen, n_segs, beta1, beta2, eps, step,
                                 grad_scale_dev, zero_grad, dtype, stochastic, seed, elem_offset, nullptr, stream);
}

extern "C" int ssi_adamw_step_seg_gscale(void* param, void* grad, void* exp_avg, void* exp_avg_sq, int64_t n, const int64_t* seg_end,
                                         const double* seg_lr, const double* seg_weight_decay, const int32_t* seg_frozen, int n_segs,
                                         double beta1, double beta2, double eps, int64_t step, const float* grad_scale_dev, int zero_grad,
                                         int dtype, int stochastic, uint64_t seed, int64_t elem_offset, const float* seg_scale_dev, void* stream) {
    SSI_CHECK_ARG(seg_scale_dev && ((uintptr_t)seg_scale_dev % 4) == 0);
    return adamw_step_seg_launch(param, grad, exp_avg, exp_avg_sq, n, seg_end, seg_lr, seg_weight_decay, seg_frozen, n_segs, beta1, beta2, eps, step,
                                 grad_scale_dev, zero_grad, dtype, stochastic, seed, elem_offset, seg_scale_dev, stream);
}

// the rounding of adamw_sr_kernel on its own: dst[i] = sr_bf16(src[i]) with the bits of (seed, step, elem_offset + i, tensor)
__global__ __launch_bounds__(256) void round_bf16_sr_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int64_t n, uint64_t seed,
                                                            uint32_t step, uint32_t tensor, int64_t vec_offset) {
    const int64_t nvec = n / 8;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
        const Vec16<float> a = load16(src + i * 8), b = load16(src + i * 8 + 4);
        const Philox4 r = sr_bits(vec_offset + i, step, tensor, seed);
        Vec16<bf16_t> o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o.v[k] = sr_bf16_value(k < 4 ? a.get(k) : b.get(k - 4), r, k);
        store16(dst + i * 8, o);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n - nvec * 8)) {
        const int k = threadIdx.x;
        dst[nvec * 8 + k] = sr_bf16_value(src[nvec * 8 + k], sr_bits(vec_offset + nvec, step, tensor, seed), k);
    }
}

extern "C" int ssi_round_bf16_sr(const float* src, void* dst, int64_t n, uint64_t seed, int64_t step, int tensor, int64_t elem_offset,
                                 void* stream) {
    SSI_CHECK_ARG(src && dst && n >= 0 && ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0);
    SSI_CHECK_ARG(step >= 0 && step < ((int64_t)1 << 32) && tensor >= 0 && elem_offset >= 0 && elem_offset % 8 == 0);
    if (n == 0) return SSI_OK;
    hipLaunchKernelGGL(round_bf16_sr_kernel, dim3(stream_grid(n / 8 + 1, 1 << 20)), dim3(256), 0, (hipStream_t)stream, src, (bf16_t*)dst, n,
                       seed, (uint32_t)step, (uint32_t)tensor, elem_offset / 8);
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

// =====================================================================================================================
// K13e fp32 exponential moving average of the parameters (ABI v17; opt-in, HipAdamW(ema_decay=...)): one more pure HBM pass over the flat
// buffer, chained to the AdamW launch on the same stream.  ema = fma(decay, ema - p, p): the subtraction rounded, then ONE fused
// multiply-add, written out (the library is built with -ffp-contract=fast, see ssi_rope_pair).  decay == 0 gives p exactly and ema == p is
// an exact fixed point: the average of a frozen or converged weight never drifts by rounding.  8 elements per thread and trip: one 16-byte
// load of bf16 parameters (two of fp32), two 16-byte loads and two 16-byte stores of the average; no LDS, no scratch, no atomics.
// =====================================================================================================================
__device__ __forceinline__ float ema_elem(float decay, float e, float p) {
    const float d = e - p;
    return __builtin_fmaf(decay, d, p);
}

template <typename T>
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const T* __restrict__ p, int64_t n, float decay,
                                                         const float* __restrict__ guard_dev) {
    if (guard_dev && !(fabsf(*guard_dev) < INFINITY)) return;  // the test of adamw_kernel's zero_grad bit 1: AdamW changed nothing, nor does the average
    const int64_t nvec = n / 8;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
        Vec16<float> e0 = load16_nt(ema + i * 8), e1 = load16_nt(ema + i * 8 + 4);
        if constexpr (Vec16<T>::N == 8) {
            const Vec16<T> pp = load16_nt(p + i * 8);
#pragma unroll
            for (int k = 0; k < 4; ++k) { e0.v[k] = ema_elem(decay, e0.v[k], pp.get(k)); e1.v[k] = ema_elem(decay, e1.v[k], pp.get(k + 4)); }
        } else {
            const Vec16<T> p0 = load16_nt(p + i * 8), p1 = load16_nt(p + i * 8 + 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) { e0.v[k] = ema_elem(decay, e0.v[k], p0.get(k)); e1.v[k] = ema_elem(decay, e1.v[k], p1.get(k)); }
        }
        store16_nt(ema + i * 8, e0); store16_nt(ema + i * 8 + 4, e1);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n - nvec * 8)) {
        const int64_t i = nvec * 8 + threadIdx.x;
        ema[i] = ema_elem(decay, ema[i], to_f32<T>(p[i]));
    }
}

extern "C" int ssi_ema_update(void* ema, const void* param, int64_t n, float decay, const float* guard_dev, int dtype, void* stream) {
    SSI_CHECK_ARG(n >= 0);
    if (!(decay >= 0.f && decay < 1.f)) { ssi_set_error("ema_update: decay = %g, must be in [0, 1)", (double)decay); return SSI_ERR_ARG; }
    if (n == 0) return SSI_OK;
    SSI_CHECK_ARG(ema && param && ((uintptr_t)ema % 16) == 0 && ((uintptr_t)param % 16) == 0);
    // 8 elements per thread; the grid is adamw_kernel's for bf16: one trip per thread up to 2^20 blocks (2^31 elements), the stride loop beyond
    SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(ema_update_kernel<T>, dim3(stream_grid(n / 8 + 1, 1 << 20)), dim3(256), 0, (hipStream_t)stream,
                                                 (float*)ema, (const T*)param, n, decay, guard_dev));
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}

// =====================================================================================================================
// 2-D transpose dst[c][r] = src[r][c] (64 x 64 tiles through LDS; 16-B global accesses on both sides).  Used once per
// optimizer step to refresh the [in, out] copies of the projection weights, so that the data-gradient GEMMs
// dX = dY W run in the k-contiguous (NT) operand form instead of the transposed-read form.
// =====================================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void transpose_kernel(const T* __restrict__ src, int64_t lds_, T* __restrict__ dst, int64_t ldd,
                                                        int64_t rows, int64_t cols) {
    constexpr int N = Vec16<T>::N;          // elements per 16 B
    constexpr int TS = 64;                  // tile edge
    __shared__ T tile[TS][TS + 2 * N / N + 2];  // +pad breaks the power-of-two row stride
    const int64_t r0 = (int64_t)blockIdx.y * TS, c0 = (int64_t)blockIdx.x * TS;
    constexpr int VPR = TS / N;             // vectors per tile row
    for (int v = threadIdx.x; v < TS * VPR; v += 256) {
        const int r = v / VPR, cv = (v % VPR) * N;
        if (r0 + r < rows && c0 + cv < cols) {
            Vec16<T> a = load16(src + (r0 + r) * lds_ + c0 + cv);
#pragma unroll
            for (int i = 0; i < N; ++i) tile[cv + i][r] = from_f32<T>(a.get(i));
        }
    }
    __syncthreads();
    for (int v = threadIdx.x; v < TS * VPR; v += 256) {
        const int c = v / VPR, rv = (v % VPR) * N;
        if (c0 + c < cols && r0 + rv < rows) {
            Vec16<T> o;
#pragma unroll
            for (int i = 0; i < N; ++i) o.set(i, to_f32<T>(tile[c][rv + i]));
            store16(dst + (c0 + c) * ldd + r0 + rv, o);
        }
    }
}

extern "C" int ssi_transpose(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows, int64_t cols, int dtype,
                             void* stream) {
    SSI_CHECK_ARG(src && dst && rows >= 0 && cols >= 0 && ld_src >= cols && ld_dst >= rows);
    SSI_CHECK_ARG(rows % 8 == 0 && cols % 8 == 0 && ld_src % 8 == 0 && ld_dst % 8 == 0);
    if (rows == 0 || cols == 0) return SSI_OK;
    SSI_CHECK_ARG(ssi_cdiv(rows, 64) <= 65535);
    dim3 grid((unsigned)ssi_cdiv(cols, 64), (unsigned)ssi_cdiv(rows, 64));
    SSI_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(transpose_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (const T*)src, ld_src,
                                                 (T*)dst, ld_dst, rows, cols));
    SSI_LAUNCH_CHECK();
    return SSI_OK;
}
