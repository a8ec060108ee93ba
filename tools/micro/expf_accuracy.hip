// How accurate are expf and logf as the library's flags compile them?  hipcc expands both in line with an extended-precision product
// (ph = x c, pl = fma(x, c, -ph) + x c_tail); under -ffp-contract=fast the backend fuses `ph - rint(ph)` (expf) and `ph + pl` (logf) with the
// product into one fma on the exact product, which counts the low part twice: expf(x) is then off by up to 2^-24 |x| relative on top of its
// 1 ulp.  Sweeps 65 536 arguments of each against the host's double; the first expf argument is the element at which tests/ce_parity.py's
// bound for the generic cross-entropy form was first missed.  Build it twice and compare:
//   hipcc -O3 -std=c++17 -ffp-contract=fast --offload-arch=gfx950 tools/micro/expf_accuracy.hip -o tools/micro/expf_accuracy
//   hipcc -O3 -std=c++17 -ffp-contract=off  --offload-arch=gfx950 tools/micro/expf_accuracy.hip -o tools/micro/expf_accuracy
// MI355X: fast — expf worst 45.2 x 2^-24 = 44.3 ulp, (error - 2 x 2^-24) / (2^-24 |x|) <= 0.947, logf 2.21 ulp; off — expf 0.81 ulp, logf 1.88 ulp.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>
__global__ void k_exp(float* o, const float* a, int n) { int i = blockIdx.x * 256 + threadIdx.x; if (i < n) o[i] = expf(a[i]); }
__global__ void k_log(float* o, const float* a, int n) { int i = blockIdx.x * 256 + threadIdx.x; if (i < n) o[i] = logf(a[i]); }
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 2; } } while (0)
int main() {
    const int n = 1 << 16;
    const double U32 = ldexp(1.0, -24);
    std::vector<float> a(n), b(n), o(n);
    a[0] = -16.466796875f;
    for (int i = 1; i < n; ++i) a[i] = -87.0f * (float)i / (float)n - 0.0001f * (float)(i % 97);
    for (int i = 0; i < n; ++i) b[i] = 1.0f + 1.0e6f * (float)i / (float)n + 0.37f * (float)(i % 89);
    float *da, *dout;
    CK(hipMalloc(&da, n * 4)); CK(hipMalloc(&dout, n * 4));
    CK(hipMemcpy(da, a.data(), n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_exp, dim3(n / 256), dim3(256), 0, 0, dout, da, n);
    CK(hipGetLastError()); CK(hipMemcpy(o.data(), dout, n * 4, hipMemcpyDeviceToHost));
    double worst_rel = 0, worst_perx = 0, worst_ulp = 0;
    for (int i = 0; i < n; ++i) {
        const double ref = exp((double)a[i]); if (ref < 1.2e-38) continue;
        const double rel = fabs((double)o[i] - ref) / ref / U32;
        int ex; frexp(ref, &ex); const double ulps = fabs((double)o[i] - ref) / ldexp(1.0, ex - 24);
        if (rel > worst_rel) worst_rel = rel;
        if (ulps > worst_ulp) worst_ulp = ulps;
        const double per = (rel - 2.0) / fabs((double)a[i]); if (per > worst_perx) worst_perx = per;
        if (i == 0) printf("expf(%.9f) = %.9e  fp64 %.12e  rel err %.2f U32 = %.2f ulp\n", a[i], o[i], ref, rel, ulps);
    }
    printf("expf sweep [-87, 0]: worst rel err %.2f U32, worst %.2f ulp, worst (rel - 2 U32) / (U32 |x|) = %.3f\n", worst_rel, worst_ulp, worst_perx);
    CK(hipMemcpy(da, b.data(), n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_log, dim3(n / 256), dim3(256), 0, 0, dout, da, n);
    CK(hipGetLastError()); CK(hipMemcpy(o.data(), dout, n * 4, hipMemcpyDeviceToHost));
    double wl = 0, wu = 0;
    for (int i = 1; i < n; ++i) {
        const double ref = log((double)b[i]); if (ref < 1e-3) continue;
        const double rel = fabs((double)o[i] - ref) / ref / U32;
        int ex; frexp(ref, &ex); const double ulps = fabs((double)o[i] - ref) / ldexp(1.0, ex - 24);
        if (rel > wl) wl = rel; if (ulps > wu) wu = ulps;
    }
    printf("logf sweep [1, 1e6]: worst err %.2f U32 |logf|, worst %.2f ulp\n", wl, wu);
    return 0;
}
