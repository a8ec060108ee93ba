"""FP8 weights restated on the CPU: the row rule of include/ssi_hip.h ("FP8 weights") is the "FP8 K/V cache" rule with a ROW of a weight matrix
``W[N, K]`` as the line, so this file only re-reads ``kv_fp8_ref.quantise`` / ``dequantise`` that way (one "kv head" per row).  Nothing here calls
a kernel; test_weight_fp8_ref.py checks it, the GPU tests test_weight_quant_fp8_gpu.py, test_gemm_wq8_gpu.py and test_weight_fp8_model_gpu.py
check the kernels against it."""
import math

import torch

import kv_fp8_ref as kq

NAN_CODE = kq.NAN_CODE
POISON_EXP = kq.POISON_EXP
BF = torch.bfloat16


def quantise(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """bf16 ``w`` [N, K] -> (codes uint8 [N, K], exponent bytes uint8 [N])."""
    assert w.dim() == 2 and w.dtype == BF
    codes, b = kq.quantise(w[:, None, :])
    return codes[:, 0].contiguous(), b[:, 0].contiguous()


def dequantise(codes: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """fp32 [N, K]: ``float(code) * 2^(b - 127)`` (exact)."""
    return kq.dequantise(codes[:, None, :], b[:, None])[:, 0]


def dequantise_bf16(codes: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The dequantised matrix stored as bf16, which the bit-equality contract of the ``_w8`` GEMMs is stated on; asserts that the store is exact
    (every finite value is a bf16 number: the header's guarantee for rows in the bf16 normal range)."""
    f = dequantise(codes, b)
    out = f.to(BF)
    fin = torch.isfinite(f)
    assert torch.equal(out.float()[fin], f[fin]) and bool(torch.isnan(out[~fin]).all())
    return out


def edge_rows(K: int, seed: int = 5) -> tuple[torch.Tensor, tuple]:
    """bf16 [n, K] rows at the edges of the rule, and their names: normal(0, 0.02) rows, a zero row, an absmax whose mantissa is exactly 1.75 and
    one a bf16 step above it, a row whose only large element is the last, -0.0 among the elements, a NaN element, an infinite element."""
    g = torch.Generator().manual_seed(seed)
    normal = lambda: torch.randn(K, generator=g) * 0.02  # noqa: E731
    rows, names = [], []

    def add(name, x):
        rows.append(x.float())
        names.append(name)

    add("normal", normal())
    add("normal 2", normal())
    add("zeros", torch.zeros(K))
    for name, m in (("m=1.75", 1.75), ("m=1.75+ulp", 1.75 + 2.0 ** -7)):
        x = normal().clamp(-0.05, 0.05)
        x[K // 3] = -m * 2.0 ** -3
        add(name, x)
    x = normal() * 1e-3
    x[K - 1] = 0.37
    add("large last", x)
    x = normal()
    x[0], x[K // 2], x[K - 1] = -0.0, -0.0, -0.0
    add("minus zero", x)
    x = normal()
    x[5 % K], x[K - 2] = math.nan, 0.11
    add("nan", x)
    x = normal()
    x[K - 1], x[1] = math.inf, -math.inf
    add("inf", x)
    return torch.stack(rows).to(BF), tuple(names)
