"""CPU restatement, in torch integer arithmetic, of the stochastic rounding of ``ssi_adamw_step_sr`` / ``ssi_round_bf16_sr``
(``include/ssi_hip.h``): Philox4x32-10, the indexing of its output by the global element index, and the fp32 -> bf16 rounding on the bit
pattern.  Exact: every quantity is an integer below 2**63 held in int64, so the GPU tests compare bit for bit."""
import math

import torch

M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
TENSOR_PARAM, TENSOR_EXP_AVG, TENSOR_EXP_AVG_SQ = 0, 1, 2


def _mulhilo(a: int, b: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(high, low) 32-bit words of a * b for a 32-bit constant and 32-bit values in int64, without leaving 63 bits: b in 16-bit halves."""
    x, y = a * (b >> 16), a * (b & 0xFFFF)          # a * b = x * 2**16 + y, both below 2**48
    return (x + (y >> 16)) >> 16, (((x & 0xFFFF) << 16) + y) & M32


def philox4x32_10(counter, key) -> list[torch.Tensor]:
    """Philox4x32 with 10 rounds.  ``counter``: four, ``key``: two 32-bit words (ints or int64 tensors of one shape); the four output words."""
    c = [torch.as_tensor(w, dtype=torch.int64) for w in counter]
    c = list(torch.broadcast_tensors(*c))
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        hi0, lo0 = _mulhilo(PHILOX_M0, c[0])
        hi1, lo1 = _mulhilo(PHILOX_M1, c[2])
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c


def random_bits(n: int, seed: int, step: int, tensor: int, elem_offset: int = 0) -> torch.Tensor:
    """The 16 random bits of elements ``elem_offset .. elem_offset + n`` (global indices) of tensor ``tensor`` at ``step``: int64 in [0, 65536)."""
    assert 0 <= step < 2 ** 32 and elem_offset >= 0
    e = elem_offset + torch.arange(n, dtype=torch.int64)
    j0 = elem_offset >> 3
    jv = j0 + torch.arange(((elem_offset + n + 7) >> 3) - j0, dtype=torch.int64)       # one generator call per 8-element vector
    w = torch.stack(philox4x32_10((jv & M32, jv >> 32, step, tensor), (seed & M32, (seed >> 32) & M32)), dim=1)   # [vectors, 4]
    k = e & 7
    return (w[(e >> 3) - j0, k >> 1] >> (16 * (k & 1))) & 0xFFFF


def f32_bits(x: torch.Tensor) -> torch.Tensor:
    assert x.dtype == torch.float32
    return x.contiguous().view(torch.int32).to(torch.int64) & M32


def bf16_bits(x: torch.Tensor) -> torch.Tensor:
    assert x.dtype == torch.bfloat16
    return x.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def bf16_from_bits(b: torch.Tensor) -> torch.Tensor:
    b = b & 0xFFFF
    return torch.where(b >= 0x8000, b - 0x10000, b).to(torch.int16).view(torch.bfloat16)


def same_bf16(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit-equal, +0 and -0 apart; a NaN equals any NaN (which NaN a round-to-nearest conversion returns is the converter's own business:
    torch's on the CPU and the GPU's instruction differ)."""
    a, b = a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)
    return a.shape == b.shape and bool(((bf16_bits(a) == bf16_bits(b)) | (a.isnan() & b.isnan())).all())


def sr_bf16(x: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """fp32 ``x`` to bf16 with the 16 random bits ``r`` (int64, broadcast against x): inf / NaN by round-to-nearest, otherwise add below the
    bf16 mantissa and truncate, unless that would carry a finite value into inf."""
    u = f32_bits(x)
    r = torch.as_tensor(r, dtype=torch.int64)
    t = (u + r) & M32
    special = (u & 0x7F800000) == 0x7F800000
    carried = (t & 0x7F800000) == 0x7F800000
    bits = torch.where(carried, u, t) >> 16
    return bf16_from_bits(torch.where(special, bf16_bits(x.to(torch.bfloat16)), bits))


def round_bf16_sr(x: torch.Tensor, *, seed: int, step: int, tensor: int, elem_offset: int = 0) -> torch.Tensor:
    return sr_bf16(x, random_bits(x.numel(), seed, step, tensor, elem_offset).reshape(x.shape))


def adamw_coefficients(lr, beta1, beta2, eps, weight_decay, step) -> dict[str, torch.Tensor]:
    """The kernel's fp32 coefficients: each computed in double from the double hyper-parameters, then rounded once (ssi_adamw_step)."""
    f = lambda d: torch.tensor(d, dtype=torch.float64).to(torch.float32)   # noqa: E731
    return dict(decay=f(1.0 - lr * weight_decay), w1=f(1.0 - beta1), beta2=f(beta2), w2=f(1.0 - beta2), eps=f(eps),
                step_size=f(lr / (1.0 - beta1 ** step)), inv_bc2_sqrt=f(1.0 / math.sqrt(1.0 - beta2 ** step)))


def adamw_f32(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step, dtype=torch.float32):
    """The pre-rounding values (p, m, v) of one AdamW step from bf16 (or wider) state, in ``dtype`` arithmetic with the kernel's fp32
    coefficients and its order of operations (fp32: without the fused multiply-adds a compiler may form; fp64: the yardstick)."""
    c = {k: t.to(dtype) for k, t in adamw_coefficients(lr, beta1, beta2, eps, weight_decay, step).items()}
    p, g, m, v = (t.to(dtype) for t in (p, g, m, v))
    pf = p * c["decay"]
    mf = m + c["w1"] * (g - m)
    vf = c["beta2"] * v + c["w2"] * g * g
    pf = pf - c["step_size"] * mf / (vf.sqrt() * c["inv_bc2_sqrt"] + c["eps"])
    return pf, mf, vf


def adamw_step_ref(p, g, m, v, *, seed=None, elem_offset=0, **hyper):
    """One bf16 AdamW step on the CPU: fp32 arithmetic, the three stores rounded to nearest (``seed`` None) or stochastically."""
    pf, mf, vf = adamw_f32(p, g, m, v, **hyper)
    if seed is None:
        return pf.to(torch.bfloat16), mf.to(torch.bfloat16), vf.to(torch.bfloat16)
    return tuple(round_bf16_sr(x, seed=seed, step=hyper["step"], tensor=t, elem_offset=elem_offset)
                 for t, x in ((TENSOR_PARAM, pf), (TENSOR_EXP_AVG, mf), (TENSOR_EXP_AVG_SQ, vf)))
