"""The FP8 K/V cache restated on the CPU (test_kv_fp8_ref.py checks this file against itself and against torch's own e4m3 cast; the GPU tests
test_kv_store_fp8_gpu.py, test_attn_decode_fp8_gpu.py and test_kv_fp8_model_gpu.py check the kernels against it).  Nothing here calls a kernel.

THE DEFINITION (include/ssi_hip.h, "FP8 K/V cache"), once more.  A cached LINE is the ``head_dim`` elements of one (position, kv head) of K (after
RoPE) or of V, in the model's dtype.  It is stored as ``head_dim`` e4m3fn codes (OCP: bias 7, no infinity, NaN = S.1111.111, largest finite 448) and
one biased exponent byte ``b``:

* ``a`` = the largest ``|x_i|`` over the line's finite elements.  ``a == 0`` or no finite element: ``b = 127``.  Otherwise ``a = m * 2^E`` with ``m``
  in [1, 2); ``e = E - 8`` if ``m <= 1.75`` else ``E - 7`` (the smallest ``e`` with ``a * 2^-e <= 448``); ``b = clamp(e, -127, 127) + 127``.  ``e``
  is read from the bits of ``a`` (an fp32 subnormal has ``E < -126``: ``b = 0``).
* ``code_i = RNE_e4m3(x_i * 2^-e)``, the scaling exact; a NaN or infinite element stores the NaN code 0x7f.
* the value of a code is ``float(code) * 2^(b - 127)``, exact in fp32.

``quantise`` takes the planted DEFECTS of the self-test by name: ``exp_plus_one``, ``threshold`` (1.75 itself on the wrong side), ``truncate`` (toward
zero instead of RNE), ``neighbour_head`` (the exponent of the next kv head); ``quantise_problem`` also ``k_exp_for_v``."""
import math
from typing import NamedTuple, Optional

import torch

import decode_ref as dr

NAN_CODE = 0x7F
POISON_EXP = 255
DEFECTS = ("exp_plus_one", "threshold", "truncate", "neighbour_head", "k_exp_for_v")


def e4m3_value_table() -> torch.Tensor:
    """float64 [256]: the value of every code (NaN at 0x7f and 0xff)."""
    out = torch.zeros(256, dtype=torch.float64)
    for c in range(256):
        sign = -1.0 if c & 0x80 else 1.0
        ex, man = (c >> 3) & 0xF, c & 7
        if ex == 15 and man == 7:
            v = math.nan
        elif ex == 0:
            v = man * 2.0 ** -9
        else:
            v = (8 + man) * 2.0 ** (ex - 7 - 3)
        out[c] = sign * v
    return out


def _pow2(n: torch.Tensor) -> torch.Tensor:
    """float64 2^n for integer n in [-1022, 1023], made from the bits: exact."""
    return ((n.long() + 1023) << 52).view(torch.float64)


def e4m3_encode(y: torch.Tensor, truncate: bool = False) -> torch.Tensor:
    """uint8 codes of float64 ``y`` by hand: round to nearest, ties to the even code; NaN and infinity: 0x7f.  Finite ``|y|`` must not exceed 448
    (the definition never relies on saturation)."""
    y = y.double()
    finite = torch.isfinite(y)
    mag = torch.where(finite, y.abs(), torch.zeros_like(y))
    assert float(mag.max()) <= 448.0 if mag.numel() else True
    rnd = torch.floor if truncate else torch.round                     # torch.round: half to even
    _, ex = torch.frexp(mag)                                            # mag = f * 2^ex, f in [0.5, 1)
    E = (ex - 1).clamp(min=-6)                                          # below the smallest normal 2^-6 the step stays 2^-9
    q = rnd(mag * _pow2(-(E - 3)))                                      # in units of 2^(E - 3): 0 .. 16, exact in float64
    up = q >= 16
    E, q = torch.where(up, E + 1, E), torch.where(up, torch.full_like(q, 8.0), q)
    normal = q >= 8
    code = torch.where(normal, ((E + 7) << 3) + (q.long() - 8), q.long())
    code = code | (torch.signbit(y).long() << 7)
    return torch.where(finite, code, torch.full_like(code, NAN_CODE)).to(torch.uint8)


def line_exponent(a: torch.Tensor, threshold_defect: bool = False) -> torch.Tensor:
    """int64 biased exponent byte from the BITS of fp32 ``a`` (>= 0, finite)."""
    bits = a.float().contiguous().view(torch.int32).long()
    field, man = bits >> 23, bits & 0x7FFFFF
    above = man >= 0x600000 if threshold_defect else man > 0x600000
    b = (field - 8 + above.long()).clamp(min=0)
    return torch.where(bits == 0, torch.full_like(b, 127), b)


def quantise(x: torch.Tensor, defect: Optional[str] = None) -> tuple[torch.Tensor, torch.Tensor]:
    """``x`` [..., n_kv, head_dim] in the model's dtype -> (codes uint8 [..., n_kv, head_dim], exponent bytes uint8 [..., n_kv])."""
    xf = x.float()
    finite = torch.isfinite(xf)
    a = torch.where(finite, xf.abs(), torch.zeros_like(xf)).amax(dim=-1)
    b = line_exponent(a, defect == "threshold")
    if defect == "exp_plus_one":
        b = torch.where(a > 0, b + 1, b)
    if defect == "neighbour_head":
        b = b.roll(-1, dims=-1)
    y = xf.double() * _pow2(127 - b)[..., None]                         # exact in float64
    if defect in ("threshold", "neighbour_head"):                       # (a defect that picks too small an exponent: saturate, as a conversion would)
        y = torch.where(torch.isfinite(y), y.clamp(-448.0, 448.0), y)
    return e4m3_encode(y, truncate=defect == "truncate"), b.to(torch.uint8)


def dequantise(codes: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """fp32 [..., n_kv, head_dim]: ``float(code) * 2^(b - 127)`` (exact)."""
    v = e4m3_value_table()[codes.long()]
    return (v * _pow2(b.long() - 127)[..., None]).float()


class QuantisedCache(NamedTuple):
    k_codes: torch.Tensor    # uint8 [n_slots, cap, n_kv * head_dim]
    v_codes: torch.Tensor
    k_exp: torch.Tensor      # uint8 [n_slots, cap, n_kv]
    v_exp: torch.Tensor

    def tensors(self, dev=None):
        return tuple(t if dev is None else t.to(dev) for t in self)


def quantise_cache(k: torch.Tensor, v: torch.Tensor, n_kv: int, live: Optional[torch.Tensor] = None, defect: Optional[str] = None):
    """Caches [n_slots, cap, n_kv * head_dim] in the model's dtype -> (QuantisedCache, dequantised k, dequantised v in that dtype).  ``live`` (bool
    [n_slots, cap]): every other position is POISONED — NaN code and exponent byte 255 in the fp8 cache, NaN in the dequantised one."""
    n_slots, cap, width = k.shape
    hd = width // n_kv
    q_defect = None if defect == "k_exp_for_v" else defect
    kc, ke = quantise(k.view(n_slots, cap, n_kv, hd), q_defect)
    vc, ve = quantise(v.view(n_slots, cap, n_kv, hd), q_defect)
    dk = dequantise(kc, ke)
    dv = dequantise(vc, ke if defect == "k_exp_for_v" else ve)
    if live is not None:
        kc[~live], vc[~live], ke[~live], ve[~live] = NAN_CODE, NAN_CODE, POISON_EXP, POISON_EXP
        dk[~live], dv[~live] = math.nan, math.nan
    q = QuantisedCache(kc.view(n_slots, cap, width).contiguous(), vc.view(n_slots, cap, width).contiguous(), ke.contiguous(), ve.contiguous())
    return q, dk.view(n_slots, cap, width).to(k.dtype), dv.view(n_slots, cap, width).to(v.dtype)


def live_positions(p: dr.Problem) -> torch.Tensor:
    """bool [n_slots, cap]: the cache positions some row of ``p`` reads."""
    n_slots, cap = p.k_cache.shape[:2]
    live = torch.zeros(n_slots, cap, dtype=torch.bool)
    for r in range(p.rows):
        s, n = int(p.slot[r]), min(int(p.kv_len[r]), cap)
        if 0 <= s < n_slots and n > 0:
            live[s, :n] = True
    return live


def quantise_problem(p: dr.Problem, defect: Optional[str] = None) -> tuple[QuantisedCache, dr.Problem]:
    """A ``decode_ref.Problem`` -> (its caches as codes and exponents, the same problem on the DEQUANTISED caches in the model's dtype).  Every
    position no row reads is poisoned in both."""
    q, dk, dv = quantise_cache(p.k_cache, p.v_cache, p.geom.n_kv, live_positions(p), defect)
    return q, p._replace(k_cache=dk, v_cache=dv)


def edge_lines(head_dim: int, dtype: torch.dtype, seed: int = 3) -> torch.Tensor:
    """[n, head_dim] lines in ``dtype`` at the edges of the definition; every line's description is in ``EDGE_NAMES`` at the same index.  The
    absmax sits in the LAST column of every other line that has one, so the maximum has to cross the lanes of a line."""
    g = torch.Generator().manual_seed(seed)
    ulp = 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -23          # of [1, 2)
    lines = []

    def line(absmax: float, specials=(), fill: float = 0.4, at_end: bool = False) -> None:
        x = (torch.rand(head_dim, generator=g).double() * 2 - 1) * fill * abs(absmax)
        sp = list(specials)
        if sp:
            x[1:1 + len(sp)] = torch.tensor(sp, dtype=torch.float64)
        x[head_dim - 1 if at_end else 0] = absmax
        lines.append(x)

    lines.append(torch.zeros(head_dim, dtype=torch.float64))                                     # 0: all zeros
    for k, m in enumerate((1.75, 1.75 - ulp, 1.75 + ulp)):                                       # 1-3: the 1.75 threshold and one ulp either side
        line(m * 2.0 ** (3 * k - 2), at_end=k == 1)
    for k in (0, -5, 9):                                                                         # 4-6: absmax = 448 * 2^k
        line(-448.0 * 2.0 ** k if k else 448.0, at_end=k == 9)
    # 7: scale 1 (absmax 256 -> e = 0): midpoints of both parities, among normals ...
    line(256.0, (17.0, 19.0, -17.0, -19.0, 1.0625, 1.1875, 208.0, 240.0, 0.017578125, 0.021484375), fill=0.0)
    # 8: ... and in the subnormals (step 2^-9): exact steps, midpoints, half the smallest one, just below and above it, -0 results
    s = 2.0 ** -9
    line(256.0, (s, 1.5 * s, 2.5 * s, 0.5 * s, 0.4921875 * s, 0.5078125 * s, 7.5 * s, -0.5 * s, -0.25 * s, 6.5 * s, 2.0 ** -30, -(2.0 ** -30)),
         fill=0.0, at_end=True)
    line(3.0, (math.nan, math.inf, -math.inf, 2.9, -1.0))                                       # 9: a NaN and infinities among finite elements
    lines.append(torch.full((head_dim,), math.nan, dtype=torch.float64))                        # 10: nothing finite
    line(2.0 ** 100 * 1.3, (2.0 ** 90, 2.0 ** 60, -1.0))                                        # 11: large
    line(2.0 ** -120 * 1.9, (2.0 ** -125, -(2.0 ** -122)), at_end=True)                         # 12: tiny, m > 1.75
    line(2.0 ** -131 if dtype == torch.bfloat16 else 2.0 ** -135, (2.0 ** -133 if dtype == torch.bfloat16 else 2.0 ** -137,), fill=0.0)   # 13: a subnormal absmax: b = 0
    line(1.0, (-1.0, 0.5, 0.99609375), fill=0.9)                                                # 14: m = 1 exactly, ties for the absmax
    return torch.stack(lines).to(dtype)


EDGE_NAMES = ("zeros", "m=1.75", "m=1.75-ulp", "m=1.75+ulp", "448", "-448*2^-5", "-448*2^9", "normal midpoints", "subnormal codes", "nan and inf",
              "all nan", "large", "tiny", "subnormal absmax", "m=1")
