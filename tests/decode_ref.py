"""Inputs, two CPU references and a per-element checker for ``ssi_attn_decode`` (test_decode_ref.py on the CPU, test_attn_decode_gpu.py on
the GPU), in the manner of ``attn_stress.py`` and ``ce_parity.py``.  Nothing here calls a kernel of this library.

A PROBLEM is one launch: ``qkv [rows, ld]``, the two caches ``[n_slots, cap, n_kv * head_dim]``, ``slot`` and ``kv_len`` per row.
``exact`` is fp64 softmax attention on the STORED inputs; ``restate`` says the kernel's rounding points again in fp32 (q scaled once by
``(float)(log2(e) / sqrt(head_dim))``, fp32 scores, max, ``exp2``, fp32 sum and fp32 P.V, one division; P never rounded to bf16) without its
chunking.  The bound per element of row r, head h:

    |out - ref| <= EPS * |ref| + C * max_{j < kv_len, d} |V[slot, j, h / g, d]|          EPS = 2^-8 for bf16 stores, 0 for fp32

``C`` covers the fp32 score, exp and accumulation error: 8 x the largest distance of the (unrounded) fp32 restatement from fp64, in units of
that row's largest |v|, over ``standard_problems`` with ``SEED`` — the margin of the attention stress test.  ``measure_c`` computes it;
``C`` / ``C_LSE`` below are the recorded results, and test_decode_ref.py holds them to the measurement."""
import functools
import math
from typing import NamedTuple, Optional

import torch

CASES = ("gauss", "sink", "newest", "spread")
SEED = 1
MARGIN = 8.0
EPS_BF16 = 2.0 ** -8
# 8 x the measured maxima (measure_c over standard_problems of both dtypes at SEED: 2.22e-6 of the largest |v|, and 6.96e-6 on the lse)
C = 1.8e-5
C_LSE = 5.6e-5


class Geometry(NamedTuple):
    n_heads: int
    n_kv: int
    head_dim: int


ISSUE_GEOMETRIES = (Geometry(8, 2, 16), Geometry(4, 1, 64), Geometry(32, 8, 64), Geometry(2, 2, 64))
# every instantiation of the kernel: g = 2 and 8 have forms of their own, g = 3 and 5 run the next wider one with idle head registers;
# head_dim 24 leaves lanes of a key group idle, head_dim 128 is the widest
MORE_GEOMETRIES = (Geometry(4, 2, 16), Geometry(8, 1, 16), Geometry(6, 2, 8), Geometry(5, 1, 24), Geometry(2, 1, 128))


def chunk_edges(head_dim: int, dtype: torch.dtype) -> tuple[int, int, int]:
    """(keys per load, keys per chunk, keys per round of the four waves) of the kernel for this head width and storage type: a key lies on
    ``head_dim * sizeof / 16`` lanes rounded up to a power of two, a wave holds 64 keys' lanes per load, a chunk is two loads."""
    lanes = head_dim * (2 if dtype == torch.bfloat16 else 4) // 16
    lpk = 1
    while lpk < lanes:
        lpk *= 2
    kpw = 64 // lpk
    return kpw, 2 * kpw, 8 * kpw


def edge_lengths(head_dim: int, dtype: torch.dtype, cap: int) -> list[int]:
    """kv_len at 1 and 2 and one below, at and one above every edge of the kernel (load, chunk, round, two rounds), within ``cap``."""
    kpw, chunk, rnd = chunk_edges(head_dim, dtype)
    out = {1, 2}
    for e in (kpw, chunk, rnd, 2 * rnd):
        out |= {e - 1, e, e + 1}
    return sorted(n for n in out if 1 <= n <= cap)


class Problem(NamedTuple):
    geom: Geometry
    dtype: torch.dtype
    qkv: torch.Tensor        # [rows, ld]
    k_cache: torch.Tensor    # [n_slots, cap, n_kv * head_dim]
    v_cache: torch.Tensor
    slot: torch.Tensor       # int32 [rows]
    kv_len: torch.Tensor     # int32 [rows]
    case: str = "gauss"

    @property
    def rows(self) -> int:
        return self.qkv.shape[0]

    @property
    def cap(self) -> int:
        return self.k_cache.shape[1]


def _unit(hd: int) -> torch.Tensor:
    u = torch.zeros(hd, dtype=torch.float32)
    u[0::2] = 1.0 / math.sqrt(hd / 2)
    return u


def make_problem(geom: Geometry, dtype: torch.dtype, kv_lens, case: str, cap: int, seed: int = SEED, poison: bool = True,
                 dead_rows=(), spare_slots: int = 2, ld_extra: int = 8) -> Problem:
    """One launch.  ``kv_lens``: the length per row (a length above ``cap`` stays in ``kv_len`` and is clamped by whoever reads it).  The
    slots are a permutation that is not the identity, with ``spare_slots`` slots no row names.  ``dead_rows``: rows whose slot is -1.
    Every q head carries ``sqrt(head_dim) * u`` and no key has a component along ``u`` but those the case puts there, so a key carrying
    ``c * u`` adds ``c`` to its scaled score: ``sink`` 10 on key 0, ``newest`` 16 on the LAST live key (a near-one-hot there: what an
    off-by-one in kv_len loses), ``spread`` a uniform draw from [-30, 30] per key.
    ``poison``: every cache position at or beyond a row's length, and every slot no row names, holds NaN."""
    assert case in CASES
    H, KV, hd = geom
    rows, n_slots = len(kv_lens), len(kv_lens) + spare_slots
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(n_slots, generator=g)
    if rows > 1 and bool((perm[:rows] == torch.arange(rows)).all()):
        perm = perm.roll(1)
    slot = perm[:rows].to(torch.int32)
    for r in dead_rows:
        slot[r] = -1
    u = _unit(hd)
    ld = (H + 2 * KV) * hd + ld_extra
    qkv = torch.randn(rows, ld, generator=g)
    q = qkv[:, : H * hd].view(rows, H, hd)
    q -= (q @ u)[..., None] * u
    q += math.sqrt(hd) * u
    kc = torch.randn(n_slots, cap, KV, hd, generator=g)
    vc = torch.randn(n_slots, cap, KV, hd, generator=g)
    kc -= (kc @ u)[..., None] * u
    lens = torch.tensor([min(int(n), cap) for n in kv_lens])
    live = torch.zeros(n_slots, cap, dtype=torch.bool)
    c = torch.zeros(n_slots, cap)
    for r in range(rows):
        s, n = int(slot[r]), int(lens[r])
        if s < 0 or n <= 0:
            continue
        live[s, :n] = True
        if case == "sink":
            c[s, 0] = 10.0
        elif case == "newest":
            c[s, n - 1] = 16.0
        elif case == "spread":
            c[s, :n] = torch.rand(n, generator=g) * 60.0 - 30.0
    kc += c[:, :, None, None] * u
    if poison:
        kc[~live] = float("nan")
        vc[~live] = float("nan")
    return Problem(geom, dtype, qkv.to(dtype), kc.view(n_slots, cap, KV * hd).to(dtype), vc.view(n_slots, cap, KV * hd).to(dtype), slot,
                   torch.tensor([int(n) for n in kv_lens], dtype=torch.int32), case)


class Result(NamedTuple):
    out: torch.Tensor        # [rows, n_heads * head_dim]
    lse: torch.Tensor        # [rows, n_heads]
    vmax: torch.Tensor       # [rows, n_heads]: the largest |v| among the row's live keys of the head's kv head
    dead: torch.Tensor       # bool [rows]: slot < 0, slot >= n_slots or kv_len <= 0 — zeros and -inf are expected


def _attend(p: Problem, ft: torch.dtype, kv_delta: int = 0, slot_shift: int = 0, head_shift: int = 0, scaled: bool = True) -> Result:
    """Softmax attention per row in ``ft`` (float64: the exact reference; float32: the restatement, with the kernel's base-2 scores).
    The other arguments are the deliberate MISTAKES of the self-test: ``kv_delta`` is added to every length, ``slot_shift`` makes row r read
    the slot of row r + slot_shift, ``head_shift`` makes query head h read kv head h / g + head_shift, ``scaled=False`` drops 1/sqrt(head_dim)."""
    H, KV, hd = p.geom
    g, rows, n_slots, cap = H // KV, p.rows, p.k_cache.shape[0], p.cap
    out = torch.zeros(rows, H * hd, dtype=ft)
    lse = torch.full((rows, H), -math.inf, dtype=ft)
    vmax = torch.zeros(rows, H, dtype=torch.float64)
    dead = torch.zeros(rows, dtype=torch.bool)
    qscale32 = torch.tensor(1.4426950408889634 / math.sqrt(hd) if scaled else 1.4426950408889634, dtype=torch.float32)
    for r in range(rows):
        s, n = int(p.slot[r]), min(int(p.kv_len[r]), cap)
        if s < 0 or s >= n_slots or n <= 0:
            dead[r] = True
            continue
        n = max(min(n + kv_delta, cap), 0)
        s = int(p.slot[(r + slot_shift) % rows]) if slot_shift else s
        K = p.k_cache[s, :n].to(ft).view(n, KV, hd).roll(-head_shift, 1)
        V = p.v_cache[s, :n].to(ft).view(n, KV, hd).roll(-head_shift, 1)
        q = p.qkv[r, : H * hd].to(ft).view(KV, g, hd)
        if ft == torch.float64:
            sc = torch.einsum("kgd,nkd->kgn", q, K) * (1.0 / math.sqrt(hd) if scaled else 1.0)
            l_ = torch.logsumexp(sc, dim=-1)
            o = torch.einsum("kgn,nkd->kgd", torch.exp(sc - l_[..., None]), V)
        else:
            sc = torch.einsum("kgd,nkd->kgn", q * qscale32, K)
            m = sc.max(dim=-1).values
            P = torch.exp2(sc - m[..., None])
            L = P.sum(dim=-1)
            o = torch.einsum("kgn,nkd->kgd", P, V) / L[..., None]
            l_ = (m + torch.log2(L)) * torch.tensor(0.69314718055994531, dtype=torch.float32)
        out[r] = o.reshape(-1)
        lse[r] = l_.reshape(-1)
        if n:
            vmax[r] = V.abs().amax(dim=(0, 2)).double().repeat_interleave(g)
    return Result(out, lse, vmax, dead)


def exact(p: Problem, **mistake) -> Result:
    return _attend(p, torch.float64, **mistake)


def restate(p: Problem) -> Result:
    """The kernel's rounding points in fp32; ``out`` is NOT yet rounded to the storage type (``stored`` does that)."""
    return _attend(p, torch.float32)


def stored(out: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    return out.to(dtype).double()


def tolerance(p: Problem, ref: Result) -> torch.Tensor:
    """[rows, n_heads * head_dim]: the bound of the module docstring."""
    hd = p.geom.head_dim
    eps = EPS_BF16 if p.dtype == torch.bfloat16 else 0.0
    return eps * ref.out.abs() + C * ref.vmax.repeat_interleave(hd, dim=1)


def violations(got_out: torch.Tensor, got_lse: Optional[torch.Tensor], p: Problem, ref: Result) -> list[str]:
    """What is wrong with a result (``got_out``: [rows, n_heads * head_dim], any float type; ``got_lse``: [rows, n_heads] or None)."""
    H, KV, hd = p.geom
    bad = []
    got = got_out.detach().cpu().double().view(p.rows, H * hd)
    live = ~ref.dead
    if ref.dead.any():
        if not bool((got[ref.dead] == 0).all()):
            bad.append(f"rows without keys must be exact zeros: {int((got[ref.dead] != 0).sum())} elements are not")
        if got_lse is not None and not bool((got_lse.detach().cpu()[ref.dead] == -math.inf).all()):
            bad.append("rows without keys must have lse = -inf")
    if not bool(torch.isfinite(got[live]).all()):
        bad.append(f"{int((~torch.isfinite(got[live])).sum())} elements are not finite (poison was read)")
    err, tol = (got - ref.out).abs(), tolerance(p, ref)
    over = ~(err <= tol) & live[:, None]
    if over.any():
        r, c = [int(x) for x in over.nonzero()[0]]
        ratio = torch.where(live[:, None], err / tol, torch.zeros_like(err))
        ratio = torch.nan_to_num(ratio, nan=math.inf)
        bad.append(f"{int(over.sum())} elements over the bound, worst {float(ratio.max()):.3g} x; first at row {r} (kv_len {int(p.kv_len[r])}, "
                   f"slot {int(p.slot[r])}) head {c // hd} column {c % hd}: {float(got[r, c]):.6g} against {float(ref.out[r, c]):.6g} "
                   f"(tolerance {float(tol[r, c]):.3g})")
    if got_lse is not None:
        le = (got_lse.detach().cpu().double()[live] - ref.lse[live]).abs()
        if le.numel() and not bool((le <= C_LSE).all()):
            bad.append(f"lse off by {float(torch.nan_to_num(le, nan=math.inf).max()):.3g} (tolerance {C_LSE:.3g})")
    return bad


def measure_c(problems) -> tuple[float, float]:
    """(largest |restate - exact| / vmax over all elements, largest |lse| distance) over ``problems``, without the margin."""
    worst, worst_lse = 0.0, 0.0
    for p in problems:
        ref, re = exact(p), restate(p)
        live = ~ref.dead
        d = (re.out.double() - ref.out).abs() / ref.vmax.repeat_interleave(p.geom.head_dim, dim=1).clamp(min=1e-30)
        worst = max(worst, float(d[live].max()))
        worst_lse = max(worst_lse, float((re.lse.double() - ref.lse)[live].abs().max()))
    return worst, worst_lse


def ragged_lengths(rows: int, head_dim: int, dtype: torch.dtype, cap: int, seed: int = SEED) -> list[int]:
    """``rows`` lengths: every edge length first, then short draws (the CPU reference walks every row)."""
    edges = edge_lengths(head_dim, dtype, cap)
    g = torch.Generator().manual_seed(seed + 100)
    fill = [int(x) for x in torch.randint(1, 48, (max(rows - len(edges), 0),), generator=g)]
    return (edges + fill)[:rows]


@functools.lru_cache(maxsize=None)
def standard_problems(dtype: torch.dtype, seed: int = SEED, poison: bool = True) -> tuple[Problem, ...]:
    """The inputs C is measured on and the CPU self-test runs over: every case at two of the issue's geometries with the edge lengths in
    a cap of 300, and one long row (1000) beside a row of length 1."""
    out = []
    for geom in (Geometry(8, 2, 16), Geometry(4, 1, 64)):
        lens = edge_lengths(geom.head_dim, dtype, 299)          # (below the cap: a length off by +1 still finds a key)
        for case in CASES:
            out.append(make_problem(geom, dtype, lens, case, 300, seed, poison))
    for case in ("gauss", "spread"):
        out.append(make_problem(Geometry(8, 2, 16), dtype, [1000, 1, 7], case, 1003, seed, poison))
    return tuple(out)
