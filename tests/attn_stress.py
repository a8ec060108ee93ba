"""Inputs that move the softmax, two CPU references and a per-row checker for the attention parity tests (test_attn_stress_ref.py on the
CPU, test_attn_stress_gpu.py and two tests of test_kernels_gpu.py on the GPU).  Nothing here calls a kernel of this library.

A ROW is one (token, head) vector of head_dim: a query head for out and dq, a kv head for dk and dv (whose value already holds the sum over the
query heads of its group).  ``row_check`` bounds every row's distance from an fp64 reference by a multiple of what a restatement of the
kernels' documented rounding points (fp32 on the CPU) is away from it — see ``row_check`` for the formula and where the margin comes from.
head_dim is the keyword ``hd`` of every function that depends on it (default ``HD`` = 64, the MFMA kernels' only one); ``GEOMETRIES`` lists the
other head sizes and head ratios, which the generic kernels serve (test_attn_generic_geometry_gpu.py)."""
import functools
import math
from typing import NamedTuple, Optional

import torch

HD = 64
CASES = ("gauss", "ramp8", "ramp5", "fall", "sink", "sharp")
SHAPES = ((2, 512, 4, 1), (2, 256, 8, 2))                     # (B, S, H, KV)
DOC_ROWS = ((100, 37, 119, 256), (1, 63, 64, 384))
DOC_CASES = (("ramp8", DOC_ROWS), ("fall", DOC_ROWS), ("sink", ((512,), (512,))))   # all at SHAPES[0]
# The head geometries off the MFMA path (the generic kernels): (hd, (B, S, H, KV), documents per row or None, cases).  ``sink`` is left out
# wherever the rows are short: with at most 130 keys its two heavy keys take most of every later row, dq comes out as a small difference of
# large terms, and the bf16 checker would be blind on 8.5 - 18 % of the dq rows (test_attn_stress_ref.py measures it), over BLIND_CAP.  At
# (2, 192, 6, 2) it is 5.8 %, under the cap, and stays.
GEO_3B = (2, 192, 6, 2)                                       # head_dim 128, three query heads per kv head: Llama-3.2-3B's
GEO_DOC_ROWS = ((100, 37, 55), (1, 63, 64, 64))
NO_SINK = tuple(c for c in CASES if c != "sink")
GEOMETRIES = ((128, GEO_3B, None, CASES),
              (128, GEO_3B, GEO_DOC_ROWS, ("ramp8", "fall")),
              (128, (1, 64, 2, 2), None, NO_SINK),
              (16, (2, 130, 3, 1), None, NO_SINK),
              (32, (1, 65, 8, 1), None, NO_SINK),
              (64, (1, 63, 3, 1), None, ("gauss",)),
              (64, (2, 128, 6, 2), None, NO_SINK))
GEO_CONFIGS = [(hd, sh, rows, c) for hd, sh, rows, cases in GEOMETRIES for c in cases]
GEO_IDS = [f"hd{hd}-{c}-{sh[0]}x{sh[1]}-{sh[2]}h{sh[3]}kv" + ("-docs" if rows else "") for hd, sh, rows, c in GEO_CONFIGS]
SEED = 1
MARGIN = 8.0          # err_row <= MARGIN * E_row: twice what a second legitimate restatement needs (3.5 on dq), rounded up
BLIND_CAP = 0.06      # share of rows whose tolerance is so wide that a wrong value would pass (the reference alone: at most 4.7 %, dq in sink; over GEOMETRIES 5.8 %, dq in sink at head_dim 128)
EPS_BF16 = 2.0 ** -8  # half a bf16 step, relative
EPS_F32 = 1e-5        # the fp32 forms: E_row floored at 1e-5 of the row
BLOCKS = ("dq", "dk", "dv")


def _bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


def _unit(hd=HD):
    u = torch.zeros(hd, dtype=torch.float64)
    u[0::2] = 1.0 / math.sqrt(hd / 2.0)
    return u


@functools.lru_cache(maxsize=None)
def make_inputs(case: str, B: int, S: int, H: int, KV: int, seed: int = SEED, hd: int = HD):
    """bf16 ``qkv [B*S, (H+2KV)*hd]`` and ``dout [B*S, H*hd]`` (treat both as read-only: they are cached).  The aligned cases take the
    component along ``u`` (1/sqrt(hd/2) on the even components of a head) out of every q and k head and add ``sqrt(hd) u`` (``8u`` at head_dim
    64) to every q head: a key carrying ``c * u`` then adds ``c`` to the scaled score of every query, at every head_dim."""
    assert case in CASES
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * S, (H + 2 * KV) * hd, generator=g, dtype=torch.float64)
    dout = torch.randn(B * S, H * hd, generator=g, dtype=torch.float64)
    q = x[:, : H * hd].view(B, S, H, hd)
    k = x[:, H * hd:(H + KV) * hd].view(B, S, KV, hd)
    u = _unit(hd)
    if case == "sharp":
        q *= 1.5
        k *= 1.5
    elif case != "gauss":
        q -= (q @ u)[..., None] * u
        k -= (k @ u)[..., None] * u
        q += math.sqrt(hd) * u
        pos = torch.arange(S, dtype=torch.float64)[None, :, None, None]
        if case in ("ramp8", "ramp5", "fall"):
            slope = {"ramp8": 8.0, "ramp5": 5.0, "fall": -1.0}[case]
            k += (slope * pos / 64.0) * u
        else:  # sink
            k[:, 0] += 4.0 * u
            k[:, S // 2 + 7] += 6.0 * u
    return x.to(torch.bfloat16), dout.to(torch.bfloat16)


def doc_arrays(rows, S):
    """doc_start / doc_end / document-relative positions (int32 [B*S]) from per-row document lengths."""
    ds, de, pos = [], [], []
    for lens in rows:
        assert sum(lens) == S
        start = 0
        for n in lens:
            ds += [start] * n
            de += [start + n] * n
            pos += list(range(n))
            start += n
    return tuple(torch.tensor(t, dtype=torch.int32) for t in (ds, de, pos))


def dense_mask(B, S, rows=None):
    """[B, S(query), S(key)] bool, written out: key <= query, and — packed rows — key and query in the same document."""
    m = torch.ones(S, S, dtype=torch.bool).tril()[None].repeat(B, 1, 1)
    if rows is not None:
        ds, de, _ = doc_arrays(rows, S)
        ds = ds.view(B, S)
        key = torch.arange(S)[None, None, :]
        m &= key >= ds[:, :, None]
    return m


def _heads(x, B, S, H, KV, hd=HD):
    q = x[:, : H * hd].view(B, S, H, hd).transpose(1, 2)
    k = x[:, H * hd:(H + KV) * hd].view(B, S, KV, hd).transpose(1, 2)
    v = x[:, (H + KV) * hd:].view(B, S, KV, hd).transpose(1, 2)
    return q, k, v


def _rows_of(t, B, S):            # [B, heads, S, 64] -> [B*S, heads*64]
    return t.transpose(1, 2).reshape(B * S, -1)


def exact_of(qkv, dout, B, S, H, KV, rows=None, *, hd=HD):
    """fp64 masked softmax attention and its autograd on the bf16 inputs: ``out [B*S, H*hd]``, ``lse [B*H*S]`` (layout [B, H, S], natural log),
    ``dqkv``; ``dq_cond [B*S, H]``: sqrt(sum_d (dO_d O_d)^2) * |sum_k P_qk K_k| / sqrt(hd), what one relative rounding of the stored O moves dq
    by through delta; ``lse_tol``: 8 x the largest deviation of a plain fp32 logsumexp of the same scores from the fp64 one, at least 2e-5."""
    root = math.sqrt(hd)
    mask = dense_mask(B, S, rows)[:, None]
    x = qkv.double().requires_grad_(True)
    q, k, v = _heads(x, B, S, H, KV, hd)
    rep = H // KV
    kx, vx = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
    sc = (q @ kx.transpose(-1, -2) / root).masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(sc, dim=-1)
    P = torch.exp(sc - lse[..., None])
    out = P @ vx
    dO = dout.double().view(B, S, H, hd).transpose(1, 2)
    out.backward(dO)
    with torch.no_grad():
        cond = (dO * out).pow(2).sum(-1).sqrt() * (P @ kx).norm(dim=-1) / root     # [B, H, S]
        q32, k32, _ = _heads(qkv.float(), B, S, H, KV, hd)
        sc32 = ((q32 @ k32.repeat_interleave(rep, dim=1).transpose(-1, -2)) * (1.0 / root)).masked_fill(~mask, float("-inf"))
        dev = float((torch.logsumexp(sc32, dim=-1).double() - lse).abs().max())
    return {"out": _rows_of(out.detach(), B, S), "lse": lse.detach().reshape(-1), "dqkv": x.grad, "dq_cond": cond.transpose(1, 2).reshape(B * S, H),
            "lse_tol": max(8.0 * dev, 2e-5)}


@functools.lru_cache(maxsize=None)
def exact(case, B, S, H, KV, rows=None, seed=SEED, hd=HD):
    """``exact_of`` the inputs of a case, computed once per (case, shape, documents, seed, head_dim)."""
    return exact_of(*make_inputs(case, B, S, H, KV, seed, hd), B, S, H, KV, rows, hd=hd)


def restate_of(qkv, dout, B, S, H, KV, rows=None, *, stale=None, mask=None, skip_dk_head=None, hd=HD):
    """fp32 with the kernels' documented rounding points and no others: P rounded to bf16 as the operand of P V and of P^T dO; O stored in bf16;
    delta = rowsum(dO * stored O); dS = P (dP - delta) rounded to bf16 as the operand of dS K and dS^T Q; gradients rounded to bf16 on store
    (``dqkv``; ``dqkv_f32`` is the same before that last rounding, for the forms that rotate first).

    ``stale``: the SECOND restatement — P rounded un-normalised under a reference maximum ``stale`` below the true one (probabilities up to
    e^stale), O divided by l afterwards, delta from that O.  ``mask`` / ``skip_dk_head`` build deliberately wrong results for the checker's
    self-test: another [B, S, S] mask; one query head (index within its group) left out of dk for the last kv head."""
    scale = 1.0 / math.sqrt(hd)
    mask = (dense_mask(B, S, rows) if mask is None else mask)[:, None]
    q, k, v = _heads(qkv.float(), B, S, H, KV, hd)
    rep = H // KV
    kx, vx = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
    sc = ((q @ kx.transpose(-1, -2)) * scale).masked_fill(~mask, float("-inf"))
    m = sc.amax(dim=-1, keepdim=True)
    if stale is None:
        p = torch.exp(sc - m)
        l = p.sum(-1, keepdim=True)
        P = p / l
        Pb = _bf(P)
    else:
        m = m - stale
        p = torch.exp(sc - m)
        l = p.sum(-1, keepdim=True)
        P = p / l
        Pb = _bf(p) / l
    lse = (m + torch.log(l)).squeeze(-1)
    Ob = _bf(Pb @ vx)
    dO = dout.float().view(B, S, H, hd).transpose(1, 2)
    delta = (dO * Ob).sum(-1, keepdim=True)
    dSb = _bf(P * (dO @ vx.transpose(-1, -2) - delta))
    dq = (dSb @ kx) * scale
    dk_h = ((dSb.transpose(-1, -2) @ q) * scale).view(B, KV, rep, S, hd)
    if skip_dk_head is not None:
        dk_h = dk_h.clone()
        dk_h[:, KV - 1, skip_dk_head] = 0
    dk = dk_h.sum(2)
    dv = (Pb.transpose(-1, -2) @ dO).view(B, KV, rep, S, hd).sum(2)
    d32 = torch.cat([_rows_of(dq, B, S), _rows_of(dk, B, S), _rows_of(dv, B, S)], dim=1)
    return {"out": _rows_of(Ob, B, S).double(), "lse": lse.reshape(-1).double(), "dqkv": _bf(d32).double(), "dqkv_f32": d32}


def restate(case, B, S, H, KV, rows=None, seed=SEED, hd=HD, **kw):
    return restate_of(*make_inputs(case, B, S, H, KV, seed, hd), B, S, H, KV, rows, hd=hd, **kw)


@functools.lru_cache(maxsize=None)
def restated(case, B, S, H, KV, rows=None, seed=SEED, hd=HD):
    return restate(case, B, S, H, KV, rows, seed, hd)


@functools.lru_cache(maxsize=None)
def restated_second(case, B, S, H, KV, rows=None, seed=SEED, hd=HD):
    return restate(case, B, S, H, KV, rows, seed, hd, stale=3.7)


def rope_transpose(dqkv, table, pos, H, KV, hd=HD):
    """dq / dk rows through the transpose (= inverse: the table is a rotation) of the adjacent-pair rotation at ``pos`` (int [B*S]), in fp64;
    dv as it is.  ``table``: [position][pair][cos, sin]."""
    d = dqkv.double().clone()
    cs = table.double()[pos.long()]                      # [B*S, hd / 2, 2]
    c, s = cs[:, None, :, 0], cs[:, None, :, 1]
    g = d[:, : (H + KV) * hd].reshape(d.shape[0], H + KV, hd // 2, 2)
    g0, g1 = g[..., 0], g[..., 1]
    d[:, : (H + KV) * hd] = torch.stack([g0 * c + g1 * s, g1 * c - g0 * s], dim=-1).reshape(d.shape[0], -1)
    return d


def rope_refs(ex, rs, table, pos, H, KV, hd=HD):
    """(exact dqkv, restated dqkv) of a backward with the RoPE backward fused in: both rotated in fp64, the restated one from its fp32 values
    and rounded to bf16 after the rotation, as the epilogues do."""
    return rope_transpose(ex["dqkv"], table, pos, H, KV, hd), _bf(rope_transpose(rs["dqkv_f32"], table, pos, H, KV, hd).float()).double()


def block_cols(block, H, KV, hd=HD):
    return {"out": (0, H * hd), "dq": (0, H * hd), "dk": (H * hd, (H + KV) * hd), "dv": ((H + KV) * hd, (H + 2 * KV) * hd)}[block]


class RowCheck(NamedTuple):
    ok: bool
    worst: float            # largest err_row / E_row
    where: tuple            # (batch row, position, head) of it
    blind: float            # share of rows with 16 E_row > max(|exact_row|, 0.02 rms_row)
    message: str
    ratio: torch.Tensor     # [B, S, heads]
    blind_rows: torch.Tensor


def row_check(got, exact_, restated_, block, B, S, *, margin=MARGIN, dq_cond=None, eps=EPS_BF16, exempt=None, name="", hd=HD) -> RowCheck:
    """Every row of ``got`` ([B*S, heads*hd], any float dtype) within ``margin * E_row`` of ``exact_`` (Euclidean norm over the hd), with

        E_row = max(|restated_row - exact_row|, eps * max(|exact_row|, 0.02 * rms_row)),

    ``rms_row`` the rms of |exact_row| over the S rows of that batch row and head, and for dq also E_row >= eps * dq_cond (``exact``): the
    rounding of the stored O enters dq through the scalar delta, and one realisation of that scalar's error does not predict another.
    ``exempt``: bool [B, S, heads] of rows left out (the caller says why)."""
    assert block in ("out",) + BLOCKS and got.shape == exact_.shape == restated_.shape and got.shape[0] == B * S
    nh = got.shape[1] // hd
    g, e, r = (t.detach().cpu().double().view(B, S, nh, hd) for t in (got, exact_, restated_))
    en = e.norm(dim=-1)
    base = torch.maximum(en, 0.02 * en.pow(2).mean(dim=1, keepdim=True).sqrt())
    E = torch.maximum((r - e).norm(dim=-1), eps * base)
    if block == "dq":
        assert dq_cond is not None
        E = torch.maximum(E, eps * dq_cond.view(B, S, nh))
    ratio = (g - e).norm(dim=-1) / E
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    blind_rows = 16.0 * E > base
    if exempt is not None:
        ratio = torch.where(exempt, torch.zeros_like(ratio), ratio)
    worst = float(ratio.max())
    b, s, h = (int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape))
    blind = float(blind_rows.double().mean())
    msg = (f"{name} {block}: worst err / E_row {worst:.3g} at (batch row {b}, position {s}, head {h}) against margin {margin:g}; "
           f"{int((ratio > margin).sum())} of {ratio.numel()} rows over; blind share {100 * blind:.2f} %")
    return RowCheck(worst <= margin, worst, (b, s, h), blind, msg, ratio, blind_rows)


def check_all(got_out, got_lse, got_dqkv, ex, rs, B, S, H, KV, *, name="", margin=MARGIN, eps=EPS_BF16, ref_dqkv=None, record=None, hd=HD):
    """All the assertions of one run of a kernel form: finite values, ``row_check`` on out / dq / dk / dv, the lse tolerance.  Any of the three
    results may be None.  ``ref_dqkv``: (exact, restated) gradients where they are not the plain ones (rope_refs).  ``record``: dict that
    collects the worst err / E_row per block (max over calls)."""
    def note(block, res):
        print(res.message)
        if record is not None:
            record[block] = max(record.get(block, 0.0), res.worst)
        assert res.ok, res.message

    if got_out is not None:
        assert torch.isfinite(got_out).all(), f"{name}: non-finite out"
        note("out", row_check(got_out, ex["out"], rs["out"], "out", B, S, margin=margin, eps=eps, name=name, hd=hd))
    if got_lse is not None:
        lse = got_lse.detach().cpu().double()
        assert torch.isfinite(lse).all(), f"{name}: non-finite lse"
        err = float((lse - ex["lse"]).abs().max())
        print(f"{name} lse: max-abs error {err:.3g} against {ex['lse_tol']:.3g} (|lse| up to {float(ex['lse'].abs().max()):.3g})")
        if record is not None:
            record["lse"] = max(record.get("lse", 0.0), err / ex["lse_tol"])
        assert err <= ex["lse_tol"], f"{name}: lse max-abs error {err:.3g} > {ex['lse_tol']:.3g}"
    if got_dqkv is not None:
        assert torch.isfinite(got_dqkv).all(), f"{name}: non-finite gradients"
        e_d, r_d = ref_dqkv if ref_dqkv is not None else (ex["dqkv"], rs["dqkv"])
        for block in BLOCKS:
            lo, hi = block_cols(block, H, KV, hd)
            note(block, row_check(got_dqkv[:, lo:hi], e_d[:, lo:hi], r_d[:, lo:hi], block, B, S, margin=margin, eps=eps,
                                  dq_cond=ex["dq_cond"] if block == "dq" else None, name=name, hd=hd))


def f32_restated(ex):
    """The "restated" reference of the fp32 forms: the exact one rounded to fp32."""
    return {k: v.float().double() for k, v in ex.items() if k in ("out", "lse", "dqkv")}
