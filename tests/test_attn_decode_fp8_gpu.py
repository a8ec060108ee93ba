"""The four fp8 decode-attention entries on the GPU.  THE CONTRACT: ``out``, ``lse`` and ``n_bad`` of an ``_fp8`` entry are BIT-EQUAL to the plain entry's
on a cache that holds the dequantised values in the model's dtype (kv_fp8_ref.py quantises on the CPU; the store kernel is test_kv_store_fp8_gpu.py's).

* slot form: every geometry of ``decode_ref`` (``ISSUE_GEOMETRIES`` and ``MORE_GEOMETRIES``: all G, idle lanes, head_dim 8 to 128), bf16 and fp32, the
  cases ``gauss``, ``sink``, ``newest``, ``spread`` over ``decode_ref.edge_lengths`` of the model dtype (the fp8 forms keep its lane layout), with a dead
  row and a slot beyond ``n_slots`` among them;
* split form: spans of one round and the library's default;
* beam forms: the pairings of prompt and generated lengths of test_attn_decode_beam_split_gpu.py (the seam inside a split, on its edge, one key either
  side), plain and split, with indices outside their caches;
* one direct check per dtype against ``decode_ref.exact`` on the dequantised problem under ``decode_ref.tolerance`` / ``C_LSE``, unchanged: no rounding
  point is new.

Every code and exponent byte a row must not read holds the NaN code and exponent byte 255 (NaN in the dequantised cache), K and V lines of a position
differ in exponent (V is scaled), and the workspace of a split launch is NaN."""
import math

import pytest
import torch

import decode_ref as dr
import kv_fp8_ref as kr
from test_attn_decode_beam_split_gpu import Beam

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = (torch.bfloat16, torch.float32)
GEOMS = dr.ISSUE_GEOMETRIES + dr.MORE_GEOMETRIES


def _name(dt):
    return "bf16" if dt == torch.bfloat16 else "fp32"


def _gid(g):
    return f"{g.n_heads}h{g.n_kv}kv{g.head_dim}"


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


def nan_ws(ops, rows, geom, keys, span):
    return torch.full((ops.attn_decode_split_workspace(rows, geom.n_heads, geom.head_dim, keys, span),), math.nan, dtype=torch.float32, device=DEV)


def fresh(p_rows, geom, dtype):
    H, _, hd = geom
    return (torch.full((p_rows, H * hd), math.nan, dtype=dtype, device=DEV), torch.full((p_rows, H), math.nan, dtype=torch.float32, device=DEV),
            torch.zeros(1, dtype=torch.int32, device=DEV))


def slot_pair(ops, q: kr.QuantisedCache, d: dr.Problem, span=None):
    """(out, lse, n_bad) of the fp8 entry on ``q`` and of the plain entry on the dequantised problem ``d``; ``span``: the split forms."""
    H, KV, hd = d.geom
    qkv, slot, kv_len = d.qkv.to(DEV), d.slot.to(DEV), d.kv_len.to(DEV)
    a, b = fresh(d.rows, d.geom, d.dtype), fresh(d.rows, d.geom, d.dtype)
    if span is None:
        ops.attn_decode_fp8(qkv, *q.tensors(DEV), slot, kv_len, a[0], a[1], H, KV, hd, n_bad=a[2])
        ops.attn_decode(qkv, d.k_cache.to(DEV), d.v_cache.to(DEV), slot, kv_len, b[0], b[1], H, KV, hd, n_bad=b[2])
    else:
        ops.attn_decode_split_fp8(qkv, *q.tensors(DEV), slot, kv_len, a[0], a[1], H, KV, hd, n_bad=a[2], span=span,
                                  workspace=nan_ws(ops, d.rows, d.geom, d.cap, span))
        ops.attn_decode_split(qkv, d.k_cache.to(DEV), d.v_cache.to(DEV), slot, kv_len, b[0], b[1], H, KV, hd, n_bad=b[2], span=span,
                              workspace=nan_ws(ops, d.rows, d.geom, d.cap, span))
    torch.cuda.synchronize()
    return a, b


def same(a, b) -> bool:
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int(a[2]) == int(b[2])


def slot_problem(geom, dtype, case, extra=()):
    """The edge lengths (and ``extra``) with a dead row and a row whose slot lies beyond the cache; V eight times K's magnitude."""
    cap = 2 * dr.chunk_edges(geom.head_dim, dtype)[2] + 3
    lens = dr.edge_lengths(geom.head_dim, dtype, cap) + list(extra) + [9, 9]
    p = dr.make_problem(geom, dtype, lens, case, cap, dead_rows=(len(lens) - 2,))
    slot = p.slot.clone()
    slot[-1] = p.k_cache.shape[0] + 3
    p = p._replace(slot=slot, v_cache=p.v_cache * 8)
    return kr.quantise_problem(p)


@pytest.fixture(scope="module")
def problems():
    made = {}

    def get(geom, dtype, case):
        if (geom, dtype, case) not in made:
            made[(geom, dtype, case)] = slot_problem(geom, dtype, case)
        return made[(geom, dtype, case)]
    return get


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_slot_form_is_bit_equal_to_the_plain_entry_on_the_dequantised_cache(ops, problems, geom, dtype):
    for case in dr.CASES:
        q, d = problems(geom, dtype, case)
        a, b = slot_pair(ops, q, d)
        assert same(a, b), case
        assert int(a[2]) == 1                                           # the slot beyond the cache, once
        assert bool((a[0][-2:] == 0).all()) and bool((a[1][-2:] == -math.inf).all())
        assert bool(torch.isfinite(a[0][:-2].float()).all()), case      # no poison was read


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_split_form_is_bit_equal_at_one_round_and_at_the_default_span(ops, problems, geom, dtype):
    rnd, default = dr.chunk_edges(geom.head_dim, dtype)[2], ops.attn_decode_split_span(geom.head_dim, dtype)
    for case in ("gauss", "spread"):
        q, d = problems(geom, dtype, case)
        for span in sorted({rnd, default}):
            a, b = slot_pair(ops, q, d, span)
            assert same(a, b), (case, span)
            assert int(a[2]) == 1 and bool(torch.isfinite(a[0][:-2].float()).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_direct_check_against_the_exact_reference_on_the_dequantised_problem(ops, problems, dtype):
    for geom in (dr.Geometry(4, 1, 64), dr.Geometry(8, 2, 16)):
        for case in dr.CASES:
            q, d = problems(geom, dtype, case)
            ref = dr.exact(d)
            a, _ = slot_pair(ops, q, d)
            assert dr.violations(a[0], a[1], d, ref) == [], (geom, case)
            a, _ = slot_pair(ops, q, d, dr.chunk_edges(geom.head_dim, dtype)[2])
            assert dr.violations(a[0], a[1], d, ref) == [], (geom, case, "split")


# ---- beam forms ---------------------------------------------------------------------------------------------------------------------------------
def quantised_beam(b: Beam):
    """The beam's two caches as fp8 and dequantised (poison kept: the NaN lines of the caches are the positions no row may read)."""
    KV = b.geom.n_kv
    live_p, live_b = ~torch.isnan(b.pk.float()).any(dim=2), ~torch.isnan(b.bk.float()).any(dim=2)
    qp, dpk, dpv = kr.quantise_cache(b.pk, b.pv * 8, KV, live_p)
    qb, dbk, dbv = kr.quantise_cache(b.bk, b.bv * 8, KV, live_b)
    return qp, qb, (dpk, dpv, dbk, dbv)


def beam_pair(ops, b: Beam, qp, qb, deq, prompt_slot=None, anc=None, span=None):
    H, KV, hd = b.geom
    rows = len(b.np_)
    dev = lambda t: t.to(DEV).contiguous()  # noqa: E731
    idx = (dev(b.prompt_slot if prompt_slot is None else prompt_slot), dev(b.prompt_len), dev(b.gen_len), dev(b.anc if anc is None else anc))
    qkv = b.qkv.to(DEV)
    x, y = fresh(rows, b.geom, b.dtype), fresh(rows, b.geom, b.dtype)
    keys = b.cap_p + min(b.cap_b, b.ld_anc)
    if span is None:
        ops.attn_decode_beam_fp8(qkv, qp.tensors(DEV), qb.tensors(DEV), *idx, x[0], x[1], H, KV, hd, n_bad=x[2])
        ops.attn_decode_beam(qkv, *(t.to(DEV) for t in deq), *idx, y[0], y[1], H, KV, hd, n_bad=y[2])
    else:
        ops.attn_decode_beam_split_fp8(qkv, qp.tensors(DEV), qb.tensors(DEV), *idx, x[0], x[1], H, KV, hd, n_bad=x[2], span=span,
                                       workspace=nan_ws(ops, rows, b.geom, keys, span))
        ops.attn_decode_beam_split(qkv, *(t.to(DEV) for t in deq), *idx, y[0], y[1], H, KV, hd, n_bad=y[2], span=span,
                                   workspace=nan_ws(ops, rows, b.geom, keys, span))
    torch.cuda.synchronize()
    return x, y


@pytest.fixture(scope="module")
def beams():
    made = {}

    def get(geom, dtype):
        if (geom, dtype) not in made:
            b = Beam(geom, dtype)
            made[(geom, dtype)] = (b,) + quantised_beam(b)
        return made[(geom, dtype)]
    return get


BEAM_GEOMS = (dr.Geometry(8, 1, 16), dr.Geometry(4, 1, 64), dr.Geometry(4, 2, 64), dr.Geometry(2, 2, 128))     # G = 8, 4, 2, 1


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geom", BEAM_GEOMS, ids=_gid)
def test_beam_forms_are_bit_equal_plain_and_split(ops, beams, geom, dtype):
    b, qp, qb, deq = beams(geom, dtype)
    spans = sorted({b.span, ops.attn_decode_split_span(geom.head_dim, dtype)})
    for span in [None] + spans:
        x, y = beam_pair(ops, b, qp, qb, deq, span=span)
        assert same(x, y), span
        assert int(x[2]) == 0 and bool(torch.isfinite(x[0].float()).all()) and bool(torch.isfinite(x[1]).all()), span
    # and against fp64 on the materialised, dequantised keys
    b2 = Beam.__new__(Beam)
    b2.__dict__.update(b.__dict__)
    b2.pk, b2.pv, b2.bk, b2.bv = deq
    p = b2.materialised()
    x, _ = beam_pair(ops, b, qp, qb, deq)
    assert dr.violations(x[0], x[1], p, dr.exact(p)) == []


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_beam_indices_outside_a_cache_are_skipped_and_counted_as_the_plain_entries_do(ops, beams, dtype):
    b, qp, qb, deq = beams(dr.Geometry(4, 1, 64), dtype)
    span = b.span
    slot, anc = b.prompt_slot.clone(), b.anc.clone()
    n_ps, n_bs = b.pk.shape[0], b.bk.shape[0]
    by = {(a, g): r for r, (a, g) in enumerate(zip(b.np_, b.ng))}
    anc[by[(span + 1, span + 1)], 5], anc[by[(span - 1, 2)], 0] = n_bs, -1            # one generated key each
    slot[by[(span, span + 1)]], slot[by[(2 * span, 2)]] = n_ps, n_ps + 12345            # the whole prompt
    r_row = by[(span - 1, 1)]
    slot[r_row], anc[r_row, 0] = n_ps, 1 << 30                                          # every key: zeros, -inf
    slot[by[(span + 1, 1)]] = -1                                                        # an inert row: not counted
    for sp in (None, span):
        x, y = beam_pair(ops, b, qp, qb, deq, prompt_slot=slot, anc=anc, span=sp)
        assert same(x, y), sp
        assert int(x[2]) == 5
        assert bool((x[0][r_row] == 0).all()) and bool((x[1][r_row] == -math.inf).all())
        live = [r for r in range(len(b.np_)) if r not in (r_row, by[(span + 1, 1)])]
        assert bool(torch.isfinite(x[0][live].float()).all())
