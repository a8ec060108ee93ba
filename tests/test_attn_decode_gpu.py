"""``ssi_attn_decode`` and ``ssi_kv_store`` on the GPU: every (row, head) of every launch against the checker of ``decode_ref.py``

    |out - ref| <= 2^-8 |ref| (bf16 stores only) + C max_j |v_j|,   C = 1.8e-5 = 8 x the fp32 restatement's distance from fp64

for bf16 and fp32, lse within C_LSE, all values finite although every cache position at or beyond a row's length and every slot no row
names holds NaN, dead rows (slot -1, kv_len 0, slot >= n_slots) exact zeros with lse -inf.

The kernel's edges (``decode_ref.chunk_edges``): a key lies on head_dim * sizeof / 16 lanes rounded up to a power of two, a wave holds 64
lanes' keys per load (KPW), takes chunks of two loads, and the four waves take a round of 8 KPW keys.  bf16 head_dim 64: 8 / 16 / 64;
fp32 head_dim 64: 4 / 8 / 32; bf16 head_dim 16: 32 / 64 / 256; fp32 head_dim 16: 16 / 32 / 128.  kv_len runs through 1, 2 and one below,
at and one above each of them and two rounds, in a cap of 300; one launch has a row of 1000 keys beside a row of one.

The kernel has ONE form; what the dispatch chooses is the number of query-head registers (1, 2, 4, 8) and the storage type: the issue's
geometries have g = 4 and 1, ``MORE_GEOMETRIES`` add g = 2, 8, 3 (runs the form of 4), 5 (the form of 8), head_dim 8, 24 (idle lanes in a
key group) and 128.  ``ssi_set_impl`` has nothing to choose here, which one test holds.

Measured on the MI355X (the module prints it, run with -s): worst error / tolerance 0.98 on bf16 outputs (a value just above a power of two,
where the store's own half step is the whole 2^-8 term) and 0.08 on fp32 outputs; lse 0.09 and 0.10 of C_LSE.  110 tests in 3 s."""
import math

import pytest
import torch

import decode_ref as dr

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = (torch.bfloat16, torch.float32)
CAP = 300
WORST = {}


def _name(dt):
    return "bf16" if dt == torch.bfloat16 else "fp32"


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"\nworst err / tolerance  {k:12s} out {WORST[k][0]:.3f}  lse {WORST[k][1]:.3f}", end="")
    print()


def launch(ops, p: dr.Problem, rows=None, with_lse=True, n_bad=None):
    """The kernel on a problem (or on the rows ``rows`` of it alone); out and lse start as NaN so that an unwritten element shows."""
    H, KV, hd = p.geom
    sel = slice(None) if rows is None else rows
    qkv = p.qkv.to(DEV)[sel]
    slot, kv_len = p.slot.to(DEV)[sel].contiguous(), p.kv_len.to(DEV)[sel].contiguous()
    n = qkv.shape[0]
    out = torch.full((n, H * hd), math.nan, dtype=p.dtype, device=DEV)
    lse = torch.full((n, H), math.nan, dtype=torch.float32, device=DEV) if with_lse else None
    ops.attn_decode(qkv, p.k_cache.to(DEV), p.v_cache.to(DEV), slot, kv_len, out, lse, H, KV, hd, n_bad=n_bad)
    torch.cuda.synchronize()
    return out, lse


def check(ops, p: dr.Problem):
    ref = dr.exact(p)
    out, lse = launch(ops, p)
    bad = dr.violations(out, lse, p, ref)
    live = ~ref.dead
    if live.any():
        ratio = ((out.cpu().double() - ref.out).abs() / dr.tolerance(p, ref))[live].max()
        lratio = (lse.cpu().double() - ref.lse)[live].abs().max() / dr.C_LSE
        w = WORST.setdefault(_name(p.dtype), [0.0, 0.0])
        w[0], w[1] = max(w[0], float(ratio)), max(w[1], float(lratio))
    assert bad == [], (p.geom, p.case, bad)
    return out, lse, ref


def edge_problem(geom, dtype, case):
    """Every edge length, a row of length 0, a row whose length lies beyond the cap (clamped), and a row with slot -1."""
    lens = dr.edge_lengths(geom.head_dim, dtype, CAP) + [0, CAP + 5, 33]
    return dr.make_problem(geom, dtype, lens, case, CAP, dead_rows=(len(lens) - 1,))


EDGE = [(g, c) for g in dr.ISSUE_GEOMETRIES for c in dr.CASES] + [(g, c) for g in dr.MORE_GEOMETRIES for c in ("gauss", "spread")]


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geom,case", EDGE, ids=[f"{g.n_heads}h{g.n_kv}kv{g.head_dim}-{c}" for g, c in EDGE])
def test_every_row_and_head_at_every_edge_length(ops, geom, case, dtype):
    p = edge_problem(geom, dtype, case)
    assert CAP % dr.chunk_edges(geom.head_dim, dtype)[1] or geom.head_dim == 128       # the cap is no multiple of the chunk
    assert not bool((p.slot[:-1] == torch.arange(p.rows - 1)).all())                    # the slots are not the identity
    _, _, ref = check(ops, p)
    assert int(ref.dead.sum()) == 2


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("case", ("newest", "spread", "sink"))
@pytest.mark.parametrize("geom", dr.ISSUE_GEOMETRIES, ids=lambda g: f"{g.n_heads}h{g.n_kv}kv{g.head_dim}")
def test_one_long_row_beside_a_row_of_one_key(ops, geom, case, dtype):
    check(ops, dr.make_problem(geom, dtype, [1000, 1, 257], case, 1003))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("rows", (1, 3))
def test_few_rows(ops, rows, dtype):
    for geom in (dr.Geometry(8, 2, 16), dr.Geometry(32, 8, 64)):
        check(ops, dr.make_problem(geom, dtype, [65, 1, 129][:rows], "spread", CAP))


def many_rows_problem(geom, dtype):
    return dr.make_problem(geom, dtype, dr.ragged_lengths(256, geom.head_dim, dtype, CAP), "spread", CAP)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geom", (dr.Geometry(8, 2, 16), dr.Geometry(4, 1, 64)), ids=lambda g: f"{g.n_heads}h{g.n_kv}kv{g.head_dim}")
def test_256_rows_and_a_row_alone_gives_the_same_bits(ops, geom, dtype):
    """Independence: the result of a row is bit-equal whether it is launched alone or among 255 others (another grid, another place in
    it, other slots alive beside it)."""
    p = many_rows_problem(geom, dtype)
    out, lse, _ = check(ops, p)
    longest = int(p.kv_len.argmax())
    for r in sorted({0, 1, longest, 100, 255}):
        o1, l1 = launch(ops, p, rows=slice(r, r + 1))
        assert torch.equal(o1[0], out[r]) and torch.equal(l1[0], lse[r]), r
    # and among a handful, in another order
    idx = torch.tensor([255, longest, 3, 0])
    o4, l4 = launch(ops, p, rows=idx.to(DEV))
    assert torch.equal(o4, out[idx.to(DEV)]) and torch.equal(l4, lse[idx.to(DEV)])


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_a_slot_beyond_the_cache_is_counted_and_gives_zeros(ops, dtype):
    p = dr.make_problem(dr.Geometry(8, 2, 16), dtype, [5, 70, 9, 64, 1], "gauss", CAP)
    n_slots = p.k_cache.shape[0]
    slot = p.slot.clone()
    slot[1], slot[3] = n_slots, n_slots + 1000
    p = p._replace(slot=slot)
    n_bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    ref = dr.exact(p)
    assert ref.dead.tolist() == [False, True, False, True, False]
    out, lse = launch(ops, p, n_bad=n_bad)
    assert dr.violations(out, lse, p, ref) == []
    assert int(n_bad) == 2
    out2, _ = launch(ops, p, with_lse=False)          # no counter, no lse: both may be NULL
    assert torch.equal(out2, out)


def test_the_impl_switch_has_nothing_to_choose(ops):
    from ssi import _lib
    p = edge_problem(dr.Geometry(4, 1, 64), torch.bfloat16, "spread")
    out, lse = launch(ops, p)
    prev = ops.set_impl(_lib.IMPL_GENERIC)
    try:
        out_g, lse_g = launch(ops, p)
    finally:
        ops.set_impl(prev)
    assert torch.equal(out_g, out) and torch.equal(lse_g, lse)


@pytest.mark.parametrize("geom", (dr.Geometry(4, 1, 12), dr.Geometry(16, 1, 16), dr.Geometry(2, 1, 136)), ids=str)
def test_other_geometries_are_refused(ops, geom):
    H, KV, hd = geom
    qkv = torch.zeros(2, (H + 2 * KV) * hd, dtype=torch.float32, device=DEV)
    cache = torch.zeros(2, 4, KV * hd, dtype=torch.float32, device=DEV)
    i32 = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="code 2"):
        ops.attn_decode(qkv, cache, cache.clone(), i32, i32, torch.zeros(2, H * hd, device=DEV), None, H, KV, hd)
    with pytest.raises(RuntimeError, match="code 2"):
        ops.kv_store(qkv, torch.zeros(2, dtype=torch.int64, device=DEV), cache, cache.clone(), H, KV, hd)


# ---- ssi_kv_store ------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("rows", (1, 5, 256))
@pytest.mark.parametrize("geom", (dr.Geometry(8, 2, 16), dr.Geometry(32, 8, 64), dr.Geometry(5, 1, 24)), ids=lambda g: f"{g.n_heads}h{g.n_kv}kv{g.head_dim}")
def test_kv_store_copies_the_bits_and_nothing_else(ops, geom, rows, dtype):
    """Bit-exact for both dtypes (the rows hold NaN payloads, infinities and denormals too), ``ld`` larger than the row, ``dest = -1``
    skipped, a ``dest`` outside the cache skipped and counted, and every cache element no row named keeps its sentinel."""
    H, KV, hd = geom
    n_slots, cap = 7, 41
    n_dest, width = n_slots * cap, KV * hd
    g = torch.Generator().manual_seed(3 + rows)
    ld = (H + 2 * KV) * hd + 24
    ibits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    raw = torch.randint(-2 ** 15, 2 ** 15, (rows, ld), generator=g).to(ibits) if dtype == torch.bfloat16 else \
        torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, ld), generator=g, dtype=torch.int64).to(ibits)
    qkv = raw.view(dtype)                                       # any bit pattern
    assert rows <= n_dest
    dest = torch.randperm(n_dest, generator=g)[:rows].to(torch.int64)      # distinct places (256 rows into 287)
    skipped, outside = [], []
    if rows >= 5:
        dest[1] = -1
        skipped = [1]
        dest[2], dest[4] = n_dest, -7
        outside = [2, 4]
    if rows == 256:
        dest[77], dest[200] = 2 ** 40, n_dest + 12345
        outside += [77, 200]
    sentinel = 0x3F9D                                           # (an ordinary finite pattern in either type)
    kc = torch.full((n_slots, cap, width), sentinel, dtype=ibits).view(dtype)
    vc = torch.full((n_slots, cap, width), sentinel, dtype=ibits).view(dtype)
    want_k, want_v = _bits(kc).clone().view(n_dest, width), _bits(vc).clone().view(n_dest, width)
    for r in range(rows):
        if r in skipped or r in outside:
            continue
        want_k[int(dest[r])] = raw[r, H * hd:(H + KV) * hd]
        want_v[int(dest[r])] = raw[r, (H + KV) * hd:(H + 2 * KV) * hd]
    kd, vd = kc.to(DEV), vc.to(DEV)
    n_bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.kv_store(qkv.to(DEV), dest.to(DEV), kd, vd, H, KV, hd, n_bad=n_bad)
    torch.cuda.synchronize()
    assert torch.equal(_bits(kd).cpu().view(n_dest, width), want_k)
    assert torch.equal(_bits(vd).cpu().view(n_dest, width), want_v)
    assert int(n_bad) == len(outside)
    if outside:                                                 # without a counter the rows are skipped all the same
        kd2, vd2 = kc.to(DEV), vc.to(DEV)
        ops.kv_store(qkv.to(DEV), dest.to(DEV), kd2, vd2, H, KV, hd)
        assert torch.equal(_bits(kd2), _bits(kd)) and torch.equal(_bits(vd2), _bits(vd))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_store_then_attend(ops, dtype):
    """The two entries together: the k / v columns of qkv rows stored at slot * cap + position are what the attention then reads."""
    geom = dr.Geometry(8, 2, 16)
    H, KV, hd = geom
    p = dr.make_problem(geom, dtype, [40, 17], "spread", 64, poison=False)
    kd, vd = torch.full_like(p.k_cache, math.nan).to(DEV), torch.full_like(p.v_cache, math.nan).to(DEV)
    for r in range(p.rows):
        s, n = int(p.slot[r]), int(p.kv_len[r])
        rows = torch.zeros(n, (H + 2 * KV) * hd, dtype=dtype)
        rows[:, H * hd:(H + KV) * hd] = p.k_cache[s, :n]
        rows[:, (H + KV) * hd:] = p.v_cache[s, :n]
        ops.kv_store(rows.to(DEV), (s * p.cap + torch.arange(n)).to(DEV), kd, vd, H, KV, hd)
    out = torch.full((p.rows, H * hd), math.nan, dtype=dtype, device=DEV)
    ops.attn_decode(p.qkv.to(DEV), kd, vd, p.slot.to(DEV), p.kv_len.to(DEV), out, None, H, KV, hd)
    assert dr.violations(out, None, p, dr.exact(p)) == []
