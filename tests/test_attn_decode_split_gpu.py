"""``ssi_attn_decode_split`` on the GPU: the keys of every (row, kv head) in spans of ``span`` keys, one workgroup each, and the merge launch behind
them — against the checker and the UNCHANGED bound of ``decode_ref.py``

    |out - ref| <= 2^-8 |ref| (bf16 stores only) + C max_j |v_j|,   C = 1.8e-5,   lse within C_LSE

(C was derived from an unchunked fp32 restatement with an 8 x margin, and the one rounding on the store is the plain kernel's), for bf16 and fp32,
``ISSUE_GEOMETRIES`` with all four cases and ``MORE_GEOMETRIES`` with two.  ``span`` is the form's round (``decode_ref.chunk_edges(...)[2]``, the
smallest legal value: many splits at short lengths); the 32 / 8 / 64 geometry also runs at the library's default span.  Lengths: ``edge_lengths``
plus one below, at and one above one and two spans and ``3 span + 1``, in a cap of ``3 span + 2``, with a row of no keys, a row whose length lies
beyond the cap and a row with slot -1.  The caches are poisoned as ``make_problem`` does, out and lse start as NaN and so does the workspace: the
merge must read the partials the walk wrote and nothing else.

Beyond the bound: rows with ``kv_len <= span`` equal ``ops.attn_decode`` by value in out and lse; dead rows, ``kv_len > cap`` and
``slot >= n_slots`` behave as the plain entry with equal ``n_bad``; a row alone equals the same row as row 5 of 7 and the same row in a cache of a
larger cap (more ``n_splits``); every refusal of the header leaves ``out`` untouched.

Measured on the MI355X (the module prints it, run with -s): worst error / tolerance 0.988 on bf16 outputs (the store's own half step, as for the plain
entry) and 0.051 on fp32 outputs; lse 0.107 and 0.096 of C_LSE."""
import math

import pytest
import torch

import decode_ref as dr

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = (torch.bfloat16, torch.float32)
WORST = {}
G1B = dr.Geometry(32, 8, 64)


def _name(dt):
    return "bf16" if dt == torch.bfloat16 else "fp32"


def _gid(g):
    return f"{g.n_heads}h{g.n_kv}kv{g.head_dim}"


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


def round_of(geom, dtype):
    return dr.chunk_edges(geom.head_dim, dtype)[2]


def workspace(ops, rows, geom, cap, span):
    """NaN everywhere: what the walk did not write must not matter."""
    n = ops.attn_decode_split_workspace(rows, geom.n_heads, geom.head_dim, cap, span)
    return torch.full((n,), math.nan, dtype=torch.float32, device=DEV)


def launch(ops, p: dr.Problem, span, rows=None, with_lse=True, n_bad=None, plain=False):
    H, KV, hd = p.geom
    sel = slice(None) if rows is None else rows
    qkv = p.qkv.to(DEV)[sel]
    slot, kv_len = p.slot.to(DEV)[sel].contiguous(), p.kv_len.to(DEV)[sel].contiguous()
    n = qkv.shape[0]
    out = torch.full((n, H * hd), math.nan, dtype=p.dtype, device=DEV)
    lse = torch.full((n, H), math.nan, dtype=torch.float32, device=DEV) if with_lse else None
    if plain:
        ops.attn_decode(qkv, p.k_cache.to(DEV), p.v_cache.to(DEV), slot, kv_len, out, lse, H, KV, hd, n_bad=n_bad)
    else:
        ops.attn_decode_split(qkv, p.k_cache.to(DEV), p.v_cache.to(DEV), slot, kv_len, out, lse, H, KV, hd, n_bad=n_bad, span=span,
                              workspace=workspace(ops, n, p.geom, p.cap, span))
    torch.cuda.synchronize()
    return out, lse


def split_problem(geom, dtype, case, span):
    """Every edge length of the kernel and of the split, a row of length 0, a row whose length lies beyond the cap (clamped), a row with slot -1."""
    cap = 3 * span + 2
    lens = sorted(set(dr.edge_lengths(geom.head_dim, dtype, cap)) | {span - 1, span, span + 1, 2 * span - 1, 2 * span, 2 * span + 1, 3 * span + 1})
    lens = lens + [0, cap + 5, 33]
    return dr.make_problem(geom, dtype, lens, case, cap, dead_rows=(len(lens) - 1,))


@pytest.fixture(scope="module")
def problems():
    """A problem and its float64 reference, computed once per (geometry, dtype, case, span)."""
    made = {}

    def get(geom, dtype, case, span):
        key = (geom, dtype, case, span)
        if key not in made:
            p = split_problem(geom, dtype, case, span)
            made[key] = (p, dr.exact(p))
        return made[key]
    return get


def check(ops, p, ref, span):
    out, lse = launch(ops, p, span)
    bad = dr.violations(out, lse, p, ref)
    live = ~ref.dead
    ratio = ((out.cpu().double() - ref.out).abs() / dr.tolerance(p, ref))[live].max()
    lratio = (lse.cpu().double() - ref.lse)[live].abs().max() / dr.C_LSE
    w = WORST.setdefault(_name(p.dtype), [0.0, 0.0])
    w[0], w[1] = max(w[0], float(ratio)), max(w[1], float(lratio))
    print(f"{_gid(p.geom)} {_name(p.dtype)} {p.case} span {span}: worst err / tolerance out {float(ratio):.3f} lse {float(lratio):.3f}")
    assert bad == [], (p.geom, p.case, span, bad)
    return out, lse


EDGE = [(g, c) for g in dr.ISSUE_GEOMETRIES for c in dr.CASES] + [(g, c) for g in dr.MORE_GEOMETRIES for c in ("gauss", "spread")]


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geom,case", EDGE, ids=[f"{_gid(g)}-{c}" for g, c in EDGE])
def test_every_row_and_head_at_every_edge_length_of_kernel_and_split(ops, problems, geom, case, dtype):
    span = round_of(geom, dtype)
    p, ref = problems(geom, dtype, case, span)
    assert int(ref.dead.sum()) == 2 and int(p.kv_len.max()) > p.cap
    out, lse = check(ops, p, ref, span)
    # rows of at most one span: the plain entry's values (a zero may differ in sign: by value, not by bit pattern)
    want, want_lse = launch(ops, p, span, plain=True)
    short = (p.kv_len <= span).to(DEV)
    assert int(short.sum()) >= 4 and int((~short).sum()) >= 6
    assert torch.equal(out[short], want[short]) and torch.equal(lse[short], want_lse[short])


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("case", dr.CASES)
def test_the_1b_geometry_at_the_default_span(ops, problems, case, dtype):
    span = ops.attn_decode_split_span(G1B.head_dim, dtype)
    assert span > 0 and span % round_of(G1B, dtype) == 0
    p, ref = problems(G1B, dtype, case, span)
    out, lse = check(ops, p, ref, span)
    want, want_lse = launch(ops, p, span, plain=True)
    short = (p.kv_len <= span).to(DEV)
    assert torch.equal(out[short], want[short]) and torch.equal(lse[short], want_lse[short])


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_dead_rows_long_rows_and_slots_beyond_the_cache_are_the_plain_entrys(ops, dtype):
    geom = dr.Geometry(8, 2, 16)
    span = round_of(geom, dtype)
    cap = 3 * span + 2
    p = dr.make_problem(geom, dtype, [5, span + 3, 9, 2 * span, 0, cap + 9, 1], "gauss", cap, dead_rows=(6,))
    n_slots = p.k_cache.shape[0]
    slot = p.slot.clone()
    slot[1], slot[3] = n_slots, n_slots + 1000
    p = p._replace(slot=slot)
    ref = dr.exact(p)
    assert ref.dead.tolist() == [False, True, False, True, True, False, True]
    n_bad, n_bad_plain = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    out, lse = launch(ops, p, span, n_bad=n_bad)
    want, want_lse = launch(ops, p, span, n_bad=n_bad_plain, plain=True)
    assert dr.violations(out, lse, p, ref) == []
    assert int(n_bad) == int(n_bad_plain) == 2
    dead = ref.dead.to(DEV)
    assert torch.equal(out[dead], want[dead]) and torch.equal(lse[dead], want_lse[dead])
    out2, _ = launch(ops, p, span, with_lse=False)          # no counter, no lse: both may be NULL
    assert torch.equal(out2, out)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geom", (dr.Geometry(8, 2, 16), G1B), ids=_gid)
def test_a_rows_result_depends_on_its_own_inputs_and_the_span_only(ops, geom, dtype):
    span = round_of(geom, dtype)
    cap = 3 * span + 2
    n = 2 * span + 1
    p = dr.make_problem(geom, dtype, [3, span, span + 7, 1, 3 * span + 1, n, 2 * span], "spread", cap)
    out, lse = launch(ops, p, span)
    o1, l1 = launch(ops, p, span, rows=slice(5, 6))         # alone: another grid, another place in it
    assert torch.equal(o1[0], out[5]) and torch.equal(l1[0], lse[5])
    # the same row in a cache of a larger cap: more splits in the grid, a longer line of partials per head
    s = int(p.slot[5])
    big_cap = 7 * span + 5
    kc = torch.full((p.k_cache.shape[0], big_cap, p.k_cache.shape[2]), math.nan).to(dtype)
    vc = kc.clone()
    kc[s, :n], vc[s, :n] = p.k_cache[s, :n], p.v_cache[s, :n]
    big = p._replace(k_cache=kc, v_cache=vc)
    o2, l2 = launch(ops, big, span, rows=slice(5, 6))
    assert torch.equal(o2[0], out[5]) and torch.equal(l2[0], lse[5])
    # other rows' queries change: this row's bits stay
    q3 = p.qkv.clone()
    q3[torch.arange(p.rows) != 5] *= -0.5
    o3, l3 = launch(ops, p._replace(qkv=q3), span)
    assert torch.equal(o3[5], out[5]) and torch.equal(l3[5], lse[5]) and not torch.equal(o3[4], out[4])


def test_refusals_leave_out_untouched(ops):
    geom, dtype = dr.Geometry(4, 1, 64), torch.bfloat16
    H, KV, hd = geom
    rnd = round_of(geom, dtype)
    cap = 3 * rnd + 2
    p = dr.make_problem(geom, dtype, [5, 2 * rnd + 1], "gauss", cap)
    qkv, kc, vc, slot, kv_len = (t.to(DEV) for t in (p.qkv, p.k_cache, p.v_cache, p.slot, p.kv_len))
    out = torch.full((p.rows, H * hd), math.nan, dtype=dtype, device=DEV)
    lib, args = ops._lib.load(), ops._slot_args("attn_decode_split", qkv, kc, vc, slot, kv_len, out, None, H, KV, hd, None)
    ws = workspace(ops, p.rows, geom, cap, rnd)
    bytes_ = ws.numel() * 4
    code, stream = ops.dtype_code(dtype), ops.stream_ptr()

    def refused(span, n_splits, ws_ptr, ws_bytes):
        rc = lib.ssi_attn_decode_split(*args, span, n_splits, ws_ptr, ws_bytes, code, stream)
        torch.cuda.synchronize()
        assert rc == 1, (span, n_splits, rc)                 # SSI_ERR_ARG
        assert bool(torch.isnan(out.float()).all())

    ok_splits = -(-cap // rnd)
    for span in (0, -rnd, rnd - 1, rnd + 8, rnd // 2):       # no positive multiple of the round
        refused(span, 65535, ws.data_ptr(), 1 << 40)
    for n_splits in (0, -1, 65536):
        refused(rnd, n_splits, ws.data_ptr(), 1 << 40)
    refused(rnd, ok_splits - 1, ws.data_ptr(), bytes_)      # n_splits * span < cap: a key could be dropped
    refused(rnd, ok_splits, None, bytes_)                   # no workspace
    refused(rnd, ok_splits, ws.data_ptr() + 4, bytes_)      # misaligned
    refused(rnd, ok_splits, ws.data_ptr(), bytes_ - 4)      # too small
    with pytest.raises(RuntimeError, match="code 1"):       # the wrapper hands the library's refusal on
        ops.attn_decode_split(qkv, kc, vc, slot, kv_len, out, None, H, KV, hd, span=rnd + 8, workspace=ws)
    with pytest.raises(RuntimeError, match="code 1"):
        ops.attn_decode_split(qkv, kc, vc, slot, kv_len, out, None, H, KV, hd, span=rnd, workspace=ws[:-1])
    assert bool(torch.isnan(out.float()).all())
    assert lib.ssi_attn_decode_split(*args, rnd, ok_splits, ws.data_ptr(), bytes_, code, stream) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all())


@pytest.mark.parametrize("geom", (dr.Geometry(4, 1, 12), dr.Geometry(16, 1, 16), dr.Geometry(2, 1, 136)), ids=str)
def test_other_geometries_are_refused(ops, geom):
    H, KV, hd = geom
    qkv = torch.zeros(2, (H + 2 * KV) * hd, dtype=torch.float32, device=DEV)
    cache = torch.zeros(2, 4, KV * hd, dtype=torch.float32, device=DEV)
    i32 = torch.zeros(2, dtype=torch.int32, device=DEV)
    assert ops.attn_decode_split_span(hd, torch.float32) == (0 if hd % 8 or hd > 128 else max(128, dr.chunk_edges(hd, torch.float32)[2]))
    with pytest.raises(RuntimeError, match="code 2"):
        ops.attn_decode_split(qkv, cache, cache.clone(), i32, i32, torch.zeros(2, H * hd, device=DEV), None, H, KV, hd, span=512,
                              workspace=torch.zeros(1 << 16, device=DEV))
