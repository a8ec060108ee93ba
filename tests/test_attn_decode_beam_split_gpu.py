"""``ssi_attn_decode_beam_split`` on the GPU: the split-KV walk over a prompt cache slot and, behind it, a beam cache read through an ancestry table.

* VALUES: out and lse ``torch.equal`` to ``ops.attn_decode_split`` with the same span on a cache in which every row's keys were materialised one
  behind the other (the walk is over the concatenated key index, and both forms run one merge);
* float64: the checker and the bound of ``decode_ref.py``, unchanged.

``span`` is the form's round.  Rows: every pairing of prompt_len in {span - 1, span, span + 1, 2 span} with gen_len in {1, 2, span + 1}: the seam
between prompt and generated keys falls inside a split, on a split edge and one key either side of it.  bf16 and fp32, the four query-head register
counts (G = 8, 4, 2, 1) at head_dim 16, 64, 64, 128.  The rows of one prompt_len share a prompt slot, the ancestry is a simulated beam history, neither
slot numbering is the identity, NaN sits in every cache position no row may read and in the whole workspace, and the pad columns of ``anc`` hold an
index far outside the cache.

Indices out of range: one key skipped; a whole split skipped (its partial is the empty state, M = -inf); the whole row skipped (zeros, lse -inf).
Each such row is counted once, however many of its keys and splits were dropped.

Measured on the MI355X: worst error / tolerance 0.960 on bf16 outputs, 0.069 on fp32 outputs."""
import math

import pytest
import torch

import decode_ref as dr

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = (torch.bfloat16, torch.float32)
GEOMS = (dr.Geometry(8, 1, 16), dr.Geometry(4, 1, 64), dr.Geometry(4, 2, 64), dr.Geometry(2, 2, 128))     # G = 8, 4, 2, 1
FAR = 1 << 30


def _name(dt):
    return "bf16" if dt == torch.bfloat16 else "fp32"


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


class Beam:
    """One launch and the materialised problem it must equal."""

    def __init__(self, geom, dtype, seed=5):
        H, KV, hd = geom
        span = self.span = dr.chunk_edges(hd, dtype)[2]
        p_lens, g_lens = [span - 1, span, span + 1, 2 * span], [1, 2, span + 1]
        pairs = [(a, b) for a in p_lens for b in g_lens]
        self.geom, self.dtype, rows = geom, dtype, len(pairs)
        self.np_, self.ng = [a for a, _ in pairs], [b for _, b in pairs]
        g = torch.Generator().manual_seed(seed)
        T = max(g_lens)
        self.cap_p, self.cap_b, self.ld_anc = max(p_lens) + 2, T + 1, T + 3
        base = dr.make_problem(geom, dtype, [a + b for a, b in pairs], "spread", max(p_lens) + T, seed, poison=False, spare_slots=0)
        self.qkv = base.qkv
        n_prompts = len(p_lens)
        pperm = torch.randperm(n_prompts + 1, generator=g).roll(1)             # prompt slot of prompt q; one slot is spare
        bperm = torch.randperm(rows + 2, generator=g).roll(1)                  # beam slot of row r; two are spare
        self.prompt_of = [p_lens.index(a) for a in self.np_]
        self.prompt_slot = torch.tensor([int(pperm[q]) for q in self.prompt_of], dtype=torch.int32)
        width, nan = KV * hd, float("nan")
        self.pk, self.pv = (torch.full((n_prompts + 1, self.cap_p, width), nan).to(dtype) for _ in range(2))
        self.bk, self.bv = (torch.full((rows + 2, self.cap_b, width), nan).to(dtype) for _ in range(2))
        anc = torch.full((rows, self.ld_anc), FAR, dtype=torch.int32)
        for q in range(n_prompts):                                             # a beam history per group of rows
            group = [r for r in range(rows) if self.prompt_of[r] == q]
            a = torch.zeros(len(group), T, dtype=torch.int32)
            for i in range(T):
                a = a[torch.randint(0, len(group), (len(group),), generator=g)]
                a[:, i] = torch.tensor([int(bperm[r]) for r in group], dtype=torch.int32)
            for j, r in enumerate(group):
                anc[r, :T] = a[j]
            s0 = int(base.slot[group[0]])                                      # the prompt's keys: those of the group's first row
            self.pk[int(pperm[q]), :p_lens[q]] = base.k_cache[s0, :p_lens[q]]
            self.pv[int(pperm[q]), :p_lens[q]] = base.v_cache[s0, :p_lens[q]]
        self.anc = anc
        filled = torch.zeros(rows + 2, self.cap_b, dtype=torch.bool)
        for r in range(rows):                                                  # a generated position: the keys of the first row that names it
            s = int(base.slot[r])
            for i in range(self.ng[r]):
                a = int(anc[r, i])
                if not filled[a, i]:
                    self.bk[a, i], self.bv[a, i] = base.k_cache[s, self.np_[r] + i], base.v_cache[s, self.np_[r] + i]
                    filled[a, i] = True
        self.prompt_len = torch.tensor(self.np_, dtype=torch.int32)
        self.gen_len = torch.tensor(self.ng, dtype=torch.int32)

    def materialised(self, skip=lambda r, j: False, prompt_slot=None, anc=None) -> dr.Problem:
        """Every row's keys one behind the other in a slot of its own (``skip(r, j)``: the concatenated key j of row r is left out and not looked up)."""
        rows, width = len(self.np_), self.pk.shape[2]
        cap = max(a + b for a, b in zip(self.np_, self.ng)) + 1
        kc, vc = (torch.full((rows, cap, width), float("nan")).to(self.dtype) for _ in range(2))
        lens = []
        for r in range(rows):
            keys = [(self.pk, self.pv, int(self.prompt_slot[r]), j) for j in range(self.np_[r])]
            keys += [(self.bk, self.bv, int(self.anc[r, i]), i) for i in range(self.ng[r])]
            keys = [k for j, k in enumerate(keys) if not skip(r, j)]
            for j, (ck, cv, s, at) in enumerate(keys):
                kc[r, j], vc[r, j] = ck[s, at], cv[s, at]
            lens.append(len(keys))
        return dr.Problem(self.geom, self.dtype, self.qkv, kc, vc, torch.arange(rows, dtype=torch.int32), torch.tensor(lens, dtype=torch.int32), "spread")


def nan_ws(ops, rows, geom, keys, span):
    return torch.full((ops.attn_decode_split_workspace(rows, geom.n_heads, geom.head_dim, keys, span),), math.nan, dtype=torch.float32, device=DEV)


def launch(ops, b: Beam, rows=None, prompt_slot=None, anc=None, with_lse=True, n_bad=None):
    H, KV, hd = b.geom
    sel = slice(None) if rows is None else rows
    dev = lambda t: t.to(DEV)[sel].contiguous()  # noqa: E731
    qkv = b.qkv.to(DEV)[sel]
    n = qkv.shape[0]
    out = torch.full((n, H * hd), math.nan, dtype=b.dtype, device=DEV)
    lse = torch.full((n, H), math.nan, dtype=torch.float32, device=DEV) if with_lse else None
    ops.attn_decode_beam_split(qkv, b.pk.to(DEV), b.pv.to(DEV), b.bk.to(DEV), b.bv.to(DEV), dev(b.prompt_slot if prompt_slot is None else prompt_slot),
                               dev(b.prompt_len), dev(b.gen_len), dev(b.anc if anc is None else anc), out, lse, H, KV, hd, n_bad=n_bad, span=b.span,
                               workspace=nan_ws(ops, n, b.geom, b.cap_p + min(b.cap_b, b.ld_anc), b.span))
    torch.cuda.synchronize()
    return out, lse


def contiguous(ops, p: dr.Problem, span):
    H, KV, hd = p.geom
    out = torch.full((p.rows, H * hd), math.nan, dtype=p.dtype, device=DEV)
    lse = torch.full((p.rows, H), math.nan, dtype=torch.float32, device=DEV)
    ops.attn_decode_split(p.qkv.to(DEV), p.k_cache.to(DEV), p.v_cache.to(DEV), p.slot.to(DEV), p.kv_len.to(DEV), out, lse, H, KV, hd, span=span,
                          workspace=nan_ws(ops, p.rows, p.geom, p.cap, span))
    torch.cuda.synchronize()
    return out, lse


@pytest.fixture(scope="module")
def beams():
    made = {}

    def get(geom, dtype):
        if (geom, dtype) not in made:
            b = Beam(geom, dtype)
            p = b.materialised()
            made[(geom, dtype)] = (b, p, dr.exact(p))
        return made[(geom, dtype)]
    return get


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g.n_heads}h{g.n_kv}kv{g.head_dim}")
def test_equal_to_the_split_slot_form_on_the_materialised_cache_and_within_the_bound(ops, beams, geom, dtype):
    b, p, ref = beams(geom, dtype)
    assert not bool((b.prompt_slot == torch.tensor(b.prompt_of)).all())                           # neither numbering is the identity
    assert len(set(b.prompt_slot.tolist())) < len(b.np_)                                           # rows share prompt slots
    n_bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, lse = launch(ops, b, n_bad=n_bad)
    want_out, want_lse = contiguous(ops, p, b.span)
    assert torch.equal(out, want_out) and torch.equal(lse, want_lse)
    assert int(n_bad) == 0                                                                          # (the pad columns of anc were not read)
    assert dr.violations(out, lse, p, ref) == []
    assert not bool(ref.dead.any())
    ratio = ((out.cpu().double() - ref.out).abs() / dr.tolerance(p, ref)).max()
    print(f"{geom} {_name(dtype)}: worst err / tolerance {float(ratio):.3f}")
    out2, _ = launch(ops, b, with_lse=False)                                                        # no counter, no lse: both may be NULL
    assert torch.equal(out2, out)
    o1, l1 = launch(ops, b, rows=slice(11, 12))                                                     # the longest row alone
    assert torch.equal(o1[0], out[11]) and torch.equal(l1[0], lse[11])


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_a_negative_prompt_slot_gives_a_zero_row(ops, beams, dtype):
    b, p, ref = beams(dr.Geometry(4, 1, 64), dtype)
    clean, clean_lse = launch(ops, b)
    off = [2, 7]
    slot = b.prompt_slot.clone()
    slot[off] = torch.tensor([-1, -(1 << 30)], dtype=torch.int32)
    n_bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, lse = launch(ops, b, prompt_slot=slot, n_bad=n_bad)
    assert bool((out[off] == 0).all()) and bool((lse[off] == -math.inf).all()) and int(n_bad) == 0
    keep = [r for r in range(len(b.np_)) if r not in off]
    assert torch.equal(out[keep], clean[keep]) and torch.equal(lse[keep], clean_lse[keep])


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geom", (dr.Geometry(4, 1, 64), dr.Geometry(8, 1, 16)), ids=lambda g: f"{g.n_heads}h{g.n_kv}kv{g.head_dim}")
def test_indices_outside_a_cache_skip_a_key_a_split_or_the_row_and_count_the_row_once(ops, beams, geom, dtype):
    b, p, ref = beams(geom, dtype)
    span = b.span
    clean, clean_lse = launch(ops, b)
    rows = len(b.np_)
    slot, anc = b.prompt_slot.clone(), b.anc.clone()
    n_ps, n_bs = b.pk.shape[0], b.bk.shape[0]
    by = {(a, g): r for r, (a, g) in enumerate(zip(b.np_, b.ng))}
    r_key, r_key2 = by[(span + 1, span + 1)], by[(span - 1, 2)]          # one generated key skipped (inside split 1; the seam's own key)
    anc[r_key, 5], anc[r_key2, 0] = n_bs, -1
    r_split, r_split2 = by[(span, span + 1)], by[(2 * span, 2)]          # a prompt slot outside its cache: split 0 (and 1) hold no key at all
    slot[r_split], slot[r_split2] = n_ps, n_ps + 12345
    r_row = by[(span - 1, 1)]                                              # neither the prompt nor the one generated key: zeros, -inf
    slot[r_row], anc[r_row, 0] = n_ps, FAR
    r_many = by[(span + 1, 2)]                                             # several bad entries in one row: still one count
    anc[r_many, 0], anc[r_many, 1] = -(1 << 31), n_bs + 7
    touched = {r_key, r_key2, r_split, r_split2, r_row, r_many}
    assert len(touched) == 6

    def skip(r, j):
        if r in (r_split, r_split2, r_row) and j < b.np_[r]:
            return True
        i = j - b.np_[r]
        return (r == r_key and i == 5) or (r == r_key2 and i == 0) or (r == r_row and i == 0) or (r == r_many and i in (0, 1))

    b2 = Beam.__new__(Beam)                                                # the dropped entries must not be looked up by the reference either
    b2.__dict__.update(b.__dict__)
    b2.prompt_slot = torch.where(slot >= n_ps, torch.zeros_like(slot), slot)
    b2.anc = torch.where((anc < 0) | (anc >= n_bs), torch.zeros_like(anc), anc)
    p2 = b2.materialised(skip)
    ref2 = dr.exact(p2)
    assert bool(ref2.dead[r_row]) and int(ref2.dead.sum()) == 1
    n_bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, lse = launch(ops, b, prompt_slot=slot, anc=anc, n_bad=n_bad)
    assert int(n_bad) == len(touched)
    assert dr.violations(out, lse, p2, ref2) == []
    assert bool((out[r_row] == 0).all()) and bool((lse[r_row] == -math.inf).all())
    keep = [r for r in range(rows) if r not in touched]
    assert torch.equal(out[keep], clean[keep]) and torch.equal(lse[keep], clean_lse[keep])
    out3, _ = launch(ops, b, prompt_slot=slot, anc=anc, with_lse=False)   # without a counter the keys are dropped all the same
    assert torch.equal(out3, out)
    # the plain beam entry counts the same rows
    H, KV, hd = geom
    n_plain = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.attn_decode_beam(b.qkv.to(DEV), b.pk.to(DEV), b.pv.to(DEV), b.bk.to(DEV), b.bv.to(DEV), slot.to(DEV), b.prompt_len.to(DEV), b.gen_len.to(DEV),
                         anc.to(DEV), torch.empty_like(out), None, H, KV, hd, n_bad=n_plain)
    assert int(n_plain) == int(n_bad)


def test_refusals_leave_out_untouched(ops, beams):
    b, _, _ = beams(dr.Geometry(4, 1, 64), torch.bfloat16)
    H, KV, hd = b.geom
    dev = lambda t: t.to(DEV)  # noqa: E731
    out = torch.full((len(b.np_), H * hd), math.nan, dtype=b.dtype, device=DEV)
    keys = b.cap_p + min(b.cap_b, b.ld_anc)
    ws = nan_ws(ops, len(b.np_), b.geom, keys, b.span)
    args = ops._beam_args("attn_decode_beam_split", dev(b.qkv), dev(b.pk), dev(b.pv), dev(b.bk), dev(b.bv), dev(b.prompt_slot), dev(b.prompt_len),
                          dev(b.gen_len), dev(b.anc), out, None, H, KV, hd, None)
    lib, code, stream = ops._lib.load(), ops.dtype_code(b.dtype), ops.stream_ptr()
    ok = -(-keys // b.span)
    for span, n_splits, ptr, nbytes in ((0, ok, ws.data_ptr(), 1 << 40), (b.span + 8, ok, ws.data_ptr(), 1 << 40), (b.span, 0, ws.data_ptr(), 1 << 40),
                                        (b.span, 65536, ws.data_ptr(), 1 << 40), (b.span, ok - 1, ws.data_ptr(), ws.numel() * 4),
                                        (b.span, ok, None, ws.numel() * 4), (b.span, ok, ws.data_ptr() + 4, ws.numel() * 4),
                                        (b.span, ok, ws.data_ptr(), ws.numel() * 4 - 4)):
        assert lib.ssi_attn_decode_beam_split(*args, span, n_splits, ptr, nbytes, code, stream) == 1, (span, n_splits)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out.float()).all())
    assert lib.ssi_attn_decode_beam_split(*args, b.span, ok, ws.data_ptr(), ws.numel() * 4, code, stream) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all())
