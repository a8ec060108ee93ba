"""``ssi_attn_decode_beam`` on the GPU: single-query attention over a prompt cache slot and, behind it, a beam cache read through an ancestry
table.  Two yardsticks per launch, for bf16 and fp32 and the four query-head register counts (G = 1, 2, 4, 8) at head_dim 16, 64, 128:

* BITS: out and lse ``torch.equal`` to ``ops.attn_decode`` on a cache in which every row's keys were materialised one behind the other (the
  two kernels share the row body; the walk is over the concatenated key index);
* float64: the checker and the bound of ``decode_ref.py`` (C = 1.8e-5 of the largest |v|, 2^-8 relative for bf16 stores, C_LSE).

Rows: every pairing of prompt_len in {0, 1, chunk - 1, chunk, chunk + 1, round - 1, round, round + 1} with gen_len in {0, 1, 5, chunk - 1,
chunk + 1, round + 1} (``decode_ref.chunk_edges``: a chunk is what one wave takes, a round what the four take), so the prompt / generated
boundary falls inside a chunk, on its edge and one off it.  The rows of one prompt_len share a prompt slot; the ancestry is a simulated
beam history (every step each row adopts a random row of its group), so rows share prefixes and point at other rows' slots.  Neither slot
numbering is the identity.  NaN sits in every prompt-cache and beam-cache position no row may read (beyond a prompt's length, positions no
ancestry names, spare slots), and the pad columns of ``anc`` hold an index far outside the cache: read, it would be counted."""
import math

import pytest
import torch

import decode_ref as dr

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = (torch.bfloat16, torch.float32)
GEOMS = (dr.Geometry(8, 1, 16), dr.Geometry(4, 1, 64), dr.Geometry(4, 2, 64), dr.Geometry(2, 2, 128))     # G = 8, 4, 2, 1
FAR = 1 << 30
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


class Beam:
    """One launch and the materialised problem it must equal."""

    def __init__(self, geom, dtype, seed=3):
        H, KV, hd = geom
        _, chunk, rnd = dr.chunk_edges(hd, dtype)
        p_lens = [0, 1, chunk - 1, chunk, chunk + 1, rnd - 1, rnd, rnd + 1]
        g_lens = [0, 1, 5, chunk - 1, chunk + 1, rnd + 1]
        pairs = [(a, b) for a in p_lens for b in g_lens]
        self.geom, self.dtype, rows = geom, dtype, len(pairs)
        self.np_, self.ng = [a for a, _ in pairs], [b for _, b in pairs]
        g = torch.Generator().manual_seed(seed)
        T = max(g_lens)
        self.cap_p, self.cap_b, self.ld_anc = max(p_lens) + 2, T + 1, T + 3
        # keys and queries from decode_ref's "spread" case (a uniform score offset per key moves the softmax), one contiguous run per row
        base = dr.make_problem(geom, dtype, [a + b for a, b in pairs], "spread", max(p_lens) + T, seed, poison=False, spare_slots=0)
        self.qkv = base.qkv
        n_prompts = len(p_lens)
        pperm = torch.randperm(n_prompts + 1, generator=g).roll(1)             # prompt slot of prompt q; one slot is spare
        bperm = torch.randperm(rows + 2, generator=g).roll(1)                  # beam slot of row r; two are spare
        self.prompt_of = [p_lens.index(a) for a in self.np_]
        self.prompt_slot = torch.tensor([int(pperm[q]) for q in self.prompt_of], dtype=torch.int32)
        width = KV * hd
        nan = float("nan")
        self.pk, self.pv = torch.full((n_prompts + 1, self.cap_p, width), nan).to(dtype), torch.full((n_prompts + 1, self.cap_p, width), nan).to(dtype)
        self.bk, self.bv = torch.full((rows + 2, self.cap_b, width), nan).to(dtype), torch.full((rows + 2, self.cap_b, width), nan).to(dtype)
        anc = torch.full((rows, self.ld_anc), FAR, dtype=torch.int32)
        for q in range(n_prompts):                                             # a beam history per group of rows
            group = [r for r in range(rows) if self.prompt_of[r] == q]
            a = torch.zeros(len(group), T, dtype=torch.int32)
            for i in range(T):
                a = a[torch.randint(0, len(group), (len(group),), generator=g)]
                a[:, i] = torch.tensor([int(bperm[r]) for r in group], dtype=torch.int32)
            for j, r in enumerate(group):
                anc[r, :T] = a[j]
            r0 = group[0]                                                      # the prompt's keys: those of the group's first row
            s0 = int(base.slot[r0])
            self.pk[int(pperm[q]), :p_lens[q]] = base.k_cache[s0, :p_lens[q]]
            self.pv[int(pperm[q]), :p_lens[q]] = base.v_cache[s0, :p_lens[q]]
        self.anc = anc
        for r in range(rows):                                                  # a generated position: the keys of the first row that names it
            s = int(base.slot[r])
            for i in range(self.ng[r]):
                a = int(anc[r, i])
                if bool(torch.isnan(self.bk[a, i, 0].float())):
                    self.bk[a, i], self.bv[a, i] = base.k_cache[s, self.np_[r] + i], base.v_cache[s, self.np_[r] + i]
        self.prompt_len = torch.tensor(self.np_, dtype=torch.int32)
        self.gen_len = torch.tensor(self.ng, dtype=torch.int32)

    def materialised(self, skip=lambda r, j: False) -> dr.Problem:
        """Every row's keys one behind the other in a slot of its own (``skip(r, j)``: the concatenated key j of row r is left out)."""
        rows, width = len(self.np_), self.pk.shape[2]
        cap = max(a + b for a, b in zip(self.np_, self.ng)) + 1
        kc, vc = torch.full((rows, cap, width), float("nan")).to(self.dtype), torch.full((rows, cap, width), float("nan")).to(self.dtype)
        lens = []
        for r in range(rows):
            keys = [(self.pk, self.pv, int(self.prompt_slot[r]), j) for j in range(self.np_[r])]
            keys += [(self.bk, self.bv, int(self.anc[r, i]), i) for i in range(self.ng[r])]
            keys = [k for j, k in enumerate(keys) if not skip(r, j)]
            for j, (ck, cv, s, at) in enumerate(keys):
                kc[r, j], vc[r, j] = ck[s, at], cv[s, at]
            lens.append(len(keys))
        slot = torch.arange(rows, dtype=torch.int32)
        return dr.Problem(self.geom, self.dtype, self.qkv, kc, vc, slot, torch.tensor(lens, dtype=torch.int32), "spread")


def launch(ops, b: Beam, rows=None, prompt_slot=None, anc=None, with_lse=True, n_bad=None):
    H, KV, hd = b.geom
    sel = slice(None) if rows is None else rows
    dev = lambda t: t.to(DEV)[sel].contiguous()  # noqa: E731
    qkv = b.qkv.to(DEV)[sel]
    n = qkv.shape[0]
    out = torch.full((n, H * hd), math.nan, dtype=b.dtype, device=DEV)
    lse = torch.full((n, H), math.nan, dtype=torch.float32, device=DEV) if with_lse else None
    ops.attn_decode_beam(qkv, b.pk.to(DEV), b.pv.to(DEV), b.bk.to(DEV), b.bv.to(DEV), dev(b.prompt_slot if prompt_slot is None else prompt_slot),
                         dev(b.prompt_len), dev(b.gen_len), dev(b.anc if anc is None else anc), out, lse, H, KV, hd, n_bad=n_bad)
    torch.cuda.synchronize()
    return out, lse


def contiguous(ops, p: dr.Problem):
    H, KV, hd = p.geom
    out = torch.full((p.rows, H * hd), math.nan, dtype=p.dtype, device=DEV)
    lse = torch.full((p.rows, H), math.nan, dtype=torch.float32, device=DEV)
    ops.attn_decode(p.qkv.to(DEV), p.k_cache.to(DEV), p.v_cache.to(DEV), p.slot.to(DEV), p.kv_len.to(DEV), out, lse, H, KV, hd)
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
def test_bit_equal_to_the_contiguous_kernel_and_within_the_bound(ops, beams, geom, dtype):
    b, p, ref = beams(geom, dtype)
    assert not bool((b.prompt_slot == torch.tensor(b.prompt_of)).all())                           # neither numbering is the identity
    assert len(set(b.prompt_slot.tolist())) < len(b.np_)                                           # rows share prompt slots
    assert any(int(b.anc[r, i]) != int(b.anc[r, b.ng[r] - 1]) for r in range(len(b.ng)) for i in range(b.ng[r]))   # ... and read other rows' slots
    n_bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, lse = launch(ops, b, n_bad=n_bad)
    want_out, want_lse = contiguous(ops, p)
    assert torch.equal(out, want_out) and torch.equal(lse, want_lse)
    assert int(n_bad) == 0                                                                          # (the pad columns of anc were not read)
    assert dr.violations(out, lse, p, ref) == []
    assert int(ref.dead.sum()) == 1                                                                 # the row without any key
    live = ~ref.dead
    ratio = ((out.cpu().double() - ref.out).abs() / dr.tolerance(p, ref))[live].max()
    lratio = (lse.cpu().double() - ref.lse)[live].abs().max() / dr.C_LSE
    w = WORST.setdefault(_name(dtype), [0.0, 0.0])
    w[0], w[1] = max(w[0], float(ratio)), max(w[1], float(lratio))
    out2, _ = launch(ops, b, with_lse=False)                                                        # no counter, no lse: both may be NULL
    assert torch.equal(out2, out)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_a_negative_prompt_slot_gives_a_zero_row(ops, beams, dtype):
    b, p, ref = beams(dr.Geometry(4, 1, 64), dtype)
    clean, clean_lse = launch(ops, b)
    off = [5, 17, 40]
    slot = b.prompt_slot.clone()
    slot[off] = torch.tensor([-1, -7, -(1 << 30)], dtype=torch.int32)
    n_bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, lse = launch(ops, b, prompt_slot=slot, n_bad=n_bad)
    assert bool((out[off] == 0).all()) and bool((lse[off] == -math.inf).all()) and int(n_bad) == 0
    keep = [r for r in range(len(b.np_)) if r not in off]
    assert torch.equal(out[keep], clean[keep]) and torch.equal(lse[keep], clean_lse[keep])


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_indices_outside_a_cache_are_counted_and_never_read(ops, beams, dtype):
    """A prompt slot at or beyond n_pslots drops the row's prompt keys, an ancestry entry outside [0, n_bslots) drops that key; the row is
    counted once however many of its keys were dropped, and what is left is the attention over the remaining keys (float64 checker)."""
    b, p, ref = beams(dr.Geometry(4, 1, 64), dtype)
    clean, clean_lse = launch(ops, b)
    rows = len(b.np_)
    slot, anc = b.prompt_slot.clone(), b.anc.clone()
    n_ps, n_bs = b.pk.shape[0], b.bk.shape[0]
    by = {(a, g): r for r, (a, g) in enumerate(zip(b.np_, b.ng))}
    chunk = dr.chunk_edges(64, dtype)[1]
    r_slot, r_slot_far, r_only_prompt = by[(chunk + 1, 5)], by[(chunk, chunk + 1)], by[(1, 0)]
    slot[r_slot], slot[r_slot_far], slot[r_only_prompt] = n_ps, n_ps + 12345, n_ps       # (the last: every key dropped -> zeros, -inf)
    r_anc, r_anc_neg, r_anc_two = by[(chunk - 1, 5)], by[(0, chunk + 1)], by[(1, chunk + 1)]
    anc[r_anc, 2] = n_bs
    anc[r_anc_neg, 0] = -1
    anc[r_anc_two, 1], anc[r_anc_two, 3] = FAR, -(1 << 31)
    touched = {r_slot, r_slot_far, r_only_prompt, r_anc, r_anc_neg, r_anc_two}

    def skip(r, j):
        if r in (r_slot, r_slot_far, r_only_prompt):
            return j < b.np_[r]
        i = j - b.np_[r]
        return (r == r_anc and i == 2) or (r == r_anc_neg and i == 0) or (r == r_anc_two and i in (1, 3))

    # the dropped entries must not be looked up by the reference either
    b2 = Beam.__new__(Beam)
    b2.__dict__.update(b.__dict__)
    b2.prompt_slot = torch.where(slot >= n_ps, torch.zeros_like(slot), slot)
    b2.anc = torch.where((anc < 0) | (anc >= n_bs), torch.zeros_like(anc), anc)
    p2 = b2.materialised(skip)
    n_bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, lse = launch(ops, b, prompt_slot=slot, anc=anc, n_bad=n_bad)
    assert int(n_bad) == len(touched)
    ref2 = dr.exact(p2)
    assert bool(ref2.dead[r_only_prompt]) and int(ref2.dead.sum()) == 2
    assert dr.violations(out, lse, p2, ref2) == []
    keep = [r for r in range(rows) if r not in touched]
    assert torch.equal(out[keep], clean[keep]) and torch.equal(lse[keep], clean_lse[keep])
    out3, _ = launch(ops, b, prompt_slot=slot, anc=anc, with_lse=False)                  # without a counter the keys are dropped all the same
    assert torch.equal(out3, out)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_a_rows_bits_do_not_depend_on_other_rows(ops, beams, dtype):
    b, p, ref = beams(dr.Geometry(8, 1, 16), dtype)
    out, lse = launch(ops, b)
    longest = max(range(len(b.np_)), key=lambda r: b.np_[r] + b.ng[r])
    for r in sorted({1, 7, longest}):
        o1, l1 = launch(ops, b, rows=slice(r, r + 1))
        assert torch.equal(o1[0], out[r]) and torch.equal(l1[0], lse[r]), r
    idx = torch.tensor([longest, 3, 30, 1])
    o4, l4 = launch(ops, b, rows=idx.to(DEV))
    assert torch.equal(o4, out[idx.to(DEV)]) and torch.equal(l4, lse[idx.to(DEV)])
    # other rows' queries change: this row's bits stay
    b3 = Beam.__new__(Beam)
    b3.__dict__.update(b.__dict__)
    b3.qkv = b.qkv.clone()
    b3.qkv[torch.arange(len(b.np_)) != longest] *= -0.5
    o5, l5 = launch(ops, b3)
    assert torch.equal(o5[longest], out[longest]) and torch.equal(l5[longest], lse[longest])
    assert not torch.equal(o5[30], out[30])                                               # (a row of many keys: its own query did change it)


@pytest.mark.parametrize("geom", (dr.Geometry(4, 1, 12), dr.Geometry(16, 1, 16), dr.Geometry(2, 1, 136)), ids=str)
def test_other_geometries_are_refused(ops, geom):
    H, KV, hd = geom
    qkv = torch.zeros(2, (H + 2 * KV) * hd, dtype=torch.float32, device=DEV)
    cache = torch.zeros(2, 4, KV * hd, dtype=torch.float32, device=DEV)
    i32 = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="code 2"):
        ops.attn_decode_beam(qkv, cache, cache.clone(), cache.clone(), cache.clone(), i32, i32, i32, torch.zeros(2, 4, dtype=torch.int32, device=DEV),
                             torch.zeros(2, H * hd, device=DEV), None, H, KV, hd)
