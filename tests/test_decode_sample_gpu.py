"""``ssi_decode_sample`` on the GPU against the float64 sampler of tests/decode_sample_ref.py: ``token`` and ``n_kept`` EXACTLY (an ambiguous
top-p boundary may take either neighbour, with that set's draw), ``logprob`` within ``ssi_decode_select``'s derived bound — both dtypes, the
vocabularies 1 .. 2049 and the flagship head's, 1 / 3 / 257 rows, every (top_k, top_p) pair with the temperatures and the mask kinds in turn;
row independence; planted rows; the C-level refusals.

Measured on the MI355X (worst ``logprob`` error / bound over all cases, printed at module end): 0.559 in bf16, 0.559 in fp32; no committed row is
ambiguous at its top-p boundary."""
import pytest
import torch

import decode_sample_ref as S
import decode_select_ref as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", (BF16, F32), ids=("bf16", "fp32"))
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(_WORST):
        print(f"\ndecode-sample worst logprob error/bound  {k:<6s} {_WORST[k]:.4f}", end="")
    print()


def _dev(t):
    return None if t is None else t.to(DEV)


def sample(x_dev, vocab, seqs, *, T, top_k=-1, top_p=1.0, seed, step, allow=None, early=None, n_gen=None, min_new=0, logprob=True, kept=True):
    from ssi import ops
    rows = x_dev.shape[0]
    tok = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    lp = torch.full((rows,), 7.0, dtype=torch.float32, device=DEV) if logprob else None
    nk = torch.full((rows,), -7, dtype=torch.int32, device=DEV) if kept else None
    ops.decode_sample(x_dev, vocab, tok, lp, nk, temperature=T, top_k=top_k, top_p=top_p, seed=seed, step=step,
                      sequence=S.seq_words(seqs).to(DEV), allow=_dev(D.pack(allow)), allow_early=_dev(D.pack(early)), n_generated=_dev(n_gen),
                      min_new=min_new)
    return tok, lp, nk


def check(x_dev, case, exp, dtype, what, **kw):
    got = sample(x_dev, case.vocab, case.seqs, seed=case.seed, step=case.step, **kw)
    bad_tok, bad_kept, ratio, misses = S.judge(got, case, exp)
    key = "bf16" if dtype == BF16 else "fp32"
    _WORST[key] = max(_WORST.get(key, 0.0), ratio)
    print(f"{what}: logprob err/bound {ratio:.4f}, ambiguous rows {int(exp.ambiguous.sum())}")
    assert bad_tok == 0 and bad_kept == 0, f"{what}: {bad_tok} tokens and {bad_kept} n_kept differ"
    assert misses == 0, f"{what}: {misses} logprobs outside the bound (worst {ratio:.3f} x)"
    return got


@DTYPES
@pytest.mark.parametrize("vocab,rows", S.SHAPES, ids=[f"{v}x{r}" for v, r in S.SHAPES])
def test_every_setting_at_every_shape(vocab, rows, dtype):
    case, found = S.case(vocab, rows, dtype)
    x_dev = case.x.to(DEV)
    for s, allow, exp in found:
        tok, lp, nk = check(x_dev, case, exp, dtype, f"{vocab}x{rows} T={s['T']} k={s['top_k']} p={s['top_p']} {s['kind']}", T=s["T"],
                            top_k=s["top_k"], top_p=s["top_p"], allow=allow)
        if s["kind"] == "empty":
            assert tok.tolist() == [-1] * rows and lp.tolist() == [0.0] * rows and nk.tolist() == [-1] * rows
    bits = torch.int16 if dtype == BF16 else torch.int32
    assert torch.equal(x_dev.cpu().view(bits), case.x.view(bits))                                 # the logits are read only


@DTYPES
def test_rows_that_are_not_16_byte_aligned_and_rows_around_min_new(dtype):
    vocab, ld = 515, 517
    x = D.make_logits(5, vocab, ld, dtype, seed=3)
    assert not D.vec_ok(ld, dtype)
    case = S.Case(x, vocab, seqs=torch.arange(5) + 40, seed=9, step=2)
    for kind, k, p in (("null", 50, 0.9), ("alternating", -1, 0.5), ("bitlast", 2, 1.0)):
        allow, M = S.masks_of(kind, vocab, 5)
        exp = case.expected(M, 0.7, k, p)
        assert exp.margin_ok.all() and not exp.ambiguous.any()
        check(x.to(DEV), case, exp, dtype, f"unaligned {kind}", T=0.7, top_k=k, top_p=p, allow=allow)
    x, allow, early, n_gen, min_new = D.min_new_case(dtype)
    case = S.Case(x, 515, seqs=torch.arange(4), seed=10, step=0)
    M = D.row_masks(4, 515, allow, early, n_gen, min_new).numpy()
    exp = case.expected(M, 1.0, 1, 1.0)
    tok, _, _ = check(x.to(DEV), case, exp, dtype, "min_new", T=1.0, top_k=1, allow=allow, early=early, n_gen=n_gen, min_new=min_new)
    assert [int(t) == 77 for t in tok] == [False, True, False, True]
    exp = case.expected(M, 1.3, 50, 0.9)
    assert exp.margin_ok.all() and not exp.ambiguous.any()
    check(x.to(DEV), case, exp, dtype, "min_new sampled", T=1.3, top_k=50, top_p=0.9, allow=allow, early=early, n_gen=n_gen, min_new=min_new)


@DTYPES
def test_row_independence_and_what_the_random_bits_depend_on(dtype):
    vocab, rows = 2049, 257
    case, found = S.case(vocab, rows, dtype)
    s, allow, _ = found[13]                                       # top_k = 50 with top_p = 0.9
    assert s["top_k"] == 50 and s["top_p"] == 0.9
    kw = dict(T=s["T"], top_k=s["top_k"], top_p=s["top_p"], allow=allow)
    x_dev = case.x.to(DEV)
    first = sample(x_dev, vocab, case.seqs, seed=case.seed, step=case.step, **kw)
    again = sample(x_dev, vocab, case.seqs, seed=case.seed, step=case.step, **kw)
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(1))
    moved = sample(case.x[perm].to(DEV), vocab, case.seqs[perm], seed=case.seed, step=case.step, **kw)
    for a, b, c in zip(first, again, moved):
        bits = torch.int32 if a.dtype == torch.float32 else a.dtype
        assert torch.equal(a.view(bits), b.view(bits))                                           # a second launch: bit for bit
        assert torch.equal(a.view(bits)[perm.to(DEV)], c.view(bits))                             # permuted rows: permuted outputs
    one = sample(case.x[100:101].to(DEV), vocab, case.seqs[100:101], seed=case.seed, step=case.step, **kw)
    assert int(one[0][0]) == int(first[0][100]) and int(one[2][0]) == int(first[2][100])
    assert one[1].view(torch.int32).tolist() == first[1][100:101].view(torch.int32).tolist()
    plain = dict(T=1.0)                                            # (over the whole row: a change of the bits moves many rows)
    base = sample(x_dev, vocab, case.seqs, seed=case.seed, step=case.step, **plain)[0]
    for other in (dict(seed=case.seed + 1, step=case.step, seqs=case.seqs), dict(seed=case.seed + (1 << 32), step=case.step, seqs=case.seqs),
                  dict(seed=case.seed, step=case.step + 1, seqs=case.seqs), dict(seed=case.seed, step=case.step, seqs=case.seqs + 1)):
        tok = sample(x_dev, vocab, other.pop("seqs"), **other, **plain)[0]
        assert not torch.equal(tok, base), other


@DTYPES
def test_planted_rows(dtype):
    vocab = 515
    x = D.make_logits(5, vocab, D.ld_of(vocab), F32, seed=31)
    allow = D.make_mask("block", vocab)
    x[0, :vocab] = torch.where(allow, torch.tensor(-float("inf")), x[0, :vocab])    # -inf everywhere allowed
    x[1, :vocab] = float("nan")                                                       # a NaN row
    x[2, :vocab] = -float("inf")                                                      # a row of -inf
    x[3, 5:vocab:7] = float("nan")                                                    # NaN in allowed columns here and there
    x[4, 3:vocab:5] = -float("inf")
    x = x.to(dtype)
    case = S.Case(x, vocab, seqs=torch.arange(5) + 7, seed=77, step=3)
    M = D.row_masks(5, vocab, allow, None, None, 0).numpy()
    first = int(torch.nonzero(allow)[0])
    for T, k, p in ((1.0, -1, 1.0), (0.7, 50, 1.0), (1.3, -1, 0.9), (1.0, 50, 0.5)):
        exp = case.expected(M, T, k, p)
        assert exp.margin_ok.all() and not exp.ambiguous.any()
        tok, _, nk = sample(x.to(DEV), vocab, case.seqs, T=T, top_k=k, top_p=p, seed=77, step=3, allow=allow)
        assert tok.tolist() == exp.token.tolist() and nk.tolist() == exp.n_kept.tolist(), (T, k, p)
        assert tok.tolist()[:3] == [first] * 3 and nk.tolist()[:3] == [1] * 3
        for r in (3, 4):
            assert bool(torch.isfinite(x[r, int(tok[r])].float()))                    # a NaN or -inf column is never drawn
    tok, lp, nk = sample(x.to(DEV), vocab, case.seqs, T=1.0, seed=77, step=3, allow=D.make_mask("empty", vocab))
    assert tok.tolist() == [-1] * 5 and lp.tolist() == [0.0] * 5 and nk.tolist() == [-1] * 5
    tok, lp, nk = sample(x.to(DEV), vocab, case.seqs, T=1.0, seed=77, step=3, allow=allow, logprob=False, kept=False)
    assert lp is None and nk is None and tok.tolist() == case.expected(M, 1.0, -1, 1.0).token.tolist()


@DTYPES
def test_top_k_1_is_decode_selects_token(dtype):
    from ssi import ops
    vocab, rows = 2049, 257
    case, _ = S.case(vocab, rows, dtype)
    allow = D.make_mask("complement", vocab)
    x_dev = case.x.to(DEV)
    tok, lp, nk = sample(x_dev, vocab, case.seqs, T=0.7, top_k=1, seed=1, step=0, allow=allow)
    want, want_lp = torch.empty_like(tok), torch.empty_like(lp)
    ops.decode_select(x_dev, vocab, want, want_lp, None, allow=D.pack(allow).to(DEV))
    # (ties at the threshold stay: where the allowed maximum occurs twice the draw is among its columns, so only the VALUE is select's)
    assert torch.equal(case.x.to(DEV)[torch.arange(rows), tok], case.x.to(DEV)[torch.arange(rows), want])
    assert torch.equal(lp.view(torch.int32), want_lp.view(torch.int32))
    single = nk == 1
    assert bool(single.any()) and torch.equal(tok[single], want[single])


def test_4096_identical_rows_with_distinct_sequences():
    vocab, rows = 8, 4096
    x = D.make_logits(1, vocab, D.ld_of(vocab), F32, seed=5).expand(rows, -1).contiguous()
    case = S.Case(x, vocab, seqs=torch.arange(rows), seed=123456789012345, step=11)
    M = torch.ones(rows, vocab, dtype=torch.bool).numpy()
    exp = case.expected(M, 1.0, -1, 1.0)
    assert exp.margin_ok.all()
    tok, _, nk = sample(x.to(DEV), vocab, case.seqs, T=1.0, seed=case.seed, step=case.step)
    assert tok.tolist() == exp.token.tolist() and nk.tolist() == [vocab] * rows
    assert len(set(tok.tolist())) > 3                               # the rows differ by their sequences alone


def test_argument_errors_and_the_empty_launch():
    from ssi import _lib
    lib = _lib.load()
    x = torch.zeros(2, 40, device=DEV)
    tok = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    seq = torch.zeros(2, dtype=torch.int32, device=DEV)
    p, t, q = x.data_ptr(), tok.data_ptr(), seq.data_ptr()

    def call(logits=p, ld=40, rows=2, vocab=33, min_new=0, token=t, T=1.0, top_k=-1, top_p=1.0, sequence=q):
        return lib.ssi_decode_sample(logits, ld, rows, vocab, None, None, None, min_new, T, top_k, top_p, 0, 0, sequence, token, None, None,
                                     _lib.SSI_F32, _lib.stream_ptr())

    for kw in (dict(logits=None), dict(token=None), dict(vocab=0), dict(ld=32), dict(vocab=2 ** 31, ld=2 ** 31), dict(min_new=-1),
               dict(T=0.0), dict(T=-1.0), dict(T=float("inf")), dict(T=float("nan")), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")),
               dict(sequence=None)):
        assert call(**kw) == 1, kw                            # SSI_ERR_ARG
    assert call(rows=0) == 0
    torch.cuda.synchronize()
    assert tok.tolist() == [-7, -7]                           # nothing was launched, nothing written
    assert call() == 0
    assert all(0 <= v < 33 for v in tok.tolist())
