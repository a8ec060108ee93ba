"""``ssi_decode_select`` on the GPU against the float64 reference of tests/decode_select_ref.py: ``token`` and ``rank`` EXACTLY, ``logprob``
within the bound derived there — both dtypes, every vocabulary edge of the 16-byte vectors and the 32-bit mask words and the flagship head's
(133 258 of 133 376), 1 / 3 / 257 rows, every mask kind, pad columns holding NaN and +inf, planted ties across lanes, waves and the vector /
tail boundary, forbidden maxima, rows around ``min_new``, degenerate rows, and the same row at three places.

Measured on the MI355X (worst ``logprob`` error / bound over all cases, printed at module end): 0.612 in bf16, 0.624 in fp32."""
import pytest
import torch

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
        print(f"\ndecode-select worst logprob error/bound  {k:<6s} {_WORST[k]:.4f}", end="")
    print()


def _dev(t):
    return None if t is None else t.to(DEV)


def select(x_dev, vocab, allow=None, early=None, n_gen=None, min_new=0, logprob=True, rank=True):
    from ssi import ops
    rows = x_dev.shape[0]
    tok = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    lp = torch.full((rows,), 7.0, dtype=torch.float32, device=DEV) if logprob else None
    rk = torch.full((rows,), -7, dtype=torch.int32, device=DEV) if rank else None
    ops.decode_select(x_dev, vocab, tok, lp, rk, allow=_dev(D.pack(allow)), allow_early=_dev(D.pack(early)), n_generated=_dev(n_gen),
                      min_new=min_new)
    return tok, lp, rk


def check(x_dev, base, dtype, what, **kw):
    got = select(x_dev, base.vocab, **kw)
    bad_tok, bad_rank, ratio, misses = D.judge(got, base.expected(**kw))
    key = "bf16" if dtype == BF16 else "fp32"
    _WORST[key] = max(_WORST.get(key, 0.0), ratio)
    print(f"{what}: logprob err/bound {ratio:.4f}")
    assert bad_tok == 0 and bad_rank == 0, f"{what}: {bad_tok} tokens and {bad_rank} ranks differ"
    assert misses == 0, f"{what}: {misses} logprobs outside the bound (worst {ratio:.3f} x)"
    return got


# every vocabulary at 3 rows; 1 and 257 rows where a reference of 257 rows is small
SHAPES = [(v, 3) for v in D.VOCABS] + [(v, r) for v in (33, 515, 2049) for r in (1, 257)]


@DTYPES
@pytest.mark.parametrize("vocab,rows", SHAPES, ids=[f"{v}x{r}" for v, r in SHAPES])
def test_every_mask_at_every_shape(vocab, rows, dtype):
    x = D.make_logits(rows, vocab, D.ld_of(vocab), dtype, seed=vocab + rows)
    base, x_dev = D.Base(x, vocab), x.to(DEV)
    for kind in D.MASK_KINDS:
        if not D.mask_exists(kind, vocab):
            continue
        tok, lp, rk = check(x_dev, base, dtype, f"{vocab}x{rows} {kind}", allow=D.make_mask(kind, vocab))
        if kind == "empty":
            assert tok.tolist() == [-1] * rows and lp.tolist() == [0.0] * rows and rk.tolist() == [-1] * rows
    assert torch.equal(x_dev.cpu().view(torch.int16 if dtype == BF16 else torch.int32),
                       x.view(torch.int16 if dtype == BF16 else torch.int32))                       # the logits are read only


@DTYPES
def test_rows_that_are_not_16_byte_aligned(dtype):
    vocab, ld = 515, 517
    x = D.make_logits(5, vocab, ld, dtype, seed=3)
    assert not D.vec_ok(ld, dtype)
    base, x_dev = D.Base(x, vocab), x.to(DEV)
    for kind in ("null", "alternating", "bitlast"):
        check(x_dev, base, dtype, f"unaligned {kind}", allow=D.make_mask(kind, vocab))
    view = x.to(DEV)[:, 1:]                                   # ld aligned or not, the base pointer is not
    check(view, D.Base(x[:, 1:], vocab - 1, vec=False), dtype, "offset base", allow=D.make_mask("alternating", vocab - 1))


@DTYPES
def test_equal_maxima_across_lanes_waves_and_the_tail(dtype):
    x, settings = D.tie_case(dtype)
    base, x_dev = D.Base(x, D.PLANT_VOCAB), x.to(DEV)
    allow, want, rank = settings[0]
    tok, _, rk = check(x_dev, base, dtype, "ties, all allowed", allow=allow)
    assert torch.equal(tok.cpu(), want) and torch.equal(rk.cpu().long(), rank)
    for allow, (i, want, rank) in settings[1:]:
        tok, _, rk = check(x_dev, base, dtype, f"ties, row {i} wants {want}", allow=allow)
        assert int(tok[i]) == want and int(rk[i]) == rank


@DTYPES
def test_the_maximum_on_forbidden_columns_gives_the_planted_rank(dtype):
    x, allow = D.forbidden_max_case(dtype)
    base, x_dev = D.Base(x, D.PLANT_VOCAB), x.to(DEV)
    _, _, rk = check(x_dev, base, dtype, "forbidden maxima", allow=allow)
    assert rk.tolist() == [D.PLANT_COUNT] * 4
    _, _, rk = check(x_dev, base, dtype, "forbidden maxima, unconstrained")
    assert rk.tolist() == [0] * 4
    tok, lp, rk = select(x_dev, D.PLANT_VOCAB, allow=allow, logprob=False, rank=False)          # both optional outputs NULL
    assert lp is None and rk is None and torch.equal(tok.cpu(), base.expected(allow)[0])


@DTYPES
def test_rows_around_min_new_take_the_early_mask(dtype):
    x, allow, early, n_gen, min_new = D.min_new_case(dtype)
    base, x_dev = D.Base(x, 515), x.to(DEV)
    tok, _, rk = check(x_dev, base, dtype, "min_new", allow=allow, early=early, n_gen=n_gen, min_new=min_new)
    assert [int(t) == 77 for t in tok] == [False, True, False, True]         # n_generated = min_new - 1, min_new, 0, 1000
    tok, _, _ = check(x_dev, base, dtype, "min_new 0", allow=allow, early=early, n_gen=torch.zeros(4, dtype=torch.int32), min_new=0)
    assert tok.tolist() == [77] * 4
    tok, _, _ = check(x_dev, base, dtype, "no n_generated", allow=allow, early=early, n_gen=None, min_new=min_new)
    assert tok.tolist() == [77] * 4
    check(x_dev, base, dtype, "early NULL", allow=allow, early=None, n_gen=n_gen, min_new=min_new)   # a NULL early mask: every column


@DTYPES
def test_degenerate_rows_still_give_an_allowed_token(dtype):
    vocab = 515
    x = D.make_logits(4, vocab, D.ld_of(vocab), F32, seed=31)
    allow = D.make_mask("block", vocab)
    x[0, :vocab] = torch.where(allow, torch.tensor(-float("inf")), x[0, :vocab])    # -inf everywhere allowed
    x[1, :vocab] = float("nan")                                                       # a NaN row
    x[2, :vocab] = -float("inf")
    x[3, 5:vocab:7] = float("nan")                                                    # NaN here and there
    tok, _, _ = select(x.to(dtype).to(DEV), vocab, allow=allow)
    for t in tok.tolist():
        assert t == -1 or (0 <= t < vocab and bool(allow[t])), tok.tolist()
    tok, _, _ = select(x.to(dtype).to(DEV), vocab, allow=D.make_mask("empty", vocab))
    assert tok.tolist() == [-1] * 4


@DTYPES
def test_a_rows_result_does_not_depend_on_its_place(dtype):
    vocab, rows = 2049, 257
    x = D.make_logits(rows, vocab, D.ld_of(vocab), dtype, seed=41)
    x[100], x[256] = x[0], x[0]
    allow = D.make_mask("complement", vocab)
    tok, lp, rk = select(x.to(DEV), vocab, allow=allow)
    one = select(x[:1].to(DEV), vocab, allow=allow)
    bits, one_bits = lp.view(torch.int32).tolist(), one[1].view(torch.int32).tolist()
    for r in (100, 256):
        assert int(tok[r]) == int(tok[0]) and int(rk[r]) == int(rk[0]) and bits[r] == bits[0]
    assert int(one[0][0]) == int(tok[0]) and one_bits[0] == bits[0] and int(one[2][0]) == int(rk[0])


def test_argument_errors_and_the_empty_launch():
    from ssi import _lib
    lib = _lib.load()
    x = torch.zeros(2, 40, device=DEV)
    tok = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    p, t = x.data_ptr(), tok.data_ptr()

    def call(logits=p, ld=40, rows=2, vocab=33, min_new=0, token=t):
        return lib.ssi_decode_select(logits, ld, rows, vocab, None, None, None, min_new, token, None, None, _lib.SSI_F32, _lib.stream_ptr())

    for kw in (dict(logits=None), dict(token=None), dict(vocab=0), dict(ld=32), dict(vocab=2 ** 31, ld=2 ** 31), dict(min_new=-1)):
        assert call(**kw) == 1, kw                            # SSI_ERR_ARG
    assert call(rows=0) == 0
    torch.cuda.synchronize()
    assert tok.tolist() == [-7, -7]                           # nothing was launched
    assert call() == 0
    assert tok.tolist() == [0, 0]
