"""The checker of ``ssi_decode_select`` (tests/decode_select_ref.py) held against itself on the CPU: the fp32 restatement of the kernel gives
the reference's tokens and ranks and stays inside the derived ``logprob`` bound on every case the GPU test runs, and each planted defect of
the restatement is caught by that same judgement."""
import pytest
import torch

import decode_select_ref as D

BF16, F32 = torch.bfloat16, torch.float32
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(_WORST):
        print(f"\ndecode-select restatement worst logprob error/bound  {k:<6s} {_WORST[k]:.4f}", end="")
    print()


def _run(x, vocab, allow=None, early=None, n_gen=None, min_new=0, mutant=None, base=None):
    base = base or D.Base(x, vocab)
    got = D.restate(x, vocab, D.pack(allow), D.pack(early), n_gen, min_new, mutant=mutant)
    return D.judge(got, base.expected(allow, early, n_gen, min_new))


def _clean(res, key):
    _WORST[key] = max(_WORST.get(key, 0.0), res[2])
    return res[0] == 0 and res[1] == 0 and res[3] == 0


@pytest.mark.parametrize("dtype", (BF16, F32), ids=("bf16", "fp32"))
@pytest.mark.parametrize("vocab", D.VOCABS)
def test_the_restatement_meets_the_reference_on_every_mask(vocab, dtype):
    x = D.make_logits(3, vocab, D.ld_of(vocab), dtype, seed=vocab)
    base = D.Base(x, vocab)
    for kind in D.MASK_KINDS:
        if D.mask_exists(kind, vocab):
            res = _run(x, vocab, allow=D.make_mask(kind, vocab), base=base)
            assert _clean(res, "bf16" if dtype == BF16 else "fp32"), (kind, res)
    tok, lp, bound, rk = base.expected(D.make_mask("empty", vocab))
    assert tok.tolist() == [-1] * 3 and rk.tolist() == [-1] * 3 and lp.tolist() == [0.0] * 3


@pytest.mark.parametrize("dtype", (BF16, F32), ids=("bf16", "fp32"))
def test_the_restatement_meets_the_reference_on_the_planted_rows(dtype):
    key = "bf16" if dtype == BF16 else "fp32"
    x = D.make_logits(257, 515, 517, dtype, seed=3)          # a row that is not 16-byte aligned: scalar loads throughout
    assert _clean(_run(x, 515, allow=D.make_mask("alternating", 515)), key)
    x, settings = D.tie_case(dtype)
    base = D.Base(x, D.PLANT_VOCAB)
    allow, want, rank = settings[0]
    tok, _, _, rk = base.expected(allow)
    assert torch.equal(tok, want) and torch.equal(rk, rank)
    for allow, (i, want, rank) in settings[1:]:
        tok, _, _, rk = base.expected(allow)
        assert int(tok[i]) == want and int(rk[i]) == rank
        assert _clean(_run(x, D.PLANT_VOCAB, allow=allow, base=base), key)
    x, allow = D.forbidden_max_case(dtype)
    base = D.Base(x, D.PLANT_VOCAB)
    assert base.expected(allow)[3].tolist() == [D.PLANT_COUNT] * 4 and base.expected(None)[3].tolist() == [0] * 4
    assert _clean(_run(x, D.PLANT_VOCAB, allow=allow, base=base), key)
    x, allow, early, n_gen, min_new = D.min_new_case(dtype)
    base = D.Base(x, 515)
    tok, _, _, rk = base.expected(allow, early, n_gen, min_new)
    assert [int(t) == 77 for t in tok] == [False, True, False, True] and [int(r) == 0 for r in rk] == [False, True, False, True]
    assert _clean(_run(x, 515, allow, early, n_gen, min_new, base=base), key)
    assert _clean(_run(x, 515, allow, early, torch.zeros(4, dtype=torch.int32), 0, base=base), key)    # min_new = 0: never early


def test_the_packed_mask_is_bit_c_mod_32_of_word_c_div_32():
    m = torch.zeros(70, dtype=torch.bool)
    m[[0, 31, 32, 69]] = True
    w = D.pack(m).long() & 0xffffffff
    assert w.tolist() == [1 | 1 << 31, 1, 1 << 5]
    from ssi.generate import _mask_words
    for kind in D.MASK_KINDS[1:]:
        for vocab in (1, 33, 515):
            if D.mask_exists(kind, vocab):
                assert torch.equal(_mask_words(D.make_mask(kind, vocab)), D.pack(D.make_mask(kind, vocab))), (kind, vocab)


def _mutant_inputs(mutant):
    """Cases aimed at the defect: (x, vocab, allow, early, n_gen, min_new)."""
    vocab = 515
    x = D.make_logits(4, vocab, D.ld_of(vocab), BF16, seed=21)
    if mutant in ("mask_ignored", "mask_in_lse", "word_bit_swap"):
        return [(x, vocab, D.make_mask(k, vocab), None, None, 0) for k in ("alternating", "block")]
    if mutant == "last_tie":
        return [(x, vocab, D.make_mask("ones", vocab), None, None, 0)]          # the integer row holds its maximum many times
    if mutant == "pad_counted":
        return [(x, vocab, None, None, None, 0)]
    if mutant == "early_at_equal":
        return [D.min_new_case(BF16)[:1] + (vocab,) + D.min_new_case(BF16)[1:]]
    raise ValueError(mutant)


@pytest.mark.parametrize("mutant", D.MUTANTS)
def test_planted_defects_are_caught(mutant):
    caught = clean = 0
    for x, vocab, allow, early, n_gen, min_new in _mutant_inputs(mutant):
        res = _run(x, vocab, allow, early, n_gen, min_new)
        clean += res[0] == 0 and res[1] == 0 and res[3] == 0
        bad = _run(x, vocab, allow, early, n_gen, min_new, mutant=mutant)
        caught += bad[0] > 0 or bad[1] > 0 or bad[3] > 0
    assert clean == len(_mutant_inputs(mutant)), "the restatement itself must pass where its mutant is judged"
    assert caught == len(_mutant_inputs(mutant)), f"{mutant} passed the check"
