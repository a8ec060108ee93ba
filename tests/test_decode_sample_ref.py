"""The checker of ``ssi_decode_sample`` checks itself on the CPU (tests/decode_sample_ref.py): the fp32 restatement of the kernel stays inside
the bounds on every committed case, every planted defect is caught, the sampler draws from the distribution it claims, and the committed
seeds meet the margin conditions the GPU test relies on."""
import numpy as np
import pytest
import torch

import decode_sample_ref as S
import decode_select_ref as D

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", (BF16, F32), ids=("bf16", "fp32"))


def _restated(case, M, s, mutant=None):
    return S.restate(case.x, case.vocab, M, T=s["T"], top_k=s["top_k"], top_p=s["top_p"], seed=case.seed, step=case.step, seqs=case.seqs,
                     mutant=mutant)


@DTYPES
@pytest.mark.parametrize("vocab,rows", S.SHAPES, ids=[f"{v}x{r}" for v, r in S.SHAPES])
def test_committed_seeds_meet_the_margin_conditions_and_the_restatement_stays_inside_the_bounds(vocab, rows, dtype):
    case, found = S.case(vocab, rows, dtype)
    assert S.conditions(case, [e for _, _, e in found])
    for s, allow, exp in found:
        assert exp.margin_ok.all(), s                                                   # best - second > 2 delta on every row
        if vocab <= 2049:
            assert not exp.ambiguous.any(), s
        else:
            assert exp.ambiguous.sum() <= S.MAX_AMBIGUOUS_FLAGSHIP * rows, s
        if rows > 3 and s["top_p"] == 1.0 and s["top_k"] not in (-1, 50):
            continue                                                                    # (the restatement sorts per row: the wide case in part)
        _, M = S.masks_of(s["kind"], vocab, rows)
        bad_tok, bad_kept, ratio, misses = S.judge(_restated(case, M, s), case, exp)
        assert (bad_tok, bad_kept, misses) == (0, 0, 0), (s, bad_tok, bad_kept, ratio)


def _wide_case(dtype, rows=33, vocab=2049, seed=21):
    x = D.make_logits(rows, vocab, D.ld_of(vocab), dtype, seed=seed)
    return S.Case(x, vocab, seqs=torch.arange(rows) * 3, seed=99, step=1)


# mutant -> (setting, which count of ``judge`` must be > 0): 0 tokens, 1 n_kept, 3 logprob misses
CATCH = {"mask_ignored": (dict(T=1.0, top_k=-1, top_p=1.0, kind="alternating"), 0),
         "mask_in_lse": (dict(T=1.0, top_k=-1, top_p=1.0, kind="block"), 3),
         "topp_before_topk": (dict(T=1.3, top_k=50, top_p=0.9, kind="null"), 1),
         "ties_dropped": (dict(T=1.0, top_k=2, top_p=1.0, kind="null"), 1),
         "temp_in_logprob": (dict(T=0.7, top_k=-1, top_p=1.0, kind="null"), 3),
         "sequence_ignored": (dict(T=1.0, top_k=-1, top_p=1.0, kind="null"), 0)}


@DTYPES
@pytest.mark.parametrize("mutant", sorted(CATCH))
def test_every_planted_defect_is_caught(mutant, dtype):
    case = _wide_case(dtype)
    s, which = CATCH[mutant]
    _, M = S.masks_of(s["kind"], case.vocab, case.rows)
    exp = case.expected(M, s["T"], s["top_k"], s["top_p"])
    assert exp.margin_ok.all() and not exp.ambiguous.any()
    assert S.judge(_restated(case, M, s), case, exp)[:2] == (0, 0) and S.judge(_restated(case, M, s), case, exp)[3] == 0
    assert S.judge(_restated(case, M, s, mutant), case, exp)[which] > 0


def test_a_32_bit_u_that_reaches_one_is_caught():
    """Sequence 47317 under seed 2^33 at step 5 gives column 1201 the word 0xffffff84: (w + 1/2) 2^-32 rounds to 1.0 in fp32, G = +inf, and that
    column wins whatever its logit.  (Found by a search over 2^25 words; the 23-bit u of the definition is 1 - 2^-24 there: G = 16.64.)"""
    vocab = 2049
    assert int(S.philox_words([47317], vocab, 1 << 33, 5)[0, 1201]) == 0xFFFFFF84
    x = D.make_logits(1, vocab, D.ld_of(vocab), F32, seed=4)
    x[0, 1201] = x[0, :vocab].min() - 30.0
    case = S.Case(x, vocab, seqs=[47317], seed=1 << 33, step=5)
    M = np.ones((1, vocab), dtype=bool)
    s = dict(T=1.0, top_k=-1, top_p=1.0)
    exp = case.expected(M, **s)
    assert exp.margin_ok.all() and int(exp.token[0]) != 1201
    assert np.isfinite(case.G).all() and abs(case.G[0, 1201] - 16.6355) < 1e-3
    assert S.judge(_restated(case, M, s), case, exp)[:2] == (0, 0)
    got = _restated(case, M, s, "u32")
    assert int(got[0][0]) == 1201 and S.judge(got, case, exp)[0] == 1


def test_gumbel_range_of_the_23_bit_u():
    g = S.gumbel64(np.array([0, 0x1FF, 0xFFFFFE00, 0xFFFFFFFF], dtype=np.int64))
    assert g[0] == g[1] and g[2] == g[3] and -2.82 < g[0] < -2.81 and 16.63 < g[3] < 16.64


def _draws(x, T, top_k, n_seq=2000, n_step=100, seed=20260101):
    """Reference draws of one row over n_seq * n_step distinct (sequence, step) pairs: the counts per column."""
    vocab = x.numel()
    X = x.double().numpy()
    cols = np.arange(vocab)
    if top_k > 0:
        cols = np.flatnonzero(X >= np.sort(X)[-top_k])
    counts = np.zeros(vocab, dtype=np.int64)
    for step in range(n_step):
        G = S.gumbel64(S.philox_words(torch.arange(n_seq), vocab, seed, step))
        counts += np.bincount(cols[np.argmax(X[cols][None, :] / T + G[:, cols], axis=1)], minlength=vocab)
    return counts, cols


@pytest.mark.parametrize("top_k,quantile", ((-1, 37.70), (4, 16.27)), ids=("all16", "top4"))
def test_the_draws_follow_the_softmax(top_k, quantile):
    """200 000 draws at V = 16, T = 0.8 against softmax(x / T) (renormalised over the top 4 with top_k = 4): chi-square below the 99.9 %
    quantile at 15 (3) degrees of freedom.  The seed is fixed: the test is deterministic."""
    x = 1.5 * torch.randn(16, generator=torch.Generator().manual_seed(7))
    T = 0.8
    counts, cols = _draws(x, T, top_k)
    assert counts.sum() == 200_000 and counts[np.setdiff1d(np.arange(16), cols)].sum() == 0
    p = torch.softmax(x.double()[cols] / T, 0).numpy()
    chi2 = float((((counts[cols] - 200_000 * p) ** 2) / (200_000 * p)).sum())
    print(f"chi-square {chi2:.2f} (limit {quantile})")
    assert chi2 < quantile
    # and the checker's own reference agrees with this direct restatement on a few pairs
    case = S.Case(x[None, :].expand(5, -1).contiguous(), 16, seqs=torch.arange(5), seed=20260101, step=3)
    exp = case.expected(np.ones((5, 16), dtype=bool), T, top_k, 1.0)
    G = S.gumbel64(S.philox_words(torch.arange(5), 16, 20260101, 3))
    assert exp.token.tolist() == cols[np.argmax(x.double().numpy()[cols][None, :] / T + G[:, cols], axis=1)].tolist()
