"""CPU self-test of tests/decode_penalty_ref.py: the fp32 restatements of the two penalised kernels pass the checker on every committed
case, and every planted defect fails it on at least one; the histories hold what the issue lists; the neutral setting is the identity."""
import numpy as np
import pytest
import torch

import decode_penalty_ref as P
import decode_select_ref as D

F32, BF16 = torch.float32, torch.bfloat16


def _run(case, drawn, exps, mutant):
    """Does the checker fail anywhere on the restatements with ``mutant`` planted?  (select fails, sample fails)"""
    sel = smp = 0
    for (kind, hist, allow, M, (r, f, p), d), dr, e in zip(case.items, drawn, exps):
        y = P.penalised(case.x, case.vocab, hist, r, f, p)
        if mutant not in P.SAMPLE_ONLY:
            got = P.restate_select(case.x, case.vocab, M, hist, r, f, p, mutant=mutant)
            bt, br, _, miss = P.judge_select(got, P.expect_select(case.base, y, M))
            sel += bt + br + miss
        got = P.restate_sample(case.x, case.vocab, M, hist, r, f, p, seed=case.seed, step=case.step, seqs=case.seqs, mutant=mutant, **d)
        bt, bk, _, miss = dr.judge(got, e)
        smp += bt + bk + miss
    return sel, smp


@pytest.fixture(scope="module")
def committed():
    return [P.case(v, r, dt) for v, r in P.CPU_SHAPES for dt in (F32, BF16)]


def test_the_restatements_pass_on_every_committed_case(committed):
    for case, drawn, exps in committed:
        assert _run(case, drawn, exps, None) == (0, 0), case.vocab
        assert all(P.clear(e) for e in exps)


@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_every_mutant_fails_on_a_committed_case(committed, mutant):
    sel = smp = 0
    for case, drawn, exps in committed[-4:]:                 # vocab 257 and 2049, both dtypes
        a, b = _run(case, drawn, exps, mutant)
        sel, smp = sel + a, smp + b
    assert smp > 0, f"{mutant}: the sampler's checker saw nothing"
    assert mutant in P.SAMPLE_ONLY or sel > 0, f"{mutant}: the selector's checker saw nothing"


def test_neutral_penalties_leave_the_row_bit_for_bit():
    case, _, _ = P.case(2049, 3, BF16)
    x = case.x.clone()
    x[0, 3], x[0, 4], x[1, 5] = 0.0, -0.0, float("-inf")
    for kind, hist, *_ in case.items:
        y = P.penalised(x, case.vocab, hist, 1.0, 0.0, 0.0)
        assert np.array_equal(y.view(np.int32), x[:, :case.vocab].float().numpy().view(np.int32)), kind


def test_the_definition_on_a_hand_made_row():
    x = torch.tensor([[2.0, -2.0, 0.0, 4.0, 1.0, 1.0, float("nan"), 3.0]])
    h = P.History([[0, 1, 2, 6]], [[3, 3, 4, 1]], ld_gen=4)
    y = P.penalised(x, 8, h, 2.0, 0.5, 0.25)
    #      prompt only: x / r    both, n = 1: x r - .75   prompt only, 0: 0    n = 2: 4 / 2 - 1.25   n = 1: .5 - .75   not in H   NaN stays   not in H
    want = [1.0, -4.75, 0.0, 0.75, -0.25, 1.0, float("nan"), 3.0]
    assert np.array_equal(np.nan_to_num(y[0], nan=-99.0), np.nan_to_num(np.array(want, np.float32), nan=-99.0))
    seen, cnt, n_bad = P.with_bad_ids(h, 8, [0]).counts(8)
    assert n_bad == 1 and cnt[0].tolist() == [0, 1, 0, 2, 1, 0, 0, 0] and seen[0].tolist() == [True] * 5 + [False, True, False]


def test_the_histories_hold_what_they_are_named_for():
    case, _, _ = P.case(2049, 3, F32)
    by_kind = {kind: (hist, allow) for kind, hist, allow, *_ in case.items}
    assert set(by_kind) == set(P.HISTORIES)
    h, allow = by_kind["edges"]
    seen, cnt, _ = h.counts(2049)
    assert seen[:, 0].all() and seen[:, 2048].all() and 2048 >= (2049 // 8) * 8                  # column 0, vocab - 1 = the scalar tail
    assert allow is not None and seen[:, int(torch.nonzero(~allow)[0])].all()                     # a disallowed column
    assert ((cnt > 0) & seen).any() and ((cnt == 0) & seen).any()                                 # the output; the prompt only
    assert by_kind["repeat300"][0].counts(2049)[1].max() >= 300
    h, _ = by_kind["congruent"]
    assert h.ld_gen == 32 and P.table_slots(32) == 64 and all(t % 64 == 63 for t in h.gens[0]) and len(set(h.gens[0])) == 31
    assert len({t % 64 for t in h.gens[1]}) == 1 and len(set(h.gens[1])) == 32                    # a full chain; row 0's wraps around
    h, _ = by_kind["full"]
    assert all(len(set(g)) == h.ld_gen == 256 for g in h.gens)
    assert by_kind["shared"][0].prompt_row is not None and len(by_kind["shared"][0].prompts) == 2
    for n in P.LD_GENS:
        h, _ = by_kind[f"ld{n}"]
        assert h.ld_gen == n and [len(g) for g in h.gens] == [0, 1, n]
    assert by_kind["empty"][0].ld_prompt == 0 and not any(by_kind["empty"][0].gens)
    assert P.lds_bytes(133_376, 256) == 20_768 and P.lds_bytes(1, 0) == 4 + 512


def test_the_settings_move_the_choice():
    """At least one committed row chooses differently under the penalties than without them (else nothing is tested)."""
    case, _, _ = P.case(2049, 3, F32)
    moved = 0
    for kind, hist, allow, M, (r, f, p), _ in case.items:
        y = P.penalised(case.x, case.vocab, hist, r, f, p)
        moved += int((P.expect_select(case.base, y, M)[3] > (case.base.expected(allow)[3])).sum())
    assert moved >= 3
