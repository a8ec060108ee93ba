"""GPU: minimum-Bayes-risk selection.  ``ssi.generate.mbr_select`` against the Python restatement of the risk (``edit_ref.mbr_ref``, built on
the restated edit distance) — exactly: the distances are integers, and the float64 sum is taken in the same order with the same operations —
and ``sample(mbr=True)`` / ``beam_search(mbr=True)`` on the fp32 ``tiny`` golden model: the candidates of the plain call (samples and beams
are bit-reproducible, so they are compared by tokens) in the restatement's order with its risks."""
import dataclasses

import numpy as np
import pytest
import torch

import edit_ref
from oracle import hf_crosscheck as hx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENS = (3, 9, 14, 5, 1)
MAX_NEW = 10


def _check(candidates):
    from ssi.generate import mbr_select
    order, risks = mbr_select(candidates, DEV)
    assert len(order) == len(risks) == len(candidates)
    for cs, o, r in zip(candidates, order, risks):
        want_o, want_r = edit_ref.mbr_ref(cs)
        assert r == want_r and o == want_o, (cs, o, r, want_o, want_r)          # bit for bit
        assert o[0] == min(range(len(cs)), key=lambda k: (r[k], k))             # the choice is the first minimum
    return order, risks


def test_select_against_the_restatement():
    rng = np.random.RandomState(3)
    seq = lambda n, v: rng.randint(0, v, size=n).tolist()   # noqa: E731
    _check([[seq(5, 4), seq(9, 4), seq(2, 4)],                                  # unequal lengths
            [seq(30, 3) for _ in range(8)],
            [seq(int(rng.randint(0, 300)), 5) for _ in range(8)],               # beyond one column block of the kernel
            [seq(7, 50), seq(7, 50)],                                           # two candidates: each is the other's only reference
            [[], seq(4, 9), [], seq(1, 9)],                                     # empty candidates (their length counts as 1 in the rate)
            [[], []]])


def test_equal_candidates_and_an_exact_tie():
    order, risks = _check([[[4, 5, 6]] * 5, [[1, 2], [1, 3], [1, 2]], [[9], [8], [7]]])
    assert risks[0] == [0.0] * 5 and order[0] == [0, 1, 2, 3, 4]               # risk 0, choice 0
    assert risks[1][0] == risks[1][2] == 0.25 and order[1] == [0, 2, 1]         # an exact tie goes to the lower index
    assert risks[2] == [1.0] * 3 and order[2] == [0, 1, 2]


def test_one_candidate_is_refused_before_any_launch():
    from ssi.generate import mbr_select
    with pytest.raises(ValueError, match="at least two"):
        mbr_select([[[1, 2], [3]], [[1]]], DEV)


@pytest.fixture(scope="module")
def tiny():
    from ssi.model import HipLlamaDecoder
    params, _, _, seed = hx.CASES["tiny"]
    model = HipLlamaDecoder(**params, dtype=torch.float32, device=DEV)
    model.load_state_dict(hx.seeded_state_dict(params, seed))
    rs = np.random.RandomState(5)
    V = params["vocab_size"]
    # a wide stop set: some candidates stop early, so their lengths differ and the stop token is cut from what is compared
    return model, [rs.randint(0, V, size=n).tolist() for n in LENS], dict(max_new_tokens=MAX_NEW, stop_token_ids=list(range(0, V, 6)), pad_id=0)


def _same_candidates_in_mbr_order(plain, mbr):
    from ssi.generate import mbr_candidate
    assert len(plain) == len(mbr) == len(LENS)
    lengths, moved = set(), 0
    for gs, ms in zip(plain, mbr):
        want_o, want_r = edit_ref.mbr_ref([mbr_candidate(g) for g in gs])
        assert [dataclasses.asdict(m) for m in ms] == [dataclasses.asdict(gs[k]) for k in want_o]      # the same Generations, reordered
        assert [m.mbr_index for m in ms] == want_o and [m.mbr_risk for m in ms] == [want_r[k] for k in want_o]
        assert all(g.mbr_risk is None for g in gs)
        lengths |= {len(mbr_candidate(g)) for g in gs}
        moved += want_o != sorted(want_o)
    assert len(lengths) > 1 and moved > 0, "the scenario shows neither unequal candidates nor a reorder"


@pytest.mark.parametrize("seed", [2026, 7])
def test_sample_with_mbr_returns_the_same_samples_in_risk_order(tiny, seed):
    from ssi.generate import sample
    model, prompts, kw = tiny
    draw = dict(n=4, temperature=0.8, top_k=20, top_p=0.9, seed=seed, batch_size=9)
    _same_candidates_in_mbr_order(sample(model, prompts, **draw, **kw), sample(model, prompts, mbr=True, **draw, **kw))


def test_beam_search_with_mbr_returns_the_same_beams_in_risk_order(tiny):
    from ssi.generate import beam_search
    model, prompts, kw = tiny
    beam = dict(beam_width=4, n_best=4, batch_size=9)
    _same_candidates_in_mbr_order(beam_search(model, prompts, **beam, **kw), beam_search(model, prompts, mbr=True, **beam, **kw))


def test_without_mbr_nothing_changes(tiny):
    from ssi.generate import Generation, beam_search, sample
    model, prompts, kw = tiny
    assert [f.name for f in dataclasses.fields(Generation)] == ["token_ids", "finish_reason", "stop_reason", "cumulative_logprob", "prompt_len",
                                                                "n_constrained", "score", "n_kept_mean"]
    for run, args in ((sample, dict(n=3, temperature=0.8, seed=1)), (beam_search, dict(beam_width=3, n_best=2))):
        off, absent = run(model, prompts, mbr=False, **args, **kw), run(model, prompts, **args, **kw)
        assert off == absent and all(g.mbr_risk is None and g.mbr_index is None for gs in off for g in gs)
    with pytest.raises(ValueError, match="at least two candidates"):
        sample(model, prompts, n=1, temperature=0.8, seed=1, mbr=True, **kw)
    with pytest.raises(ValueError, match="at least two candidates"):
        beam_search(model, prompts, beam_width=3, n_best=1, mbr=True, **kw)
