"""``ssi.generate.sample`` on the fp32 ``tiny`` golden model against a continuation of the CPU oracle by full recompute that draws with the
reference sampler of tests/decode_sample_ref.py: tokens, finish reasons and cumulative log-probabilities for ``n = 1`` and ``n = 3`` (sample
``j`` of prompt ``i`` is the oracle's continuation with sequence ``3 i + j``), two identical calls bit-equal, and a training step bit-equal
with a ``sample`` call between its forward and its backward.

The model's fp32 logits lie within ``1e-4 * logits_absmax`` of the oracle's (test_generate_model_gpu.py), so equal tokens are a fair demand
where the oracle's draw is clear of that: at every step the best score in the kept set leads the second by more than
``1e-3 * logits_absmax / T`` (a logit off by e moves a score by e / T, two of them the gap by 2e-4 absmax / T: five times that), and the thresholds, which sit between logits that move, too, cannot
move the draw: it is the same with ``top_p`` lower or higher by ``1e-3 * logits_absmax / T`` (logits off by e change every mass by at most
2 e / T relatively and M / Z by at most 4 e / T; e = 1e-4 absmax, and 2.5 times that is taken), and with ``top_k`` one lower or higher
wherever the k-th and (k + 1)-th logits are closer than ``2e-3 * logits_absmax`` (elsewhere the top-k set cannot change).  All of it is
asserted on the oracle alone, no step left out."""
import numpy as np
import pytest
import torch

import decode_sample_ref as S
from oracle import hf_crosscheck as hx

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PROMPT_SEED = 5               # chosen on the CPU: with these prompts and SEED the oracle alone meets the conditions above
LENS = (3, 9, 14)
MAX_NEW = 8
SEED = 2026
DRAW = dict(temperature=0.8, top_k=20, top_p=0.9)


def hip_model(params, sd, dtype=torch.float32):
    from ssi.model import HipLlamaDecoder
    m = HipLlamaDecoder(**params, dtype=dtype, device=DEV)
    m.load_state_dict(sd)
    return m


@pytest.fixture(scope="module")
def tiny():
    params, _, _, seed = hx.CASES["tiny"]
    sd = hx.seeded_state_dict(params, seed)
    return params, sd, hx.oracle_model(params, sd, chunks=0)


def prompts_of(vocab):
    rs = np.random.RandomState(PROMPT_SEED)
    return [rs.randint(0, vocab, size=n).tolist() for n in LENS]


def oracle_sample(ref, prompt, n_new, sequence, stop=()):
    """The oracle's sampled continuation by full recompute: (tokens, log-probabilities, smallest score gap * T / |logit|max, stable)."""
    toks, lps, lead, stable = list(prompt), [], np.inf, True
    for t in range(n_new):
        with torch.no_grad():
            row = ref(torch.tensor(toks, dtype=torch.int64)[None])[0][-1].double()
        V = row.numel()
        case = S.Case(row[None, :].float(), V, seqs=[sequence], seed=SEED, step=t)
        M = np.ones((1, V), dtype=bool)
        T, k, p = DRAW["temperature"], DRAW["top_k"], DRAW["top_p"]
        exp = case.expected(M, T, k, p)
        tok = int(exp.token[0])
        lead = min(lead, float(exp.gap[0]) * T / float(row.abs().max()))
        absmax = float(row.abs().max())
        dp = 1e-3 * absmax / T
        top = torch.sort(row, descending=True).values
        near = [kk for kk in (k - 1, k + 1) if float(top[min(k, kk) - 1] - top[min(k, kk)]) < 2e-3 * absmax]
        for kk, pp in [(kk, p) for kk in near] + [(k, p - dp), (k, min(p + dp, 1.0))]:
            stable = stable and int(case.expected(M, T, kk, pp).token[0]) == tok
        lps.append(float(torch.log_softmax(row, -1)[tok]))
        toks.append(tok)
        if tok in stop:
            break
    return toks[len(prompt):], lps, lead, stable


@pytest.fixture(scope="module")
def sampled(tiny):
    params, sd, ref = tiny
    prompts = prompts_of(params["vocab_size"])
    want = {(i, j): oracle_sample(ref, p, MAX_NEW, 3 * i + j) for i, p in enumerate(prompts) for j in range(3)}
    for key, w in want.items():
        assert w[2] > 1e-3 and w[3], f"prompt {key[0]} sample {key[1]}: lead {w[2]:.3e} of the largest logit, stable thresholds {w[3]}"
    return prompts, want, hip_model(params, sd), ref


def test_n_3_samples_equal_the_oracles_draws_with_sequence_3i_plus_j(sampled):
    from ssi.generate import sample
    prompts, want, model, _ = sampled
    got = sample(model, prompts, n=3, seed=SEED, max_new_tokens=MAX_NEW, stop_token_ids=[], pad_id=0, **DRAW)
    assert [len(g) for g in got] == [3] * len(prompts)
    for i, p in enumerate(prompts):
        for j in range(3):
            g, w = got[i][j], want[(i, j)]
            assert g.token_ids == w[0] and g.finish_reason == "length" and g.stop_reason is None and g.prompt_len == len(p), (i, j)
            assert abs(g.cumulative_logprob - sum(w[1])) <= 1e-5 * abs(sum(w[1])), (i, j)
            assert 1.0 <= g.n_kept_mean <= DRAW["top_k"]
    assert len({tuple(g.token_ids) for gs in got for g in gs}) > len(prompts)           # the samples of a prompt differ
    assert model.training
    # two identical calls: bit-equal; smaller groups and another order of the prompts: the same samples per prompt
    again = sample(model, prompts, n=3, seed=SEED, max_new_tokens=MAX_NEW, stop_token_ids=[], pad_id=0, **DRAW)
    assert [[(g.token_ids, g.cumulative_logprob, g.n_kept_mean) for g in gs] for gs in again] == \
           [[(g.token_ids, g.cumulative_logprob, g.n_kept_mean) for g in gs] for gs in got]
    small = sample(model, prompts, n=3, seed=SEED, max_new_tokens=MAX_NEW, stop_token_ids=[], pad_id=0, batch_size=7, **DRAW)
    assert [[g.token_ids for g in gs] for gs in small] == [[g.token_ids for g in gs] for gs in got]


def test_n_1_equals_the_oracles_draws_and_stops(sampled):
    from ssi.generate import sample
    prompts, _, model, ref = sampled
    # n = 1: the sequence of prompt i is i
    want = [oracle_sample(ref, p, MAX_NEW, i) for i, p in enumerate(prompts)]
    for i, w in enumerate(want):
        assert w[2] > 1e-3 and w[3], f"prompt {i}: lead {w[2]:.3e} of the largest logit, stable thresholds {w[3]}"
    got = sample(model, prompts, seed=SEED, max_new_tokens=MAX_NEW, stop_token_ids=[], pad_id=0, **DRAW)
    for i, (gs, w) in enumerate(zip(got, want)):
        assert len(gs) == 1 and gs[0].token_ids == w[0] and gs[0].finish_reason == "length", i
        assert abs(gs[0].cumulative_logprob - sum(w[1])) <= 1e-5 * abs(sum(w[1])), i
    stop = want[1][0][4]
    got = sample(model, prompts, seed=SEED, max_new_tokens=MAX_NEW, stop_token_ids=[stop], pad_id=0, batch_size=3, **DRAW)
    for i, (gs, w) in enumerate(zip(got, want)):
        if stop in w[0]:
            cut = w[0].index(stop) + 1
            assert gs[0].token_ids == w[0][:cut] and gs[0].finish_reason == "stop" and gs[0].stop_reason == stop, i
        else:
            assert gs[0].token_ids == w[0] and gs[0].finish_reason == "length", i
    assert got[1][0].finish_reason == "stop"
    # an allowed set and a minimum length: every token allowed, no stop token among the first three
    allowed = list(range(40, 300))
    got = sample(model, prompts, n=2, seed=SEED, max_new_tokens=8, stop_token_ids=[50, 60], pad_id=0, allowed_token_ids=allowed, min_new_tokens=3,
                 temperature=1.3)
    for gs in got:
        for g in gs:
            assert all(40 <= t < 300 for t in g.token_ids) and not {50, 60} & set(g.token_ids[:3]) and len(g.token_ids) >= 3


def test_a_training_step_is_bit_equal_with_a_sample_call_between_forward_and_backward(tiny):
    from ssi.generate import sample
    from ssi.loss import CEWithChunkedOutputLoss, compute_loss
    params, sd, _ = tiny
    _, b, s, seed = hx.CASES["tiny"]
    dbatch = {k: v.to(DEV) for k, v in hx.seeded_batch(params["vocab_size"], b, s, seed).items()}
    prompts = prompts_of(params["vocab_size"])

    def step(model, between=None):
        model.set_num_output_chunks(8)
        loss = compute_loss(dbatch, model, CEWithChunkedOutputLoss())
        if between is not None:
            between()
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), model._flat_grad.clone()

    def draw(model):
        for n in (1, 3):
            out = sample(model, prompts, n=n, seed=SEED, max_new_tokens=10, stop_token_ids=[], pad_id=0, **DRAW)
            assert all(len(g.token_ids) == 10 for gs in out for g in gs)

    loss0, grad0 = step(hip_model(params, sd))
    mid = hip_model(params, sd)
    loss1, grad1 = step(mid, between=lambda: draw(mid))
    assert torch.equal(loss1, loss0) and torch.equal(grad1, grad0)
    assert bool(torch.isfinite(grad0).all()) and float(grad0.abs().max()) > 0
