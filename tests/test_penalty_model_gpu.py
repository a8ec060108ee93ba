"""``generate`` and ``sample`` under repetition and frequency penalties on the fp32 ``tiny`` golden model against a continuation of the CPU
oracle by full recompute that takes the PENALISED argmax in float64 (``generate``) or draws with the reference sampler on the penalised
row (``sample``, ``n = 2``): tokens, finish reasons and cumulative log-probabilities; and a training step bit-equal with penalised calls
between its forward and its backward.

The model's fp32 logits lie within ``1e-4 * logits_absmax`` of the oracle's (test_generate_model_gpu.py).  A penalised value is the logit
times at most ``max(r, 1 / r) = 1.3`` less a term that depends on the history alone, so it moves by at most 1.3e-4 absmax and a gap between
two of them by 2.6e-4 absmax; equal tokens are demanded where the oracle's best penalised value leads the second by more than
``1e-3 * logits_absmax`` at every step (greedy), and where the draw meets test_sample_model_gpu.py's conditions on the penalised row (its
lead over the runner-up score, and the same draw with ``top_p`` and ``top_k`` moved across what the logits' error can reach).  All of it is
asserted on the oracle alone, no step left out; the prompts were chosen on the CPU so that it holds."""
import numpy as np
import pytest
import torch

import decode_penalty_ref as P
import decode_sample_ref as S
from oracle import hf_crosscheck as hx

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PROMPT_SEED = 1               # chosen on the CPU: with these prompts and SEED the oracle alone meets the conditions above
LENS = (3, 9, 14)
MAX_NEW = 10
SEED = 2030
PEN = dict(repetition_penalty=1.3, frequency_penalty=0.5)
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


def _row(ref, toks):
    with torch.no_grad():
        return ref(torch.tensor(toks, dtype=torch.int64)[None])[0][-1].double()


def penalised64(row, prompt, gen, r, f, p=0.0):
    """The definition in float64: where(x > 0, x / r, x r) - (f n + p [n > 0]) on the ids of the prompt and the output, x elsewhere."""
    n = torch.zeros_like(row)
    for t in gen:
        n[t] += 1
    seen = torch.zeros_like(row, dtype=torch.bool)
    seen[list(prompt) + list(gen)] = True
    y = torch.where(row > 0, row / r, row * r) - (f * n + p * (n > 0))
    return torch.where(seen, y, row)


def oracle_greedy(ref, prompt, n_new):
    """(tokens, log-probabilities, smallest lead of the best penalised value / |logit|max, steps whose token is not the raw row's first)."""
    toks, lps, lead, moved = list(prompt), [], np.inf, 0
    for _ in range(n_new):
        row = _row(ref, toks)
        y = penalised64(row, prompt, toks[len(prompt):], PEN["repetition_penalty"], PEN["frequency_penalty"])
        top = torch.sort(y, descending=True).values
        tok = int(y.argmax())
        lead = min(lead, float(top[0] - top[1]) / float(row.abs().max()))
        moved += tok != int(row.argmax())
        lps.append(float(torch.log_softmax(row, -1)[tok]))
        toks.append(tok)
    return toks[len(prompt):], lps, lead, moved


def oracle_sample(ref, prompt, n_new, sequence):
    """test_sample_model_gpu.py's continuation with the draw on the penalised row: (tokens, log-probabilities, lead, stable)."""
    toks, lps, lead, stable = list(prompt), [], np.inf, True
    T, k, p = DRAW["temperature"], DRAW["top_k"], DRAW["top_p"]
    for t in range(n_new):
        row = _row(ref, toks)
        V, absmax = row.numel(), float(row.abs().max())
        hist = P.History([prompt], [toks[len(prompt):]], ld_gen=n_new)
        y = P.penalised(row[None, :].float(), V, hist, PEN["repetition_penalty"], PEN["frequency_penalty"], 0.0)
        case = S.Case(torch.from_numpy(y), V, seqs=[sequence], seed=SEED, step=t)
        M = np.ones((1, V), dtype=bool)
        exp = case.expected(M, T, k, p)
        tok = int(exp.token[0])
        lead = min(lead, float(exp.gap[0]) * T / (1.3 * absmax))
        dp = 1.3e-3 * absmax / T
        top = np.sort(y[0])[::-1]
        near = [kk for kk in (k - 1, k + 1) if float(top[min(k, kk) - 1] - top[min(k, kk)]) < 2.6e-3 * absmax]
        for kk, pp in [(kk, p) for kk in near] + [(k, p - dp), (k, min(p + dp, 1.0))]:
            stable = stable and int(case.expected(M, T, kk, pp).token[0]) == tok
        lps.append(float(torch.log_softmax(row, -1)[tok]))
        toks.append(tok)
    return toks[len(prompt):], lps, lead, stable


@pytest.fixture(scope="module")
def setup(tiny):
    params, sd, ref = tiny
    return prompts_of(params["vocab_size"]), hip_model(params, sd), ref


def test_generate_takes_the_penalised_argmax_of_the_oracle(setup):
    from ssi.generate import generate
    prompts, model, ref = setup
    want = [oracle_greedy(ref, p, MAX_NEW) for p in prompts]
    for p, w in zip(prompts, want):
        assert w[2] > 1e-3, f"prompt of {len(p)}: the oracle's best penalised value leads by {w[2]:.3e} of the largest logit"
    assert sum(w[3] for w in want) >= 1                               # the setting changes at least one step's choice
    got = generate(model, prompts, max_new_tokens=MAX_NEW, stop_token_ids=[], pad_id=0, logprobs=True, **PEN)
    for g, w, p in zip(got, want, prompts):
        assert g.token_ids == w[0] and g.finish_reason == "length" and g.stop_reason is None and g.prompt_len == len(p)
        assert abs(g.cumulative_logprob - sum(w[1])) <= 1e-5 * abs(sum(w[1]))
        assert g.n_constrained == w[3]                                # rank != 0 exactly where the penalties changed the choice
    plain = generate(model, prompts, max_new_tokens=MAX_NEW, stop_token_ids=[], pad_id=0)
    assert [g.token_ids for g in plain] != [g.token_ids for g in got] and plain[0].n_constrained is None
    # a stop token, smaller groups: the same tokens up to the stop
    stop = want[1][0][4]
    cut = generate(model, prompts, max_new_tokens=MAX_NEW, stop_token_ids=[stop], pad_id=0, batch_size=2, **PEN)
    for g, w in zip(cut, want):
        if stop in w[0]:
            assert g.token_ids == w[0][:w[0].index(stop) + 1] and g.finish_reason == "stop" and g.stop_reason == stop
        else:
            assert g.token_ids == w[0] and g.finish_reason == "length"
    assert cut[1].finish_reason == "stop"


def test_two_samples_per_prompt_equal_the_oracles_draws_on_the_penalised_row(setup):
    from ssi.generate import sample
    prompts, model, ref = setup
    want = {(i, j): oracle_sample(ref, p, MAX_NEW, 2 * i + j) for i, p in enumerate(prompts) for j in range(2)}
    for key, w in want.items():
        assert w[2] > 1e-3 and w[3], f"prompt {key[0]} sample {key[1]}: lead {w[2]:.3e} of the largest logit, stable thresholds {w[3]}"
    got = sample(model, prompts, n=2, seed=SEED, max_new_tokens=MAX_NEW, stop_token_ids=[], pad_id=0, **DRAW, **PEN)
    for i, p in enumerate(prompts):
        for j in range(2):
            g, w = got[i][j], want[(i, j)]
            assert g.token_ids == w[0] and g.finish_reason == "length" and g.prompt_len == len(p), (i, j)
            assert abs(g.cumulative_logprob - sum(w[1])) <= 1e-5 * abs(sum(w[1])), (i, j)
    plain = sample(model, prompts, n=2, seed=SEED, max_new_tokens=MAX_NEW, stop_token_ids=[], pad_id=0, **DRAW)
    assert [[g.token_ids for g in gs] for gs in plain] != [[g.token_ids for g in gs] for gs in got]      # the penalties moved a draw
    one = sample(model, prompts, n=1, seed=SEED, max_new_tokens=MAX_NEW, stop_token_ids=[], pad_id=0, batch_size=2, **DRAW, **PEN)
    assert all(len(gs) == 1 and len(gs[0].token_ids) == MAX_NEW for gs in one)


def test_a_training_step_is_bit_equal_with_penalised_calls_between_forward_and_backward(tiny):
    from ssi.generate import generate, sample
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

    def calls(model):
        out = generate(model, prompts, max_new_tokens=6, stop_token_ids=[], pad_id=0, **PEN)
        assert all(len(g.token_ids) == 6 for g in out)
        for n in (1, 2):
            out = sample(model, prompts, n=n, seed=SEED, max_new_tokens=6, stop_token_ids=[], pad_id=0, presence_penalty=0.5, **DRAW)
            assert all(len(g.token_ids) == 6 for gs in out for g in gs)

    loss0, grad0 = step(hip_model(params, sd))
    mid = hip_model(params, sd)
    loss1, grad1 = step(mid, between=lambda: calls(mid))
    assert torch.equal(loss1, loss0) and torch.equal(grad1, grad0)
    assert bool(torch.isfinite(grad0).all()) and float(grad0.abs().max()) > 0
