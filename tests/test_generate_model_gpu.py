"""Generation on the model (``HipLlamaDecoder.new_kv_cache / prefill / decode_step``, ``ssi.generate.generate``) against ``OracleLlama`` on
the CPU: weights and batches from ``oracle.hf_crosscheck``.

* teacher-forced, fp32, ``tiny`` and ``small``: ragged prompts (the first 1 and 17 tokens of the two seeded rows) in one ``prefill``, then the
  true next tokens through ``decode_step`` to the end of the rows; the logits of the prefill and of EVERY step within
  ``1e-4 * logits_absmax`` of the oracle's full-forward logits at those positions (the criterion of ``test_model_gpu.py``);
* bf16 on an MFMA-shaped model (the padded 256-row path): the same walk with 5 sequences; the largest distance of the decode logits from
  the fp32 oracle at most 2 x that of the model's OWN bf16 full forward, measured in the same test;
* the greedy loop, fp32 ``tiny``: the tokens of ``generate`` equal the oracle's greedy continuation by full recompute, on prompts chosen so
  that the oracle's top-1 logit leads its top-2 by more than ``1e-3 * logits_absmax`` at every step (asserted here, no step left out);
  shuffled prompts, smaller groups, the cumulative log-probability, stopping, and the host refusals;
* training is untouched: loss and gradients bit-equal with a ``generate`` before the step and between its forward and its backward.

Measured on the MI355X: fp32 decode logits 1.8e-6 (tiny) and 5.0e-6 (small) from the oracle against tolerances of 2.6e-4 and 3.8e-4; bf16 decode
8.19e-2 against the full forward's own 8.81e-2 (0.93 x)."""
import numpy as np
import pytest
import torch

from oracle import hf_crosscheck as hx

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MFMA_PARAMS = dict(vocab_size=700, num_layers=2, num_heads=8, num_kv_heads=2, embed_dim=512, max_seq_len=512, intermediate_dim=512)
GREEDY_PROMPT_SEED = 5        # chosen on the CPU: with these prompts the oracle alone meets the margin condition below (lead 5e-3 of absmax)
GREEDY_LENS = (3, 9, 1, 14)
MAX_NEW = 24


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


def oracle_logits(ref, tokens_1d):
    with torch.no_grad():
        return ref(tokens_1d[None])[0].double()          # [S, V]


def teacher_forced_walk(model, rows, prompt_lens):
    """``prefill`` of ``rows[i][:prompt_lens[i]]``, then every further token of every row through ``decode_step``.  Returns a list of
    ``(row, position, logits [V] on the CPU)``: the logits that predict position + 1."""
    n, S, V = len(rows), rows[0].numel(), model.vocab_size
    cache = model.new_kv_cache(n, S + max(prompt_lens))
    got = []
    logits = model.prefill(cache, [rows[i][:prompt_lens[i]] for i in range(n)], max_new_tokens=S - min(prompt_lens))
    assert logits.shape == (n, model.vocab_pad)
    for i in range(n):
        got.append((i, prompt_lens[i] - 1, logits[i, :V].float().cpu()))
    at = list(prompt_lens)
    while any(a < S for a in at):
        live = [a < S for a in at]
        tok = torch.tensor([int(rows[i][at[i]]) if live[i] else 0 for i in range(n)], dtype=torch.int64, device=DEV)
        slot = torch.tensor([i if live[i] else -1 for i in range(n)], dtype=torch.int32, device=DEV)
        logits = model.decode_step(cache, tok, slot)
        assert logits.shape == (n, model.vocab_pad)
        for i in range(n):
            if live[i]:
                got.append((i, at[i], logits[i, :V].float().cpu()))
                at[i] += 1
    assert cache.lengths.cpu().tolist() == [S] * n and int(cache.errors) == 0
    return got


@pytest.mark.parametrize("case", ("tiny", "small"))
def test_teacher_forced_logits_fp32(case):
    params, b, s, seed = hx.CASES[case]
    sd = hx.seeded_state_dict(params, seed)
    rows = list(hx.seeded_batch(params["vocab_size"], b, s, seed)["tokens"])
    ref = hx.oracle_model(params, sd, chunks=0)
    want = [oracle_logits(ref, r) for r in rows]
    absmax = max(float(w.abs().max()) for w in want)
    got = teacher_forced_walk(hip_model(params, sd), rows, (1, 17))
    assert len(got) == 2 * s - 1 - 17 + 2                  # the prefill's two rows and every step of either row
    worst = max(float((g.double() - want[i][pos]).abs().max()) for i, pos, g in got)
    print(f"{case}: decode logits max-abs error {worst:.3e}, tolerance {1e-4 * absmax:.3e}")
    for i, pos, g in got:
        err = float((g.double() - want[i][pos]).abs().max())
        assert err <= 1e-4 * absmax, f"row {i} position {pos}: {err} > {1e-4 * absmax}"


def test_teacher_forced_logits_bf16_on_the_mfma_path():
    params, seed, S = MFMA_PARAMS, 21, 40
    sd = hx.seeded_state_dict(params, seed)
    rs = np.random.RandomState(seed + 1)
    rows = list(torch.from_numpy(rs.randint(0, params["vocab_size"], size=(5, S)).astype(np.int64)))
    ref = hx.oracle_model(params, sd, chunks=0)
    want = [oracle_logits(ref, r) for r in rows]
    model = hip_model(params, sd, torch.bfloat16)
    assert model._mfma_shapes()
    model.eval()
    with torch.no_grad():
        full = model(tokens=torch.stack(rows).to(DEV)).double().cpu()           # [5, S, V]: the parent's code
    full_err = max(float((full[i] - want[i]).abs().max()) for i in range(5))
    got = teacher_forced_walk(model, rows, (1, 17, 5, 9, 30))
    dec_err = max(float((g.double() - want[i][pos]).abs().max()) for i, pos, g in got)
    print(f"bf16: decode {dec_err:.4e}, own full forward {full_err:.4e} from the fp32 oracle (ratio {dec_err / full_err:.2f})")
    assert dec_err <= 2.0 * full_err


# ---- the greedy loop ------------------------------------------------------------------------------------------------------------
def greedy_prompts(vocab):
    rs = np.random.RandomState(GREEDY_PROMPT_SEED)
    return [rs.randint(0, vocab, size=n).tolist() for n in GREEDY_LENS]


def oracle_greedy(ref, prompt, n_new):
    """Greedy continuation by full recompute: (tokens, smallest top-1 lead, largest |logit|, log-probabilities of the tokens)."""
    toks, lead, absmax, lps = list(prompt), [], 0.0, []
    for _ in range(n_new):
        row = oracle_logits(ref, torch.tensor(toks, dtype=torch.int64))[-1]
        top = row.topk(2).values
        lead.append(float(top[0] - top[1]))
        absmax = max(absmax, float(row.abs().max()))
        t = int(row.argmax())
        lps.append(float(torch.log_softmax(row, -1)[t]))
        toks.append(t)
    return toks[len(prompt):], min(lead), absmax, lps


@pytest.fixture(scope="module")
def greedy(tiny):
    params, sd, ref = tiny
    prompts = greedy_prompts(params["vocab_size"])
    want = [oracle_greedy(ref, p, MAX_NEW) for p in prompts]
    absmax = max(w[2] for w in want)
    for p, w in zip(prompts, want):       # the condition under which "equal tokens" is a fair demand of an fp32 model within 1e-4
        assert w[1] > 1e-3 * absmax, f"prompt of {len(p)}: the oracle's top-1 leads by {w[1]:.3e}, needs {1e-3 * absmax:.3e}"
    return prompts, want, hip_model(params, sd)


def test_greedy_tokens_equal_the_oracles(greedy):
    from ssi.generate import generate
    prompts, want, model = greedy
    gens = generate(model, prompts, max_new_tokens=MAX_NEW, stop_token_ids=[], pad_id=0, logprobs=True)
    for p, g, w in zip(prompts, gens, want):
        assert g.token_ids == w[0] and g.finish_reason == "length" and g.stop_reason is None and g.prompt_len == len(p)
        assert abs(g.cumulative_logprob - sum(w[3])) <= 1e-5 * abs(sum(w[3]))
    assert model.training                                                      # (put back as it was found)
    # shuffled, and in groups of three: the same tokens per prompt
    order = [2, 0, 3, 1]
    shuffled = generate(model, [prompts[i] for i in order], max_new_tokens=MAX_NEW, stop_token_ids=[], pad_id=0)
    assert [g.token_ids for g in shuffled] == [want[i][0] for i in order]
    assert all(g.cumulative_logprob is None for g in shuffled)
    small = generate(model, prompts, max_new_tokens=MAX_NEW, stop_token_ids=[], pad_id=0, batch_size=3)
    assert [g.token_ids for g in small] == [w[0] for w in want]


def test_stopping(greedy):
    from ssi.generate import generate
    prompts, want, model = greedy
    i, k = 1, 5
    stop = want[i][0][k]
    gens = generate(model, prompts, max_new_tokens=MAX_NEW, stop_token_ids=[stop], pad_id=0)
    for j, (g, w) in enumerate(zip(gens, want)):
        if stop in w[0]:
            cut = w[0].index(stop) + 1
            assert g.token_ids == w[0][:cut] and g.finish_reason == "stop" and g.stop_reason == stop, j
        else:                                                                   # unchanged, token for token
            assert g.token_ids == w[0] and g.finish_reason == "length" and g.stop_reason is None, j
    assert gens[i].finish_reason == "stop" and len(gens[i].token_ids) <= k + 1
    # every row stops at its first token: the group ends at the first read-back, the results are one token each
    firsts = [w[0][0] for w in want]
    gens = generate(model, prompts, max_new_tokens=MAX_NEW, stop_token_ids=firsts, pad_id=0)
    assert [g.token_ids for g in gens] == [[t] for t in firsts] and all(g.finish_reason == "stop" for g in gens)
    gens = generate(model, prompts, max_new_tokens=2, stop_token_ids=[], pad_id=0)
    assert [g.token_ids for g in gens] == [w[0][:2] for w in want] and all(g.finish_reason == "length" for g in gens)


def test_host_refusals_come_before_any_launch(tiny):
    from ssi.generate import generate
    params, sd, _ = tiny
    model = hip_model(params, sd)
    cache = model.new_kv_cache(2, 16)
    kw = dict(stop_token_ids=[], pad_id=0)
    with pytest.raises(ValueError, match="cap"):
        model.prefill(cache, [[1, 2, 3], [4]], max_new_tokens=14)               # 3 + 14 > 16
    with pytest.raises(ValueError, match="empty"):
        model.prefill(cache, [[1, 2, 3], []])
    with pytest.raises(ValueError, match="slots"):
        model.prefill(cache, [[1], [2], [3]])
    with pytest.raises(ValueError, match="empty"):
        generate(model, [[5, 6], []], max_new_tokens=4, **kw)
    with pytest.raises(ValueError, match="max_seq_len|RoPE"):
        generate(model, [[5, 6, 7]], max_new_tokens=params["max_seq_len"] - 2, **kw)
    short = hip_model(dict(params, max_seq_len=64), sd)
    with pytest.raises(ValueError, match="max_seq_len|RoPE"):
        generate(short, [list(range(60))], max_new_tokens=8, **kw)
    assert model._arena.buf == {} and short._arena.buf == {}                   # nothing ran: no activation buffer was ever asked for
    assert cache.lengths.cpu().tolist() == [0, 0] and int(cache.errors) == 0


# ---- training is untouched --------------------------------------------------------------------------------------------------------
def _step(model, dbatch, between=None):
    from ssi.loss import CEWithChunkedOutputLoss, compute_loss
    model.set_num_output_chunks(8)
    loss = compute_loss(dbatch, model, CEWithChunkedOutputLoss())
    if between is not None:
        between()
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), model._flat_grad.clone()


@pytest.mark.parametrize("which", ("tiny-fp32", "mfma-bf16"))
def test_a_training_step_is_bit_equal_with_generation_around_it(which):
    from ssi.generate import generate
    if which == "tiny-fp32":
        params, b, s, seed = hx.CASES["tiny"]
        dtype = torch.float32
    else:
        params, b, s, seed, dtype = MFMA_PARAMS, 2, 128, 21, torch.bfloat16
    sd = hx.seeded_state_dict(params, seed)
    dbatch = {k: v.to(DEV) for k, v in hx.seeded_batch(params["vocab_size"], b, s, seed).items()}
    prompts = greedy_prompts(params["vocab_size"])

    def gen(model):
        out = generate(model, prompts, max_new_tokens=10, stop_token_ids=[], pad_id=0, logprobs=True)
        assert all(len(g.token_ids) == 10 for g in out)

    loss0, grad0 = _step(hip_model(params, sd, dtype), dbatch)
    before = hip_model(params, sd, dtype)
    gen(before)
    loss1, grad1 = _step(before, dbatch)
    assert torch.equal(loss1, loss0) and torch.equal(grad1, grad0)
    mid = hip_model(params, sd, dtype)
    loss2, grad2 = _step(mid, dbatch, between=lambda: gen(mid))
    assert torch.equal(loss2, loss0) and torch.equal(grad2, grad0)
    assert bool(torch.isfinite(grad0.float()).all()) and float(grad0.float().abs().max()) > 0
