"""``ssi.generate.beam_search`` on the fp32 ``tiny`` model of ``oracle.hf_crosscheck`` against the rules said again in plain Python
(tests/beam_ref.py) on ``OracleLlama`` by full recompute: tokens, finish reasons, hypothesis order and scores.

Setup: W = 3, 12 new tokens, prompts of 3, 9, 1 and 14 tokens from ``RandomState(5)``, the stop set the next 40 ``randint(0, 515)`` draws of
that stream (37 distinct ids).  "Equal hypotheses" is a fair demand of an fp32 model within 1e-4 of the oracle only where the oracle's own
choices are not close calls, so the MARGIN CONDITION is asserted here on the oracle, no step left out: at every step the adjacent gaps among
the first W + 1 continuations and among the first W + 1 merged entries are at least 1e-3 x the largest |logit| met, and adjacent final scores
differ by at least 1e-3.  Measured on the CPU with length_penalty 1: smallest step gap 3.1e-3 (1.06e-3 of absmax 2.95), smallest final gap
4.4e-3; the pools of two prompts fill early (after steps 9 and 5), two prompts end by length.  With length_penalty 0 the steps are the same
and the smallest final gap is 1.1e-1.

Further: n_best 1 and 3, shuffled prompts and a smaller batch_size, min_new_tokens with an allowed set (properties, not equality: the margin
does not hold there), beam_width 1 against ``generate``, no cache error, and a training step bit-equal around a ``beam_search``."""
import numpy as np
import pytest
import torch

import beam_ref as br
from oracle import hf_crosscheck as hx

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W, MAX_NEW, LENS, SEED = 3, 12, (3, 9, 1, 14), 5


def hip_model(params, sd, dtype=torch.float32):
    from ssi.model import HipLlamaDecoder
    m = HipLlamaDecoder(**params, dtype=dtype, device=DEV)
    m.load_state_dict(sd)
    return m


@pytest.fixture(scope="module")
def setup():
    params, _, _, seed = hx.CASES["tiny"]
    sd = hx.seeded_state_dict(params, seed)
    ref = hx.oracle_model(params, sd, chunks=0)
    rs = np.random.RandomState(SEED)
    prompts = [rs.randint(0, params["vocab_size"], size=n).tolist() for n in LENS]
    stops = sorted({int(t) for t in rs.randint(0, 515, size=40)})
    memo, absmax = {}, [0.0]

    def step_logprobs(tokens):
        key = tuple(tokens)
        if key not in memo:
            with torch.no_grad():
                row = ref(torch.tensor(tokens, dtype=torch.int64)[None])[0][-1].double()
            absmax[0] = max(absmax[0], float(row.abs().max()))
            memo[key] = torch.log_softmax(row, -1).tolist()
        return memo[key]

    return params, sd, prompts, stops, step_logprobs, absmax, hip_model(params, sd)


@pytest.fixture(scope="module")
def oracle(setup):
    """The restatement's pools (all of them: n_best = W) per length penalty, with the margin condition asserted."""
    params, sd, prompts, stops, step_logprobs, absmax, _ = setup
    want = {}
    for pen in (1.0, 0.0):
        runs = []
        for p in prompts:
            tr = {}
            hyps = br.beam_search_ref(step_logprobs, p, beam_width=W, max_new_tokens=MAX_NEW, stop_token_ids=stops, length_penalty=pen, n_best=W, trace=tr)
            runs.append((hyps, tr))
        want[pen] = runs
    need = 1e-3 * absmax[0]
    for pen, runs in want.items():
        for p, (hyps, tr) in zip(prompts, runs):
            assert min(tr["cont_gaps"]) >= need, f"penalty {pen}, prompt of {len(p)}: continuation gap {min(tr['cont_gaps']):.3e} < {need:.3e}"
            assert min(tr["merged_gaps"]) >= need, f"penalty {pen}, prompt of {len(p)}: merged gap {min(tr['merged_gaps']):.3e} < {need:.3e}"
            assert min(tr["final_gaps"]) >= 1e-3, f"penalty {pen}, prompt of {len(p)}: final gap {min(tr['final_gaps']):.3e}"
    dones = [tr["done_at"] for _, tr in want[1.0]]
    assert sum(d is not None for d in dones) == 2 and sum(d is None for d in dones) == 2      # both ends of rule 6 are walked
    print(f"margin: absmax {absmax[0]:.3f}, smallest step gap {min(min(tr['cont_gaps'] + tr['merged_gaps']) for _, tr in want[1.0]):.3e}, "
          f"smallest final gap {min(min(tr['final_gaps']) for _, tr in want[1.0]):.3e}, pools full after steps {dones}")
    return want


def same(got, hyps, n_best, prompt_len):
    assert len(got) == n_best
    for g, h in zip(got, hyps[:n_best]):
        assert g.token_ids == h.token_ids and g.finish_reason == h.finish_reason and g.stop_reason == h.stop_reason
        assert abs(g.score - h.score) <= 1e-4 and abs(g.cumulative_logprob - h.cumulative_logprob) <= 1e-4 * max(1.0, len(h.token_ids))
        assert g.prompt_len == prompt_len and g.n_constrained is None


@pytest.mark.parametrize("n_best", (1, 3))
@pytest.mark.parametrize("pen", (1.0, 0.0))
def test_hypotheses_equal_the_restatement_on_the_oracle(setup, oracle, pen, n_best):
    from ssi.generate import beam_search
    params, sd, prompts, stops, _, _, model = setup
    kw = dict(beam_width=W, max_new_tokens=MAX_NEW, stop_token_ids=stops, pad_id=0, length_penalty=pen, n_best=n_best)
    found = beam_search(model, prompts, **kw)
    assert len(found) == len(prompts)
    for p, got, (hyps, _) in zip(prompts, found, oracle[pen]):
        same(got, hyps, n_best, len(p))
        assert [g.score for g in got] == sorted((g.score for g in got), reverse=True)
    assert model.training                                                      # (put back as it was found)
    if n_best == 3:                                                            # shuffled, and two prompts to a group: the same per prompt
        order = [2, 0, 3, 1]
        shuffled = beam_search(model, [prompts[i] for i in order], **kw)
        for i, got in zip(order, shuffled):
            same(got, oracle[pen][i][0], n_best, len(prompts[i]))
        small = beam_search(model, prompts, batch_size=2 * W + 1, **kw)
        for p, got, (hyps, _) in zip(prompts, small, oracle[pen]):
            same(got, hyps, n_best, len(p))


def test_min_new_tokens_and_an_allowed_set_are_honoured(setup):
    from ssi.generate import beam_search
    params, sd, prompts, stops, _, _, model = setup
    V, m = params["vocab_size"], 4
    allowed = [t for t in range(0, V, 2)]
    found = beam_search(model, prompts, beam_width=W, max_new_tokens=MAX_NEW, stop_token_ids=stops, pad_id=0, n_best=W,
                        allowed_token_ids=allowed, min_new_tokens=m)
    ok = set(allowed) | set(stops)
    for got in found:
        assert len(got) == W
        for g in got:
            assert all(t in ok for t in g.token_ids) and not set(g.token_ids[:m]) & set(stops)
            assert not set(g.token_ids[:-1]) & set(stops)                      # a stop token ends a hypothesis wherever it stands
            assert (g.finish_reason == "stop") == (g.token_ids[-1] in stops) and m < len(g.token_ids) <= MAX_NEW
            assert g.finish_reason == "stop" or len(g.token_ids) == MAX_NEW
            assert g.cumulative_logprob < 0 and abs(g.score - g.cumulative_logprob / len(g.token_ids)) <= 1e-5 * abs(g.score)


def test_beam_width_one_is_greedy(setup):
    from ssi.generate import beam_search, generate
    params, sd, prompts, stops, _, _, model = setup
    for stop in (stops, []):
        greedy = generate(model, prompts, max_new_tokens=MAX_NEW, stop_token_ids=stop, pad_id=0, logprobs=True)
        beam = beam_search(model, prompts, beam_width=1, max_new_tokens=MAX_NEW, stop_token_ids=stop, pad_id=0)
        for g, b in zip(greedy, beam):
            assert len(b) == 1 and b[0].token_ids == g.token_ids and b[0].finish_reason == g.finish_reason and b[0].stop_reason == g.stop_reason
            assert abs(b[0].cumulative_logprob - g.cumulative_logprob) <= 1e-4


def test_beam_width_one_is_greedy_on_the_padded_bf16_path():
    """An MFMA-shaped bf16 model pads a step to 256 rows with inert rows: the attention is bit-equal to the greedy step's, so are the tokens."""
    from ssi.generate import beam_search, generate
    params = dict(vocab_size=700, num_layers=2, num_heads=8, num_kv_heads=2, embed_dim=512, max_seq_len=512, intermediate_dim=512)
    model = hip_model(params, hx.seeded_state_dict(params, 21), torch.bfloat16)
    assert model._mfma_shapes()
    rs = np.random.RandomState(SEED)
    prompts = [rs.randint(0, 700, size=n).tolist() for n in LENS + (40,)]
    greedy = generate(model, prompts, max_new_tokens=10, stop_token_ids=[3, 5], pad_id=0)
    beam = beam_search(model, prompts, beam_width=1, max_new_tokens=10, stop_token_ids=[3, 5], pad_id=0)
    assert [b[0].token_ids for b in beam] == [g.token_ids for g in greedy]
    wide = beam_search(model, prompts, beam_width=4, max_new_tokens=10, stop_token_ids=[3, 5], pad_id=0, n_best=4)
    for got in wide:
        assert len(got) == 4 and [h.score for h in got] == sorted((h.score for h in got), reverse=True)
        assert len({tuple(h.token_ids) for h in got}) == 4                      # distinct hypotheses


def test_the_steps_leave_no_cache_error(setup):
    """``beam_search`` raises on ``cache.errors != 0``; here the two caches of a hand-driven step are looked at directly."""
    params, sd, prompts, stops, _, _, model = setup
    model.eval()
    n = len(prompts)
    pcache, bcache = model.new_kv_cache(n, max(LENS)), model.new_kv_cache(n * W, 4)
    with torch.inference_mode():
        logits = model.prefill(pcache, prompts)
        tok = logits[:, :params["vocab_size"]].argmax(-1).repeat_interleave(W)
        anc = torch.zeros((n * W, 4), dtype=torch.int32, device=DEV)
        own = torch.arange(n * W, dtype=torch.int32, device=DEV)
        plen = torch.tensor(LENS, dtype=torch.int32, device=DEV).repeat_interleave(W)
        anc[:, 0] = own
        l0 = model.decode_step_beam(pcache, bcache, tok, own // W, plen, anc, 0)
        anc[:, 1] = own
        anc[:, 0] = own // W * W                                               # every beam descends from beam 0 of its prompt
        l1 = model.decode_step_beam(pcache, bcache, tok, own // W, plen, anc, 1)
    model.train()
    assert int(pcache.errors) == 0 and int(bcache.errors) == 0
    assert l0.shape == (n * W, model.vocab_pad) and torch.equal(l0[0], l0[1]) and torch.equal(l1[0], l1[2])      # equal inputs, equal rows
    with pytest.raises(ValueError):
        model.decode_step_beam(pcache, bcache, tok, own // W, plen, anc, 4)                                      # beyond the beam cache


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


def test_a_training_step_is_bit_equal_with_a_beam_search_inside_it(setup):
    from ssi.generate import beam_search
    params, sd, prompts, stops, _, _, _ = setup
    _, b, s, seed = hx.CASES["tiny"]
    dbatch = {k: v.to(DEV) for k, v in hx.seeded_batch(params["vocab_size"], b, s, seed).items()}

    def search(model):
        out = beam_search(model, prompts, beam_width=W, max_new_tokens=6, stop_token_ids=[], pad_id=0, n_best=W)
        assert all(len(g) == W and all(len(h.token_ids) == 6 for h in g) for g in out)

    loss0, grad0 = _step(hip_model(params, sd), dbatch)
    mid = hip_model(params, sd)
    loss1, grad1 = _step(mid, dbatch, between=lambda: search(mid))
    assert torch.equal(loss1, loss0) and torch.equal(grad1, grad0)
    assert bool(torch.isfinite(grad0).all()) and float(grad0.abs().max()) > 0
