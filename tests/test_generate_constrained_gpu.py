"""Constrained greedy generation (``ssi.generate.generate`` with ``allowed_token_ids`` / ``min_new_tokens``, tokens from
``ops.decode_select``) against a constrained greedy continuation of ``OracleLlama`` by full recompute on the CPU, restated here: fp32 on
``hx.CASES["tiny"]`` (V = 515), the prompts of ``test_generate_model_gpu.py`` (seed 5, lengths 3, 9, 1, 14), 24 new tokens.

Settings: (a) allowed = [128, 320), no stop tokens; (b) the same with stop tokens 188 and 309; (c) the same with ``min_new_tokens = 10``.
In every setting the oracle's chosen token leads the allowed runner-up by more than ``1e-3 * logits_absmax`` at EVERY step (asserted, no step
left out: the condition under which equal tokens are a fair demand of an fp32 model within 1e-4), the constraint binds on some steps of every
row and, in (c), a stop token is held back on some steps (both asserted non-zero).  Tokens, finish reasons and ``n_constrained`` equal the
oracle's; ``cumulative_logprob`` is within 1e-5 relative of the oracle's UNMASKED ``log_softmax`` sum.

Also: an all-true mask reproduces the unconstrained ``generate``; shuffled prompts and groups of three; ``score_sequences`` on prompt +
generation reproduces ``cumulative_logprob``; a constrained ``generate`` between a training forward and its backward leaves loss and
gradients bit-equal."""
import numpy as np
import pytest
import torch

from oracle import hf_crosscheck as hx

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PROMPT_SEED, PROMPT_LENS, MAX_NEW = 5, (3, 9, 1, 14), 24
ALLOWED = (128, 320)                              # [first, last + 1)
STOPS = (188, 309)
SETTINGS = {"a": dict(stops=(), min_new=0), "b": dict(stops=STOPS, min_new=0), "c": dict(stops=STOPS, min_new=10)}


def hip_model(params, sd, dtype=torch.float32):
    from ssi.model import HipLlamaDecoder
    m = HipLlamaDecoder(**params, dtype=dtype, device=DEV)
    m.load_state_dict(sd)
    return m


def prompts_of(vocab):
    rs = np.random.RandomState(PROMPT_SEED)
    return [rs.randint(0, vocab, size=n).tolist() for n in PROMPT_LENS]


def allowed_ids():
    return list(range(*ALLOWED))


def oracle_constrained(ref, prompt, n_new, allowed, stops, min_new):
    """Constrained greedy continuation by full recompute.  ``allowed``: bool [V] WITHOUT the stop tokens, which are allowed from the
    ``min_new``-th token on.  Returns a dict: tokens, finish (reason, stop token), the smallest lead of the chosen token over the allowed
    runner-up, the largest |logit|, the unmasked log-probabilities, the steps on which the constraint changed the choice, and the steps on
    which a stop token would have been chosen had ``min_new`` not held it back."""
    V = allowed.numel()
    stop_mask = torch.zeros(V, dtype=torch.bool)
    if stops:
        stop_mask[list(stops)] = True
    toks, out = list(prompt), dict(tokens=[], lead=float("inf"), absmax=0.0, lps=[], binding=0, held=0, finish=("length", None))
    for t in range(n_new):
        with torch.no_grad():
            row = ref(torch.tensor(toks, dtype=torch.int64)[None])[0, -1].double()
        late = allowed | stop_mask
        mask = (allowed & ~stop_mask) if t < min_new else late
        masked = torch.where(mask, row, torch.full_like(row, -float("inf")))
        tok = int(masked.argmax())
        top = masked.topk(2).values
        out["lead"] = min(out["lead"], float(top[0] - top[1]))
        out["absmax"] = max(out["absmax"], float(row.abs().max()))
        out["lps"].append(float(torch.log_softmax(row, -1)[tok]))
        out["binding"] += int(tok != int(row.argmax()))
        if t < min_new:
            late_tok = int(torch.where(late, row, torch.full_like(row, -float("inf"))).argmax())
            out["held"] += int(bool(stop_mask[late_tok]))
        out["tokens"].append(tok)
        toks.append(tok)
        if bool(stop_mask[tok]):
            out["finish"] = ("stop", tok)
            break
    return out


@pytest.fixture(scope="module")
def world():
    """The oracle's continuations of every setting, computed once, and the model."""
    params, _, _, seed = hx.CASES["tiny"]
    sd = hx.seeded_state_dict(params, seed)
    ref = hx.oracle_model(params, sd, chunks=0)
    V = params["vocab_size"]
    prompts = prompts_of(V)
    allowed = torch.zeros(V, dtype=torch.bool)
    allowed[ALLOWED[0]:ALLOWED[1]] = True
    want = {k: [oracle_constrained(ref, p, MAX_NEW, allowed, s["stops"], s["min_new"]) for p in prompts] for k, s in SETTINGS.items()}
    return params, sd, prompts, want, hip_model(params, sd)


def run(model, prompts, setting, **kw):
    from ssi.generate import generate
    s = SETTINGS[setting]
    return generate(model, prompts, max_new_tokens=MAX_NEW, stop_token_ids=list(s["stops"]), pad_id=0, allowed_token_ids=allowed_ids(),
                    min_new_tokens=s["min_new"], **kw)


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_constrained_tokens_equal_the_oracles(world, setting):
    params, sd, prompts, want, model = world
    w = want[setting]
    absmax = max(x["absmax"] for x in w)
    for p, x in zip(prompts, w):
        print(f"({setting}) prompt of {len(p)}: lead {x['lead'] / absmax:.3e} of absmax, binding {x['binding']}, held back {x['held']}, "
              f"{len(x['tokens'])} tokens, {x['finish']}")
        assert x["lead"] > 1e-3 * absmax, f"prompt of {len(p)}: the chosen token leads by {x['lead']:.3e}, needs {1e-3 * absmax:.3e}"
        assert x["binding"] > 0
    if setting == "b":
        assert any(x["finish"][0] == "stop" for x in w)
    if setting == "c":
        assert sum(x["held"] for x in w) > 0 and any(x["held"] > 0 and len(x["tokens"]) > SETTINGS["c"]["min_new"] for x in w)
    gens = run(model, prompts, setting, logprobs=True)
    for p, g, x in zip(prompts, gens, w):
        assert g.token_ids == x["tokens"] and (g.finish_reason, g.stop_reason) == x["finish"] and g.prompt_len == len(p)
        assert g.n_constrained == x["binding"]
        assert abs(g.cumulative_logprob - sum(x["lps"])) <= 1e-5 * abs(sum(x["lps"]))
        assert all(ALLOWED[0] <= t < ALLOWED[1] or t in STOPS for t in g.token_ids)
    assert model.training
    # shuffled, and in groups of three: the same per prompt
    order = [2, 0, 3, 1]
    shuffled = run(model, [prompts[i] for i in order], setting)
    assert [g.token_ids for g in shuffled] == [w[i]["tokens"] for i in order]
    assert [g.n_constrained for g in shuffled] == [w[i]["binding"] for i in order] and all(g.cumulative_logprob is None for g in shuffled)
    small = run(model, prompts, setting, batch_size=3)
    assert [g.token_ids for g in small] == [x["tokens"] for x in w] and [g.n_constrained for g in small] == [x["binding"] for x in w]


def test_an_all_true_mask_is_the_unconstrained_generation(world):
    from ssi.generate import generate
    params, sd, prompts, _, model = world
    kw = dict(max_new_tokens=MAX_NEW, stop_token_ids=[], pad_id=0, logprobs=True)
    plain = generate(model, prompts, **kw)
    full = generate(model, prompts, allowed_token_ids=torch.ones(params["vocab_size"], dtype=torch.bool), **kw)
    assert [g.token_ids for g in full] == [g.token_ids for g in plain]
    assert [g.n_constrained for g in full] == [0] * len(prompts) and all(g.n_constrained is None for g in plain)
    for f, p in zip(full, plain):
        assert abs(f.cumulative_logprob - p.cumulative_logprob) <= 1e-5 * abs(p.cumulative_logprob)
    only_min = generate(model, prompts, min_new_tokens=3, **kw)                  # no stop tokens: nothing to hold back
    assert [g.token_ids for g in only_min] == [g.token_ids for g in plain] and [g.n_constrained for g in only_min] == [0] * len(prompts)


def test_scoring_the_generation_reproduces_its_logprob(world):
    from ssi.score import score_sequences
    params, sd, prompts, _, model = world
    gens = run(model, prompts, "c", logprobs=True)
    seqs = [p + g.token_ids for p, g in zip(prompts, gens)]
    scores = score_sequences(model, seqs, score_from=[len(p) for p in prompts], pad_id=0, device=DEV, row_len=64)
    assert scores.n_tokens.tolist() == [len(g.token_ids) for g in gens]
    for i, g in enumerate(gens):
        assert abs(g.cumulative_logprob - float(scores.logprob[i])) <= 1e-5 * abs(g.cumulative_logprob)


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


def test_a_training_step_is_bit_equal_with_constrained_generation_inside_it(world):
    params, sd, prompts, _, _ = world
    _, b, s, seed = hx.CASES["tiny"]
    dbatch = {k: v.to(DEV) for k, v in hx.seeded_batch(params["vocab_size"], b, s, seed).items()}

    def gen(model):
        out = run(model, prompts, "c", logprobs=True)
        assert all(len(g.token_ids) >= SETTINGS["c"]["min_new"] for g in out)

    loss0, grad0 = _step(hip_model(params, sd), dbatch)
    mid = hip_model(params, sd)
    loss1, grad1 = _step(mid, dbatch, between=lambda: gen(mid))
    assert torch.equal(loss1, loss0) and torch.equal(grad1, grad0)
    assert bool(torch.isfinite(grad0.float()).all()) and float(grad0.float().abs().max()) > 0
