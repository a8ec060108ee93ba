"""Continuous batching on the model (``generate`` / ``sample(n=1)`` with ``continuous=True``: a pool of rows refilled as sequences finish).

(a) fp32 ``tiny``, greedy, 10 prompts of varied length in a pool of 3 with a stop set chosen on the CPU: tokens, finish reasons and
    ``cumulative_logprob`` against the oracle's greedy continuation by full recompute, under the margin condition of
    tests/test_generate_model_gpu.py (the oracle's top-1 leads its top-2 by more than ``1e-3 * logits_absmax`` at every step), which ALL ten
    prompts meet on the oracle (asserted, none left out).  The test asserts that the refill path runs: at least three distinct generated
    lengths, at least one row that ends by length, at least two admissions after the first; and that the schedule the device arrived at is
    the host simulation's for the lengths that came out.
(b) the same for ``sample(n=1)`` with a temperature per prompt, against the continuation that draws with the reference sampler of
    tests/decode_sample_ref.py, under the conditions of tests/test_sample_model_gpu.py.
(c) the bf16 model of tests/test_small_batch_model_gpu.py: a small-batch pool admits prompt by prompt, skinny rows do not depend on their
    neighbours and a sample is a pure function of (seed, input index, step), so a prompt's tokens and ``cumulative_logprob`` are BIT-EQUAL
    to the static small-batch run's — at pools of 2 and 5, ``admit_min`` 1 and 2 and shuffled input, greedy under a constraint and sampled
    under penalties.
(d) a training step is bit-equal with a continuous ``generate`` between its forward and its backward."""
import numpy as np
import pytest
import torch

import decode_sample_ref as S
from oracle import hf_crosscheck as hx

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENS = (3, 9, 1, 14, 6, 2, 11, 4, 8, 5)
POOL = 3
# chosen on the CPU: with these prompts the oracle alone meets the conditions of the two tests, and these stop sets spread the lengths
GREEDY_PROMPT_SEED, GREEDY_MAX_NEW, GREEDY_STOPS = 0, 20, (115, 203, 243, 300)             # lengths 7 1 1 20 3 20 20 2 12 20
SAMPLE_PROMPT_SEED, SAMPLE_MAX_NEW, SAMPLE_STOPS, SEED = 7, 12, (178, 221, 354, 405), 2027      # lengths 12 7 9 1 11 12 8 12 10 5
TEMPS = (0.7, 0.8, 1.0, 1.2, 0.9, 1.1, 0.75, 1.3, 0.85, 1.0)
TOP_K, TOP_P = 20, 0.9


def prompts_of(seed, vocab):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, vocab, size=n).tolist() for n in LENS]


def cut(tokens, stops):
    """(the tokens up to and including the first stop token, the finish reason, the stop reason)"""
    for k, t in enumerate(tokens):
        if t in stops:
            return tokens[:k + 1], "stop", t
    return tokens, "length", None


def oracle_sample(ref, prompt, n_new, sequence, T, stops):
    """tests/test_sample_model_gpu.py's continuation with the prompt's own temperature, ended at a stop token: (tokens, log-probabilities,
    smallest score gap * T / |logit|max, the thresholds are stable)."""
    toks, lps, lead, stable = list(prompt), [], np.inf, True
    for t in range(n_new):
        with torch.no_grad():
            row = ref(torch.tensor(toks, dtype=torch.int64)[None])[0][-1].double()
        V, M = row.numel(), np.ones((1, row.numel()), dtype=bool)
        case = S.Case(row[None, :].float(), V, seqs=[sequence], seed=SEED, step=t)
        exp = case.expected(M, T, TOP_K, TOP_P)
        tok, absmax = int(exp.token[0]), float(row.abs().max())
        lead = min(lead, float(exp.gap[0]) * T / absmax)
        dp = 1e-3 * absmax / T
        top = torch.sort(row, descending=True).values
        near = [kk for kk in (TOP_K - 1, TOP_K + 1) if float(top[min(TOP_K, kk) - 1] - top[min(TOP_K, kk)]) < 2e-3 * absmax]
        for kk, pp in [(kk, TOP_P) for kk in near] + [(TOP_K, TOP_P - dp), (TOP_K, min(TOP_P + dp, 1.0))]:
            stable = stable and int(case.expected(M, T, kk, pp).token[0]) == tok
        lps.append(float(torch.log_softmax(row, -1)[tok]))
        toks.append(tok)
        if tok in stops:
            break
    return toks[len(prompt):], lps, lead, stable


@pytest.fixture(scope="module")
def base():
    import test_generate_model_gpu as g
    return g


@pytest.fixture(scope="module")
def tiny(base):
    params, _, _, seed = hx.CASES["tiny"]
    sd = hx.seeded_state_dict(params, seed)
    return params, hx.oracle_model(params, sd, chunks=0), base.hip_model(params, sd)


def refill_ran(gens, stats, max_new, admit_min):
    """What guarantees that the refill path ran, and that the device's schedule is the host simulation's for these lengths."""
    from ssi.generate import plan_groups, simulate_pool
    n = [len(g.token_ids) for g in gens]
    assert len(set(n)) >= 3 and any(g.finish_reason == "length" for g in gens) and stats["admissions"] >= 3, (n, stats)
    order = [i for grp in plan_groups([g.prompt_len for g in gens], POOL) for i in grp]
    sim = simulate_pool(n, order, POOL, admit_min, max_new)
    assert stats == dict(sim.report(), continuous=True), (stats, sim.report())
    assert stats["row_steps_live"] == sum(n) and stats["row_steps_total"] == POOL * stats["decode_steps"]


def test_greedy_pool_of_3_equals_the_oracles_continuations(base, tiny):
    from ssi.generate import generate
    params, ref, model = tiny
    prompts = prompts_of(GREEDY_PROMPT_SEED, params["vocab_size"])
    want = [base.oracle_greedy(ref, p, GREEDY_MAX_NEW) for p in prompts]
    absmax = max(w[2] for w in want)
    for p, w in zip(prompts, want):                       # every prompt, every step: none is left out
        assert w[1] > 1e-3 * absmax, f"prompt of {len(p)}: the oracle's top-1 leads by {w[1]:.3e}, needs {1e-3 * absmax:.3e}"
    for admit_min in (1, 2):
        stats = {}
        gens = generate(model, prompts, max_new_tokens=GREEDY_MAX_NEW, stop_token_ids=list(GREEDY_STOPS), pad_id=0, logprobs=True, batch_size=POOL,
                        continuous=True, admit_min=admit_min, continuous_report=stats)
        for i, (p, g, w) in enumerate(zip(prompts, gens, want)):
            toks, reason, stop = cut(w[0], GREEDY_STOPS)
            assert (g.token_ids, g.finish_reason, g.stop_reason, g.prompt_len) == (toks, reason, stop, len(p)), (admit_min, i)
            lp = sum(w[3][:len(toks)])
            assert abs(g.cumulative_logprob - lp) <= 1e-5 * abs(lp), (admit_min, i)
        refill_ran(gens, stats, GREEDY_MAX_NEW, admit_min)
    assert model.training                                  # (put back as it was found)
    # no stop set: every row runs to the length, and the pool takes the steps of the static groups
    stats = {}
    gens = generate(model, prompts, max_new_tokens=6, stop_token_ids=[], pad_id=0, batch_size=POOL, continuous=True, continuous_report=stats)
    assert [g.token_ids for g in gens] == [w[0][:6] for w in want] and all(g.finish_reason == "length" for g in gens)
    assert stats["decode_steps"] == 4 * 6 and stats["row_steps_live"] == 60 and stats["admissions"] == 4


def test_sampled_pool_of_3_with_a_temperature_per_prompt_equals_the_reference_draws(tiny):
    from ssi.generate import sample
    params, ref, model = tiny
    prompts = prompts_of(SAMPLE_PROMPT_SEED, params["vocab_size"])
    want = [oracle_sample(ref, p, SAMPLE_MAX_NEW, i, TEMPS[i], SAMPLE_STOPS) for i, p in enumerate(prompts)]
    for i, w in enumerate(want):
        assert w[2] > 1e-3 and w[3], f"prompt {i}: lead {w[2]:.3e} of the largest logit, stable thresholds {w[3]}"
    kw = dict(seed=SEED, max_new_tokens=SAMPLE_MAX_NEW, stop_token_ids=list(SAMPLE_STOPS), pad_id=0, temperature=list(TEMPS), top_k=TOP_K,
              top_p=TOP_P, batch_size=POOL)
    stats = {}
    got = sample(model, prompts, continuous=True, admit_min=1, continuous_report=stats, **kw)
    static = sample(model, prompts, **kw)                  # the static groups with the same per-prompt list: the _rows entries there, too
    for which, found in (("continuous", got), ("static", static)):
        for i, (gs, w) in enumerate(zip(found, want)):
            toks, reason, stop = cut(w[0], SAMPLE_STOPS)
            assert len(gs) == 1 and (gs[0].token_ids, gs[0].finish_reason, gs[0].stop_reason) == (toks, reason, stop), (which, i)
            lp = sum(w[1][:len(toks)])
            assert abs(gs[0].cumulative_logprob - lp) <= 1e-5 * abs(lp), (which, i)
            assert 1.0 <= gs[0].n_kept_mean <= TOP_K
    refill_ran([gs[0] for gs in got], stats, SAMPLE_MAX_NEW, 1)


# ---- (c) bit-equality with the static small-batch run ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mfma(base):
    model = base.hip_model(base.MFMA_PARAMS, hx.seeded_state_dict(base.MFMA_PARAMS, 21), torch.bfloat16)
    assert model._mfma_shapes() and model.takes_small_batch(5, True)
    return model


def _spread_prompts():
    rs = np.random.RandomState(17)
    return [rs.randint(0, 700, size=int(rs.randint(2, 30))).tolist() for _ in range(11)]


def _fields(g):
    return g.token_ids, g.finish_reason, g.stop_reason, g.cumulative_logprob, g.n_constrained, g.n_kept_mean, g.prompt_len


def _spread(gens):
    n = [len(g.token_ids) for g in gens]
    assert len(set(n)) >= 3 and any(g.finish_reason == "length" for g in gens) and any(g.finish_reason == "stop" for g in gens), n


def test_small_batch_pools_are_bit_equal_to_the_static_small_batch_run_greedy_constrained(mfma):
    from ssi.generate import generate
    prompts = _spread_prompts()
    kw = dict(max_new_tokens=20, stop_token_ids=list(range(100, 700, 9)), pad_id=0, logprobs=True, small_batch=True,
              allowed_token_ids=list(range(100, 700)), min_new_tokens=2)
    report = {}
    static = generate(mfma, prompts, small_batch_report=report, **kw)
    assert report["small_batch_groups"] == 1
    _spread(static)
    order = [7, 2, 10, 0, 5, 9, 1, 8, 3, 6, 4]
    for pool, admit_min, perm in ((2, 1, None), (5, 2, None), (5, 1, order), (2, 2, order)):
        at = perm or list(range(len(prompts)))
        stats, report = {}, {}
        got = generate(mfma, [prompts[i] for i in at], batch_size=pool, continuous=True, admit_min=admit_min, continuous_report=stats,
                       small_batch_report=report, **kw)
        assert [_fields(g) for g in got] == [_fields(static[i]) for i in at], (pool, admit_min, perm)
        assert stats["admissions"] >= 3 and report["small_batch_groups"] == 1
    plain = generate(mfma, prompts, batch_size=5, continuous=True, **dict(kw, allowed_token_ids=None, min_new_tokens=0))      # the argmax chooser
    assert [_fields(g) for g in plain] == [_fields(g) for g in generate(mfma, prompts, **dict(kw, allowed_token_ids=None, min_new_tokens=0))]


def test_small_batch_pools_are_bit_equal_to_the_static_small_batch_run_sampled_with_penalties(mfma):
    from ssi.generate import sample
    prompts = _spread_prompts()
    kw = dict(temperature=0.9, top_k=50, top_p=0.95, seed=1234, max_new_tokens=20, stop_token_ids=list(range(0, 700, 29)), pad_id=0,
              small_batch=True, repetition_penalty=1.2, frequency_penalty=0.3, presence_penalty=-0.2)
    static = [gs[0] for gs in sample(mfma, prompts, **kw)]
    _spread(static)
    order = [7, 2, 10, 0, 5, 9, 1, 8, 3, 6, 4]
    for pool, admit_min, perm in ((2, 1, None), (5, 2, None), (5, 1, order), (2, 2, order)):
        # (a sample is a function of the INPUT index: the shuffled call is compared with the static run of the same shuffled input)
        at = perm or list(range(len(prompts)))
        want = static if perm is None else [gs[0] for gs in sample(mfma, [prompts[i] for i in at], **kw)]
        stats = {}
        got = sample(mfma, [prompts[i] for i in at], batch_size=pool, continuous=True, admit_min=admit_min, continuous_report=stats, **kw)
        assert [_fields(gs[0]) for gs in got] == [_fields(g) for g in want], (pool, admit_min, perm)
        assert stats["admissions"] >= 3
    split = dict(kw, split_kv=True)                       # both on the split side of split_max_rows
    assert mfma.takes_split_kv(5, True) and mfma.takes_split_kv(len(prompts), True)
    assert [_fields(gs[0]) for gs in sample(mfma, prompts, batch_size=5, continuous=True, admit_min=1, **split)] == \
           [_fields(gs[0]) for gs in sample(mfma, prompts, **split)]


def test_the_fp8_cache_and_larger_pools_run_and_agree_with_the_schedule(mfma):
    """A packed pool (more rows than the skinny path takes) and an fp8 cache: held to the invariants of the loop, not to the static run's bits."""
    from ssi.generate import generate, plan_groups, simulate_pool
    rs = np.random.RandomState(3)
    prompts = [rs.randint(0, 700, size=int(rs.randint(2, 20))).tolist() for _ in range(150)]
    for kv in (None, "fp8"):
        stats = {}
        gens = generate(mfma, prompts, max_new_tokens=12, stop_token_ids=list(range(0, 700, 7)), pad_id=0, batch_size=70, continuous=True,
                        admit_min=8, continuous_report=stats, kv_cache_dtype=kv, logprobs=True)
        n = [len(g.token_ids) for g in gens]
        order = [i for grp in plan_groups([len(p) for p in prompts], 70) for i in grp]
        assert stats == dict(simulate_pool(n, order, 70, 8, 12).report(), continuous=True)
        for g in gens:
            stopped = [t % 7 == 0 for t in g.token_ids]
            assert 1 <= len(g.token_ids) <= 12 and not any(stopped[:-1]) and stopped[-1] == (g.finish_reason == "stop")
            assert g.cumulative_logprob < 0.0


# ---- (d) training is untouched ---------------------------------------------------------------------------------------------------------
def test_a_training_step_is_bit_equal_with_a_continuous_generate_inside_it(base):
    from ssi.generate import generate
    params, b, s, seed, dtype = base.MFMA_PARAMS, 2, 128, 21, torch.bfloat16
    sd = hx.seeded_state_dict(params, seed)
    dbatch = {k: v.to(DEV) for k, v in hx.seeded_batch(params["vocab_size"], b, s, seed).items()}
    prompts = _spread_prompts()

    def gen(model):
        stats = {}
        out = generate(model, prompts, max_new_tokens=10, stop_token_ids=list(range(0, 700, 9)), pad_id=0, logprobs=True, batch_size=3,
                       continuous=True, admit_min=1, continuous_report=stats)
        assert len(out) == len(prompts) and stats["admissions"] >= 3

    loss0, grad0 = base._step(base.hip_model(params, sd, dtype), dbatch)
    mid = base.hip_model(params, sd, dtype)
    loss1, grad1 = base._step(mid, dbatch, between=lambda: gen(mid))
    assert torch.equal(loss1, loss0) and torch.equal(grad1, grad0)
    assert bool(torch.isfinite(grad0.float()).all()) and float(grad0.float().abs().max()) > 0
