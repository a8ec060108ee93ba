"""The FP8 K/V cache on the model: ``new_kv_cache(..., dtype="fp8")``, ``prefill``, ``decode_step`` / ``decode_step_beam`` and the three loops of
``ssi.generate`` with ``kv_cache_dtype="fp8"``.

* teacher-forced walk (tests/test_generate_model_gpu.py's, its cache made fp8) against an INJECTED oracle: the cache is read back and dequantised on
  the host (kv_fp8_ref.py), and the CPU oracle recomputes every row in full with its attention patched here — queries at prompt positions attend
  over the oracle's own K / V (prefill attention runs on the unquantised K / V of the packed forward), queries at generated positions over the
  GPU's dequantised K / V.  What is left between the two is the arithmetic the existing walk tests bound, so the bounds are theirs: fp32 ``tiny``
  within ``1e-4 * logits_absmax``; bf16 on the MFMA shapes ``err <= 2.0 x`` the model's own full-forward error;
* separately, every cached line is a plausible quantisation of the oracle's: its exponent within one of the reference quantiser's on the oracle's
  line, every dequantised element within one e4m3 step (at that exponent) of the oracle's element (the exact rule is test_kv_store_fp8_gpu.py's);
* the loops: ``generate``, ``sample(n=2)`` and ``beam_search(beam_width=3)`` run on fp8 caches with ``errors == 0``; ``beam_search(beam_width=1)``
  returns ``generate``'s tokens; with ``small_batch`` and ``split_kv`` on, a prompt's tokens and ``cumulative_logprob`` are bit-equal alone and
  among 5; a training step is bit-equal with an fp8 generation between its forward and its backward;
* ``kv_cache_dtype="auto"`` and ``None`` give the tokens, log-probabilities and launches of a call without the argument, and an fp8 step differs from
  the plain step in the store and attention entries only."""
import contextlib

import numpy as np
import pytest
import torch

import kv_fp8_ref as kr
from oracle import hf_crosscheck as hx
from oracle import llama_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KW = dict(stop_token_ids=[], pad_id=0)


@pytest.fixture(scope="module")
def base():
    import test_generate_model_gpu as g
    return g


@contextlib.contextmanager
def fp8_caches(model):
    """Every cache ``model`` opens in the body is an fp8 cache; yields the list of them."""
    made, real = [], model.new_kv_cache

    def new(n_slots, cap, dtype=None):
        made.append(real(n_slots, cap, "fp8"))
        return made[-1]
    model.new_kv_cache = new
    try:
        yield made
    finally:
        del model.new_kv_cache


def dequantised(cache, model):
    """fp32 K and V ``[layers, n_slots, cap, n_kv, head_dim]`` of an fp8 cache, and its exponent bytes."""
    L, n, cap, KV, hd = model.num_layers, cache.n_slots, cache.cap, model.num_kv_heads, model.head_dim
    ke, ve = cache.k_exp.cpu(), cache.v_exp.cpu()
    return (kr.dequantise(cache.k.cpu().view(L, n, cap, KV, hd), ke), kr.dequantise(cache.v.cpu().view(L, n, cap, KV, hd), ve), ke, ve)


def injected_oracle_logits(ref, row, prompt_len, dk, dv):
    """The oracle's logits [S, V] (float64) for one row, by full recompute, with its attention patched: queries below ``prompt_len`` attend causally
    over the oracle's own K / V, the others over ``dk`` / ``dv`` ([layers, S, n_kv, head_dim], the GPU's dequantised cache lines of the row).  Also
    the oracle's own K (after RoPE) and V per layer, [layers, S, n_kv, head_dim]."""
    real = llama_oracle.F.scaled_dot_product_attention
    own_k, own_v = [], []

    def patched(q, k, v, attn_mask=None, dropout_p=0.0, is_causal=False):
        assert attn_mask is None and is_causal and q.shape[0] == 1
        layer, rep = len(own_k), q.shape[1] // dk.shape[2]
        own_k.append(k[0, ::rep].transpose(0, 1))                       # [S, n_kv, head_dim]
        own_v.append(v[0, ::rep].transpose(0, 1))
        gk = dk[layer].to(q.dtype).transpose(0, 1).repeat_interleave(rep, dim=0)[None]
        gv = dv[layer].to(q.dtype).transpose(0, 1).repeat_interleave(rep, dim=0)[None]
        mine, theirs = real(q, k, v, is_causal=True), real(q, gk, gv, is_causal=True)
        generated = (torch.arange(q.shape[2]) >= prompt_len)[None, None, :, None]
        return torch.where(generated, theirs, mine)

    llama_oracle.F.scaled_dot_product_attention = patched
    try:
        with torch.no_grad():
            logits = ref(row[None])[0].double()
    finally:
        llama_oracle.F.scaled_dot_product_attention = real
    return logits, torch.stack(own_k), torch.stack(own_v)


def walk(base, model, rows, lens):
    """The teacher-forced walk on an fp8 cache: its logits, and the cache."""
    with fp8_caches(model) as made:
        got = base.teacher_forced_walk(model, rows, lens)
    assert len(made) == 1 and made[0].dtype == "fp8" and int(made[0].errors) == 0
    return got, made[0]


def e4m3_step(y):
    """The spacing of e4m3 codes at magnitude ``y`` (float64)."""
    E = torch.frexp(y.abs().clamp(min=2.0 ** -6))[1] - 1
    return torch.exp2((E - 3).double())


def plausible(deq, exps, own, what):
    """Every cached line [.., n_kv, head_dim] against the oracle's: exponent within one of the reference's, elements within one e4m3 step."""
    _, b_ref = kr.quantise(own.float())
    assert int((exps.long() - b_ref.long()).abs().max()) <= 1, what
    scale = torch.exp2(127.0 - exps.double())[..., None]
    y_got, y_own = deq.double() * scale, own.double() * scale
    over = (y_got - y_own).abs() > e4m3_step(torch.maximum(y_got.abs(), y_own.abs()))
    assert not bool(over.any()), (what, int(over.sum()))


def test_teacher_forced_logits_fp32_against_the_injected_oracle(base):
    params, b, s, seed = hx.CASES["tiny"]
    sd = hx.seeded_state_dict(params, seed)
    rows = list(hx.seeded_batch(params["vocab_size"], b, s, seed)["tokens"])
    lens = (1, 17)
    ref = hx.oracle_model(params, sd, chunks=0)
    model = base.hip_model(params, sd)
    got, cache = walk(base, model, rows, lens)
    dk, dv, ke, ve = dequantised(cache, model)
    want, absmax = [], 0.0
    for i, row in enumerate(rows):
        logits, own_k, own_v = injected_oracle_logits(ref, row, lens[i], dk[:, i, :s], dv[:, i, :s])
        want.append(logits)
        absmax = max(absmax, float(logits.abs().max()))
        plausible(dk[:, i, :s], ke[:, i, :s], own_k, f"K of row {i}")
        plausible(dv[:, i, :s], ve[:, i, :s], own_v, f"V of row {i}")
    plain = max(float((g.double() - base.oracle_logits(ref, rows[i])[pos]).abs().max()) for i, pos, g in got)
    worst = max(float((g.double() - want[i][pos]).abs().max()) for i, pos, g in got)
    print(f"tiny fp32, fp8 cache: decode logits max-abs error {worst:.3e} against the injected oracle (tolerance {1e-4 * absmax:.3e}); "
          f"{plain:.3e} against the unquantised oracle")
    assert worst <= 1e-4 * absmax
    assert plain > 1e-4 * absmax                                         # the cache does change values: the injection is what the bound needs


def test_teacher_forced_logits_bf16_on_the_mfma_path_against_the_injected_oracle(base):
    params, seed, S = base.MFMA_PARAMS, 21, 40
    sd = hx.seeded_state_dict(params, seed)
    rs = np.random.RandomState(seed + 1)
    rows = list(torch.from_numpy(rs.randint(0, params["vocab_size"], size=(5, S)).astype(np.int64)))
    lens = (1, 17, 5, 9, 30)
    ref = hx.oracle_model(params, sd, chunks=0)
    model = base.hip_model(params, sd, torch.bfloat16)
    assert model._mfma_shapes()
    model.eval()
    with torch.no_grad():
        full = model(tokens=torch.stack(rows).to(DEV)).double().cpu()
    full_err = max(float((full[i] - base.oracle_logits(ref, rows[i])).abs().max()) for i in range(5))
    got, cache = walk(base, model, rows, lens)
    dk, dv, _, _ = dequantised(cache, model)
    want = [injected_oracle_logits(ref, rows[i], lens[i], dk[:, i, :S], dv[:, i, :S])[0] for i in range(5)]
    dec_err = max(float((g.double() - want[i][pos]).abs().max()) for i, pos, g in got)
    print(f"bf16, fp8 cache: decode {dec_err:.4e} from the injected oracle, own full forward {full_err:.4e} from the fp32 oracle "
          f"(ratio {dec_err / full_err:.2f})")
    assert dec_err <= 2.0 * full_err


# ---- the loops -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny32(base):
    params, _, _, seed = hx.CASES["tiny"]
    params = dict(params, max_seq_len=512)
    model = base.hip_model(params, hx.seeded_state_dict(params, seed))
    model.eval()
    return model


@pytest.fixture(scope="module")
def mfma(base):
    model = base.hip_model(base.MFMA_PARAMS, hx.seeded_state_dict(base.MFMA_PARAMS, 21), torch.bfloat16)
    assert model._mfma_shapes() and model.head_dim == 64
    model.split_span = 64
    model.eval()
    return model


def prompts_of(n, seed=7, lo=20, hi=90):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 500, size=int(rs.randint(lo, hi))).tolist() for _ in range(n)]


def spy_caches(model):
    made, real = [], model.new_kv_cache

    def new(*a, **k):
        made.append(real(*a, **k))
        return made[-1]
    model.new_kv_cache = new
    return made


def test_the_three_loops_run_on_fp8_caches_without_errors(tiny32):
    from ssi.generate import beam_search, generate, sample
    model, prompts = tiny32, prompts_of(4)
    made = spy_caches(model)
    try:
        g = generate(model, prompts, max_new_tokens=9, logprobs=True, kv_cache_dtype="fp8", **KW)
        s = sample(model, prompts, n=2, temperature=0.8, seed=5, max_new_tokens=9, kv_cache_dtype="fp8", **KW)
        b = beam_search(model, prompts, beam_width=3, n_best=3, max_new_tokens=9, kv_cache_dtype="fp8", **KW)
        b1 = beam_search(model, prompts, beam_width=1, max_new_tokens=9, kv_cache_dtype="fp8", **KW)
    finally:
        del model.new_kv_cache
    assert len(made) == 1 + 2 + 2 + 2 and all(c.dtype == "fp8" and c.k.dtype == torch.uint8 and int(c.errors) == 0 for c in made)
    assert all(len(x.token_ids) == 9 for x in g) and all(len(xs) == 2 for xs in s) and all(len(xs) == 3 for xs in b)
    assert all(np.isfinite(x.cumulative_logprob) for x in g)
    assert [x[0].token_ids for x in b1] == [x.token_ids for x in g]      # a beam of one is the greedy path, under fp8 too
    plain = generate(model, prompts, max_new_tokens=9, logprobs=True, **KW)
    assert any(x.cumulative_logprob != y.cumulative_logprob for x, y in zip(g, plain))     # it is not a no-op


@pytest.mark.parametrize("which", ("tiny32", "mfma"))
def test_a_prompt_alone_and_among_5_with_small_batch_and_split_kv(request, which):
    from ssi.generate import generate
    model = request.getfixturevalue(which)
    prompts = prompts_of(5, seed=11, lo=70, hi=160)
    kw = dict(max_new_tokens=10, logprobs=True, small_batch=True, split_kv=True, kv_cache_dtype="fp8", **KW)
    report = {}
    alone = generate(model, prompts[:1], small_batch_report=report, **kw)[0]
    among = generate(model, prompts, **kw)[0]
    assert report.get("split_kv_groups") == 1 and (which == "tiny32" or report.get("small_batch_groups") == 1)
    assert among.token_ids == alone.token_ids and among.cumulative_logprob == alone.cumulative_logprob


def test_a_training_step_is_bit_equal_with_an_fp8_generation_inside_it(base):
    from ssi.generate import generate
    params, b, s, seed, dtype = base.MFMA_PARAMS, 2, 128, 21, torch.bfloat16
    sd = hx.seeded_state_dict(params, seed)
    dbatch = {k: v.to(DEV) for k, v in hx.seeded_batch(params["vocab_size"], b, s, seed).items()}
    prompts = prompts_of(3, seed=13)

    def gen(model):
        out = generate(model, prompts, max_new_tokens=10, logprobs=True, kv_cache_dtype="fp8", **KW)
        assert all(len(g.token_ids) == 10 for g in out)

    loss0, grad0 = base._step(base.hip_model(params, sd, dtype), dbatch)
    mid = base.hip_model(params, sd, dtype)
    loss1, grad1 = base._step(mid, dbatch, between=lambda: gen(mid))
    assert torch.equal(loss1, loss0) and torch.equal(grad1, grad0)
    assert bool(torch.isfinite(grad0.float()).all()) and float(grad0.float().abs().max()) > 0


# ---- dispatch --------------------------------------------------------------------------------------------------------------------------------------
def _traced(model, body):
    import launch_trace
    tr = launch_trace.Tracer()
    tr.watch(model)
    with tr.scenario():
        out = body()
    return tr.entries, out


def test_auto_and_none_are_the_call_without_the_argument(tiny32):
    from ssi.generate import generate
    model, prompts = tiny32, prompts_of(3, seed=17)
    kw = dict(max_new_tokens=6, logprobs=True, **KW)
    want_trace, want = _traced(model, lambda: generate(model, prompts, **kw))
    for value in (None, "auto"):
        trace, got = _traced(model, lambda: generate(model, prompts, kv_cache_dtype=value, **kw))
        assert trace == want_trace, value
        assert [(g.token_ids, g.cumulative_logprob) for g in got] == [(g.token_ids, g.cumulative_logprob) for g in want]
    names = {e[0] for e in want_trace}
    assert "kv_store" in names and "attn_decode" in names and not any(n.endswith("_fp8") for n in names)
    with pytest.raises(ValueError):
        generate(model, prompts, kv_cache_dtype="fp16", **kw)


@pytest.mark.parametrize("flags", ({}, {"split_kv": True}), ids=("plain", "split_kv"))
def test_an_fp8_step_differs_in_the_store_and_attention_entries_only(tiny32, flags):
    model = tiny32
    tok = torch.arange(3, dtype=torch.int64, device=DEV) + 11
    slot = torch.arange(3, dtype=torch.int32, device=DEV)

    def step(dtype):
        cache = model.new_kv_cache(3, 150, dtype)
        model.prefill(cache, [[3 + i, 5, 7] * 30 for i in range(3)], max_new_tokens=4)
        trace, _ = _traced(model, lambda: model.decode_step(cache, tok, slot, **flags))
        assert int(cache.errors) == 0
        return trace

    plain, fp8 = step(None), step("fp8")
    assert len(plain) == len(fp8)
    attn = "attn_decode_split" if flags else "attn_decode"
    L = model.num_layers
    assert [e[0] for e in fp8].count("kv_store_fp8") == L and [e[0] for e in fp8].count(attn + "_fp8") == L
    for k, (p, q) in enumerate(zip(plain, fp8)):
        if p[0] in ("kv_store", attn):
            assert q[0] == p[0] + "_fp8", k
            assert q[1][0] == p[1][0] and q[1][-3:] == p[1][-3:]        # the same qkv, the same geometry ...
            assert q[2].keys() == p[2].keys()                           # ... and the same keywords (n_bad; span and workspace)
        else:
            assert q == p, f"call {k} ({p[0]}) differs"


def test_mixed_caches_and_foreign_dtypes_are_refused(tiny32):
    model = tiny32
    with pytest.raises(ValueError):
        model.new_kv_cache(2, 8, "fp16")
    pc, bc = model.new_kv_cache(1, 8, "fp8"), model.new_kv_cache(2, 4)
    tok = torch.zeros(2, dtype=torch.int64, device=DEV)
    z = torch.zeros(2, dtype=torch.int32, device=DEV)
    anc = torch.zeros((2, 4), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="different kinds"):
        model.decode_step_beam(pc, bc, tok, z, z + 1, anc, 0)
