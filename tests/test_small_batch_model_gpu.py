"""Small-batch decoding on the model: ``decode_step(..., small_batch=True)`` / ``decode_step_beam(..., small_batch=True)`` and the three loops of
``ssi.generate`` with the flag, on the ``MFMA_PARAMS`` model of tests/test_generate_model_gpu.py (vocab 700, 2 layers, D = 512) in bf16.

* teacher-forced walk (that file's ``teacher_forced_walk``, its ``decode_step`` given the flag) with 5 sequences (one m-tile) and with 20 (two):
  the largest distance of the decode logits from the fp32 oracle at most 2.0 x that of the model's own bf16 full forward, measured in the same
  test — the criterion and the factor of ``test_teacher_forced_logits_bf16_on_the_mfma_path``;
* dispatch, from tests/launch_trace.Tracer: a small-batch step calls the three skinny ops on tensors of exactly ``rows`` rows and none of
  ``gemm``, ``gemm_rope``, ``gemm_swiglu_fwd``; without the flag, or with 65 rows, the calls are those of the plain step, entry for entry;
* the loops, by row independence: one prompt alone, among 5 and among 40 gives the same tokens and bit-equal ``cumulative_logprob`` under
  ``generate`` and ``sample(n=2)``; ``beam_search(beam_width=4)`` on one prompt equals the same prompt among 3;
* the fp32 ``tiny`` model takes no skinny path: the flag changes nothing;
* a training step is bit-equal with a small-batch ``generate`` between its forward and its backward.

A group that decodes on the skinny path also prefills prompt by prompt (``prefill(..., separate=True)``): packed with others, where a prompt lies in
its row and how many rows the forward has (the K split of its GEMMs) enter the bits of its K / V — the first version of the loop tests met exactly
that: equal tokens, ``cumulative_logprob`` -44.6330 among 5 against -44.6479 alone.

Measured on the MI355X: 5 sequences: decode 8.51e-2 against the full forward's own 8.81e-2 (0.97 x); 20 sequences: 1.093e-1 against 1.093e-1 (1.00 x)."""
import functools

import numpy as np
import pytest
import torch

from oracle import hf_crosscheck as hx

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KW = dict(stop_token_ids=[], pad_id=0)


@pytest.fixture(scope="module")
def base():
    import test_generate_model_gpu as g
    return g


@pytest.fixture(scope="module")
def mfma(base):
    sd = hx.seeded_state_dict(base.MFMA_PARAMS, 21)
    model = base.hip_model(base.MFMA_PARAMS, sd, torch.bfloat16)
    assert model._mfma_shapes() and model.skinny_max_rows <= 64
    model.eval()
    return model, sd


def prompts_of(n, seed=7, lo=2, hi=30):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 700, size=int(rs.randint(lo, hi))).tolist() for _ in range(n)]


@pytest.mark.parametrize("n_seq", (5, 20))
def test_teacher_forced_logits_of_the_small_batch_step(base, mfma, n_seq):
    model, sd = mfma
    params, S = base.MFMA_PARAMS, 40
    rs = np.random.RandomState(22)
    rows = list(torch.from_numpy(rs.randint(0, params["vocab_size"], size=(n_seq, S)).astype(np.int64)))
    ref = hx.oracle_model(params, sd, chunks=0)
    want = [base.oracle_logits(ref, r) for r in rows]
    with torch.no_grad():
        full = model(tokens=torch.stack(rows).to(DEV)).double().cpu()
    full_err = max(float((full[i] - want[i]).abs().max()) for i in range(n_seq))
    lens = tuple((1, 17, 5, 9, 30)[i % 5] + i // 5 for i in range(n_seq))
    assert model.takes_small_batch(n_seq, True)
    plain_step = model.decode_step
    model.decode_step = functools.partial(plain_step, small_batch=True)
    try:
        got = base.teacher_forced_walk(model, rows, lens)
    finally:
        del model.decode_step
    dec_err = max(float((g.double() - want[i][pos]).abs().max()) for i, pos, g in got)
    print(f"bf16, {n_seq} sequences: small-batch decode {dec_err:.4e}, own full forward {full_err:.4e} from the fp32 oracle (ratio {dec_err / full_err:.2f})")
    assert dec_err <= 2.0 * full_err


# ---- dispatch ------------------------------------------------------------------------------------------------------------------------
SKINNY = {"gemm_skinny", "gemm_skinny_rope", "gemm_skinny_swiglu"}
TILED = {"gemm", "gemm_rope", "gemm_swiglu_fwd", "gemm_splitk"}


def _trace_step(model, rows, **flag):
    import launch_trace
    tr = launch_trace.Tracer()
    tr.watch(model)
    cache = model.new_kv_cache(rows, 16)
    model.prefill(cache, [[3 + i, 5, 7] for i in range(rows)], max_new_tokens=4)
    tok = torch.arange(rows, dtype=torch.int64, device=DEV) + 11
    slot = torch.arange(rows, dtype=torch.int32, device=DEV)
    with tr.scenario(caches=[cache]):
        logits = model.decode_step(cache, tok, slot, **flag)
    assert logits.shape == (rows, model.vocab_pad)
    return tr.entries


def _rows_of(entry):
    return {a[2][0] for a in entry[1] + list(entry[2].values()) if isinstance(a, list) and len(a) == 5 and a[0] not in ("param", "rope")
            and not str(a[0]).startswith("cache.") and len(a[2]) == 2}


@pytest.mark.parametrize("rows", (1, 8, 33, 64))
def test_a_small_batch_step_runs_the_skinny_ops_on_unpadded_rows(mfma, rows):
    model, _ = mfma
    L = model.num_layers
    got = _trace_step(model, rows, small_batch=True)
    names = [e[0] for e in got]
    assert not TILED & set(names), names
    assert names.count("gemm_skinny_rope") == L and names.count("gemm_skinny_swiglu") == L and names.count("gemm_skinny") == 2 * L + 1
    assert names.count("kv_store") == L and names.count("attn_decode") == L and names.count("rmsnorm_fwd") == 2 * L + 1 and names.count("embed_fwd") == 1
    for e in got:
        if e[0] in SKINNY | {"rmsnorm_fwd", "embed_fwd", "kv_store", "attn_decode"}:
            assert _rows_of(e) == {rows}, e
        for a in e[1]:
            if isinstance(a, list) and len(a) == 5 and isinstance(a[0], str) and "." in a[0] and not a[0].startswith("cache."):
                assert a[0].endswith(".s"), f"a small-batch step touched the buffer {a[0]}"
    sw = next(e for e in got if e[0] == "gemm_skinny_swiglu")
    assert sw[1][2] is None                                             # no [gate | up] is written in a decode step


@pytest.mark.parametrize("rows,flag", ((8, {}), (8, {"small_batch": False}), (65, {"small_batch": True})))
def test_without_the_flag_or_with_65_rows_the_step_is_the_plain_one(mfma, rows, flag):
    model, _ = mfma
    plain = _trace_step(model, rows)
    assert not SKINNY & {e[0] for e in plain} and {e[0] for e in plain} >= {"gemm", "gemm_rope", "gemm_swiglu_fwd"}
    got = _trace_step(model, rows, **flag)
    assert len(got) == len(plain)
    for k, (w, g) in enumerate(zip(plain, got)):
        assert g == w, f"call {k} differs"


def test_the_modes_share_no_buffer(mfma, base):
    model = base.hip_model(base.MFMA_PARAMS, mfma[1], torch.bfloat16)
    model.eval()
    _trace_step(model, 8)
    before = {n: (t.data_ptr(), tuple(t.shape)) for n, t in model._arena.buf.items() if t is not None}
    _trace_step(model, 8, small_batch=True)
    after = {n: (t.data_ptr(), tuple(t.shape)) for n, t in model._arena.buf.items() if t is not None}
    assert all(after[n] == v for n, v in before.items())                # no *.g (or *.x) buffer was reshaped or moved
    new = set(after) - set(before)
    assert new and all(n.endswith(".s") for n in new), new


# ---- the loops ---------------------------------------------------------------------------------------------------------------------------
def test_generate_one_prompt_alone_among_5_and_among_40(mfma):
    from ssi.generate import generate
    model, _ = mfma
    prompts = prompts_of(40)
    alone = generate(model, prompts[:1], max_new_tokens=12, logprobs=True, small_batch=True, **KW)[0]
    assert len(alone.token_ids) == 12
    for n in (5, 40):
        among = generate(model, prompts[:n], max_new_tokens=12, logprobs=True, small_batch=True, **KW)[0]
        assert among.token_ids == alone.token_ids, n
        assert among.cumulative_logprob == alone.cumulative_logprob, (n, among.cumulative_logprob, alone.cumulative_logprob)


def test_sample_one_prompt_alone_among_5_and_among_40(mfma):
    from ssi.generate import sample
    model, _ = mfma
    prompts = prompts_of(40)
    draw = dict(n=2, temperature=0.9, top_k=50, seed=1234, max_new_tokens=12, small_batch=True, **KW)
    alone = sample(model, prompts[:1], **draw)[0]
    for n in (5, 40):                                                   # batch_size 64: groups of 32 prompts = 64 rows, the most the skinny path takes
        among = sample(model, prompts[:n], batch_size=64, **draw)[0]
        for a, b in zip(alone, among):
            assert b.token_ids == a.token_ids and b.cumulative_logprob == a.cumulative_logprob, n


def test_beam_search_one_prompt_alone_and_among_3(mfma):
    from ssi.generate import beam_search
    model, _ = mfma
    prompts = prompts_of(3, seed=9)
    kw = dict(beam_width=4, n_best=4, max_new_tokens=10, small_batch=True, **KW)
    alone = beam_search(model, prompts[:1], **kw)[0]
    among = beam_search(model, prompts, **kw)[0]
    assert [(h.token_ids, h.cumulative_logprob, h.score) for h in among] == [(h.token_ids, h.cumulative_logprob, h.score) for h in alone]


def test_on_the_fp32_model_the_flag_changes_nothing(base):
    from ssi.generate import generate, sample
    params, _, _, seed = hx.CASES["tiny"]
    model = base.hip_model(params, hx.seeded_state_dict(params, seed))
    assert not model.takes_small_batch(1, True)
    prompts = base.greedy_prompts(params["vocab_size"])
    a = generate(model, prompts, max_new_tokens=8, logprobs=True, **KW)
    b = generate(model, prompts, max_new_tokens=8, logprobs=True, small_batch=True, **KW)
    assert [(g.token_ids, g.cumulative_logprob) for g in a] == [(g.token_ids, g.cumulative_logprob) for g in b]
    draw = dict(n=2, temperature=0.8, seed=3, max_new_tokens=8, **KW)
    a, b = sample(model, prompts, **draw), sample(model, prompts, small_batch=True, **draw)
    assert [[(g.token_ids, g.cumulative_logprob) for g in gs] for gs in a] == [[(g.token_ids, g.cumulative_logprob) for g in gs] for gs in b]
    assert not [n for n in model._arena.buf if n.endswith(".s")]


def test_a_training_step_is_bit_equal_with_a_small_batch_generate_inside_it(base):
    from ssi.generate import generate
    params, b, s, seed, dtype = base.MFMA_PARAMS, 2, 128, 21, torch.bfloat16
    sd = hx.seeded_state_dict(params, seed)
    dbatch = {k: v.to(DEV) for k, v in hx.seeded_batch(params["vocab_size"], b, s, seed).items()}
    prompts = base.greedy_prompts(params["vocab_size"])

    def gen(model):
        out = generate(model, prompts, max_new_tokens=10, logprobs=True, small_batch=True, **KW)
        assert all(len(g.token_ids) == 10 for g in out) and any(n.endswith(".s") for n in model._arena.buf)

    loss0, grad0 = base._step(base.hip_model(params, sd, dtype), dbatch)
    mid = base.hip_model(params, sd, dtype)
    loss1, grad1 = base._step(mid, dbatch, between=lambda: gen(mid))
    assert torch.equal(loss1, loss0) and torch.equal(grad1, grad0)
    assert bool(torch.isfinite(grad0.float()).all()) and float(grad0.float().abs().max()) > 0
