"""Split-KV decode attention on the model: ``decode_step(..., split_kv=True)`` / ``decode_step_beam(..., split_kv=True)`` and the three loops of
``ssi.generate`` with the flag, on the ``MFMA_PARAMS`` model of tests/test_generate_model_gpu.py in bf16 with ``split_span = 64`` and on the fp32
``tiny`` model (head_dim 16) with its form's round of 128 keys.  Every test pins ``split_span`` (and, where it matters, ``split_max_rows``) on the
instance, so nothing here moves when the measured defaults do.  Prompts are 70 to 200 tokens: the steps cross two or three split edges.

* teacher-forced walk (that file's ``teacher_forced_walk``, its ``decode_step`` given the flag): bf16 under that file's criterion — the largest
  distance of the decode logits from the fp32 oracle at most 2.0 x that of the model's own bf16 full forward; fp32 within 1e-4 of the logits' absmax;
* dispatch, from tests/launch_trace.Tracer: with the flag a step calls ``attn_decode_split`` once per layer and ``attn_decode`` never, on the step's
  rows and a workspace ``ws.splitkv.g`` / ``.s``; without the flag, or with ``split_max_rows + 1`` rows, the calls are the plain step's, entry for
  entry; the same for ``decode_step_beam``;
* the loops, by row independence: one prompt alone, among 5 and among ``min(40, split_max_rows)`` gives equal tokens and bit-equal
  ``cumulative_logprob`` under ``generate``, with and without ``small_batch``; ``sample(n=2)`` and ``beam_search(beam_width=4)`` alone against among 3;
* a training step is bit-equal with a split-KV ``generate`` between its forward and its backward.

Measured on the MI355X: bf16 decode 1.214e-1 against the full forward's own 1.136e-1 (1.07 x), padded and small-batch alike; fp32 1.97e-6 against a
tolerance of 2.96e-4."""
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
    assert model._mfma_shapes() and model.head_dim == 64
    model.split_span = 64
    model.eval()
    return model, sd


def tiny_params():
    params, _, _, seed = hx.CASES["tiny"]
    return dict(params, max_seq_len=512), seed


@pytest.fixture(scope="module")
def tiny32(base):
    params, seed = tiny_params()
    sd = hx.seeded_state_dict(params, seed)
    model = base.hip_model(params, sd)
    from ssi import ops
    model.split_span = 128
    assert ops.attn_decode_split_span(model.head_dim, torch.float32) % 128 == 0 and model.head_dim == 16      # 128: the round of fp32 at head_dim 16
    model.eval()
    return model, sd, params


def prompts_of(n, seed=7, lo=70, hi=201):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 500, size=int(rs.randint(lo, hi))).tolist() for _ in range(n)]


def _walk(base, model, rows, lens, **flag):
    assert model.takes_split_kv(len(rows), True)
    plain_step = model.decode_step
    model.decode_step = functools.partial(plain_step, split_kv=True, **flag)
    try:
        return base.teacher_forced_walk(model, rows, lens)
    finally:
        del model.decode_step


@pytest.mark.parametrize("small_batch", (False, True), ids=("padded", "small_batch"))
def test_teacher_forced_logits_bf16(base, mfma, small_batch):
    model, sd = mfma
    params, S = base.MFMA_PARAMS, 220
    rs = np.random.RandomState(23)
    rows = list(torch.from_numpy(rs.randint(0, params["vocab_size"], size=(5, S)).astype(np.int64)))
    ref = hx.oracle_model(params, sd, chunks=0)
    want = [base.oracle_logits(ref, r) for r in rows]
    with torch.no_grad():
        full = model(tokens=torch.stack(rows).to(DEV)).double().cpu()
    full_err = max(float((full[i] - want[i]).abs().max()) for i in range(5))
    got = _walk(base, model, rows, (70, 100, 130, 200, 90), small_batch=small_batch)      # steps at 70 .. 219 keys: the edges 128 and 192
    dec_err = max(float((g.double() - want[i][pos]).abs().max()) for i, pos, g in got)
    print(f"bf16, span 64: split-KV decode {dec_err:.4e}, own full forward {full_err:.4e} from the fp32 oracle (ratio {dec_err / full_err:.2f})")
    assert dec_err <= 2.0 * full_err


def test_teacher_forced_logits_fp32(base, tiny32):
    model, sd, params = tiny32
    S = 300
    rs = np.random.RandomState(24)
    rows = list(torch.from_numpy(rs.randint(0, params["vocab_size"], size=(2, S)).astype(np.int64)))
    ref = hx.oracle_model(params, sd, chunks=0)
    want = [base.oracle_logits(ref, r) for r in rows]
    absmax = max(float(w.abs().max()) for w in want)
    got = _walk(base, model, rows, (70, 200))                                            # steps at 70 .. 299 keys: the edges 128 and 256
    worst = max(float((g.double() - want[i][pos]).abs().max()) for i, pos, g in got)
    print(f"fp32, span 128: split-KV decode logits max-abs error {worst:.3e}, tolerance {1e-4 * absmax:.3e}")
    assert worst <= 1e-4 * absmax


# ---- dispatch ------------------------------------------------------------------------------------------------------------------------
def _trace_step(model, rows, **flag):
    import launch_trace
    tr = launch_trace.Tracer()
    tr.watch(model)
    cache = model.new_kv_cache(rows, 150)
    model.prefill(cache, [[3 + i % 50, 5, 7] * 30 for i in range(rows)], max_new_tokens=4)
    tok = torch.arange(rows, dtype=torch.int64, device=DEV) + 11
    slot = torch.arange(rows, dtype=torch.int32, device=DEV)
    with tr.scenario(caches=[cache]):
        logits = model.decode_step(cache, tok, slot, **flag)
    assert logits.shape == (rows, model.vocab_pad) and int(cache.errors) == 0
    return tr.entries


def _trace_beam_step(model, n_prompts, W, **flag):
    import launch_trace
    tr = launch_trace.Tracer()
    tr.watch(model)
    rows = n_prompts * W
    pcache, bcache = model.new_kv_cache(n_prompts, 100), model.new_kv_cache(rows, 8)
    model.prefill(pcache, [[3 + i, 5, 7] * 30 for i in range(n_prompts)])
    tok = torch.arange(rows, dtype=torch.int64, device=DEV) + 11
    own = torch.arange(rows, dtype=torch.int32, device=DEV)
    plen = torch.full((rows,), 90, dtype=torch.int32, device=DEV)
    anc = own[:, None].expand(rows, 8).contiguous()
    with tr.scenario(caches=[pcache]):
        logits = model.decode_step_beam(pcache, bcache, tok, own // W, plen, anc, 0, **flag)
    assert logits.shape == (rows, model.vocab_pad) and int(bcache.errors) == 0
    return tr.entries


def _where(entry, key):
    a = entry[2][key]
    return a[0] if isinstance(a, list) else a


@pytest.mark.parametrize("which,rows,small", (("mfma", 1, False), ("mfma", 8, False), ("mfma", 8, True), ("tiny32", 3, False)))
def test_a_split_kv_step_calls_the_split_op_once_per_layer(request, which, rows, small):
    model = request.getfixturevalue(which)[0]
    L = model.num_layers
    got = _trace_step(model, rows, split_kv=True, small_batch=small)
    names = [e[0] for e in got]
    assert names.count("attn_decode_split") == L and names.count("attn_decode") == 0 and names.count("kv_store") == L
    R = rows if model.takes_small_batch(rows, small) else model._padded_rows(rows)
    mode = "s" if model.takes_small_batch(rows, small) else "g"
    for e in got:
        if e[0] == "attn_decode_split":
            assert e[1][0][2][0] == R                                        # the step's rows, padded or not
            assert e[2]["span"] == model.split_span and _where(e, "workspace") == "ws.splitkv." + mode
    plain = _trace_step(model, rows, small_batch=small)
    assert [e[0] for e in plain].count("attn_decode") == L and "attn_decode_split" not in [e[0] for e in plain]
    strip = lambda es: [e[0] for e in es if not e[0].startswith("attn_decode")]  # noqa: E731
    assert strip(got) == strip(plain)                                        # nothing else of the step differs


@pytest.mark.parametrize("rows,flag,limit", ((8, {}, None), (8, {"split_kv": False}, None), (9, {"split_kv": True}, 8), (1, {"split_kv": True}, 0)))
def test_without_the_flag_or_beyond_split_max_rows_the_step_is_the_plain_one(mfma, rows, flag, limit):
    model, _ = mfma
    plain = _trace_step(model, rows)
    assert "attn_decode_split" not in {e[0] for e in plain}
    if limit is not None:
        model.split_max_rows = limit
    try:
        assert not model.takes_split_kv(rows, flag.get("split_kv", False))
        got = _trace_step(model, rows, **flag)
    finally:
        if limit is not None:
            del model.split_max_rows
    assert len(got) == len(plain)
    for k, (w, g) in enumerate(zip(plain, got)):
        assert g == w, f"call {k} differs"


def test_the_beam_step_dispatches_alike(mfma):
    model, _ = mfma
    L = model.num_layers
    plain = _trace_beam_step(model, 2, 4)
    got = _trace_beam_step(model, 2, 4, split_kv=True)
    names = [e[0] for e in got]
    assert names.count("attn_decode_beam_split") == L and names.count("attn_decode_beam") == 0
    assert [e[0] for e in plain].count("attn_decode_beam") == L
    for e in got:
        if e[0] == "attn_decode_beam_split":
            assert e[2]["span"] == 64 and _where(e, "workspace") == "ws.splitkv.g" and e[1][0][2][0] == 256
    off = _trace_beam_step(model, 2, 4, split_kv=False)
    assert off == plain
    model.split_max_rows = 7
    try:
        beyond = _trace_beam_step(model, 2, 4, split_kv=True)
    finally:
        del model.split_max_rows
    assert beyond == plain


def test_the_split_workspace_is_a_buffer_of_its_own(mfma, base):
    model = base.hip_model(base.MFMA_PARAMS, mfma[1], torch.bfloat16)
    model.split_span = 64
    model.eval()
    _trace_step(model, 8)
    before = {n: (t.data_ptr(), tuple(t.shape)) for n, t in model._arena.buf.items() if t is not None}
    _trace_step(model, 8, split_kv=True)
    after = {n: (t.data_ptr(), tuple(t.shape)) for n, t in model._arena.buf.items() if t is not None}
    assert all(after[n] == v for n, v in before.items())
    assert set(after) - set(before) == {"ws.splitkv.g"}


# ---- the loops ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small_batch", (False, True), ids=("padded", "small_batch"))
def test_generate_one_prompt_alone_among_5_and_among_40(mfma, small_batch):
    from ssi.generate import generate
    model, _ = mfma
    most = min(40, model.split_max_rows)
    assert most >= 5, "the class default split_max_rows leaves no group to compare (pin it on the instance if the measurement set it to 0)"
    prompts = prompts_of(most)
    kw = dict(max_new_tokens=12, logprobs=True, small_batch=small_batch, split_kv=True, **KW)
    report = {}
    alone = generate(model, prompts[:1], small_batch_report=report, **kw)[0]
    assert len(alone.token_ids) == 12 and report.get("split_kv_groups") == 1
    for n in (5, most):
        among = generate(model, prompts[:n], **kw)[0]
        assert among.token_ids == alone.token_ids, n
        assert among.cumulative_logprob == alone.cumulative_logprob, (n, among.cumulative_logprob, alone.cumulative_logprob)


def test_sample_and_beam_search_one_prompt_alone_and_among_3(mfma):
    from ssi.generate import beam_search, sample
    model, _ = mfma
    prompts = prompts_of(3, seed=9)
    draw = dict(n=2, temperature=0.9, top_k=50, seed=1234, max_new_tokens=12, split_kv=True, **KW)
    alone, among = sample(model, prompts[:1], **draw)[0], sample(model, prompts, **draw)[0]
    for a, b in zip(alone, among):
        assert b.token_ids == a.token_ids and b.cumulative_logprob == a.cumulative_logprob
    kw = dict(beam_width=4, n_best=4, max_new_tokens=10, split_kv=True, **KW)
    alone, among = beam_search(model, prompts[:1], **kw)[0], beam_search(model, prompts, **kw)[0]
    assert [(h.token_ids, h.cumulative_logprob, h.score) for h in among] == [(h.token_ids, h.cumulative_logprob, h.score) for h in alone]


def test_split_kv_moves_the_bits_of_a_long_row_and_not_the_tokens_much(mfma):
    """The flag is not a no-op: past one span the merge order differs from the plain kernel's, so log-probabilities differ in their last bits."""
    from ssi.generate import generate
    model, _ = mfma
    prompts = prompts_of(2, seed=3, lo=190, hi=201)
    a = generate(model, prompts, max_new_tokens=8, logprobs=True, **KW)
    b = generate(model, prompts, max_new_tokens=8, logprobs=True, split_kv=True, **KW)
    for x, y in zip(a, b):
        assert abs(x.cumulative_logprob - y.cumulative_logprob) <= 0.25


def test_a_training_step_is_bit_equal_with_a_split_kv_generate_inside_it(base):
    from ssi.generate import generate
    params, b, s, seed, dtype = base.MFMA_PARAMS, 2, 128, 21, torch.bfloat16
    sd = hx.seeded_state_dict(params, seed)
    dbatch = {k: v.to(DEV) for k, v in hx.seeded_batch(params["vocab_size"], b, s, seed).items()}
    prompts = prompts_of(3, seed=11)

    def gen(model):
        model.split_span = 64
        out = generate(model, prompts, max_new_tokens=10, logprobs=True, split_kv=True, **KW)
        assert all(len(g.token_ids) == 10 for g in out) and "ws.splitkv.g" in model._arena.buf

    loss0, grad0 = base._step(base.hip_model(params, sd, dtype), dbatch)
    mid = base.hip_model(params, sd, dtype)
    loss1, grad1 = base._step(mid, dbatch, between=lambda: gen(mid))
    assert torch.equal(loss1, loss0) and torch.equal(grad1, grad0)
    assert bool(torch.isfinite(grad0.float()).all()) and float(grad0.float().abs().max()) > 0
