"""FP8 weights on the model: ``HipLlamaDecoder.quantize_weights`` and ``decode_step`` / ``decode_step_beam`` / the loops of ``ssi.generate`` with
them, on the ``MFMA_PARAMS`` model of tests/test_generate_model_gpu.py (vocab 700, 2 layers, D = 512) in bf16: the smallest geometry that takes the
small-batch path, as tests/test_small_batch_model_gpu.py builds it.

The property: model A with ``weight_quant=qw`` computes, bit for bit, what a model B computes whose matrices hold the DEQUANTISED values.  B is a
copy of A whose ``wqkv``, ``wo``, ``w13`` (gate and up) and ``w2`` of every layer are overwritten with the values of qw's codes (made on the CPU by
tests/weight_fp8_ref.py, which asserts they are exact in bf16).  The tied embedding has two readers, and FP8 weights change one of them: the
embedding GATHER keeps reading the bf16 table (in A and therefore in B), the HEAD reads the codes.  So B's table stays as it is and B's head (its
``_head_logits``) multiplies by a dequantised copy of the table held beside it — with ``head=False`` B's head is simply its own.  Both caches are
prefilled by A, on the unquantised weights, as ``prefill`` always runs.

* ``decode_step`` at 1, 5 and 40 rows over 4 consecutive steps, and ``decode_step_beam`` over 4 steps: bit-equal logits and bit-equal caches;
* ``head=False``: bit-equal to B with its own head, and different from the full object's logits;
* ``generate(..., small_batch=True, weight_dtype="fp8")``: tokens and ``cumulative_logprob`` of the same loop driven through B's steps; a prebuilt
  object gives the same; the group is counted; ``sample`` and ``beam_search`` run on the same steps;
* ``weight_dtype=None`` / "auto": tokens and bits of the call without the argument;
* a training step's loss and gradients are bit-equal with such a ``generate`` between its forward and its backward;
* an object of another model is refused."""
import numpy as np
import pytest
import torch

import weight_fp8_ref as wq
from oracle import hf_crosscheck as hx

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KW = dict(stop_token_ids=[], pad_id=0)
BF = torch.bfloat16


@pytest.fixture(scope="module")
def base():
    import test_generate_model_gpu as g
    return g


@pytest.fixture(scope="module")
def models(base):
    """(A, qw, B with the dequantised head, B with its own head), built once and never modified."""
    from ssi import ops
    sd = hx.seeded_state_dict(base.MFMA_PARAMS, 21)
    A = base.hip_model(base.MFMA_PARAMS, sd, BF)
    A.eval()
    assert A.takes_small_batch(1, True)
    qw = A.quantize_weights()
    assert qw.head and set(qw.mats) == {f"L{l}.{m}" for l in range(A.num_layers) for m in ("wqkv", "wo", "w13", "w2")} | {"emb"}
    assert qw.nbytes() == sum(A._view(n).numel() + A._view(n).shape[0] for n in qw.mats)

    def dequantised(name):
        codes, exps = qw.mats[name]
        ref_c, ref_b = wq.quantise(A._view(name).cpu())                 # the quantiser on the model's own matrices, against the CPU rule
        assert torch.equal(codes.cpu(), ref_c) and torch.equal(exps.cpu(), ref_b), name
        return wq.dequantise_bf16(ref_c, ref_b).to(DEV)

    def model_b(head):
        B = base.hip_model(base.MFMA_PARAMS, sd, BF)
        B.eval()
        for name in qw.mats:
            if name != "emb":
                B._view(name).copy_(dequantised(name))
        B.prefill = A.prefill                                           # prompts always run on the unquantised weights
        if head:
            table = dequantised("emb")

            def head_logits(hn, arena_name=None, skinny=False, weight_quant=None):
                assert skinny and arena_name is None and weight_quant is None
                logits = torch.empty((hn.shape[0], B.vocab_pad), dtype=BF, device=DEV)
                ops.gemm_skinny(hn, table, logits)
                return logits
            B._head_logits = head_logits
        return B

    return A, qw, model_b(True), model_b(False)


def prompts_of(n, seed=7, lo=2, hi=30):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 700, size=int(rs.randint(lo, hi))).tolist() for _ in range(n)]


def same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(a.view(torch.int16) if a.dtype == BF else a, b.view(torch.int16) if b.dtype == BF else b), what


@pytest.mark.parametrize("rows", (1, 5, 40))
def test_decode_step_is_bit_equal_to_the_model_of_dequantised_weights(models, rows):
    A, qw, B, _ = models
    prompts = prompts_of(rows)
    ca, cb = A.new_kv_cache(rows, 40), A.new_kv_cache(rows, 40)
    first = A.prefill(ca, prompts, max_new_tokens=4)
    A.prefill(cb, prompts, max_new_tokens=4)
    tok = first[:, :A.vocab_size].float().argmax(dim=-1)
    slot = torch.arange(rows, dtype=torch.int32, device=DEV)
    for step in range(4):
        la = A.decode_step(ca, tok, slot, small_batch=True, weight_quant=qw)
        lb = B.decode_step(cb, tok, slot, small_batch=True)
        same(la, lb, f"logits of step {step} at {rows} rows")
        assert bool(torch.isfinite(la.float()).all())
        tok = la[:, :A.vocab_size].float().argmax(dim=-1)
    same(ca.k, cb.k, "K cache")
    same(ca.v, cb.v, "V cache")
    assert torch.equal(ca.lengths, cb.lengths) and int(ca.errors) == 0 and int(cb.errors) == 0


def prefilled(A, prompts, rows):
    c = A.new_kv_cache(rows, 40)
    A.prefill(c, prompts, max_new_tokens=4)
    return c


def test_decode_step_beam_is_bit_equal(models):
    A, qw, B, _ = models
    n, W, steps = 3, 2, 4
    rows = n * W
    prompts = prompts_of(n, seed=3)
    pc = A.new_kv_cache(n, 32)
    first = A.prefill(pc, prompts)
    ba, bb = A.new_kv_cache(rows, steps), A.new_kv_cache(rows, steps)
    own = torch.arange(rows, dtype=torch.int32, device=DEV)
    seq_of = own // W
    plen = torch.tensor([len(p) for p in prompts], dtype=torch.int32, device=DEV).repeat_interleave(W)
    anc = own[:, None].expand(rows, steps).contiguous()
    top = first[:n, :A.vocab_size].float().topk(W, dim=-1).indices.reshape(-1)         # beam b of a prompt starts with its b-th best token
    tok = top
    for t in range(steps):
        la = A.decode_step_beam(pc, ba, tok, seq_of, plen, anc, t, small_batch=True, weight_quant=qw)
        lb = B.decode_step_beam(pc, bb, tok, seq_of, plen, anc, t, small_batch=True)
        same(la, lb, f"beam logits of step {t}")
        tok = la[:, :A.vocab_size].float().argmax(dim=-1)
    same(ba.k, bb.k, "beam K cache")
    assert int(ba.errors) == 0 and int(bb.errors) == 0


def test_without_the_head_the_head_runs_on_the_bf16_table(models):
    A, qw, B, B_own_head = models
    qn = A.quantize_weights(head=False)
    assert not qn.head and "emb" not in qn.mats and qn.nbytes() < qw.nbytes()
    rows = 5
    prompts = prompts_of(rows, seed=11)
    slot = torch.arange(rows, dtype=torch.int32, device=DEV)
    ca, cb, cf = (prefilled(A, prompts, rows) for _ in range(3))
    tok = torch.arange(rows, dtype=torch.int64, device=DEV) * 13 + 5
    la = A.decode_step(ca, tok, slot, small_batch=True, weight_quant=qn)
    same(la, B_own_head.decode_step(cb, tok, slot, small_batch=True), "head=False")
    assert not torch.equal(la, A.decode_step(cf, tok, slot, small_batch=True, weight_quant=qw))


def test_generate_with_fp8_weights_is_the_loop_through_the_dequantised_model(models):
    from ssi.generate import beam_search, generate, sample
    A, qw, B, _ = models
    prompts = prompts_of(5)
    kw = dict(max_new_tokens=12, logprobs=True, small_batch=True, **KW)
    want = generate(B, prompts, **kw)
    report = {}
    got = generate(A, prompts, weight_dtype="fp8", small_batch_report=report, **kw)
    assert [(g.token_ids, g.cumulative_logprob) for g in got] == [(g.token_ids, g.cumulative_logprob) for g in want]
    assert all(len(g.token_ids) == 12 for g in got) and report == {"small_batch_groups": 1, "fp8_weight_groups": 1}
    again = generate(A, prompts, weight_dtype="fp8", weight_quant=qw, **kw)
    assert [(g.token_ids, g.cumulative_logprob) for g in again] == [(g.token_ids, g.cumulative_logprob) for g in want]
    plain = generate(A, prompts, **kw)
    assert [g.cumulative_logprob for g in plain] != [g.cumulative_logprob for g in want]           # the quantisation is not a no-op on this model
    draw = dict(n=2, temperature=0.9, top_k=50, seed=12, max_new_tokens=8, small_batch=True, **KW)
    a, b = sample(A, prompts[:3], weight_dtype="fp8", weight_quant=qw, **draw), sample(B, prompts[:3], **draw)
    assert [[(g.token_ids, g.cumulative_logprob) for g in gs] for gs in a] == [[(g.token_ids, g.cumulative_logprob) for g in gs] for gs in b]
    beam = dict(beam_width=3, n_best=3, max_new_tokens=6, small_batch=True, **KW)
    a, b = beam_search(A, prompts[:2], weight_dtype="fp8", weight_quant=qw, **beam), beam_search(B, prompts[:2], **beam)
    assert [[(h.token_ids, h.cumulative_logprob, h.score) for h in hs] for hs in a] == [[(h.token_ids, h.cumulative_logprob, h.score) for h in hs] for hs in b]


def test_a_group_off_the_small_batch_path_is_untouched(models):
    from ssi.generate import generate
    A, qw, _, _ = models
    prompts = prompts_of(66, seed=5, hi=8)                                 # one group of 66 rows: the tile path
    kw = dict(max_new_tokens=3, logprobs=True, small_batch=True, **KW)
    report = {}
    got = generate(A, prompts, weight_dtype="fp8", weight_quant=qw, small_batch_report=report, **kw)
    want = generate(A, prompts, **kw)
    assert [(g.token_ids, g.cumulative_logprob) for g in got] == [(g.token_ids, g.cumulative_logprob) for g in want] and not report


def test_auto_and_none_are_the_call_without_the_argument(models):
    from ssi.generate import generate
    A, _, _, _ = models
    prompts = prompts_of(5, seed=2)
    kw = dict(max_new_tokens=10, logprobs=True, small_batch=True, **KW)
    want = generate(A, prompts, **kw)
    for value in (None, "auto"):
        report = {}
        got = generate(A, prompts, weight_dtype=value, small_batch_report=report, **kw)
        assert [(g.token_ids, g.cumulative_logprob) for g in got] == [(g.token_ids, g.cumulative_logprob) for g in want]
        assert report == {"small_batch_groups": 1}


def test_an_object_of_another_model_and_an_fp32_model_are_refused(models, base):
    A, qw, _, _ = models
    other = dict(base.MFMA_PARAMS, num_layers=1)
    small = base.hip_model(other, hx.seeded_state_dict(other, 3), BF)
    cache = small.new_kv_cache(1, 8)
    small.prefill(cache, [[1, 2, 3]], max_new_tokens=2)
    tok, slot = torch.tensor([5], device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="weight_quant"):
        small.decode_step(cache, tok, slot, small_batch=True, weight_quant=qw)
    assert int(cache.lengths[0]) == 3                                      # refused before anything ran
    params, _, _, seed = hx.CASES["tiny"]
    f32 = base.hip_model(params, hx.seeded_state_dict(params, seed))
    with pytest.raises(ValueError, match="quantize_weights"):
        f32.quantize_weights()


def test_a_training_step_is_bit_equal_with_an_fp8_weight_generate_inside_it(base):
    from ssi.generate import generate
    params, b, s, seed, dtype = base.MFMA_PARAMS, 2, 128, 21, BF
    sd = hx.seeded_state_dict(params, seed)
    dbatch = {k: v.to(DEV) for k, v in hx.seeded_batch(params["vocab_size"], b, s, seed).items()}
    prompts = base.greedy_prompts(params["vocab_size"])

    def gen(model):
        report = {}
        out = generate(model, prompts, max_new_tokens=10, logprobs=True, small_batch=True, weight_dtype="fp8", small_batch_report=report, **KW)
        assert all(len(g.token_ids) == 10 for g in out) and report.get("fp8_weight_groups") == 1

    loss0, grad0 = base._step(base.hip_model(params, sd, dtype), dbatch)
    mid = base.hip_model(params, sd, dtype)
    loss1, grad1 = base._step(mid, dbatch, between=lambda: gen(mid))
    assert torch.equal(loss1, loss0) and torch.equal(grad1, grad0)
    assert bool(torch.isfinite(grad0.float()).all()) and float(grad0.float().abs().max()) > 0
