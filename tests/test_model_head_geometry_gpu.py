"""The whole model at Llama-3.2-3B's head geometry — head_dim 128, three query heads per kv head (``ssi/llama_configs.py``:
``configllama3_2_3b``) — against the live ``OracleLlama`` on the CPU, weights from ``oracle.hf_crosscheck.seeded_state_dict``.  Every other model
of the suite has head_dim 8 to 64 and 2 or 4 query heads per kv head.

``GEOMETRY_3B`` keeps the head geometry and shrinks the rest: qkv_dim 1280, and in bf16 ``_mfma_shapes()`` holds, so the projections, the MLP
and the head run on the MFMA GEMMs while attention — ``ssi_attn_mfma_supported`` takes head_dim 64 and 1, 2 or 4 heads per kv head — runs on
csrc/attention_generic.hip in the forward and the backward, and RoPE is a launch of its own behind the QKV GEMM.  That mixed path is what a
bf16 3B run is.  Criteria: those of the tests named in each docstring, unchanged.

``small_batch=True``: ``ssi_gemm_skinny_rope`` rotates head_dim 64 only, so this model keeps the tile path with the flag
(``HipLlamaDecoder.takes_small_batch``), bit for bit.  Before that guard ``decode_step(..., small_batch=True)``, ``generate(...,
small_batch=True)`` and ``ssi.prompting.probe`` raised here: "ssi_gemm_skinny_rope failed with code 2: ssi_gemm_skinny_rope: head_dim 64 and
rotated columns within N only (head_dim=128 n_heads_rot=8 N=1280)".

Measured on the MI355X: fp32 loss equal to the oracle's to the last printed digit (7.9116821; packed 7.3404374); bf16 loss 7.538407 against
7.540642 (3.0e-4 relative), largest relative gradient error 4.4e-2 (limit 6e-2); fp32 decode logits 2.2e-5 from the oracle against a tolerance
of 5.9e-4; bf16 decode 1.767e-1 against the full forward's own 1.810e-1 (0.98 x)."""
import numpy as np
import pytest
import torch

from oracle import hf_crosscheck as hx

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEOMETRY_3B = dict(vocab_size=700, num_layers=2, num_heads=6, num_kv_heads=2, embed_dim=768,
                   max_seq_len=256, intermediate_dim=1024)
SEED = 31
GEMMS = {"gemm", "gemm_splitk", "gemm_batched", "gemm_rope", "gemm_swiglu_fwd", "gemm_swiglu_bwd"}
ATTENTION = {"attn_fwd", "attn_bwd"}


@pytest.fixture(scope="module")
def base():
    import test_generate_model_gpu as g
    return g


@pytest.fixture(scope="module")
def weights():
    return hx.seeded_state_dict(GEOMETRY_3B, SEED)


@pytest.fixture(scope="module")
def oracle(weights):
    return hx.oracle_model(GEOMETRY_3B, weights, chunks=0)


def _model(weights, dtype):
    from ssi.model import HipLlamaDecoder
    m = HipLlamaDecoder(**GEOMETRY_3B, dtype=dtype, device=DEV)
    m.load_state_dict(weights)
    assert m.head_dim == 128 and m.num_heads // m.num_kv_heads == 3 and m.qkv_dim == 1280
    assert m._mfma_shapes() == (dtype == torch.bfloat16)
    return m


def _oracle_step(weights, batch):
    from oracle.llama_oracle import OracleCEWithChunkedOutputLoss
    from oracle.llama_oracle import compute_loss as oracle_loss
    ref_model = hx.oracle_model(GEOMETRY_3B, weights)
    ref = oracle_loss(batch, ref_model, OracleCEWithChunkedOutputLoss())
    ref.backward()
    return ref, ref_model


def _to_dev(batch):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


# ---- training ---------------------------------------------------------------------------------------------------------------------------
def test_fp32_training_step_on_a_ragged_batch_with_an_ignored_row(weights):
    """Loss and every gradient, the batch and the criterion of ``test_fp32_model_matches_live_oracle_on_ragged_batch_with_ignored_row``: 3 x 29
    tokens, an all-ignored row, ignore spans at both ends; loss 1e-5 relative, gradients rtol 5e-3 / atol 1e-6."""
    from ssi.loss import CEWithChunkedOutputLoss, compute_loss
    g = torch.Generator().manual_seed(5)
    tok = torch.randint(0, GEOMETRY_3B["vocab_size"], (3, 29), generator=g)
    lab = tok.clone()
    lab[0] = -100
    lab[1, :7] = -100
    lab[2, -9:] = -100
    batch = {"tokens": tok, "labels": lab}
    ref, ref_model = _oracle_step(weights, batch)
    model = _model(weights, torch.float32)
    loss = compute_loss(_to_dev(batch), model, CEWithChunkedOutputLoss())
    loss.backward()
    print(f"fp32: loss {loss.item():.7f} against the oracle's {ref.item():.7f}")
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    for (k, p), (k2, p2) in zip(model.named_parameters(), ref_model.named_parameters()):
        assert k == k2
        torch.testing.assert_close(p.grad.cpu(), p2.grad, rtol=5e-3, atol=1e-6, msg=lambda m: f"{k}: {m}")


def _step_bits(model, dbatch, tracer=None):
    import contextlib
    from ssi.loss import CEWithChunkedOutputLoss, compute_loss
    with (tracer.scenario() if tracer is not None else contextlib.nullcontext()):
        loss = compute_loss(dbatch, model, CEWithChunkedOutputLoss())
        loss.backward()
        torch.cuda.synchronize()
    return loss


def test_bf16_training_step_on_the_mixed_path(weights):
    """The criteria of ``test_bf16_mfma_shaped_model_matches_oracle`` (loss 1e-2, every gradient 6e-2 in relative L2) on 2 x 128 tokens, and
    the path: no attention plan at this geometry; the attention backward on the generic kernels (``attn_last_dispatch()``); and a second
    step, on a fresh model, with every GEMM call forced onto the MFMA kernels and every attention call onto the generic ones — a forced call
    raises where its kernel does not take the shape — gives the same loss and gradients bit for bit: it is what ran unforced."""
    import launch_trace
    from ssi import _lib, ops
    batch = hx.seeded_batch(GEOMETRY_3B["vocab_size"], 2, 128, SEED)
    ref, ref_model = _oracle_step(weights, batch)
    model = _model(weights, torch.bfloat16)
    assert model.build_attn_plan(torch.arange(128).repeat(2, 1)) is None
    assert model.padded_seq_len(2, 128) == 128
    dbatch = _to_dev(batch)
    loss = _step_bits(model, dbatch)
    used = ops.attn_last_dispatch()
    assert (used & (0x10000 | _lib.ATTN_USED_DQ2 | _lib.ATTN_USED_DKV2 | _lib.ATTN_USED_HEAD_SPLIT | _lib.ATTN_USED_PLAN)) == 0, hex(used)
    print(f"bf16: loss {loss.item():.6f} against the oracle's {ref.item():.6f}")
    assert abs(loss.item() - ref.item()) <= 1e-2 * abs(ref.item())
    worst = 0.0
    for (k, p), (_, p2) in zip(model.named_parameters(), ref_model.named_parameters()):
        rel = float((p.grad.float().cpu() - p2.grad).norm() / p2.grad.norm())
        worst = max(worst, rel)
        assert rel <= 6e-2, f"{k}: relative gradient error {rel}"
    print(f"bf16: largest relative gradient error {worst:.3e}")

    class Forced(launch_trace.Tracer):
        def call(self, name, fn, args, kw):
            impl = _lib.IMPL_MFMA if name in GEMMS else _lib.IMPL_GENERIC if name in ATTENTION else None
            if impl is None:
                return fn(*args, **kw)
            prev = ops.set_impl(impl)
            try:
                return fn(*args, **kw)
            finally:
                ops.set_impl(prev)

    forced = _model(weights, torch.bfloat16)
    tr = Forced()
    tr.watch(forced)
    loss2 = _step_bits(forced, dbatch, tr)
    names = [e[0] for e in tr.entries]
    L = GEOMETRY_3B["num_layers"]
    assert names.count("attn_fwd") == L and names.count("attn_bwd") == L and names.count("gemm_rope") == L and names.count("gemm_swiglu_fwd") == L
    for e in tr.entries:
        if e[0] in ATTENTION:                                               # (B, S, H, KV, head_dim) on the model's bf16 qkv
            at = 3 if e[0] == "attn_fwd" else 6
            assert e[1][at:at + 5] == [2, 128, 6, 2, 128] and e[1][0][-1] == str(torch.bfloat16), e
    assert torch.equal(loss2.detach(), loss.detach()) and torch.equal(forced._flat_grad, model._flat_grad)


@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
def test_packed_rows_against_the_block_causal_oracle(weights, dtype_name):
    """The construction and the criteria of ``test_packed_batch_matches_oracle_with_block_causal_mask``: packs of short documents with a masked
    prompt span each, ``input_pos`` restarting per document, against the oracle fed torchtune's dense block-causal mask — loss and every
    gradient (fp32 1e-5 / 5e-3, bf16 1e-2 / 6e-2 in relative L2).  In bf16 the 200 positions are padded to 256 inside the fused loss."""
    from oracle.llama_oracle import OracleCEWithChunkedOutputLoss
    from oracle.llama_oracle import compute_loss as oracle_loss
    from ssi.data import PackedDataset, packed_block_causal_mask, padded_collate_packed
    from ssi.loss import CEWithChunkedOutputLoss, compute_loss
    bf16 = dtype_name == "bf16"
    S = 200 if bf16 else 100
    g = torch.Generator().manual_seed(51)
    lengths = [57, 130, 9, 77, 64, 33, 12] if bf16 else [31, 7, 44, 13, 50, 26]
    samples = []
    for n in lengths:
        toks = torch.randint(0, GEOMETRY_3B["vocab_size"], (n,), generator=g).tolist()
        samples.append({"tokens": toks, "labels": [(-100 if i < 3 else t) for i, t in enumerate(toks)]})
    packs = PackedDataset(samples, max_seq_len=S, padding_idx=0)
    batch = padded_collate_packed([packs[0], packs[1]])
    assert all(len(s) >= 3 for s in batch["seq_lens"])                      # several documents in either row
    ref_model = hx.oracle_model(GEOMETRY_3B, weights)
    ref_batch = {"tokens": batch["tokens"], "labels": batch["labels"], "input_pos": batch["input_pos"],
                 "mask": packed_block_causal_mask(batch["seq_lens"])}
    ref = oracle_loss(ref_batch, ref_model, OracleCEWithChunkedOutputLoss())
    ref.backward()
    model = _model(weights, torch.bfloat16 if bf16 else torch.float32)
    dbatch = _to_dev(batch)
    loss = compute_loss(dbatch, model, CEWithChunkedOutputLoss())
    loss.backward()
    tol_l, tol_g = (1e-2, 6e-2) if bf16 else (1e-5, 5e-3)
    print(f"packed {dtype_name}: loss {loss.item():.7f} against the oracle's {ref.item():.7f}")
    assert abs(loss.item() - ref.item()) <= tol_l * abs(ref.item())
    for (k, p), (_, p2) in zip(model.named_parameters(), ref_model.named_parameters()):
        rel = float((p.grad.float().cpu() - p2.grad).norm() / p2.grad.norm())
        assert rel <= tol_g, f"{k}: relative gradient error {rel}"
    plain = compute_loss({"tokens": dbatch["tokens"], "labels": dbatch["labels"]}, model, CEWithChunkedOutputLoss())
    assert abs(plain.item() - loss.item()) > 1e-4 * abs(loss.item())        # without input_pos the documents see each other
    model.eval()
    with torch.no_grad():
        l_eval = compute_loss(dbatch, model, CEWithChunkedOutputLoss())
    assert abs(l_eval.item() - loss.item()) <= 1e-6 * abs(loss.item()) + (1e-3 if bf16 else 0)


# ---- generation -----------------------------------------------------------------------------------------------------------------------
def _walk_rows(n, S, seed):
    rs = np.random.RandomState(seed)
    return list(torch.from_numpy(rs.randint(0, GEOMETRY_3B["vocab_size"], size=(n, S)).astype(np.int64)))


def test_teacher_forced_logits_fp32(base, weights, oracle):
    """``test_generate_model_gpu.teacher_forced_walk``: ragged prompts (1 and 17 tokens) in one ``prefill``, then every further token through
    ``decode_step``; the logits of the prefill and of every step within ``1e-4 * logits_absmax`` of the oracle's, ``cache.errors == 0`` (the
    walk asserts it)."""
    S = 33
    rows = _walk_rows(2, S, SEED + 1)
    want = [base.oracle_logits(oracle, r) for r in rows]
    absmax = max(float(w.abs().max()) for w in want)
    got = base.teacher_forced_walk(_model(weights, torch.float32), rows, (1, 17))
    assert len(got) == 2 * S - 1 - 17 + 2
    worst = max(float((g.double() - want[i][pos]).abs().max()) for i, pos, g in got)
    print(f"fp32: decode logits max-abs error {worst:.3e}, tolerance {1e-4 * absmax:.3e}")
    for i, pos, g in got:
        err = float((g.double() - want[i][pos]).abs().max())
        assert err <= 1e-4 * absmax, f"row {i} position {pos}: {err} > {1e-4 * absmax}"


def test_teacher_forced_logits_bf16(base, weights, oracle):
    """The same walk with 5 sequences in bf16 (the padded 256-row step): the decode logits at most 2 x as far from the fp32 oracle as the
    model's own bf16 full forward, measured here — the criterion of ``test_teacher_forced_logits_bf16_on_the_mfma_path``."""
    S = 40
    rows = _walk_rows(5, S, SEED + 2)
    want = [base.oracle_logits(oracle, r) for r in rows]
    model = _model(weights, torch.bfloat16)
    model.eval()
    with torch.no_grad():
        full = model(tokens=torch.stack(rows).to(DEV)).double().cpu()
    full_err = max(float((full[i] - want[i]).abs().max()) for i in range(5))
    got = base.teacher_forced_walk(model, rows, (1, 17, 5, 9, 30))
    dec_err = max(float((g.double() - want[i][pos]).abs().max()) for i, pos, g in got)
    print(f"bf16: decode {dec_err:.4e}, own full forward {full_err:.4e} from the fp32 oracle (ratio {dec_err / full_err:.2f})")
    assert dec_err <= 2.0 * full_err


# ---- small_batch=True -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bf16_model(weights):
    m = _model(weights, torch.bfloat16)
    m.eval()
    return m


def _prompts(n, seed=7):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, GEOMETRY_3B["vocab_size"], size=int(rs.randint(2, 12))).tolist() for _ in range(n)]


@pytest.mark.parametrize("rows", (1, 5, 64))
def test_a_flagged_decode_step_is_the_plain_step(bf16_model, rows):
    """``decode_step(..., small_batch=True)`` does not raise and — a shape off the skinny path keeps the tile path, launch for launch — gives
    the logits of the call without the flag, bit for bit."""
    model = bf16_model
    assert model._mfma_shapes() and not model.takes_small_batch(rows, True)
    prompts = _prompts(rows)
    tok = torch.arange(rows, dtype=torch.int64, device=DEV) + 11
    slot = torch.arange(rows, dtype=torch.int32, device=DEV)
    got = {}
    for flag in (False, True):
        cache = model.new_kv_cache(rows, 16)
        model.prefill(cache, prompts, max_new_tokens=2)
        first = model.decode_step(cache, tok, slot, small_batch=flag)
        got[flag] = (first, model.decode_step(cache, tok + 1, slot, small_batch=flag))
        assert int(cache.errors) == 0 and cache.lengths.cpu().tolist() == [len(p) + 2 for p in prompts]
    for plain, flagged in zip(got[False], got[True]):
        assert plain.shape == (rows, model.vocab_pad) and bool(torch.isfinite(plain.float()).all())
        assert torch.equal(plain, flagged)
    assert not [n for n in model._arena.buf if n.endswith(".s")]              # no buffer of the skinny path was ever asked for


class _Tok:
    special_tokens = {"<|eot_id|>": 699}
    eos_id, eom_id, eot_id, pad_id = 697, 698, 699, 0

    def decode(self, ids, **kw):
        return " ".join(str(t) for t in ids)


def test_generate_with_the_flag_counts_no_small_batch_group(bf16_model, tmp_path):
    """``generate(..., small_batch=True)`` gives the tokens and log-probabilities of the plain call, and the run summary of ``generate_file``
    says that no group took the skinny path."""
    from ssi.generate import generate, generate_file
    prompts = _prompts(5)
    kw = dict(max_new_tokens=6, stop_token_ids=[], pad_id=0, logprobs=True)
    plain = generate(bf16_model, prompts, **kw)
    report = {}
    flagged = generate(bf16_model, prompts, small_batch=True, small_batch_report=report, **kw)
    assert [(g.token_ids, g.cumulative_logprob) for g in flagged] == [(g.token_ids, g.cumulative_logprob) for g in plain]
    assert all(len(g.token_ids) == 6 for g in flagged) and report.get("small_batch_groups", 0) == 0
    summary = generate_file(bf16_model, _Tok(), None, str(tmp_path / "g.jsonl"), max_new_tokens=6, stop_token_ids=[], prompts=prompts,
                            small_batch=True)
    assert summary["small_batch_groups"] == 0 and summary["items"] == 5 and summary["generated_tokens"] == 30


def test_the_prompt_tool_returns_tokens(bf16_model):
    """``ssi.prompting.probe`` always passes ``small_batch=True``: one short prompt comes back with its tokens."""
    from ssi.prompting import probe
    found = probe(bf16_model, _Tok(), [[5, 6, 7]], max_new_tokens=4, stop_token_ids=[])
    assert len(found) == 1 and found[0].prompt_ids == [5, 6, 7] and len(found[0].generations) == 1
    g = found[0].generations[0]
    assert len(g.token_ids) == 4 and all(0 <= t < GEOMETRY_3B["vocab_size"] for t in g.token_ids) and g.cumulative_logprob is not None
    assert found[0].texts == [" ".join(str(t) for t in g.token_ids)]
