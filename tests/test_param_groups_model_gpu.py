"""GPU: parameter groups (``param_groups`` rules -> segments of the flat buffer) through the optimizer, the backward and the trainer, on the small
MFMA geometry of ``tests/test_trainer_gpu.py`` in bf16 and one tiny fp32 model.

* nothing frozen (an lr scale on the new rows, no decay on the norm scales): two steps through ``HipAdamW.step()`` and through the
  under-backward path give parameters and moments bit-equal to per-segment launches of the plain kernel on clones fed the same gradients;
* stage-1 rules (only the new rows of the tied embedding train) through ``Trainer.train()``: what is frozen does not move, no weight-gradient
  GEMM writes a fully frozen weight, the head's weight gradient covers the row span only, armed and unarmed runs are bit-equal;
* the gradient of the trainable rows under stage 1 against the unruled backward's (the launch shapes differ: the bound is the one
  ``tests/test_model_gpu.py`` uses for weight gradients computed by a different launch, ``2**-6 max|g|``; ``bf16_dist`` reports the rest);
* clipping takes the norm over the trainable ranges only (the frozen gradient memory holds NaN); resume is bit-exact and the saved optimizer
  state has today's keys."""
import math
import os

import pytest
import torch

from test_trainer_gpu import MFMA_SMALL, _Remap

pytestmark = pytest.mark.gpu
DEV = "cuda"
EMB = "tok_embeddings.weight"
BF16_MODEL = dict(vocab_size=368, num_layers=2, num_heads=4, num_kv_heads=2, embed_dim=256, max_seq_len=512, intermediate_dim=512)
BF16_TYPES = {"text": (0, 299), "special_text": (300, 315), "dsu": (316, 365), "modality": (366, 367)}
F32_MODEL = dict(vocab_size=72, num_layers=1, num_heads=2, num_kv_heads=1, embed_dim=32, max_seq_len=64, intermediate_dim=64)
F32_TYPES = {"text": (0, 49), "dsu": (50, 69), "modality": (70, 71)}
STAGE1 = [{"params": [EMB], "token_types": ["dsu", "modality"]}, {"params": ["*"], "frozen": True}]
SCALED = [{"params": [EMB], "token_types": ["dsu", "modality"], "lr_scale": 4.0}, {"params": ["*.scale"], "weight_decay": 0.0}]
HYPER = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


def _model(params, dtype, seed=11):
    from ssi.model import HipLlamaDecoder
    model = HipLlamaDecoder(**params, dtype=dtype, device=DEV)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_((torch.randn(p.shape, generator=g) * 0.05).to(dtype))
    model.set_num_output_chunks(8)
    model.train()
    return model


def _segments(model, rules, types):
    from ssi.param_groups import model_layout, resolve
    layout, total = model_layout(model)
    return resolve(rules, layout, total, types)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- nothing frozen ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params,types,dtype,sr", [(BF16_MODEL, BF16_TYPES, torch.bfloat16, False), (BF16_MODEL, BF16_TYPES, torch.bfloat16, True),
                                                   (F32_MODEL, F32_TYPES, torch.float32, False)], ids=["bf16", "bf16-sr", "fp32"])
@pytest.mark.parametrize("under_backward", [False, True], ids=["step", "under-backward"])
def test_lr_scale_and_no_decay_equal_per_segment_launches_of_the_plain_kernel(params, types, dtype, sr, under_backward):
    from ssi import ops
    from ssi.optimizer import HipAdamW, scale_grads
    model = _model(params, dtype)
    segs = _segments(model, SCALED, types)
    assert len(segs) >= 4 and not any(s.frozen for s in segs) and {s.lr_scale for s in segs} == {1.0, 4.0}
    opt = HipAdamW(model.parameters(), model=model, stochastic_rounding=sr, stochastic_rounding_seed=77 if sr else None, param_segments=segs, **HYPER)
    P, M, V = model._flat.clone(), torch.zeros_like(model._flat), torch.zeros_like(model._flat)
    gen = torch.Generator().manual_seed(5)
    for step in (1, 2):
        G = (torch.randn(model._flat.numel(), generator=gen) * 30.0).to(dtype).to(DEV)
        model._flat_grad.copy_(G)
        model.attach_grads()
        scale = torch.full((1,), float(torch.tensor(1 / 37)), dtype=torch.float32, device=DEV)
        if under_backward:   # what the window's last backward does: every bucket announced once, in its order
            assert opt.overlap_with_backward(scale)
            listener = model.bucket_listener
            for bucket in model.buckets:
                listener(*bucket)
        else:
            scale_grads(model, torch.tensor(1 / 37))
        opt.step()
        opt.zero_grad(set_to_none=True)
        for s in segs:   # the oracle: the plain kernel on this segment's slice alone
            sl = slice(s.start, s.end)
            ops.adamw_step(P[sl], G[sl], M[sl], V[sl], lr=HYPER["lr"] * s.lr_scale, beta1=0.9, beta2=0.999, eps=1e-8,
                           weight_decay=HYPER["weight_decay"] if s.weight_decay is None else s.weight_decay, step=step, grad_scale_dev=scale,
                           sr_seed=77 if sr else None, elem_offset=s.start)
        torch.cuda.synchronize()
        for name, x, y in (("param", model._flat, P), ("exp_avg", opt._exp_avg, M), ("exp_avg_sq", opt._exp_avg_sq, V)):
            assert torch.equal(_bits(x), _bits(y)), (name, step)
    assert opt._step_count == 2 and list(opt.state_dict()["param_groups"][0]) == list(HipAdamW(model.parameters(), model=model, **HYPER).state_dict()["param_groups"][0])


# ---- stage 1 through the trainer ----------------------------------------------------------------------------------------------------------
def _trainer(tmp, name, rules, dtype="bf16", overrides=(), model=MFMA_SMALL, seq=128):
    from conftest import PKG
    from ssi.config import compose
    from ssi.constants import SEED
    from ssi.train_utils import resolve_n_dsus
    from ssi.trainer import Trainer, set_seed
    out = tmp / name
    cfg = compose(os.path.join(PKG, "conf"), "sft", [
        "data=sft/mls-speechtokenizer-rvq_0", f"dtype={dtype}", f"tokenizer.max_seq_len={seq}", "data.train.dataloader.batch_size=2",
        "data.dev.dataloader.batch_size=2", "data.train.dataset.n_samples=24", "data.dev.dataset.n_samples=6", "gradient_accumulation_steps=2",
        "eval_steps=1000", "save_steps=1000", "lr_scheduler.num_warmup_steps=100", "optimizer.lr=2e-2", f"output_dir={out}",
        f"checkpointer.output_dir={out}/checkpoints", f"checkpointer.checkpoint_dir={out}/none", "checkpointer.allow_random_init=true", *overrides])
    cfg.model_overrides = dict(model)
    cfg.speech.n_dsus = 50
    cfg.data.n_dsus = 50
    if rules is not None:
        cfg.param_groups = rules
    resolve_n_dsus(cfg)
    set_seed(SEED)
    t = Trainer(cfg)
    t.setup()
    V = t._llama_config.vocab_size
    t.data_train, t.data_dev = _Remap(t.data_train, V), _Remap(t.data_dev, V)
    t._loss_log = []
    return t


def _trainable_rows(t):
    rows = torch.zeros(t._llama_config.vocab_size, dtype=torch.bool)
    for kind in ("dsu", "modality"):
        lo, hi = t.token_type_ranges[kind]
        rows[lo:hi + 1] = True
    return rows


def _record_wgrad_launches(monkeypatch, model, log):
    from ssi import ops
    G = model._flat_grad
    for fn in ("gemm", "gemm_splitk", "gemm_batched"):
        real = getattr(ops, fn)

        def wrapped(layout, a, b, c, *args, _real=real, _fn=fn, **kw):
            if layout == ops.GEMM_TN:
                off = (c.data_ptr() - G.data_ptr()) // G.element_size()
                assert 0 <= off < G.numel(), "a weight-gradient GEMM writes outside the gradient buffer"
                if c.dim() == 3:   # batched: one range per layer of the group
                    log.extend((_fn, off + k * c.stride(0), off + k * c.stride(0) + c.shape[1] * c.shape[2]) for k in range(c.shape[0]))
                else:
                    log.append((_fn, off, off + c.shape[0] * c.shape[1]))
            return _real(layout, a, b, c, *args, **kw)

        monkeypatch.setattr(ops, fn, wrapped)


def test_stage_one_through_the_trainer(tmp_path, monkeypatch):
    base = _trainer(tmp_path, "none", None, overrides=["max_steps=2"])
    init = {k: v.detach().clone() for k, v in base.model.state_dict().items()}
    base.train()
    loss_unruled = list(base._loss_log)
    base.cleanup()
    del base
    runs = {}
    for name, extra in (("armed", []), ("off", ["adamw_under_backward=false"])):
        t = _trainer(tmp_path, name, STAGE1, overrides=["max_steps=2", *extra])
        rows = _trainable_rows(t)
        assert 0 < int(rows.sum()) < rows.numel()
        for k, p in t.model.named_parameters():
            assert torch.equal(p.detach(), init[k]), k                                  # (same seeded weights as the unruled run)
            assert p.requires_grad == (k == EMB) and p.grad is None
        launches = []
        _record_wgrad_launches(monkeypatch, t.model, launches)
        armed = []
        real = t.optimizer.overlap_with_backward
        t.optimizer.overlap_with_backward = lambda s, real=real, armed=armed: (armed.append(1), real(s))[1]
        t.train()
        torch.cuda.synchronize()
        assert len(armed) == (2 if name == "armed" else 0) and t.optimizer._step_count == 2
        # no weight-gradient GEMM wrote a fully frozen weight; the only one left is the head's, over the 256-aligned span of the new rows
        m = t.model
        assert launches and all(not m._range_frozen(lo, hi) for _, lo, hi in launches), launches
        r0, r1 = m._emb_span
        first, last = int(rows.nonzero()[0]), int(rows.nonzero()[-1])
        assert r0 % 256 == 0 and r0 <= first and last < r1 and (r0, r1) != (0, m.vocab_pad), (r0, r1, first, last, m.vocab_pad)
        assert {(lo, hi) for _, lo, hi in launches} == {(r0 * m.embed_dim, r1 * m.embed_dim)} and len(launches) >= 2   # one per head backward
        sd = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
        rows = rows.to(DEV)
        opt_sd = t.optimizer.state_dict()
        by_name = dict(zip([k for k, _ in t.model.named_parameters()], [opt_sd["state"][i] for i in range(len(opt_sd["state"]))]))
        for k, v in sd.items():
            if k == EMB:
                assert torch.equal(v[~rows], init[k][~rows]), "a frozen embedding row moved"
                assert not torch.equal(v[rows], init[k][rows]), "the trainable rows did not move"
                for mom in ("exp_avg", "exp_avg_sq"):
                    assert not by_name[k][mom][:rows.numel()][~rows].float().any() and by_name[k][mom][:rows.numel()][rows].float().any()
            else:
                assert torch.equal(v, init[k]), k
                assert not by_name[k]["exp_avg"].float().any() and not by_name[k]["exp_avg_sq"].float().any(), k
        for k, p in t.model.named_parameters():
            assert p.requires_grad == (k == EMB) and (p.grad is None or k == EMB)
        runs[name] = (list(t._loss_log), sd)
        t.cleanup()
        monkeypatch.undo()
        del t
    assert runs["armed"][0][0] == loss_unruled[0]                                        # step 1: the same forward on the same weights
    assert runs["armed"][0] == runs["off"][0] and all(torch.equal(runs["armed"][1][k], runs["off"][1][k]) for k in init)


# ---- the gradient the head computes for the span, clipping ------------------------------------------------------------------------------------
def test_trainable_rows_gradient_and_the_clip_norm():
    from bf16_dist import bf16_distance
    from oracle import hf_crosscheck as hx
    from ssi.loss import CEWithChunkedOutputLoss, compute_loss
    from ssi.optimizer import HipAdamW, clip_grad_norm_, scale_grads
    from ssi.param_groups import trainable_ranges
    batch = {k: v.to(DEV) for k, v in hx.seeded_batch(BF16_MODEL["vocab_size"], 2, 128, 9).items()}
    n = int((batch["labels"] != -100).sum())
    plain, ruled = _model(BF16_MODEL, torch.bfloat16), _model(BF16_MODEL, torch.bfloat16)
    segs = _segments(ruled, STAGE1, BF16_TYPES)
    opt = HipAdamW(ruled.parameters(), model=ruled, param_segments=segs, **HYPER)
    for m in (plain, ruled):
        (compute_loss(batch, m, CEWithChunkedOutputLoss()) * n).backward()
    rows = torch.zeros(BF16_MODEL["vocab_size"], dtype=torch.bool)
    rows[316:368] = True
    g, ref = ruled.tok_embeddings.weight.grad[rows.to(DEV)], plain.tok_embeddings.weight.grad[rows.to(DEV)]
    eq, steps = bf16_distance(g.cpu(), ref.cpu(), floor=float(ref.float().abs().max()) * 2 ** -7)
    diff = float((g.float() - ref.float()).abs().max())
    print(f"trainable rows' gradient, span launch against whole-vocabulary launch: {eq:.4f} bit-equal, {steps:.2f} bf16 steps, max |diff| {diff:.3e}")
    assert float(ref.float().abs().max()) > 0 and diff <= 2 ** -6 * float(ref.float().abs().max())
    assert all(p.grad is None for k, p in ruled.named_parameters() if k != EMB)
    # clipping: the frozen ranges of the gradient buffer are unspecified — NaN here — and the norm is the trainable ranges' alone
    G = ruled._flat_grad
    for s in segs:
        if s.frozen:
            G[s.start:s.end] = float("nan")
    scale = 1 / n
    norm64 = math.sqrt(sum(float((G[lo:hi].double() * float(torch.tensor(scale))).square().sum()) for lo, hi in trainable_ranges(segs)))
    scale_grads(ruled, torch.tensor(scale))
    max_norm = norm64 / 2
    total = float(clip_grad_norm_(ruled, max_norm))
    assert math.isfinite(total) and abs(total - norm64) / norm64 <= 1e-7, (total, norm64)   # the bound of the existing clip test
    before = ruled._flat.clone()
    opt.step()
    torch.cuda.synchronize()
    assert bool(ruled._flat.float().isfinite().all())
    moved = (ruled._flat != before)
    assert bool(moved.any()) and all(not bool(moved[s.start:s.end].any()) for s in segs if s.frozen)


# ---- resume ---------------------------------------------------------------------------------------------------------------------------------
def test_resume_with_rules_is_bit_exact_and_the_state_is_todays(tmp_path):
    from safetensors import safe_open
    from ssi.constants import OPTIMIZER_KEY
    full = _trainer(tmp_path, "full", STAGE1, overrides=["max_steps=4"])
    full.train()
    losses = list(full._loss_log)
    final = {k: v.detach().clone() for k, v in full.model.state_dict().items()}
    m_full = full.optimizer._exp_avg.clone()
    full.cleanup()
    del full
    b1 = _trainer(tmp_path, "b1", STAGE1, overrides=["max_steps=2", "save_steps=2", "eval_steps=2"])
    b1.train()
    b1.cleanup()
    names = [k for k, _ in b1.model.named_parameters()]
    del b1
    ckpt = tmp_path / "b1" / "checkpoints"
    state = torch.load(ckpt / "training_state.pt", map_location="cpu", weights_only=False)[OPTIMIZER_KEY]
    assert len(state["param_groups"]) == 1 and len(state["param_groups"][0]["params"]) == len(names) == len(state["state"])
    with safe_open(str(ckpt / "step_2" / "model.safetensors"), "pt") as f:
        assert len(list(f.keys())) >= len(names)                                         # every parameter, frozen or not
    resume = [f"checkpointer.checkpoint_dir={ckpt}/step_2", "checkpointer.allow_random_init=false",
              f"checkpointer.training_state_checkpoint={ckpt}/training_state.pt"]
    b2 = _trainer(tmp_path, "b2", STAGE1, overrides=["max_steps=4", *resume])
    assert b2.global_step == 2 and b2.optimizer._step_count == 2
    b2.train()
    assert b2._loss_log == losses[2:]
    assert all(torch.equal(v, final[k]) for k, v in b2.model.state_dict().items()) and torch.equal(b2.optimizer._exp_avg, m_full)
    ruled_state = b2.optimizer.state_dict()
    b2.cleanup()
    del b2
    # a state saved under the rules resumes without them (everything trains from there) ...
    b3 = _trainer(tmp_path, "b3", None, overrides=["max_steps=3", *resume])
    assert b3.optimizer._segments is None and b3.optimizer._step_count == 2 and all(p.requires_grad for p in b3.model.parameters())
    b3.train()
    assert len(b3._loss_log) == 1 and math.isfinite(b3._loss_log[0])
    assert any(not torch.equal(v, final[k]) for k, v in b3.model.state_dict().items() if k != EMB)   # what the rules froze trains now
    unruled_state = b3.optimizer.state_dict()
    # ... and the other way round: the optimizer's state is the same one torch group either way
    assert list(unruled_state["param_groups"][0]) == list(ruled_state["param_groups"][0]) == list(state["param_groups"][0])
    from ssi.optimizer import HipAdamW
    other = HipAdamW(b3.model.parameters(), model=b3.model, param_segments=_segments(b3.model, STAGE1, b3.token_type_ranges), lr=2e-2)
    other.load_state_dict(unruled_state)
    assert other._step_count == 3 and torch.equal(other._exp_avg, b3.optimizer._exp_avg)
    b3.cleanup()
