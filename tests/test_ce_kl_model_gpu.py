"""GPU: the KL term against a frozen teacher from the model up — ``HipLlamaDecoder.fused_loss(teacher=, teacher_kl_coeff=, teacher_kl_ranges=)``,
``compute_loss`` with the same keywords on both routes, and the trainer's ``teacher_kl_coeff`` (``loss`` stays the cross-entropy part, ``kl_loss``
joins the record, ``dev_loss`` never sees the teacher, and the teacher is never optimised or saved).

The small models and batches are those of ``tests/test_ce_z_model_gpu.py``, and so are the bounds of the route agreement: fp32 loss 1e-5
relative, gradients rtol 5e-3, atol 1e-6; bf16 loss 1e-2 relative, gradients 5e-2 of the norm of the difference per parameter.  The teacher is a
second model with the student's weights plus seeded noise of 2 % of each tensor's RMS.

The KL part is small against this teacher (4e-4 to 9e-4) and is held to the same relative bound as the other parts: 1e-5 of it in fp32 is 6e-9.
A row's KL is then a small difference of two log-sum-exps whose fp32 rounding alone (2.4e-7 at an lse of 6.3) leaves 2e-8 in the mean over the
~170 labelled rows, so both routes carry the rows' normalisers in fp64: the generic kernel form (the one fp32 takes) sums them beside the KL,
the literal route takes its ``log_softmax`` in fp64."""
import os

import pytest
import torch
import torch.nn.functional as F

from test_ce_metrics_gpu import _model
from test_ce_smooth_model_gpu import _assert_grads_close
from test_ce_z_model_gpu import TIMING, _batch, _Literal, _loss_and_grads, _shifted

pytestmark = pytest.mark.gpu

DEV = "cuda"
B = 0.5
KL_ATOL = 2e-5                      # the kernel's atol on row_kl (tests/test_ce_kl_gpu.py), k = 1


def _teacher(dtype, student, noise=0.02):
    teacher = _model(dtype)
    sd = {k: v.detach().clone() for k, v in student.state_dict().items()}
    g = torch.Generator().manual_seed(11)
    if noise:
        for k, v in sd.items():
            rms = float(v.float().pow(2).mean().sqrt())
            sd[k] = (v.float() + noise * rms * torch.randn(v.shape, generator=g).to(v.device)).to(v.dtype)
    teacher.load_state_dict(sd)
    teacher.eval()
    return teacher


def _kl_rows(model, teacher, batch):
    """KL(teacher || model) per position ``[B, S]`` in plain torch over the two models' literal logits (with grad to ``model``)."""
    kw = dict(tokens=batch["tokens"], input_pos=batch.get("input_pos"))
    logits = model(**kw)
    with torch.no_grad():
        t = teacher(**kw)
    x = (torch.cat(logits, dim=1) if isinstance(logits, list) else logits).float()
    t = (torch.cat(t, dim=1) if isinstance(t, list) else t).float()
    kl = F.kl_div(torch.log_softmax(x, -1), torch.log_softmax(t, -1), log_target=True, reduction="none").sum(-1)
    return x, kl


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_route_agrees_with_the_literal_route(dtype, packed):
    from ssi.loss import CEWithChunkedOutputLoss
    model = _model(dtype)
    model.train()
    teacher = _teacher(dtype, model)
    batch = _batch(packed, dtype)
    kw = dict(teacher=teacher, teacher_kl_coeff=B)
    fused, g_fused = _loss_and_grads(model, batch, CEWithChunkedOutputLoss(), **kw)
    parts_fused = (float(model.last_ce_loss), float(model.last_kl_loss))
    literal, g_lit = _loss_and_grads(model, batch, _Literal(), **kw)
    parts_lit = (float(model.last_ce_loss), float(model.last_kl_loss))
    plain, g_plain = _loss_and_grads(model, batch, CEWithChunkedOutputLoss())
    loss_tol = 1e-5 if dtype == torch.float32 else 1e-2
    print(f"fused {float(fused):.7f} = {parts_fused}, literal {float(literal):.7f} = {parts_lit}, without the teacher {float(plain):.7f}")
    assert parts_fused[1] > 0
    assert abs(float(fused) - float(literal)) <= loss_tol * abs(float(literal))
    for a, b in zip(parts_fused, parts_lit):
        assert abs(a - b) <= loss_tol * abs(b)
    _assert_grads_close(g_fused, g_lit, dtype)
    # ... and the KL term is in the gradient: the embedding gradient moves against the plain one as far as the literal route's does
    emb = "tok_embeddings.weight"
    moved = float((g_fused[emb] - g_plain[emb]).norm()) / float(g_plain[emb].norm())
    moved_lit = float((g_lit[emb] - g_plain[emb]).norm()) / float(g_plain[emb].norm())
    print(f"embedding gradient moved by {moved:.3e} of the plain one's norm (literal route {moved_lit:.3e})")
    assert moved > 0.1 * moved_lit > 0, (moved, moved_lit)


@pytest.mark.parametrize("ranges", [None, [(0, 257)]])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_with_loss_weights_and_ranges_against_torch_on_the_literal_logits(dtype, packed, ranges):
    """``sum_i (w_i nll_i + b k_i KL_i) / n_valid`` with ``k_i = w_i [label_i in a range]``, over the two models' literal logits."""
    from ssi.loss import CEWithChunkedOutputLoss
    model = _model(dtype)
    model.train()
    teacher = _teacher(dtype, model)
    batch = _batch(packed, dtype)
    w = 3.0 * torch.rand(batch["tokens"].shape, generator=torch.Generator().manual_seed(5))
    w[0, 30], w[1, 40] = 0.0, 1.0
    w = w.to(DEV)
    fused, g_fused = _loss_and_grads(model, {**batch, "loss_weights": w}, CEWithChunkedOutputLoss(), teacher=teacher, teacher_kl_coeff=B,
                                     teacher_kl_ranges=ranges)
    ce_fused, kl_fused = float(model.last_ce_loss), float(model.last_kl_loss)
    model.zero_grad()
    x, kl = _kl_rows(model, teacher, batch)
    y = _shifted(batch)
    valid = y != -100
    inside = torch.ones_like(valid) if ranges is None else (y >= ranges[0][0]) & (y <= ranges[0][1])
    assert ranges is None or 0 < int((valid & inside).sum()) < int(valid.sum())
    nll = torch.logsumexp(x, dim=-1) - x.gather(-1, torch.where(valid, y, torch.zeros_like(y))[..., None])[..., 0]
    ce = (w * valid * nll).sum() / valid.sum()
    klp = B * (w * (valid & inside) * kl).sum() / valid.sum()
    (ce + klp).backward()
    g_ref = {k: p.grad.detach().float().clone() for k, p in model.named_parameters()}
    loss_tol = 1e-5 if dtype == torch.float32 else 1e-2
    print(f"fused {float(fused):.7f} = {ce_fused:.7f} + {kl_fused:.7f}, torch on the literal logits {float(ce.detach()):.7f} + {float(klp.detach()):.7f}")
    assert abs(float(fused) - float((ce + klp).detach())) <= loss_tol * abs(float((ce + klp).detach()))
    assert abs(ce_fused - float(ce.detach())) <= loss_tol * abs(float(ce.detach())) and kl_fused > 0
    _assert_grads_close(g_fused, g_ref, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_teacher_identical_to_the_student_adds_nothing(dtype):
    from ssi.loss import CEWithChunkedOutputLoss
    model = _model(dtype)
    model.train()
    teacher = _teacher(dtype, model, noise=0.0)
    batch = _batch(False, dtype)
    total, g = _loss_and_grads(model, batch, CEWithChunkedOutputLoss(), teacher=teacher, teacher_kl_coeff=2.0)
    kl = float(model.last_kl_loss)
    plain, g_plain = _loss_and_grads(model, batch, CEWithChunkedOutputLoss())
    print(f"kl part {kl:.3e}")
    assert abs(kl) <= 2.0 * KL_ATOL and torch.equal(model.last_ce_loss, plain)
    _assert_grads_close(g, g_plain, dtype)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_the_default_path_is_untouched_and_the_teacher_stays_frozen(dtype, packed, monkeypatch):
    from ssi import ops
    from ssi.eval import LabelMetrics, SeqScores
    from ssi.loss import CEWithChunkedOutputLoss
    model = _model(dtype)
    model.train()
    teacher = _teacher(dtype, model)
    keep = {k: v.detach().clone() for k, v in teacher.state_dict().items()}
    batch = _batch(packed, dtype)
    calls = []
    real = ops.ce_fwd_kl
    monkeypatch.setattr(ops, "ce_fwd_kl", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    without, g_without = _loss_and_grads(model, batch, CEWithChunkedOutputLoss())
    zero, g_zero = _loss_and_grads(model, batch, CEWithChunkedOutputLoss(), teacher=teacher, teacher_kl_coeff=0.0)
    assert torch.equal(without, zero) and all(torch.equal(g_without[k], g_zero[k]) for k in g_zero)
    assert not calls and not [n for n in model._arena.buf if n.startswith("row_kl")] and "logits.t" not in teacher._arena.buf, \
        "coefficient 0 issued a KL launch, allocated a row_kl buffer or ran the teacher"
    with torch.no_grad():
        plain_eval = model.fused_loss(batch["tokens"], _shifted(batch), input_pos=batch.get("input_pos"))
    # the coefficient > 0 under grad: the total and the parts left on the model; the teacher untouched and without gradients
    total, _ = _loss_and_grads(model, batch, CEWithChunkedOutputLoss(), teacher=teacher, teacher_kl_coeff=B)
    assert len(calls) == 1 and "row_kl" in model._arena.buf and "logits.t" in teacher._arena.buf and "logits.t" not in model._arena.buf
    assert torch.equal(model.last_ce_loss, without), "last_ce_loss is not the loss of a forward without the option on the same weights"
    assert torch.equal(total, model.last_ce_loss + model.last_kl_loss) and float(model.last_kl_loss) > 0
    assert all(torch.equal(v, keep[k]) for k, v in teacher.state_dict().items()), "a training step wrote the teacher"
    assert all(p.grad is None for p in teacher.parameters())
    # ... and without grad: no gradient is written
    with torch.no_grad():
        total_eval = model.fused_loss(batch["tokens"], _shifted(batch), input_pos=batch.get("input_pos"), teacher=teacher, teacher_kl_coeff=B)
        assert len(calls) == 2 and "row_kl.x" in model._arena.buf
        assert torch.equal(model.last_ce_loss, plain_eval) and torch.equal(total_eval, model.last_ce_loss + model.last_kl_loss)
        args = (batch["tokens"], _shifted(batch))
        for name, kw in (("label_metrics", {"label_metrics": LabelMetrics({"a": (0, 99)}, 5, torch.device(DEV))}),
                         ("seq_scores", {"seq_scores": SeqScores([(0, 0, 8)], 5, torch.zeros(1, 4, dtype=torch.float64, device=DEV))}),
                         ("z_loss_coeff", {"z_loss_coeff": 1e-4}), ("label_smoothing", {"label_smoothing": 0.1})):
            with pytest.raises(ValueError, match="teacher_kl_coeff and " + name):
                model.fused_loss(*args, input_pos=batch.get("input_pos"), teacher=teacher, teacher_kl_coeff=B, **kw)
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="teacher_kl_coeff"):
            model.fused_loss(batch["tokens"], _shifted(batch), teacher=teacher, teacher_kl_coeff=bad)
    with pytest.raises(ValueError, match="teacher"):
        model.fused_loss(batch["tokens"], _shifted(batch), teacher_kl_coeff=B)                       # no teacher
    with pytest.raises(ValueError, match="teacher"):
        model.fused_loss(batch["tokens"], _shifted(batch), teacher=model, teacher_kl_coeff=B)        # the model itself
    assert len(calls) == 2


def test_a_teacher_of_another_vocabulary_or_dtype_is_refused():
    from ssi.model import HipLlamaDecoder
    model = _model(torch.float32)
    batch = _batch(False, torch.float32)
    other = HipLlamaDecoder(vocab_size=523, num_layers=1, num_heads=8, num_kv_heads=2, embed_dim=128, max_seq_len=256, intermediate_dim=256,
                            dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="vocab_size"):
        model.fused_loss(batch["tokens"], _shifted(batch), teacher=other, teacher_kl_coeff=B)
    other = HipLlamaDecoder(vocab_size=515, num_layers=1, num_heads=4, num_kv_heads=2, embed_dim=256, max_seq_len=256, intermediate_dim=256,
                            dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="dtype"):
        model.fused_loss(batch["tokens"], _shifted(batch), teacher=other, teacher_kl_coeff=B)


# ---- trainer --------------------------------------------------------------------------------------------------------------------------------
def _run(tmp_path, name, extra=()):
    from test_trainer_gpu import MFMA_SMALL, _trainer
    t = _trainer(tmp_path, name, dtype="bf16", model=MFMA_SMALL, seq=128,
                 overrides=["max_steps=3", "eval_steps=3", "save_steps=3", "data.train.dataset.fixed_len=false", "lr_scheduler.num_warmup_steps=0",
                            "optimizer.lr=2e-3", *extra])
    teacher_before = None if t.teacher is None else {k: v.detach().clone() for k, v in t.teacher.state_dict().items()}
    seen, real = [], t.model.fused_loss
    t.model.fused_loss = lambda *a, real=real, seen=seen, **k: (seen.append((torch.is_grad_enabled(), k.get("teacher") is not None,
                                                                             k.get("teacher_kl_coeff", 0.0), k.get("teacher_kl_ranges"))),
                                                                real(*a, **k))[1]
    t.train()
    again = t._evaluate()
    saved = sorted(os.listdir(tmp_path / name / "checkpoints" / "step_3"))
    from safetensors import safe_open
    names = []
    for f in saved:
        if f.endswith(".safetensors"):
            with safe_open(str(tmp_path / name / "checkpoints" / "step_3" / f), "pt") as fh:
                names += list(fh.keys())
    out = dict(rec=[{k: r[k] for k in r if k not in TIMING} for r in t.wandb_logger.records], dev_again=again, seen=list(seen), saved=saved,
               names=sorted(names), teacher=t.teacher, teacher_before=teacher_before, optimizer_params=sum(len(g["params"]) for g in t.optimizer.param_groups),
               model_params=len(list(t.model.parameters())), ranges=t.teacher_kl_ranges, text=t.token_type_ranges["text"])
    t.cleanup()
    return out


def test_trainer_logs_the_part_keeps_the_dev_loss_plain_and_the_teacher_frozen(tmp_path):
    on = _run(tmp_path, "on", ["teacher_kl_coeff=0.5", "teacher_kl_token_types=[text]"])
    off = _run(tmp_path, "off")
    assert [r["step"] for r in on["rec"]] == [1, 2, 3] == [r["step"] for r in off["rec"]]
    print([(r["loss"], r["kl_loss"]) for r in on["rec"]], [r["loss"] for r in off["rec"]])
    assert all("loss" in r and "kl_loss" in r for r in on["rec"]) and all("kl_loss" not in r for r in off["rec"])
    assert all(set(a) - set(b) == {"kl_loss"} and set(b) <= set(a) for a, b in zip(on["rec"], off["rec"]))
    # step 1: the same weights in both runs (the teacher is built from the model's own seeded initial weights): the cross-entropy part is that
    # of the run without the option; from step 2 on the model has left the teacher
    assert abs(on["rec"][0]["loss"] - off["rec"][0]["loss"]) <= 1e-2 * abs(off["rec"][0]["loss"])
    # (the synthetic rows carry their labels on speech units: on text labels alone the part is an exact 0 here, and the gradient the plain one)
    everywhere = _run(tmp_path, "everywhere", ["teacher_kl_coeff=0.5"])
    print([(r["loss"], r["kl_loss"]) for r in everywhere["rec"]])
    assert everywhere["ranges"] is None and all(r["kl_loss"] > 0 for r in everywhere["rec"][1:])
    assert abs(everywhere["rec"][0]["loss"] - off["rec"][0]["loss"]) <= 1e-2 * abs(off["rec"][0]["loss"])
    assert everywhere["names"] == off["names"]
    # every training forward got the teacher, the coefficient and the text range; no forward without grad (the dev loss) ever did
    assert on["ranges"] == [tuple(on["text"])]
    assert all(t and b == 0.5 and r == on["ranges"] for grad, t, b, r in on["seen"] if grad)
    assert all(not t and b == 0.0 for grad, t, b, r in on["seen"] if not grad)
    assert any(grad for grad, *_ in on["seen"]) and any(not grad for grad, *_ in on["seen"])
    assert "dev_loss" in on["rec"][2] and on["rec"][2]["dev_loss"] == on["dev_again"]
    # the teacher: bitwise what it was, no gradients, not in the optimizer, not in the checkpoint
    assert off["teacher"] is None and on["teacher"] is not None and not on["teacher"].training
    assert all(torch.equal(v, on["teacher_before"][k]) for k, v in on["teacher"].state_dict().items())
    assert all(p.grad is None for p in on["teacher"].parameters())
    assert on["optimizer_params"] == off["optimizer_params"] <= on["model_params"]
    assert on["saved"] == off["saved"] and on["names"] == off["names"] and on["names"]


def test_trainer_setup_refuses_an_unknown_token_type_and_a_missing_teacher(tmp_path):
    from test_trainer_gpu import MFMA_SMALL, _trainer
    common = dict(dtype="bf16", model=MFMA_SMALL, seq=128)
    with pytest.raises(ValueError, match="teacher_kl_token_types names"):
        _trainer(tmp_path, "kinds", overrides=["teacher_kl_coeff=0.5", "teacher_kl_token_types=[words]"], **common)
    # the model itself may start from seeded random weights here; a teacher directory that holds no model, and no leave to make one up
    t = _trainer(tmp_path, "dir", overrides=["teacher_kl_coeff=0.5"], **common)
    ck = {k: t.cfg.checkpointer[k] for k in t.cfg.checkpointer}
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError, match="teacher_checkpoint_dir"):
        t._setup_teacher({**ck, "checkpoint_dir": str(empty), "allow_random_init": False})
    t.cleanup()
