"""GPU: the auxiliary z-loss from the model up — ``HipLlamaDecoder.fused_loss(z_loss_coeff=)``, ``compute_loss(z_loss_coeff=)`` on both routes,
and the trainer's ``z_loss_coeff`` (``loss`` stays the cross-entropy part, ``z_loss`` joins the record, ``dev_loss`` never sees the coefficient).

The small models are those of ``tests/test_ce_metrics_gpu.py``.  Route agreement (fused against literal) uses the bounds the fused route is held
to against the oracle in ``tests/test_model_gpu.py`` — there is no fused-against-literal test there to take them from:
fp32 ``test_fp32_model_matches_live_oracle_on_ragged_batch_with_ignored_row`` (loss 1e-5 relative; gradients rtol 5e-3, atol 1e-6), bf16
``test_bf16_model_close_to_fp32_oracle`` (loss 1e-2 relative; gradients 5e-2 of the norm, applied here to the norm of the DIFFERENCE per
parameter, which bounds the difference of the norms)."""
import pytest
import torch

from test_ce_metrics_gpu import _model, _model_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda"
Z = 0.05   # vocabulary 515: lse ~ 6.3, f = 1 + 2 z lse ~ 1.6 — the z part moves every gradient visibly


class _Literal:
    """A loss_fn that is not ``CEWithChunkedOutputLoss``: ``compute_loss`` takes the literal route ``loss_fn(model(...), labels)``."""
    ignore_index = -100

    def __init__(self):
        from ssi.loss import CEWithChunkedOutputLoss
        self.inner = CEWithChunkedOutputLoss()

    def __call__(self, logits, labels):
        return self.inner(logits, labels)


def _batch(packed, dtype):
    S = 96 if dtype == torch.float32 else 128
    tokens, input_pos = _model_inputs(packed, S)
    labels = tokens.clone()                      # unshifted, as a batch carries them; compute_loss shifts
    labels[0, 5:19] = -100
    labels[1, :9] = -100
    batch = {"tokens": tokens.to(DEV), "labels": labels.to(DEV)}
    if input_pos is not None:
        batch["input_pos"] = input_pos.to(DEV)
    return batch


def _shifted(batch):
    labels = batch["labels"]
    return torch.hstack((labels[..., 1:], torch.full_like(labels[..., -1:], -100)))


def _grads(model):
    return {k: p.grad.detach().float().clone() for k, p in model.named_parameters()}


def _loss_and_grads(model, batch, loss_fn, **kw):
    from ssi.loss import compute_loss
    model.zero_grad()
    loss = compute_loss(batch, model, loss_fn, **kw)
    loss.backward()
    return loss.detach().clone(), _grads(model)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_route_agrees_with_the_literal_route(dtype, packed):
    from ssi.loss import CEWithChunkedOutputLoss
    model = _model(dtype)
    model.train()
    batch = _batch(packed, dtype)
    fused, g_fused = _loss_and_grads(model, batch, CEWithChunkedOutputLoss(), z_loss_coeff=Z)
    parts_fused = (float(model.last_ce_loss), float(model.last_z_loss))
    literal, g_lit = _loss_and_grads(model, batch, _Literal(), z_loss_coeff=Z)
    parts_lit = (float(model.last_ce_loss), float(model.last_z_loss))
    plain, g_plain = _loss_and_grads(model, batch, CEWithChunkedOutputLoss())
    loss_tol = 1e-5 if dtype == torch.float32 else 1e-2
    print(f"fused {float(fused):.7f} = {parts_fused}, literal {float(literal):.7f} = {parts_lit}, without z {float(plain):.7f}")
    assert parts_fused[1] > 0.1 * parts_fused[0] > 0            # the z part is no rounding error of the total
    assert abs(float(fused) - float(literal)) <= loss_tol * abs(float(literal))
    for a, b in zip(parts_fused, parts_lit):
        assert abs(a - b) <= loss_tol * abs(b)
    worst = 0.0
    for k in g_lit:
        if dtype == torch.float32:
            torch.testing.assert_close(g_fused[k], g_lit[k], rtol=5e-3, atol=1e-6, msg=lambda m, k=k: f"{k}: {m}")
        else:
            rel = float((g_fused[k] - g_lit[k]).norm()) / (float(g_lit[k].norm()) + 1e-30)
            worst = max(worst, rel)
            assert float((g_fused[k] - g_lit[k]).norm()) <= 5e-2 * float(g_lit[k].norm()) + 1e-6, (k, rel)
        # ... and the z part is in the gradient: without it the gradients are far away by the same measure
    print(f"worst relative gradient difference (bf16 only) {worst:.3e}")
    moved = float((g_fused["tok_embeddings.weight"] - g_plain["tok_embeddings.weight"]).norm()) / float(g_plain["tok_embeddings.weight"].norm())
    assert moved > 0.1, moved


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_the_default_path_is_untouched_and_the_scalars_are_the_parts(dtype, packed, monkeypatch):
    from ssi import ops
    from ssi.eval import LabelMetrics
    from ssi.loss import CEWithChunkedOutputLoss
    model = _model(dtype)
    model.train()
    batch = _batch(packed, dtype)
    calls = []
    real = ops.ce_fwd_z
    monkeypatch.setattr(ops, "ce_fwd_z", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    without, g_without = _loss_and_grads(model, batch, CEWithChunkedOutputLoss())
    zero, g_zero = _loss_and_grads(model, batch, CEWithChunkedOutputLoss(), z_loss_coeff=0.0)
    assert torch.equal(without, zero) and all(torch.equal(g_without[k], g_zero[k]) for k in g_zero)
    with torch.no_grad():
        plain_eval = model.fused_loss(batch["tokens"], _shifted(batch), input_pos=batch.get("input_pos"), z_loss_coeff=0.0)
    assert not calls and not [n for n in model._arena.buf if n.startswith("row_z")], "z = 0 issued a z launch or allocated a row_z buffer"
    assert model.last_ce_loss is None and model.last_z_loss is None
    # z > 0 under grad: the total, and the two parts left on the model
    total, _ = _loss_and_grads(model, batch, CEWithChunkedOutputLoss(), z_loss_coeff=Z)
    assert len(calls) == 1 and "row_z" in model._arena.buf
    assert torch.equal(model.last_ce_loss, without), "last_ce_loss is not the loss of a z = 0 forward on the same weights"
    assert torch.equal(total, model.last_ce_loss + model.last_z_loss) and float(model.last_z_loss) > 0
    # ... and without grad
    with torch.no_grad():
        total_eval = model.fused_loss(batch["tokens"], _shifted(batch), input_pos=batch.get("input_pos"), z_loss_coeff=Z)
        assert len(calls) == 2 and "row_z.x" in model._arena.buf
        assert torch.equal(model.last_ce_loss, plain_eval) and torch.equal(total_eval, model.last_ce_loss + model.last_z_loss)
        with pytest.raises(ValueError, match="label_metrics"):
            model.fused_loss(batch["tokens"], _shifted(batch), input_pos=batch.get("input_pos"), z_loss_coeff=Z,
                             label_metrics=LabelMetrics({"a": (0, 99)}, 5, torch.device(DEV)))
    for bad in (-1e-3, float("nan")):
        with pytest.raises(ValueError, match="z_loss_coeff"):
            model.fused_loss(batch["tokens"], _shifted(batch), z_loss_coeff=bad)


# ---- trainer --------------------------------------------------------------------------------------------------------------------------------
TIMING = ("duration_step", "tokens_per_second_per_gpu", "train_clock_time")


def _run(tmp_path, name, dtype, extra=(), config_name="sft", label_first=False):
    from test_trainer_gpu import MFMA_SMALL, SMALL, _trainer
    t = _trainer(tmp_path, name, config_name=config_name, dtype=dtype, model=SMALL if dtype == "fp32" else MFMA_SMALL,
                 seq=96 if dtype == "fp32" else 128, overrides=["max_steps=4", "eval_steps=2", "data.train.dataset.fixed_len=false", *extra])
    t.data_train.label_first = label_first
    seen, real = [], t.model.fused_loss
    t.model.fused_loss = lambda *a, real=real, seen=seen, **k: (seen.append((torch.is_grad_enabled(), k.get("z_loss_coeff", 0.0))), real(*a, **k))[1]
    t.train()
    again = t._evaluate()                                   # the weights of the last step, no coefficient anywhere near
    out = dict(rec=[{k: r[k] for k in r if k not in TIMING} for r in t.wandb_logger.records], losses=list(t._loss_log), dev_again=again,
               w={k: v.detach().float().clone() for k, v in t.model.state_dict().items()}, seen=list(seen), z=t.z_loss_coeff)
    t.cleanup()
    return out


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_trainer_logs_the_two_parts_and_keeps_the_dev_loss_plain(tmp_path, dtype):
    moving = ["lr_scheduler.num_warmup_steps=0", "optimizer.lr=2e-3"]   # (with a warm-up the first step has lr 0 and moves no weight)
    on = _run(tmp_path, "on", dtype, ["z_loss_coeff=1e-2", *moving])
    off = _run(tmp_path, "off", dtype, ["z_loss_coeff=0.0", *moving])
    waiting = _run(tmp_path, "waiting", dtype, ["z_loss_coeff=1e-2", "lagged_readback=false", *moving])
    assert on["z"] == 1e-2 and off["z"] == 0.0
    assert [r["step"] for r in on["rec"]] == [1, 2, 3, 4] == [r["step"] for r in off["rec"]]
    print([(r["loss"], r["z_loss"]) for r in on["rec"]], [r["loss"] for r in off["rec"]])
    assert all(r["z_loss"] > 0 for r in on["rec"])
    assert on["rec"][0]["loss"] == off["rec"][0]["loss"]              # the same weights: the cross-entropy part does not move, bit for bit
    assert all(a["loss"] != b["loss"] for a, b in zip(on["rec"][1:], off["rec"][1:]))   # from step 2 on the runs have different weights
    assert on["losses"] == [r["loss"] for r in on["rec"]]
    # coefficient 0: the record of before, key for key
    assert all("z_loss" not in r for r in off["rec"]) and all(set(a) - set(b) == {"z_loss"} and set(b) <= set(a) for a, b in zip(on["rec"], off["rec"]))
    # the dev loss is the plain cross-entropy: no forward without grad ever got the coefficient, every training forward did
    assert all(z == 1e-2 for grad, z in on["seen"] if grad) and all(z == 0.0 for grad, z in on["seen"] if not grad)
    assert any(grad for grad, _ in on["seen"]) and any(not grad for grad, _ in on["seen"])
    assert "dev_loss" in on["rec"][1] and "dev_loss" in on["rec"][3] and "dev_loss" not in on["rec"][0]
    assert on["rec"][3]["dev_loss"] == on["dev_again"]
    # the boundary that does not wait for the device logs what the waiting one logs
    assert on["rec"] == waiting["rec"] and all(torch.equal(on["w"][k], waiting["w"][k]) for k in on["w"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_a_window_run_as_one_batch_is_the_micro_batch_loop_with_a_z_loss(tmp_path, dtype):
    """The bounds of ``tests/test_trainer_gpu.py::test_a_window_run_as_one_batch_is_the_micro_batch_loop`` (losses 2e-6 / 3e-3 relative, weights
    2e-3 / 6e-2 absolute), on its CPT rows (the case where the joined window needs per-row weights): the z part takes the weights and the
    divisor of the cross-entropy part."""
    extra = ["z_loss_coeff=1e-2", "gradient_accumulation_steps=3", "data.train.dataset.n_samples=36", "eval_steps=1000"]
    a = _run(tmp_path, "joined", dtype, extra, config_name="cpt", label_first=True)
    b = _run(tmp_path, "loop", dtype, [*extra, "fuse_accumulation_window=false"], config_name="cpt", label_first=True)
    assert len([1 for grad, _ in a["seen"] if grad]) == 4 and len([1 for grad, _ in b["seen"] if grad]) == 12
    tol = 2e-6 if dtype == "fp32" else 3e-3
    for key in ("loss", "z_loss"):
        xs, ys = [r[key] for r in a["rec"]], [r[key] for r in b["rec"]]
        print(key, xs, ys)
        assert len(set(xs)) == 4 and all(abs(x - y) <= tol * abs(y) for x, y in zip(xs, ys)), (key, xs, ys)
    worst = max(float((a["w"][k] - b["w"][k]).abs().max()) for k in a["w"])
    assert worst <= (2e-3 if dtype == "fp32" else 6e-2), worst
