"""GPU: label smoothing from the model up — ``HipLlamaDecoder.fused_loss(label_smoothing=)``, ``compute_loss(label_smoothing=)`` on both routes,
and the trainer's ``label_smoothing`` (``loss`` stays the plain cross-entropy part, ``smooth_loss`` joins the record, ``dev_loss`` never sees the
coefficient).

The small models and batches are those of ``tests/test_ce_z_model_gpu.py``, and so are the bounds of the route agreement (taken there from
``tests/test_model_gpu.py``): fp32 loss 1e-5 relative, gradients rtol 5e-3, atol 1e-6; bf16 loss 1e-2 relative, gradients 5e-2 of the norm,
applied to the norm of the difference per parameter."""
import pytest
import torch

from test_ce_metrics_gpu import _model
from test_ce_z_model_gpu import TIMING, Z, _batch, _Literal, _loss_and_grads, _shifted

pytestmark = pytest.mark.gpu

DEV = "cuda"
E = 0.1


def _assert_grads_close(g_fused, g_ref, dtype):
    worst = 0.0
    for k in g_ref:
        if dtype == torch.float32:
            torch.testing.assert_close(g_fused[k], g_ref[k], rtol=5e-3, atol=1e-6, msg=lambda m, k=k: f"{k}: {m}")
        else:
            rel = float((g_fused[k] - g_ref[k]).norm()) / (float(g_ref[k].norm()) + 1e-30)
            worst = max(worst, rel)
            assert float((g_fused[k] - g_ref[k]).norm()) <= 5e-2 * float(g_ref[k].norm()) + 1e-6, (k, rel)
    print(f"worst relative gradient difference (bf16 only) {worst:.3e}")


@pytest.mark.parametrize("z", [0.0, Z])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_route_agrees_with_the_literal_route(dtype, packed, z):
    from ssi.loss import CEWithChunkedOutputLoss
    model = _model(dtype)
    model.train()
    batch = _batch(packed, dtype)
    names = ("last_ce_loss", "last_smooth_loss") + (("last_z_loss",) if z else ())
    fused, g_fused = _loss_and_grads(model, batch, CEWithChunkedOutputLoss(), label_smoothing=E, z_loss_coeff=z)
    parts_fused = [float(getattr(model, n)) for n in names]
    literal, g_lit = _loss_and_grads(model, batch, _Literal(), label_smoothing=E, z_loss_coeff=z)
    parts_lit = [float(getattr(model, n)) for n in names]
    plain, g_plain = _loss_and_grads(model, batch, CEWithChunkedOutputLoss(), z_loss_coeff=z)
    loss_tol = 1e-5 if dtype == torch.float32 else 1e-2
    print(f"fused {float(fused):.7f} = {parts_fused}, literal {float(literal):.7f} = {parts_lit}, without smoothing {float(plain):.7f}")
    assert parts_fused[1] > 0.05 * parts_fused[0] > 0           # the uniform part is no rounding error of the total
    assert abs(float(fused) - float(literal)) <= loss_tol * abs(float(literal))
    for a, b in zip(parts_fused, parts_lit):
        assert abs(a - b) <= loss_tol * abs(b)
    _assert_grads_close(g_fused, g_lit, dtype)
    # ... and the smoothing is in the gradient: e (onehot - 1 / V) per row against (p - onehot), about e of it
    moved = float((g_fused["tok_embeddings.weight"] - g_plain["tok_embeddings.weight"]).norm()) / float(g_plain["tok_embeddings.weight"].norm())
    assert moved > 0.02, moved


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_with_loss_weights_against_torch_on_the_literal_logits(dtype, packed):
    """The literal route of ``compute_loss`` takes no ``loss_weights``; the same expression over ``model(...)``'s logits, in plain torch:
    ``sum_i w_i ((1 - e) nll_i + e u_i + z lse_i^2) / n_valid``."""
    from ssi.loss import CEWithChunkedOutputLoss
    model = _model(dtype)
    model.train()
    batch = _batch(packed, dtype)
    w = 3.0 * torch.rand(batch["tokens"].shape, generator=torch.Generator().manual_seed(5))
    w[0, 30], w[1, 40] = 0.0, 1.0
    w = w.to(DEV)
    fused, g_fused = _loss_and_grads(model, {**batch, "loss_weights": w}, CEWithChunkedOutputLoss(), label_smoothing=E, z_loss_coeff=Z)
    model.zero_grad()
    logits = model(tokens=batch["tokens"], input_pos=batch.get("input_pos"))
    x = (torch.cat(logits, dim=1) if isinstance(logits, list) else logits).float()
    y = _shifted(batch)
    valid = y != -100
    lse = torch.logsumexp(x, dim=-1)
    nll = lse - x.gather(-1, torch.where(valid, y, torch.zeros_like(y))[..., None])[..., 0]
    u = lse - x.mean(dim=-1)
    want = (w * valid * ((1.0 - E) * nll + E * u + Z * lse * lse)).sum() / valid.sum()
    want.backward()
    want = want.detach()
    g_ref = {k: p.grad.detach().float().clone() for k, p in model.named_parameters()}
    loss_tol = 1e-5 if dtype == torch.float32 else 1e-2
    print(f"fused {float(fused):.7f}, torch on the literal logits {float(want):.7f}")
    assert abs(float(fused) - float(want)) <= loss_tol * abs(float(want))
    _assert_grads_close(g_fused, g_ref, dtype)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_the_default_path_is_untouched_and_the_scalars_are_the_parts(dtype, packed, monkeypatch):
    from ssi import ops
    from ssi.eval import LabelMetrics, SeqScores
    from ssi.loss import CEWithChunkedOutputLoss
    model = _model(dtype)
    model.train()
    batch = _batch(packed, dtype)
    calls = []
    real = ops.ce_fwd_smooth
    monkeypatch.setattr(ops, "ce_fwd_smooth", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    without, g_without = _loss_and_grads(model, batch, CEWithChunkedOutputLoss())
    zero, g_zero = _loss_and_grads(model, batch, CEWithChunkedOutputLoss(), label_smoothing=0.0)
    assert torch.equal(without, zero) and all(torch.equal(g_without[k], g_zero[k]) for k in g_zero)
    with torch.no_grad():
        plain_eval = model.fused_loss(batch["tokens"], _shifted(batch), input_pos=batch.get("input_pos"), label_smoothing=0.0)
    assert not calls and not [n for n in model._arena.buf if n.startswith("row_u")], "e = 0 issued a smoothing launch or allocated a row_u buffer"
    assert model.last_ce_loss is None and model.last_smooth_loss is None and model.last_z_loss is None
    # e > 0 under grad: the total, and the parts left on the model
    total, _ = _loss_and_grads(model, batch, CEWithChunkedOutputLoss(), label_smoothing=E)
    assert len(calls) == 1 and "row_u" in model._arena.buf and not [n for n in model._arena.buf if n.startswith("row_z")]
    assert torch.equal(model.last_ce_loss, without), "last_ce_loss is not the loss of a forward without the option on the same weights"
    assert torch.equal(total, model.last_ce_loss * (1.0 - E) + model.last_smooth_loss) and float(model.last_smooth_loss) > 0
    # ... with a z-loss as well
    total_z, _ = _loss_and_grads(model, batch, CEWithChunkedOutputLoss(), label_smoothing=E, z_loss_coeff=Z)
    assert len(calls) == 2 and torch.equal(model.last_ce_loss, without) and float(model.last_z_loss) > 0
    assert torch.equal(total_z, model.last_ce_loss * (1.0 - E) + model.last_smooth_loss + model.last_z_loss)
    # ... and without grad
    with torch.no_grad():
        total_eval = model.fused_loss(batch["tokens"], _shifted(batch), input_pos=batch.get("input_pos"), label_smoothing=E)
        assert len(calls) == 3 and "row_u.x" in model._arena.buf
        assert torch.equal(model.last_ce_loss, plain_eval)
        assert torch.equal(total_eval, model.last_ce_loss * (1.0 - E) + model.last_smooth_loss)
        with pytest.raises(ValueError, match="label_metrics"):
            model.fused_loss(batch["tokens"], _shifted(batch), input_pos=batch.get("input_pos"), label_smoothing=E,
                             label_metrics=LabelMetrics({"a": (0, 99)}, 5, torch.device(DEV)))
        with pytest.raises(ValueError, match="seq_scores"):
            model.fused_loss(batch["tokens"], _shifted(batch), input_pos=batch.get("input_pos"), label_smoothing=E,
                             seq_scores=SeqScores([(0, 0, 8)], 5, torch.zeros(1, 4, dtype=torch.float64, device=DEV)))
    for bad in (-1e-3, 1.0, float("nan")):
        with pytest.raises(ValueError, match="label_smoothing"):
            model.fused_loss(batch["tokens"], _shifted(batch), label_smoothing=bad)


# ---- trainer --------------------------------------------------------------------------------------------------------------------------------
def _run(tmp_path, name, dtype, extra=(), drop_key=False, monkeypatch=None):
    import ssi.config
    from test_trainer_gpu import MFMA_SMALL, SMALL, _trainer
    if drop_key:  # a config from before the key existed: composed as usual, then the key taken out before the trainer sees it
        real_compose = ssi.config.compose

        def compose(*a, **k):
            cfg = real_compose(*a, **k)
            del cfg.label_smoothing
            return cfg
        monkeypatch.setattr(ssi.config, "compose", compose)
    t = _trainer(tmp_path, name, dtype=dtype, model=SMALL if dtype == "fp32" else MFMA_SMALL, seq=96 if dtype == "fp32" else 128,
                 overrides=["max_steps=4", "eval_steps=2", "data.train.dataset.fixed_len=false", *extra])
    if drop_key:
        monkeypatch.undo()
        assert "label_smoothing" not in t.cfg
    seen, real = [], t.model.fused_loss
    t.model.fused_loss = lambda *a, real=real, seen=seen, **k: (seen.append((torch.is_grad_enabled(), k.get("label_smoothing", 0.0))), real(*a, **k))[1]
    t.train()
    again = t._evaluate()                                   # the weights of the last step, no coefficient anywhere near
    out = dict(rec=[{k: r[k] for k in r if k not in TIMING} for r in t.wandb_logger.records], losses=list(t._loss_log), dev_again=again,
               w={k: v.detach().float().clone() for k, v in t.model.state_dict().items()}, seen=list(seen), e=t.label_smoothing)
    t.cleanup()
    return out


MOVING = ["lr_scheduler.num_warmup_steps=0", "optimizer.lr=2e-3"]   # (with a warm-up the first step has lr 0 and moves no weight)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_trainer_logs_the_parts_and_keeps_the_dev_loss_plain(tmp_path, dtype):
    on = _run(tmp_path, "on", dtype, ["label_smoothing=0.1", *MOVING])
    off = _run(tmp_path, "off", dtype, ["label_smoothing=0.0", *MOVING])
    assert on["e"] == 0.1 and off["e"] == 0.0
    assert [r["step"] for r in on["rec"]] == [1, 2, 3, 4] == [r["step"] for r in off["rec"]]
    print([(r["loss"], r["smooth_loss"]) for r in on["rec"]], [r["loss"] for r in off["rec"]])
    assert all(r["smooth_loss"] > 0 for r in on["rec"])
    assert on["rec"][0]["loss"] == off["rec"][0]["loss"]              # the same weights: the cross-entropy part does not move, bit for bit
    assert all(a["loss"] != b["loss"] for a, b in zip(on["rec"][1:], off["rec"][1:]))   # from step 2 on the runs have different weights
    assert on["losses"] == [r["loss"] for r in on["rec"]]
    # the record gains smooth_loss and no other key; coefficient 0: the record of before, key for key
    assert all("smooth_loss" not in r for r in off["rec"])
    assert all(set(a) - set(b) == {"smooth_loss"} and set(b) <= set(a) for a, b in zip(on["rec"], off["rec"]))
    # the dev loss is the plain cross-entropy: no forward without grad ever got the coefficient, every training forward did
    assert all(e == 0.1 for grad, e in on["seen"] if grad) and all(e == 0.0 for grad, e in on["seen"] if not grad)
    assert any(grad for grad, _ in on["seen"]) and any(not grad for grad, _ in on["seen"])
    assert "dev_loss" in on["rec"][1] and "dev_loss" in on["rec"][3] and "dev_loss" not in on["rec"][0]
    assert on["rec"][3]["dev_loss"] == on["dev_again"]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_dev_loss_of_a_fixed_model_does_not_see_the_key(tmp_path, dtype):
    """With the default warm-up the first optimizer step has lr 0 and moves no weight: the dev loss after it is that of the initial model, with
    the key and without it."""
    first = ["eval_steps=1", "save_steps=1000", "max_steps=1"]
    on = _run(tmp_path, "on", dtype, ["label_smoothing=0.1", *first])
    off = _run(tmp_path, "off", dtype, ["label_smoothing=0.0", *first])
    assert all(torch.equal(on["w"][k], off["w"][k]) for k in on["w"]), "the first step moved a weight: the models are not the same"
    assert on["rec"][0]["dev_loss"] == off["rec"][0]["dev_loss"] == on["dev_again"] == off["dev_again"]
    assert on["rec"][0]["loss"] == off["rec"][0]["loss"] and on["rec"][0]["smooth_loss"] > 0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_the_key_at_zero_is_a_run_without_the_key(tmp_path, dtype, monkeypatch):
    zero = _run(tmp_path, "zero", dtype, ["label_smoothing=0.0", *MOVING])
    absent = _run(tmp_path, "absent", dtype, MOVING, drop_key=True, monkeypatch=monkeypatch)
    assert zero["e"] == 0.0 and absent["e"] == 0.0
    assert zero["rec"] == absent["rec"] and all("smooth_loss" not in r for r in zero["rec"])
    assert all(torch.equal(zero["w"][k], absent["w"][k]) for k in zero["w"])
    assert all(e == 0.0 for _, e in zero["seen"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_both_options_on_and_the_boundary_that_does_not_wait(tmp_path, dtype):
    both = ["label_smoothing=0.1", "z_loss_coeff=1e-2", *MOVING]
    lagged = _run(tmp_path, "lagged", dtype, [*both, "lagged_readback=true"])
    waiting = _run(tmp_path, "waiting", dtype, [*both, "lagged_readback=false"])
    print([(r["loss"], r["smooth_loss"], r["z_loss"]) for r in lagged["rec"]])
    assert all(r["smooth_loss"] > 0 and r["z_loss"] > 0 and r["smooth_loss"] != r["z_loss"] for r in lagged["rec"])
    assert lagged["rec"] == waiting["rec"] and all(torch.equal(lagged["w"][k], waiting["w"][k]) for k in lagged["w"])
    # the two sums do not trade places: smooth_loss is that of a run with the smoothing alone at the first step (the same weights)
    alone = _run(tmp_path, "alone", dtype, ["label_smoothing=0.1", "max_steps=1", *MOVING])
    assert alone["rec"][0]["smooth_loss"] == lagged["rec"][0]["smooth_loss"] and alone["rec"][0]["loss"] == lagged["rec"][0]["loss"]
