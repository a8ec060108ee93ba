"""GPU: the parameter average (``ema_decay``) through ``HipAdamW`` and the trainer, on a small decoder (2 layers, dim 128, vocabulary 368,
rows of 128 tokens).

The optimizer tests feed seeded gradients straight into the flat gradient buffer (the backward is not under test): after every step the
parameters are read back and the reference formula of ``tests/test_ema_gpu.py`` is applied on the CPU with ``ema_decay_at(step)``, a chain of
its own from the initial weights; the acceptance per tensor is that file's (within 1 fp32 ulp, at most ``max(1, n // 10**5)`` elements not
bit-equal).  Everything else here is exact: parameters and moments do not notice the average, the under-backward path leaves the same
average as the plain step, a frozen element's average never moves, ``ema_weights()`` puts the parameters back bit for bit, and a resumed run
carries the same average as an uninterrupted one."""
import logging
import math
import os

import pytest
import torch

from test_ema_gpu import _check, _reference
from test_param_groups_model_gpu import BF16_TYPES, STAGE1, _bits, _model, _segments, _trainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = dict(vocab_size=368, num_layers=2, num_heads=2, num_kv_heads=1, embed_dim=128, max_seq_len=128, intermediate_dim=256)
SMALL_TRAINER = {"num_layers": 2, "num_heads": 2, "num_kv_heads": 1, "embed_dim": 128, "intermediate_dim": 256, "max_seq_len": 512,
                 "_base_vocab_size_txt": 300, "_n_special_txt": 16}
HYPER = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
TIMING = ("duration_step", "tokens_per_second_per_gpu", "train_clock_time")


def _grads(model, gen, dtype):
    return (torch.randn(model._flat.numel(), generator=gen) * 30.0).to(dtype).to(DEV)


def _one_step(model, opt, G, under_backward=False, scale_value=1 / 37):
    from ssi.optimizer import scale_grads
    model._flat_grad.copy_(G)
    model.attach_grads()
    if under_backward:   # what the window's last backward does: every bucket announced once, in its order
        assert opt.overlap_with_backward(torch.full((1,), float(torch.tensor(scale_value)), dtype=torch.float32, device=DEV))
        listener = model.bucket_listener
        for bucket in model.buckets:
            listener(*bucket)
    else:
        scale_grads(model, torch.tensor(scale_value))
    opt.step()
    opt.zero_grad(set_to_none=True)


def _follow(model, opt, chain, step, decay, warmup=True):
    """One link of the manual loop: the parameters as they are now into ``chain`` (fp32 tensors on the CPU by state-dict name) with the
    reference formula, then the optimizer's average against it, tensor by tensor."""
    from ssi.optimizer import ema_decay_at
    d = ema_decay_at(step, decay, warmup)
    got = opt.ema_state_dict()
    assert list(got) == [k for k, _ in model.named_parameters()]
    for k, p in model.named_parameters():
        chain[k] = _reference(p.detach().cpu().reshape(-1), chain[k].reshape(-1), d).view(p.shape)
        assert got[k].dtype == torch.float32 and got[k].shape == p.shape
        _check(got[k].cpu().reshape(-1), chain[k].reshape(-1), p.numel(), (k, step))


@pytest.mark.parametrize("dtype,steps", [(torch.bfloat16, 5), (torch.float32, 2)], ids=["bf16", "fp32"])
def test_optimizer_follows_a_manual_loop_and_leaves_adamw_alone(dtype, steps):
    from ssi.optimizer import HipAdamW
    with_avg, without = _model(SMALL, dtype), _model(SMALL, dtype)
    opt = HipAdamW(with_avg.parameters(), model=with_avg, ema_decay=0.9, **HYPER)
    plain = HipAdamW(without.parameters(), model=without, **HYPER)
    assert plain._ema is None and opt._ema.dtype == torch.float32 and opt._ema.numel() == with_avg._flat.numel()
    assert opt._ema.data_ptr() != with_avg._flat.data_ptr() and torch.equal(opt._ema, with_avg._flat.float())
    chain = {k: p.detach().float().cpu() for k, p in with_avg.named_parameters()}
    gen = torch.Generator().manual_seed(5)
    for step in range(1, steps + 1):
        G = _grads(with_avg, gen, dtype)
        _one_step(with_avg, opt, G)
        _one_step(without, plain, G)
        torch.cuda.synchronize()
        _follow(with_avg, opt, chain, step, 0.9)
        for name, x, y in (("param", with_avg._flat, without._flat), ("exp_avg", opt._exp_avg, plain._exp_avg), ("exp_avg_sq", opt._exp_avg_sq, plain._exp_avg_sq)):
            assert torch.equal(_bits(x), _bits(y)), (name, step)
    assert not torch.equal(opt._ema, with_avg._flat.float())
    # the optimizer state is the one it was: an average is the run's configuration, and a state saved either way loads either way
    assert list(opt.state_dict()["state"][0]) == list(plain.state_dict()["state"][0]) and list(opt.state_dict()["param_groups"][0]) == list(plain.state_dict()["param_groups"][0])
    plain.load_state_dict(opt.state_dict())
    opt.load_state_dict(plain.state_dict())
    assert opt._step_count == steps and torch.equal(opt._ema, with_avg._flat.float())      # after load_state_dict: what the model holds
    saved = {k: v + 1 for k, v in opt.ema_state_dict().items()}
    opt.load_ema_state_dict(saved)
    assert all(torch.equal(v, saved[k]) for k, v in opt.ema_state_dict().items())
    with pytest.raises(RuntimeError, match="missing keys"):
        opt.load_ema_state_dict({k: v for k, v in saved.items() if k != "norm.scale"})
    with pytest.raises(RuntimeError, match="size mismatch"):
        opt.load_ema_state_dict({**saved, "norm.scale": saved["norm.scale"][:-1]})
    for bad in (1.0, -0.1, float("nan"), True, "0.9"):
        with pytest.raises(ValueError, match="ema_decay"):
            HipAdamW(without.parameters(), model=without, ema_decay=bad, **HYPER)


def test_under_the_backward_the_average_is_the_plain_steps():
    from ssi.optimizer import HipAdamW
    a, b = _model(SMALL, torch.bfloat16), _model(SMALL, torch.bfloat16)
    armed, plain = HipAdamW(a.parameters(), model=a, ema_decay=0.9, **HYPER), HipAdamW(b.parameters(), model=b, ema_decay=0.9, **HYPER)
    gen = torch.Generator().manual_seed(6)
    for step in (1, 2):
        G = _grads(a, gen, torch.bfloat16)
        _one_step(a, armed, G, under_backward=True)
        _one_step(b, plain, G)
        torch.cuda.synchronize()
        assert torch.equal(armed._ema, plain._ema) and torch.equal(_bits(a._flat), _bits(b._flat)), step
        assert not torch.equal(armed._ema, a._flat.float())
    # a window without a label: the factor 1 / 0 is not finite, the launches under the backward change nothing, the caller cancels
    before_ema, before_p = armed._ema.clone(), a._flat.clone()
    a._flat_grad.copy_(_grads(a, gen, torch.bfloat16))
    a.attach_grads()
    assert armed.overlap_with_backward(1.0 / torch.zeros(1, dtype=torch.float32, device=DEV))
    listener = a.bucket_listener
    for bucket in a.buckets:
        listener(*bucket)
    with pytest.raises(RuntimeError, match="armed"):
        with armed.ema_weights():
            pass
    armed.cancel_overlap()
    armed.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    assert torch.equal(armed._ema, before_ema) and torch.equal(_bits(a._flat), _bits(before_p)) and armed._step_count == 2


@pytest.mark.parametrize("under_backward", [False, True], ids=["step", "under-backward"])
def test_stage_one_rules_freeze_the_average_too(under_backward):
    from ssi.optimizer import HipAdamW, ema_decay_at
    from ssi.param_groups import trainable_ranges
    model = _model(SMALL, torch.bfloat16)
    segs = _segments(model, STAGE1, BF16_TYPES)
    ranges = trainable_ranges(segs)
    assert any(s.frozen for s in segs) and ranges and sum(hi - lo for lo, hi in ranges) < model._flat.numel() // 4
    opt = HipAdamW(model.parameters(), model=model, param_segments=segs, ema_decay=0.9, **HYPER)
    init = opt._ema.clone()
    chain = init.cpu()
    gen = torch.Generator().manual_seed(8)
    for step in (1, 2, 3):
        G = _grads(model, gen, torch.bfloat16)
        for s in segs:
            if s.frozen:
                G[s.start:s.end] = float("nan")                                          # frozen gradient memory is unspecified
        _one_step(model, opt, G, under_backward=under_backward)
        torch.cuda.synchronize()
        flat = model._flat.cpu()
        for lo, hi in ranges:
            chain[lo:hi] = _reference(flat[lo:hi], chain[lo:hi], ema_decay_at(step, 0.9))
            _check(opt._ema[lo:hi].cpu(), chain[lo:hi], hi - lo, (lo, hi, step))
            assert not torch.equal(opt._ema[lo:hi], init[lo:hi])
        for s in segs:
            if s.frozen:
                assert torch.equal(opt._ema[s.start:s.end], init[s.start:s.end]), (s.start, s.end, step)
    assert bool(torch.isfinite(opt._ema).all())


def test_ema_weights_swaps_in_the_rounded_average_and_puts_the_parameters_back():
    from ssi.optimizer import HipAdamW
    model = _model(SMALL, torch.bfloat16)
    opt = HipAdamW(model.parameters(), model=model, ema_decay=0.9, ema_warmup=False, **HYPER)
    gen = torch.Generator().manual_seed(9)
    for _ in range(2):
        _one_step(model, opt, _grads(model, gen, torch.bfloat16), under_backward=True)
    before, avg = model._flat.clone(), opt._ema.clone()
    ptr = model._flat.data_ptr()
    with opt.ema_weights():
        assert model._flat.data_ptr() == ptr                                             # the parameters' views stay valid
        assert torch.equal(_bits(model._flat), _bits(avg.to(torch.bfloat16))) and not torch.equal(_bits(model._flat), _bits(before))
        assert torch.equal(_bits(model.norm.scale.detach()), _bits(opt.ema_state_dict()["norm.scale"].to(torch.bfloat16)))
        with pytest.raises(RuntimeError, match="nest"):
            with opt.ema_weights():
                pass
        assert torch.equal(_bits(model._flat), _bits(avg.to(torch.bfloat16)))           # the refused entry changed nothing
    assert torch.equal(_bits(model._flat), _bits(before)) and torch.equal(opt._ema, avg) and opt._ema_stash is None
    with pytest.raises(KeyError, match="boom"):
        with opt.ema_weights():
            raise KeyError("boom")
    assert torch.equal(_bits(model._flat), _bits(before)) and opt._ema_stash is None
    with opt.ema_weights():                                                              # usable again
        pass
    plain = HipAdamW(model.parameters(), model=model, **HYPER)
    with pytest.raises(RuntimeError, match="ema_decay"):
        with plain.ema_weights():
            pass


def _run(tmp_path, name, overrides):
    t = _trainer(tmp_path, name, None, overrides=["eval_steps=2", "save_steps=4", *overrides], model=SMALL_TRAINER)
    return t


def test_trainer_logs_saves_and_resumes_the_average(tmp_path, caplog):
    from ssi.checkpoint import EMA_STATE_FILENAME, make_checkpointer
    off = _run(tmp_path, "off", ["max_steps=6"])
    assert off.optimizer._ema is None
    off.train()
    rec_off = list(off.wandb_logger.records)
    off.cleanup()
    assert not os.path.exists(tmp_path / "off" / "checkpoints" / EMA_STATE_FILENAME) and not os.path.exists(tmp_path / "off" / "checkpoints" / "step_4" / "ema")
    del off

    on = _run(tmp_path, "on", ["max_steps=6", "ema_decay=0.9"])
    at_save = {}
    real = on.checkpointer.save_ema_checkpoint
    on.checkpointer.save_ema_checkpoint = lambda sd, ema, step: (at_save.update({step: on.optimizer._ema.clone()}), real(sd, ema, step))[1]
    on.train()
    torch.cuda.synchronize()
    rec_on = list(on.wandb_logger.records)
    assert [r["step"] for r in rec_on] == [r["step"] for r in rec_off] == [1, 2, 3, 4, 5, 6]
    for a, b in zip(rec_on, rec_off):
        assert ("dev_loss_ema" in a) == (a["step"] in (2, 4, 6)) and ("dev_loss" in a) == (a["step"] in (2, 4, 6))
        assert {k: v for k, v in a.items() if k not in TIMING and k != "dev_loss_ema"} == {k: v for k, v in b.items() if k not in TIMING}, a["step"]
    assert all(r["dev_loss_ema"] != r["dev_loss"] and math.isfinite(r["dev_loss_ema"]) for r in rec_on if "dev_loss" in r)
    final_ema = on.optimizer.ema_state_dict()
    final_weights = {k: v.detach().clone() for k, v in on.model.state_dict().items()}
    ckpt = tmp_path / "on" / "checkpoints"
    assert list(at_save) == [4] and os.path.isfile(ckpt / "step_4" / "ema" / "model.safetensors") and os.path.isfile(ckpt / EMA_STATE_FILENAME)
    loaded = make_checkpointer(checkpoint_dir=str(ckpt / "step_4" / "ema"), output_dir=str(tmp_path / "scratch")).load_checkpoint()["model"]
    plain_ckpt = make_checkpointer(checkpoint_dir=str(ckpt / "step_4"), output_dir=str(tmp_path / "scratch")).load_checkpoint()["model"]
    names = {id(p): k for k, p in on.model.named_parameters()}
    for p, name, rows in on.model._param_src:
        k = names[id(p)]
        want = on.model._view(name, rows, at_save[4]).to(torch.bfloat16).cpu()
        assert loaded[k].dtype == torch.bfloat16 and torch.equal(_bits(loaded[k]), _bits(want)), k
    assert sorted(loaded) == sorted(plain_ckpt) and any(not torch.equal(loaded[k], plain_ckpt[k]) for k in loaded)
    dev6 = rec_on[-1]["dev_loss_ema"]
    on.cleanup()
    del on

    resume = [f"checkpointer.checkpoint_dir={ckpt}/step_4", "checkpointer.allow_random_init=false",
              f"checkpointer.training_state_checkpoint={ckpt}/training_state.pt"]
    again = _run(tmp_path, "again", ["max_steps=6", "ema_decay=0.9", *resume])
    assert again.global_step == 4 and torch.equal(again.optimizer._ema, at_save[4])
    again.train()
    torch.cuda.synchronize()
    got = again.optimizer.ema_state_dict()
    assert all(torch.equal(got[k], final_ema[k]) for k in final_ema)
    assert all(torch.equal(v, final_weights[k]) for k, v in again.model.state_dict().items())
    assert [r["step"] for r in again.wandb_logger.records] == [5, 6] and again.wandb_logger.records[-1]["dev_loss_ema"] == dev6
    again.cleanup()
    del again

    os.remove(ckpt / EMA_STATE_FILENAME)
    with caplog.at_level(logging.WARNING, logger="ssi.trainer"):
        fresh = _run(tmp_path, "fresh", ["max_steps=6", "ema_decay=0.9", *resume])
    assert any("starts from the loaded weights" in r.getMessage() and EMA_STATE_FILENAME in r.getMessage() for r in caplog.records)
    assert torch.equal(fresh.optimizer._ema, fresh.model._flat.float()) and not torch.equal(fresh.optimizer._ema, at_save[4])
    fresh.cleanup()
