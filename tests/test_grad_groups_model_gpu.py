"""GPU: gradient groups (``grad_groups``: per-group gradient norms and clipping on the flat buffer) through the optimizer and the trainer, on the
small MFMA geometry and the tiny fp32 model of ``tests/test_param_groups_model_gpu.py``.

The bound of the logged norms is ``ssi_sumsq_groups``' own (``tests/test_sumsq_groups_gpu.py``: ``B = D u / (1 - D u)`` on the sum of squares, half
of it on the root, plus two fp32 roundings for the root and the product with the scale)."""
import math
import os

import pytest
import torch

import grad_groups_ref as ref
from test_param_groups_model_gpu import BF16_TYPES, EMB, F32_MODEL, F32_TYPES, HYPER, STAGE1, _bits, _model, _segments
from test_sumsq_groups_gpu import bound
from test_trainer_gpu import MFMA_SMALL, _Remap

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
GROUPS = [{"name": "new_rows", "params": [EMB], "token_types": ["dsu", "modality"]}, {"name": "embedding", "params": [EMB]},
          {"name": "norms", "params": ["*.scale"]}, {"name": "attn", "params": ["*.attn.*"]}]
U = 2.0 ** -24


def _groups(model, node, types, segments=None):
    from ssi.grad_groups import GradGroups
    from ssi.param_groups import model_layout
    layout, total = model_layout(model)
    return GradGroups.from_config(node, layout, total, types, segments, device=DEV)


def _group_ranges(gg):
    out, start = [[] for _ in gg.names], 0
    for e, g in zip(gg.seg_end, gg.seg_group):
        if g >= 0:
            out[g].append((start, e))
        start = e
    return out


def _norm64(G, ranges, scale):
    return [math.sqrt(sum(float(G[a:b].double().square().sum()) for a, b in r)) * abs(scale) for r in ranges]


def _norm_bound(model, gg):
    return 0.5 * bound(model._flat.numel(), model._flat.dtype, len(gg.seg_end)) * 1.01 + 2 * U


def _fill_grads(model, gen, std=30.0):
    G = (torch.randn(model._flat.numel(), generator=gen) * std).to(model._flat.dtype).to(DEV)
    model._flat_grad.copy_(G)
    model.attach_grads()
    return G


def _window(model, opt, scale, max_norm=None):
    """What ``Trainer._apply_window`` does with the optimizer."""
    from ssi.optimizer import clip_grad_norm_from_group_sums, scale_grads
    scale_grads(model, torch.tensor(scale))
    sums = opt.measure_grad_group_sums().clone()
    total = clip_grad_norm_from_group_sums(model, max_norm, sums) if max_norm is not None else None
    pending = model.pending_grad_scale.clone()
    values = {k: v.clone() for k, v in opt.apply_grad_groups().items()}
    opt.step()
    opt.zero_grad(set_to_none=True)
    return sums, pending, values, total


def _oracle_step(ops, P, G, M, V, refined, coef, pending, step):
    """Per refined segment the plain kernel with the product of the pending scale and the group's coefficient (a skipped group: left alone)."""
    for s, g in refined:
        if s.frozen:
            continue
        gs = pending * coef[g:g + 1]
        if not bool(torch.isfinite(gs)):
            continue
        sl = slice(s.start, s.end)
        ops.adamw_step(P[sl], G[sl], M[sl], V[sl], lr=HYPER["lr"] * s.lr_scale, beta1=0.9, beta2=0.999, eps=1e-8,
                       weight_decay=HYPER["weight_decay"] if s.weight_decay is None else s.weight_decay, step=step, grad_scale_dev=gs.clone(),
                       elem_offset=s.start)


def _same_state(model, opt, P, M, V):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in ((model._flat, P), (opt._exp_avg, M), (opt._exp_avg_sq, V)))


# ---- the optimizer alone, tiny fp32 model -----------------------------------------------------------------------------------------------------
def test_b_a_threshold_that_never_binds_changes_no_bit():
    from ssi.optimizer import HipAdamW, scale_grads
    plain, ruled = _model(F32_MODEL, F32), _model(F32_MODEL, F32)
    gg = _groups(ruled, {"groups": GROUPS, "clip": {"max_norm": 1e9}}, F32_TYPES)
    assert gg.names == ["new_rows", "embedding", "norms", "attn", "other"]
    opt_p = HipAdamW(plain.parameters(), model=plain, **HYPER)
    opt_r = HipAdamW(ruled.parameters(), model=ruled, grad_groups=gg, **HYPER)
    gen = torch.Generator().manual_seed(5)
    for step in (1, 2, 3):
        G = _fill_grads(ruled, gen)
        plain._flat_grad.copy_(G)
        plain.attach_grads()
        scale_grads(plain, torch.tensor(1 / 37))
        opt_p.step()
        opt_p.zero_grad(set_to_none=True)
        _, _, values, _ = _window(ruled, opt_r, 1 / 37)
        assert torch.equal(values["clip"], torch.ones_like(values["clip"])) and not values["skipped"].any()
    torch.cuda.synchronize()
    assert _same_state(ruled, opt_r, plain._flat, opt_p._exp_avg, opt_p._exp_avg_sq)


def test_c_a_threshold_that_binds_on_one_group_equals_per_segment_launches():
    from ssi import ops
    from ssi.optimizer import HipAdamW
    model = _model(F32_MODEL, F32)
    node = {"groups": [dict(GROUPS[0], max_norm=0.5)] + GROUPS[1:], "clip": {"max_norm": 1e9}}
    gg = _groups(model, node, F32_TYPES)
    opt = HipAdamW(model.parameters(), model=model, grad_groups=gg, **HYPER)
    P, M, V = model._flat.clone(), torch.zeros_like(model._flat), torch.zeros_like(model._flat)
    gen = torch.Generator().manual_seed(6)
    for step in (1, 2):
        G = _fill_grads(model, gen)
        sums, pending, values, _ = _window(model, opt, 1 / 37)
        n = sums.sqrt() * pending.abs()
        coef = torch.minimum(torch.ones_like(n), gg.clip.max_norm / (n + 1e-6))          # from the kernel's own sums
        assert torch.equal(coef, values["clip"]) and float(coef[0]) < 1 and torch.equal(coef[1:], torch.ones_like(coef[1:]))
        _oracle_step(ops, P, G, M, V, gg.refined, coef, pending, step)
        torch.cuda.synchronize()
        assert _same_state(model, opt, P, M, V), step
    assert abs(float(n[0]) * float(coef[0]) - 0.5) <= 1e-5                                # the clipped group's norm is its threshold


def test_d_adaptive_six_steps_equal_the_restatement():
    from ssi.optimizer import HipAdamW
    model = _model(F32_MODEL, F32)
    adaptive = {"rel": 1.05, "beta": 0.9, "warmup_steps": 2}
    gg = _groups(model, {"groups": GROUPS, "clip": {"adaptive": adaptive, "max_norm": 40.0}}, F32_TYPES)
    opt = HipAdamW(model.parameters(), model=model, grad_groups=gg, **HYPER)
    gen = torch.Generator().manual_seed(7)
    norms, got = [], []
    for step, std in enumerate((30.0, 25.0, 28.0, 300.0, 27.0, 26.0), start=1):   # a spike after the warm-up
        _fill_grads(model, gen, std)
        if step == 5:
            a, b = _group_ranges(gg)[2][0]
            model._flat_grad[a:b] = float("inf")                                          # one group's norm overflows: skipped, gamma held
        sums, pending, values, _ = _window(model, opt, 1 / 37)
        norms.append((sums.sqrt() * pending.abs()).double().cpu().tolist())
        got.append(torch.stack([values["clip"], values["ema"], values["skipped"]], dim=1).double().cpu().numpy())
    for g, name in enumerate(gg.names):
        want = ref.run([row[g] for row in norms], max_norm=40.0, adaptive=adaptive)
        for t in range(6):
            for k in range(3):
                a, w = got[t][g, k], want[t, k]
                assert (math.isnan(a) and math.isnan(w)) or abs(a - w) <= 1e-6 * abs(w), (name, t, k, a, w)
    assert got[3][0, 0] < 0.2 and got[5][2, 2] == 1 and math.isnan(got[4][2, 0])
    assert bool(model._flat.isfinite().all())


def test_e_a_group_with_an_inf_gradient_keeps_its_bits():
    from ssi.optimizer import HipAdamW
    model = _model(F32_MODEL, F32)
    gg = _groups(model, {"groups": GROUPS, "clip": {"max_norm": 1.0}}, F32_TYPES)
    opt = HipAdamW(model.parameters(), model=model, grad_groups=gg, **HYPER)
    gen = torch.Generator().manual_seed(8)
    _fill_grads(model, gen)
    _window(model, opt, 1 / 37)
    before = [t.clone() for t in (model._flat, opt._exp_avg, opt._exp_avg_sq)]
    _fill_grads(model, gen)
    ranges = _group_ranges(gg)
    a, b = ranges[3][0]
    model._flat_grad[a + 3] = float("inf")                                                # one element of "attn"
    _, _, values, _ = _window(model, opt, 1 / 37)
    torch.cuda.synchronize()
    assert values["skipped"].tolist() == [0, 0, 0, 1, 0] and math.isnan(float(values["clip"][3]))
    for g, rs in enumerate(ranges):
        for lo, hi in rs:
            same = all(torch.equal(_bits(x[lo:hi]), _bits(y[lo:hi])) for x, y in zip((model._flat, opt._exp_avg, opt._exp_avg_sq), before))
            assert same == (g == 3), (gg.names[g], lo, hi)
    assert bool(model._flat.isfinite().all()) and opt._step_count == 2


def test_f_with_stage_one_param_groups_frozen_ranges_are_never_read():
    from ssi import ops
    from ssi.optimizer import HipAdamW
    model = _model(F32_MODEL, F32)
    segs = _segments(model, STAGE1, F32_TYPES)
    gg = _groups(model, {"groups": GROUPS[:1], "clip": {"max_norm": 0.25}}, F32_TYPES, segs)
    assert gg.names == ["new_rows"] and -1 in gg.seg_group
    opt = HipAdamW(model.parameters(), model=model, param_segments=segs, grad_groups=gg, **HYPER)
    P, M, V = model._flat.clone(), torch.zeros_like(model._flat), torch.zeros_like(model._flat)
    gen = torch.Generator().manual_seed(9)
    G = (torch.randn(model._flat.numel(), generator=gen) * 30.0).to(DEV)
    for s in segs:
        if s.frozen:
            G[s.start:s.end] = float("nan")                                               # a frozen gradient is unspecified
    model._flat_grad.copy_(G)
    model.attach_grads()
    sums, pending, values, _ = _window(model, opt, 1 / 37)
    assert bool(torch.isfinite(sums).all()) and float(values["clip"][0]) < 1 and not values["skipped"].any()
    _oracle_step(ops, P, G, M, V, gg.refined, values["clip"], pending, 1)
    torch.cuda.synchronize()
    assert _same_state(model, opt, P, M, V)
    for s in segs:
        assert torch.equal(model._flat[s.start:s.end], P[s.start:s.end]) and (not s.frozen or not opt._exp_avg[s.start:s.end].any())


# ---- through the trainer ------------------------------------------------------------------------------------------------------------------------
def _trainer(tmp, name, grad_groups, overrides=(), rules=None):
    from conftest import PKG
    from ssi.config import compose
    from ssi.constants import SEED
    from ssi.train_utils import resolve_n_dsus
    from ssi.trainer import Trainer, set_seed
    out = tmp / name
    cfg = compose(os.path.join(PKG, "conf"), "sft", [
        "data=sft/mls-speechtokenizer-rvq_0", "dtype=bf16", "tokenizer.max_seq_len=128", "data.train.dataloader.batch_size=2",
        "data.dev.dataloader.batch_size=2", "data.train.dataset.n_samples=24", "data.dev.dataset.n_samples=6", "gradient_accumulation_steps=2",
        "eval_steps=1000", "save_steps=1000", "log_interval=1", "lr_scheduler.num_warmup_steps=100", "optimizer.lr=2e-2", f"output_dir={out}",
        f"checkpointer.output_dir={out}/checkpoints", f"checkpointer.checkpoint_dir={out}/none", "checkpointer.allow_random_init=true", *overrides])
    cfg.model_overrides = dict(MFMA_SMALL)
    cfg.speech.n_dsus = 50
    cfg.data.n_dsus = 50
    if rules is not None:
        cfg.param_groups = rules
    if grad_groups is not None:
        cfg.grad_groups = grad_groups
    resolve_n_dsus(cfg)
    set_seed(SEED)
    t = Trainer(cfg)
    t.setup()
    V = t._llama_config.vocab_size
    t.data_train, t.data_dev = _Remap(t.data_train, V), _Remap(t.data_dev, V)
    t._loss_log = []
    t.records = []
    real = t.wandb_logger.log_dict
    t.wandb_logger.log_dict = lambda payload, step, real=real, t=t: (t.records.append((step, dict(payload))), real(payload, step=step))[1]
    return t


def _final(t):
    torch.cuda.synchronize()
    return [x.detach().clone() for x in (t.model._flat, t.optimizer._exp_avg, t.optimizer._exp_avg_sq)]


@pytest.fixture(scope="module")
def unkeyed(tmp_path_factory):
    """Three steps without the key: parameters and moments, shared by (a) and (b')."""
    t = _trainer(tmp_path_factory.mktemp("plain"), "plain", None, overrides=["max_steps=3"])
    t.train()
    out = (_final(t), list(t._loss_log), [dict(r) for _, r in t.records])
    t.cleanup()
    return out


def test_a_clip_null_changes_no_bit_and_logs_the_norms(tmp_path, unkeyed, monkeypatch):
    t = _trainer(tmp_path, "logged", {"groups": GROUPS, "clip": None}, overrides=["max_steps=3"])
    gg = t.optimizer._groups
    assert gg.names == ["new_rows", "embedding", "norms", "attn", "other"] and gg.clip is None
    seen = []
    real = t.optimizer.apply_grad_groups

    def spy():   # the gradient views and the scale of each window, as float64 norms
        G, scale = t.model._flat_grad, float(t.model.pending_grad_scale)
        seen.append(_norm64(G, _group_ranges(gg), scale))
        return real()
    monkeypatch.setattr(t.optimizer, "apply_grad_groups", spy)
    armed = []
    real_arm = t.optimizer.overlap_with_backward
    t.optimizer.overlap_with_backward = lambda s: (armed.append(1), real_arm(s))[1]
    t.train()
    state, losses, records = _final(t), list(t._loss_log), [dict(r) for _, r in t.records]
    t.cleanup()
    assert len(armed) == 3                                                                # AdamW stays under the backward
    assert losses == unkeyed[1] and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(state, unkeyed[0]))
    assert len(records) == 3 and len(seen) == 3
    b = _norm_bound(t.model, gg)
    for rec, want in zip(records, seen):
        assert sorted(k for k in rec if k.startswith("grad_")) == sorted(f"grad_norm.{n}" for n in gg.names)
        for name, w in zip(gg.names, want):
            got = rec[f"grad_norm.{name}"]
            print(f"grad_norm.{name}: logged {got:.7e} float64 {w:.7e} rel {abs(got - w) / w:.2e} bound {b:.2e}")
            assert w > 0 and abs(got - w) <= b * w
    assert not any(k.startswith("grad_") for r in unkeyed[2] for k in r)                  # without the key: no log key


def test_h_global_clip_from_the_group_sums_without_a_second_pass(tmp_path, monkeypatch):
    from ssi import ops
    calls = []
    real = ops.sumsq
    monkeypatch.setattr(ops, "sumsq", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    t = _trainer(tmp_path, "both", {"groups": GROUPS, "clip": {"max_norm": 1e9}}, overrides=["max_steps=2", "clip_grad_norm=0.05"])
    sums = []
    real_measure = t.optimizer.measure_grad_group_sums
    scales = []

    def spy():
        scales.append(t.model.pending_grad_scale.clone())
        s = real_measure()
        sums.append(s.clone())
        return s
    monkeypatch.setattr(t.optimizer, "measure_grad_group_sums", spy)
    t.train()
    torch.cuda.synchronize()
    records = [r for _, r in t.records]
    t.cleanup()
    assert not calls and len(records) == 2
    for rec, s, sc in zip(records, sums, scales):
        tot = s[0:1]
        for k in range(1, s.numel()):
            tot = tot + s[k:k + 1]
        want = float(tot.sqrt() * sc.abs())
        assert rec["grad_norm"] == want and want > 0.05                                   # the root of the summed group sums; the clip binds
        coef = min(1.0, 0.05 / (want + 1e-6))
        for k, name in enumerate(t.optimizer._groups.names):                              # the groups see the gradient after the global clip
            assert abs(rec[f"grad_norm.{name}"] - float(s[k].sqrt()) * float(sc.abs()) * coef) <= 1e-6 * rec[f"grad_norm.{name}"]
            assert rec[f"grad_clip.{name}"] == 1.0 and rec[f"grad_skipped.{name}"] == 0


def test_g_resume_is_bit_exact_gamma_included(tmp_path):
    node = {"groups": GROUPS, "clip": {"adaptive": {"rel": 1.02, "beta": 0.9, "warmup_steps": 1}, "max_norm": 1.0}}
    full = _trainer(tmp_path, "full", node, overrides=["max_steps=4"])
    full.train()
    want, losses = _final(full), list(full._loss_log)
    clip_full = full.optimizer._groups.clip.state_dict()
    full.cleanup()
    del full
    b1 = _trainer(tmp_path, "b1", node, overrides=["max_steps=2", "save_steps=2", "eval_steps=2"])
    b1.train()
    b1.cleanup()
    del b1
    ckpt = tmp_path / "b1" / "checkpoints"
    resume = [f"checkpointer.checkpoint_dir={ckpt}/step_2", "checkpointer.allow_random_init=false",
              f"checkpointer.training_state_checkpoint={ckpt}/training_state.pt"]
    b2 = _trainer(tmp_path, "b2", node, overrides=["max_steps=4", *resume])
    assert b2.optimizer._groups.clip.t == 2 and bool(b2.optimizer._groups.clip.has_gamma.all())
    b2.train()
    got = _final(b2)
    clip_b2 = b2.optimizer._groups.clip.state_dict()
    b2.cleanup()
    assert b2._loss_log == losses[2:] and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want))
    assert clip_b2["t"] == clip_full["t"] == 4
    assert all(torch.equal(clip_b2["groups"][n].view(torch.int32), clip_full["groups"][n].view(torch.int32)) for n in clip_full["groups"])
    del b2
    # the key belongs to the run's configuration: the state saved with it loads without it
    b3 = _trainer(tmp_path, "b3", None, overrides=["max_steps=3", *resume])
    assert b3.optimizer._groups is None and b3.optimizer._step_count == 2
    b3.train()
    assert len(b3._loss_log) == 1 and math.isfinite(b3._loss_log[0])
    b3.cleanup()
    del b3
    # ... and the other way round: a state saved without the key loads with it, every group starting unset
    c1 = _trainer(tmp_path, "c1", None, overrides=["max_steps=2", "save_steps=2", "eval_steps=2"])
    c1.train()
    c1.cleanup()
    del c1
    ckpt = tmp_path / "c1" / "checkpoints"
    resume = [f"checkpointer.checkpoint_dir={ckpt}/step_2", "checkpointer.allow_random_init=false",
              f"checkpointer.training_state_checkpoint={ckpt}/training_state.pt"]
    c2 = _trainer(tmp_path, "c2", node, overrides=["max_steps=3", *resume])
    clip = c2.optimizer._groups.clip
    assert c2.optimizer._step_count == 2 and clip.t == 0 and not clip.has_gamma.any()
    c2.train()
    assert len(c2._loss_log) == 1 and math.isfinite(c2._loss_log[0]) and clip.t == 1 and bool(clip.has_gamma.all())
    c2.cleanup()
