"""CPU: the host side of the KL term against a frozen teacher — the literal route of ``compute_loss(teacher=, teacher_kl_coeff=, teacher_kl_ranges=)``
on stand-in models against a hand-written fp64 expression, the masking by label ranges, the refusals of ``check_loss_options`` and of the config
validation, and the ctypes declaration of ``ssi_ce_fwd_kl`` against the header."""
import ctypes
import os
import re

import pytest
import torch

from test_ce_z_host import C_TYPES, _batch, _MeanCE, _StandIn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _teacher(vocab, chunks=0):
    teacher = _StandIn(vocab, chunks)
    with torch.no_grad():
        teacher.table.add_(0.7 * torch.randn(vocab, vocab, generator=torch.Generator().manual_seed(9)))
    return teacher


@pytest.mark.parametrize("ranges", [None, [(0, 5), (17, 19)]])
@pytest.mark.parametrize("chunks,teacher_chunks", [(0, 0), (4, 4), (4, 0)])
def test_literal_route_adds_the_coefficient_times_the_mean_kl_over_the_shifted_valid_labels(chunks, teacher_chunks, ranges):
    from ssi.loss import compute_loss
    vocab, b = 23, 0.5
    model, teacher, batch = _StandIn(vocab, chunks), _teacher(vocab, teacher_chunks), _batch(vocab)
    keep = {k: v.clone() for k, v in batch.items()}
    teacher_keep = teacher.table.detach().clone()
    plain = compute_loss(batch, model, _MeanCE())
    assert not hasattr(model, "last_kl_loss")
    assert torch.equal(compute_loss(batch, model, _MeanCE(), teacher=teacher, teacher_kl_coeff=0.0), plain) and not hasattr(model, "last_kl_loss")
    total = compute_loss(batch, model, _MeanCE(), teacher=teacher, teacher_kl_coeff=b, teacher_kl_ranges=ranges)
    total.backward()
    plain, total = plain.detach(), total.detach()
    assert all(torch.equal(batch[k], keep[k]) for k in keep)
    assert teacher.table.grad is None and torch.equal(teacher.table.detach(), teacher_keep), "the teacher is frozen"
    # by hand, in fp64
    table = model.table.detach().double().requires_grad_(True)
    shifted = torch.hstack((batch["labels"][:, 1:], torch.full((3, 1), -100)))
    x, t = table[batch["tokens"]], teacher.table.detach().double()[batch["tokens"]]
    valid = shifted != -100
    inside = torch.ones_like(valid)
    if ranges is not None:
        inside = torch.zeros_like(valid)
        for lo, hi in ranges:
            inside |= (shifted >= lo) & (shifted <= hi)
        assert 0 < int((valid & inside).sum()) < int(valid.sum()), "the ranges select some valid labels, not all"
    logp, logq = torch.log_softmax(x, -1), torch.log_softmax(t, -1)
    kl = (logq.exp() * (logq - logp)).sum(-1)
    nll = -logp.gather(-1, torch.where(valid, shifted, torch.zeros_like(shifted))[..., None])[..., 0]
    n_valid = valid.sum()
    ce64, kl64 = (nll * valid).sum() / n_valid, b * (kl * (valid & inside)).sum() / n_valid
    (ce64 + kl64).backward()
    ce64, kl64 = ce64.detach(), kl64.detach()
    assert float(total) == pytest.approx(float(ce64 + kl64), rel=1e-6) and float(kl64) > 1e-3 * float(ce64)   # a thousand times the bound: the term is in the sum
    assert float(model.last_ce_loss) == pytest.approx(float(ce64), rel=1e-6) and torch.equal(model.last_ce_loss, plain)
    assert float(model.last_kl_loss) == pytest.approx(float(kl64), rel=1e-6)
    assert not model.last_ce_loss.requires_grad and not model.last_kl_loss.requires_grad
    torch.testing.assert_close(model.table.grad.double(), table.grad, rtol=1e-5, atol=1e-7)


def test_a_teacher_equal_to_the_model_adds_nothing():
    from ssi.loss import compute_loss
    model, batch = _StandIn(23), _batch(23)
    teacher = _StandIn(23)
    total = compute_loss(batch, model, _MeanCE(), teacher=teacher, teacher_kl_coeff=2.0)
    assert abs(float(model.last_kl_loss)) < 1e-6 and float(total.detach()) == pytest.approx(float(model.last_ce_loss), abs=1e-6)


def test_the_range_mask_on_shifted_labels():
    from ssi.loss import kl_range_mask
    labels = torch.tensor([[0, 4, 5, 6, -100], [19, 20, 17, 16, 3]])
    assert kl_range_mask(labels, None) is None
    got = kl_range_mask(labels, [(0, 5), (17, 19)])                  # inclusive at both ends; the ignore index lies in no range
    assert got.dtype == torch.bool and got.shape == labels.shape
    assert got.tolist() == [[True, True, True, False, False], [True, False, True, False, True]]
    assert not kl_range_mask(labels, []).any()


def test_bad_values_and_combinations_are_refused():
    from ssi.loss import check_loss_options, compute_loss
    model, teacher, batch = _StandIn(23), _teacher(23), _batch(23)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="teacher_kl_coeff"):
            compute_loss(batch, model, _MeanCE(), teacher=teacher, teacher_kl_coeff=bad)
    with pytest.raises(ValueError, match="needs a teacher"):
        compute_loss(batch, model, _MeanCE(), teacher_kl_coeff=0.5)
    for kw in ({"label_metrics": object()}, {"seq_scores": object()}, {"z_loss_coeff": 1e-4}, {"label_smoothing": 0.1}):
        with pytest.raises(ValueError, match="teacher_kl_coeff and " + next(iter(kw))):
            compute_loss(batch, model, _MeanCE(), teacher=teacher, teacher_kl_coeff=0.5, **kw)
        args = {"label_smoothing": 0.0, "z_loss_coeff": 0.0, **kw}
        with pytest.raises(ValueError, match="fused_loss: teacher_kl_coeff and " + next(iter(kw))):
            check_loss_options("fused_loss", teacher_kl_coeff=0.5, **args)
        check_loss_options("fused_loss", teacher_kl_coeff=0.0, **args)   # off: the combinations of before
    assert check_loss_options("fused_loss", 0.1, 1e-4) == (0.1, 1e-4)    # what it returns is what it returned


def test_the_config_keys_are_validated_and_default_to_off():
    from conftest import PKG
    from ssi.config import OmegaConf, compose
    from ssi.train_utils import validate_train_cfg
    from ssi.trainer import Trainer
    base = {"speech": {"n_dsus": 5000}, "dtype": "bf16", "gradient_accumulation_steps": 1, "max_steps": 1, "log_interval": 1, "eval_steps": 2,
            "save_steps": 4}
    validate_train_cfg(OmegaConf.create(base))                      # absent: off
    for good in (0.0, 0, 0.5, 3, "1e-1"):
        validate_train_cfg(OmegaConf.create({**base, "teacher_kl_coeff": good}))
    validate_train_cfg(OmegaConf.create({**base, "teacher_kl_coeff": 0.5, "teacher_kl_token_types": ["text"], "teacher_checkpoint_dir": "/some/where"}))
    validate_train_cfg(OmegaConf.create({**base, "teacher_kl_coeff": 0.0, "z_loss_coeff": 1e-4, "label_smoothing": 0.1}))   # off: nothing to refuse
    for bad in (-0.1, float("nan"), float("inf"), "much", True):
        with pytest.raises(ValueError, match="teacher_kl_coeff"):
            validate_train_cfg(OmegaConf.create({**base, "teacher_kl_coeff": bad}))
        with pytest.raises(ValueError, match="teacher_kl_coeff"):     # ... which is where Trainer.setup() starts
            Trainer(OmegaConf.create({**base, "teacher_kl_coeff": bad})).setup()
    for other in ({"z_loss_coeff": 1e-4}, {"label_smoothing": 0.1}):
        with pytest.raises(ValueError, match="'teacher_kl_coeff' and '" + next(iter(other))):
            validate_train_cfg(OmegaConf.create({**base, "teacher_kl_coeff": 0.5, **other}))
    for bad in ("text", [], [3]):
        with pytest.raises(ValueError, match="teacher_kl_token_types"):
            validate_train_cfg(OmegaConf.create({**base, "teacher_kl_coeff": 0.5, "teacher_kl_token_types": bad}))
    with pytest.raises(ValueError, match="teacher_checkpoint_dir"):
        validate_train_cfg(OmegaConf.create({**base, "teacher_kl_coeff": 0.5, "teacher_checkpoint_dir": 7}))
    cfg = compose(os.path.join(PKG, "conf"), "sft", ["data=sft/mls-hubert_large_ll60k-layer_22"])
    assert cfg.teacher_kl_coeff == 0.0 and cfg.teacher_checkpoint_dir is None and cfg.teacher_kl_token_types is None
    t = Trainer(cfg)
    assert t.teacher_kl_coeff == 0.0 and t.teacher is None and t.teacher_kl_ranges is None
    for key in ("teacher_kl_coeff", "teacher_checkpoint_dir", "teacher_kl_token_types"):
        line = next(l for l in open(os.path.join(PKG, "conf", "training.yaml")) if l.startswith(key + ":"))
        assert "not in the reference" in line
    import inspect
    from ssi.loss import compute_loss
    params = inspect.signature(compute_loss).parameters
    assert list(params)[:3] == ["batch", "model", "loss_fn"]                  # the reference's signature is a prefix
    assert params["teacher"].default is None and params["teacher_kl_coeff"].default == 0.0 and params["teacher_kl_ranges"].default is None


def test_lib_declares_ssi_ce_fwd_kl_with_the_headers_signature():
    from ssi import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssi_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+ssi_ce_fwd_kl\s*\(([^)]*)\)\s*;", text)
    assert m, "include/ssi_hip.h does not declare ssi_ce_fwd_kl"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    names = [re.split(r"[ *]", p)[-1] for p in params]
    assert names == ["logits", "ld", "teacher", "ld_teacher", "teacher_lse", "labels", "row_weight", "row_kl_weight", "rows", "vocab",
                     "ignore_index", "kl_coeff", "row_loss", "row_lse", "row_kl", "write_grad", "dtype", "stream"]
    want = [ctypes.c_void_p if "*" in p else C_TYPES[p.rsplit(" ", 1)[0].replace("const ", "")] for p in params]
    res, args = _lib.PROTOTYPES["ssi_ce_fwd_kl"]
    assert res is ctypes.c_int and args == want
    assert _lib.ABI_VERSION >= 15 and re.search(r"#define SSI_ABI_VERSION (\d+)", text).group(1) == str(_lib.ABI_VERSION)
    from ssi import ops
    assert "ce_fwd_kl" in ops.__all__ and callable(ops.ce_fwd_kl)
