"""CPU: the host side of label smoothing — the literal route of ``compute_loss(label_smoothing=)`` on a stand-in model against a hand-written
fp64 expression and against torch's own ``label_smoothing``, the validation of the argument and of the config key, and the ctypes declaration
of ``ssi_ce_fwd_smooth`` against the header."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from test_ce_z_host import C_TYPES, _batch, _MeanCE, _StandIn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("z", [0.0, 0.3])
@pytest.mark.parametrize("chunks", [0, 4])
def test_literal_route_is_torchs_label_smoothing_over_the_shifted_valid_labels(chunks, z):
    from ssi.loss import compute_loss
    vocab, e = 23, 0.1
    model, batch = _StandIn(vocab, chunks), _batch(vocab)
    keep = {k: v.clone() for k, v in batch.items()}
    plain = compute_loss(batch, model, _MeanCE())
    assert not hasattr(model, "last_smooth_loss")
    assert torch.equal(compute_loss(batch, model, _MeanCE(), label_smoothing=0.0), plain) and not hasattr(model, "last_smooth_loss")
    total = compute_loss(batch, model, _MeanCE(), label_smoothing=e, z_loss_coeff=z)
    total.backward()
    plain, total = plain.detach(), total.detach()
    assert all(torch.equal(batch[k], keep[k]) for k in keep)
    # by hand, in fp64
    table = model.table.detach().double().requires_grad_(True)
    shifted = torch.hstack((batch["labels"][:, 1:], torch.full((3, 1), -100)))
    x = table[batch["tokens"]]
    valid = shifted != -100
    lse = torch.logsumexp(x, dim=-1)
    nll = lse - x.gather(-1, torch.where(valid, shifted, torch.zeros_like(shifted))[..., None])[..., 0]
    n_valid = valid.sum()
    ce64, u64 = (nll * valid).sum() / n_valid, e * ((lse - x.mean(dim=-1)) * valid).sum() / n_valid
    z64 = z * (lse * lse * valid).sum() / n_valid
    ((1 - e) * ce64 + u64 + z64).backward()
    ce64, u64, z64 = ce64.detach(), u64.detach(), z64.detach()
    assert float(total) == pytest.approx(float((1 - e) * ce64 + u64 + z64), rel=1e-6) and float(u64) > 0.02 * float(ce64)
    assert float(model.last_ce_loss) == pytest.approx(float(ce64), rel=1e-6) and torch.equal(model.last_ce_loss, plain)
    assert float(model.last_smooth_loss) == pytest.approx(float(u64), rel=1e-6)
    assert not model.last_ce_loss.requires_grad and not model.last_smooth_loss.requires_grad
    if z:
        assert float(model.last_z_loss) == pytest.approx(float(z64), rel=1e-6)
    else:
        assert not hasattr(model, "last_z_loss")
    torch.testing.assert_close(model.table.grad.double(), table.grad, rtol=1e-5, atol=1e-7)
    # torch's own label smoothing on the same logits, in fp64
    t64 = F.cross_entropy(table.detach()[batch["tokens"]].reshape(-1, vocab), shifted.reshape(-1), label_smoothing=e, ignore_index=-100)
    assert float(total - z64) == pytest.approx(float(t64), rel=1e-6)


def test_bad_values_and_combinations_are_refused():
    from ssi.loss import compute_loss
    model, batch = _StandIn(23), _batch(23)
    with pytest.raises(ValueError, match="loss_weights"):
        compute_loss({**batch, "loss_weights": torch.ones(3, 17)}, model, _MeanCE(), label_smoothing=0.1)
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="label_smoothing"):
            compute_loss(batch, model, _MeanCE(), label_smoothing=bad)
    for kw in ({"label_metrics": object()}, {"seq_scores": object()}):
        with pytest.raises(ValueError, match="label_smoothing"):
            compute_loss(batch, model, _MeanCE(), label_smoothing=0.1, **kw)


def test_the_config_key_is_validated_and_defaults_to_off():
    from conftest import PKG
    from ssi.config import OmegaConf, compose
    from ssi.train_utils import validate_train_cfg
    from ssi.trainer import Trainer
    base = {"speech": {"n_dsus": 5000}, "dtype": "bf16", "gradient_accumulation_steps": 1, "max_steps": 1, "log_interval": 1, "eval_steps": 2,
            "save_steps": 4}
    validate_train_cfg(OmegaConf.create(base))                      # absent: off
    for good in (0.0, 0, 0.1, 0.999, "1e-1"):                        # ("1e-1": YAML 1.1 reads it as a string, the config layer as a float)
        validate_train_cfg(OmegaConf.create({**base, "label_smoothing": good}))
    validate_train_cfg(OmegaConf.create({**base, "label_smoothing": 0.1, "z_loss_coeff": 1e-4}))   # both at once
    for bad in (-0.1, 1.0, 1, float("nan"), float("inf"), "much", True):
        with pytest.raises(ValueError, match="label_smoothing"):
            validate_train_cfg(OmegaConf.create({**base, "label_smoothing": bad}))
        with pytest.raises(ValueError, match="label_smoothing"):     # ... which is where Trainer.setup() starts
            Trainer(OmegaConf.create({**base, "label_smoothing": bad})).setup()
    cfg = compose(os.path.join(PKG, "conf"), "sft", ["data=sft/mls-hubert_large_ll60k-layer_22"])
    assert cfg.label_smoothing == 0.0 and Trainer(cfg).label_smoothing == 0.0
    line = next(l for l in open(os.path.join(PKG, "conf", "training.yaml")) if l.startswith("label_smoothing:"))
    assert "not in the reference" in line and "dev_loss" in line
    import inspect
    from ssi.loss import CEWithChunkedOutputLoss, compute_loss
    assert list(inspect.signature(compute_loss).parameters)[:3] == ["batch", "model", "loss_fn"]                  # the reference's signature is a prefix
    assert inspect.signature(compute_loss).parameters["label_smoothing"].default == 0.0
    assert list(inspect.signature(CEWithChunkedOutputLoss.__init__).parameters) == ["self", "num_output_chunks", "ignore_index"]  # torchtune's


def test_lib_declares_ssi_ce_fwd_smooth_with_the_headers_signature():
    from ssi import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssi_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+ssi_ce_fwd_smooth\s*\(([^)]*)\)\s*;", text)
    assert m, "include/ssi_hip.h does not declare ssi_ce_fwd_smooth"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    names = [re.split(r"[ *]", p)[-1] for p in params]
    assert names == ["logits", "ld", "labels", "row_weight", "rows", "vocab", "ignore_index", "smoothing", "z_coeff", "row_loss", "row_lse",
                     "row_u", "row_z", "write_grad", "dtype", "stream"]
    want = [ctypes.c_void_p if "*" in p else C_TYPES[p.rsplit(" ", 1)[0].replace("const ", "")] for p in params]
    res, args = _lib.PROTOTYPES["ssi_ce_fwd_smooth"]
    assert res is ctypes.c_int and args == want
    assert _lib.ABI_VERSION >= 14 and re.search(r"#define SSI_ABI_VERSION (\d+)", text).group(1) == str(_lib.ABI_VERSION)
    from ssi import ops
    assert "ce_fwd_smooth" in ops.__all__ and callable(ops.ce_fwd_smooth)
