"""CPU: the host side of the auxiliary z-loss — the literal route of ``compute_loss(z_loss_coeff=)`` on a stand-in model against a hand-written
fp64 expression, the config validation, and the ctypes declaration of ``ssi_ce_fwd_z`` against the header."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _StandIn(torch.nn.Module):
    """tokens -> logits ``[B, S, V]`` (or their chunks along S) from one embedding-like parameter; no ``fused_loss``: the literal route."""

    def __init__(self, vocab, chunks=0):
        super().__init__()
        self.table = torch.nn.Parameter(torch.randn(vocab, vocab, generator=torch.Generator().manual_seed(3)) * 2.0)
        self.chunks = chunks

    def forward(self, tokens, mask=None, encoder_input=None, encoder_mask=None, input_pos=None):
        logits = self.table[tokens]
        return list(logits.chunk(self.chunks, dim=1)) if self.chunks else logits


class _MeanCE:
    ignore_index = -100

    def __call__(self, logits, labels):
        if isinstance(logits, list):
            logits, labels = torch.cat(logits, dim=1).reshape(-1, logits[0].size(-1)), labels.reshape(-1)
        return F.cross_entropy(logits.float(), labels, ignore_index=self.ignore_index)


def _batch(vocab):
    g = torch.Generator().manual_seed(4)
    tokens = torch.randint(0, vocab, (3, 17), generator=g)
    labels = torch.randint(0, vocab, (3, 17), generator=g)
    labels[0, :5] = -100
    labels[2] = -100
    return {"tokens": tokens, "labels": labels}


@pytest.mark.parametrize("chunks", [0, 4])
def test_literal_route_adds_z_times_mean_squared_lse_over_the_shifted_valid_labels(chunks):
    from ssi.loss import compute_loss
    vocab, z = 23, 0.3
    model, batch = _StandIn(vocab, chunks), _batch(vocab)
    keep = {k: v.clone() for k, v in batch.items()}
    plain = compute_loss(batch, model, _MeanCE())
    assert not hasattr(model, "last_z_loss")
    assert torch.equal(compute_loss(batch, model, _MeanCE(), z_loss_coeff=0.0), plain)
    total = compute_loss(batch, model, _MeanCE(), z_loss_coeff=z)
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
    ce64, z64 = (nll * valid).sum() / n_valid, z * (lse * lse * valid).sum() / n_valid
    (ce64 + z64).backward()
    ce64, z64 = ce64.detach(), z64.detach()
    assert float(plain) == pytest.approx(float(ce64), rel=1e-6)
    assert float(total) == pytest.approx(float(ce64 + z64), rel=1e-6) and float(z64) > 0.1 * float(ce64)
    assert float(model.last_ce_loss) == pytest.approx(float(ce64), rel=1e-6) and float(model.last_z_loss) == pytest.approx(float(z64), rel=1e-6)
    assert not model.last_ce_loss.requires_grad and not model.last_z_loss.requires_grad
    torch.testing.assert_close(model.table.grad.double(), table.grad, rtol=1e-5, atol=1e-7)


def test_literal_route_refuses_loss_weights_and_bad_coefficients():
    from ssi.loss import compute_loss
    model, batch = _StandIn(23), _batch(23)
    with pytest.raises(ValueError, match="loss_weights"):
        compute_loss({**batch, "loss_weights": torch.ones(3, 17)}, model, _MeanCE(), z_loss_coeff=0.1)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="z_loss_coeff"):
            compute_loss(batch, model, _MeanCE(), z_loss_coeff=bad)


def test_the_config_key_is_validated_and_defaults_to_off():
    from conftest import PKG
    from ssi.config import OmegaConf, compose
    from ssi.train_utils import validate_train_cfg
    from ssi.trainer import Trainer
    base = {"speech": {"n_dsus": 5000}, "dtype": "bf16", "gradient_accumulation_steps": 1, "max_steps": 1, "log_interval": 1, "eval_steps": 2,
            "save_steps": 4}
    validate_train_cfg(OmegaConf.create(base))                      # absent: off
    for good in (0.0, 0, 1e-4, "1e-4"):                              # ("1e-4": YAML 1.1 reads it as a string, the config layer as a float)
        validate_train_cfg(OmegaConf.create({**base, "z_loss_coeff": good}))
    for bad in (-1e-4, float("nan"), float("inf"), "much", True):
        with pytest.raises(ValueError, match="z_loss_coeff"):
            validate_train_cfg(OmegaConf.create({**base, "z_loss_coeff": bad}))
        with pytest.raises(ValueError, match="z_loss_coeff"):        # ... which is where Trainer.setup() starts
            Trainer(OmegaConf.create({**base, "z_loss_coeff": bad})).setup()
    cfg = compose(os.path.join(PKG, "conf"), "sft", ["data=sft/mls-hubert_large_ll60k-layer_22"])
    assert cfg.z_loss_coeff == 0.0 and Trainer(cfg).z_loss_coeff == 0.0
    line = next(l for l in open(os.path.join(PKG, "conf", "training.yaml")) if l.startswith("z_loss_coeff:"))
    assert "not in the reference" in line and "dev_loss" in line
    import inspect
    from ssi.loss import CEWithChunkedOutputLoss, compute_loss
    assert list(inspect.signature(compute_loss).parameters)[:3] == ["batch", "model", "loss_fn"]                  # the reference's signature is a prefix
    assert list(inspect.signature(CEWithChunkedOutputLoss.__init__).parameters) == ["self", "num_output_chunks", "ignore_index"]  # torchtune's


C_TYPES = {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}


def test_lib_declares_ssi_ce_fwd_z_with_the_headers_signature():
    from ssi import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ssi_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+ssi_ce_fwd_z\s*\(([^)]*)\)\s*;", text)
    assert m, "include/ssi_hip.h does not declare ssi_ce_fwd_z"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    names = [re.split(r"[ *]", p)[-1] for p in params]
    assert names == ["logits", "ld", "labels", "row_weight", "rows", "vocab", "ignore_index", "z_coeff", "row_loss", "row_lse", "row_z",
                     "write_grad", "dtype", "stream"]
    want = [ctypes.c_void_p if "*" in p else C_TYPES[p.rsplit(" ", 1)[0].replace("const ", "")] for p in params]
    res, args = _lib.PROTOTYPES["ssi_ce_fwd_z"]
    assert res is ctypes.c_int and args == want
    assert _lib.ABI_VERSION >= 12 and re.search(r"#define SSI_ABI_VERSION (\d+)", text).group(1) == str(_lib.ABI_VERSION)
