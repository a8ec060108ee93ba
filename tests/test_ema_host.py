"""CPU: the host side of the parameter average (``ema_decay``): the decay schedule, the config keys, the ABI plumbing, and that a trainer
whose config lacks the keys touches its optimizer and checkpointer exactly as before."""
import math
import os
import re
import struct
from unittest.mock import MagicMock

import pytest
import torch

from conftest import ROOT

PKG = os.path.join(ROOT, "speech-integration_amd")


def _f32(x: float) -> float:
    return struct.unpack("f", struct.pack("f", x))[0]


def test_decay_schedule_values_monotone_and_capped():
    from ssi.optimizer import ema_decay_at
    d = 0.9999
    assert ema_decay_at(1, d) == _f32(2 / 11) and ema_decay_at(10, d) == _f32(11 / 20) and ema_decay_at(10 ** 6, d) == _f32(d)
    assert ema_decay_at(1, d, False) == ema_decay_at(10, d, False) == ema_decay_at(10 ** 6, d, False) == _f32(d)
    assert ema_decay_at(1, 0.1) == _f32(0.1) and ema_decay_at(1, 0.0) == 0.0         # a decay below the warmup's is not raised to it
    for decay in (0.0, 0.5, 0.9, 0.999, 0.9999):
        values = [ema_decay_at(t, decay) for t in range(1, 200001, 7)] + [ema_decay_at(10 ** 6, decay)]
        assert all(a <= b for a, b in zip(values, values[1:])), decay
        assert all(0.0 <= v <= _f32(decay) for v in values), decay
        for t in (1, 2, 9, 10, 11, 89, 90, 8990, 89990, 10 ** 6):                    # the fp32 rounding of the double formula
            assert ema_decay_at(t, decay) == _f32(min(decay, (1.0 + t) / (10.0 + t))), (decay, t)
    assert isinstance(ema_decay_at(3, 0.9), float) and torch.tensor(ema_decay_at(3, 0.999), dtype=torch.float32).item() == ema_decay_at(3, 0.999)


def test_validate_train_cfg_checks_the_three_keys():
    from ssi.config import OmegaConf
    from ssi.train_utils import validate_train_cfg
    base = {"speech": {"n_dsus": 5000}, "dtype": "bf16", "gradient_accumulation_steps": 1, "max_steps": 1, "log_interval": 1, "eval_steps": 2,
            "save_steps": 4}
    validate_train_cfg(OmegaConf.create(base))                                           # absent: off
    for ok in (None, 0, 0.999, 0.9999):
        validate_train_cfg(OmegaConf.create({**base, "ema_decay": ok}))
    for bad in (-0.1, 1.0, float("nan"), True, "0.9"):
        with pytest.raises(ValueError, match="ema_decay"):
            validate_train_cfg(OmegaConf.create({**base, "ema_decay": bad}))
    for key in ("ema_warmup", "ema_eval"):
        validate_train_cfg(OmegaConf.create({**base, "ema_decay": 0.9, key: False}))
        for bad in (1, "yes", 0.5):
            with pytest.raises(ValueError, match=key):
                validate_train_cfg(OmegaConf.create({**base, "ema_decay": 0.9, key: bad}))


def test_training_yaml_has_the_keys_with_their_defaults():
    from ssi.config import compose
    lines = {k: next(l for l in open(os.path.join(PKG, "conf", "training.yaml")) if l.startswith(k + ":")) for k in ("ema_decay", "ema_warmup", "ema_eval")}
    assert lines["ema_decay"].split("#")[0].split(":", 1)[1].strip() == "null"
    assert lines["ema_warmup"].split("#")[0].split(":", 1)[1].strip() == "true" and lines["ema_eval"].split("#")[0].split(":", 1)[1].strip() == "true"
    assert all("# not in the reference:" in l for l in lines.values())
    cfg = compose(os.path.join(PKG, "conf"), "sft", ["data=sft/mls-hubert_large_ll60k-layer_22"])
    assert cfg.ema_decay is None and cfg.ema_warmup is True and cfg.ema_eval is True


def test_abi_version_symbol_and_wrapper():
    from ssi import _lib, ops
    text = open(os.path.join(ROOT, "include", "ssi_hip.h")).read()
    assert _lib.ABI_VERSION >= 17 and re.search(r"#define SSI_ABI_VERSION (\d+)", text).group(1) == str(_lib.ABI_VERSION)
    assert re.search(r"\bint ssi_ema_update\(", text) and "__builtin_fmaf(decay, ema[i] - p, p)" in text
    assert re.search(r"\* 17: \+ ssi_ema_update \(.*; opt-in\)", text)
    assert "ssi_ema_update" in _lib.PROTOTYPES and len(_lib.PROTOTYPES["ssi_ema_update"][1]) == 7
    assert "ema_update" in ops.__all__ and callable(ops.ema_update)
    with pytest.raises(_lib.HipLibraryError):
        ops.ema_update(torch.zeros(16), torch.zeros(16, dtype=torch.bfloat16), decay=0.9)
    with pytest.raises(TypeError):
        ops.ema_update(torch.zeros(16, dtype=torch.bfloat16), torch.zeros(16, dtype=torch.bfloat16), decay=0.9)


def test_setup_optimizer_refuses_the_average_on_a_foreign_module():
    from ssi.config import OmegaConf
    from ssi.optimizer import setup_optimizer
    cfg = OmegaConf.create({"optimizer": {"lr": 1e-3}, "ema_decay": 0.9})
    with pytest.raises(ValueError, match="ema_decay"):
        setup_optimizer(cfg, torch.nn.Linear(4, 4))
    assert isinstance(setup_optimizer(OmegaConf.create({"optimizer": {"lr": 1e-3}, "ema_decay": None}), torch.nn.Linear(4, 4)), torch.optim.AdamW)
    assert isinstance(setup_optimizer(OmegaConf.create({"optimizer": {"lr": 1e-3}}), torch.nn.Linear(4, 4)), torch.optim.AdamW)


def test_without_the_keys_the_trainer_touches_optimizer_and_checkpointer_as_before():
    from test_host_logic import _trainer_for_optimizer_step
    t, _ = _trainer_for_optimizer_step()
    t.model.state_dict = MagicMock(return_value={"w": torch.zeros(1)})
    t.global_step = 3
    t.save_checkpoint()
    assert [c[0] for c in t.checkpointer.method_calls] == ["save_model_checkpoint", "save_training_state"]
    assert [c[0] for c in t.optimizer.method_calls] == ["state_dict"]
    # a step that evaluates: one dev loss, no second one, no new key, nothing asked of the optimizer
    t.optimizer.reset_mock()
    t._evaluate = MagicMock(return_value=1.25)
    t.cfg.eval_steps = 1
    t.global_step = 1
    t._log_metrics(0, 1, 0.5)
    record = t.wandb_logger.log_dict.call_args.args[0]
    assert record["dev_loss"] == 1.25 and "dev_loss_ema" not in record
    t._evaluate.assert_called_once()
    assert [c[0] for c in t.optimizer.method_calls] == []
    assert t._evaluate_ema() is None and math.isfinite(record["loss"])
    # the same with the key present and null
    t.cfg.ema_decay = None
    t.save_checkpoint()
    assert "save_ema_checkpoint" not in [c[0] for c in t.checkpointer.method_calls]


def test_hf_checkpointer_writes_the_average_as_a_self_contained_hf_directory(tmp_path):
    from safetensors.torch import load_file
    from ssi.checkpoint import EMA_STATE_FILENAME, FullModelHFCheckpointer, tune_to_hf
    from ssi.constants import MODEL_KEY
    from test_checkpoint_hf import CONV, _tune_sd, _write_hf_dir
    sd = _tune_sd()
    src, out = tmp_path / "hf_model", tmp_path / "out"
    _write_hf_dir(src, tune_to_hf(sd, **CONV), shards=2)
    ck = FullModelHFCheckpointer(src, None, output_dir=out)
    ck.load_checkpoint()
    avg = {k: v.float() + 0.25 for k, v in sd.items()}
    ck.save_model_checkpoint(sd, 4)
    d = ck.save_ema_checkpoint({k: v.to(sd[k].dtype) for k, v in avg.items()}, avg, 4)
    assert str(d) == str(out / "step_4" / "ema") and sorted(f.name for f in (out / "step_4" / "ema").iterdir()) == sorted(
        f.name for f in (out / "step_4").iterdir() if f.name != "ema")                   # exactly the format step_4/ has
    again = FullModelHFCheckpointer(out / "step_4" / "ema", None, output_dir=tmp_path / "out2").load_checkpoint()[MODEL_KEY]
    assert sorted(again) == sorted(sd) and all(torch.equal(again[k], avg[k].to(sd[k].dtype)) for k in sd)
    state = load_file(str(out / EMA_STATE_FILENAME))
    assert all(state[k].dtype == torch.float32 and torch.equal(state[k], avg[k]) for k in sd)


def test_checkpointer_writes_the_average_as_a_model_directory_and_the_fp32_state(tmp_path):
    from safetensors.torch import load_file
    from ssi.checkpoint import EMA_STATE_FILENAME, make_checkpointer
    ck = make_checkpointer(checkpoint_dir=str(tmp_path / "none"), output_dir=str(tmp_path / "out"), allow_random_init=True)
    avg = {"w": torch.tensor([1.0, 2.0, 3.0]), "b": torch.tensor([0.1])}
    rounded = {k: v.to(torch.bfloat16) for k, v in avg.items()}
    ck.save_model_checkpoint({k: v + 1 for k, v in rounded.items()}, 4)
    ck.save_ema_checkpoint(rounded, avg, 4)
    assert sorted(os.listdir(tmp_path / "out")) == [EMA_STATE_FILENAME, "step_4"]
    assert sorted(os.listdir(tmp_path / "out" / "step_4")) == ["ema", "model.safetensors"] and os.listdir(tmp_path / "out" / "step_4" / "ema") == ["model.safetensors"]
    state = load_file(str(tmp_path / "out" / EMA_STATE_FILENAME))
    assert all(state[k].dtype == torch.float32 and torch.equal(state[k], avg[k]) for k in avg)
    loaded = make_checkpointer(checkpoint_dir=str(tmp_path / "out" / "step_4" / "ema"), output_dir=str(tmp_path / "out2")).load_checkpoint()["model"]
    assert all(loaded[k].dtype == torch.bfloat16 and torch.equal(loaded[k], rounded[k]) for k in avg)
