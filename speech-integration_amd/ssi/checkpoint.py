"""Checkpoint I/O either side of the hot path.

``FullModelHFCheckpointer`` (second half of this file) reads and writes HF-format Llama-3.2 model directories exactly as the
reference's class of the same name does (``/root/reference/ssi/checkpoint.py:209-468``): sharded safetensors, config.json
validation, HF<->torchtune key map with the q/k row permutation, ``step_N/`` output directories, schema-v1
``training_state.pt`` (``constants.py:78-89``).  ``TuneCheckpointer`` is the single-file variant used when ``checkpoint_dir`` is
not an HF model directory: ONE safetensors file whose keys are the torchtune names the model exposes; with no weights on disk
it raises unless ``allow_random_init`` was set (then the model is random-initialised, seeded — there are no Llama weights on the
build/GPU image and no network).  Both expose
``load_checkpoint() -> {"model": state_dict | None, ...training-state keys}``, ``save_model_checkpoint(state_dict, step)``,
``save_training_state(...)``, ``training_state_checkpoint``; ``make_checkpointer`` picks one."""

from __future__ import annotations

import logging
import os
import random
from typing import Any

import numpy as np
import torch

from .constants import (CHECKPOINT_VERSION, CHECKPOINT_VERSION_KEY, CONSUMED_SAMPLES_KEY, CUMULATIVE_METRICS_KEY,
                        GLOBAL_STEP_KEY, LR_SCHEDULER_KEY, MODEL_KEY, OPTIMIZER_KEY, RNG_KEY, SEED_KEY, TRAINING_HPARAMS_KEY)

LOGGER = logging.getLogger(__name__)
MODEL_FILENAME = "model.safetensors"
TRAINING_STATE_FILENAME = "training_state.pt"


def resolve_checkpointer_output_dir(cfg, wandb_logger) -> str:
    base = cfg.get("output_dir") or os.path.join(os.getcwd(), "outputs")
    return os.path.join(str(base), f"{getattr(wandb_logger, 'run_name', 'local')}-id_{getattr(wandb_logger, 'run_id', '0')}", "checkpoints")


def save_rng_states() -> dict[str, Any]:
    """Python / NumPy / torch generator states (what ``/root/reference/ssi/checkpoint.py:188-197`` saves).  The NumPy Mersenne-Twister
    key array is stored as a TENSOR, under a key of its own (``numpy_global_tensors``): ``training_state.pt`` then holds nothing but
    tensors and plain containers and loads with ``torch.load(weights_only=True)``.  The reference's ``numpy_global`` entry is the raw
    ``np.random.get_state()`` tuple (an ndarray inside), which that restricted loader refuses — the two writers' files are therefore
    NOT interchangeable ("training_state.pt"); model weights (safetensors) are."""
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    state = {"python": random.getstate(),
             "numpy_global_tensors": (str(kind), torch.from_numpy(np.asarray(keys, dtype=np.int64)), int(pos), int(has_gauss), float(cached)),
             "torch_cpu": torch.get_rng_state()}
    if torch.cuda.is_available():
        state["torch_cuda"] = torch.cuda.get_rng_state_all()
    return state


def restore_rng_states(state: dict[str, Any]) -> None:
    py = state["python"]
    random.setstate((py[0], tuple(py[1]), py[2]))  # lists -> tuples if a loader relaxed them
    # "numpy_global" with a tensor inside: files this package wrote before the key was renamed
    entry = state.get("numpy_global_tensors", state.get("numpy_global"))
    if entry is None or not torch.is_tensor(entry[1]):
        raise RuntimeError("training state without a loadable NumPy generator state: neither `numpy_global_tensors` (this package) nor a "
                           "tensor-valued `numpy_global` (its early builds); the reference stores the state as a NumPy array, which the "
                           "restricted loader never unpickles (INTEGRATION.md, training-state compatibility)")
    kind, keys, pos, has_gauss, cached = entry
    np.random.set_state((str(kind), keys.numpy().astype(np.uint32), int(pos), int(has_gauss), float(cached)))
    torch.set_rng_state(state["torch_cpu"])
    if "torch_cuda" in state and torch.cuda.is_available():
        torch.cuda.set_rng_state_all(state["torch_cuda"])


def load_training_state(path: str) -> dict[str, Any]:
    """``training_state.pt`` through the restricted unpickler only (tensors, numbers, strings, lists/tuples/dicts): nothing in the
    file is executed (reference: ``safe_torch_load``, ``ssi/checkpoint.py:334``)."""
    import pickle
    try:
        return torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError as e:
        raise RuntimeError(
            f"{path}: not loadable by the restricted loader (weights_only=True).  It was written by the reference trainer or by an early "
            "build of this package, whose RNG section holds NumPy arrays (`numpy_global` / `numpy`); such objects are never unpickled "
            "here.  Resume from a training state written by this package, or restart the optimizer state from the model weights "
            f"(checkpointer.training_state_checkpoint=null).  Loader message: {e}") from e


@torch.no_grad()
def random_init_(model, seed: int, std: float = 0.02) -> None:
    """Seeded N(0, std^2) weights, unit norm scales (throughput and parity tests are weight-value independent)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    for name, p in model.named_parameters():
        if name.endswith("scale"):
            p.fill_(1.0)
        else:
            rows = max(1, (1 << 22) // max(1, p.shape[-1]))  # stream in ~4M-element slabs to bound host memory
            flat = p.view(-1, p.shape[-1])
            for r0 in range(0, flat.shape[0], rows):
                blk = torch.randn(min(rows, flat.shape[0] - r0), flat.shape[1], generator=g) * std
                flat[r0:r0 + blk.shape[0]].copy_(blk.to(p.dtype))


EMA_STATE_FILENAME = "ema_state.safetensors"   # the fp32 parameter averages of a run with ema_decay, beside training_state.pt


class TuneCheckpointer:
    def __init__(self, checkpoint_dir: str | None = None, checkpoint_files: Any = None, config_json: Any = None,
                 output_dir: str | None = None, training_state_checkpoint: str | None = None, safe_serialization: bool = True,
                 model_expectations: Any = None, allow_random_init: bool = False, **_: Any) -> None:
        self.checkpoint_dir, self.output_dir = checkpoint_dir, output_dir
        self.training_state_checkpoint = training_state_checkpoint
        self.model_expectations = model_expectations
        self.allow_random_init = bool(allow_random_init)
        if self.training_state_checkpoint is not None and not os.path.isfile(str(self.training_state_checkpoint)):
            raise FileNotFoundError(f"Recipe checkpoint file {self.training_state_checkpoint} not found.")

    def load_checkpoint(self) -> dict[str, Any]:
        out: dict[str, Any] = {MODEL_KEY: None}
        path = os.path.join(str(self.checkpoint_dir), MODEL_FILENAME) if self.checkpoint_dir else None
        if path and os.path.exists(path):
            from safetensors.torch import load_file
            out[MODEL_KEY] = load_file(path)
            LOGGER.info(f"Loaded {len(out[MODEL_KEY])} tensors from {path}")
        elif self.allow_random_init:
            LOGGER.warning(f"No {MODEL_FILENAME} under {self.checkpoint_dir!r}: checkpointer.allow_random_init is set, the model "
                           "will be random-initialised (seeded).")
        else:  # a mistyped or unmounted checkpoint_dir must not silently train from noise (reference: ssi/checkpoint.py:263-264)
            raise FileNotFoundError(f"No {MODEL_FILENAME} (and no HF config.json) under checkpoint_dir={self.checkpoint_dir!r}. Point "
                                    "checkpointer.checkpoint_dir at a model directory, or set checkpointer.allow_random_init=true to "
                                    "train from seeded random weights.")
        if self.training_state_checkpoint is not None:
            out.update(load_training_state(self.training_state_checkpoint))
        return out

    def save_model_checkpoint(self, state_dict: dict[str, torch.Tensor], global_step: int) -> str:
        return self._save_model_file(state_dict, os.path.join(str(self.output_dir), f"step_{global_step}"))

    @staticmethod
    def _save_model_file(state_dict: dict[str, torch.Tensor], d: str) -> str:
        from safetensors.torch import save_file
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, MODEL_FILENAME)
        save_file({k: v.detach().to("cpu").contiguous() for k, v in state_dict.items()}, path)
        return path

    def save_ema_checkpoint(self, model_state_dict: dict[str, torch.Tensor], ema_state_dict: dict[str, torch.Tensor], global_step: int) -> str:
        """(not in the reference; a run with ``ema_decay``) ``model_state_dict``: the averaged weights in the model's dtype, written under
        ``step_N/ema/`` in exactly the format ``step_N/`` has — a model directory of its own.  ``ema_state_dict``: the fp32 averages by
        state-dict name, written to ``ema_state.safetensors`` beside ``training_state.pt`` (overwritten by every save, as that file is)."""
        d = self._save_ema_model(model_state_dict, global_step)
        self._save_ema_state(ema_state_dict)
        return d

    def _save_ema_model(self, model_state_dict: dict[str, torch.Tensor], global_step: int) -> str:
        d = os.path.join(str(self.output_dir), f"step_{global_step}", "ema")
        self._save_model_file(model_state_dict, d)
        return d

    def _save_ema_state(self, ema_state_dict: dict[str, torch.Tensor]) -> str:
        from safetensors.torch import save_file
        os.makedirs(str(self.output_dir), exist_ok=True)
        path = os.path.join(str(self.output_dir), EMA_STATE_FILENAME)
        save_file({k: v.detach().to("cpu", torch.float32).contiguous() for k, v in ema_state_dict.items()}, path)
        return path

    def save_training_state(self, optimizer_state_dict, lr_scheduler_state_dict, global_step: int, seed: int,
                            training_hparams: dict, consumed_samples: int, cumulative_metrics: dict) -> str:
        os.makedirs(str(self.output_dir), exist_ok=True)
        path = os.path.join(str(self.output_dir), TRAINING_STATE_FILENAME)
        torch.save({
            CHECKPOINT_VERSION_KEY: CHECKPOINT_VERSION, OPTIMIZER_KEY: optimizer_state_dict,
            LR_SCHEDULER_KEY: lr_scheduler_state_dict, GLOBAL_STEP_KEY: global_step, SEED_KEY: seed, RNG_KEY: save_rng_states(),
            TRAINING_HPARAMS_KEY: training_hparams, CONSUMED_SAMPLES_KEY: consumed_samples,
            CUMULATIVE_METRICS_KEY: cumulative_metrics}, path)
        return path


# =====================================================================================================================
# HF-format checkpoints: the on-disk format either side of the hot path.
# Mirrors the reference's ``FullModelHFCheckpointer`` (``/root/reference/ssi/checkpoint.py:209-468``) and the torchtune 0.5.0
# ``convert_weights.hf_to_tune / tune_to_hf`` it calls (``:325-331, :352-358``; key map and q/k row permutation restated from
# SURVEY.md §8b / Appendix A.3).  Only safetensors are read (nothing in a checkpoint file is executed).
# =====================================================================================================================
import gc
import json
import re
import shutil
from pathlib import Path

SHARD_FNAME = "model-{cpt_idx}-of-{num_shards}"
SAFETENSOR_INDEX_FNAME = "model.safetensors.index.json"
LLAMA_3_2_CONFIG_RELPATH = Path("config.json")
SUFFIXES_TO_NOT_COPY = (".safetensors", ".bin", ".pt", ".pth", ".index.json")

_HF_TO_TUNE = {
    "model.embed_tokens.weight": "tok_embeddings.weight",
    "model.layers.{}.self_attn.q_proj.weight": "layers.{}.attn.q_proj.weight",
    "model.layers.{}.self_attn.k_proj.weight": "layers.{}.attn.k_proj.weight",
    "model.layers.{}.self_attn.v_proj.weight": "layers.{}.attn.v_proj.weight",
    "model.layers.{}.self_attn.o_proj.weight": "layers.{}.attn.output_proj.weight",
    "model.layers.{}.mlp.gate_proj.weight": "layers.{}.mlp.w1.weight",
    "model.layers.{}.mlp.down_proj.weight": "layers.{}.mlp.w2.weight",
    "model.layers.{}.mlp.up_proj.weight": "layers.{}.mlp.w3.weight",
    "model.layers.{}.input_layernorm.weight": "layers.{}.sa_norm.scale",
    "model.layers.{}.post_attention_layernorm.weight": "layers.{}.mlp_norm.scale",
    "model.norm.weight": "norm.scale",
    "lm_head.weight": "output.weight",
}
_TUNE_TO_HF = {v: k for k, v in _HF_TO_TUNE.items()}
_LAYER_RE = re.compile(r"(\.layers\.|^layers\.)(\d+)\.")


def _map_key(key: str, table: dict[str, str]) -> str:
    m = _LAYER_RE.search(key)
    if m is None:
        if key not in table:
            raise KeyError(f"unexpected checkpoint key {key!r}")
        return table[key]
    generic = key[:m.start(2)] + "{}" + key[m.end(2):]
    if generic not in table:
        raise KeyError(f"unexpected checkpoint key {key!r}")
    return table[generic].format(m.group(2))


def _permute_hf_to_tune(w: torch.Tensor, n_heads: int, head_dim: int) -> torch.Tensor:
    """HF stores q/k projection rows per head as [first halves | second halves] (rotate-half RoPE); torchtune interleaves the
    pairs (x[2i], x[2i+1]): ``W.view(n, 2, hd/2, dim).transpose(1, 2).reshape(n*hd, dim)``."""
    dim = w.shape[1]
    return w.view(n_heads, 2, head_dim // 2, dim).transpose(1, 2).reshape(n_heads * head_dim, dim).contiguous()


def _permute_tune_to_hf(w: torch.Tensor, n_heads: int, head_dim: int) -> torch.Tensor:
    dim = w.shape[1]
    return w.view(n_heads, head_dim // 2, 2, dim).transpose(1, 2).reshape(n_heads * head_dim, dim).contiguous()


def hf_to_tune(state_dict: dict[str, torch.Tensor], num_heads: int, num_kv_heads: int, dim: int,
               head_dim: int | None = None, tie_word_embeddings: bool = True) -> dict[str, torch.Tensor]:
    head_dim = head_dim or dim // num_heads
    out: dict[str, torch.Tensor] = {}
    for key, value in state_dict.items():
        if "rotary_emb.inv_freq" in key:
            continue  # derived buffer, never a parameter
        if key == "lm_head.weight" and tie_word_embeddings:
            continue  # tied head: the embedding is the only copy (torchtune's Llama-3.2 builder has no output.weight)
        new_key = _map_key(key, _HF_TO_TUNE)
        if new_key.endswith("attn.q_proj.weight"):
            value = _permute_hf_to_tune(value, num_heads, head_dim)
        elif new_key.endswith("attn.k_proj.weight"):
            value = _permute_hf_to_tune(value, num_kv_heads, head_dim)
        out[new_key] = value
    return out


def tune_to_hf(state_dict: dict[str, torch.Tensor], num_heads: int, num_kv_heads: int, dim: int,
               head_dim: int | None = None) -> dict[str, torch.Tensor]:
    head_dim = head_dim or dim // num_heads
    out: dict[str, torch.Tensor] = {}
    for key, value in state_dict.items():
        new_key = _map_key(key, _TUNE_TO_HF)
        if key.endswith("attn.q_proj.weight"):
            value = _permute_tune_to_hf(value, num_heads, head_dim)
        elif key.endswith("attn.k_proj.weight"):
            value = _permute_tune_to_hf(value, num_kv_heads, head_dim)
        out[new_key] = value
    return out


def discover_safetensor_files(checkpoint_dir: Path) -> list[str]:
    """Sorted ``*.safetensors`` shard names of a directory; raises on none, or on both base (``model-*``) and fine-tuned
    (``ft-model-*``) shards (``/root/reference/ssi/checkpoint.py:53-90``)."""
    checkpoint_dir = Path(checkpoint_dir)
    if not checkpoint_dir.exists():
        raise FileNotFoundError(f"Checkpoint directory does not exist: {checkpoint_dir}")
    st_files = sorted(f.name for f in checkpoint_dir.glob("*.safetensors"))
    if not st_files:
        raise ValueError(f"No safetensors files found in {checkpoint_dir}. Directory contents: {sorted(f.name for f in checkpoint_dir.iterdir())}")
    if [f for f in st_files if f.startswith("model-")] and [f for f in st_files if f.startswith("ft-model-")]:
        raise ValueError(f"Ambiguous checkpoint files in {checkpoint_dir}: both base and fine-tuned shards present. "
                         f"Specify checkpoint_files explicitly to disambiguate.")
    return st_files


def validate_checkpoint_dir(checkpoint_dir: Path, config: dict[str, Any], expectations: Any | None = None) -> None:
    """Non-destructive checks of config.json against the model the trainer is about to build (layer count, hidden size, vocab
    size, shard count when the expectations object carries them); ``ValueError`` with the mismatch spelled out."""
    if expectations is None:
        return
    name = getattr(expectations, "model_name", "the model")
    checks = [("num_hidden_layers", getattr(expectations, "num_layers", None)), ("hidden_size", getattr(expectations, "hidden_size", None)),
              ("vocab_size", getattr(expectations, "vocab_size", None))]
    for key, want in checks:
        if want is not None and key in config and int(config[key]) != int(want):
            raise ValueError(f"{checkpoint_dir}/config.json has {key}={config[key]}, {name} expects {want}")
    n_shards = getattr(expectations, "n_shards", None)
    if n_shards is not None:
        found = len([f for f in Path(checkpoint_dir).glob("*.safetensors")])
        if found != int(n_shards):
            raise ValueError(f"{checkpoint_dir} holds {found} safetensors shard(s), {name} expects {n_shards}")


class FullModelHFCheckpointer(TuneCheckpointer):
    """HF-format Llama-3.2 checkpoints <-> the torchtune-key state dict the model exposes.  Same constructor keywords, methods
    and on-disk layout as the reference: sharded ``model-0000i-of-0000n.safetensors`` + ``model.safetensors.index.json`` in a
    self-contained ``step_N/`` directory (config / tokenizer files copied next to the weights), ``training_state.pt`` (schema
    v1) at the output root."""

    def __init__(self, checkpoint_dir, checkpoint_files: Any = None, *, config_json: Any = None, output_dir,
                 training_state_checkpoint: Any = None, safe_serialization: bool = True, model_expectations: Any = None, **_: Any) -> None:
        super().__init__(checkpoint_dir=str(checkpoint_dir), output_dir=str(output_dir),
                         training_state_checkpoint=str(training_state_checkpoint) if training_state_checkpoint is not None else None,
                         model_expectations=model_expectations)
        if not safe_serialization:
            raise ValueError("only safetensors serialization is supported (pickle-based .bin files are never written or read)")
        self._ckpt_dir, self._out_dir = Path(checkpoint_dir), Path(output_dir)
        if self._out_dir.resolve() == self._ckpt_dir.resolve() or self._ckpt_dir.resolve() in self._out_dir.resolve().parents:
            raise ValueError(f"output_dir {self._out_dir} must not lie inside checkpoint_dir {self._ckpt_dir}")
        self._out_dir.mkdir(parents=True, exist_ok=True)
        config_json = Path(config_json) if config_json is not None else self._ckpt_dir / LLAMA_3_2_CONFIG_RELPATH
        if not config_json.exists():
            raise FileNotFoundError(f"No config.json found at {config_json} — expected an HF-format model directory.")
        self._config = json.loads(config_json.read_text())
        if checkpoint_files is None:
            checkpoint_files = discover_safetensor_files(self._ckpt_dir)
        elif isinstance(checkpoint_files, dict) or (hasattr(checkpoint_files, "keys") and "filename_format" in checkpoint_files):
            n = int(checkpoint_files["max_filename"])
            checkpoint_files = [str(checkpoint_files["filename_format"]).format(str(i).zfill(len(str(checkpoint_files["max_filename"]))), checkpoint_files["max_filename"])
                                for i in range(1, n + 1)]
        validate_checkpoint_dir(self._ckpt_dir, self._config, model_expectations)
        self._checkpoint_paths = [self._ckpt_dir / str(f) for f in sorted(str(f) for f in checkpoint_files)]
        for p in self._checkpoint_paths:
            if not p.is_file():
                raise FileNotFoundError(f"checkpoint file {p} not found")
        self._weight_map: dict[str, str] | None = None

    def _conv_kwargs(self) -> dict[str, Any]:
        c = self._config
        return dict(num_heads=c["num_attention_heads"], num_kv_heads=c["num_key_value_heads"], dim=c["hidden_size"], head_dim=c.get("head_dim"))

    def load_checkpoint(self) -> dict[str, Any]:
        from safetensors.torch import load_file
        self._weight_map = {}
        merged: dict[str, torch.Tensor] = {}
        for idx, path in enumerate(self._checkpoint_paths):
            shard = load_file(str(path))
            for key, value in shard.items():
                if not isinstance(value, torch.Tensor):
                    raise ValueError(f"Expected all values in the state dict to be torch.Tensor. Found {type(value)} instead.")
                self._weight_map[key] = f"{idx + 1:04}"
            merged.update(shard)
            del shard
            gc.collect()
        out: dict[str, Any] = {MODEL_KEY: hf_to_tune(merged, **self._conv_kwargs(), tie_word_embeddings=self._config.get("tie_word_embeddings", True))}
        if self.training_state_checkpoint is not None:
            out.update(load_training_state(self.training_state_checkpoint))
        return out

    def save_full_model(self, state_dict: dict[str, Any], output_dir: Path) -> None:
        from safetensors.torch import save_file
        if self._weight_map is None:
            raise ValueError("Weight map is not initialized. Please load a checkpoint before saving.")
        hf_sd = tune_to_hf(state_dict[MODEL_KEY], **self._conv_kwargs())
        split: dict[str, dict[str, torch.Tensor]] = {}
        total_size = 0
        for key, weight in hf_sd.items():
            shard_id = self._weight_map.get(key, "0001")
            split.setdefault(shard_id, {})[key] = weight.detach().to("cpu").contiguous()
            total_size += weight.numel() * weight.element_size()
        output_dir = Path(output_dir)
        output_dir.mkdir(parents=True, exist_ok=True)
        names = {}
        for shard_id, sd in split.items():
            names[shard_id] = SHARD_FNAME.format(cpt_idx=f"{shard_id}".zfill(5), num_shards=f"{len(split)}".zfill(5)) + ".safetensors"
            save_file(sd, str(output_dir / names[shard_id]), metadata={"format": "pt"})
        weight_map = {k: names[self._weight_map.get(k, "0001")] for k in hf_sd}
        (output_dir / SAFETENSOR_INDEX_FNAME).write_text(json.dumps({"metadata": {"total_size": total_size}, "weight_map": weight_map}, indent=2))

    def save_model_checkpoint(self, model_state_dict: dict[str, torch.Tensor], global_step: int, *, output_dir: Any = None,
                              ignore_suffixes: Any = None) -> Path:
        output_dir = Path(output_dir) if output_dir is not None else self._out_dir / f"step_{global_step}"
        self.save_full_model({MODEL_KEY: model_state_dict}, output_dir)
        skip = tuple(ignore_suffixes) if ignore_suffixes is not None else (*SUFFIXES_TO_NOT_COPY, "torchtune_config.yaml")
        for f in self._ckpt_dir.iterdir():  # config, tokenizer, generation config ...: the directory is usable by HF tooling
            if f.is_file() and not f.name.endswith(skip):
                shutil.copy2(f, output_dir / f.name)
        return output_dir

    def _save_ema_model(self, model_state_dict: dict[str, torch.Tensor], global_step: int) -> str:
        return str(self.save_model_checkpoint(model_state_dict, global_step, output_dir=self._out_dir / f"step_{global_step}" / "ema"))


def make_checkpointer(**kwargs: Any):
    """HF-format checkpointer when ``checkpoint_dir`` is an HF model directory (has config.json); the single-file torchtune-key
    checkpointer when it holds a ``model.safetensors`` this trainer wrote, or when ``allow_random_init`` is set explicitly (seeded
    random weights: the build and GPU images hold no Llama weights).  Anything else is an error at load time, as in the reference
    (``/root/reference/ssi/checkpoint.py:263-264``) — a wrong path never silently trains from noise."""
    d = kwargs.get("checkpoint_dir")
    if d and (Path(str(d)) / LLAMA_3_2_CONFIG_RELPATH).exists():
        kwargs.pop("allow_random_init", None)
        return FullModelHFCheckpointer(**kwargs)
    return TuneCheckpointer(**kwargs)
