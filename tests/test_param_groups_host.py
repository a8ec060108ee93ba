"""CPU: ``param_groups`` rules -> segments of the flat parameter buffer (``ssi/param_groups.py``), on a stand-in layout of the decoder's shape
(2 layers; the embedding first with padding rows behind it, then the attention weights, then the MLP blocks and norm scales, then the final
norm — ``HipLlamaDecoder``'s order), plus the config plumbing and the ABI version."""
import os
import re

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "speech-integration_amd")
V, VPAD, D, Q, KVD, I, L = 100, 128, 16, 16, 8, 32, 2
EMB = "tok_embeddings.weight"
TYPES = {"text": (0, 79), "dsu": (80, 95), "special_text": (96, 97), "modality": (98, 99)}   # inclusive, as get_token_type_ranges gives them


def _layout():
    lay, off = {}, 0
    lay[EMB] = (0, V, D)
    off = VPAD * D
    for l in range(L):
        for nm, rows in (("q_proj", Q), ("k_proj", KVD), ("v_proj", KVD)):
            lay[f"layers.{l}.attn.{nm}.weight"] = (off, rows, D)
            off += rows * D
        lay[f"layers.{l}.attn.output_proj.weight"] = (off, D, Q)
        off += D * Q
    for l in range(L):
        lay[f"layers.{l}.mlp.w1.weight"] = (off, I, D)
        lay[f"layers.{l}.mlp.w3.weight"] = (off + I * D, I, D)
        off += 2 * I * D
        lay[f"layers.{l}.mlp.w2.weight"] = (off, D, I)
        off += D * I
        for nm in ("sa_norm", "mlp_norm"):
            lay[f"layers.{l}.{nm}.scale"] = (off, 1, D)
            off += D
    lay["norm.scale"] = (off, 1, D)
    return lay, off + D


LAYOUT, TOTAL = _layout()


def _resolve(rules, types=TYPES):
    from ssi.param_groups import resolve
    return resolve(rules, LAYOUT, TOTAL, types)


def _at(segs, elem):
    return next(s for s in segs if s.start <= elem < s.end)


def _covers(segs):
    assert segs[0].start == 0 and segs[-1].end == TOTAL
    assert all(a.end == b.start for a, b in zip(segs, segs[1:])) and all(s.end > s.start for s in segs)
    assert all(s.start % 8 == 0 for s in segs)                       # a 16-byte vector lies in one segment
    assert all(a.setting != b.setting for a, b in zip(segs, segs[1:]))   # merged


def test_stage_one_rules_token_type_rows_and_padding():
    segs = _resolve([{"params": [EMB], "token_types": ["dsu", "modality"]}, {"params": ["*"], "frozen": True}])
    _covers(segs)
    # rows 80..95 and 98..99 trainable; 0..79, 96..97 frozen; the padding rows 100..127 join the modality rows in front of them
    assert [(s.start, s.end, s.frozen) for s in segs] == [(0, 80 * D, True), (80 * D, 96 * D, False), (96 * D, 98 * D, True),
                                                         (98 * D, VPAD * D, False), (VPAD * D, TOTAL, True)]
    assert all(s.lr_scale == 1.0 and s.weight_decay is None for s in segs if not s.frozen)


def test_first_match_wins_and_unmatched_keeps_the_defaults():
    segs = _resolve([{"params": ["layers.0.*"], "lr_scale": 0.5}, {"params": ["layers.*"], "lr_scale": 2.0, "weight_decay": 0.0}])
    _covers(segs)
    q0, q1 = LAYOUT["layers.0.attn.q_proj.weight"][0], LAYOUT["layers.1.attn.q_proj.weight"][0]
    assert _at(segs, q0).lr_scale == 0.5 and _at(segs, q0).weight_decay is None
    assert _at(segs, q1).lr_scale == 2.0 and _at(segs, q1).weight_decay == 0.0
    emb, norm = _at(segs, 0), _at(segs, TOTAL - 1)
    assert (emb.lr_scale, emb.weight_decay, emb.frozen) == (1.0, None, False) == (norm.lr_scale, norm.weight_decay, norm.frozen)
    # a rule with token types in front of a rule for the whole embedding: the rows it names are its own, the rest the second rule's
    segs = _resolve([{"params": [EMB], "token_types": ["dsu"], "lr_scale": 4.0}, {"params": [EMB], "weight_decay": 0.0}])
    assert _at(segs, 80 * D).lr_scale == 4.0 and _at(segs, 80 * D).weight_decay is None
    assert _at(segs, 0).weight_decay == 0.0 and _at(segs, 97 * D).weight_decay == 0.0 and _at(segs, VPAD * D).weight_decay is None


def test_fused_weights_resolve_to_row_ranges():
    segs = _resolve([{"params": ["*.k_proj.weight"], "frozen": True}, {"params": ["*.mlp.w3.weight"], "lr_scale": 3.0}])
    _covers(segs)
    for l in range(L):
        k_off, k_rows, _ = LAYOUT[f"layers.{l}.attn.k_proj.weight"]
        s = _at(segs, k_off)
        assert (s.start, s.end, s.frozen) == (k_off, k_off + k_rows * D, True)          # q in front and v behind are not frozen
        w3 = LAYOUT[f"layers.{l}.mlp.w3.weight"][0]
        s = _at(segs, w3)
        assert (s.start, s.end, s.lr_scale) == (w3, w3 + I * D, 3.0) and _at(segs, w3 - 1).lr_scale == 1.0


def test_no_decay_on_norm_scales_merges_adjacent_ranges():
    segs = _resolve([{"params": ["*.scale"], "weight_decay": 0.0}])
    _covers(segs)
    # per layer sa_norm and mlp_norm lie side by side: one range; the last layer's pair and the final norm too
    assert sum(1 for s in segs if s.weight_decay == 0.0) == L
    last = segs[-1]
    assert last.weight_decay == 0.0 and last.end - last.start == 3 * D
    assert len(_resolve([{"params": ["*"], "lr_scale": 1.0}])) == 1                     # a rule that says the default: everything merges


@pytest.mark.parametrize("rules, needle", [
    ([{"params": ["*"], "lr": 1.0}], "unknown keys"),
    ([{"params": ["layers.7.*"]}], "no parameter matches"),
    ([{"params": ["*.weight"], "token_types": ["dsu"]}], "token_types"),
    ([{"params": [EMB], "token_types": ["phoneme"]}], "unknown token type"),
    ([{"params": ["*"], "lr_scale": float("nan")}], "lr_scale"),
    ([{"params": ["*"], "lr_scale": -1.0}], "lr_scale"),
    ([{"params": ["*"], "weight_decay": float("inf")}], "weight_decay"),
    ([{"params": ["*"], "weight_decay": -0.1}], "weight_decay"),
    ([{"frozen": True}], "params"),
])
def test_bad_rules_are_value_errors_naming_the_rule(rules, needle):
    with pytest.raises(ValueError) as e:
        _resolve(rules)
    assert needle in str(e.value) and "rule 0" in str(e.value)


def test_helpers_clip_and_trainable_ranges():
    from ssi.param_groups import Segment, check_segments, clip, trainable_ranges
    segs = [Segment(0, 64, frozen=True), Segment(64, 128), Segment(128, 256, lr_scale=2.0), Segment(256, 300, frozen=True)]
    assert check_segments(segs, 300) == segs
    assert trainable_ranges(segs) == [(64, 256)]
    assert [(s.start, s.end) for s in clip(segs, 32, 130)] == [(32, 64), (64, 128), (128, 130)]
    with pytest.raises(ValueError):
        check_segments(segs, 301)
    with pytest.raises(ValueError):
        check_segments([Segment(0, 12), Segment(12, 300)], 300)


def test_validate_train_cfg_checks_the_shape_of_param_groups():
    from ssi.config import OmegaConf, compose
    from ssi.train_utils import validate_train_cfg
    base = {"speech": {"n_dsus": 5000}, "dtype": "bf16", "gradient_accumulation_steps": 1, "max_steps": 1, "log_interval": 1, "eval_steps": 2,
            "save_steps": 4}
    validate_train_cfg(OmegaConf.create(base))                                           # absent: off
    validate_train_cfg(OmegaConf.create({**base, "param_groups": None}))
    validate_train_cfg(OmegaConf.create({**base, "param_groups": [{"params": ["*"], "frozen": True}]}))
    for bad in ("all", [], {"params": ["*"]}, ["*.scale"]):
        with pytest.raises(ValueError, match="param_groups"):
            validate_train_cfg(OmegaConf.create({**base, "param_groups": bad}))
    cfg = compose(os.path.join(PKG, "conf"), "sft", ["data=sft/mls-hubert_large_ll60k-layer_22"])
    assert cfg.param_groups is None
    # the rules of a composed config are mappings the resolver reads as they are
    cfg.param_groups = [{"params": [EMB], "token_types": ["dsu"], "lr_scale": 2}, {"params": ["*"], "frozen": True}]
    segs = _resolve(cfg.param_groups)
    assert [s.frozen for s in segs] == [True, False, True] and segs[1].lr_scale == 2.0


def test_training_yaml_has_the_key_with_default_null():
    line = next(l for l in open(os.path.join(PKG, "conf", "training.yaml")) if l.startswith("param_groups:"))
    assert line.split("#")[0].split(":", 1)[1].strip() == "null" and "# not in the reference:" in line


def test_abi_version_and_symbol():
    from ssi import _lib, ops
    text = open(os.path.join(ROOT, "include", "ssi_hip.h")).read()
    assert _lib.ABI_VERSION >= 16 and re.search(r"#define SSI_ABI_VERSION (\d+)", text).group(1) == str(_lib.ABI_VERSION)
    assert "ssi_adamw_step_seg" in _lib.PROTOTYPES and re.search(r"#define SSI_ADAMW_MAX_SEGS (\d+)", text).group(1) == str(_lib.ADAMW_MAX_SEGS)
    assert "adamw_step_seg" in ops.__all__ and callable(ops.adamw_step_seg)
