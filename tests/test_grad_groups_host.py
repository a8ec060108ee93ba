"""CPU: ``grad_groups`` rules -> the group table of the flat gradient buffer and the refined AdamW segments (``ssi/grad_groups.py``), on the
stand-in layout of ``tests/test_param_groups_host.py``, plus the config plumbing."""
import os

import pytest

from conftest import ROOT
from test_param_groups_host import D, EMB, LAYOUT, TOTAL, TYPES, VPAD

PKG = os.path.join(ROOT, "speech-integration_amd")
EXAMPLE = [{"name": "new_rows", "params": [EMB], "token_types": ["dsu", "modality"]}, {"name": "embedding", "params": [EMB]},
           {"name": "norms", "params": ["*.scale"]}]
STAGE1 = [{"params": [EMB], "token_types": ["dsu", "modality"]}, {"params": ["*"], "frozen": True}]


def _table(rules, segments=None, types=TYPES):
    from ssi.grad_groups import resolve_groups
    return resolve_groups(rules, LAYOUT, TOTAL, types, segments)


def _segments(rules):
    from ssi.param_groups import resolve
    return resolve(rules, LAYOUT, TOTAL, TYPES)


def _ranges(table):
    names, ends, groups = table
    out, start = {}, 0
    for e, g in zip(ends, groups):
        out.setdefault(names[g] if g >= 0 else None, []).append((start, e))
        start = e
    return out


def _well_formed(table):
    names, ends, groups = table
    assert ends[-1] == TOTAL and all(a < b for a, b in zip(ends, ends[1:])) and all(e % 8 == 0 for e in ends[:-1])
    assert all(-1 <= g < len(names) for g in groups) and all(a != b for a, b in zip(groups, groups[1:]))   # merged
    assert {g for g in groups if g >= 0} == set(range(len(names)))                                         # every group has elements


def test_the_example_resolves_to_the_expected_ranges():
    table = _table(EXAMPLE)
    _well_formed(table)
    assert table[0] == ["new_rows", "embedding", "norms", "other"]
    r = _ranges(table)
    # rows 80..95 (dsu) and 98..99 (modality); the padding rows 100..127 join the modality rows in front of them
    assert r["new_rows"] == [(80 * D, 96 * D), (98 * D, VPAD * D)]
    assert r["embedding"] == [(0, 80 * D), (96 * D, 98 * D)]
    scales = sorted((off, off + cols) for n, (off, rows, cols) in LAYOUT.items() if n.endswith(".scale"))
    merged = []
    for a, b in scales:
        if merged and merged[-1][1] == a:
            merged[-1] = (merged[-1][0], b)
        else:
            merged.append((a, b))
    assert r["norms"] == merged
    covered = sorted(x for v in r.values() for x in v)
    assert covered[0][0] == 0 and covered[-1][1] == TOTAL and all(a[1] == b[0] for a, b in zip(covered, covered[1:]))   # exactly one group each


def test_first_match_wins_and_row_ranges_of_fused_weights():
    table = _table([{"name": "q", "params": ["*.q_proj.weight"]}, {"name": "attn", "params": ["*.attn.*"]}, {"name": "w1", "params": ["*.mlp.w1.weight"]}])
    _well_formed(table)
    r = _ranges(table)
    for l in range(2):
        off, rows, cols = LAYOUT[f"layers.{l}.attn.q_proj.weight"]
        assert (off, off + rows * cols) in r["q"]
        off, rows, cols = LAYOUT[f"layers.{l}.mlp.w1.weight"]
        assert (off, off + rows * cols) in r["w1"]
    k = LAYOUT["layers.0.attn.k_proj.weight"]
    assert any(a <= k[0] < b for a, b in r["attn"]) and not any(a <= LAYOUT["layers.0.attn.q_proj.weight"][0] < b for a, b in r["attn"])
    assert "other" in r


def test_no_other_when_the_rules_take_everything():
    table = _table([{"name": "emb", "params": [EMB]}, {"name": "rest", "params": ["*"]}])
    assert table[0] == ["emb", "rest"] and table[1] == [VPAD * D, TOTAL] and table[2] == [0, 1]


def test_frozen_ranges_get_minus_one():
    segs = _segments(STAGE1)
    table = _table([{"name": "new_rows", "params": [EMB], "token_types": ["dsu", "modality"]}], segs)
    _well_formed(table)
    assert table[0] == ["new_rows"]                     # "other" would be all frozen: it is not a group
    assert table[1] == [80 * D, 96 * D, 98 * D, VPAD * D, TOTAL] and table[2] == [-1, 0, -1, 0, -1]
    # only some of a group frozen: the rest of it stays
    segs = _segments([{"params": ["layers.0.*"], "frozen": True}])
    table = _table([{"name": "norms", "params": ["*.scale"]}], segs)
    r = _ranges(table)
    off = LAYOUT["layers.0.sa_norm.scale"][0]
    assert any(a <= off < b for a, b in r[None]) and all(not (a <= off < b) for a, b in r["norms"]) and r["norms"] and r["other"]


def test_refine_against_hand_written_tables():
    from ssi.grad_groups import refine
    from ssi.param_groups import Segment
    table = (["a", "b"], [64, 128, 256], [0, 1, 0])
    assert refine(None, table) == [(Segment(0, 64), 0), (Segment(64, 128), 1), (Segment(128, 256), 0)]
    segs = [Segment(0, 32, 2.0, 0.0, False), Segment(32, 160, 1.0, None, False), Segment(160, 256, 0.5, None, False)]
    assert refine(segs, table) == [(Segment(0, 32, 2.0, 0.0, False), 0), (Segment(32, 64, 1.0, None, False), 0), (Segment(64, 128, 1.0, None, False), 1),
                                   (Segment(128, 160, 1.0, None, False), 0), (Segment(160, 256, 0.5, None, False), 0)]
    frozen = [Segment(0, 64, frozen=True), Segment(64, 256)]
    assert refine(frozen, (["a"], [64, 256], [-1, 0])) == [(Segment(0, 64, frozen=True), -1), (Segment(64, 256), 0)]
    with pytest.raises(ValueError):
        refine(frozen, (["a"], [256], [0]))             # a frozen segment inside a group
    with pytest.raises(ValueError):
        refine([Segment(0, 128)], table)                # another buffer


@pytest.mark.parametrize("rules,segments,needle", [
    ([{"name": "a", "params": [EMB], "lr_scale": 2.0}], None, "unknown keys"),
    ([{"name": "a", "params": [EMB]}, {"name": "a", "params": ["*"]}], None, "duplicate"),
    ([{"name": "", "params": [EMB]}], None, "name"),
    ([{"params": [EMB]}], None, "name"),
    ([{"name": "other", "params": [EMB]}], None, "reserved"),
    ([{"name": "a", "params": ["no.such.*"]}], None, "no parameter matches"),
    ([{"name": "a", "params": [EMB], "token_types": ["nope"]}], None, "unknown token type"),
    ([{"name": "a", "params": [EMB], "max_norm": -1.0}], None, "max_norm"),
    ([{"name": f"g{k}", "params": [EMB]} for k in range(64)], None, "more than"),
    ([{"name": "a", "params": ["layers.0.*"]}], "freeze_layer0", "frozen"),
    ([{"name": "a", "params": ["*"]}, {"name": "late", "params": [EMB]}], None, "no element is left"),
    ([], None, "non-empty"),
])
def test_every_problem_is_a_value_error_naming_the_rule(rules, segments, needle):
    segs = _segments([{"params": ["layers.0.*"], "frozen": True}]) if segments else None
    with pytest.raises(ValueError) as e:
        _table(rules, segs)
    msg = str(e.value)
    assert needle in msg and "grad_groups" in msg and "param_groups rule" not in msg
    if rules and "name" in rules[-1] and rules[-1]["name"] and needle not in ("more than",):
        assert "rule" in msg


def test_validate_train_cfg_accepts_and_refuses():
    from ssi.config import OmegaConf, compose
    from ssi.train_utils import validate_train_cfg
    assert compose(os.path.join(PKG, "conf"), "sft", ["data=sft/mls-speechtokenizer-rvq_0"]).grad_groups is None   # the default
    cfg = OmegaConf.create({"speech": {"n_dsus": 5000}, "dtype": "bf16", "gradient_accumulation_steps": 1, "max_steps": 1, "log_interval": 1,
                            "eval_steps": 2, "save_steps": 4, "grad_groups": None})
    validate_train_cfg(cfg)
    for clip in (None, {"max_norm": 1.0}, {"adaptive": {"rel": 1.05, "beta": 0.98, "warmup_steps": 100}, "max_norm": 1.0}, {"adaptive": {}}):
        cfg.grad_groups = {"groups": EXAMPLE, "clip": clip}
        validate_train_cfg(cfg)
    for bad in ([{"name": "a", "params": [EMB]}], {"clip": None}, {"groups": []}, {"groups": EXAMPLE, "clip": {}}, {"groups": EXAMPLE, "clip": {"max_norm": 0}},
                {"groups": EXAMPLE, "clip": {"adaptive": {"beta": 1.0}}}, {"groups": EXAMPLE, "clip": {"adaptive": {"warmup_steps": -1}}},
                {"groups": EXAMPLE, "clip": {"threshold": 1.0}}, {"groups": EXAMPLE, "norm": True}, {"groups": [{"name": "other", "params": ["*"]}]}):
        cfg.grad_groups = bad
        with pytest.raises(ValueError):
            validate_train_cfg(cfg)


def test_grad_groups_object_and_the_rules_own_threshold():
    import math
    from ssi.grad_groups import GradGroups
    node = {"groups": [dict(EXAMPLE[0], max_norm=0.5), EXAMPLE[1], dict(EXAMPLE[2], max_norm=None)], "clip": {"max_norm": 1.0}}
    gg = GradGroups.from_config(node, LAYOUT, TOTAL, TYPES)
    assert gg.names == ["new_rows", "embedding", "norms", "other"] and gg.n_groups == 4
    assert gg.clip.max_norm.tolist() == [0.5, 1.0, math.inf, 1.0] and gg.clip.adaptive is None
    assert [s.end for s, _ in gg.refined] == gg.seg_end and [g for _, g in gg.refined] == gg.seg_group
    logged = GradGroups.from_config({"groups": EXAMPLE, "clip": None}, LAYOUT, TOTAL, TYPES)
    assert logged.clip is None
    with pytest.raises(ValueError):
        GradGroups.from_config({"groups": [dict(EXAMPLE[0], max_norm=0.5)], "clip": None}, LAYOUT, TOTAL, TYPES)


def test_null_adds_nothing_to_the_optimizer():
    """Without the key ``setup_optimizer`` builds the optimizer it always built: no argument of the new kind reaches it."""
    import inspect
    from ssi import optimizer
    assert inspect.signature(optimizer.HipAdamW.__init__).parameters["grad_groups"].default is None
    seen = {}

    class Stub:
        def __init__(self, params, **kw):
            seen.update(kw)

        def load_state_dict(self, sd):
            pass

    class Model:
        _flat = None

        def parameters(self):
            return []

    class Cfg(dict):
        optimizer = {"lr": 1e-3}
    real = optimizer.HipAdamW
    optimizer.HipAdamW = Stub
    try:
        optimizer.setup_optimizer(Cfg(), Model())
    finally:
        optimizer.HipAdamW = real
    assert seen["grad_groups"] is None and "param_segments" not in seen
