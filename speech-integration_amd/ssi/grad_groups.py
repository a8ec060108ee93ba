"""Gradient groups: per-group gradient norms of the flat gradient buffer, and optionally a clip per group (not in the reference; config key
``grad_groups``, default null).

The missing half of ``param_groups``: the same rule language names GROUPS of the flat buffer — the new rows of the tied embedding against its
pretrained rows, the norm scales, the attention weights — and every optimizer step ONE HIP pass (``ssi_sumsq_groups``) yields each group's sum of
squares.  The norms are logged per group; with ``clip`` every group is clipped on its own, to a fixed threshold or adaptively against a running
average of its own norm, and the coefficient rides into the one-launch AdamW as a per-segment DEVICE scale (``ssi_adamw_step_seg_gscale``): the
host reads nothing back to decide anything.  ::

    grad_groups:
      groups:                     # param_groups' matching (params, token_types) plus a unique `name`; the first matching rule wins
        - {name: new_rows,  params: [tok_embeddings.weight], token_types: [dsu, modality]}
        - {name: embedding, params: [tok_embeddings.weight]}
        - {name: norms,     params: ["*.scale"]}
        # what no rule matches forms the group "other"
      clip: null                  # null: the norms are only logged
      # clip: {max_norm: 1.0}     # every group clipped to max_norm; a rule's own `max_norm` (a number, or null = never) overrides
      # clip: {adaptive: {rel: 1.05, beta: 0.98, warmup_steps: 100}, max_norm: 1.0}

Resolution reuses ``param_groups.resolve``: ``q_proj`` / ``w1`` resolve to their row ranges of the fused weights, padding rows and gaps join the
segment in front of them, every boundary is a multiple of 8 elements.  Every element belongs to exactly one group; the elements of a frozen
``param_groups`` segment belong to none (group -1: their gradient memory is unspecified and is not read).

THE CLIP RULE (AdaGC's idea, arXiv:2502.11034; this definition is the contract, restated in ``tests/grad_groups_ref.py``).  Per optimizer step
``t`` = 1, 2, ... of the applied windows and per group ``g``: let ``n = sqrt(sumsq[g]) * |pending scale|`` — the norm of the group's gradient
as AdamW would see it, after ``scale_grads`` and after the global clip if ``clip_grad_norm`` is set — and ``m`` the group's ``max_norm``, or +inf.

* ``n`` not finite: the group is skipped this step — its coefficient is NaN, so the kernel leaves its segments alone; ``gamma`` stays,
  ``skipped[g] += 1``.
* ``gamma`` unset, or fixed mode, or ``t <= warmup_steps``: ``c = min(1, m / (n + 1e-6))``; in adaptive mode with ``n > 0``:
  ``gamma = min(gamma, c n)``, an unset ``gamma`` takes the value ``c n``.
* otherwise: ``c = min(1, min(m, rel gamma) / (n + 1e-6))`` and ``gamma = beta gamma + (1 - beta) c n``.

``gamma`` is unset until the group's first finite non-zero norm.  Every segment of group ``g`` is scaled by ``c[g]``.  All of it is torch ops on
``[n_groups]`` fp32 tensors where the sums live; only ``t`` is a host number."""

from __future__ import annotations

import math
from typing import Any, Mapping, Optional, Sequence

import torch
from torch import Tensor

from . import param_groups as pg
from ._lib import SUMSQ_MAX_GROUPS, SUMSQ_MAX_SEGS
from .param_groups import Segment

RULE_KEYS = ("name", "params", "token_types", "max_norm")
CONFIG_KEYS = ("groups", "clip")
CLIP_KEYS = ("max_norm", "adaptive")
ADAPTIVE_KEYS = ("rel", "beta", "warmup_steps")
OTHER = "other"
_UNSET = object()

GroupTable = tuple  # (names, seg_end, seg_group)


def _plain(node: Any) -> Any:
    """Config nodes as plain containers."""
    if hasattr(node, "keys"):
        return {str(k): _plain(node[k]) for k in node.keys()}
    if isinstance(node, (list, tuple)) or (hasattr(node, "__len__") and hasattr(node, "__getitem__") and not isinstance(node, (str, bytes))):
        return [_plain(v) for v in node]
    return node


def _threshold(what: str, value: Any) -> float:
    """A ``max_norm``: a finite number > 0, or null = never clipped."""
    if value is None:
        return math.inf
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or value <= 0:
        raise ValueError(f"grad_groups {what}: 'max_norm' must be null or a finite number > 0, got {value!r}")
    return float(value)


def _check_rules(rules: Any) -> list[dict]:
    if rules is None or isinstance(rules, (str, bytes)) or hasattr(rules, "keys") or not hasattr(rules, "__len__") or len(rules) == 0:
        raise ValueError(f"grad_groups: 'groups' must be a non-empty list of rules, got {rules!r}")
    out, seen = [], set()
    for i, rule in enumerate(rules):
        what = f"rule {i}"
        if not hasattr(rule, "keys"):
            raise ValueError(f"grad_groups {what}: a rule is a mapping, got {rule!r}")
        rule = _plain(rule)
        name = rule.get("name")
        if not isinstance(name, str) or not name.strip():
            raise ValueError(f"grad_groups {what}: 'name' must be a non-empty string, got {name!r}")
        what = f"rule {i} (name={name!r})"
        unknown = sorted(k for k in rule if k not in RULE_KEYS)
        if unknown:
            raise ValueError(f"grad_groups {what}: unknown keys {unknown} (known: {list(RULE_KEYS)})")
        if name == OTHER:
            raise ValueError(f"grad_groups {what}: the name {OTHER!r} is reserved for what no rule matches")
        if name in seen:
            raise ValueError(f"grad_groups {what}: duplicate name")
        seen.add(name)
        if "max_norm" in rule:
            _threshold(what, rule["max_norm"])
        out.append(rule)
    if len(out) + 1 > SUMSQ_MAX_GROUPS:
        raise ValueError(f"grad_groups: {len(out)} rules and {OTHER!r} are more than the {SUMSQ_MAX_GROUPS} groups one pass sums (rule {SUMSQ_MAX_GROUPS - 1}, "
                         f"name={out[SUMSQ_MAX_GROUPS - 1]['name']!r}, is one too many)")
    return out


def resolve_groups(rules: Sequence[Mapping], layout: pg.Layout, total: int, token_type_ranges: Optional[Mapping[str, tuple[int, int]]] = None,
                   param_segments: Optional[Sequence[Segment]] = None) -> GroupTable:
    """``(names, seg_end, seg_group)``: consecutive segments covering ``[0, total)`` (``seg_end`` ascending, multiples of 8 but the last) with
    the index into ``names`` of each one's group, or -1 where ``param_segments`` freezes.  Adjacent segments of one group are merged.  ``names``
    are the rules' in their order, then ``"other"`` if an unfrozen element matches no rule.  Every problem is a ``ValueError`` naming the rule."""
    rules = _check_rules(rules)
    # param_groups' resolution, with the rule's index carried as the segment's label (its lr_scale: segments of different rules never merge)
    labelled = [{"params": r.get("params"), "lr_scale": float(i + 2), **({"token_types": r["token_types"]} if r.get("token_types") is not None else {})}
                for i, r in enumerate(rules)]
    try:
        segs = pg.resolve(labelled, layout, total, token_type_ranges)
    except ValueError as e:
        msg = str(e).replace("param_groups", "grad_groups")
        for i, r in enumerate(rules):
            msg = msg.replace(f"rule {i} (params=", f"rule {i} (name={r['name']!r}, params=").replace(f"grad_groups rule {i}:", f"grad_groups rule {i} (name={r['name']!r}):")
        raise ValueError(msg) from None
    cuts = sorted({0, int(total)} | {s.end for s in segs} | {s.end for s in (param_segments or ())})
    frozen = [(s.start, s.end) for s in (param_segments or ()) if s.frozen]
    pieces: list[tuple[int, int]] = []   # (end, label), label: rule index, len(rules) for what no rule matches, -1 frozen
    for a, b in zip(cuts, cuts[1:]):
        if any(lo <= a and b <= hi for lo, hi in frozen):
            label = -1
        else:
            s = next(s for s in segs if s.start <= a and b <= s.end)
            label = int(s.lr_scale) - 2 if s.lr_scale != 1.0 else len(rules)
        if pieces and pieces[-1][1] == label:
            pieces[-1] = (b, label)
        else:
            pieces.append((b, label))
    live = {label for _, label in pieces}
    for i, r in enumerate(rules):
        if i not in live:   # (resolve has already refused a rule that matches no parameter at all)
            matched_any = any(int(s.lr_scale) - 2 == i for s in segs)
            raise ValueError(f"grad_groups rule {i} (name={r['name']!r}): " + ("every element of the group is frozen by param_groups" if matched_any
                             else "no element is left for the group: the rules before it take everything it matches"))
    names = [r["name"] for r in rules] + ([OTHER] if len(rules) in live else [])
    if len(pieces) > SUMSQ_MAX_SEGS:
        raise ValueError(f"grad_groups: the rules cut the flat buffer into {len(pieces)} segments, one pass takes {SUMSQ_MAX_SEGS}")
    for end, _ in pieces[:-1]:
        if end % 8:
            raise ValueError(f"grad_groups: a segment ends at element {end}, not a multiple of 8 (16-byte vectors must lie in one segment)")
    return names, [end for end, _ in pieces], [label for _, label in pieces]


def refine(param_segments: Optional[Sequence[Segment]], table: GroupTable) -> list[tuple[Segment, int]]:
    """The AdamW segments split at the group boundaries, each with its group index (-1: frozen): what ``HipAdamW._update`` launches over under
    a clip rule.  Without ``param_segments`` every segment runs at lr scale 1 with the optimizer's decay."""
    _, seg_end, seg_group = table
    total = int(seg_end[-1])
    base = list(param_segments) if param_segments is not None else [Segment(0, total)]
    if base[0].start != 0 or base[-1].end != total:
        raise ValueError(f"refine: the parameter segments cover [{base[0].start}, {base[-1].end}), the group table [0, {total})")
    out: list[tuple[Segment, int]] = []
    start = 0
    for end, group in zip(seg_end, seg_group):
        for s in pg.clip(base, start, int(end)):
            if s.frozen != (group < 0):
                raise ValueError(f"refine: [{s.start}, {s.end}) is {'frozen' if s.frozen else 'trainable'} but its group is {group}")
            out.append((s, int(group)))
        start = int(end)
    return out


def _check_clip(clip: Any) -> Optional[dict]:
    """``clip`` of the config as ``{"max_norm": float (inf = never), "adaptive": None | {"rel", "beta", "warmup_steps"}}``, or None."""
    if clip is None:
        return None
    if not hasattr(clip, "keys"):
        raise ValueError(f"grad_groups: 'clip' must be null or a mapping, got {clip!r}")
    clip = _plain(clip)
    unknown = sorted(k for k in clip if k not in CLIP_KEYS)
    if unknown:
        raise ValueError(f"grad_groups clip: unknown keys {unknown} (known: {list(CLIP_KEYS)})")
    out = {"max_norm": _threshold("clip", clip.get("max_norm")), "adaptive": None}
    a = clip.get("adaptive")
    if a is not None:
        if not hasattr(a, "keys"):
            raise ValueError(f"grad_groups clip: 'adaptive' must be null or a mapping, got {a!r}")
        unknown = sorted(k for k in a if k not in ADAPTIVE_KEYS)
        if unknown:
            raise ValueError(f"grad_groups clip.adaptive: unknown keys {unknown} (known: {list(ADAPTIVE_KEYS)})")
        rel, beta, warm = a.get("rel", 1.05), a.get("beta", 0.98), a.get("warmup_steps", 100)
        if isinstance(rel, bool) or not isinstance(rel, (int, float)) or not math.isfinite(rel) or rel <= 0:
            raise ValueError(f"grad_groups clip.adaptive: 'rel' must be a finite number > 0, got {rel!r}")
        if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not 0 <= beta < 1:
            raise ValueError(f"grad_groups clip.adaptive: 'beta' must be a number in [0, 1), got {beta!r}")
        if isinstance(warm, bool) or not isinstance(warm, int) or warm < 0:
            raise ValueError(f"grad_groups clip.adaptive: 'warmup_steps' must be an integer >= 0, got {warm!r}")
        out["adaptive"] = {"rel": float(rel), "beta": float(beta), "warmup_steps": int(warm)}
    elif "max_norm" not in clip:
        raise ValueError("grad_groups clip: needs 'max_norm', 'adaptive' or both")
    return out


def check_config(node: Any) -> Optional[dict]:
    """The ``grad_groups`` config value as plain containers after the checks that need no model: ``{"groups": [...], "clip": None | {...}}``."""
    if node is None:
        return None
    if not hasattr(node, "keys"):
        raise ValueError(f"config field 'grad_groups' must be null or a mapping with 'groups' (and 'clip'), got {node!r}")
    node = _plain(node)
    unknown = sorted(k for k in node if k not in CONFIG_KEYS)
    if unknown:
        raise ValueError(f"grad_groups: unknown keys {unknown} (known: {list(CONFIG_KEYS)})")
    return {"groups": _check_rules(node.get("groups")), "clip": _check_clip(node.get("clip"))}


class GroupClip:
    """The clip rule of the module docstring and its state: ``gamma``, ``has_gamma`` and ``skipped`` are fp32 ``[n_groups]`` tensors on
    ``device``, ``t`` counts the applied windows.  ``update`` is torch ops only: nothing is read back, no Python branch looks at a device value."""

    def __init__(self, names: Sequence[str], max_norm: Sequence[float], adaptive: Optional[Mapping] = None, device="cpu"):
        self.names = list(names)
        n = len(self.names)
        assert len(max_norm) == n
        self.adaptive = None if adaptive is None else dict(adaptive)
        self.max_norm = torch.tensor([float(m) for m in max_norm], dtype=torch.float32, device=device)
        self.gamma = torch.zeros(n, dtype=torch.float32, device=device)
        self.has_gamma = torch.zeros(n, dtype=torch.float32, device=device)
        self.skipped = torch.zeros(n, dtype=torch.float32, device=device)
        self.t = 0

    def update(self, sumsq: Tensor, scale: Optional[Tensor]) -> Tensor:
        """One applied window: the coefficients ``c`` (NaN: skipped) from the groups' sums of squares and the pending gradient scale."""
        self.t += 1
        n = sumsq.sqrt() if scale is None else sumsq.sqrt() * scale.reshape(()).abs()
        finite = torch.isfinite(n)
        one = torch.ones_like(n)
        if self.adaptive is None:
            c = torch.minimum(one, self.max_norm / (n + 1e-6))
        else:
            rel, beta = self.adaptive["rel"], self.adaptive["beta"]
            has = self.has_gamma > 0
            first = ~has if self.t > self.adaptive["warmup_steps"] else torch.ones_like(has)   # unset, or still warming up
            limit = torch.where(first, self.max_norm, torch.minimum(self.max_norm, rel * self.gamma))
            c = torch.minimum(one, limit / (n + 1e-6))
            cn = c * n
            positive = n > 0
            g_first = torch.where(positive, torch.where(has, torch.minimum(self.gamma, cn), cn), self.gamma)
            g_else = beta * self.gamma + (1.0 - beta) * cn
            self.gamma = torch.where(finite, torch.where(first, g_first, g_else), self.gamma)
            self.has_gamma = torch.where(finite & positive, one, self.has_gamma)
        self.skipped = self.skipped + (~finite).to(torch.float32)
        return torch.where(finite, c, torch.full_like(c, math.nan))

    def state_dict(self) -> dict:
        """By group name: ``[gamma, has_gamma, skipped]`` (fp32, CPU), and ``t``."""
        rows = torch.stack([self.gamma, self.has_gamma, self.skipped], dim=1).detach().to("cpu")
        return {"t": int(self.t), "groups": {name: rows[i].clone() for i, name in enumerate(self.names)}}

    def load_state_dict(self, state: Mapping) -> None:
        """A group without saved state starts unset; saved groups this run does not have are ignored."""
        self.t = int(state.get("t", 0))
        groups = state.get("groups", {})
        rows = torch.zeros(len(self.names), 3, dtype=torch.float32)
        for i, name in enumerate(self.names):
            if name in groups:
                rows[i] = torch.as_tensor(groups[name], dtype=torch.float32).reshape(3)
        rows = rows.to(self.gamma.device)
        self.gamma, self.has_gamma, self.skipped = rows[:, 0].contiguous(), rows[:, 1].contiguous(), rows[:, 2].contiguous()


class GradGroups:
    """What ``HipAdamW(grad_groups=...)`` takes: the group table, the refined AdamW segments and, with a clip rule, its state."""

    def __init__(self, table: GroupTable, clip: Optional[Mapping] = None, param_segments: Optional[Sequence[Segment]] = None,
                 rule_max_norm: Optional[Mapping[str, float]] = None, device="cpu"):
        self.names, self.seg_end, self.seg_group = list(table[0]), [int(e) for e in table[1]], [int(g) for g in table[2]]
        self.n_groups = len(self.names)
        self.refined = refine(param_segments, table)
        self.clip: Optional[GroupClip] = None
        if clip is not None:
            own = dict(rule_max_norm or {})
            self.clip = GroupClip(self.names, [own.get(name, clip["max_norm"]) for name in self.names], clip.get("adaptive"), device=device)

    @classmethod
    def from_config(cls, node: Any, layout: pg.Layout, total: int, token_type_ranges=None, param_segments=None, device="cpu") -> "GradGroups":
        cfg = check_config(node)
        table = resolve_groups(cfg["groups"], layout, total, token_type_ranges, param_segments)
        own = {r["name"]: _threshold(f"rule (name={r['name']!r})", r["max_norm"]) for r in cfg["groups"] if "max_norm" in r}
        if own and cfg["clip"] is None:
            raise ValueError(f"grad_groups: the rules {sorted(own)} set 'max_norm' but 'clip' is null: nothing would be clipped")
        return cls(table, cfg["clip"], param_segments, own, device=device)

    def describe(self) -> str:
        sizes = [0] * self.n_groups
        start = 0
        for end, g in zip(self.seg_end, self.seg_group):
            if g >= 0:
                sizes[g] += end - start
            start = end
        return "; ".join(f"{name}: {n} elements" for name, n in zip(self.names, sizes))
