"""Parameter groups as element ranges of the flat parameter buffer (not in the reference; config key ``param_groups``, default null).

The setting this project exists for treats two kinds of weight differently — the new vocabulary rows of the tied embedding and the pretrained
rest — and the boundary runs through the middle of ONE tensor, which torch's param groups cannot say.  The flat buffer can: a rule set is
resolved, on the host, into consecutive :class:`Segment` s that cover ``[0, total)``, each with an lr scale, a weight decay (``None``: the
optimizer's) and a frozen flag; ``HipAdamW`` applies them in one ``ssi_adamw_step_seg`` launch and the decoder skips the weight-gradient
launches of what is frozen.

A rule is a mapping::

    params: ["tok_embeddings.weight"]   # fnmatch patterns over the state-dict (torchtune) names
    token_types: [dsu, modality]        # optional, embedding only: the rows of these blocks of token_type_ranges
    lr_scale: 1.0                       # finite, >= 0: the range runs at lr_scale x the scheduler's lr
    weight_decay: null                  # null: the optimizer's
    frozen: false

The first matching rule wins; what no rule matches keeps the optimizer's settings.  ``q_proj`` / ``k_proj`` / ``v_proj`` are row ranges of the
fused ``wqkv`` and ``w1`` / ``w3`` of ``w13``, so they resolve to ranges of their own.  Elements that belong to no parameter (the vocabulary
padding rows, alignment gaps) join the segment in front of them: they are zero with a zero gradient, and the arithmetic keeps them zero.
Adjacent ranges with equal settings merge.  Resolution needs only a plain description of the layout (:func:`model_layout`), no GPU."""

from __future__ import annotations

import math
from dataclasses import dataclass
from fnmatch import fnmatchcase
from typing import Any, Iterable, Mapping, Optional, Sequence

RULE_KEYS = ("params", "token_types", "lr_scale", "weight_decay", "frozen")
EMBEDDING = "tok_embeddings.weight"

Layout = Mapping[str, tuple[int, int, int]]   # state-dict name -> (offset in the flat buffer, rows, columns); a vector is one row


@dataclass(frozen=True)
class Segment:
    start: int
    end: int
    lr_scale: float = 1.0
    weight_decay: Optional[float] = None
    frozen: bool = False

    @property
    def setting(self) -> tuple:
        # (a frozen range has no other setting: frozen ranges always merge)
        return (True,) if self.frozen else (False, self.lr_scale, self.weight_decay)


def model_layout(model) -> tuple[dict[str, tuple[int, int, int]], int]:
    """``(layout, total)`` of a ``HipLlamaDecoder``, read off ``_slices`` and ``_param_src``."""
    names = {id(p): n for n, p in model.named_parameters()}
    layout = {}
    for p, src, rows in model._param_src:
        off, shape = model._slices[src]
        cols = 1
        for s in shape[1:]:
            cols *= s
        if len(shape) == 1:
            layout[names[id(p)]] = (off, 1, shape[0])
        else:
            r0, r1 = rows if rows is not None else (0, shape[0])
            layout[names[id(p)]] = (off + r0 * cols, r1 - r0, cols)
    return layout, int(model._flat.numel())


def _number(rule_name: str, key: str, value: Any) -> float:
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or value < 0:
        raise ValueError(f"param_groups {rule_name}: '{key}' must be a finite number >= 0, got {value!r}")
    return float(value)


def _normalise(index: int, rule: Mapping) -> dict:
    name = f"rule {index}"
    if not hasattr(rule, "keys"):
        raise ValueError(f"param_groups {name}: a rule is a mapping, got {rule!r}")
    unknown = sorted(k for k in rule.keys() if k not in RULE_KEYS)
    if unknown:
        raise ValueError(f"param_groups {name}: unknown keys {unknown} (known: {list(RULE_KEYS)})")
    pats = rule.get("params")
    if isinstance(pats, str):
        pats = [pats]
    if pats is None or len(pats) == 0 or not all(isinstance(p, str) for p in pats):
        raise ValueError(f"param_groups {name}: 'params' must be a non-empty list of name patterns, got {pats!r}")
    name = f"rule {index} (params={list(pats)})"
    kinds = rule.get("token_types")
    if kinds is not None and (isinstance(kinds, str) or len(kinds) == 0 or not all(isinstance(k, str) for k in kinds)):
        raise ValueError(f"param_groups {name}: 'token_types' must be a non-empty list of token type names, got {kinds!r}")
    wd = rule.get("weight_decay")
    frozen = rule.get("frozen", False)
    if not isinstance(frozen, bool):
        raise ValueError(f"param_groups {name}: 'frozen' must be true or false, got {frozen!r}")
    return dict(name=name, params=list(pats), token_types=None if kinds is None else list(kinds),
                lr_scale=_number(name, "lr_scale", rule.get("lr_scale", 1.0)),
                weight_decay=None if wd is None else _number(name, "weight_decay", wd), frozen=frozen)


def resolve(rules: Optional[Sequence[Mapping]], layout: Layout, total: int,
            token_type_ranges: Optional[Mapping[str, tuple[int, int]]] = None) -> list[Segment]:
    """The segments of ``rules`` on ``layout``: consecutive, covering ``[0, total)``, every start a multiple of 8.  ``token_type_ranges``:
    inclusive ``(first, last)`` row ids per kind, as ``get_token_type_ranges`` gives them.  Every problem is a ``ValueError`` naming the rule."""
    if rules is None or isinstance(rules, (str, bytes)) or hasattr(rules, "keys") or len(rules) == 0:
        raise ValueError(f"param_groups must be a non-empty list of rules, got {rules!r}")
    rules = [_normalise(i, r) for i, r in enumerate(rules)]
    names = sorted(layout, key=lambda n: layout[n][0])
    for r in rules:
        r["matched"] = [n for n in names if any(fnmatchcase(n, pat) for pat in r["params"])]
        if not r["matched"]:
            raise ValueError(f"param_groups {r['name']}: no parameter matches (names are the state-dict ones, e.g. {names[:3]})")
        if r["token_types"] is not None:
            if r["matched"] != [EMBEDDING]:
                raise ValueError(f"param_groups {r['name']}: 'token_types' selects rows of {EMBEDDING} only, but the patterns match "
                                 f"{[n for n in r['matched'] if n != EMBEDDING][:3]}")
            known = dict(token_type_ranges or {})
            rows = layout[EMBEDDING][1]
            r["rows"] = []
            for kind in r["token_types"]:
                if kind not in known:
                    raise ValueError(f"param_groups {r['name']}: unknown token type {kind!r} (known: {sorted(known)})")
                first, last = known[kind]
                if not 0 <= first <= last < rows:
                    raise ValueError(f"param_groups {r['name']}: token type {kind!r} = rows {first}..{last} is outside the embedding's {rows} rows")
                r["rows"].append((int(first), int(last) + 1))

    def segment(start: int, end: int, r: Optional[dict]) -> Segment:
        return Segment(start, end) if r is None else Segment(start, end, r["lr_scale"], r["weight_decay"], r["frozen"])

    pieces: list[Segment] = []
    for n in names:
        off, rows, cols = layout[n]
        mine = [r for r in rules if n in r["matched"]]
        if not any(r["token_types"] is not None for r in mine):
            pieces.append(segment(off, off + rows * cols, mine[0] if mine else None))
            continue
        cuts = sorted({0, rows} | {c for r in mine if r["token_types"] is not None for lohi in r["rows"] for c in lohi})
        for a, b in zip(cuts, cuts[1:]):   # an elementary row interval lies inside or outside every rule's rows: the first rule that holds it
            first = next((r for r in mine if r["token_types"] is None or any(lo <= a and b <= hi for lo, hi in r["rows"])), None)
            pieces.append(segment(off + a * cols, off + b * cols, first))
    out: list[Segment] = []
    pos = 0
    for j, s in enumerate(pieces):
        if s.start < pos or s.end <= s.start:
            raise ValueError(f"param_groups: the layout's parameters overlap or are empty at element {s.start}")
        start = 0 if j == 0 else s.start                                   # (a gap in front of the first parameter joins it)
        end = pieces[j + 1].start if j + 1 < len(pieces) else int(total)   # what follows a parameter and belongs to none joins it
        if end < s.end:
            raise ValueError(f"param_groups: the layout's parameters overlap at element {end}")
        pos = end
        if start % 8:
            raise ValueError(f"param_groups: a range starts at element {start}, not a multiple of 8 (16-byte vectors must lie in one range)")
        if out and out[-1].setting == s.setting:
            out[-1] = Segment(out[-1].start, end, out[-1].lr_scale, out[-1].weight_decay, out[-1].frozen)
        else:
            out.append(Segment(start, end, s.lr_scale, s.weight_decay, s.frozen))
    return out


def check_segments(segments: Iterable[Segment], total: int) -> list[Segment]:
    """``segments`` as a list, after checking that they are what the optimizer kernel takes: consecutive over ``[0, total)``, starts multiples of 8."""
    segs = list(segments)
    pos = 0
    for s in segs:
        if s.start != pos or s.end <= s.start or s.start % 8:
            raise ValueError(f"param segments must be consecutive, non-empty and start on multiples of 8: {s} after element {pos}")
        if not s.frozen:
            _number(f"segment [{s.start}, {s.end})", "lr_scale", s.lr_scale)
            if s.weight_decay is not None:
                _number(f"segment [{s.start}, {s.end})", "weight_decay", s.weight_decay)
        pos = s.end
    if pos != total:
        raise ValueError(f"param segments cover [0, {pos}), the flat buffer has {total} elements")
    return segs


def clip(segments: Sequence[Segment], lo: int, hi: int) -> list[Segment]:
    """The parts of ``segments`` inside ``[lo, hi)``, in buffer coordinates."""
    return [Segment(max(s.start, lo), min(s.end, hi), s.lr_scale, s.weight_decay, s.frozen) for s in segments if s.start < hi and s.end > lo]


def all_frozen(segments: Sequence[Segment], lo: int, hi: int) -> bool:
    return all(s.frozen for s in segments if s.start < hi and s.end > lo)


def trainable_ranges(segments: Sequence[Segment]) -> list[tuple[int, int]]:
    """Maximal ``[lo, hi)`` ranges that hold no frozen element, ascending."""
    out: list[tuple[int, int]] = []
    for s in segments:
        if s.frozen:
            continue
        if out and out[-1][1] == s.start:
            out[-1] = (out[-1][0], s.end)
        else:
            out.append((s.start, s.end))
    return out


def describe(segments: Sequence[Segment]) -> str:
    parts = []
    for s in segments:
        what = "frozen" if s.frozen else f"lr x {s.lr_scale:g}, weight_decay {'default' if s.weight_decay is None else format(s.weight_decay, 'g')}"
        parts.append(f"[{s.start}, {s.end}): {what}")
    return "; ".join(parts)
