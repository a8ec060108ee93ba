"""Error rates from edit distances on the device (the reference's ``scripts/wer.py`` computes WER with ``evaluate``'s ``wer`` metric on
``whisper_normalizer``-normalised text; neither package is a dependency here).

``edit_counts`` hands lists of integer sequences to ``ssi_edit_distance`` (``include/ssi_hip.h`` holds the definition) and reads the
``{dist, S, D, I}`` of every pair back once.  ``error_rate`` turns texts (words or characters) or token ids into such sequences and the
counts into the CORPUS rate ``(S + D + I) / n_ref`` — what ``evaluate``'s ``wer`` computes, not a mean of per-utterance rates.  The
aggregation (``aggregate``), the normalisers and ``word_ids`` are pure host functions."""

from __future__ import annotations

import json
import re
import unicodedata
from collections.abc import Sequence
from typing import Any

import numpy as np
import torch

from . import _lib, ops

NORMALIZERS = ("whisper", "basic", "none")
LEVELS = ("word", "char", "token")


def pack_sequences(seqs: Sequence[Sequence[int]]) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(flat, start, length)`` as int64 arrays: the sequences end to end, and where each lies.  Ids outside int32 are a ``ValueError``."""
    try:
        arrays = [np.asarray(s, dtype=np.int64).reshape(-1) for s in seqs]
    except OverflowError as e:
        raise ValueError("ids must fit int32") from e
    length = np.array([a.size for a in arrays], dtype=np.int64)
    start = np.cumsum(length) - length
    flat = np.concatenate(arrays) if arrays else np.zeros(0, dtype=np.int64)
    if flat.size and (int(flat.min()) < -2 ** 31 or int(flat.max()) >= 2 ** 31):
        raise ValueError("ids must fit int32")
    return flat, start, length


def edit_distance_pairs(seqs: Sequence[Sequence[int]], pairs: Sequence[tuple[int, int]], device) -> torch.Tensor:
    """int32 ``[len(pairs), 4]`` ON THE DEVICE: ``{dist, S, D, I}`` of ``(reference, hypothesis) = (seqs[a], seqs[b])`` for every ``(a, b)`` of
    ``pairs``.  Every sequence is stored once, whatever the number of pairs it is in; no read-back."""
    flat, start, length = pack_sequences(seqs)
    max_len = int(length.max()) if length.size else 0
    if max_len > _lib.EDIT_MAX_LEN:
        raise ValueError(f"a sequence of {max_len} ids: ssi_edit_distance takes at most {_lib.EDIT_MAX_LEN}")
    dev = torch.device(device)
    at = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    tokens = torch.from_numpy(flat.astype(np.int32)).to(dev)
    spans = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (start[at[:, 0]], length[at[:, 0]].astype(np.int32),
                                                                        start[at[:, 1]], length[at[:, 1]].astype(np.int32))]
    out = torch.empty((len(at), 4), dtype=torch.int32, device=dev)
    ops.edit_distance(tokens, *spans, out, max_len)
    return out


def edit_counts(refs: Sequence[Sequence[int]], hyps: Sequence[Sequence[int]], device) -> torch.Tensor:
    """int32 ``[n, 4]`` (on the host) = ``{dist, S, D, I}`` of ``hyps[k]`` against ``refs[k]``: one launch, one read-back."""
    if len(refs) != len(hyps):
        raise ValueError(f"{len(refs)} references for {len(hyps)} hypotheses")
    n = len(refs)
    return edit_distance_pairs(list(refs) + list(hyps), [(k, n + k) for k in range(n)], device).cpu()


def _basic(text: str) -> str:
    text = unicodedata.normalize("NFKC", text).lower()
    text = "".join(" " if unicodedata.category(ch)[0] in "PS" else ch for ch in text)
    return " ".join(text.split())


def normalize(text: str, normalizer: str | None = "basic") -> str:
    """``"basic"``: Unicode NFKC, then lower case, then every character of a Unicode punctuation or symbol category (P*, S*) replaced by a
    space, then runs of whitespace collapsed to one space and the ends stripped.  ``"whisper"``: ``whisper_normalizer``'s
    ``EnglishTextNormalizer`` (what the reference uses), an ``ImportError`` with a clear message where the package is absent.  ``"none"`` (or
    None): the text as it is."""
    if normalizer is None or normalizer == "none":
        return text
    if normalizer == "basic":
        return _basic(text)
    if normalizer == "whisper":
        return _whisper()(text)
    raise ValueError(f"normalizer = {normalizer!r}: one of {NORMALIZERS}")


_WHISPER: list = []


def _whisper():
    if not _WHISPER:
        try:
            from whisper_normalizer.english import EnglishTextNormalizer
        except ImportError as e:
            raise ImportError("normalizer 'whisper' needs the whisper_normalizer package, which is not installed; "
                              "use normalizer 'basic' (NFKC, lower case, punctuation to spaces) or 'none'") from e
        _WHISPER.append(EnglishTextNormalizer())
    return _WHISPER[0]


def word_ids(refs: Sequence[str], hyps: Sequence[str]) -> tuple[list[list[int]], list[list[int]]]:
    """The whitespace-split words of both lists as ids of ONE dictionary (ids in order of first appearance, references first)."""
    table: dict[str, int] = {}
    return tuple([[table.setdefault(w, len(table)) for w in text.split()] for text in texts] for texts in (refs, hyps))  # type: ignore[return-value]


def aggregate(counts: Sequence[Sequence[int]], ref_lens: Sequence[int]) -> dict[str, Any]:
    """The corpus numbers from per-utterance ``{dist, S, D, I}`` rows and reference lengths: ``wer = (S + D + I) / n_ref`` (None when
    ``n_ref == 0``: no rate rather than a NaN), ``hits = n_ref - S - D``, and ``n_empty_refs``, the utterances whose reference is empty (all
    of their hypothesis counts as insertions)."""
    rows = [[int(v) for v in row] for row in counts]
    if len(rows) != len(ref_lens):
        raise ValueError(f"{len(rows)} count rows for {len(ref_lens)} references")
    if any(min(row) < 0 for row in rows):
        raise ValueError("a count row is negative: ssi_edit_distance refused a span")
    s, d, i = (sum(row[k] for row in rows) for k in (1, 2, 3))
    n_ref = int(sum(ref_lens))
    return {"wer": (s + d + i) / n_ref if n_ref else None, "n_ref": n_ref, "substitutions": s, "deletions": d, "insertions": i,
            "hits": n_ref - s - d, "n_utterances": len(rows), "n_empty_refs": sum(1 for n in ref_lens if n == 0)}


def error_rate(refs: Sequence[Any], hyps: Sequence[Any], level: str = "word", normalizer: str | None = "basic", device="cuda") -> dict[str, Any]:
    """``aggregate`` of the edit counts of ``hyps`` against ``refs``.  ``level="word"``: texts, normalised, split at whitespace;
    ``"char"``: texts, normalised, character by character; ``"token"``: sequences of ids as they are (no normaliser)."""
    if level not in LEVELS:
        raise ValueError(f"level = {level!r}: one of {LEVELS}")
    if len(refs) != len(hyps):
        raise ValueError(f"{len(refs)} references for {len(hyps)} hypotheses")
    if level == "token":
        r, h = [list(x) for x in refs], [list(x) for x in hyps]
    else:
        rt, ht = [normalize(t, normalizer) for t in refs], [normalize(t, normalizer) for t in hyps]
        r, h = word_ids(rt, ht) if level == "word" else ([[ord(c) for c in t] for t in rt], [[ord(c) for c in t] for t in ht])
    return aggregate(edit_counts(r, h, device).tolist(), [len(x) for x in r])


# ---- files -----------------------------------------------------------------------------------------------------------------------
def read_generations(path: str) -> tuple[list[Any], list[str]]:
    """``(ids, texts)`` of a generations JSONL: ``outputs[0]["text"]`` of every line, as the reference reads it."""
    ids, texts = [], []
    with open(path, encoding="utf-8") as f:
        for line in f:
            if line.strip():
                item = json.loads(line)
                ids.append(item.get("id", len(ids)))
                texts.append(item["outputs"][0]["text"])
    return ids, texts


def read_references(path: str, ids: Sequence[Any], column: str = "transcript") -> list[str]:
    """The references of ``ids`` from ``path``: a JSONL (``.jsonl`` / ``.json``) with ``id`` and ``text`` or ``column`` per line, matched by
    id; any other file is one reference per line in the order of ``ids``."""
    if re.search(r"\.jsonl?$", path):
        table = {}
        with open(path, encoding="utf-8") as f:
            for ln, line in enumerate(f, 1):
                if line.strip():
                    item = json.loads(line)
                    key = next((k for k in ("text", column, "transcript") if k in item), None)
                    if key is None or "id" not in item:
                        raise ValueError(f"{path}:{ln}: a reference needs 'id' and 'text' or '{column}'")
                    table[item["id"]] = item[key]
        missing = [i for i in ids if i not in table]
        if missing:
            raise ValueError(f"{path}: no reference for {len(missing)} ids (first: {missing[0]!r})")
        return [table[i] for i in ids]
    with open(path, encoding="utf-8") as f:
        lines = f.read().splitlines()
    if len(lines) != len(ids):
        raise ValueError(f"{path}: {len(lines)} lines for {len(ids)} generations")
    return lines
