"""Likelihood scoring (not in the reference): the log-probability of each of many sequences, not of a batch.

What zero-shot comparisons of speech-unit language models need — which of two unit sequences the model finds more probable (sWUGGY / sBLIMP /
spoken StoryCloze style pair accuracy), N-best rescoring of transcripts given the units, per-utterance perplexity for data filtering — is
forward + cross-entropy, the path ``ssi.eval.compute_dataset_metrics`` runs, reduced per DOCUMENT of a packed row instead of per token type.

``score_sequences`` packs the sequences into full rows on the host (first-fit decreasing: a 30-token item does not cost a 2048-position row),
runs ``compute_loss(batch, model, loss_fn, seq_scores=...)`` over batches of rows under ``inference_mode`` (block-causal over the documents
through ``input_pos``; on the HIP decoder ``ssi_ce_fwd_metrics`` + ``ssi_seq_score_reduce``, on any other model the same arithmetic in plain
torch), keeps every result in one device tensor and reads it back once, in the caller's order."""

from __future__ import annotations

import json
import logging
import math
from collections.abc import Callable, Sequence
from dataclasses import dataclass
from typing import Any

import torch
from torch import Tensor

from .constants import CROSS_ENTROPY_IGNORE_IDX
from .eval import SeqScores
from .loss import CEWithChunkedOutputLoss, compute_loss

LOGGER = logging.getLogger(__name__)

__all__ = ["SequenceScores", "pack_for_scoring", "scoring_batches", "prefill_batches", "score_sequences", "pair_accuracy", "score_file"]


@dataclass
class SequenceScores:
    """One entry per input sequence, in INPUT order.  ``logprob``: float64, minus the sum of the counted tokens' nll (natural log);
    ``n_tokens``: how many tokens counted; ``n_top1`` / ``n_topk``: how many of them were the model's first choice / among its ``topk`` first;
    ``mean_logprob``: ``logprob / n_tokens``, NaN where nothing counted; ``token_logprobs``: per sequence a float32 tensor of the counted
    tokens' log-probabilities (``token_logprobs=True`` only)."""
    logprob: Tensor
    n_tokens: Tensor
    n_top1: Tensor
    n_topk: Tensor
    mean_logprob: Tensor
    topk: int
    token_logprobs: list[Tensor] | None = None

    def __len__(self) -> int:
        return int(self.logprob.numel())


def pack_for_scoring(lengths: Sequence[int], row_len: int) -> list[list[int]]:
    """First-fit decreasing: sequences by falling length (ties by index), each into the first row with room; a new row when there is none.
    Returns the rows as lists of sequence indices in the order they lie in the row.  Host only and deterministic."""
    for i, n in enumerate(lengths):
        if n > row_len:
            raise ValueError(f"sequence {i} has {n} tokens, more than row_len = {row_len}")
    rows: list[list[int]] = []
    room: list[int] = []
    first_open = 0                                   # rows before it are full: not looked at again
    for i in sorted(range(len(lengths)), key=lambda j: (-lengths[j], j)):
        n = lengths[i]
        while first_open < len(room) and room[first_open] == 0:
            first_open += 1
        r = next((k for k in range(first_open, len(room)) if room[k] >= n), len(room))
        if r == len(room):
            rows.append([])
            room.append(row_len)
        rows[r].append(i)
        room[r] -= n
    return rows


def _place_rows(sequences: list[Tensor], chunk: list[list[int]], row_len: int, pad_id: int) -> tuple[Tensor, Tensor, list[tuple[int, int, int, int]]]:
    """The placement loop of every packed host batch: ``chunk``'s rows (``pack_for_scoring``'s) as int64 ``tokens`` (``pad_id`` on the tail) and
    ``input_pos`` (restarting at 0 with every sequence and on the tail), and ``(row, start, length, index)`` of every sequence as they lie."""
    tokens = torch.full((len(chunk), row_len), pad_id, dtype=torch.int64)
    input_pos = torch.empty(len(chunk), row_len, dtype=torch.int64)
    placed = []
    for r, members in enumerate(chunk):
        at = 0
        for i in members:
            n = sequences[i].numel()
            tokens[r, at:at + n] = sequences[i]
            input_pos[r, at:at + n] = torch.arange(n)
            placed.append((r, at, n, i))
            at += n
        input_pos[r, at:] = torch.arange(row_len - at)     # the tail: a document of its own
    return tokens, input_pos, placed


def scoring_batches(sequences: list[Tensor], score_from: list[int], rows: list[list[int]], row_len: int, rows_per_batch: int, pad_id: int,
                    ignore_index: int = CROSS_ENTROPY_IGNORE_IDX, dense_mask: bool = False, token_logprobs: bool = False):
    """The packed host batches of ``score_sequences``, one at a time (``sequences``: int64 tensors; ``rows``: ``pack_for_scoring``'s).
    ``labels`` are UNSHIFTED (``compute_loss`` shifts them): the tokens, ``ignore_index`` on every document's context (its first token at
    least) and on the tail, so after the shift the last position of a document predicts nothing.  ``input_pos`` restarts at 0 with every
    document; the tail, filled with ``pad_id``, is a document of its own.
    ``seq_spans``: per sequence ``(row in the batch, start, end)`` in SHIFTED-label positions; ``seq_index``: which input sequence each is."""
    for b0 in range(0, len(rows), rows_per_batch):
        chunk = rows[b0:b0 + rows_per_batch]
        tokens, input_pos, placed = _place_rows(sequences, chunk, row_len, pad_id)
        labels = torch.full((len(chunk), row_len), ignore_index, dtype=torch.int64)
        spans, tok_pos = [], []
        for r, at, n, i in placed:
            sf = score_from[i]
            labels[r, at + sf:at + n] = sequences[i][sf:]
            lo, hi = at + min(sf, n) - 1, at + n - 1      # the label of position p sits at p - 1 after the shift
            spans.append((r, max(lo, 0), max(hi, lo, 0)))
            if token_logprobs:
                tok_pos.append(torch.stack([torch.full((max(hi - lo, 0),), r, dtype=torch.int64), torch.arange(lo, max(hi, lo))], dim=1))
        batch: dict[str, Any] = {"tokens": tokens, "labels": labels, "input_pos": input_pos,
                                 "seq_spans": torch.tensor(spans, dtype=torch.int64).reshape(-1, 3), "seq_index": [p[3] for p in placed]}
        if token_logprobs:
            batch["tok_pos"] = torch.cat(tok_pos) if tok_pos else torch.zeros(0, 2, dtype=torch.int64)
        if dense_mask:                                         # a model that takes the dense block-causal mask instead of input_pos alone
            from .data.packed import packed_block_causal_mask
            docs = [[n for r, _, n, _ in placed if r == k and n] for k in range(len(chunk))]   # per row: its documents' lengths, then the tail's
            batch["mask"] = packed_block_causal_mask([torch.tensor(d + [row_len - sum(d)] * (sum(d) < row_len), dtype=torch.int64) for d in docs])
        yield batch


def prefill_batches(sequences: list[Tensor], cap: int, row_len: int, rows_per_batch: int):
    """The packed host batches of ``HipLlamaDecoder.prefill``, one at a time (prompt ``i`` fills slot ``i`` of a K/V cache of ``cap`` positions per
    slot): ``tokens`` and ``input_pos`` as ``scoring_batches`` makes them with ``pad_id=0``; ``dest`` (int64, same shape): where a position's K / V
    go, ``slot * cap + position``, -1 on the tail; and per prompt of the batch the flat position of its LAST token and its index (int64 tensors)."""
    rows = pack_for_scoring([s.numel() for s in sequences], row_len)
    for b0 in range(0, len(rows), rows_per_batch):
        tokens, input_pos, placed = _place_rows(sequences, rows[b0:b0 + rows_per_batch], row_len, 0)
        dest = torch.full_like(tokens, -1)
        for r, at, n, i in placed:
            dest[r, at:at + n] = i * cap + torch.arange(n)
        last = torch.tensor([r * row_len + at + n - 1 for r, at, n, _ in placed], dtype=torch.int64)
        yield tokens, input_pos, dest, last, torch.tensor([p[3] for p in placed], dtype=torch.int64)


def score_sequences(model, sequences: Sequence[Any], *, score_from: Sequence[int] | None = None, pad_id: int, device: torch.device | str,
                    row_len: int = 2048, rows_per_batch: int = 8, topk: int = 5, token_logprobs: bool = False,
                    loss_fn: Callable | None = None) -> SequenceScores:
    """``sequences``: 1-D integer sequences (lists or tensors).  ``score_from[i]`` (default 1, >= 1): the first token index of sequence ``i``
    that counts; everything before it is context — a BOS, or the speech units an N-best hypothesis is conditioned on.  The first token of a
    sequence never counts (nothing predicts it).  A sequence longer than ``row_len`` raises.  ``loss_fn``: default
    ``CEWithChunkedOutputLoss()``; with a model that has no ``fused_loss`` the batches also carry the dense block-causal ``mask`` and the
    scores come from ``SeqScores.add_logits``."""
    device = torch.device(device)
    row_len, rows_per_batch, topk = int(row_len), int(rows_per_batch), int(topk)
    if row_len < 1 or rows_per_batch < 1 or topk < 1:
        raise ValueError(f"row_len, rows_per_batch and topk must be >= 1 (got {row_len}, {rows_per_batch}, {topk})")
    seqs = [torch.as_tensor(s, dtype=torch.int64).reshape(-1) for s in sequences]
    n = len(seqs)
    sfs = [1] * n if score_from is None else [int(v) for v in score_from]
    if len(sfs) != n:
        raise ValueError(f"score_from has {len(sfs)} entries for {n} sequences")
    for i, sf in enumerate(sfs):
        if sf < 1:
            raise ValueError(f"score_from[{i}] = {sf}: the first token of a sequence never counts, so score_from must be >= 1")
    rows = pack_for_scoring([s.numel() for s in seqs], row_len)
    loss_fn = CEWithChunkedOutputLoss() if loss_fn is None else loss_fn
    ignore_index = getattr(loss_fn, "ignore_index", CROSS_ENTROPY_IGNORE_IDX)
    fused = hasattr(model, "fused_loss")
    stream = scoring_batches(seqs, sfs, rows, row_len, rows_per_batch, int(pad_id), ignore_index, not fused, token_logprobs)
    if device.type == "cuda":
        from .data.prefetch import DevicePrefetcher
        stream = DevicePrefetcher(stream, device, depth=2)
    out = torch.zeros(n, 4, dtype=torch.float64, device=device)   # in PLACEMENT order: every batch writes its own slice
    order: list[int] = []
    tok_nll: list[Tensor] = []
    was_training = bool(getattr(model, "training", False))
    model.eval()
    try:
        with torch.inference_mode():
            for batch in stream:
                index = batch.pop("seq_index")
                spans = batch.pop("seq_spans")
                tok_pos = batch.pop("tok_pos", None)
                if device.type != "cuda":
                    spans = spans.to(device)
                    batch = {k: v.to(device) for k, v in batch.items()}
                scores = SeqScores(spans, topk, out[len(order):len(order) + len(index)], keep_rows=token_logprobs)
                order += index
                compute_loss(batch, model, loss_fn, seq_scores=scores)
                if token_logprobs:
                    tp = tok_pos.to(scores.row_nll.device)
                    tok_nll.append(scores.row_nll.reshape(-1)[tp[:, 0] * scores.row_len + tp[:, 1]])
    finally:
        if was_training:
            model.train()
    host = out.cpu()                                           # the one read-back
    placed = torch.empty_like(host)
    placed[torch.tensor(order, dtype=torch.int64)] = host
    n_tokens = placed[:, 0].round().to(torch.int64)
    logprob = -placed[:, 1]
    mean = torch.where(n_tokens > 0, logprob / n_tokens.clamp(min=1), torch.full_like(logprob, math.nan))
    per_token = None
    if token_logprobs:
        flat = -(torch.cat(tok_nll).cpu() if tok_nll else torch.zeros(0))
        per_token = [torch.zeros(0)] * n
        at = 0
        for i in order:
            k = max(seqs[i].numel() - sfs[i], 0)
            per_token[i] = flat[at:at + k].float()
            at += k
    return SequenceScores(logprob=logprob, n_tokens=n_tokens, n_top1=placed[:, 2].round().to(torch.int64),
                          n_topk=placed[:, 3].round().to(torch.int64), mean_logprob=mean, topk=topk, token_logprobs=per_token)


def pair_accuracy(scores: SequenceScores, positive_idx: Sequence[int], negative_idx: Sequence[int], normalize: str = "sum") -> tuple[float, int]:
    """The share of pairs ``(positive_idx[j], negative_idx[j])`` whose positive scores higher; a tie counts one half.  ``normalize``: ``"sum"``
    compares ``logprob``, ``"mean"`` compares ``mean_logprob`` (per counted token).  Returns ``(accuracy, n_pairs)``; NaN for no pairs."""
    if normalize not in ("sum", "mean"):
        raise ValueError(f"normalize must be 'sum' or 'mean' (got {normalize!r})")
    if len(positive_idx) != len(negative_idx):
        raise ValueError(f"{len(positive_idx)} positives against {len(negative_idx)} negatives")
    n = len(positive_idx)
    if n == 0:
        return math.nan, 0
    v = scores.logprob if normalize == "sum" else scores.mean_logprob
    pos, neg = v[torch.as_tensor(positive_idx, dtype=torch.int64)], v[torch.as_tensor(negative_idx, dtype=torch.int64)]
    return (int((pos > neg).sum()) + 0.5 * int((pos == neg).sum())) / n, n


def _read_items(tokenizer, in_path: str) -> tuple[list[Any], list[list[int]], list[int], list[int], list[int]]:
    ids, seqs, sfs, pos, neg = [], [], [], [], []
    groups: dict[Any, tuple[list[int], list[int]]] = {}
    with open(in_path, encoding="utf-8") as f:
        for ln, line in enumerate(f, 1):
            if not line.strip():
                continue
            item = json.loads(line)
            if ("tokens" in item) == ("text" in item):
                raise ValueError(f"{in_path}:{ln}: an item needs exactly one of 'tokens' and 'text'")
            if "prompt_tokens" in item and "prompt" in item:
                raise ValueError(f"{in_path}:{ln}: at most one of 'prompt_tokens' and 'prompt'")
            context: list[int] = []
            if "prompt_tokens" in item:
                context = [int(t) for t in item["prompt_tokens"]]
            elif "prompt" in item:
                context = list(tokenizer.encode(item["prompt"], add_bos=True, add_eos=False))
            if "tokens" in item:
                body = [int(t) for t in item["tokens"]]
            else:                                              # the BOS opens the sequence: a prompt, where there is one, carries it
                body = list(tokenizer.encode(item["text"], add_bos=not context, add_eos=False))
            k = len(seqs)
            ids.append(item.get("id", k))
            seqs.append(context + body)
            sfs.append(max(len(context), 1))
            if item.get("pair") is not None:
                groups.setdefault(item["pair"], ([], []))[0 if item.get("positive") else 1].append(k)
    for name, (p, q) in groups.items():
        if not p or not q:
            raise ValueError(f"{in_path}: pair {name!r} needs a positive item and a negative one")
        for a in p:
            for b in q:
                pos.append(a)
                neg.append(b)
    return ids, seqs, sfs, pos, neg


def score_file(model, tokenizer, in_path: str, out_path: str | None, **kw) -> dict[str, Any]:
    """JSONL in, JSONL out.  Every input line: ``id``; exactly one of ``tokens`` (ids, taken as they are) and ``text`` (the tokenizer's
    ``encode`` with BOS and without EOS); optional ``prompt_tokens`` / ``prompt``: context that is prepended and not scored (a ``prompt`` carries
    the BOS then); optional ``pair`` (any value: items with the same one are compared) and ``positive`` (true on the item that should win).
    Every output line: ``id``, ``logprob``, ``mean_logprob`` (null where nothing counted), ``n_tokens``, ``n_top1``.  ``out_path=None`` writes
    nothing.  Returns ``{"items", "tokens"}`` and, where there are pairs, ``pair_acc`` (sum), ``pair_acc_mean`` and ``pair_n``.  ``kw`` goes to
    ``score_sequences``; ``pad_id`` defaults to the tokenizer's."""
    ids, seqs, sfs, pos, neg = _read_items(tokenizer, in_path)
    kw.setdefault("pad_id", int(getattr(tokenizer, "pad_id", 0) or 0))
    scores = score_sequences(model, seqs, score_from=sfs, **kw)
    if out_path is not None:
        with open(out_path, "w", encoding="utf-8") as f:
            for i, item_id in enumerate(ids):
                n = int(scores.n_tokens[i])
                f.write(json.dumps({"id": item_id, "logprob": float(scores.logprob[i]), "mean_logprob": float(scores.mean_logprob[i]) if n else None,
                                    "n_tokens": n, "n_top1": int(scores.n_top1[i])}) + "\n")
    summary: dict[str, Any] = {"items": len(ids), "tokens": int(scores.n_tokens.sum())}
    if pos:
        summary["pair_acc"], summary["pair_n"] = pair_accuracy(scores, pos, neg, "sum")
        summary["pair_acc_mean"] = pair_accuracy(scores, pos, neg, "mean")[0]
    return summary
