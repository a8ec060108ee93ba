"""Dev-set loss (reference: ``/root/reference/ssi/eval.py:15-41``): forward-only use of the hot path.

Same result as the reference (sum over dev batches of ``loss_b * n_b`` divided by ``sum n_b``, with ``n_b`` the UNSHIFTED
count of non-ignored labels) but accumulated on the device with a single host sync at the end, and all-reduced across
data-parallel ranks when a process group is initialised (the reference omits that reduction,
``plans/Training Cleanup Tasks.md:83-87``).

Round 5: the dev loader's batches (2 rows each by default, ``conf/data/_sft_base.yaml:45``) reach the model ``join_batches`` at a time as one
batch (``ssi/data/window.py``: rows end to end without their padding; the sum of ``loss_b x n_b`` is kept by per-token weights exactly as for a
training window), collated and copied ahead by the prefetch thread — a forward over 2 x 2048 positions fills the GPU as badly as a training
micro-batch of that size does."""

from __future__ import annotations

import logging
from collections.abc import Callable

import torch
import torch.distributed as dist

from .loss import compute_loss

LOGGER = logging.getLogger(__name__)


def batch_to_device(batch: dict, device: torch.device) -> None:
    """In-place move of tensor values (torchtune ``utils.batch_to_device``); non-tensor values are left alone."""
    for k, v in batch.items():
        if isinstance(v, dict):
            batch_to_device(v, device)
        elif isinstance(v, torch.Tensor):
            batch[k] = v.to(device, non_blocking=True)
        elif getattr(v, "is_attn_plan", False) and torch.device(device).type == "cuda":  # ssi.attn_plan.AttnPlan: host copy kept
            batch[k] = v.to_device(device)


def _joined(data_dev, model, loss_fn, device: torch.device, join_batches: int, max_tokens: int, pad_id: int, prefetch: int):
    """The dev batches, ``join_batches`` at a time as one batch where they can be joined (``fused_windows``: plain right-padded batches or
    packs of one length; anything else passes through as it came), prepared ``prefetch`` batches ahead on a background thread."""
    from .data.window import fused_windows
    tiles = getattr(model, "_mfma_shapes", lambda: False)()
    stream = (b for _, b in fused_windows(enumerate(data_dev), join_batches, max_tokens=max_tokens, partial_windows=True, pad_id=pad_id,
                                          ignore_index=loss_fn.ignore_index, multiple=256 if tiles else 1, padded_len=model.padded_seq_len))
    if torch.device(device).type == "cuda" and prefetch > 0:
        from .data.prefetch import DevicePrefetcher
        return DevicePrefetcher(stream, device, depth=prefetch)
    return stream


class LabelMetrics:
    """Per-token-type sums over the labels of a dev set, kept on the device (not in the reference): ``acc`` is fp64 ``[n_types + 1, 4]`` =
    {n_labels, sum nll, n(rank == 0), n(rank < topk)}; its rows are ``token_type_ranges`` in order, then ``all`` (every valid label, also one
    that lies in no range).  The type is that of the LABEL, the token being predicted.  ``rank`` is the label's position in a stable descending
    sort of its logits row (``#{x > x[label]} + #{c < label: x[c] == x[label]}``): 0 iff ``argmax(row) == label`` with torch's first-occurrence
    rule.  ``HipLlamaDecoder.fused_loss(label_metrics=...)`` adds to ``acc`` from its cross-entropy launch (``ssi_ce_fwd_metrics``,
    ``ssi_ce_metrics_reduce``); ``add_logits`` is the same arithmetic in plain torch for any other model."""

    def __init__(self, token_type_ranges: dict[str, tuple[int, int]], topk: int, device: torch.device):
        if "all" in token_type_ranges:
            raise ValueError("'all' is reserved for the row over every valid label")
        if int(topk) < 1:
            raise ValueError(f"topk must be >= 1 (got {topk})")
        self.names = list(token_type_ranges)
        self.topk = int(topk)
        self.ranges_dev = torch.tensor([v for lohi in token_type_ranges.values() for v in lohi], dtype=torch.int64, device=device)
        self.acc = torch.zeros(len(self.names) + 1, 4, dtype=torch.float64, device=device)

    def add_logits(self, logits, labels: torch.Tensor, ignore_index: int) -> None:
        """``logits``: ``[..., V]`` or the list of chunks along dim 1 that ``model(...)`` returns; ``labels``: the shifted labels, same leading shape."""
        if isinstance(logits, (list, tuple)):
            logits = torch.cat(list(logits), dim=1)
        x = logits.reshape(-1, logits.size(-1))
        labels = labels.reshape(-1).to(x.device)
        vocab = x.size(-1)
        valid = (labels != ignore_index) & (labels >= 0) & (labels < vocab)
        x, lab = x[valid].float(), labels[valid]
        xl = x.gather(1, lab[:, None])
        nll = (torch.logsumexp(x, dim=1) - xl[:, 0]).double()
        below = torch.arange(vocab, device=x.device)[None, :] < lab[:, None]
        rank = ((x > xl) | ((x == xl) & below)).sum(dim=1)
        lo, hi = self.ranges_dev.view(-1, 2)[:, 0], self.ranges_dev.view(-1, 2)[:, 1]
        member = (lab[None, :] >= lo.to(x.device)[:, None]) & (lab[None, :] <= hi.to(x.device)[:, None])
        member = torch.cat([member, torch.ones_like(lab, dtype=torch.bool)[None, :]]).double()  # [n_types + 1, n_valid]
        cols = torch.stack([torch.ones_like(nll), nll, (rank == 0).double(), (rank < self.topk).double()], dim=1)
        self.acc += (member @ cols).to(self.acc.device)

    def result(self) -> dict[str, float | int]:
        """``dev_n_labels.<type>`` for every type and ``all``; ``dev_loss.<type>``, ``dev_acc.<type>``, ``dev_acc_top<k>.<type>`` (token-level: sum / n
        over the whole dev set) only where there are labels — no NaN reaches the log record.  One device read-back."""
        out: dict[str, float | int] = {}
        for name, (n, nll, top1, topk) in zip(self.names + ["all"], self.acc.tolist()):
            out[f"dev_n_labels.{name}"] = int(n)
            if n > 0:
                out[f"dev_loss.{name}"] = nll / n
                out[f"dev_acc.{name}"] = top1 / n
                out[f"dev_acc_top{self.topk}.{name}"] = topk / n
        return out


class SeqScores:
    """Per-sequence sums over the labels of ONE batch (not in the reference; the sibling of ``LabelMetrics``): ``out`` is fp64 ``[n_seq, 4]`` =
    {n_labels, sum nll, n(rank == 0), n(rank < topk)}, row i over the shifted-label positions ``[start_i, end_i)`` of batch row ``row_i``;
    it is OVERWRITTEN, so a caller hands every batch its own slice of one result tensor and reads back once.  ``spans``: host integer triples
    ``(row, start, end)`` (a list, or an int64 ``[n_seq, 3]`` tensor — one already on the device is used as it is, which is how a prefetched
    batch carries it).  Positions are those of the batch as the caller built it: ``HipLlamaDecoder.fused_loss(seq_scores=...)`` makes the flat
    offsets after its own right-padding (``ssi_ce_fwd_metrics`` + ``ssi_seq_score_reduce``); ``add_logits`` is the same arithmetic in plain
    torch for any other model.  ``keep_rows``: also leave ``row_nll`` (fp32 ``[rows, row_len]``, 0 where the label is ignored) on the object."""

    def __init__(self, spans, topk: int, out: torch.Tensor, keep_rows: bool = False):
        if int(topk) < 1:
            raise ValueError(f"topk must be >= 1 (got {topk})")
        spans = spans if torch.is_tensor(spans) else torch.tensor([tuple(int(v) for v in t) for t in spans], dtype=torch.int64).reshape(-1, 3)
        if spans.dim() != 2 or spans.size(1) != 3 or spans.dtype != torch.int64:
            raise ValueError("spans must be int64 triples (row, start, end)")
        if out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != 4 * spans.size(0):
            raise ValueError(f"out must be a contiguous float64 [{spans.size(0)}, 4] tensor")
        self.spans, self.topk, self.out, self.keep_rows = spans, int(topk), out, bool(keep_rows)
        self.row_nll: torch.Tensor | None = None
        self.row_len = 0

    def flat_spans(self, row_len: int, device) -> tuple[torch.Tensor, torch.Tensor]:
        """Device int64 ``(start, end)`` of every sequence in a ``[rows, row_len]`` batch laid out flat: ``row * row_len + pos``."""
        sp = self.spans.to(device)
        base = sp[:, 0] * int(row_len)
        return (base + sp[:, 1]).contiguous(), (base + sp[:, 2]).contiguous()

    def add_logits(self, logits, labels: torch.Tensor, ignore_index: int) -> None:
        """``logits``: ``[B, S, V]`` or the list of chunks along dim 1 that ``model(...)`` returns; ``labels``: the shifted labels ``[B, S]``.  The
        rank rule of ``LabelMetrics.add_logits``; fp64 sums per sequence."""
        if isinstance(logits, (list, tuple)):
            logits = torch.cat(list(logits), dim=1)
        B, S = labels.shape[0], labels.shape[-1]
        x = logits.reshape(-1, logits.size(-1))
        labels = labels.reshape(-1).to(x.device)
        vocab = x.size(-1)
        valid = (labels != ignore_index) & (labels >= 0) & (labels < vocab)
        xv, lab = x[valid].float(), labels[valid]
        xl = xv.gather(1, lab[:, None])
        nll = torch.logsumexp(xv, dim=1) - xl[:, 0]
        below = torch.arange(vocab, device=x.device)[None, :] < lab[:, None]
        rank = ((xv > xl) | ((xv == xl) & below)).sum(dim=1)
        cols = torch.zeros(B * S, 4, dtype=torch.float64, device=x.device)
        cols[valid] = torch.stack([torch.ones_like(nll).double(), nll.double(), (rank == 0).double(), (rank < self.topk).double()], dim=1)
        start, end = self.flat_spans(S, "cpu")
        end = end.clamp(0, B * S)
        start = torch.minimum(start.clamp(min=0), end)
        sums = [cols[a:b].sum(dim=0) for a, b in zip(start.tolist(), end.tolist())]
        self.out.view(-1, 4).copy_(torch.stack(sums) if sums else cols[:0])
        if self.keep_rows:
            row_nll = torch.zeros(B * S, dtype=torch.float32, device=x.device)
            row_nll[valid] = nll
            self.row_nll, self.row_len = row_nll, S


def compute_dataset_metrics(model, data_dev, loss_fn: Callable, epoch: int, global_step: int, steps_per_epoch: int, device: torch.device, *,
                            token_type_ranges: dict[str, tuple[int, int]], topk: int = 5, join_batches: int = 0, max_tokens: int = 32768,
                            pad_id: int = 0, prefetch: int = 2) -> dict[str, float | int]:
    """``compute_dataset_loss`` plus loss and top-1 / top-k accuracy per token type of the label (not in the reference).  ``dev_loss`` is the
    float ``compute_dataset_loss`` returns on the same data and settings, bit for bit: the same loop, the same launches but for the
    cross-entropy kernel, which also ranks each label in its row (``LabelMetrics``).  The per-type values are token-level sums over the whole dev
    set, so — unlike the reference's ``dev_loss`` — they do not depend on how it is batched or joined.  Under data parallelism the accumulator
    is all-reduced beside the two scalars."""
    from .data.unpad import loss_inputs
    dev_loss_running = torch.zeros((), dtype=torch.float64, device=device)
    num_tokens_dev = torch.zeros((), dtype=torch.float64, device=device)
    metrics = LabelMetrics(token_type_ranges, topk, device)
    joinable = join_batches > 1 and hasattr(model, "fused_loss") and hasattr(model, "padded_seq_len")
    batches = _joined(data_dev, model, loss_fn, device, join_batches, max_tokens, pad_id, prefetch) if joinable else data_dev
    model.eval()
    with torch.inference_mode():
        for i_dev, dev_batch in enumerate(batches):
            batch_to_device(dev_batch, device)
            n_b = (dev_batch["labels"] != loss_fn.ignore_index).sum()
            dev_loss_running += compute_loss(loss_inputs(dev_batch), model, loss_fn, label_metrics=metrics).double() * n_b
            num_tokens_dev += n_b
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        both = torch.stack([dev_loss_running, num_tokens_dev])
        dist.all_reduce(both)
        dist.all_reduce(metrics.acc)
        dev_loss_running, num_tokens_dev = both[0], both[1]
    model.train()
    out: dict[str, float | int] = {"dev_loss": float((dev_loss_running / num_tokens_dev).item())}
    out.update(metrics.result())
    k = metrics.topk
    per_type = " | ".join(f"{name}: loss {out[f'dev_loss.{name}']:.4f} acc {out[f'dev_acc.{name}']:.4f} top{k} {out[f'dev_acc_top{k}.{name}']:.4f}"
                          for name in metrics.names + ["all"] if out[f"dev_n_labels.{name}"])
    LOGGER.info(f"Epoch {epoch + 1:03d} | Global Step {global_step} | Dev Loss: {out['dev_loss']:.4f}" + (f" | {per_type}" if per_type else ""))
    return out


def compute_dataset_loss(model, data_dev, loss_fn: Callable, epoch: int, global_step: int, steps_per_epoch: int,
                         device: torch.device, *, join_batches: int = 0, max_tokens: int = 32768, pad_id: int = 0, prefetch: int = 2) -> float:
    """The reference's signature; the keyword arguments are this build's (``join_batches`` <= 1: every dev batch on its own, as the reference)."""
    from .data.unpad import loss_inputs
    dev_loss_running = torch.zeros((), dtype=torch.float64, device=device)
    num_tokens_dev = torch.zeros((), dtype=torch.float64, device=device)
    joinable = join_batches > 1 and hasattr(model, "fused_loss") and hasattr(model, "padded_seq_len")
    batches = _joined(data_dev, model, loss_fn, device, join_batches, max_tokens, pad_id, prefetch) if joinable else data_dev
    model.eval()
    with torch.inference_mode():
        for i_dev, dev_batch in enumerate(batches):
            batch_to_device(dev_batch, device)
            n_b = (dev_batch["labels"] != loss_fn.ignore_index).sum()  # (a joined batch: the sum of its batches' counts)
            dev_loss_running += compute_loss(loss_inputs(dev_batch), model, loss_fn).double() * n_b
            num_tokens_dev += n_b
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        both = torch.stack([dev_loss_running, num_tokens_dev])
        dist.all_reduce(both)
        dev_loss_running, num_tokens_dev = both[0], both[1]
    model.train()
    value = float((dev_loss_running / num_tokens_dev).item())
    LOGGER.info(f"Epoch {epoch + 1:03d} | Global Step {global_step} | Dev Loss: {value:.4f}")
    return value
