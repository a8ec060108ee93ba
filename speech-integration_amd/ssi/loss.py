"""Loss of the training step (reference: ``/root/reference/ssi/loss.py:7-22`` + torchtune ``CEWithChunkedOutputLoss``).

``compute_loss(batch, model, loss_fn)`` keeps the reference signature and semantics: forward, shift labels left by one
(last position ignored), mean NLL over the SHIFTED non-ignored labels, ``batch`` not mutated.  When ``model`` is the HIP
decoder and ``loss_fn`` is :class:`CEWithChunkedOutputLoss`, the LM head and the cross-entropy run fused on the GPU
(K8+K9); any other (model, loss_fn) pair takes the literal reference route ``loss_fn(model(...), labels)``."""

from __future__ import annotations

import math
from collections.abc import Callable

import torch
from torch import Tensor

from . import ops
from .constants import CROSS_ENTROPY_IGNORE_IDX


class CEWithChunkedOutputLoss(torch.nn.Module):
    """Same constructor, attributes and call contract as torchtune 0.5.0's class of that name (``trainer.py:300``):
    ``loss_fn(list_of_logit_chunks, labels[B, S]) -> sum NLL / count(labels != ignore_index)``; also accepts one
    ``[N, V]`` tensor with flat labels (``loss.py:17-19``).  The arithmetic is the HIP cross-entropy kernel (fp32
    log-sum-exp per row, deterministic row reduction); logits must be GPU tensors."""

    def __init__(self, num_output_chunks: int = 8, ignore_index: int = CROSS_ENTROPY_IGNORE_IDX):
        super().__init__()
        self.num_output_chunks = num_output_chunks
        self.ignore_index = ignore_index

    def forward(self, logits, labels: Tensor) -> Tensor:
        if isinstance(logits, (list, tuple)):
            label_chunks = [c.reshape(-1) for c in labels.chunk(self.num_output_chunks, dim=1)]
            logit_chunks = [c.reshape(-1, c.size(-1)) for c in logits]
            if len(label_chunks) != len(logit_chunks):
                raise ValueError(f"{len(logit_chunks)} logit chunks vs {len(label_chunks)} label chunks")
            logits2d, labels1d = torch.cat(logit_chunks, dim=0), torch.cat(label_chunks, dim=0)
        else:
            logits2d, labels1d = logits.reshape(-1, logits.size(-1)), labels.reshape(-1)
        return _CrossEntropyFn.apply(logits2d, labels1d.contiguous(), self.ignore_index)


class _CrossEntropyFn(torch.autograd.Function):
    """Stand-alone CE over materialised logits (used when logits come from ``model(...)`` rather than the fused path)."""

    @staticmethod
    def forward(ctx, logits: Tensor, labels: Tensor, ignore_index: int) -> Tensor:
        rows, vocab = logits.shape
        ld = (vocab + 7) // 8 * 8
        work = torch.empty(rows, ld, dtype=logits.dtype, device=logits.device)
        work[:, :vocab].copy_(logits)
        row_loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
        ops.ce_fwd(work, labels, vocab, ignore_index, row_loss, None, ctx.needs_input_grad[0])
        out = torch.empty(4, dtype=torch.float32, device=logits.device)
        ops.ce_reduce(row_loss, labels, vocab, ignore_index, out)
        ctx.vocab = vocab
        ctx.save_for_backward(work, out)
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        work, out = ctx.saved_tensors
        ops.scale_(work, 1.0, (grad_out.to(torch.float32).reshape(1) / out[2:3]).contiguous())
        return work[:, : ctx.vocab], None, None


def _z_term(logits, labels: Tensor, ignore_index: int) -> Tensor:
    """``sum over valid labels of logsumexp(logits.float())^2 / n_valid`` in plain torch (the literal route's z-loss, coefficient not applied);
    ``logits``: one ``[B, S, V]`` tensor or the list of its chunks along ``S``."""
    chunks = logits if isinstance(logits, (list, tuple)) else [logits]
    lse = torch.cat([torch.logsumexp(c.float(), dim=-1) for c in chunks], dim=1)
    valid = labels != ignore_index
    return (lse * lse * valid).sum() / valid.sum()


def _uniform_term(logits, labels: Tensor, ignore_index: int) -> Tensor:
    """``sum over valid labels of (logsumexp(x) - mean(x)) / n_valid``, ``x = logits.float()``, in plain torch (the literal route's label
    smoothing: the cross-entropy against the uniform distribution, coefficient not applied); ``logits`` as for ``_z_term``."""
    chunks = logits if isinstance(logits, (list, tuple)) else [logits]
    u = torch.cat([torch.logsumexp(c.float(), dim=-1) - c.float().mean(dim=-1) for c in chunks], dim=1)
    valid = labels != ignore_index
    return (u * valid).sum() / valid.sum()


def kl_range_mask(labels: Tensor, ranges) -> Tensor | None:
    """Where the KL term against the teacher lives: a bool tensor shaped like the (shifted) ``labels``, true where the label id lies in one of
    the inclusive ``(lo, hi)`` pairs of ``ranges`` (as ``get_token_type_ranges`` gives them); ``None`` for ``ranges=None`` — every labelled
    position.  A few elementwise ops on the labels' device, no sync."""
    if ranges is None:
        return None
    mask = torch.zeros_like(labels, dtype=torch.bool)
    for lo, hi in ranges:
        mask |= (labels >= int(lo)) & (labels <= int(hi))
    return mask


def _kl_term(logits, teacher_logits, labels: Tensor, ignore_index: int, ranges) -> Tensor:
    """``sum over valid labels (inside ``ranges``) of KL(softmax(teacher_i) || softmax(logits_i)) / n_valid`` in plain torch (the literal
    route's teacher term, coefficient not applied); both logits as for ``_z_term``, chunked or not.  In fp64: against a teacher close to the
    model a row's KL is a small difference of two log-sum-exps, and their fp32 rounding (2.4e-7 at an lse of 6) would be 1e-4 of it."""
    x = torch.cat(list(logits), dim=1) if isinstance(logits, (list, tuple)) else logits
    t = torch.cat(list(teacher_logits), dim=1) if isinstance(teacher_logits, (list, tuple)) else teacher_logits
    kl = torch.nn.functional.kl_div(torch.log_softmax(x.double(), dim=-1), torch.log_softmax(t.double(), dim=-1), log_target=True,
                                    reduction="none").sum(dim=-1)
    valid = labels != ignore_index
    inside = kl_range_mask(labels, ranges)
    return (kl * (valid if inside is None else valid & inside)).sum() / valid.sum()


def check_loss_options(who: str, label_smoothing: float, z_loss_coeff: float, label_metrics=None, seq_scores=None,
                       under_grad: bool = False, teacher_kl_coeff: float = 0.0) -> tuple[float, float]:
    """The rules of the loss options, said once for ``compute_loss`` and ``model.fused_loss`` (``who``): both coefficients as floats in their
    ranges; neither combines with ``label_metrics`` or ``seq_scores`` (dev-set metrics and sequence scores are plain cross-entropy); and, with
    ``under_grad`` (a training forward of the fused route), those two forward-only forms are refused.  ``teacher_kl_coeff`` (finite, >= 0):
    ``> 0`` combines with none of the four — the KL term has a cross-entropy kernel form of its own, without the z-loss and the smoothing."""
    e, z, b = float(label_smoothing), float(z_loss_coeff), float(teacher_kl_coeff)
    if not (math.isfinite(b) and b >= 0.0):
        raise ValueError(f"teacher_kl_coeff must be finite and >= 0, got {b!r}")
    if b > 0.0:
        for name, on in (("label_metrics", label_metrics is not None), ("seq_scores", seq_scores is not None), ("z_loss_coeff", z > 0.0),
                         ("label_smoothing", e > 0.0)):
            if on:
                raise ValueError(f"{who}: teacher_kl_coeff and {name} do not combine in one call (the KL term against the teacher has a "
                                 "cross-entropy form of its own)")
    if not (math.isfinite(e) and 0.0 <= e < 1.0):
        raise ValueError(f"label_smoothing must be finite and in [0, 1), got {e!r}")
    if not (math.isfinite(z) and z >= 0.0):
        raise ValueError(f"z_loss_coeff must be finite and >= 0, got {z!r}")
    plain = [(name, what) for name, given, what in (("label_metrics", label_metrics, "the dev set's metrics are"),
                                                    ("seq_scores", seq_scores, "a sequence's score is")) if given is not None]
    if plain:
        name, what = plain[0]
        for coeff, value in (("label_smoothing", e), ("z_loss_coeff", z)):
            if value > 0.0:
                raise ValueError(f"{who}: {coeff} and {name} do not combine in one call ({what} plain cross-entropy)")
        if under_grad:
            raise RuntimeError(f"{who}({name}=...) is forward-only: call it under torch.no_grad() / inference_mode() or on model.eval(); "
                               "the training step's cross-entropy kernel does not rank labels")
    return e, z


def compute_loss(batch: dict[str, Tensor], model, loss_fn: Callable, label_metrics=None, z_loss_coeff: float = 0.0,
                 seq_scores=None, label_smoothing: float = 0.0, teacher=None, teacher_kl_coeff: float = 0.0, teacher_kl_ranges=None) -> Tensor:
    """``label_metrics`` (``ssi.eval.LabelMetrics``, forward-only, not in the reference): loss and top-k hits of the shifted labels are added to it
    per token type — by the cross-entropy kernel on the fused route, in plain torch from the logits on the literal one.  The loss is unchanged.
    ``z_loss_coeff`` (not in the reference; finite, >= 0): ``> 0`` adds the auxiliary z-loss ``z sum_i w_i logsumexp(logits_i)^2 / n_valid`` —
    inside the cross-entropy kernel on the fused route (``model.fused_loss``), in plain torch on the literal one.  Either route then leaves
    the two parts on the model as ``last_ce_loss`` and ``last_z_loss`` (detached scalars).  ``0.0``: exactly the loss of before.
    ``seq_scores`` (``ssi.eval.SeqScores``, forward-only, not in the reference): the sums of nll and top-k hits of the shifted labels over each
    of its sequences ``(row, start, end)`` of this batch are written to its ``out`` — by ``ssi_seq_score_reduce`` on the fused route, in
    plain torch from the logits on the literal one.  The loss is unchanged.  Not together with ``z_loss_coeff > 0``.
    ``label_smoothing`` (not in the reference; finite, in ``[0, 1)``): ``e > 0`` makes the objective that of
    ``F.cross_entropy(label_smoothing=e)``, ``(1 - e) ce + e mean_i (logsumexp(logits_i) - mean_c logits_ic)`` (+ the z part) — inside the
    cross-entropy kernel on the fused route, in plain torch on the literal one.  Either route leaves ``last_ce_loss`` (the plain
    cross-entropy) and ``last_smooth_loss`` (``e`` x the uniform part) on the model.  Not together with ``label_metrics`` or ``seq_scores``.
    ``0.0``: exactly the loss of before.
    ``teacher`` with ``teacher_kl_coeff`` (not in the reference; finite, >= 0): ``b > 0`` adds ``b sum_i k_i KL(teacher_i || model_i) / n_valid``
    on the next-token distributions against a frozen second model run on the same batch — inside the cross-entropy kernel on the fused route
    (``model.fused_loss``), in plain torch on ``teacher(...)`` logits on the literal one.  ``teacher_kl_ranges`` (inclusive ``(lo, hi)`` label-id
    pairs, or ``None``: every labelled position) says where the term lives.  Either route leaves ``last_ce_loss`` and ``last_kl_loss``
    (coefficient applied) on the model; the teacher gets no gradient.  Not together with the four options above.  ``0.0``: exactly the loss
    of before, and the teacher is not run."""
    label_smoothing, z_loss_coeff = check_loss_options("compute_loss", label_smoothing, z_loss_coeff, label_metrics, seq_scores,
                                                       teacher_kl_coeff=teacher_kl_coeff)
    teacher_kl_coeff = float(teacher_kl_coeff)
    if teacher_kl_coeff > 0.0 and teacher is None:
        raise ValueError("compute_loss: teacher_kl_coeff > 0 needs a teacher")
    labels = batch["labels"]
    ignore_index = loss_fn.ignore_index
    labels = torch.hstack((labels[..., 1:], torch.full_like(labels[..., -1:], ignore_index)))  # new tensor: batch untouched
    if (hasattr(model, "fused_loss") and isinstance(loss_fn, CEWithChunkedOutputLoss) and batch.get("encoder_input") is None
            and (batch.get("mask") is None or batch.get("input_pos") is not None)):
        # packed batches (ssi/data/packed.py) carry input_pos: block-causal attention, per-document RoPE positions
        extra = {}
        if batch.get("attn_plan") is not None:  # made on the host beside a packed batch (ssi/attn_plan.py): pipelined attention backward
            extra["attn_plan"] = batch["attn_plan"]
        if batch.get("loss_weights") is not None:  # an accumulation window run as one batch (ssi/data/window.py): weights per SHIFTED label
            extra["loss_weights"] = batch["loss_weights"]
        if label_metrics is not None:
            extra["label_metrics"] = label_metrics
        if z_loss_coeff > 0.0:
            extra["z_loss_coeff"] = z_loss_coeff
        if seq_scores is not None:
            extra["seq_scores"] = seq_scores
        if label_smoothing > 0.0:
            extra["label_smoothing"] = label_smoothing
        if teacher_kl_coeff > 0.0:
            extra.update(teacher=teacher, teacher_kl_coeff=teacher_kl_coeff, teacher_kl_ranges=teacher_kl_ranges)
        return model.fused_loss(batch["tokens"], labels, ignore_index, input_pos=batch.get("input_pos"), **extra)
    if batch.get("loss_weights") is not None:
        raise ValueError("loss_weights need the fused LM head + cross-entropy of the HIP decoder (model.fused_loss)")
    logits = model(
        tokens=batch["tokens"],
        mask=batch.get("mask"),
        encoder_input=batch.get("encoder_input"),
        encoder_mask=batch.get("encoder_mask"),
        input_pos=batch.get("input_pos"),
    )
    if label_metrics is not None:
        label_metrics.add_logits(logits, labels, ignore_index)
    if seq_scores is not None:
        seq_scores.add_logits(logits, labels, ignore_index)
    z_part = z_loss_coeff * _z_term(logits, labels, ignore_index) if z_loss_coeff > 0.0 else None
    u_part = label_smoothing * _uniform_term(logits, labels, ignore_index) if label_smoothing > 0.0 else None
    kl_part = None
    if teacher_kl_coeff > 0.0:
        with torch.no_grad():
            teacher_logits = teacher(tokens=batch["tokens"], mask=batch.get("mask"), encoder_input=batch.get("encoder_input"),
                                     encoder_mask=batch.get("encoder_mask"), input_pos=batch.get("input_pos"))
        kl_part = (teacher_kl_coeff * _kl_term(logits, teacher_logits, labels, ignore_index, teacher_kl_ranges)).float()
        del teacher_logits
    if not isinstance(logits, list):
        labels = labels.reshape(-1)
        logits = logits.reshape(-1, logits.size(-1))
    loss = loss_fn(logits, labels)
    del logits
    ce = loss
    if u_part is not None:
        model.last_ce_loss, model.last_smooth_loss = ce.detach(), u_part.detach()
        loss = (1.0 - label_smoothing) * ce + u_part
    if z_part is not None:
        model.last_ce_loss, model.last_z_loss = ce.detach(), z_part.detach()
        loss = loss + z_part
    if kl_part is not None:
        model.last_ce_loss, model.last_kl_loss = ce.detach(), kl_part.detach()
        loss = loss + kl_part
    return loss
