"""Generation on the HIP decoder — greedy, sampled and beam search (the reference generates with vLLM, ``scripts/generate.py``: greedy,
``n = 1``): what turns a checkpoint into the transcripts the reference's ``scripts/wer.py`` scores.

``generate`` sorts the prompts by length and runs them in static groups of ``batch_size``: one ``prefill`` per group (the packed forward
of the dev loss and of ``ssi.score``, block-causal over the prompts, every layer's K / V scattered into a cache by ``ssi_kv_store``), then
``decode_step`` per new token (one row per sequence on the training step's GEMMs, ``ssi_attn_decode`` over the cache).  A finished row
goes inert — its slot is masked to -1, so it costs no attention and writes no cache — and the group ends when every row has finished or
at ``max_new_tokens``; whether every row has finished is read back every ``READBACK_EVERY`` steps, not every step.

The three entry points check their own arguments and share ``_run_groups``; ``generate`` and ``sample`` run a group in the one ``_token_loop``,
given a chooser (``_Argmax``, ``_Select``, ``_Sample``: the step's tokens) and a stepper (``_own_slots``, ``_shared_prompt``: the next logits), each
built per group.  Beam search is another algorithm and keeps a loop of its own, ``_beam_group``.

Constraints (vLLM's ``allowed_token_ids`` and ``min_tokens``; both keep decoding greedy): with ``allowed_token_ids`` or ``min_new_tokens`` the
token of a step is the first maximum among the ALLOWED columns, from ``ssi_decode_select`` — one launch that also gives the token's
log-probability under the unconstrained distribution and its rank there (0: the constraint did not bind).  The stop tokens are always allowed;
none of them can be one of a row's first ``min_new_tokens`` tokens.  Without either argument the loop is the unconstrained one, launch for launch.

Beam search (``beam_search``; ``gen.beam_width`` in ``conf/generate.yaml`` — not a ``sampling_params`` key, as vLLM keeps ``BeamSearchParams``
apart): ``beam_width`` hypotheses per prompt are rows of one decode step.  They share the prompt's K / V and every generated position before
they diverged: ``decode_step_beam`` writes a row's K / V into a beam cache at (row, step) and reads through an ancestry table
(``ssi_attn_decode_beam``), so a reorder copies the small table and never the cache.  The ``beam_width`` best allowed continuations of a
row and the row's log-normaliser come from ``ssi_topk_logprob``; the bookkeeping of a step is a few ``[n_seq, ...]`` torch ops on the device.

Sampling (``sample``; ``gen.sample`` in ``conf/generate.yaml``): the token of a step is ``ssi_decode_sample``'s — a draw from
``softmax(x / temperature)`` over the allowed columns that top-k and then top-p keep, by Gumbel-max on counter-based random bits keyed by
``(seed, sequence, step)`` with ``sequence = prompt index in input order * n + sample index``.  How the prompts were grouped, sorted and batched
never enters the bits.  ``n = 1`` steps as ``generate`` does; ``n`` in 2..8 runs a prompt's samples as rows of ``decode_step_beam`` with the identity
ancestry, so the prompt is prefilled once and its K / V are shared as beams share them.

Penalties (vLLM's ``repetition_penalty``, ``frequency_penalty`` and ``presence_penalty``; arguments of ``generate`` and ``sample``,
``gen.penalties`` in ``conf/generate.yaml``): with any of them off its neutral value the token of a step comes from ``ssi_decode_select_pen`` /
``ssi_decode_sample_pen``, which choose on the penalised row — built in the kernel from the group's prompt table and the loop's own output
tensor, never stored — and report the log-probability (and the rank) of the raw one.  With all three neutral nothing of this runs.

Continuous batching (``continuous=True`` of ``generate`` and of ``sample`` with ``n = 1``; ``gen.continuous`` in ``conf/generate.yaml``):
``batch_size`` rows and cache slots form a pool; at a read-back the finished rows are harvested and queued prompts prefilled into their
slots (``prefill(slots=...)``), by a schedule that is host code (``PoolSchedule``).  The rows of a step then have different ages, so the
sampler runs on ``ssi_decode_sample_rows`` / ``ssi_decode_sample_pen_rows``, which take the step (and the draw parameters) per row; the same
entries serve per-prompt ``temperature`` / ``top_k`` / ``top_p`` lists in either mode.  Without the flag nothing of this runs.

Minimum-Bayes-risk selection (``mbr_select``; ``mbr=True`` of ``sample`` with ``n >= 2`` and of ``beam_search`` with ``n_best >= 2``;
``gen.mbr`` in ``conf/generate.yaml``): a prompt's candidates are reordered by their expected token error rate against each other, from the
edit distances of every unordered pair (``ssi_edit_distance``, one launch and one read-back per call).  Without the flag nothing of this runs.

Out of scope: per-row penalties, per-line parameters in the prompts JSONL, ``n > 8`` and ``best_of``, sampling
inside beam search, ``beam_width > 8``, sharing the prompt's K / V read among a prompt's beams, beam
search under data parallelism, pools for ``n > 1`` and for beams, paged caches, prefill rows mixed into a decode step (chunked prefill),
moving a draining pool of few live rows onto the skinny path, HIP graphs, generation under data parallelism; for MBR selection posterior
weights from ``cumulative_logprob``, word-level MBR and MBR under ``continuous``.  WER itself is ``ssi.wer`` and ``scripts/wer.py``."""

from __future__ import annotations

import json
import logging
from collections.abc import Sequence
from dataclasses import dataclass
from typing import Any

import numpy as np
import torch
from torch import Tensor

from . import ops
from .constants import CROSS_ENTROPY_IGNORE_IDX

LOGGER = logging.getLogger(__name__)

__all__ = ["Generation", "READBACK_EVERY", "MAX_BEAM_WIDTH", "MAX_SAMPLES", "plan_groups", "allowed_mask", "generate", "beam_search", "sample",
           "generate_file", "output_record", "check_greedy", "check_sampling", "check_penalties", "check_continuous", "ADMIT_MIN_DEFAULT", "PoolSchedule", "simulate_pool",
           "static_steps"]

READBACK_EVERY = 8    # decode steps between two read-backs of "has every row of the group finished?"
MAX_BEAM_WIDTH = 8    # the k of ssi_topk_logprob
MAX_SAMPLES = 8       # samples per prompt of ``sample``: the rows of a prompt in ``decode_step_beam``, as many as beams
ADMIT_MIN_DEFAULT = 32   # ``admit_min=None`` of the pool loop: the free rows an admission waits for (how it was chosen: README, "Continuous batching")


@dataclass
class Generation:
    """``token_ids``: the generated tokens, INCLUDING the stop token that ended it; ``finish_reason``: ``"stop"`` or ``"length"``;
    ``stop_reason``: the stop token's id, or None; ``cumulative_logprob``: the sum of the chosen tokens' log-probabilities (natural log;
    None without ``logprobs=True``); ``prompt_len``: tokens in the prompt; ``n_constrained``: the steps at which the constraint changed the
    choice (the chosen token was not the row's unconstrained first), None when no constraint was given — penalties count there: under
    ``generate`` with a penalty set it is the steps at which the mask OR the penalties changed the choice; ``score`` (``beam_search`` only):
    ``cumulative_logprob / len(token_ids) ** length_penalty``, what the hypotheses of a prompt are ordered by; ``n_kept_mean`` (``sample``
    only): the mean over the generated tokens of the size of the set each was drawn from (after the mask, top-k and top-p); ``mbr_risk``
    (``sample`` / ``beam_search`` with ``mbr=True`` only, None otherwise): the candidate's risk under ``mbr_select``.  It is set on the
    instance and is deliberately NOT a dataclass field: ``dataclasses.asdict`` of a Generation, which recorded results are compared by,
    stays what it was."""
    token_ids: list[int]
    finish_reason: str
    stop_reason: int | None
    cumulative_logprob: float | None
    prompt_len: int
    n_constrained: int | None = None
    score: float | None = None
    n_kept_mean: float | None = None
    mbr_risk = None
    mbr_index = None          # with mbr_risk: the candidate's position before the reorder


def plan_groups(lengths: Sequence[int], batch_size: int) -> list[list[int]]:
    """The static groups: prompt indices by rising length (ties by index), ``batch_size`` at a time.  Host only and deterministic."""
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1 (got {batch_size})")
    order = sorted(range(len(lengths)), key=lambda i: (lengths[i], i))
    return [order[a:a + batch_size] for a in range(0, len(order), batch_size)]


def allowed_mask(vocab_size: int, ids: Sequence[int] = (), ranges: Sequence[tuple[int, int]] = ()) -> Tensor:
    """Bool ``[vocab_size]``: True at every id of ``ids`` and of the inclusive ``(first, last)`` pairs of ``ranges`` (as
    ``get_token_type_ranges`` gives them).  ``ValueError`` for anything outside ``[0, vocab_size)``."""
    mask = torch.zeros(int(vocab_size), dtype=torch.bool)
    for first, last in ranges:
        first, last = int(first), int(last)
        if not 0 <= first <= last < vocab_size:
            raise ValueError(f"allowed_mask: the range ({first}, {last}) is not inside the vocabulary [0, {vocab_size})")
        mask[first:last + 1] = True
    ids = [int(t) for t in ids]
    bad = [t for t in ids if not 0 <= t < vocab_size]
    if bad:
        raise ValueError(f"allowed_mask: ids outside the vocabulary [0, {vocab_size}): {bad[:8]}")
    if ids:
        mask[torch.tensor(ids, dtype=torch.int64)] = True
    return mask


def _mask_words(mask: Tensor) -> Tensor:
    """The bit mask ``ssi_decode_select`` reads: int32 words, bit ``c % 32`` of word ``c // 32`` = ``mask[c]``."""
    words = (mask.numel() + 31) // 32
    bits = torch.zeros(words * 32, dtype=torch.int64)
    bits[:mask.numel()] = mask.to(torch.int64)
    w = (bits.view(words, 32) << torch.arange(32, dtype=torch.int64)).sum(1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


@dataclass
class _Constraint:
    """What a constrained loop needs on the device: the allowed set after ``min_new`` tokens and before (``early``: without the stop tokens;
    None when ``min_new == 0``), as bool vectors for the self-check and as the kernel's bit masks."""
    allow: Tensor
    allow_words: Tensor
    early: Tensor | None
    early_words: Tensor | None
    min_new: int


def _constraint_masks(vocab_size: int, allowed_token_ids, min_new_tokens: int, stop_token_ids: Sequence[int]) -> tuple[Tensor, Tensor] | None:
    """The host checks of ``allowed_token_ids`` / ``min_new_tokens``: (allowed with the stop tokens, allowed without them) as bool vectors on
    the CPU, or None when neither argument is set.  Every refusal is a ``ValueError``."""
    if min_new_tokens < 0:
        raise ValueError(f"min_new_tokens must be >= 0 (got {min_new_tokens})")
    if allowed_token_ids is None and min_new_tokens == 0:
        return None
    if allowed_token_ids is None:
        allow = torch.ones(vocab_size, dtype=torch.bool)
    elif isinstance(allowed_token_ids, Tensor) and allowed_token_ids.dtype == torch.bool:
        if tuple(allowed_token_ids.shape) != (vocab_size,):
            raise ValueError(f"allowed_token_ids as a mask is bool [{vocab_size}] (got {tuple(allowed_token_ids.shape)})")
        allow = allowed_token_ids.detach().cpu().clone()
    else:
        allow = allowed_mask(vocab_size, ids=[int(t) for t in allowed_token_ids])
    if not bool(allow.any()):
        raise ValueError("allowed_token_ids allows no token")
    stops = allowed_mask(vocab_size, ids=[int(t) for t in stop_token_ids])
    early = allow & ~stops
    if min_new_tokens > 0 and not bool(early.any()):
        raise ValueError(f"min_new_tokens = {min_new_tokens}, but nothing is allowed besides the stop tokens")
    return allow | stops, early


@dataclass
class _Penalty:
    r: float
    f: float
    p: float


def _check_penalties(repetition_penalty, frequency_penalty, presence_penalty) -> _Penalty | None:
    """The ranges of the three penalties (``ValueError``): ``repetition_penalty`` finite and > 0, the other two in [-2, 2].  None when all
    three are neutral (1, 0, 0): nothing of the penalised path then runs."""
    def number(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or abs(v) == float("inf"):
            raise ValueError(f"{name} = {v!r}: a finite number")
        return float(v)
    r, f, p = number("repetition_penalty", repetition_penalty), number("frequency_penalty", frequency_penalty), number("presence_penalty", presence_penalty)
    if not r > 0.0:
        raise ValueError(f"repetition_penalty = {r!r}: a finite number > 0")
    for name, v in (("frequency_penalty", f), ("presence_penalty", p)):
        if not -2.0 <= v <= 2.0:
            raise ValueError(f"{name} = {v!r}: a number in [-2, 2]")
    return None if (r, f, p) == (1.0, 0.0, 0.0) else _Penalty(r, f, p)


def _prompt_table(seqs: list[Tensor], dev) -> tuple[Tensor, Tensor]:
    """A group's prompts as the penalised kernels read them: int32 ``[len(seqs), longest]`` (zero-filled) and the int32 lengths."""
    lens = [int(s.numel()) for s in seqs]
    table = torch.zeros((len(seqs), max(lens)), dtype=torch.int32)
    for i, s in enumerate(seqs):
        table[i, :lens[i]] = s.to(torch.int32)
    return table.to(dev), torch.tensor(lens, dtype=torch.int32).to(dev)


def _constraint(masks: tuple[Tensor, Tensor] | None, min_new: int, dev) -> _Constraint | None:
    """What ``_constraint_masks`` returned, on the device (None stays None: no constraint)."""
    if masks is None:
        return None
    allow, early = (m.to(dev) for m in masks)
    return _Constraint(allow, _mask_words(masks[0]).to(dev), early if min_new else None, _mask_words(masks[1]).to(dev) if min_new else None, min_new)


def check_kv_cache_dtype(kv_cache_dtype) -> str | None:
    """``kv_cache_dtype`` of the three loops: None or "auto" (the model's dtype; not one launch, buffer or bit differs from a call without it) or
    "fp8" (``HipLlamaDecoder.new_kv_cache(..., dtype="fp8")``: vLLM's ``kv_cache_dtype="fp8"``, with one power-of-two scale per cached line);
    anything else is a ``ValueError`` before any launch.  Returns what ``new_kv_cache`` takes."""
    if kv_cache_dtype is None or (isinstance(kv_cache_dtype, str) and kv_cache_dtype in ("auto", "fp8")):
        return None if kv_cache_dtype in (None, "auto") else "fp8"
    raise ValueError(f"kv_cache_dtype = {kv_cache_dtype!r}: None, 'auto' or 'fp8'")


def check_weight_dtype(weight_dtype, small_batch: bool = True) -> str | None:
    """``weight_dtype`` of the three loops: None or "auto" (the model's weights; not one launch, buffer, summary key or bit differs from a call
    without it) or "fp8" (``HipLlamaDecoder.quantize_weights``: vLLM's ``quantization="fp8"``, with one power-of-two scale per output channel,
    read by the small-batch decode steps alone, so "fp8" without ``small_batch=True`` is refused); anything else is a ``ValueError`` before any launch."""
    if weight_dtype is None or (isinstance(weight_dtype, str) and weight_dtype in ("auto", "fp8")):
        if weight_dtype == "fp8" and not small_batch:
            raise ValueError("weight_dtype = 'fp8' without small_batch=True: FP8 weights serve the small-batch decode step alone")
        return None if weight_dtype in (None, "auto") else "fp8"
    raise ValueError(f"weight_dtype = {weight_dtype!r}: None, 'auto' or 'fp8'")


def _weight_source(model, weight_dtype, weight_quant, small_batch: bool):
    """None without FP8 weights; otherwise a function that hands out the quantised weights: the prebuilt ``weight_quant`` (checked against the
    model here, before any launch), or what ``model.quantize_weights()`` builds ONCE, when the first group that decodes on the skinny path asks."""
    if check_weight_dtype(weight_dtype, small_batch) is None:
        if weight_quant is not None:
            raise ValueError("weight_quant without weight_dtype='fp8'")
        return None
    if weight_quant is not None:
        model._check_weight_quant(weight_quant)
    built = [weight_quant]

    def source():
        if built[0] is None:
            built[0] = model.quantize_weights()
        return built[0]
    return source


def _new_cache(model, n_slots: int, cap: int, kv_dtype: str | None):
    """``model.new_kv_cache`` as it was always called, or of the kind ``check_kv_cache_dtype`` let through."""
    return model.new_kv_cache(n_slots, cap) if kv_dtype is None else model.new_kv_cache(n_slots, cap, dtype=kv_dtype)


def _small_batch_kw(model, rows: int, small_batch: bool, report: dict | None, split_kv: bool = False, weights=None) -> tuple[dict, dict]:
    """The keywords of a group of ``rows`` rows, decided once per group: (``prefill``'s, a decode step's).  Without a flag both are empty — the
    calls are then the plain ones, argument for argument.  With ``small_batch`` every step gets ``small_batch``, and a group that decodes on the
    skinny path prefills prompt by prompt (``separate``), so that nothing of a prompt's result depends on the prompts beside it; such a group is
    counted in ``report`` (the ``small_batch_groups`` of the run summary: what ran, counted where it ran).  ``split_kv`` likewise: every step
    gets ``split_kv``, and a group whose steps take the split-KV attention (``HipLlamaDecoder.takes_split_kv``) prefills prompt by prompt and is
    counted as one of the ``split_kv_groups``.  ``weights`` (``_weight_source``'s; only with ``small_batch``): a group that decodes on the skinny
    path gets ``weight_quant`` with every step and is counted as one of the ``fp8_weight_groups``; any other group is untouched."""
    prefill_kw, step_kw = {}, {}
    if weights is not None and model.takes_small_batch(rows, small_batch):
        step_kw["weight_quant"] = weights()
        if report is not None:
            report["fp8_weight_groups"] = report.get("fp8_weight_groups", 0) + 1
    for flag, on, takes in (("small_batch", small_batch, model.takes_small_batch if small_batch else None),
                            ("split_kv", split_kv, model.takes_split_kv if split_kv else None)):
        if not on:
            continue
        step_kw[flag] = True
        if takes(rows, True):
            prefill_kw = {"separate": True}
            if report is not None:
                report[flag + "_groups"] = report.get(flag + "_groups", 0) + 1
    return prefill_kw, step_kw


def _run_groups(model, prompts: Sequence[Any], per_group: int, max_new_tokens: int, stop_token_ids: Sequence[int], masks, min_new: int,
                open_caches, run_group) -> list:
    """What ``generate``, ``sample`` and ``beam_search`` do alike once their own arguments are checked: the prompts as tensors, the groups of
    ``per_group`` prompts, the length check (the last host check: every prompt, before the first launch), then under ``eval()`` and
    ``inference_mode`` one ``open_caches(n_slots, longest prompt)``, the constraint of ``masks`` on the device (``con``), and per group
    ``run_group(caches, con, seqs, index, stop)`` — ``index``: the prompts' places in the input, ``stop``: the stop tokens on the device —
    which returns one result per prompt.  Results in INPUT order."""
    seqs = [torch.as_tensor(p, dtype=torch.int64).reshape(-1) for p in prompts]
    lens = [int(s.numel()) for s in seqs]
    if not seqs:
        return []
    groups = plan_groups(lens, per_group)
    model.check_generation_lengths(lens, max_new_tokens, len(seqs), max(lens) + max_new_tokens)
    stop = torch.tensor(sorted({int(t) for t in stop_token_ids}), dtype=torch.int64, device=model.device)
    results: list = [None] * len(seqs)
    was_training = bool(model.training)
    model.eval()
    try:
        with torch.inference_mode():
            caches, con = open_caches(min(per_group, len(seqs)), max(lens)), _constraint(masks, min_new, model.device)
            for group in groups:
                for i, found in zip(group, run_group(caches, con, [seqs[i] for i in group], group, stop)):
                    results[i] = found
    finally:
        if was_training:
            model.train()
    return results


def _token_loop(choose, started, caches, refused: str, prompt_len: list[int], max_new: int, stop: Tensor, pad_id: int) -> list[Generation]:
    """One group of ``generate`` or ``sample``, one row per entry of ``prompt_len``.  The loop owns which rows are alive, their tokens and
    counts, the stop test and the read-back; ``choose(t, logits, alive, n_gen, out)`` gives the step's tokens (int64, >= 0) and ``started``
    is the prefill's logits with the stepper, ``step(t, tokens, alive)``: the next logits.  At the end what the ``caches`` refused is an
    error (``refused``: its message), then ``choose.finish`` raises its own and hands back the per-row fields it alone knows."""
    rows, dev = len(prompt_len), stop.device
    logits, step = started
    alive = torch.ones(rows, dtype=torch.bool, device=dev)
    out = torch.full((rows, max_new), pad_id, dtype=torch.int64, device=dev)
    n_gen = torch.zeros(rows, dtype=torch.int32, device=dev)       # (int32: what the selection kernels read)
    stop_tok = torch.full((rows,), -1, dtype=torch.int64, device=dev)
    for t in range(max_new):
        tok = choose(t, logits, alive, n_gen, out)
        out[:, t] = torch.where(alive, tok, out[:, t])
        n_gen += alive
        stopped = alive & torch.isin(tok, stop)
        stop_tok = torch.where(stopped, tok, stop_tok)
        alive = alive & ~stopped
        if t + 1 == max_new:
            break
        if (t + 1) % READBACK_EVERY == 0 and not bool(alive.any()):   # the read-back
            break
        logits = step(t, torch.where(alive, tok, torch.zeros_like(tok)), alive)
    host_out, host_n, host_stop = out.cpu(), n_gen.cpu().tolist(), stop_tok.cpu().tolist()
    errors = sum(int(c.errors) for c in caches)
    if errors != 0:
        raise RuntimeError(refused.format(errors))
    extras = choose.finish(host_n)
    return [Generation(token_ids=host_out[r, :host_n[r]].tolist(), finish_reason="stop" if host_stop[r] >= 0 else "length",
                       stop_reason=host_stop[r] if host_stop[r] >= 0 else None, prompt_len=prompt_len[r], **extras[r]) for r in range(rows)]


# ---- continuous batching: the pool of rows, refilled as sequences finish -------------------------------------------------------------
class PoolSchedule:
    """The schedule of a pool of ``pool`` rows (and cache slots), host only: which queued prompt enters which free row, and when.  The pool
    loop drives it with what the device reported; ``simulate_pool`` drives it with generated lengths known after the fact.

    ``order``: the queue, prompt numbers in the order they are admitted (``plan_groups``' order).  One decode step is one choice of a token by
    every live row.  After a step the host reads the device back (``reads_back``) every ``cadence`` steps, and also at the step by which every
    owned row must have ended (``max_new`` steps after its admission: a read-back that cannot come too early).  At a read-back the finished
    rows are released, and ``admit`` hands queued prompts the lowest free rows when ``free >= min(admit_min, queued)`` or no row is alive.
    ``report``: ``decode_steps``, ``row_steps_live`` (one per generated token), ``row_steps_total = decode_steps * pool``, ``admissions``."""

    def __init__(self, order: Sequence[int], pool: int, admit_min: int, max_new: int, cadence: int = READBACK_EVERY):
        pool, admit_min, max_new, cadence = int(pool), int(admit_min), int(max_new), int(cadence)
        if pool < 1 or admit_min < 1 or max_new < 1 or cadence < 1:
            raise ValueError(f"PoolSchedule: pool, admit_min, max_new and cadence must be >= 1 (got {pool}, {admit_min}, {max_new}, {cadence})")
        self.queue, self.pool, self.admit_min, self.max_new, self.cadence = [int(i) for i in order], pool, admit_min, max_new, cadence
        if len(set(self.queue)) != len(self.queue):
            raise ValueError("PoolSchedule: a prompt is queued twice")
        self.next = 0                                   # the queue's head
        self.owner = [-1] * pool                        # the prompt of a row; -1: free
        self.deadline = [0] * pool                      # the step count by which an owned row has ended
        self.decode_steps, self.row_steps_live = 0, 0
        self.admissions: list[list[tuple[int, int]]] = []      # per admission: (prompt, row)
        self.slot_of: dict[int, int] = {}

    @property
    def queued(self) -> int:
        return len(self.queue) - self.next

    def owned(self) -> list[int]:
        return [r for r, o in enumerate(self.owner) if o >= 0]

    def done(self) -> bool:
        return self.queued == 0 and not self.owned()

    def admit(self) -> list[tuple[int, int]]:
        free = [r for r, o in enumerate(self.owner) if o < 0]
        if self.queued == 0 or not free or (len(free) < min(self.admit_min, self.queued) and len(free) < self.pool):
            return []
        pairs = []
        for r in free[:self.queued]:
            i = self.queue[self.next]
            self.next += 1
            self.owner[r], self.deadline[r], self.slot_of[i] = i, self.decode_steps + self.max_new, r
            pairs.append((i, r))
        self.admissions.append(pairs)
        return pairs

    def stepped(self) -> None:
        self.decode_steps += 1

    def reads_back(self) -> bool:
        owned = self.owned()
        return self.decode_steps % self.cadence == 0 or (bool(owned) and self.decode_steps >= max(self.deadline[r] for r in owned))

    def release(self, row: int, n_generated: int) -> int:
        i = self.owner[row]
        if i < 0:
            raise ValueError(f"PoolSchedule: row {row} is free")
        self.owner[row] = -1
        self.row_steps_live += int(n_generated)
        return i

    def report(self) -> dict[str, int]:
        return {"decode_steps": self.decode_steps, "row_steps_live": self.row_steps_live, "row_steps_total": self.decode_steps * self.pool,
                "admissions": len(self.admissions)}


def simulate_pool(generated: Sequence[int], order: Sequence[int], pool: int, admit_min: int, max_new: int,
                  cadence: int = READBACK_EVERY) -> PoolSchedule:
    """The pool loop's schedule on the host: ``generated[i]`` (1 .. ``max_new``) is the number of tokens prompt ``i`` turns out to generate.
    Returns the finished ``PoolSchedule``: its ``admissions``, ``slot_of`` and ``report()`` are what the loop on the device arrives at."""
    sched = PoolSchedule(order, pool, admit_min, max_new, cadence)
    left = [0] * sched.pool
    for i, r in sched.admit():
        left[r] = int(generated[i])
    while not sched.done():
        sched.stepped()
        for r in sched.owned():
            left[r] = max(left[r] - 1, 0)
        if sched.reads_back():
            for r in sched.owned():
                if left[r] == 0:
                    sched.release(r, generated[sched.owner[r]])
            for i, r in sched.admit():
                left[r] = int(generated[i])
    return sched


def static_steps(generated: Sequence[int], groups: Sequence[Sequence[int]], max_new: int, cadence: int = READBACK_EVERY) -> int:
    """The decode steps of the static groups for the same lengths: a group runs until a read-back (every ``cadence`` steps) finds every row
    finished, ``max_new`` at the most — ``_token_loop``'s rule."""
    return sum(min(-(-max(generated[i] for i in g) // cadence) * cadence, max_new) for g in groups)


def _run_pool(model, prompts: Sequence[Any], pool: int, max_new: int, stop_token_ids: Sequence[int], masks, min_new: int, kv_dtype, admit_min,
              make_choose, refused: str, pad_id: int, small_batch: bool, report: dict | None, split_kv: bool, weights,
              stats: dict | None) -> list[Generation]:
    """``generate`` and ``sample`` (``n == 1``) under ``continuous=True``: ONE cache of ``pool`` slots, row ``r`` of every step is whatever
    sequence owns slot ``r`` (a free row is inert), and at a read-back the finished rows are harvested and queued prompts admitted into the
    free rows by ``PoolSchedule`` — one ``prefill(slots=...)``, whose logits rows replace those rows of the step's logits; the rows' state is
    reset, and their next choice is their step 0.  ``make_choose(seqs, pool, con)`` builds the chooser over the call's prompts.  Results in
    INPUT order; ``stats`` (a dict, or None) receives the schedule's report."""
    seqs = [torch.as_tensor(p, dtype=torch.int64).reshape(-1) for p in prompts]
    lens = [int(s.numel()) for s in seqs]
    if stats is not None:
        stats.update(continuous=True, decode_steps=0, row_steps_live=0, row_steps_total=0, admissions=0)
    if not seqs:
        return []
    pool = min(int(pool), len(seqs))
    sched = PoolSchedule([i for g in plan_groups(lens, pool) for i in g], pool, ADMIT_MIN_DEFAULT if admit_min is None else admit_min, max_new)
    model.check_generation_lengths(lens, max_new, len(seqs), max(lens) + max_new)
    dev = model.device
    stop = torch.tensor(sorted({int(t) for t in stop_token_ids}), dtype=torch.int64, device=dev)
    results: list = [None] * len(seqs)
    was_training = bool(model.training)
    model.eval()
    try:
        with torch.inference_mode():
            cache, con = _new_cache(model, pool, max(lens) + max_new, kv_dtype), _constraint(masks, min_new, dev)
            prefill_kw, step_kw = _small_batch_kw(model, pool, small_batch, report, split_kv, weights)
            choose = make_choose(seqs, pool, con)
            own = torch.arange(pool, dtype=torch.int32, device=dev)
            none = torch.full_like(own, -1)
            alive = torch.zeros(pool, dtype=torch.bool, device=dev)
            out = torch.full((pool, max_new), pad_id, dtype=torch.int64, device=dev)
            n_gen = torch.zeros(pool, dtype=torch.int32, device=dev)
            stop_tok = torch.full((pool,), -1, dtype=torch.int64, device=dev)
            logits = None

            def admit(pairs: list[tuple[int, int]]) -> None:
                nonlocal logits
                rows = torch.tensor([r for _, r in pairs], dtype=torch.int64, device=dev)
                new = model.prefill(cache, [seqs[i] for i, _ in pairs], max_new_tokens=max_new, slots=[r for _, r in pairs], **prefill_kw)
                if logits is None:
                    logits = new.new_zeros((pool, new.shape[1]))
                logits[rows] = new
                n_gen[rows], stop_tok[rows], out[rows], alive[rows] = 0, -1, pad_id, True
                choose.admit(rows, [i for i, _ in pairs])

            def harvest(host_alive: list[int], host_n: list[int]) -> None:
                done = [r for r in sched.owned() if not host_alive[r]]
                if not done:
                    return
                rows = torch.tensor(done, dtype=torch.int64, device=dev)
                host_out, host_stop = out[rows].cpu(), stop_tok[rows].cpu().tolist()
                extras = choose.harvest(rows, [host_n[r] for r in done])
                for j, r in enumerate(done):
                    i = sched.release(r, host_n[r])
                    results[i] = Generation(token_ids=host_out[j, :host_n[r]].tolist(), finish_reason="stop" if host_stop[j] >= 0 else "length",
                                            stop_reason=host_stop[j] if host_stop[j] >= 0 else None, prompt_len=lens[i], **extras[j])

            admit(sched.admit())
            limit = (len(seqs) + 1) * (max_new + sched.cadence)      # (every admitted row ends within max_new steps: never reached)
            while True:
                tok = choose(sched.decode_steps, logits, alive, n_gen, out)
                at = n_gen.long().clamp(max=max_new - 1)[:, None]
                out.scatter_(1, at, torch.where(alive, tok, out.gather(1, at)[:, 0])[:, None])
                n_gen += alive
                stopped = alive & torch.isin(tok, stop)
                stop_tok = torch.where(stopped, tok, stop_tok)
                alive = alive & ~stopped & (n_gen < max_new)
                sched.stepped()
                pairs, idle = [], False
                if sched.reads_back():                      # the read-back: one copy
                    host = torch.stack([alive.to(torch.int32), n_gen]).cpu().tolist()
                    harvest(*host)
                    if sched.done():
                        break
                    idle = not sched.owned()
                    pairs = sched.admit()
                if sched.decode_steps > limit:
                    raise RuntimeError("continuous batching: the pool did not drain (a row outlived max_new_tokens)")
                if not idle:                                # (nothing alive: the admitted rows' logits are all the next step reads)
                    logits = model.decode_step(cache, torch.where(alive, tok, torch.zeros_like(tok)), torch.where(alive, own, none), **step_kw)
                if pairs:
                    admit(pairs)
            errors = int(cache.errors)
            if errors != 0:
                raise RuntimeError(refused.format(errors))
            choose.close()
    finally:
        if was_training:
            model.train()
    if stats is not None:
        stats.update(sched.report())
    return results


def _check_continuous(who: str, continuous, admit_min) -> bool:
    """``continuous`` a bool, ``admit_min`` None (``ADMIT_MIN_DEFAULT``) or an integer >= 1 and only with ``continuous`` (``ValueError``)."""
    if not isinstance(continuous, bool):
        raise ValueError(f"{who}: continuous = {continuous!r}: True or False")
    if admit_min is not None and (isinstance(admit_min, bool) or not isinstance(admit_min, int) or admit_min < 1):
        raise ValueError(f"{who}: admit_min = {admit_min!r}: None or an integer >= 1")
    if admit_min is not None and not continuous:
        raise ValueError(f"{who}: admit_min without continuous=True")
    return continuous


# ---- the choosers: the token of a step ---------------------------------------------------------------------------------------------
class _Argmax:
    """``generate`` without constraint or penalty: ``argmax`` over the real columns, torch's first-occurrence rule.  With ``logprobs`` the
    forward-only ``ops.ce_fwd_metrics`` gives the token's log-probability, and its rank there is the free self-check."""

    def __init__(self, model, rows: int, logprobs: bool):
        dev = model.device
        self.V, self.rows, self.logprobs = model.vocab_size, rows, logprobs
        self.cum = torch.zeros(rows, dtype=torch.float64, device=dev)
        self.not_top = torch.zeros(1, dtype=torch.int64, device=dev)
        if logprobs:
            self.row_loss, self.row_nll = torch.empty(rows, dtype=torch.float32, device=dev), torch.empty(rows, dtype=torch.float32, device=dev)
            self.row_rank = torch.empty(rows, dtype=torch.int32, device=dev)

    def __call__(self, t: int, logits: Tensor, alive: Tensor, n_gen: Tensor, out: Tensor) -> Tensor:
        tok = logits[:, :self.V].argmax(dim=-1)
        if self.logprobs:
            labels = torch.where(alive, tok, torch.full_like(tok, CROSS_ENTROPY_IGNORE_IDX))
            ops.ce_fwd_metrics(logits, labels, self.V, CROSS_ENTROPY_IGNORE_IDX, self.row_loss, None, self.row_nll, self.row_rank)
            self.cum -= torch.where(alive, self.row_nll, torch.zeros_like(self.row_nll)).double()
            self.not_top += (alive & (self.row_rank != 0)).sum()      # the free self-check: the chosen token is the row's first
        return tok

    def finish(self, host_n: list[int]) -> list[dict]:
        self.close()
        host_cum = self.cum.cpu().tolist() if self.logprobs else [None] * self.rows
        return [dict(cumulative_logprob=c) for c in host_cum]

    # the pool loop (``continuous=True``): a row starts a new sequence, a finished row hands over its fields, the end-of-call check runs once
    def admit(self, rows: Tensor, prompts: list[int]) -> None:
        self.cum[rows] = 0.0

    def harvest(self, rows: Tensor, host_n: list[int]) -> list[dict]:
        host_cum = self.cum[rows].cpu().tolist() if self.logprobs else [None] * len(host_n)
        return [dict(cumulative_logprob=c) for c in host_cum]

    def close(self) -> None:
        if int(self.not_top) != 0:
            raise RuntimeError(f"generate: on {int(self.not_top)} rows the chosen token was not ranked first by ce_fwd_metrics")


class _Selection:
    """What ``_Select`` and ``_Sample`` share: the token and log-probability buffers, the mask and penalty keywords of a launch, the self-check
    "every live row's token is >= 0 and allowed", and the group's end.  ``who`` names the entry point in the messages; ``pen`` set: the
    penalised kernel, on the group's prompt table (row ``r`` reads line ``prompt_row[r]``; None: line ``r``)."""

    def __init__(self, who: str, model, seqs: list[Tensor], rows: int, con: _Constraint | None, pen: _Penalty | None, logprobs: bool = True,
                 prompt_row: Tensor | None = None):
        dev = model.device
        self.who, self.V, self.con, self.hist = who, int(model.vocab_size), con, None
        self.tok = torch.empty(rows, dtype=torch.int64, device=dev)
        self.row_lp = torch.empty(rows, dtype=torch.float32, device=dev) if logprobs else None
        self.cum = torch.zeros(rows, dtype=torch.float64, device=dev)
        self.bad = torch.zeros(1, dtype=torch.int64, device=dev)
        if pen is not None:
            ptab, plen = _prompt_table(seqs, dev)
            self.n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
            self.hist = dict(prompt_ids=ptab, prompt_len=plen, **({} if prompt_row is None else {"prompt_row": prompt_row}),
                             repetition_penalty=pen.r, frequency_penalty=pen.f, presence_penalty=pen.p, n_bad=self.n_bad)

    def launch_kw(self, n_gen: Tensor, out: Tensor) -> dict:
        """The mask and penalty keywords of a selection launch.  No constraint and no penalty: none at all; ``n_generated`` is None under a
        constraint without ``min_new`` (nothing reads it then) and always there under a penalty, with the loop's tokens as ``gen_ids``."""
        con = self.con
        kw = {} if con is None else dict(n_generated=n_gen if con.min_new else None, allow=con.allow_words, allow_early=con.early_words, min_new=con.min_new)
        return kw if self.hist is None else dict(kw, n_generated=n_gen, gen_ids=out, **self.hist)

    def refused(self, at: Tensor, n_gen: Tensor) -> Tensor:
        """Per row: the kernel chose no token, or one that is not allowed (``at``: the tokens clamped to >= 0)."""
        none, con = self.tok < 0, self.con
        if con is None:
            return none
        return none | ~(con.allow[at] if con.early is None else torch.where(n_gen < con.min_new, con.early[at], con.allow[at]))

    def admit(self, rows: Tensor, prompts: list[int]) -> None:
        """The pool loop: ``rows`` start the sequences of ``prompts`` (their places in the input, which are the lines of the call's one prompt
        table); a chooser resets its own per-row sums on top."""
        self.cum[rows] = 0.0
        if self.hist is not None:
            self.hist["prompt_row"][rows] = torch.tensor(prompts, dtype=torch.int32).to(rows.device)

    def close(self) -> None:
        self.check()

    def check(self) -> None:
        if self.hist is not None and int(self.n_bad) != 0:
            raise RuntimeError(f"{self.who}: on {int(self.n_bad)} row-steps the penalised selection met an id outside the vocabulary in the row's history")
        if int(self.bad) != 0:
            raise RuntimeError(f"{self.who}: on {int(self.bad)} rows {self.refusal}")


class _Select(_Selection):
    """``generate`` under a constraint or a penalty: ``ops.decode_select`` / ``ops.decode_select_pen`` — the first allowed maximum, its
    log-probability over ALL columns and its rank in the raw row (not 0: the mask or the penalties changed the choice)."""
    refusal = "decode_select chose no token or one that is not allowed"

    def __init__(self, model, seqs: list[Tensor], con: _Constraint | None, pen: _Penalty | None, logprobs: bool, pool: int | None = None):
        """``pool`` (the pool loop): that many rows over the prompt table of the whole call, the line of a row set when it is admitted."""
        rows = len(seqs) if pool is None else pool
        line = torch.zeros(rows, dtype=torch.int32, device=model.device) if pool is not None and pen is not None else None
        super().__init__("generate", model, seqs, rows, con, pen, logprobs, prompt_row=line)
        self.row_rank = torch.empty(rows, dtype=torch.int32, device=model.device)
        self.n_con = torch.zeros(rows, dtype=torch.int64, device=model.device)

    def __call__(self, t: int, logits: Tensor, alive: Tensor, n_gen: Tensor, out: Tensor) -> Tensor:
        select = ops.decode_select if self.hist is None else ops.decode_select_pen
        select(logits, self.V, self.tok, self.row_lp, self.row_rank, **self.launch_kw(n_gen, out))
        at = self.tok.clamp(min=0)                      # (a new tensor per step, as argmax gives; never a negative embedding index)
        self.bad += (alive & self.refused(at, n_gen)).sum()
        self.n_con += alive & (self.row_rank != 0)
        if self.row_lp is not None:
            self.cum += torch.where(alive, self.row_lp, torch.zeros_like(self.row_lp)).double()
        return at

    def finish(self, host_n: list[int]) -> list[dict]:
        self.check()
        host_cum = self.cum.cpu().tolist() if self.row_lp is not None else [None] * len(host_n)
        return [dict(cumulative_logprob=c, n_constrained=k) for c, k in zip(host_cum, self.n_con.cpu().tolist())]

    def admit(self, rows: Tensor, prompts: list[int]) -> None:
        super().admit(rows, prompts)
        self.n_con[rows] = 0

    def harvest(self, rows: Tensor, host_n: list[int]) -> list[dict]:
        host_cum = self.cum[rows].cpu().tolist() if self.row_lp is not None else [None] * len(host_n)
        return [dict(cumulative_logprob=c, n_constrained=k) for c, k in zip(host_cum, self.n_con[rows].cpu().tolist())]


class _Sample(_Selection):
    """``sample``: ``ops.decode_sample`` / ``ops.decode_sample_pen`` with ``step`` the loop index and ``sequence`` the rows' numbers — row
    ``s * n + j`` is sample ``j`` of the group's prompt ``s``, whose place in the input is ``index[s]``.  The self-check adds "drawn from a set of
    at least one column"."""
    refusal = "decode_sample chose no token, one that is not allowed, or kept no column"

    def __init__(self, model, seqs: list[Tensor], index: list[int], n: int, draw: dict, con: _Constraint | None, pen: _Penalty | None,
                 pool: int | None = None):
        """``draw``: what ``_check_draws`` returned — with scalars alone (and no ``pool``) the launches are the scalar entries', argument for
        argument; a per-prompt value (a float64 / int64 tensor over ALL prompts of the call, on the CPU) or ``pool`` takes the ``_rows``
        entries, with ``step = n_gen`` per row.  ``pool`` (the pool loop; ``n == 1``): that many rows over the prompt table of the whole call;
        a row's sequence number, prompt line and draw parameters are set when it is admitted (``index`` is not read)."""
        dev, rows = model.device, (len(seqs) * n if pool is None else pool)
        if pool is None:
            line = torch.arange(rows, dtype=torch.int32, device=dev) // n if pen is not None else None
            number = (torch.tensor(index, dtype=torch.int64) * n).repeat_interleave(n) + torch.arange(n, dtype=torch.int64).repeat(len(seqs))
        else:
            line = torch.zeros(rows, dtype=torch.int32, device=dev) if pen is not None else None
            number = torch.zeros(rows, dtype=torch.int64)
        super().__init__("sample", model, seqs, rows, con, pen, prompt_row=line)
        self.sequence = self._words(number).to(dev)
        self.per_prompt = {k: v.to(dev) for k, v in draw.items() if isinstance(v, Tensor)}
        self.by_row = pool is not None or bool(self.per_prompt)
        self.draw = dict(draw)
        for k, v in self.per_prompt.items():              # the row's own value: of its prompt in a static group, set on admission in a pool
            self.draw[k] = v[torch.tensor(index, dtype=torch.int64, device=dev)].repeat_interleave(n) if pool is None else torch.ones(rows, dtype=v.dtype, device=dev)
        self.row_kept = torch.empty(rows, dtype=torch.int32, device=dev)
        self.kept_sum = torch.zeros(rows, dtype=torch.int64, device=dev)

    @staticmethod
    def _words(number: Tensor) -> Tensor:
        return torch.where(number >= 2 ** 31, number - 2 ** 32, number).to(torch.int32)      # (the kernel reads it as unsigned)

    def __call__(self, t: int, logits: Tensor, alive: Tensor, n_gen: Tensor, out: Tensor) -> Tensor:
        if self.by_row:     # a live row of a static group is at step t == n_gen; the rows of a pool have their own ages
            sample = ops.decode_sample_rows if self.hist is None else ops.decode_sample_pen_rows
            sample(logits, self.V, self.tok, self.row_lp, self.row_kept, step=n_gen, sequence=self.sequence, **self.launch_kw(n_gen, out), **self.draw)
        else:
            sample = ops.decode_sample if self.hist is None else ops.decode_sample_pen
            sample(logits, self.V, self.tok, self.row_lp, self.row_kept, step=t, sequence=self.sequence, **self.launch_kw(n_gen, out), **self.draw)
        at = self.tok.clamp(min=0)                      # (a new tensor per step; never a negative embedding index)
        self.bad += (alive & (self.refused(at, n_gen) | (self.row_kept < 1))).sum()
        self.cum += torch.where(alive, self.row_lp, torch.zeros_like(self.row_lp)).double()
        self.kept_sum += torch.where(alive, self.row_kept, torch.zeros_like(self.row_kept))
        return at

    def finish(self, host_n: list[int]) -> list[dict]:
        host_cum, host_kept = self.cum.cpu().tolist(), self.kept_sum.cpu().tolist()
        self.check()
        return [dict(cumulative_logprob=c, n_kept_mean=k / max(m, 1)) for c, k, m in zip(host_cum, host_kept, host_n)]

    def admit(self, rows: Tensor, prompts: list[int]) -> None:
        super().admit(rows, prompts)
        self.kept_sum[rows] = 0
        at = torch.tensor(prompts, dtype=torch.int64)
        self.sequence[rows] = self._words(at).to(rows.device)
        for k, v in self.per_prompt.items():
            self.draw[k][rows] = v[at.to(rows.device)]

    def harvest(self, rows: Tensor, host_n: list[int]) -> list[dict]:
        host_cum, host_kept = self.cum[rows].cpu().tolist(), self.kept_sum[rows].cpu().tolist()
        return [dict(cumulative_logprob=c, n_kept_mean=k / max(m, 1)) for c, k, m in zip(host_cum, host_kept, host_n)]


# ---- the steppers: the next logits -------------------------------------------------------------------------------------------------
def _own_slots(model, caches, seqs: list[Tensor], max_new: int, small_batch: bool, report: dict | None, split_kv: bool = False, weights=None):
    """Row ``r`` is prompt ``r`` and decodes on slot ``r`` of the one cache: ``prefill`` with room for the new tokens, then ``decode_step``.
    Returns the prefill's logits and the stepper."""
    prefill_kw, step_kw = _small_batch_kw(model, len(seqs), small_batch, report, split_kv, weights)
    logits = model.prefill(caches[0], seqs, max_new_tokens=max_new, **prefill_kw)
    own = torch.arange(len(seqs), dtype=torch.int32, device=model.device)
    none = torch.full_like(own, -1)
    return logits, lambda t, tokens, alive: model.decode_step(caches[0], tokens, torch.where(alive, own, none), **step_kw)


def _shared_prompt(model, caches, seqs: list[Tensor], n: int, max_new: int, small_batch: bool, report: dict | None, split_kv: bool = False,
                   weights=None):
    """Row ``s * n + j`` is continuation ``j`` of prompt ``s``: the prompt is prefilled once into the prompt cache, its logits row repeated
    ``n`` times for step 0, and the rows run on ``decode_step_beam`` with the identity ancestry — a row reads its own generated positions."""
    rows, dev = len(seqs) * n, model.device
    prefill_kw, step_kw = _small_batch_kw(model, rows, small_batch, report, split_kv, weights)
    logits = model.prefill(caches[0], seqs, **prefill_kw)[:len(seqs)].repeat_interleave(n, dim=0)
    own = torch.arange(rows, dtype=torch.int32, device=dev)
    seq_of, none = own // n, torch.full_like(own, -1)
    plen = torch.tensor([int(s.numel()) for s in seqs], dtype=torch.int32).to(dev).repeat_interleave(n)
    anc = own[:, None].expand(rows, max_new).contiguous()
    return logits, lambda t, tokens, alive: model.decode_step_beam(*caches, tokens, torch.where(alive, seq_of, none), plen, anc, t, **step_kw)


def generate(model, prompts: Sequence[Any], *, max_new_tokens: int, stop_token_ids: Sequence[int], pad_id: int, batch_size: int = 256,
             logprobs: bool = False, device: torch.device | str | None = None, allowed_token_ids: Sequence[int] | Tensor | None = None,
             min_new_tokens: int = 0, repetition_penalty: float = 1.0, frequency_penalty: float = 0.0,
             presence_penalty: float = 0.0, small_batch: bool = False, small_batch_report: dict | None = None,
             split_kv: bool = False, kv_cache_dtype: str | None = None, weight_dtype: str | None = None, weight_quant=None,
             continuous: bool = False, admit_min: int | None = None, continuous_report: dict | None = None) -> list[Generation]:
    """Greedy continuation of every prompt (1-D integer sequences), results in INPUT order.  The token of a step is ``argmax`` over the real
    columns ``[:, :vocab_size]`` of the step's logits, with torch's first-occurrence rule.  ``pad_id`` fills the rows that have finished.
    ``logprobs=True``: the forward-only ``ops.ce_fwd_metrics`` runs on the step's logits with the chosen token as label, which gives its
    log-probability with no new kernel; the label's rank it also writes must be 0 on every live row (``RuntimeError`` otherwise).
    ``allowed_token_ids`` (ids, or a bool ``[vocab_size]`` mask; the stop tokens are always added) and ``min_new_tokens`` (no stop token among
    a row's first so many tokens): the token of a step, the first included, is ``ops.decode_select``'s — the first maximum among the allowed
    columns — and with ``logprobs=True`` the sum is of that kernel's log-probabilities, which are over ALL columns (``ops.ce_fwd_metrics`` is
    not launched); the self-check is "every live row's token is >= 0 and allowed".  With neither, nothing of the above runs.
    ``repetition_penalty``, ``frequency_penalty``, ``presence_penalty`` (vLLM's; neutral at 1, 0, 0): with any of them set the token of a step
    is ``ops.decode_select_pen``'s — the first allowed maximum of the penalised row, with NULL masks when there is no constraint — in place of
    ``argmax`` and the cross-entropy launch; the log-probabilities stay those of the raw row, and ``n_constrained`` counts the steps whose
    token was not the raw row's first.  An id the kernel had to skip (outside the vocabulary) is a ``RuntimeError`` at the end of the group.
    ``small_batch``: handed to every ``decode_step`` of every group; a group of 1 to ``model.skinny_max_rows`` rows then decodes unpadded on the
    skinny GEMMs (``HipLlamaDecoder.takes_small_batch``), a larger one takes the tile path by itself.  A row's tokens and log-probabilities do
    not depend on the rows beside it.  ``False``: not one launch or buffer differs.  ``small_batch_report`` (a dict, or None): every group that
    took the skinny path adds 1 to its ``"small_batch_groups"``.
    ``split_kv``: handed to every ``decode_step`` of every group; a group of 1 to ``model.split_max_rows`` rows then runs the split-KV decode
    attention (``HipLlamaDecoder.takes_split_kv``) and prefills prompt by prompt, and adds 1 to ``"split_kv_groups"`` of ``small_batch_report``.
    A row still depends on itself alone, but its bits depend on whether its group splits: tokens and ``cumulative_logprob`` are bit-equal among
    groups on the same side of ``split_max_rows`` (as for ``skinny_max_rows``).  ``False``: not one launch or buffer differs.
    ``kv_cache_dtype``: None or "auto" — the caches hold the model's dtype; "fp8" — they hold e4m3 codes with one power-of-two exponent per cached
    line (``check_kv_cache_dtype``): the store and the attention of every step are the ``_fp8`` entries, the prompt's own attention in ``prefill``
    runs on the unquantised K / V, and values change (opt-in).  Orthogonal to ``small_batch`` and ``split_kv``.
    ``weight_dtype``: None or "auto" — the model's weights; "fp8" (only with ``small_batch=True``; ``check_weight_dtype``) — every group that decodes
    on the skinny path reads the layer GEMMs' weights and the head as e4m3 codes with one power-of-two exponent per output channel
    (``HipLlamaDecoder.quantize_weights``) and adds 1 to ``"fp8_weight_groups"`` of ``small_batch_report``; ``prefill``, the embedding gather and
    every other group run on the bf16 weights, and values change (opt-in).  ``weight_quant``: a ``QuantWeights`` built before, to reuse it across
    calls; without it one is built in the call, when the first such group starts.
    ``continuous`` (continuous batching; opt-in): ``batch_size`` is then a POOL of that many rows and cache slots over one cache of
    ``max(lens) + max_new_tokens`` positions; the queue is ``plan_groups``' order, a finished row is harvested at the next read-back and a
    queued prompt prefilled into its slot (``prefill(slots=...)``; ``PoolSchedule``), so a row of a step is whatever sequence owns its slot.
    ``admit_min`` (None: ``ADMIT_MIN_DEFAULT``): an admission waits for ``min(admit_min, queued)`` free rows, or for the pool to be empty.
    A pool that takes the small-batch path (``batch_size <= skinny_max_rows`` with ``small_batch=True``) admits prompt by prompt, and a
    prompt's tokens and ``cumulative_logprob`` are then bit-equal to the static ``small_batch`` run's whatever the pool size, ``admit_min`` and
    the input order (with ``split_kv``: against static groups on the same side of ``split_max_rows``); a larger pool admits packed, and packing
    enters a prompt's bits as it does in a static group.  ``continuous_report`` (a dict, or None) receives ``continuous``, ``decode_steps``,
    ``row_steps_live``, ``row_steps_total`` and ``admissions``.  ``False``: not one launch, buffer or bit differs.
    Refused before any launch (``ValueError``): a penalty outside its range, an empty prompt, a prompt that with ``max_new_tokens`` exceeds the model's RoPE table or
    ``max_seq_len``; ``min_new_tokens < 0``, an allowed or stop id outside the vocabulary (under a constraint), an empty allowed set,
    ``min_new_tokens > 0`` with nothing allowed besides the stop tokens."""
    max_new_tokens, batch_size, min_new_tokens = int(max_new_tokens), int(batch_size), int(min_new_tokens)
    kv_dtype = check_kv_cache_dtype(kv_cache_dtype)
    weights = _weight_source(model, weight_dtype, weight_quant, small_batch)
    pen = _check_penalties(repetition_penalty, frequency_penalty, presence_penalty)
    masks = _constraint_masks(int(model.vocab_size), allowed_token_ids, min_new_tokens, stop_token_ids)
    if max_new_tokens < 1:
        raise ValueError(f"max_new_tokens must be >= 1 (got {max_new_tokens})")
    device = torch.device(device) if device is not None else model.device
    if device != model.device:
        raise ValueError(f"generate: device {device} is not the model's ({model.device})")
    refused = "generate: the K/V cache kernels refused {} rows (a destination or a slot outside the cache)"
    if _check_continuous("generate", continuous, admit_min):
        if batch_size < 1:
            raise ValueError(f"batch_size must be >= 1 (got {batch_size})")

        def make_choose(seqs, pool, con):
            return _Argmax(model, pool, logprobs) if con is None and pen is None else _Select(model, seqs, con, pen, logprobs, pool=pool)

        return _run_pool(model, prompts, batch_size, max_new_tokens, stop_token_ids, masks, min_new_tokens, kv_dtype, admit_min, make_choose,
                         refused, int(pad_id), small_batch, small_batch_report, split_kv, weights, continuous_report)

    def run_group(caches, con, seqs: list[Tensor], index: list[int], stop: Tensor) -> list[Generation]:
        started = _own_slots(model, caches, seqs, max_new_tokens, small_batch, small_batch_report, split_kv, weights)
        choose = _Argmax(model, len(seqs), logprobs) if con is None and pen is None else _Select(model, seqs, con, pen, logprobs)
        return _token_loop(choose, started, caches, refused, [int(s.numel()) for s in seqs], max_new_tokens, stop, int(pad_id))

    return _run_groups(model, prompts, batch_size, max_new_tokens, stop_token_ids, masks, min_new_tokens,
                       lambda n_slots, longest: (_new_cache(model, n_slots, longest + max_new_tokens, kv_dtype),), run_group)


# ---- minimum-Bayes-risk selection ------------------------------------------------------------------------------------------------
def mbr_select(candidates: Sequence[Sequence[Sequence[int]]], device) -> tuple[list[list[int]], list[list[float]]]:
    """Minimum-Bayes-risk order of every prompt's candidates (``candidates[p][k]``: the token ids of candidate ``k`` of prompt ``p``, at
    least two per prompt).  ``risk_k = (1 / (n - 1)) * sum_{j != k} dist(c_j, c_k) / max(1, len(c_j))``: the expected token error rate of
    ``c_k`` with the other candidates as equally weighted pseudo-references.  ``dist`` is symmetric, so every unordered pair is computed
    once, all prompts in one ``ssi_edit_distance`` launch; the sum is taken in float64 on the device, over ``j`` in index order (one add per
    candidate position, so the bits do not depend on a reduction's shape), and read back once.
    Returns ``(order, risk)``: ``order[p]`` the candidate indices by rising risk, then by index (``order[p][0]`` is the first minimum);
    ``risk[p][k]`` the risk of candidate ``k`` (input order)."""
    from .wer import edit_distance_pairs
    cands = [list(cs) for cs in candidates]
    if any(len(cs) < 2 for cs in cands):
        raise ValueError("mbr_select: every prompt needs at least two candidates (the risk of one candidate against no other is undefined)")
    if not cands:
        return [], []
    dev = torch.device(device)
    seqs = [c for cs in cands for c in cs]
    base, pairs, width = 0, [], max(len(cs) for cs in cands)
    other = np.full((len(seqs), width), -1, dtype=np.int64)                # [candidate k, position j] -> its pair, -1 where j == k or absent
    ref_of = np.zeros((len(seqs), width), dtype=np.int64)                  # ... -> the flat index of candidate j
    for cs in cands:
        n = len(cs)
        for j in range(n):
            ref_of[base:base + n, j] = base + j
            for k in range(j + 1, n):
                other[base + k, j] = other[base + j, k] = len(pairs)
                pairs.append((base + j, base + k))
        base += n
    dist = edit_distance_pairs(seqs, pairs, dev)[:, 0].to(torch.float64)
    length = torch.tensor([max(1, len(c)) for c in seqs], dtype=torch.float64).to(dev)
    count = torch.tensor([len(cs) - 1 for cs in cands for _ in cs], dtype=torch.float64).to(dev)
    other, ref_of = torch.from_numpy(other).to(dev), torch.from_numpy(ref_of).to(dev)
    term = torch.where(other >= 0, dist[other.clamp(min=0)] / length[ref_of], torch.zeros((), dtype=torch.float64, device=dev))
    risk = torch.zeros(len(seqs), dtype=torch.float64, device=dev)
    for j in range(width):
        risk = risk + term[:, j]
    flat = (risk / count).tolist()                                         # the read-back
    order, risks, base = [], [], 0
    for cs in cands:
        r = flat[base:base + len(cs)]
        base += len(cs)
        risks.append(r)
        order.append(sorted(range(len(cs)), key=lambda k: (r[k], k)))
    return order, risks


def mbr_candidate(gen: Generation) -> list[int]:
    """What MBR compares: the generated ids up to and without the stop token."""
    return list(gen.token_ids[:-1] if gen.finish_reason == "stop" else gen.token_ids)


def _mbr_reorder(found: list[list[Generation]], device) -> list[list[Generation]]:
    """Every prompt's Generations in ``mbr_select``'s order, ``mbr_risk`` set and ``mbr_index`` (the position before the reorder) beside it."""
    order, risks = mbr_select([[mbr_candidate(g) for g in gs] for gs in found], device)
    out = []
    for gs, o, r in zip(found, order, risks):
        for k, g in enumerate(gs):
            g.mbr_risk, g.mbr_index = r[k], k
        out.append([gs[k] for k in o])
    return out


def _check_mbr(who: str, mbr, n: int, what: str) -> bool:
    if not isinstance(mbr, bool):
        raise ValueError(f"{who}: mbr = {mbr!r}: True or False")
    if mbr and n < 2:
        raise ValueError(f"{who}: mbr=True needs at least two candidates per prompt ({what} = {n})")
    return mbr


# ---- beam search -----------------------------------------------------------------------------------------------------------------
def _check_beam(beam_width, length_penalty, n_best) -> tuple[int, float, int]:
    """The ranges of the three beam arguments (``ValueError``): ``1 <= n_best <= beam_width <= MAX_BEAM_WIDTH``, ``length_penalty`` finite, >= 0."""
    for name, v in (("beam_width", beam_width), ("n_best", n_best)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name} = {v!r}: an integer")
    if not 1 <= beam_width <= MAX_BEAM_WIDTH:
        raise ValueError(f"beam_width = {beam_width}: 1 to {MAX_BEAM_WIDTH}")
    if not 1 <= n_best <= beam_width:
        raise ValueError(f"n_best = {n_best}: 1 to beam_width ({beam_width})")
    if isinstance(length_penalty, bool) or not isinstance(length_penalty, (int, float)) or not 0.0 <= float(length_penalty) < float("inf"):
        raise ValueError(f"length_penalty = {length_penalty!r}: a finite number >= 0")
    return beam_width, float(length_penalty), n_best


def beam_search(model, prompts: Sequence[Any], *, beam_width: int, max_new_tokens: int, stop_token_ids: Sequence[int], pad_id: int,
                length_penalty: float = 1.0, n_best: int = 1, allowed_token_ids: Sequence[int] | Tensor | None = None, min_new_tokens: int = 0,
                batch_size: int = 256, repetition_penalty: float = 1.0, frequency_penalty: float = 0.0,
                presence_penalty: float = 0.0, small_batch: bool = False, small_batch_report: dict | None = None,
             split_kv: bool = False, kv_cache_dtype: str | None = None, weight_dtype: str | None = None,
             weight_quant=None, continuous: bool = False, admit_min: int | None = None, mbr: bool = False) -> list[list[Generation]]:
    """The ``n_best <= beam_width <= 8`` best hypotheses of every prompt, best first, in INPUT order; ``cumulative_logprob`` (the sum of the
    tokens' log-probabilities under the unconstrained distribution) and ``score`` are always set.  A group holds ``batch_size // beam_width``
    prompts, so a step is at most ``batch_size`` rows.  The rules, with ``W = beam_width``:

    1. At step ``t`` a prompt has live beams ``b = 0..`` with fp32 scores ``s_b``; one beam with score 0 at ``t = 0`` (the prefill's logits row).
    2. Continuations: the ``W`` best triples ``(s_b + lp, b, token)`` over the live beams' allowed NON-stop tokens, by score descending, then
       beam ascending, then token ascending (``ops.topk_logprob`` with ``k = W`` per row under the allowed-minus-stops mask).
    3. Finishers: for every live beam and stop token ``s_b + (x[stop] - lse)``; none while ``t < min_new_tokens``.
    4. Continuations and finishers are merged in the same order.  Every finisher among the first ``W`` entries joins the prompt's pool: final
       score ``score / (t + 1) ** length_penalty``, ``finish_reason`` ``"stop"``, the stop token included.
    5. The ``W`` continuations become the next beams.
    6. A prompt is done when its pool holds at least ``W`` hypotheses.  After ``max_new_tokens`` the live beams join it with ``"length"`` and
       ``s / max_new_tokens ** length_penalty``.
    7. The result: the pool by final score descending (stable in the order of joining), cut to ``n_best``.

    Refused before any launch (``ValueError``): the three beam arguments outside their ranges, a penalty off its neutral value (vLLM's beam
    search ignores them, and ``ssi_topk_logprob`` knows none), and everything ``generate`` refuses.
    ``small_batch``, ``split_kv``: handed to every ``decode_step_beam`` (``generate``'s rules, on the group's ``prompts * beam_width`` rows).
    ``kv_cache_dtype``: ``generate``'s; the prompt cache and the beam cache are of the same kind.
    ``weight_dtype``, ``weight_quant``: ``generate``'s.
    ``continuous=True`` is refused (``ValueError``): the beams of a prompt share its slot, and refilling that is not built.
    ``mbr=True`` (``n_best >= 2``, else a ``ValueError`` before any launch): every prompt's ``n_best`` hypotheses come back in
    ``mbr_select``'s order instead of by score, each with its ``mbr_risk``."""
    W, length_penalty, n_best = _check_beam(beam_width, length_penalty, n_best)
    mbr = _check_mbr("beam_search", mbr, n_best, "n_best")
    if _check_continuous("beam_search", continuous, admit_min):
        raise ValueError("beam_search: continuous batching is not built for beam search (the beams of a prompt share its slot)")
    kv_dtype = check_kv_cache_dtype(kv_cache_dtype)
    weights = _weight_source(model, weight_dtype, weight_quant, small_batch)
    if _check_penalties(repetition_penalty, frequency_penalty, presence_penalty) is not None:
        raise ValueError("beam_search: repetition, frequency and presence penalties are not part of beam search")
    max_new_tokens, batch_size, min_new_tokens, V = int(max_new_tokens), int(batch_size), int(min_new_tokens), int(model.vocab_size)
    masks = _constraint_masks(V, allowed_token_ids, min_new_tokens, stop_token_ids)
    stops = allowed_mask(V, ids=[int(t) for t in stop_token_ids])
    cont = (masks[1] if masks is not None else ~stops)
    if not bool(cont.any()):
        raise ValueError("beam_search: nothing is allowed besides the stop tokens")
    if max_new_tokens < 1:
        raise ValueError(f"max_new_tokens must be >= 1 (got {max_new_tokens})")
    if batch_size < W:
        raise ValueError(f"batch_size = {batch_size} holds no prompt of beam_width = {W}")

    def open_caches(n_slots: int, longest: int):
        return (_new_cache(model, n_slots, longest, kv_dtype), _new_cache(model, n_slots * W, max_new_tokens, kv_dtype),
                _mask_words(cont).to(model.device))

    def run_group(caches, con, seqs: list[Tensor], index: list[int], stop: Tensor) -> list[list[Generation]]:
        return _beam_group(model, *caches[:2], seqs, W, max_new_tokens, stop, int(pad_id), length_penalty, n_best, caches[2], min_new_tokens,
                           small_batch, small_batch_report, split_kv, weights)

    found = _run_groups(model, prompts, batch_size // W, max_new_tokens, stop_token_ids, None, 0, open_caches, run_group)      # (its mask is cont)
    return _mbr_reorder(found, model.device) if mbr else found


def _beam_group(model, pcache, bcache, seqs: list[Tensor], W: int, max_new: int, stop: Tensor, pad_id: int, length_penalty: float, n_best: int,
                cont_words: Tensor, min_new: int, small_batch: bool = False, report: dict | None = None, split_kv: bool = False,
                weights=None) -> list[list[Generation]]:
    """One group: row ``s * W + b`` is beam ``b`` of prompt ``s``.  Everything of a step stays on the device."""
    n, dev, V, S = len(seqs), model.device, int(model.vocab_size), int(stop.numel())
    R, P, NEG = n * W, 2 * W, float("-inf")     # a pool never holds more than (W - 1) + W hypotheses; place P takes what is not stored
    i64, f32 = dict(dtype=torch.int64, device=dev), dict(dtype=torch.float32, device=dev)
    prefill_kw, step_kw = _small_batch_kw(model, R, small_batch, report, split_kv, weights)
    logits = model.prefill(pcache, seqs, **prefill_kw)
    own = torch.arange(R, dtype=torch.int32, device=dev)
    seq_of = own // W
    plen = torch.tensor([int(s.numel()) for s in seqs], dtype=torch.int32).to(dev).repeat_interleave(W)
    scores = torch.full((n, W), NEG, **f32)
    scores[:, 0] = 0.0
    hist = torch.full((R, max_new), pad_id, **i64)
    anc = torch.zeros((R, max_new), dtype=torch.int32, device=dev)
    pool_score, pool_raw = torch.full((n, P + 1), NEG, **f32), torch.zeros((n, P + 1), **f32)
    pool_len, pool_stop = torch.zeros((n, P + 1), **i64), torch.full((n, P + 1), -1, **i64)
    pool_tok = torch.full((n, P + 1, max_new), pad_id, **i64)
    count, done = torch.zeros(n, **i64), torch.zeros(n, dtype=torch.bool, device=dev)
    idx, lp, lse = torch.empty((R, W), dtype=torch.int32, device=dev), torch.empty((R, W), **f32), torch.empty(R, **f32)
    beam_of = torch.cat([torch.arange(W, **i64).repeat_interleave(W), torch.arange(W, **i64).repeat_interleave(S)]).expand(n, -1)
    is_fin = torch.cat([torch.zeros(W * W, dtype=torch.bool, device=dev), torch.ones(W * S, dtype=torch.bool, device=dev)]).expand(n, -1)
    place = torch.arange(W * W + W * S, **i64)

    def join(who: Tensor, final: Tensor, raw: Tensor, length: int, stop_tok: Tensor, beams: Tensor, last_tok: Tensor | None, at: int) -> None:
        """The entries ``who`` (bool ``[n, m]``) join their prompts' pools, in the order of their columns."""
        nonlocal count
        dest = torch.where(who, count[:, None] + who.cumsum(1) - 1, torch.full_like(beams, P))
        pool_score.scatter_(1, dest, final)
        pool_raw.scatter_(1, dest, raw)
        pool_len.scatter_(1, dest, torch.full_like(dest, length))
        pool_stop.scatter_(1, dest, stop_tok)
        toks = hist.view(n, W, max_new).gather(1, beams[:, :, None].expand(-1, -1, max_new))
        if last_tok is not None:
            toks[:, :, at] = last_tok
        pool_tok.scatter_(1, dest[:, :, None].expand(-1, -1, max_new), toks)
        count = count + who.sum(1)

    for t in range(max_new):
        rows = n if t == 0 else R                       # step 0 reads the prefill's row of every prompt: its one beam
        ops.topk_logprob(logits, V, W, idx[:rows], lp[:rows], lse[:rows], mask=cont_words)
        fin_lp = logits[:, stop].float() - lse[:rows, None]
        nb = rows // n
        c_tok, c_lp, fin_lp = idx[:rows].long().view(n, nb, W), lp[:rows].view(n, nb, W), fin_lp.view(n, nb, S)
        c_sc = torch.where(c_tok >= 0, scores[:, :, None] + c_lp, torch.full_like(scores, NEG)[:, :, None])      # ([n, 1, W] spreads over the beams)
        f_sc = scores[:, :, None] + fin_lp if t >= min_new else torch.full((n, W, S), NEG, **f32)
        sc = torch.cat([c_sc.reshape(n, W * W), f_sc.reshape(n, W * S)], dim=1)
        sc = torch.where(sc.isnan(), torch.full_like(sc, NEG), sc)
        tk = torch.cat([c_tok.expand(n, W, W).reshape(n, W * W), stop.expand(n, W, S).reshape(n, W * S)], dim=1)
        # the order of rules 2 and 4: (beam, token) ascending first, then a stable sort by score descending
        o = torch.argsort(beam_of * V + tk.clamp(min=0), dim=1, stable=True)
        sc, o2 = torch.sort(sc.gather(1, o), dim=1, descending=True, stable=True)
        o = o.gather(1, o2)
        tk, bm, fin = tk.gather(1, o), beam_of.gather(1, o), is_fin.gather(1, o)
        valid = sc > NEG
        who = fin & valid & (place < W) & ~done[:, None]
        join(who[:, :W], sc[:, :W] / float((t + 1) ** length_penalty), sc[:, :W], t + 1, tk[:, :W], bm[:, :W], tk[:, :W], t)
        is_cont = ~fin & valid
        nth = is_cont.cumsum(1) - 1
        dest = torch.where(is_cont & (nth < W), nth, torch.full_like(nth, W))
        new_sc = torch.full((n, W + 1), NEG, **f32).scatter_(1, dest, sc)[:, :W].contiguous()
        parent = torch.zeros((n, W + 1), **i64).scatter_(1, dest, bm)[:, :W].contiguous()
        new_tok = torch.zeros((n, W + 1), **i64).scatter_(1, dest, tk)[:, :W].contiguous()
        done = done | (count >= W)
        live = (new_sc > NEG) & ~done[:, None]
        scores = torch.where(live, new_sc, torch.full_like(new_sc, NEG))
        prow = (torch.arange(n, **i64)[:, None] * W + parent).view(R)
        hist = hist.index_select(0, prow)
        hist[:, t] = torch.where(live.view(R), new_tok.view(R), torch.full_like(prow, pad_id))
        if t + 1 == max_new:
            break
        if (t + 1) % READBACK_EVERY == 0 and bool(done.all()):      # the read-back
            break
        anc = anc.index_select(0, prow)
        anc[:, t] = own
        logits = model.decode_step_beam(pcache, bcache, torch.where(live, new_tok, torch.zeros_like(new_tok)).view(R),
                                        torch.where(live.view(R), seq_of, torch.full_like(seq_of, -1)), plen, anc, t, **step_kw)
    live = scores > NEG                                 # what is still alive after max_new tokens ends by length (none in a group that ended early)
    all_beams = torch.arange(W, **i64).expand(n, W)
    join(live & ~done[:, None], scores / float(max_new ** length_penalty), scores, max_new, torch.full((n, W), -1, **i64), all_beams, None, 0)
    best, order = torch.sort(pool_score[:, :P], dim=1, descending=True, stable=True)
    h_score, h_raw = best.cpu().tolist(), pool_raw[:, :P].gather(1, order).cpu().tolist()
    h_len, h_stop = pool_len[:, :P].gather(1, order).cpu().tolist(), pool_stop[:, :P].gather(1, order).cpu().tolist()
    h_tok, h_count = pool_tok[:, :P].gather(1, order[:, :, None].expand(-1, -1, max_new)).cpu(), count.cpu().tolist()
    errors = int(pcache.errors) + int(bcache.errors)
    if errors != 0:
        raise RuntimeError(f"beam_search: the K/V cache kernels refused {errors} rows (a destination, a slot or an ancestry entry outside its cache)")
    out = []
    for s in range(n):
        out.append([Generation(token_ids=h_tok[s, j, :h_len[s][j]].tolist(), finish_reason="stop" if h_stop[s][j] >= 0 else "length",
                               stop_reason=h_stop[s][j] if h_stop[s][j] >= 0 else None, cumulative_logprob=h_raw[s][j],
                               prompt_len=int(seqs[s].numel()), score=h_score[s][j]) for j in range(min(n_best, h_count[s]))])
    return out


# ---- sampling --------------------------------------------------------------------------------------------------------------------
def _check_sample(n, temperature, top_k, top_p, seed) -> tuple[int, float, int, float, int]:
    """The ranges of the sampling arguments (``ValueError``)."""
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= MAX_SAMPLES:
        raise ValueError(f"n = {n!r}: an integer from 1 to {MAX_SAMPLES}")
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not 0.0 < float(temperature) < float("inf"):
        raise ValueError(f"temperature = {temperature!r}: a finite number > 0 (greedy decoding is generate, not temperature 0)")
    if isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or not 0.0 < float(top_p) <= 1.0:
        raise ValueError(f"top_p = {top_p!r}: a number in (0, 1]")
    if isinstance(top_k, bool) or not isinstance(top_k, int):
        raise ValueError(f"top_k = {top_k!r}: an integer (<= 0: no top-k)")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed = {seed!r}: an integer in [0, 2^64)")
    return n, float(temperature), top_k, float(top_p), seed


def _check_draws(n, temperature, top_k, top_p, seed, n_prompts: int) -> tuple[int, dict]:
    """``sample``'s draw arguments, each of ``temperature``, ``top_k`` and ``top_p`` a number or a list / tuple of one per prompt, every value
    by ``_check_sample``'s rules (``ValueError``).  Returns ``n`` and the keywords of a sampling launch: a number stays the scalar it was, a
    list becomes a CPU tensor over the prompts (float64; int64 for ``top_k``, clamped as ``ops`` clamps the scalar)."""
    given = {"temperature": temperature, "top_k": top_k, "top_p": top_p}
    lists = {k: list(v) for k, v in given.items() if isinstance(v, (list, tuple))}
    for k, v in lists.items():
        if len(v) != n_prompts:
            raise ValueError(f"{k}: {len(v)} values for {n_prompts} prompts (one per prompt, or one number)")
    one = {k: (lists[k][0] if k in lists and lists[k] else (v if k not in lists else {"temperature": 1.0, "top_k": -1, "top_p": 1.0}[k]))
           for k, v in given.items()}
    n, t, k, p, seed = _check_sample(n, one["temperature"], one["top_k"], one["top_p"], seed)
    draw: dict = dict(temperature=t, top_k=k, top_p=p, seed=seed)
    for i in range(n_prompts if lists else 0):
        try:
            got = _check_sample(n, *(lists[name][i] if name in lists else draw[name] for name in ("temperature", "top_k", "top_p")), seed)
        except ValueError as e:
            raise ValueError(f"prompt {i}: {e}") from None
        for name, v in zip(("temperature", "top_k", "top_p"), got[1:4]):
            if name in lists:
                lists[name][i] = v
    for name, v in lists.items():
        draw[name] = (torch.tensor([max(-1, min(x, 2 ** 62)) for x in v], dtype=torch.int64) if name == "top_k"
                      else torch.tensor(v, dtype=torch.float64))
    return n, draw


def sample(model, prompts: Sequence[Any], *, n: int = 1, temperature: float, top_k: int = -1, top_p: float = 1.0, seed: int, max_new_tokens: int,
           stop_token_ids: Sequence[int], pad_id: int, batch_size: int = 256, allowed_token_ids: Sequence[int] | Tensor | None = None,
           min_new_tokens: int = 0, repetition_penalty: float = 1.0, frequency_penalty: float = 0.0,
           presence_penalty: float = 0.0, small_batch: bool = False, small_batch_report: dict | None = None,
             split_kv: bool = False, kv_cache_dtype: str | None = None, weight_dtype: str | None = None,
             weight_quant=None, continuous: bool = False, admit_min: int | None = None,
             continuous_report: dict | None = None, mbr: bool = False) -> list[list[Generation]]:
    """``n`` (1..8) sampled continuations of every prompt, in INPUT order and per prompt in sample order; ``cumulative_logprob`` (the tokens'
    log-probabilities under the unconstrained distribution at temperature 1, what ``ssi.score`` assigns) and ``n_kept_mean`` are always set.
    The token of a step is ``ops.decode_sample``'s with ``step`` the loop index and ``sequence = prompt index * n + sample index``: a pure function
    of ``(seed, sequence, step)`` and the row's logits, so ``batch_size``, the grouping and the order of the prompts never enter the random bits.
    ``top_k <= 0``: no top-k; ties at either threshold stay; top-p acts after top-k on the renormalised rest (vLLM's order).
    ``n = 1``: ``generate``'s stepping (``prefill``, ``decode_step``).  ``n > 1``: a group holds ``batch_size // n`` prompts; the prompt is prefilled
    once, its logits row repeated ``n`` times at step 0, and the samples run as rows of ``decode_step_beam`` with the identity ancestry.  The
    self-check per live row: the token is >= 0, allowed, and drawn from a set of at least one column (``RuntimeError``).
    ``repetition_penalty``, ``frequency_penalty``, ``presence_penalty``: with any of them off its neutral value the step's token is
    ``ops.decode_sample_pen``'s, drawn on the penalised row (penalties before temperature, top-k and top-p); the ``n`` samples of a prompt share
    one line of the group's prompt table.  The log-probabilities stay those of the raw row.
    Refused before any launch (``ValueError``): ``n`` outside 1..8, ``temperature`` not finite or <= 0 (greedy decoding is ``generate``), ``top_p``
    outside (0, 1], a non-integer ``top_k``, a negative ``seed``, and everything ``generate`` refuses.
    ``small_batch``, ``split_kv``: handed to every decode step (``generate``'s rules, on the group's ``prompts * n`` rows).
    ``kv_cache_dtype``: ``generate``'s; with ``n > 1`` the prompt cache and the samples' cache are of the same kind.
    ``weight_dtype``, ``weight_quant``: ``generate``'s.
    ``temperature``, ``top_k`` and ``top_p`` may each be a list or tuple with one value per prompt (every value by the rules above; another
    length is a ``ValueError``): the step's token then comes from ``ops.decode_sample_rows`` / ``ops.decode_sample_pen_rows``, whose row ``r`` has
    the bits of the scalar entry launched with the row's own values.  With scalars the static path launches what it always launched.
    ``continuous``, ``admit_min``, ``continuous_report``: ``generate``'s, for ``n == 1`` (``n > 1`` with ``continuous=True`` is a ``ValueError``:
    the samples of a prompt share its slot); the pool's steps go through the ``_rows`` entries with ``step`` = the row's own token count, so a
    sample stays the pure function of ``(seed, sequence, step)`` and the row that it is in a static group.
    ``mbr=True`` (``n >= 2``, else a ``ValueError`` before any launch): the same ``n`` samples of every prompt, in ``mbr_select``'s order
    instead of sample order, each with its ``mbr_risk``."""
    n, draw = _check_draws(n, temperature, top_k, top_p, seed, len(prompts))
    mbr = _check_mbr("sample", mbr, n, "n")
    kv_dtype = check_kv_cache_dtype(kv_cache_dtype)
    weights = _weight_source(model, weight_dtype, weight_quant, small_batch)
    pen = _check_penalties(repetition_penalty, frequency_penalty, presence_penalty)
    max_new_tokens, batch_size, min_new_tokens, V = int(max_new_tokens), int(batch_size), int(min_new_tokens), int(model.vocab_size)
    masks = _constraint_masks(V, allowed_token_ids, min_new_tokens, stop_token_ids)
    if max_new_tokens < 1:
        raise ValueError(f"max_new_tokens must be >= 1 (got {max_new_tokens})")
    if batch_size < n:
        raise ValueError(f"batch_size = {batch_size} holds no prompt of n = {n}")
    if len(prompts) * n > 2 ** 32:
        raise ValueError(f"{len(prompts)} prompts x {n} samples do not fit the 32-bit sequence number")
    refused = "sample: the K/V cache kernels refused {} rows (a destination, a slot or an ancestry entry outside its cache)"
    if _check_continuous("sample", continuous, admit_min):
        if n != 1:
            raise ValueError(f"sample: continuous batching is built for n = 1 (got n = {n}: the samples of a prompt share its slot)")
        found = _run_pool(model, prompts, batch_size, max_new_tokens, stop_token_ids, masks, min_new_tokens, kv_dtype, admit_min,
                          lambda seqs, pool, con: _Sample(model, seqs, [], 1, draw, con, pen, pool=pool), refused, int(pad_id), small_batch,
                          small_batch_report, split_kv, weights, continuous_report)
        return [[g] for g in found]

    def open_caches(n_slots: int, longest: int):
        if n == 1:
            return (_new_cache(model, n_slots, longest + max_new_tokens, kv_dtype),)
        return _new_cache(model, n_slots, longest, kv_dtype), _new_cache(model, n_slots * n, max_new_tokens, kv_dtype)

    def run_group(caches, con, seqs: list[Tensor], index: list[int], stop: Tensor) -> list[list[Generation]]:
        if n == 1:          # no prompt to share: every row on its own slot, as ``generate``
            started = _own_slots(model, caches, seqs, max_new_tokens, small_batch, small_batch_report, split_kv, weights)
        else:
            started = _shared_prompt(model, caches, seqs, n, max_new_tokens, small_batch, small_batch_report, split_kv, weights)
        choose = _Sample(model, seqs, index, n, draw, con, pen)
        found = _token_loop(choose, started, caches, refused, [int(s.numel()) for s in seqs for _ in range(n)], max_new_tokens, stop, int(pad_id))
        return [found[s * n:s * n + n] for s in range(len(seqs))]

    found = _run_groups(model, prompts, batch_size // n, max_new_tokens, stop_token_ids, masks, min_new_tokens, open_caches, run_group)
    return _mbr_reorder(found, model.device) if mbr else found


# ---- JSONL in, JSONL out ---------------------------------------------------------------------------------------------------------
def output_record(item_id: Any, prompt_ids: Sequence[int], gen: "Generation | Sequence[Generation]", tokenizer, decoding: dict | None = None) -> dict[str, Any]:
    """One output line in the shape of the reference's generations file: ``outputs`` is a list with ONE entry (greedy, ``n = 1``) whose
    ``text`` is what the reference's ``extract_texts_from_generations_jsonl`` reads — or, for a list of hypotheses (beam search with
    ``n_best``), one entry each, ``index`` 0.. in the list's order (best first)."""
    decoding = dict(decoding or {})
    special = {v: k for k, v in getattr(tokenizer, "special_tokens", {}).items()}
    gens = [gen] if isinstance(gen, Generation) else list(gen)
    mbr = [{} if g.mbr_risk is None else {"index": g.mbr_index, "mbr_risk": g.mbr_risk} for g in gens]   # risk order: ``index`` is the original one
    return {"id": item_id, "prompt_token_ids": [int(t) for t in prompt_ids], "prompt": tokenizer.decode(list(prompt_ids), **decoding),
            "outputs": [dict({"index": j, "text": tokenizer.decode(g.token_ids, **decoding), "token_ids": g.token_ids,
                              "cumulative_logprob": g.cumulative_logprob, "finish_reason": g.finish_reason, "stop_reason": g.stop_reason,
                              "stop_reason_text": special.get(g.stop_reason) if g.stop_reason is not None else None}, **m)
                        for j, (g, m) in enumerate(zip(gens, mbr))]}


def _read_prompts(tokenizer, in_path: str) -> tuple[list[Any], list[list[int]]]:
    ids, prompts = [], []
    with open(in_path, encoding="utf-8") as f:
        for ln, line in enumerate(f, 1):
            if not line.strip():
                continue
            item = json.loads(line)
            if ("prompt_tokens" in item) == ("prompt" in item):
                raise ValueError(f"{in_path}:{ln}: an item needs exactly one of 'prompt_tokens' and 'prompt'")
            if "prompt_tokens" in item:
                toks = [int(t) for t in item["prompt_tokens"]]
            else:
                toks = list(tokenizer.encode(item["prompt"], add_bos=True, add_eos=False))
            ids.append(item.get("id", len(ids)))
            prompts.append(toks)
    return ids, prompts


def default_stop_token_ids(tokenizer) -> list[int]:
    """``[eom_id, eot_id, eos_id]``, as the reference sets them when the configuration names none."""
    return [int(tokenizer.eom_id), int(tokenizer.eot_id), int(tokenizer.eos_id)]


def generate_file(model, tokenizer, in_path: str | None, out_path: str, *, max_new_tokens: int, stop_token_ids: Sequence[int] | None = None,
                  tokenizer_decoding: dict | None = None, prompts: Sequence[Sequence[int]] | None = None, ids: Sequence[Any] | None = None,
                  **kw) -> dict[str, Any]:
    """JSONL in, JSONL out, in the style of ``score_file``.  Every input line: ``id`` and exactly one of ``prompt_tokens`` (ids, taken as they
    are) and ``prompt`` (the tokenizer's ``encode`` with BOS and without EOS).  ``in_path=None``: the prompts (and ids) come as arguments —
    how ``scripts/generate.py`` hands over a data split.  Every output line: ``id``, ``prompt_token_ids``, ``prompt`` and ``outputs``, a list
    with one entry holding ``index, text, token_ids, cumulative_logprob, finish_reason, stop_reason, stop_reason_text``, in INPUT order.
    ``stop_token_ids`` default to the tokenizer's ``[eom_id, eot_id, eos_id]``; ``pad_id`` to the tokenizer's; ``kw`` goes to ``generate``.
    Returns ``{"items", "generated_tokens", "stopped"}``, and under a constraint (``allowed_token_ids`` / ``min_new_tokens`` in ``kw``) also
    ``"constrained_tokens"``: the tokens the constraint changed, over all items.
    ``beam_width > 1`` in ``kw`` (with ``length_penalty``, ``n_best``): ``beam_search`` instead of ``generate``; ``outputs`` then holds ``n_best``
    entries, ``index`` 0.., best first, the summary counts every written hypothesis and gains ``"beam_width"``.  ``beam_width = 1`` (the default)
    is the greedy path: nothing of beam search runs.
    ``sample=True`` in ``kw`` (with ``temperature``, ``seed`` and optionally ``n``, ``top_k``, ``top_p``): ``sample`` instead; ``outputs`` holds ``n``
    entries, ``index`` 0.. in sample order, and the summary gains ``"sampled": True``, ``"n"`` and ``"kept_tokens_mean"`` (the mean over all generated
    tokens of the size of the set each was drawn from).  Not together with ``beam_width > 1``.
    ``repetition_penalty``, ``frequency_penalty``, ``presence_penalty`` in ``kw`` go to ``generate`` / ``sample`` (``beam_search`` refuses them off
    their neutral values); when any is set the summary gains the three values, and on the greedy path ``"constrained_tokens"``.
    ``small_batch=True`` in ``kw`` goes to whichever loop runs, and the summary gains ``"small_batch_groups"``: the number of groups that decoded on
    the skinny path.  ``split_kv=True`` likewise, with ``"split_kv_groups"``: the groups that ran the split-KV decode attention.  ``False`` (the
    default of both) is not passed on and adds no key.
    ``kv_cache_dtype`` in ``kw`` goes to whichever loop runs (``check_kv_cache_dtype``, refused here before a prompt is read); the summary gains
    ``"kv_cache_dtype": "fp8"`` under fp8 alone — None and "auto" are not passed on and add no key.
    ``weight_dtype`` (and ``weight_quant``) in ``kw`` likewise (``check_weight_dtype``: "fp8" needs ``small_batch=True``); under fp8 alone the summary
    gains ``"fp8_weight_groups"``: the groups whose steps read FP8 weights.
    ``continuous=True`` (and ``admit_min``) in ``kw`` go to ``generate`` / ``sample`` (``n > 1`` and ``beam_width > 1`` refuse it), and the summary
    gains ``"continuous": True``, ``"decode_steps"``, ``"row_steps_live"``, ``"row_steps_total"`` and ``"admissions"``; ``False`` (the default) and
    a null ``admit_min`` are not passed on and add no key.
    ``mbr=True`` in ``kw`` goes to ``sample`` / ``beam_search`` (greedy decoding has one candidate and refuses it): ``outputs`` are then in risk
    order — ``outputs[0]`` is the MBR choice, what ``scripts/wer.py`` scores — each with ``mbr_risk`` and its original ``index``, and the summary
    gains ``"mbr_changed"``: the prompts whose first output is not candidate 0.  ``False`` (the default) is not passed on and adds no key."""
    if not kw.get("mbr", False):
        kw.pop("mbr", None)
    kv_dtype = check_kv_cache_dtype(kw.pop("kv_cache_dtype", None))
    fp8 = {} if kv_dtype is None else {"kv_cache_dtype": kv_dtype}
    w8 = {} if check_weight_dtype(kw.pop("weight_dtype", None), bool(kw.get("small_batch", False))) is None else {"weight_dtype": "fp8"}
    if not w8 and kw.get("weight_quant") is not None:
        raise ValueError("weight_quant without weight_dtype='fp8'")
    if not w8:
        kw.pop("weight_quant", None)
    if in_path is not None:
        ids, prompts = _read_prompts(tokenizer, in_path)
    elif prompts is None:
        raise ValueError("generate_file: an input file or prompts")
    else:
        prompts = [[int(t) for t in p] for p in prompts]
        ids = list(ids) if ids is not None else list(range(len(prompts)))
    if stop_token_ids is None:
        stop_token_ids = default_stop_token_ids(tokenizer)
    kw.setdefault("pad_id", int(getattr(tokenizer, "pad_id", 0) or 0))
    flags = {flag: True for flag in ("small_batch", "split_kv") if kw.pop(flag, False)}
    if not flags:
        return dict(_run_file(model, tokenizer, ids, prompts, out_path, max_new_tokens, stop_token_ids, tokenizer_decoding, dict(kw, **fp8)), **fp8)
    report = {flag + "_groups": 0 for flag in flags}          # counted by the loop, group by group, where the path is taken
    if w8:
        report["fp8_weight_groups"] = 0
    summary = _run_file(model, tokenizer, ids, prompts, out_path, max_new_tokens, stop_token_ids, tokenizer_decoding,
                        dict(kw, small_batch_report=report, **flags, **fp8, **w8))
    return dict(summary, **report, **fp8)


def _run_file(model, tokenizer, ids, prompts, out_path, max_new_tokens, stop_token_ids, tokenizer_decoding, kw: dict) -> dict[str, Any]:
    """``generate_file`` behind its input handling: picks the loop (greedy, beam search, sampling), writes the lines, returns the summary.
    Under beam search and sampling ``logprobs`` is not an option (every hypothesis and sample carries its log-probability), and ``device`` must
    be the model's, as ``generate`` asks."""
    kw = dict(kw)
    beam = {k: kw.pop(k) for k in ("beam_width", "length_penalty", "n_best") if k in kw}
    pen = _check_penalties(kw.get("repetition_penalty", 1.0), kw.get("frequency_penalty", 0.0), kw.get("presence_penalty", 0.0))
    pen_summary = {} if pen is None else {"repetition_penalty": pen.r, "frequency_penalty": pen.f, "presence_penalty": pen.p}
    draw = {k: kw.pop(k) for k in ("sample", "n", "temperature", "top_k", "top_p", "seed") if k in kw}
    sampled = bool(draw.pop("sample", False))
    if draw and not sampled:
        raise ValueError(f"generate_file: {sorted(draw)} without sample=True")
    beams = int(beam.get("beam_width", 1)) != 1
    if sampled and beams:
        raise ValueError("generate_file: sample together with beam_width > 1 (sampling inside beam search is not built)")
    if not (sampled or beams):
        _check_beam(1, beam.get("length_penalty", 1.0), beam.get("n_best", 1))      # (n_best > 1 needs a beam)
        if "mbr" in kw:
            raise ValueError("generate_file: mbr=True needs candidates to choose among: sample=True with n >= 2, or beam_width > 1 with n_best >= 2")
    run, mode = (sample, draw) if sampled else (beam_search, beam) if beams else (generate, {})
    if sampled or beams:
        kw.pop("logprobs", None)
        device = kw.pop("device", None)
        if device is not None and torch.device(device) != model.device:
            raise ValueError(f"generate: device {device} is not the model's ({model.device})")
    pool = {k: v for k, v in (("continuous", kw.pop("continuous", False)), ("admit_min", kw.pop("admit_min", None))) if v not in (False, None)}
    stats: dict = {}
    if pool.get("continuous") is True and not beams:      # (beam search refuses the flag itself)
        pool["continuous_report"] = stats
    found = run(model, prompts, max_new_tokens=max_new_tokens, stop_token_ids=stop_token_ids, **mode, **kw, **pool)
    with open(out_path, "w", encoding="utf-8") as f:
        for item_id, p, g in zip(ids, prompts, found):
            f.write(json.dumps(output_record(item_id, p, g, tokenizer, tokenizer_decoding), ensure_ascii=False) + "\n")
    gens = [g for gs in found for g in gs] if sampled or beams else found       # every written hypothesis or sample counts
    tokens = sum(len(g.token_ids) for g in gens)
    summary = {"items": len(found), "generated_tokens": tokens, "stopped": sum(g.finish_reason == "stop" for g in gens)}
    if sampled:
        kept = sum((g.n_kept_mean or 0.0) * len(g.token_ids) for g in gens)
        summary.update(sampled=True, n=int(draw.get("n", 1)), kept_tokens_mean=kept / max(tokens, 1))
    elif beams:
        summary["beam_width"] = int(beam["beam_width"])
    elif kw.get("allowed_token_ids") is not None or int(kw.get("min_new_tokens", 0)) != 0 or pen is not None:
        summary["constrained_tokens"] = sum(g.n_constrained or 0 for g in gens)
    if kw.get("mbr"):
        summary["mbr_changed"] = sum(gs[0].mbr_index != 0 for gs in found)
    return dict(summary, **pen_summary, **stats)       # (pen_summary: empty under beam search, which refuses a set penalty)


# ---- what the script accepts of the reference's sampling_params ------------------------------------------------------------------
GREEDY = {"n": 1, "temperature": 0.0, "top_p": 1.0, "top_k": -1, "presence_penalty": 0.0, "frequency_penalty": 0.0, "repetition_penalty": 1.0}


def check_greedy(sampling_params) -> None:
    """``NotImplementedError`` for anything but greedy decoding of one sequence: ``temperature != 0``, ``top_p != 1``, ``top_k != -1``, a
    penalty off its default, ``n != 1`` (the reference pins its WER to greedy, too).  ``max_tokens`` and ``stop_token_ids`` are free;
    ``min_tokens`` (an integer >= 0) and ``allowed_token_ids`` (null or a list of integers) keep decoding greedy and pass (``ValueError`` for
    another value); a key this module does not know is refused as well."""
    for key in sampling_params:
        if key in ("max_tokens", "stop_token_ids"):
            continue
        if key == "min_tokens":
            value = sampling_params[key]
            if isinstance(value, bool) or not isinstance(value, int) or value < 0:
                raise ValueError(f"sampling_params.min_tokens = {value!r}: an integer >= 0")
            continue
        if key == "allowed_token_ids":
            value = sampling_params[key]
            if value is not None and (isinstance(value, (str, bytes)) or not hasattr(value, "__iter__")
                                      or any(isinstance(t, bool) or not isinstance(t, int) for t in value)):
                raise ValueError(f"sampling_params.allowed_token_ids = {value!r}: null or a list of integers")
            continue
        if key not in GREEDY:
            raise NotImplementedError(f"sampling_params.{key} is not supported: generation is greedy")
        value = sampling_params[key]
        if value is None or float(value) != float(GREEDY[key]):
            raise NotImplementedError(f"sampling_params.{key} = {value!r}: only greedy decoding is built ({key} = {GREEDY[key]!r})")


SAMPLING_KEYS = ("n", "temperature", "top_k", "top_p")
PENALTY_KEYS = {"repetition_penalty": 1.0, "frequency_penalty": 0.0, "presence_penalty": 0.0}


def check_penalties(sampling_params) -> dict[str, float]:
    """What ``gen.penalties: true`` accepts of ``sampling_params``: ``repetition_penalty`` finite and > 0, ``frequency_penalty`` and
    ``presence_penalty`` in [-2, 2] (``ValueError`` otherwise; an absent key or null is the neutral value).  Returns the three as the keyword
    arguments of ``generate`` / ``sample``; the caller hands the rest of ``sampling_params``, without these keys, to ``check_greedy`` or
    ``check_sampling`` unchanged."""
    got = {k: (sampling_params[k] if k in sampling_params and sampling_params[k] is not None else v) for k, v in PENALTY_KEYS.items()}
    try:
        _check_penalties(got["repetition_penalty"], got["frequency_penalty"], got["presence_penalty"])
    except ValueError as e:
        raise ValueError(f"sampling_params.{e}") from None
    return {k: float(v) for k, v in got.items()}


def check_continuous(continuous, admit_min, beam_width: int = 1, n: int = 1) -> dict[str, Any]:
    """What ``gen.continuous`` and ``gen.admit_min`` accept, before anything is loaded: ``continuous`` null or a bool, ``admit_min`` null or an
    integer >= 1 and only with ``continuous: true``; ``continuous: true`` not with ``gen.beam_width > 1`` or ``sampling_params.n > 1``
    (``ValueError``).  Returns the keyword arguments of ``generate_file``: none at all without the flag."""
    if continuous is not None and not isinstance(continuous, bool):
        raise ValueError(f"gen.continuous = {continuous!r}: true or false")
    if admit_min is not None and (isinstance(admit_min, bool) or not isinstance(admit_min, int) or admit_min < 1):
        raise ValueError(f"gen.admit_min = {admit_min!r}: null or an integer >= 1")
    if not continuous:
        if admit_min is not None:
            raise ValueError("gen.admit_min without gen.continuous=true")
        return {}
    if int(beam_width) != 1:
        raise ValueError("gen.continuous=true together with gen.beam_width > 1: continuous batching is not built for beam search")
    if int(n) != 1:
        raise ValueError("gen.continuous=true together with sampling_params.n > 1: continuous batching is not built for several samples of a prompt")
    return {"continuous": True} if admit_min is None else {"continuous": True, "admit_min": int(admit_min)}


def check_sampling(sampling_params) -> dict[str, Any]:
    """What ``gen.sample: true`` accepts of ``sampling_params``: ``temperature > 0``, an integer ``top_k``, ``top_p`` in (0, 1] and ``n`` in
    1..8, besides what ``check_greedy`` lets through.  Still ``NotImplementedError``: a penalty off its default, ``best_of``, an unknown key.
    ``ValueError``: ``temperature = 0`` (that is greedy decoding: ``gen.sample: false``) and every value outside its range.  Returns the four
    sampling arguments of ``sample`` (``n`` 1, ``top_k`` -1 and ``top_p`` 1 where the key is absent; ``temperature`` must be there)."""
    check_greedy({k: sampling_params[k] for k in sampling_params if k not in SAMPLING_KEYS})
    got = {k: sampling_params[k] for k in SAMPLING_KEYS if k in sampling_params}
    if got.get("temperature") is None:
        raise ValueError("sampling_params.temperature: gen.sample needs a temperature > 0")
    if not isinstance(got["temperature"], bool) and isinstance(got["temperature"], (int, float)) and float(got["temperature"]) == 0.0:
        raise ValueError("sampling_params.temperature = 0 is greedy decoding: gen.sample=false")
    top_p = got.get("top_p", 1.0)
    if isinstance(top_p, int) and not isinstance(top_p, bool):
        top_p = float(top_p)
    n, temperature, top_k, top_p, _ = _check_sample(got.get("n", 1), got["temperature"], got.get("top_k", -1), top_p, 0)
    return {"n": n, "temperature": temperature, "top_k": top_k, "top_p": top_p}
