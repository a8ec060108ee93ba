"""Generation from an arbitrary prompt: what the reference plans as "standalone sample-wise generation" — a Python function and a light command
line (``scripts/prompt.py``) that take a raw string, raw token ids or a Jinja2 template with the speech and modality variables, decode greedily
with one sample by default, and give the text back.

``render_prompt`` turns exactly one of the three inputs into token ids on the host.  ``probe`` runs the prompts through ``ssi.generate`` with
``small_batch=True`` — one prompt, or a handful with a few samples each, is a decode step of 1 to 64 rows, which the skinny GEMMs run unpadded —
and returns the ``Generation``s with their decoded text."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, Mapping, Sequence

from .generate import Generation, check_kv_cache_dtype, check_weight_dtype, default_stop_token_ids, generate, output_record, sample
from .tokenizer import MODALITY_TOKEN_SPEECH, MODALITY_TOKEN_TEXT, deduplicate_units, units_to_text

__all__ = ["render_prompt", "render_template", "probe", "Probe", "prompt_records"]


def _jinja2():
    try:
        import jinja2
    except ImportError as e:
        raise RuntimeError("a prompt template needs the jinja2 package, which is not installed; pass the prompt as text or as token ids instead") from e
    return jinja2


def render_template(template: str, variables: Mapping[str, Any] | None = None, *, deduplicate: bool = False, unit_bpe: Any = None) -> str:
    """The text of a Jinja2 ``template`` (a path to a file, or the template itself).  ``MODALITY_TOKEN_SPEECH`` and ``MODALITY_TOKEN_TEXT`` are
    supplied (a caller's value of the same name wins); ``speech_units``, a list of ints, is rendered as the units' private-use characters
    (``units_to_text``), after ``deduplicate_units`` when ``deduplicate`` and after ``unit_bpe`` (a merges file or a ``UnitBPE``; None: nothing is
    imported) has encoded them.  An undefined variable is an error, not an empty string."""
    jinja2 = _jinja2()
    source = template
    if os.path.isfile(template):
        with open(template, encoding="utf-8") as f:
            source = f.read()
    values: dict[str, Any] = {"MODALITY_TOKEN_SPEECH": MODALITY_TOKEN_SPEECH, "MODALITY_TOKEN_TEXT": MODALITY_TOKEN_TEXT}
    values.update(variables or {})
    units = values.get("speech_units")
    if units is not None and not isinstance(units, str):
        units = [int(u) for u in units]
        units = deduplicate_units(units) if deduplicate else units
        if unit_bpe is not None:
            from .tokenizer.unit_bpe import load_unit_bpe
            units = load_unit_bpe(unit_bpe).encode(units)
        values["speech_units"] = units_to_text(units)
    env = jinja2.Environment(undefined=jinja2.StrictUndefined, keep_trailing_newline=False, autoescape=False)
    return env.from_string(source).render(**values)


def render_prompt(tokenizer, *, text: str | None = None, token_ids: Sequence[int] | None = None, template: str | None = None,
                  variables: Mapping[str, Any] | None = None, deduplicate: bool = False, unit_bpe: Any = None) -> list[int]:
    """Token ids of a prompt given as exactly one of ``text`` (the tokenizer's ``encode`` with BOS, without EOS), ``token_ids`` (taken as they
    are; each must lie in ``[0, tokenizer.vocab_size)``) and ``template`` (``render_template`` with ``variables``, then as ``text``).
    ``ValueError``: none or several of the three, ``variables`` without a template, an empty prompt, an id outside the vocabulary."""
    given = [k for k, v in (("text", text), ("token_ids", token_ids), ("template", template)) if v is not None]
    if len(given) != 1:
        raise ValueError(f"render_prompt: exactly one of text, token_ids and template (got {given or 'none'})")
    if (variables or deduplicate or unit_bpe is not None) and template is None:
        raise ValueError("render_prompt: variables, deduplicate and unit_bpe belong to a template")
    if token_ids is not None:
        ids = [int(t) for t in token_ids]
        vocab = getattr(tokenizer, "vocab_size", None)
        bad = [t for t in ids if t < 0 or (vocab is not None and t >= int(vocab))]
        if bad:
            raise ValueError(f"render_prompt: token ids {bad[:8]} lie outside the vocabulary [0, {vocab})")
    else:
        ids = [int(t) for t in tokenizer.encode(text if text is not None else render_template(template, variables, deduplicate=deduplicate,
                                                                                                  **({} if unit_bpe is None else {"unit_bpe": unit_bpe})),
                                                add_bos=True, add_eos=False)]
    if not ids:
        raise ValueError("render_prompt: the prompt is empty")
    return ids


@dataclass
class Probe:
    """One prompt's result: its ids, and one ``Generation`` per sample with the decoded ``texts`` beside it."""
    prompt_ids: list[int]
    generations: list[Generation]
    texts: list[str]


def probe(model, tokenizer, prompts: Sequence[Sequence[int]], *, max_new_tokens: int = 128, n: int = 1, temperature: float = 0.0, top_k: int = -1,
          top_p: float = 1.0, seed: int = 0, repetition_penalty: float = 1.0, frequency_penalty: float = 0.0, presence_penalty: float = 0.0,
          stop_token_ids: Sequence[int] | None = None, tokenizer_decoding: Mapping[str, Any] | None = None, batch_size: int = 64,
          split_kv: bool = False, kv_cache_dtype: str | None = None, weight_dtype: str | None = None, weight_quant=None, mbr: bool = False) -> list[Probe]:
    """Continue every prompt (token ids, as ``render_prompt`` gives them): greedily (``generate``, with log-probabilities) at ``temperature``
    0, where ``n`` must be 1, else ``n`` samples (``sample``) — both with ``small_batch=True`` and groups of at most ``batch_size`` rows, so a few
    prompts never pay a 256-row step.  ``split_kv``: handed on to the loop (the split-KV decode attention).  ``kv_cache_dtype``: None, "auto" or
    "fp8", handed on to the loop when it is "fp8" (``ssi.generate.check_kv_cache_dtype``).  ``weight_dtype``: None, "auto" or "fp8"
    (``ssi.generate.check_weight_dtype``); under "fp8" the model's weights are quantised ONCE for the whole call (``model.quantize_weights()``, or the
    ``weight_quant`` built before and handed in to reuse it across calls) and every group reads the same object.  ``stop_token_ids`` default to the tokenizer's ``[eom_id, eot_id, eos_id]``.
    ``mbr=True`` (``n >= 2`` samples, else a ``ValueError``): every prompt's samples in minimum-Bayes-risk order (``sample(mbr=True)``)."""
    prompts = [[int(t) for t in p] for p in prompts]
    if mbr and (float(temperature) == 0.0 or int(n) < 2):
        raise ValueError("probe: mbr=True chooses among samples: a temperature > 0 and n >= 2")
    stop = default_stop_token_ids(tokenizer) if stop_token_ids is None else [int(t) for t in stop_token_ids]
    kw = dict(max_new_tokens=int(max_new_tokens), stop_token_ids=stop, pad_id=int(getattr(tokenizer, "pad_id", 0) or 0), batch_size=int(batch_size),
              repetition_penalty=repetition_penalty, frequency_penalty=frequency_penalty, presence_penalty=presence_penalty, small_batch=True,
              **({"split_kv": True} if split_kv else {}), **({"kv_cache_dtype": "fp8"} if check_kv_cache_dtype(kv_cache_dtype) else {}))
    if check_weight_dtype(weight_dtype) is not None:
        kw.update(weight_dtype="fp8", weight_quant=weight_quant if weight_quant is not None else model.quantize_weights())
    if float(temperature) == 0.0:
        if int(n) != 1 or int(top_k) > 0 or float(top_p) != 1.0:
            raise ValueError("probe: temperature 0 is greedy decoding: one sample, no top-k, no top-p (set a temperature to draw)")
        found = [[g] for g in generate(model, prompts, logprobs=True, **kw)]
    else:
        found = sample(model, prompts, n=int(n), temperature=float(temperature), top_k=int(top_k), top_p=float(top_p), seed=int(seed), **kw,
                       **({"mbr": True} if mbr else {}))
    decoding = dict(tokenizer_decoding or {})
    return [Probe(p, list(gs), [tokenizer.decode(g.token_ids, **decoding) for g in gs]) for p, gs in zip(prompts, found)]


def prompt_records(probes: Sequence[Probe], tokenizer, tokenizer_decoding: Mapping[str, Any] | None = None) -> list[dict[str, Any]]:
    """One ``output_record`` per prompt (the generations file's line: ``id``, ``prompt_token_ids``, ``prompt``, ``outputs``), ``id`` 0.. ."""
    return [output_record(i, p.prompt_ids, p.generations if len(p.generations) > 1 else p.generations[0], tokenizer, dict(tokenizer_decoding or {}))
            for i, p in enumerate(probes)]
