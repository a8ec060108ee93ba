#!/usr/bin/env python
"""Generation entry point, greedy, (gen.beam_width > 1) beam search or (gen.sample=true) sampling, either of the outer two under (gen.penalties=true) repetition, frequency and presence penalties (the reference's scripts/generate.py runs vLLM): a generations JSONL the reference's scripts/wer.py reads.
    python scripts/generate.py speech.n_dsus=5000 gen.input=prompts.jsonl gen.output_dir=out [key=value ...]
    python scripts/generate.py speech.n_dsus=5000 data=sft/<dataset> gen.split=dev gen.output_dir=out
"""
import logging
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

try:  # real Hydra if the environment has it, else the built-in composer with the same decorator shape
    import hydra
    main_decorator = hydra.main
except ImportError:
    from ssi.config import main as main_decorator

from ssi.generate import check_continuous, check_greedy, check_kv_cache_dtype, check_penalties, check_weight_dtype, check_sampling, generate_file

LOGGER = logging.getLogger(__name__)


def split_prompts(cfg, tokenizer) -> tuple[list, list]:
    """The prompts of ``cfg.data[cfg.gen.split]`` through ``SFTDataset(inference=True)``: an empty assistant message to be continued."""
    from ssi.data.sft import SFTDataset
    if cfg.get("data") is None:
        raise ValueError("generate: gen.input or a data config (data=sft/...)")
    node = cfg.data[cfg.gen.split].dataset
    kw = {k: node[k] for k in node if k not in ("inference", "fixed_len")}
    data = SFTDataset(model_tokenizer=tokenizer, inference=True, **kw)
    prompts = [list(data[i]["tokens"]) for i in range(len(data))]
    return list(range(len(prompts))), prompts


def allowed_tokens(cfg, token_type_ranges: dict, vocab_size: int):
    """The union of ``gen.allowed_token_types`` (kinds of ``get_token_type_ranges``) and ``sampling_params.allowed_token_ids`` as a bool mask
    over the vocabulary; None when neither is set."""
    from ssi.generate import allowed_mask
    kinds, ids = cfg.gen.get("allowed_token_types"), cfg.sampling_params.get("allowed_token_ids")
    if kinds is None and ids is None:
        return None
    unknown = [k for k in kinds or [] if k not in token_type_ranges]
    if unknown:
        raise ValueError(f"gen.allowed_token_types names {unknown}: the token types of this vocabulary are {list(token_type_ranges)}")
    return allowed_mask(vocab_size, ids=[int(t) for t in ids or []], ranges=[tuple(token_type_ranges[k]) for k in kinds or []])


@main_decorator(config_path="../conf", config_name="generate", version_base=None)
def main(cfg):
    sampled = bool(cfg.gen.get("sample") or False)          # everything below: before anything is loaded
    if sampled and int(cfg.gen.get("beam_width") or 1) != 1:
        raise ValueError("gen.sample=true together with gen.beam_width > 1: sampling inside beam search is not built")
    penalties, params = {}, cfg.sampling_params
    if bool(cfg.gen.get("penalties") or False):              # without it every refusal of a penalty below is what it was
        if int(cfg.gen.get("beam_width") or 1) != 1:
            raise ValueError("gen.penalties=true together with gen.beam_width > 1: beam search takes no penalties")
        penalties = check_penalties(params)
        params = {k: params[k] for k in params if k not in penalties}
    draw = dict(check_sampling(params), sample=True, seed=int(cfg.gen.get("seed") or 0)) if sampled else {}
    if not sampled:
        check_greedy(params)
    if bool(cfg.gen.get("mbr") or False) and int(draw.get("n", 1)) < 2 and min(int(cfg.gen.get("beam_width") or 1), int(cfg.gen.get("n_best") or 1)) < 2:
        raise ValueError("gen.mbr=true needs candidates to choose among: gen.sample=true with sampling_params.n >= 2, or gen.beam_width > 1 with gen.n_best >= 2")
    pool = check_continuous(cfg.gen.get("continuous"), cfg.gen.get("admit_min"), int(cfg.gen.get("beam_width") or 1), int(draw.get("n", 1)))
    from ssi.model import get_device, get_dtype
    from ssi.train_utils import resolve_n_dsus
    from ssi.trainer import Trainer
    resolve_n_dsus(cfg)
    t = Trainer(cfg)  # model, tokenizer and checkpointer as a training run sets them up; no optimizer, no data loaders
    t.device, t.dtype = get_device(cfg.device), get_dtype(cfg.dtype)
    t._setup_model()
    t._setup_tokenizer()
    os.makedirs(str(cfg.gen.output_dir), exist_ok=True)
    out_path = os.path.join(str(cfg.gen.output_dir), str(cfg.gen.output_filename))
    ids = prompts = None
    if cfg.gen.get("input") is None:
        ids, prompts = split_prompts(cfg, t.tokenizer)
    stop = cfg.sampling_params.get("stop_token_ids")
    constraints = {}          # with the defaults the call below is the unconstrained one
    allowed = allowed_tokens(cfg, t.token_type_ranges, int(t.model.vocab_size))
    if allowed is not None:
        constraints["allowed_token_ids"] = allowed
    if int(cfg.sampling_params.get("min_tokens") or 0) > 0:
        constraints["min_new_tokens"] = int(cfg.sampling_params.min_tokens)
    if int(cfg.gen.get("beam_width") or 1) != 1:          # beam search: gen.* keys, not sampling_params (which stay greedy, n = 1)
        constraints.update(beam_width=int(cfg.gen.beam_width), length_penalty=float(cfg.gen.get("length_penalty", 1.0)),
                           n_best=int(cfg.gen.get("n_best", 1)))
    constraints.update(draw)          # gen.sample: the sampling_params that check_sampling let through, and gen.seed
    constraints.update(penalties)     # gen.penalties: the three values check_penalties let through
    if bool(cfg.gen.get("small_batch") or False):          # gen.small_batch: groups of at most 64 rows on the skinny GEMMs; absent from the call otherwise
        constraints["small_batch"] = True
    if bool(cfg.gen.get("split_kv") or False):             # gen.split_kv: the split-KV decode attention for groups of few rows; absent from the call otherwise
        constraints["split_kv"] = True
    if check_kv_cache_dtype(cfg.gen.get("kv_cache_dtype")) is not None:   # gen.kv_cache_dtype: fp8; auto (or the key absent) is absent from the call
        constraints["kv_cache_dtype"] = "fp8"
    if check_weight_dtype(cfg.gen.get("weight_dtype"), bool(cfg.gen.get("small_batch") or False)) is not None:   # gen.weight_dtype: fp8 (needs gen.small_batch); auto (or the key absent) is absent from the call
        constraints["weight_dtype"] = "fp8"
    if bool(cfg.gen.get("mbr") or False):                  # gen.mbr: outputs in minimum-Bayes-risk order; absent from the call otherwise
        constraints["mbr"] = True
    constraints.update(pool)          # gen.continuous: batch_size is a pool of rows that is refilled; false (or the key absent) is absent from the call
    summary = generate_file(t.model, t.tokenizer, None if prompts is not None else str(cfg.gen.input), out_path,
                            max_new_tokens=int(cfg.sampling_params.max_tokens), stop_token_ids=None if stop is None else [int(s) for s in stop],
                            tokenizer_decoding={k: cfg.tokenizer_decoding[k] for k in cfg.tokenizer_decoding}, prompts=prompts, ids=ids,
                            batch_size=int(cfg.gen.batch_size), logprobs=bool(cfg.gen.logprobs), device=t.device, **constraints)
    LOGGER.info(" | ".join(f"{k}: {v}" for k, v in summary.items()) + f" | wrote {out_path}")
    return summary


if __name__ == "__main__":
    main()
