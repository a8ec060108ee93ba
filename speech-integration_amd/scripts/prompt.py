#!/usr/bin/env python
"""Generate from one prompt (or a few): a raw string, raw token ids, or a Jinja2 template with the speech and modality variables.  Greedy with one
sample by default; the text goes to stdout (the reference plans this as its standalone sample-wise generation; it has no such tool).
    python scripts/prompt.py --checkpoint-dir CKPT --n-dsus 5000 --prompt "The capital of France is"
    python scripts/prompt.py --checkpoint-dir CKPT --n-dsus 5000 --tokens "128000 791 6864"
    python scripts/prompt.py --checkpoint-dir CKPT --n-dsus 5000 --template asr.j2 --units "17 17 403 9" --dedup --var lang=en -n 4 --temperature 0.8
A decode step of these few rows runs unpadded on the skinny GEMMs (ssi.prompting.probe, small_batch=True).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--checkpoint-dir", required=True, help="directory of the extended model's checkpoint (checkpointer.checkpoint_dir)")
    p.add_argument("--n-dsus", type=int, required=True, help="number of speech units of the extended vocabulary (speech.n_dsus)")
    p.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"))
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--prompt", action="append", help="a raw text prompt (may be repeated)")
    src.add_argument("--tokens", action="append", help="a prompt as token ids separated by spaces or commas (may be repeated)")
    src.add_argument("--template", help="a Jinja2 template: a path, or the template itself")
    p.add_argument("--var", action="append", default=[], metavar="K=V", help="a template variable (may be repeated)")
    p.add_argument("--units", help="speech units for the template's speech_units variable, separated by spaces or commas")
    p.add_argument("--dedup", action="store_true", help="collapse runs of equal speech units before they are rendered")
    p.add_argument("--unit-bpe", metavar="FILE", help="a merges file of scripts/unit_bpe.py train: the --units are BPE-encoded (after --dedup); "
                                                      "--n-dsus is then its n_base + n_merges")
    p.add_argument("--max-new-tokens", type=int, default=128)
    p.add_argument("-n", type=int, default=1, help="samples per prompt (needs --temperature > 0)")
    p.add_argument("--temperature", type=float, default=0.0, help="0: greedy decoding")
    p.add_argument("--top-k", type=int, default=-1)
    p.add_argument("--top-p", type=float, default=1.0)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--repetition-penalty", type=float, default=1.0)
    p.add_argument("--frequency-penalty", type=float, default=0.0)
    p.add_argument("--presence-penalty", type=float, default=0.0)
    p.add_argument("--split-kv", action="store_true", help="split-KV decode attention: the keys of a row over several workgroups (long prompts)")
    p.add_argument("--kv-cache-dtype", choices=("auto", "fp8"), default="auto",
                   help="fp8: the K/V cache as e4m3 codes with one power-of-two scale per cached line (changes values); auto: the model's dtype")
    p.add_argument("--weight-dtype", choices=("auto", "fp8"), default="auto",
                   help="fp8: the decode steps read the projection weights and the head as e4m3 codes with one power-of-two scale per output "
                        "channel, quantised once (changes values); auto: the model's weights")
    p.add_argument("--mbr", action="store_true",
                   help="print a prompt's samples in minimum-Bayes-risk order (by expected token error rate against each other); needs -n >= 2")
    p.add_argument("--jsonl", metavar="OUT", help="also write one record per prompt (the generations file's line format)")
    return p


def ints(text: str) -> list[int]:
    return [int(t) for t in text.replace(",", " ").split()]


def template_variables(args) -> dict:
    out = {}
    for kv in args.var:
        if "=" not in kv:
            raise ValueError(f"--var {kv!r}: K=V")
        k, v = kv.split("=", 1)
        out[k] = v
    if args.units is not None:
        out["speech_units"] = ints(args.units)
    return out


def prompts_of(args, tokenizer) -> list[list[int]]:
    """The prompts' token ids from the parsed arguments (``ValueError`` for --var / --units / --dedup without --template)."""
    from ssi.prompting import render_prompt
    unit_bpe = getattr(args, "unit_bpe", None)
    if args.template is None and (args.var or args.units is not None or args.dedup or unit_bpe is not None):
        raise ValueError("--var, --units, --dedup and --unit-bpe belong to --template")
    if args.template is not None:
        return [render_prompt(tokenizer, template=args.template, variables=template_variables(args), deduplicate=args.dedup,
                              **({} if unit_bpe is None else {"unit_bpe": unit_bpe}))]
    if args.tokens is not None:
        return [render_prompt(tokenizer, token_ids=ints(t)) for t in args.tokens]
    return [render_prompt(tokenizer, text=t) for t in args.prompt]


def check_sampling_options(args) -> None:
    """What ``probe`` would refuse, refused before anything is loaded: temperature 0 is greedy decoding of one sample (``ValueError``)."""
    if args.temperature < 0 or args.n < 1 or args.max_new_tokens < 1:
        raise ValueError("--temperature must be >= 0, -n and --max-new-tokens >= 1")
    if args.temperature == 0 and (args.n != 1 or args.top_k > 0 or args.top_p != 1.0):
        raise ValueError("-n, --top-k and --top-p need --temperature > 0 (temperature 0 is greedy decoding: one sample, no top-k, no top-p)")
    if args.template is None and (args.var or args.units is not None or args.dedup):
        raise ValueError("--var, --units and --dedup belong to --template")
    if getattr(args, "mbr", False) and args.n < 2:
        raise ValueError("--mbr chooses among a prompt's samples: -n >= 2 (and --temperature > 0)")


def load(args):
    """Model and tokenizer as a generation run sets them up, from the committed generate configuration."""
    from ssi.config import compose
    from ssi.model import get_device, get_dtype
    from ssi.train_utils import resolve_n_dsus
    from ssi.trainer import Trainer
    conf = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "conf")
    cfg = compose(conf, "generate", [f"speech.n_dsus={args.n_dsus}", f"checkpointer.checkpoint_dir={args.checkpoint_dir}", f"dtype={args.dtype}",
                                     "gen.output_dir=."] + ([f"speech.unit_bpe={args.unit_bpe}"] if getattr(args, "unit_bpe", None) else []))
    resolve_n_dsus(cfg)
    t = Trainer(cfg)
    t.device, t.dtype = get_device(cfg.device), get_dtype(cfg.dtype)
    t._setup_model()
    t._setup_tokenizer()
    return t.model, t.tokenizer, {k: cfg.tokenizer_decoding[k] for k in cfg.tokenizer_decoding}


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    check_sampling_options(args)          # before the checkpoint is loaded
    from ssi.prompting import probe, prompt_records
    model, tokenizer, decoding = load(args)
    prompts = prompts_of(args, tokenizer)
    found = probe(model, tokenizer, prompts, max_new_tokens=args.max_new_tokens, n=args.n, temperature=args.temperature, top_k=args.top_k,
                  top_p=args.top_p, seed=args.seed, repetition_penalty=args.repetition_penalty, frequency_penalty=args.frequency_penalty,
                  presence_penalty=args.presence_penalty, tokenizer_decoding=decoding, split_kv=args.split_kv,
                  kv_cache_dtype=args.kv_cache_dtype, weight_dtype=args.weight_dtype, **({"mbr": True} if args.mbr else {}))
    for p in found:
        for text in p.texts:
            print(text)
    if args.jsonl:
        with open(args.jsonl, "w", encoding="utf-8") as f:
            for rec in prompt_records(found, tokenizer, decoding):
                f.write(json.dumps(rec, ensure_ascii=False) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
