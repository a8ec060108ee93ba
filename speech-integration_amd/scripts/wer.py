#!/usr/bin/env python
"""Word error rate of a generations JSONL (the reference's scripts/wer.py, on ssi_edit_distance instead of `evaluate`): writes wer.json beside
the generations and refuses to overwrite it.
    python scripts/wer.py out/generations.jsonl --references refs.jsonl [--normalizer basic] [--level word]
    python scripts/wer.py <dataset>/<split>/generations.jsonl            # references from the Hugging Face dataset, as the reference does
"""
import json
import logging
import os
import sys
from argparse import ArgumentParser, Namespace
from pathlib import Path
from pprint import pformat

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from ssi import wer as W  # noqa: E402

LOGGER = logging.getLogger(__name__)


def parse_args(argv=None) -> Namespace:
    parser = ArgumentParser(description="Error rate of generated transcripts against their references.")
    parser.add_argument("generations_jsonl", type=Path, help="generations JSONL, as scripts/generate.py writes it")
    parser.add_argument("--dataset", type=str, help="dataset that holds the references (default: the grandparent folder's name)")
    parser.add_argument("--split", type=str, help="split of that dataset (default: the parent folder's name)")
    parser.add_argument("--gt_transcript_colname", type=str, default="transcript", help="column (or JSONL key) of the reference text")
    parser.add_argument("--normalizer", type=str, default="whisper", choices=list(W.NORMALIZERS), help="applied to both sides before splitting")
    parser.add_argument("--references", type=Path, default=None,
                        help="References from a file instead of a dataset: a JSONL with id and text (or the transcript column) per line, "
                             "or a text file with one reference per line in the order of the generations.")
    parser.add_argument("--level", type=str, default="word", choices=["word", "char"], help="Unit of the error rate.")
    parser.add_argument("--device", type=str, default="cuda", help="Device of the edit-distance kernel.")
    return parser.parse_args(argv)


def dataset_references(dataset: str, split: str, column: str) -> list[str]:
    try:
        from datasets import load_dataset
    except ImportError as e:
        raise ImportError("--dataset / --split need the `datasets` package, which is not installed; pass --references FILE") from e
    return list(load_dataset(dataset, split=split)[column])


def main(args: Namespace) -> dict:
    wer_json = args.generations_jsonl.parent / "wer.json"
    if wer_json.exists():
        with open(wer_json) as f:
            contents = pformat(json.load(f))
        raise FileExistsError(f"{wer_json} is already there and is not overwritten; it holds: " + contents)
    ids, generated = W.read_generations(str(args.generations_jsonl))
    if args.references is not None:
        reference = W.read_references(str(args.references), ids, args.gt_transcript_colname)
    else:
        if args.dataset is None:
            args.dataset = args.generations_jsonl.parents[1].name
            LOGGER.info(f"dataset taken from the path: {args.dataset}")
        if args.split is None:
            args.split = args.generations_jsonl.parent.name
            LOGGER.info(f"split taken from the path: {args.split}")
        reference = dataset_references(args.dataset, args.split, args.gt_transcript_colname)
    result = W.error_rate(reference, generated, level=args.level, normalizer=args.normalizer, device=args.device)
    result.update(level=args.level, normalizer=args.normalizer)
    with open(wer_json, "x") as f:
        json.dump(result, f, indent=4)
    LOGGER.info(" | ".join(f"{k}: {v}" for k, v in result.items()))
    LOGGER.info(f"wrote {wer_json}")
    return result


if __name__ == "__main__":
    logging.basicConfig(level=os.environ.get("LOG_LEVEL", "INFO").upper(), stream=sys.stdout, force=True)
    main(parse_args())
