#!/usr/bin/env python
"""Byte-pair encoding over discrete speech units: learn merges on the device, encode a JSONL with them, and report the compression.
    python scripts/unit_bpe.py train units.jsonl --n-base 5000 --n-merges 3000 --output merges.json [--column speech_tokens] [--max-ids N]
    python scripts/unit_bpe.py encode units.jsonl merges.json --output encoded.jsonl
    python scripts/unit_bpe.py stats units.jsonl merges.json
The merges file is what ``speech.unit_bpe`` names; ``speech.n_dsus`` is then its n_base + n_merges.
"""
import json
import logging
import os
import sys
from argparse import ArgumentParser, Namespace
from pathlib import Path

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from ssi.tokenizer import deduplicate_units  # noqa: E402
from ssi.tokenizer import unit_bpe as UB  # noqa: E402

LOGGER = logging.getLogger(__name__)
ENCODE_BATCH = 4096   # sequences per launch of the encode kernel


def parse_args(argv=None) -> Namespace:
    parser = ArgumentParser(description="Byte-pair encoding over discrete speech units.")
    sub = parser.add_subparsers(dest="command", required=True)

    def common(p, merges: bool):
        p.add_argument("jsonl", type=Path, help="JSONL with one sample per line")
        if merges:
            p.add_argument("merges", type=Path, help="merges file written by train")
        p.add_argument("--column", type=str, default="speech_tokens", help="key that holds the list of units")
        p.add_argument("--dedup", dest="dedup", action="store_true", default=True, help="collapse runs of equal units first (speech.deduplicate; default)")
        p.add_argument("--no-dedup", dest="dedup", action="store_false")
        p.add_argument("--device", type=str, default="cuda")

    t = sub.add_parser("train", help="learn merges and write the merges file (never overwritten)")
    common(t, merges=False)
    t.add_argument("--n-base", type=int, required=True, help="number of units of the tokenizer (the data config's n_dsus)")
    t.add_argument("--n-merges", type=int, required=True)
    t.add_argument("--min-frequency", type=int, default=2)
    t.add_argument("--max-ids", type=int, default=None, help="train on the first sequences that hold at most this many ids")
    t.add_argument("--output", type=Path, required=True)
    e = sub.add_parser("encode", help="write the JSONL with the units column replaced by its encoding (never overwritten)")
    common(e, merges=True)
    e.add_argument("--host", action="store_true", help="encode on the host (UnitBPE.encode) instead of the kernel")
    e.add_argument("--output", type=Path, required=True)
    s = sub.add_parser("stats", help="compression ratio and length histogram")
    common(s, merges=True)
    s.add_argument("--host", action="store_true")
    return parser.parse_args(argv)


def read_rows(path: Path) -> list[dict]:
    with open(path, encoding="utf-8") as f:
        return [json.loads(line) for line in f if line.strip()]


def units_of(rows: list[dict], column: str, dedup: bool) -> list[list[int]]:
    out = []
    for i, r in enumerate(rows):
        if column not in r:
            raise KeyError(f"line {i + 1} has no key {column!r} (keys: {sorted(r)})")
        units = [int(u) for u in r[column]]
        out.append(deduplicate_units(units) if dedup else units)
    return out


def refuse_overwrite(path: Path) -> None:
    if path.exists():
        raise FileExistsError(f"{path} is already there and is not overwritten")


def encode_all(bpe, seqs: list[list[int]], device: str, host: bool) -> list[list[int]]:
    """The kernel for every sequence it takes, the host encoder for longer ones."""
    from ssi import _lib
    if host:
        return [bpe.encode(s) for s in seqs]
    out: list = [None] * len(seqs)
    short = [i for i, s in enumerate(seqs) if len(s) <= _lib.BPE_ENCODE_MAX_LEN]
    for at in range(0, len(short), ENCODE_BATCH):
        idx = short[at:at + ENCODE_BATCH]
        for i, enc in zip(idx, bpe.encode_many([seqs[i] for i in idx], device=device)):
            out[i] = enc
    for i, s in enumerate(seqs):
        if out[i] is None:
            out[i] = bpe.encode(s)
    return out


def train(args: Namespace) -> dict:
    refuse_overwrite(args.output)
    seqs = units_of(read_rows(args.jsonl), args.column, args.dedup)
    left_out = 0
    if args.max_ids is not None:
        total, keep = 0, 0
        for s in seqs:
            if total + len(s) > args.max_ids:
                break
            total += len(s)
            keep += 1
        left_out = len(seqs) - keep
        print(f"--max-ids {args.max_ids}: training on the first {keep} sequences ({total} ids); left out {left_out} sequences "
              f"({sum(len(s) for s in seqs[keep:])} ids)")
        seqs = seqs[:keep]
    bpe = UB.train(seqs, args.n_base, args.n_merges, args.min_frequency, device=args.device)
    with open(args.output, "x", encoding="utf-8") as f:
        json.dump(bpe.to_dict(), f)
        f.write("\n")
    c = bpe.corpus
    print(f"{bpe.n_merges} merges (asked for {args.n_merges}); {c['ids_before']} ids -> {c['ids_after']} "
          f"(ratio {c['ids_before'] / max(c['ids_after'], 1):.3f}); speech.n_dsus = {bpe.vocab_size}; wrote {args.output}")
    return {"n_merges": bpe.n_merges, "left_out": left_out, **c}


def encode(args: Namespace) -> dict:
    refuse_overwrite(args.output)
    bpe = UB.UnitBPE.load(args.merges)
    rows = read_rows(args.jsonl)
    encoded = encode_all(bpe, units_of(rows, args.column, args.dedup), args.device, args.host)
    with open(args.output, "x", encoding="utf-8") as f:
        for r, e in zip(rows, encoded):
            f.write(json.dumps({**r, args.column: e}) + "\n")
    print(f"wrote {args.output} ({len(rows)} lines)")
    return {"lines": len(rows)}


def stats(args: Namespace) -> dict:
    bpe = UB.UnitBPE.load(args.merges)
    seqs = units_of(read_rows(args.jsonl), args.column, args.dedup)
    encoded = encode_all(bpe, seqs, args.device, args.host)
    before, after = sum(map(len, seqs)), sum(map(len, encoded))
    edges = [0, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
    hist = lambda lens: {f"{lo}-{hi - 1}" if hi else f"{lo}+": sum(lo <= n and (not hi or n < hi) for n in lens)   # noqa: E731
                         for lo, hi in zip(edges, edges[1:] + [None])}
    result = {"sequences": len(seqs), "ids_before": before, "ids_after": after, "ratio": before / max(after, 1),
              "lengths_before": hist(list(map(len, seqs))), "lengths_after": hist(list(map(len, encoded)))}
    print(json.dumps(result, indent=2))
    return result


def main(args: Namespace) -> dict:
    return {"train": train, "encode": encode, "stats": stats}[args.command](args)


if __name__ == "__main__":
    logging.basicConfig(level=os.environ.get("LOG_LEVEL", "INFO").upper(), stream=sys.stdout, force=True)
    main(parse_args())
