#!/usr/bin/env python
"""Likelihood scoring at full size (`ssi.score.score_sequences`): 1B model, bf16, seeded random weights.  Two synthetic sets of speech-unit
sequences — 4096 with lengths U(16, 64) (word- and sentence-pair items) and 512 with lengths U(400, 1100) (utterances) — scored packed into
rows of 2048, and a 256-item sample of the short set scored one sequence per row in batches of 8 rows (each row as long as the sample's
longest item: the only way to get per-sequence numbers through the batch loss, a forward per batch and a read-back per row).  Every case runs
once untimed and then `reps` times; the result is sequences/s and scored tokens/s of the median run.
usage: python tools/score_bench.py [out.json] [reps=3]"""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speech-integration_amd")
sys.path[:0] = [ROOT, PKG]
import torch  # noqa: E402
from ssi.config import compose  # noqa: E402
from ssi.eval import SeqScores  # noqa: E402
from ssi.loss import compute_loss  # noqa: E402
from ssi.model import get_device, get_dtype  # noqa: E402
from ssi.score import score_sequences, scoring_batches  # noqa: E402
from ssi.trainer import Trainer  # noqa: E402

reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
tmp = tempfile.mkdtemp(prefix="ssi_score_")
cfg = compose(os.path.join(PKG, "conf"), "score", ["speech.n_dsus=5000", "dtype=bf16", f"output_dir={tmp}", f"checkpointer.checkpoint_dir={tmp}/none",
                                                   "checkpointer.allow_random_init=true", "score.input=-", "score.output=-"])
t = Trainer(cfg)
t.device, t.dtype = get_device(cfg.device), get_dtype(cfg.dtype)
t._setup_model()
t._setup_tokenizer()
t._setup_loss()
lo, hi = t.token_type_ranges["dsu"]
g = torch.Generator().manual_seed(17)


def units(n_items, a, b):
    return [torch.randint(lo, hi + 1, (int(n),), generator=g) for n in torch.randint(a, b + 1, (n_items,), generator=g)]


def one_per_row(seqs):
    """Every sequence a row of its own, 8 rows per batch, the four numbers of each row read back batch by batch."""
    row_len = max(s.numel() for s in seqs)
    out = []
    with torch.inference_mode():
        for batch in scoring_batches(seqs, [1] * len(seqs), [[i] for i in range(len(seqs))], row_len, 8, pad_id=0):
            batch.pop("seq_index")
            res = torch.zeros(batch["tokens"].shape[0], 4, dtype=torch.float64, device=t.device)
            scores = SeqScores(batch.pop("seq_spans"), 5, res)
            compute_loss({k: v.to(t.device) for k, v in batch.items()}, t.model, t.loss_fn, seq_scores=scores)
            out.append(res.cpu())
    return torch.cat(out)


def timed(name, fn, n_seq, n_tok):
    fn()  # not timed: code objects, the arena at this shape
    secs = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    med = statistics.median(secs)
    run = {"sequences": n_seq, "scored_tokens": n_tok, "seconds": [round(s, 4) for s in secs], "sequences_per_s": round(n_seq / med, 1),
           "scored_tokens_per_s": round(n_tok / med, 1)}
    print(f"{name}: {run}", flush=True)
    return run


short, long_ = units(4096, 16, 64), units(512, 400, 1100)
sample = short[:256]
kw = dict(pad_id=0, device=t.device, row_len=2048, rows_per_batch=8, topk=5, loss_fn=t.loss_fn)
res = {"model": "Llama-3.2-1B + 5000 units, bf16, random weights", "row_len": 2048, "rows_per_batch": 8, "reps": reps, "runs": {}}
for name, seqs, fn in (("short_packed", short, lambda: score_sequences(t.model, short, **kw)),
                       ("long_packed", long_, lambda: score_sequences(t.model, long_, **kw)),
                       ("sample_packed", sample, lambda: score_sequences(t.model, sample, **kw)),
                       ("sample_one_per_row", sample, lambda: one_per_row(sample))):
    res["runs"][name] = timed(name, fn, len(seqs), sum(s.numel() - 1 for s in seqs))
packed, alone = score_sequences(t.model, sample, **kw), one_per_row(sample)
res["sample_worst_rel_diff_of_sum_nll"] = float(((-packed.logprob - alone[:, 1]).abs() / alone[:, 1].abs()).max())
res["sample_counts_equal"] = bool((packed.n_tokens == alone[:, 0].long()).all())
res["sample_packed_over_one_per_row"] = round(res["runs"]["sample_packed"]["sequences_per_s"] / res["runs"]["sample_one_per_row"]["sequences_per_s"], 2)
print({k: v for k, v in res.items() if k.startswith("sample_")}, flush=True)
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
