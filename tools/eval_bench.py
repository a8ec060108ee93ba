#!/usr/bin/env python
"""Dev-set loss at full size (`Trainer._evaluate()`, reference ssi/eval.py:15-41): 1B model, bf16, N ragged dev samples in the dev loader's
batches of 2 rows — batch by batch as the reference runs them, and `eval_join_batches` at a time as one batch (ssi/eval.py, round 5); each
also with `eval_token_metrics` on (loss and top-k accuracy per token type from the label-rank cross-entropy kernel): off and on alternate, every
combination twice, in this one process.  The yardstick of an "on" run is the "off" run of the same call.
usage: python tools/eval_bench.py [n_samples=512] [out.json]"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speech-integration_amd")
sys.path[:0] = [ROOT, PKG]
import torch  # noqa: E402
from ssi.config import compose  # noqa: E402
from ssi.train_utils import resolve_n_dsus  # noqa: E402
from ssi.trainer import Trainer  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
tmp = tempfile.mkdtemp(prefix="ssi_eval_")
cfg = compose(os.path.join(PKG, "conf"), "sft", [
    "data=sft/mls-hubert_large_ll60k-layer_22", "dtype=bf16", "max_steps=1", "tokenizer.max_seq_len=2048", "data.train.dataset.n_samples=8",
    f"data.dev.dataset.n_samples={n}", "data.dev.dataset.fixed_len=false", "data.dev.dataloader.batch_size=2", f"output_dir={tmp}",
    f"checkpointer.output_dir={tmp}/ckpt", f"checkpointer.checkpoint_dir={tmp}/none", "checkpointer.allow_random_init=true", "speech.n_dsus=5000"])
resolve_n_dsus(cfg)
t = Trainer(cfg)
t.setup()
res = {"dev_samples": n, "dev_batch_size": 2, "runs": {}}
t.cfg.eval_join_batches, t.cfg.eval_token_metrics = 16, True
t._evaluate()  # not timed: the first pass loads code objects and grows the arena to the joined batches' size
for join, metrics in ((16, False), (16, True), (0, False), (0, True)) * 2:
    t.cfg.eval_join_batches, t.cfg.eval_token_metrics = join, metrics
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    value = t._evaluate()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    run = {"seconds": round(dt, 3), "dev_loss": value}
    if metrics:
        run["metrics"] = {k: v for k, v in t.dev_metrics.items() if k != "dev_loss"}
    res["runs"].setdefault(f"join_{join}" + ("_metrics" if metrics else ""), []).append(run)
    print(f"eval_join_batches={join:2d} eval_token_metrics={int(metrics)}: {dt:.3f} s, dev loss {value:.6f}", flush=True)
for join in (16, 0):
    off, on = ([r["seconds"] for r in res["runs"][f"join_{join}{sfx}"]] for sfx in ("", "_metrics"))
    res[f"join_{join}_summary"] = {"off_s": off, "on_s": on, "off_spread_pct": round(100 * (max(off) - min(off)) / min(off), 2),
                                  "on_over_off_pct": round(100 * (sum(on) / sum(off) - 1), 2),
                                  "dev_loss_bit_equal": len({r["dev_loss"] for sfx in ("", "_metrics") for r in res["runs"][f"join_{join}{sfx}"]}) == 1}
    print(f"join {join}: {res[f'join_{join}_summary']}", flush=True)
if len(sys.argv) > 2:
    json.dump(res, open(sys.argv[2], "w"), indent=1)
t.cleanup()
