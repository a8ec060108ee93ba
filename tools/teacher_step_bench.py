"""Step time of the trainer with and without the frozen teacher (``teacher_kl_coeff``) on the synthetic headline geometry of ``bench.py
--through-trainer``: Llama-3.2-1B + 5000 DSUs, batch 8 x 2048, bf16, gradient_accumulation_steps 1, random-init weights.  One JSON line:
``ms_per_step`` (mean and median over the steps after the warm-up) of a run without the option, with it on every labelled position, and with it
on text labels only (``teacher_kl_token_types=[text]``), in that order, each in a fresh trainer.

    python tools/teacher_step_bench.py [--steps 15] [--warmup 5] [--coeff 0.5]"""
import argparse
import json
import os
import shutil
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speech-integration_amd")
sys.path.insert(0, PKG)


def run(args, extra):
    from ssi.config import compose
    from ssi.train_utils import resolve_n_dsus
    from ssi.trainer import Trainer
    tmp = tempfile.mkdtemp(prefix="ssi_teacher_step_")
    steps = args.warmup + args.steps
    cfg = compose(os.path.join(PKG, "conf"), "sft", [
        "data=sft/mls-hubert_large_ll60k-layer_22", "dtype=bf16", f"max_steps={steps}", "gradient_accumulation_steps=1",
        f"tokenizer.max_seq_len={args.seq}", f"data.train.dataset.n_samples={steps * args.batch}", "data.dev.dataset.n_samples=8",
        f"data.train.dataloader.batch_size={args.batch}", "eval_steps=1000000000", "save_steps=1000000000", f"output_dir={tmp}",
        f"checkpointer.output_dir={tmp}/ckpt", f"checkpointer.checkpoint_dir={tmp}/none", "checkpointer.allow_random_init=true",
        "speech.n_dsus=5000", *extra])
    resolve_n_dsus(cfg)
    t = Trainer(cfg)
    t.setup()
    t.train()
    torch.cuda.synchronize()
    rec = t.wandb_logger.records[args.warmup:]
    assert len(rec) == args.steps
    dur = sorted(1e3 * r["duration_step"] for r in rec)
    out = {"ms_per_step_mean": round(sum(dur) / len(dur), 3), "ms_per_step_median": round(dur[len(dur) // 2], 3), "ms_per_step_min": round(dur[0], 3),
           "last_loss": rec[-1]["loss"], "last_kl_loss": rec[-1].get("kl_loss")}
    t.cleanup()
    del t
    torch.cuda.empty_cache()
    shutil.rmtree(tmp, ignore_errors=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--coeff", type=float, default=0.5)
    args = ap.parse_args()
    on = [f"teacher_kl_coeff={args.coeff}"]
    runs = {"without": run(args, []), "with_teacher": run(args, on), "with_teacher_text_only": run(args, [*on, "teacher_kl_token_types=[text]"])}
    print(json.dumps({"what": "trainer step time with and without teacher_kl_coeff", "batch": args.batch, "seq": args.seq, "dtype": "bf16",
                      "steps": args.steps, "warmup": args.warmup, "teacher_kl_coeff": args.coeff, "runs": runs}))
