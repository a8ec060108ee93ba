#!/usr/bin/env python
"""Likelihood scoring entry point (not in the reference): the log-probability of every sequence of a JSONL file, and pair accuracy where
the file names pairs (ssi/score.py).
    python scripts/score.py speech.n_dsus=5000 score.input=items.jsonl score.output=scores.jsonl [key=value ...]
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

from ssi.score import score_file
from ssi.model import get_device, get_dtype
from ssi.train_utils import resolve_n_dsus
from ssi.trainer import Trainer

LOGGER = logging.getLogger(__name__)


@main_decorator(config_path="../conf", config_name="score", version_base=None)
def main(cfg):
    resolve_n_dsus(cfg)
    t = Trainer(cfg)  # model, tokenizer and checkpointer as a training run sets them up; no optimizer, no data loaders
    t.device, t.dtype = get_device(cfg.device), get_dtype(cfg.dtype)
    t._setup_model()
    t._setup_tokenizer()
    t._setup_loss()
    summary = score_file(t.model, t.tokenizer, str(cfg.score.input), str(cfg.score.output), device=t.device, row_len=int(cfg.score.row_len),
                         rows_per_batch=int(cfg.score.rows_per_batch), topk=int(cfg.score.topk), loss_fn=t.loss_fn)
    LOGGER.info(" | ".join(f"{k}: {v}" for k, v in summary.items()))
    return summary


if __name__ == "__main__":
    main()
