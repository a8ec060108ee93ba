"""CPU: ``ssi.eval.compute_dataset_metrics`` on its plain-torch route (a model without ``fused_loss``): the rank rule on hand-made ties, the
token-level aggregation over batches of unequal size, the type of the LABEL through ``get_token_type_ranges`` of a real vocabulary layout, the
all-reduce over two gloo ranks, and the config defaults.  The GPU route (``ssi_ce_fwd_metrics``) is held to the same arithmetic in
tests/test_ce_metrics_gpu.py."""
import copy
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from conftest import PKG, ROOT

V = 16
REL = 1e-6   # per-token nll is fp32 arithmetic on the logits (as the reference's loss and the kernel), summed in fp64: a few fp32 roundings (6e-8 each)
RANGES = {"text": (0, 5), "dsu": (6, 11), "modality": (12, 13), "special_text": (14, 15)}


class _Loss:
    """sum NLL / count(labels != ignore_index) over flat logits: what the reference's loss computes, without its chunking."""
    ignore_index = -100

    def __call__(self, logits, labels):
        if isinstance(logits, list):   # chunks along the sequence, labels [B, S]
            logits, labels = torch.cat(logits, dim=1).reshape(-1, V), labels.reshape(-1)
        return F.cross_entropy(logits.float(), labels, ignore_index=self.ignore_index, reduction="sum") / (labels != self.ignore_index).sum()


class _Stub:
    """A model whose logits at a position are a fixed row chosen by the token there: ``table[token]``."""

    def __init__(self, table, chunks=0):
        self.table, self.chunks, self.training = table, chunks, True

    def eval(self):
        self.training = False

    def train(self):
        self.training = True

    def __call__(self, tokens, mask=None, encoder_input=None, encoder_mask=None, input_pos=None):
        logits = self.table[tokens]
        return list(logits.chunk(self.chunks, dim=1)) if self.chunks else logits


def _table(seed=3):
    """Rows with ties: values drawn from a few levels, so that equal logits above, below and at the label are common."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 4, (V, V), generator=g).float() * 0.75


def _batches(seed=4, sizes=((2, 9), (3, 5), (1, 12), (2, 7))):
    g = torch.Generator().manual_seed(seed)
    out = []
    for b, s in sizes:
        tok = torch.randint(0, 12, (b, s), generator=g)        # no token of the last two types: no LABEL of them either
        lab = tok.clone()
        lab[0, :2] = -100
        lab[-1, -2:] = -100
        out.append({"tokens": tok, "labels": lab})
    return out


def _by_definition(table, batches, ranges, topk):
    """Every (logits row, shifted label) pair of the dev set in one go; rank = the label's position in a stable descending sort."""
    rows, labels = [], []
    for b in batches:
        shifted = torch.hstack((b["labels"][:, 1:], torch.full_like(b["labels"][:, -1:], -100)))
        rows.append(table[b["tokens"]].reshape(-1, V))
        labels.append(shifted.reshape(-1))
    x, lab = torch.cat(rows), torch.cat(labels)
    x, lab = x[lab != -100], lab[lab != -100]
    order = torch.sort(x, dim=1, descending=True, stable=True).indices
    rank = (order == lab[:, None]).int().argmax(1)
    nll = F.cross_entropy(x.double(), lab, reduction="none")
    out = {}
    for name, (lo, hi) in list(ranges.items()) + [("all", (0, V - 1))]:
        m = (lab >= lo) & (lab <= hi)
        n = int(m.sum())
        out[f"dev_n_labels.{name}"] = n
        if n:
            out[f"dev_loss.{name}"] = float(nll[m].sum() / n)
            out[f"dev_acc.{name}"] = float((rank[m] == 0).sum()) / n
            out[f"dev_acc_top{topk}.{name}"] = float((rank[m] < topk).sum()) / n
    return out


def _run(model, batches, ranges=RANGES, topk=3, metrics=True):
    from ssi.eval import compute_dataset_loss, compute_dataset_metrics
    kw = dict(epoch=0, global_step=1, steps_per_epoch=10, device=torch.device("cpu"))
    data = [{k: v.clone() for k, v in b.items()} for b in batches]
    if metrics:
        return compute_dataset_metrics(model, data, _Loss(), token_type_ranges=ranges, topk=topk, **kw)
    return compute_dataset_loss(model, data, _Loss(), **kw)


def test_the_rank_rule_on_hand_made_ties():
    from ssi.eval import LabelMetrics
    x = torch.tensor([[1.0, 3.0, 3.0, 0.0, 3.0],    # label 2: one equal maximum before it, one after            -> rank 1
                      [1.0, 3.0, 3.0, 0.0, 3.0],    # label 1: the first of the equal maxima                       -> rank 0 (argmax)
                      [2.0, 2.0, 2.0, 2.0, 2.0],    # all equal                                                    -> rank == label = 3
                      [0.5, -1.0, 4.0, 0.5, 0.0],   # label 3: one above, an equal value at a smaller index        -> rank 2
                      [0.5, -1.0, 4.0, 0.5, 0.0],   # ignored
                      [0.5, -1.0, 4.0, 0.5, 0.0]])  # out of range: counts nowhere
    labels = torch.tensor([2, 1, 3, 3, -100, 5])
    for topk, hits in ((1, 1), (2, 2), (3, 3), (4, 4)):
        m = LabelMetrics({"low": (0, 2), "high": (3, 4), "none": (7, 9)}, topk, torch.device("cpu"))
        m.add_logits(x[None], labels[None], -100)
        n, nll, top1, topn = m.acc[-1].tolist()
        assert (n, top1, topn) == (4, 1, hits)
        assert nll == pytest.approx(float(F.cross_entropy(x[:4].double(), labels[:4], reduction="sum")), rel=REL)
        assert m.acc[:, 0].tolist() == [2, 2, 0, 4] and m.acc[0, 2] == 1 and m.acc[1, 2] == 0
        r = m.result()
        assert r["dev_n_labels.none"] == 0 and not [k for k in r if k.endswith(".none") and not k.startswith("dev_n_labels")]
        assert r[f"dev_acc_top{topk}.all"] == hits / 4 and r["dev_acc.low"] == 0.5
    assert (x[:4].argmax(1) == labels[:4]).tolist() == [False, True, False, False]   # rank 0 <=> torch's first-occurrence argmax
    with pytest.raises(ValueError):
        LabelMetrics({"all": (0, 1)}, 5, torch.device("cpu"))
    with pytest.raises(ValueError):
        LabelMetrics({"a": (0, 1)}, 0, torch.device("cpu"))


@pytest.mark.parametrize("chunks", [0, 4])
def test_token_level_values_over_batches_of_unequal_size(chunks):
    table, batches = _table(), _batches()
    got = _run(_Stub(table, chunks), batches)
    want = _by_definition(table, batches, RANGES, 3)
    assert set(got) == set(want) | {"dev_loss"}
    for k, v in want.items():
        assert got[k] == (v if k.startswith("dev_n_labels") else pytest.approx(v, rel=REL)), k
    assert got["dev_n_labels.text"] > 0 and got["dev_n_labels.dsu"] > 0
    assert 0 < got["dev_acc.all"] < got["dev_acc_top3.all"] < 1
    # types without labels report their count alone: no NaN reaches the log record
    for name in ("modality", "special_text"):
        assert got[f"dev_n_labels.{name}"] == 0 and not {f"dev_loss.{name}", f"dev_acc.{name}", f"dev_acc_top3.{name}"} & set(got)
    assert sum(got[f"dev_n_labels.{n}"] for n in RANGES) == got["dev_n_labels.all"]
    # dev_loss is compute_dataset_loss's value, bit for bit (it is batch-weighted, so it is NOT dev_loss.all)
    assert got["dev_loss"] == _run(_Stub(table, chunks), batches, metrics=False)
    # token-level: the same dev set batched differently gives the same per-type values
    rows = [{k: v[i:i + 1] for k, v in b.items()} for b in batches for i in range(b["tokens"].shape[0])]
    one_by_one = _run(_Stub(table, chunks), rows)
    for k, v in want.items():
        assert one_by_one[k] == (v if k.startswith("dev_n_labels") else pytest.approx(v, rel=REL)), k


def test_the_type_is_that_of_the_label_in_a_real_vocabulary_layout():
    from ssi.eval import LabelMetrics
    from ssi.llama_configs import configllama3_2_1b
    from ssi.train_utils import get_token_type_ranges
    c = copy.deepcopy(configllama3_2_1b)
    c.n_dsus, c.modality_tokens = 5000, True
    ranges = get_token_type_ranges(c)
    assert list(ranges) == ["text", "dsu", "modality", "special_text"]
    labels = torch.tensor([[0, 127_999, 128_000, 132_999, 130_000, 133_000, 133_257, -100]])
    cols = torch.tensor([0, 127_999, 128_000, 132_999, 130_000, 133_000, 133_257, 5])
    logits = torch.zeros(1, 8, c.vocab_size)
    logits[0, torch.arange(8), cols] = 1.0                     # every label on top of its row ...
    logits[0, 2, 7] = 2.0                                      # ... but the first dsu label: one column above it
    m = LabelMetrics(ranges, 5, torch.device("cpu"))
    m.add_logits(logits, labels, -100)
    r = m.result()
    assert [r[f"dev_n_labels.{t}"] for t in ("text", "dsu", "modality", "special_text", "all")] == [2, 3, 1, 1, 7]
    assert r["dev_acc.text"] == 1.0 and r["dev_acc.dsu"] == pytest.approx(2 / 3) and r["dev_acc_top5.dsu"] == 1.0 and r["dev_acc.all"] == pytest.approx(6 / 7)
    assert r["dev_loss.dsu"] > r["dev_loss.text"]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world_size, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world_size))
    for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    try:
        mine = _batches()[rank::world_size]                    # rank 0: batches 0 and 2, rank 1: 1 and 3
        torch.save(_run(_Stub(_table()), mine), os.path.join(out_dir, f"m{rank}.pt"))
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_report_the_metrics_of_the_union_of_their_shards(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "m0.pt", weights_only=False)
    r1 = torch.load(tmp_path / "m1.pt", weights_only=False)
    whole = _run(_Stub(_table()), _batches())
    assert r0 == r1
    assert set(r0) == set(whole)
    for k, v in whole.items():   # the same fp32 values in fp64 sums of another order
        assert r0[k] == (v if k.startswith("dev_n_labels") else pytest.approx(v, rel=1e-12)), k
    alone = _run(_Stub(_table()), _batches()[0::2])
    assert alone["dev_n_labels.all"] < r0["dev_n_labels.all"]   # (the shards differ: the sum was really taken)


def test_config_defaults_leave_the_metrics_off():
    from ssi.config import compose
    cfg = compose(os.path.join(PKG, "conf"), "sft", ["data=sft/mls-hubert_large_ll60k-layer_22"])
    assert cfg.eval_token_metrics is False and cfg.eval_topk == 5
    cpt = compose(os.path.join(PKG, "conf"), "cpt", ["data=cpt/mls-mimi-srvq_0", "eval_token_metrics=true", "eval_topk=10"])
    assert cpt.eval_token_metrics is True and cpt.eval_topk == 10


def test_trainer_merges_the_keys_into_the_record_of_an_evaluating_step():
    """``Trainer._evaluate`` / ``_log_metrics`` with mock components (as tests/test_host_logic.py drives the state machine): off -> the record
    has ``dev_loss`` alone; on -> the per-type keys of the same pass beside it, and the same ``dev_loss``."""
    from unittest.mock import MagicMock
    from ssi.config import OmegaConf
    from ssi.trainer import Trainer, TrainingGeometry

    def record(**extra):
        cfg = OmegaConf.create({"gradient_accumulation_steps": 1, "clip_grad_norm": None, "eval_steps": 1, "log_interval": 1, "save_steps": 1000,
                                "eval_join_batches": 16, **extra})
        t = Trainer(cfg)
        t.world_size, t.rank, t.device = 1, 0, torch.device("cpu")
        t.model, t.loss_fn, t.data_dev = _Stub(_table()), _Loss(), _batches()
        t.optimizer = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=0.5)
        t.wandb_logger, t.tokenizer = MagicMock(), MagicMock()
        t.tokenizer.pad_id = 15
        t.token_type_ranges = RANGES
        t.geometry = TrainingGeometry(2, 100, 100, 100, 1, 1, 1)
        t.global_step, t.num_tokens_step, t.t_step_start = 1, 10, 0.0
        t._log_metrics(0, 1, 1.25)
        return t.wandb_logger.log_dict.call_args[0][0]

    off, on = record(), record(eval_token_metrics=True, eval_topk=3)
    assert "dev_loss" in off and not [k for k in off if k.startswith(("dev_loss.", "dev_acc", "dev_n_labels"))]
    assert on["dev_loss"] == off["dev_loss"]
    want = _by_definition(_table(), _batches(), RANGES, 3)
    assert {k: on[k] for k in want} == {k: (v if k.startswith("dev_n_labels") else pytest.approx(v, rel=REL)) for k, v in want.items()}
    assert set(on) - set(off) == set(want)
