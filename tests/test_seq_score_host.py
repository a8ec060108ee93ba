"""CPU: ``ssi.score`` on its plain-torch route (a model without ``fused_loss``): the packed layout ``score_sequences`` builds, every sequence's
score against the same sequence run alone through the seeded tiny oracle model, ``pair_accuracy``, the JSONL round trip of ``score_file``, the
trainer's ``eval_pairs`` and the ABI number.  The GPU route (``ssi_seq_score_reduce``) is held to the same arithmetic in
tests/test_seq_score_gpu.py."""
import json
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import PKG, ROOT
from test_label_metrics import _Loss, _Stub, _table

REL = 1e-5   # the project's fp32 bound (tests/test_model_gpu.py): packed against alone differ by the shapes of the attention's reductions


# ---- layout ---------------------------------------------------------------------------------------------------------------------------------
LENGTHS = [5, 2048, 1, 700, 700, 649, 2]
SCORE_FROM = [1, 1, 1, 300, 1, 649, 5]       # a long context, one that covers the whole sequence, one beyond its end


def _layout(lengths=LENGTHS, score_from=SCORE_FROM, row_len=2048, rows_per_batch=2):
    from ssi.score import pack_for_scoring, scoring_batches
    seqs = [torch.arange(n) + 1000 * (i + 1) for i, n in enumerate(lengths)]
    rows = pack_for_scoring(lengths, row_len)
    return seqs, rows, list(scoring_batches(seqs, score_from, rows, row_len, rows_per_batch, pad_id=7, token_logprobs=True))


def test_first_fit_decreasing_places_every_sequence_once():
    from ssi.score import pack_for_scoring
    rows = pack_for_scoring(LENGTHS, 2048)
    # by falling length, ties by index: 2048 fills a row; 700 + 700 + 649 = 2049 does not fit, so 649 opens a third; 5, 2, 1 go to the second
    assert rows == [[1], [3, 4, 0, 6, 2], [5]]
    assert sorted(i for r in rows for i in r) == list(range(len(LENGTHS)))
    assert pack_for_scoring(LENGTHS, 2048) == rows
    assert pack_for_scoring([], 8) == []
    assert pack_for_scoring([3, 3, 2, 2, 2], 4) == [[0], [1], [2, 3], [4]]


def test_a_sequence_longer_than_the_row_raises_and_names_its_index():
    from ssi.score import score_sequences
    seqs = [list(range(n)) for n in LENGTHS] + [list(range(2049))]
    with pytest.raises(ValueError, match=r"sequence 7 has 2049 tokens"):
        score_sequences(None, seqs, pad_id=0, device="cpu", row_len=2048)
    with pytest.raises(ValueError, match=r"score_from\[1\]"):
        score_sequences(None, [[1, 2], [3, 4]], score_from=[1, 0], pad_id=0, device="cpu")


def test_tokens_positions_and_labels_of_the_packed_rows():
    seqs, rows, batches = _layout()
    assert [b["tokens"].shape for b in batches] == [(2, 2048), (1, 2048)]
    seen = []
    flat_rows = [(b, r) for b in batches for r in range(b["tokens"].shape[0])]
    assert len(flat_rows) == len(rows)
    for (b, r), members in zip(flat_rows, rows):
        at = 0
        want_labels = torch.full((2048,), -100)
        for i in members:
            n, sf = LENGTHS[i], SCORE_FROM[i]
            assert torch.equal(b["tokens"][r, at:at + n], seqs[i])
            assert torch.equal(b["input_pos"][r, at:at + n], torch.arange(n))           # restarts with every document
            want_labels[at + sf:at + n] = seqs[i][sf:]
            k = b["seq_index"].index(i)
            row, lo, hi = b["seq_spans"][k].tolist()
            assert row == r and hi - lo == max(n - sf, 0)
            if n > sf:                                                                 # shifted positions: the label of p sits at p - 1
                assert (lo, hi) == (at + sf - 1, at + n - 1)
            seen.append(i)
            at += n
        assert (b["tokens"][r, at:] == 7).all()                                         # the tail: pad_id, a document of its own, ignored
        assert torch.equal(b["input_pos"][r, at:], torch.arange(2048 - at))
        assert torch.equal(b["labels"][r], want_labels)                                 # -100 EXACTLY on context, first tokens and tail
    assert sorted(seen) == list(range(len(LENGTHS)))
    # after compute_loss's shift no position predicts across a document boundary: the label at a document's last position is ignored
    for b in batches:
        shifted = torch.hstack((b["labels"][:, 1:], torch.full_like(b["labels"][:, -1:], -100)))
        last = (b["input_pos"][:, 1:] == 0).nonzero()                                   # (row, p): p + 1 opens a document
        assert (shifted[last[:, 0], last[:, 1]] == -100).all()
        for (row, lo, hi) in b["seq_spans"].tolist():
            assert (shifted[row, lo:hi] != -100).all()
        assert int((shifted != -100).sum()) == sum(hi - lo for _, lo, hi in b["seq_spans"].tolist()) == b["tok_pos"].shape[0]
    again = _layout()[2]
    for a, b in zip(batches, again):
        assert a.keys() == b.keys() and a["seq_index"] == b["seq_index"]
        assert all(torch.equal(a[k], b[k]) for k in a if torch.is_tensor(a[k]))


# ---- values ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle():
    from oracle import hf_crosscheck as hx
    params = hx.CASES["tiny"][0]
    return hx.oracle_model(params, hx.seeded_state_dict(params, 41), chunks=0), params["vocab_size"]


@pytest.fixture(scope="module")
def sequences(oracle):
    g = torch.Generator().manual_seed(9)
    return [torch.randint(0, oracle[1], (n,), generator=g) for n in (5, 64, 1, 20, 20, 23, 2, 40)]


@pytest.fixture(scope="module")
def alone(oracle, sequences):
    """Per sequence the fp32 log-probabilities of its tokens 1.., from the sequence run as the only document of a batch.  Computed once."""
    model, out = oracle[0], []
    with torch.no_grad():
        for s in sequences:
            logits = model(s[None])[0].float()
            out.append(-F.cross_entropy(logits[:-1], s[1:], reduction="none"))
    return out


def _score(oracle, seqs, **kw):
    from ssi.score import score_sequences
    return score_sequences(oracle[0], seqs, pad_id=3, device="cpu", row_len=64, rows_per_batch=2, topk=3, loss_fn=_Loss(), **kw)


def test_every_sequence_scores_as_it_does_alone(oracle, sequences, alone):
    got = _score(oracle, sequences, token_logprobs=True)
    assert len(got) == len(sequences) and got.logprob.dtype == torch.float64
    for i, (s, ref) in enumerate(zip(sequences, alone)):
        assert int(got.n_tokens[i]) == s.numel() - 1
        assert float(got.logprob[i]) == pytest.approx(float(ref.double().sum()), rel=REL), i
        assert 0 <= int(got.n_top1[i]) <= int(got.n_topk[i]) <= int(got.n_tokens[i])
        assert got.token_logprobs[i].dtype == torch.float32 and got.token_logprobs[i].shape == ref.shape
        torch.testing.assert_close(got.token_logprobs[i], ref, rtol=1e-4, atol=1e-5)
        assert float(got.token_logprobs[i].double().sum()) == pytest.approx(float(got.logprob[i]), rel=1e-6)
        if s.numel() > 1:
            assert float(got.mean_logprob[i]) == pytest.approx(float(got.logprob[i]) / (s.numel() - 1), rel=1e-12)
    assert math.isnan(float(got.mean_logprob[2])) and float(got.logprob[2]) == 0.0      # one token: nothing counts
    with torch.no_grad():                                                               # top-1 by definition on one sequence
        logits = oracle[0](sequences[1][None])[0].float()
    assert int(got.n_top1[1]) == int((logits[:-1].argmax(1) == sequences[1][1:]).sum())
    assert oracle[0].training                                                           # the mode it came in is restored


def test_permuting_the_input_permutes_the_output(oracle, sequences):
    base = _score(oracle, sequences)
    perm = [3, 7, 0, 5, 1, 6, 2, 4]
    got = _score(oracle, [sequences[j] for j in perm])
    for k, j in enumerate(perm):
        # (two sequences of one length swap places in their row when their input order swaps: the same values to rounding)
        assert float(got.logprob[k]) == pytest.approx(float(base.logprob[j]), rel=REL)
        assert int(got.n_tokens[k]) == int(base.n_tokens[j]) and int(got.n_topk[k]) == int(base.n_topk[j])


def test_score_from_removes_exactly_the_context_terms(oracle, sequences, alone):
    score_from = [1, 30, 1, 20, 7, 1, 9, 39]
    got = _score(oracle, sequences, score_from=score_from, token_logprobs=True)
    for i, (s, ref, sf) in enumerate(zip(sequences, alone, score_from)):
        assert int(got.n_tokens[i]) == max(s.numel() - sf, 0)
        assert float(got.logprob[i]) == pytest.approx(float(ref[sf - 1:].double().sum()), rel=REL), i
        assert got.token_logprobs[i].numel() == max(s.numel() - sf, 0)


# ---- pair accuracy --------------------------------------------------------------------------------------------------------------------------
def _scores(logprob, n_tokens):
    from ssi.score import SequenceScores
    lp, n = torch.tensor(logprob, dtype=torch.float64), torch.tensor(n_tokens)
    return SequenceScores(logprob=lp, n_tokens=n, n_top1=n * 0, n_topk=n * 0, mean_logprob=lp / n, topk=5)


def test_pair_accuracy_on_a_hand_made_table():
    from ssi.score import pair_accuracy
    #            0      1      2      3      4      5
    s = _scores([-10.0, -12.0, -8.0, -8.0, -30.0, -20.0], [5, 4, 4, 4, 10, 5])
    # sum:  (0,1) -10 > -12 win | (2,3) tie | (4,5) -30 < -20 loss          -> (1 + 0.5 + 0) / 3
    # mean: (0,1) -2 > -3 win   | (2,3) tie | (4,5) -3 > -4 win             -> (1 + 0.5 + 1) / 3
    assert pair_accuracy(s, [0, 2, 4], [1, 3, 5]) == (pytest.approx(0.5), 3)
    assert pair_accuracy(s, [0, 2, 4], [1, 3, 5], normalize="mean") == (pytest.approx(2.5 / 3), 3)
    assert pair_accuracy(s, [2], [3], "sum") == (0.5, 1)
    acc, n = pair_accuracy(s, [], [])
    assert math.isnan(acc) and n == 0
    with pytest.raises(ValueError):
        pair_accuracy(s, [0], [1], normalize="max")
    with pytest.raises(ValueError):
        pair_accuracy(s, [0, 1], [1])


# ---- score_file and the trainer -------------------------------------------------------------------------------------------------------------
ITEMS = [
    {"id": "a+", "tokens": [1, 4, 2, 9, 3], "pair": "a", "positive": True},
    {"id": "a-", "tokens": [1, 4, 2, 9, 8, 8, 0], "pair": "a"},
    {"id": "b+", "prompt_tokens": [5, 6, 7], "tokens": [2, 2], "pair": "b", "positive": True},
    {"id": "b-", "prompt_tokens": [5, 6, 7], "tokens": [10, 11], "pair": "b", "positive": False},
    {"id": "solo", "tokens": [3]},
]


def _stub_logprob(table, context, body):
    seq = torch.tensor(context + body)
    lp = torch.log_softmax(table[seq[:-1]].double(), dim=1).gather(1, seq[1:, None])[:, 0]
    return float(lp[max(len(context), 1) - 1:].sum()), len(seq) - max(len(context), 1)


def _write_items(path):
    with open(path, "w") as f:
        for item in ITEMS:
            f.write(json.dumps(item) + "\n")


def _pairs_by_definition(table):
    lp = {it["id"]: _stub_logprob(table, it.get("prompt_tokens", []), it["tokens"]) for it in ITEMS}
    def acc(value):
        wins = [(value(*lp[p]) > value(*lp[q])) + 0.5 * (value(*lp[p]) == value(*lp[q])) for p, q in (("a+", "a-"), ("b+", "b-"))]
        return sum(wins) / 2
    return lp, acc(lambda s, n: s), acc(lambda s, n: s / n)


def test_score_file_round_trip(tmp_path):
    from unittest.mock import MagicMock
    from ssi.score import score_file
    table = _table()
    _write_items(tmp_path / "in.jsonl")
    tok = MagicMock()
    tok.pad_id = 15
    summary = score_file(_Stub(table), tok, str(tmp_path / "in.jsonl"), str(tmp_path / "out.jsonl"), device="cpu", row_len=16, rows_per_batch=1,
                         loss_fn=_Loss())
    lines = [json.loads(x) for x in open(tmp_path / "out.jsonl")]
    assert [x["id"] for x in lines] == [it["id"] for it in ITEMS]
    lp, acc_sum, acc_mean = _pairs_by_definition(table)
    for x in lines:
        want, n = lp[x["id"]]
        assert set(x) == {"id", "logprob", "mean_logprob", "n_tokens", "n_top1"} and x["n_tokens"] == n
        assert x["logprob"] == pytest.approx(want, rel=1e-6)
        assert x["mean_logprob"] == (pytest.approx(want / n, rel=1e-6) if n else None)
    assert lines[2]["n_tokens"] == 2 and lines[4]["n_tokens"] == 0                       # the prompt is context; one token scores nothing
    assert summary == {"items": 5, "tokens": 4 + 6 + 2 + 2, "pair_acc": acc_sum, "pair_acc_mean": acc_mean, "pair_n": 2}
    tok.encode.assert_not_called()
    # text goes through the tokenizer: BOS and no EOS; after a prompt the prompt carries the BOS
    tok.encode.side_effect = lambda text, add_bos, add_eos: ([1] if add_bos else []) + [ord(c) % 12 for c in text] + ([2] if add_eos else [])
    with open(tmp_path / "text.jsonl", "w") as f:
        f.write(json.dumps({"id": 0, "text": "abc"}) + "\n" + json.dumps({"id": 1, "prompt": "xy", "text": "abc"}) + "\n")
    s2 = score_file(_Stub(table), tok, str(tmp_path / "text.jsonl"), None, device="cpu", row_len=16, loss_fn=_Loss())
    assert s2 == {"items": 2, "tokens": 3 + 3}
    with open(tmp_path / "bad.jsonl", "w") as f:
        f.write(json.dumps({"id": 0, "text": "abc", "tokens": [1]}) + "\n")
    with pytest.raises(ValueError, match="exactly one"):
        score_file(_Stub(table), tok, str(tmp_path / "bad.jsonl"), None, device="cpu", loss_fn=_Loss())


def test_config_default_leaves_the_pairs_off():
    from ssi.config import compose
    cfg = compose(os.path.join(PKG, "conf"), "sft", ["data=sft/mls-hubert_large_ll60k-layer_22"])
    assert cfg.eval_pairs is None
    cpt = compose(os.path.join(PKG, "conf"), "cpt", ["data=cpt/mls-mimi-srvq_0", "eval_pairs=dev_pairs.jsonl"])
    assert cpt.eval_pairs == "dev_pairs.jsonl"
    score = compose(os.path.join(PKG, "conf"), "score", ["speech.n_dsus=5000", "score.input=a.jsonl", "score.output=b.jsonl"])
    assert (score.score.row_len, score.score.rows_per_batch, score.score.topk) == (2048, 8, 5) and score.score.input == "a.jsonl"


def test_trainer_merges_the_pair_keys_into_the_record_of_an_evaluating_step(tmp_path):
    from unittest.mock import MagicMock
    from ssi.config import OmegaConf
    from ssi.trainer import Trainer, TrainingGeometry
    from test_label_metrics import RANGES, _batches
    _write_items(tmp_path / "pairs.jsonl")

    def record(**extra):
        cfg = OmegaConf.create({"gradient_accumulation_steps": 1, "clip_grad_norm": None, "eval_steps": 1, "log_interval": 1, "save_steps": 1000,
                                "eval_join_batches": 16, "tokenizer": {"max_seq_len": 32}, **extra})
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

    off, on = record(), record(eval_pairs=str(tmp_path / "pairs.jsonl"))
    also = record(eval_pairs=str(tmp_path / "pairs.jsonl"), eval_token_metrics=True, eval_topk=3)
    _, acc_sum, acc_mean = _pairs_by_definition(_table())
    assert not [k for k in off if k.startswith("dev_pair")]
    assert set(on) - set(off) == {"dev_pair_acc", "dev_pair_acc_mean", "dev_pair_n"}
    assert (on["dev_pair_acc"], on["dev_pair_acc_mean"], on["dev_pair_n"]) == (acc_sum, acc_mean, 2)
    assert on["dev_loss"] == off["dev_loss"] == also["dev_loss"]
    assert {k: also[k] for k in on if k.startswith("dev_pair")} == {k: on[k] for k in on if k.startswith("dev_pair")}
    assert "dev_n_labels.all" in also


def test_header_and_binding_agree_on_abi_13_and_the_prototype():
    from ssi import _lib
    text = open(os.path.join(ROOT, "include", "ssi_hip.h")).read()
    assert _lib.ABI_VERSION >= 13 and re.search(r"#define SSI_ABI_VERSION (\d+)", text).group(1) == str(_lib.ABI_VERSION)
    proto = re.search(r"int ssi_seq_score_reduce\(([^)]*)\);", text).group(1)
    assert len(proto.split(",")) == len(_lib.PROTOTYPES["ssi_seq_score_reduce"][1]) == 9
