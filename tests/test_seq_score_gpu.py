"""GPU: the per-sequence reduce (``ssi_seq_score_reduce``), ``HipLlamaDecoder.fused_loss(seq_scores=...)`` against the plain-torch arithmetic of
``SeqScores.add_logits``, no leak between the documents of a packed row, ``score_sequences`` packed against one sequence per row, the scoring
script and the trainer's ``eval_pairs``.

The small models and inputs are those of ``tests/test_ce_metrics_gpu.py``.  Counts are exact integers and compared with ``==``; the bounds on
``sum nll`` between the routes are the ones ``tests/test_ce_z_model_gpu.py`` takes from ``tests/test_model_gpu.py`` (1e-5 relative in fp32,
1e-2 in bf16)."""
import importlib.util
import json
import math
import os

import pytest
import torch

from test_ce_metrics_gpu import _model, _model_inputs, ranked_labels

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOPK = 3


# ---- the reduce alone -----------------------------------------------------------------------------------------------------------------------
def _rows(rows, seed):
    g = torch.Generator().manual_seed(seed)
    nll = (torch.rand(rows, generator=g) * 12.0).float()
    rank = torch.randint(0, 10, (rows,), generator=g).to(torch.int32)
    rank[torch.randperm(rows, generator=g)[: rows // 3]] = -1            # a third of the positions do not count
    return nll, rank


def _by_definition(nll, rank, start, end, topk):
    """[n_labels, fsum of the fp32 nll values, n(rank == 0), n(rank < topk)] of positions [start, end) clamped as the header says."""
    rows = nll.numel()
    end = min(max(end, 0), rows)
    start = min(max(start, 0), end)
    r, x = rank[start:end], nll[start:end]
    keep = r >= 0
    return [int(keep.sum()), math.fsum(x[keep].tolist()), int((r[keep] == 0).sum()), int((r[keep] < topk).sum())]


def _reduce(ops, nll_dev, rank_dev, rows, spans, topk=TOPK):
    start = torch.tensor([a for a, _ in spans], dtype=torch.int64, device=DEV)
    end = torch.tensor([b for _, b in spans], dtype=torch.int64, device=DEV)
    out = torch.full((len(spans), 4), 7.0, dtype=torch.float64, device=DEV)   # overwritten, not added to
    ops.seq_score_reduce(nll_dev, rank_dev, rows, start, end, topk, out)
    return out.cpu()


def _check(got, nll, rank, spans, topk=TOPK):
    for i, (a, b) in enumerate(spans):
        n, s, top1, topn = _by_definition(nll, rank, a, b, topk)
        assert got[i, [0, 2, 3]].tolist() == [n, top1, topn], (i, a, b)
        # an fp64 sum of n <= 2e4 non-negative fp32 terms in any order: off by at most n * 2^-53 of the sum
        assert float(got[i, 1]) == pytest.approx(s, rel=1e-11, abs=0), (i, a, b)


# lengths 107, 0, 64, 1, 65, 63 in an order that is not that of their positions; positions 107..109 lie in no sequence, the last sequence ends
# at rows and overlaps the two before it (sequences need not tile the rows); then three more: an end past rows, a start below 0, a start
# behind its end
SIX = [(0, 107), (150, 150), (110, 174), (240, 241), (174, 239), (237, 300)]
NINE = SIX + [(280, 350), (-5, 10), (200, 190)]


def test_reduce_on_short_sequences_in_partial_workgroups():
    from ssi import ops
    rows = 300
    nll, rank = _rows(rows, 3)
    nll_dev, rank_dev = nll.to(DEV), rank.to(DEV)
    assert [b - a for a, b in SIX] == [107, 0, 64, 1, 65, 63]
    six, nine = _reduce(ops, nll_dev, rank_dev, rows, SIX), _reduce(ops, nll_dev, rank_dev, rows, NINE)
    _check(six, nll, rank, SIX)
    _check(nine, nll, rank, NINE)
    assert six[1].tolist() == [0.0] * 4 and nine[8].tolist() == [0.0] * 4                 # empty sequences: four zeros
    assert nine[6, 0] == _by_definition(nll, rank, 280, 300, TOPK)[0] > 0                 # clamped to rows
    assert torch.equal(nine[:6], six)                                                     # independent of n_seq and of the wave that took it
    assert torch.equal(_reduce(ops, nll_dev, rank_dev, rows, NINE), nine)                 # bit-identical twice
    moved = _reduce(ops, nll_dev, rank_dev, rows, list(reversed(NINE)))
    assert torch.equal(moved, nine.flip(0))                                               # ... and of where in the list it stands
    other_k = _reduce(ops, nll_dev, rank_dev, rows, SIX, topk=10)
    assert torch.equal(other_k[:, 3], other_k[:, 0]) and torch.equal(other_k[:, :3], six[:, :3])


def test_reduce_on_one_long_sequence():
    from ssi import ops
    rows = 20_100
    nll, rank = _rows(rows, 4)
    spans = [(37, 20_037), (0, 5)]
    got = _reduce(ops, nll.to(DEV), rank.to(DEV), rows, spans)
    _check(got, nll, rank, spans)
    assert got[0, 0] > 13_000


def test_reduce_argument_checks():
    from ssi import _lib
    lib = _lib.load()
    nll, rank = (t.to(DEV) for t in _rows(16, 5))
    span = torch.tensor([0, 16], dtype=torch.int64, device=DEV)
    out = torch.zeros(4, dtype=torch.float64, device=DEV)
    call = lambda n_seq, topk, rows=16: lib.ssi_seq_score_reduce(nll.data_ptr(), rank.data_ptr(), rows, span[:1].data_ptr(), span[1:].data_ptr(),  # noqa: E731
                                                                 n_seq, topk, out.data_ptr(), None)
    assert call(0, TOPK) == 0 and lib.ssi_seq_score_reduce(None, None, 0, None, None, 0, 1, None, None) == 0    # n_seq == 0: SSI_OK, no launch
    assert call(1, 0) == 1 and call(1, -1) == 1                                                                   # SSI_ERR_ARG
    assert call(1, TOPK, rows=1 << 31) == 1
    assert lib.ssi_seq_score_reduce(nll.data_ptr(), rank.data_ptr(), 16, None, span[1:].data_ptr(), 1, TOPK, out.data_ptr(), None) == 1
    assert lib.ssi_seq_score_reduce(None, rank.data_ptr(), 16, span[:1].data_ptr(), span[1:].data_ptr(), 1, TOPK, out.data_ptr(), None) == 1
    assert call(1, TOPK) == 0
    torch.cuda.synchronize()
    assert out[0] > 0


# ---- model: the routes agree ----------------------------------------------------------------------------------------------------------------
def _packed(dtype):
    """Two rows of two documents each; (tokens, input_pos, the cut, S) on the host."""
    S = 96 if dtype == torch.float32 else 128
    tokens, input_pos = _model_inputs(True, S)
    return tokens, input_pos, S // 2 - 3, S


def _spans(cut, S):
    """(row, start, end) in shifted-label positions: document 0 is predicted at [0, cut - 1), document 1 at [cut, S - 1)."""
    return [(1, cut, S - 1), (0, 0, cut - 1), (0, cut, S - 1), (1, 0, cut - 1)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_loss_with_seq_scores_against_the_torch_route(dtype):
    from ssi.eval import LabelMetrics, SeqScores
    model = _model(dtype)
    tokens_cpu, pos_cpu, cut, S = _packed(dtype)
    tokens, input_pos = tokens_cpu.to(DEV), pos_cpu.to(DEV)
    spans = _spans(cut, S)
    ranges = {"a": (0, 99), "b": (100, 399)}
    with torch.no_grad():
        logits = model(tokens, input_pos=input_pos).cpu()       # the fp32 copy of the model-dtype logits: both routes rank the same stored values
        # labels at positions 0..7 of their rows' sorted logits (top-1 and top-3 hits and misses all occur); each document's first label ignored:
        # unshifted labels[0] and labels[cut] are -100, which after the shift is position cut - 1 (nothing predicts a row's first token)
        shifted_cpu = ranked_labels(logits.reshape(2 * S, -1), logits.shape[-1]).view(2, S).clone()
        shifted_cpu[:, cut - 1] = -100
        shifted_cpu[:, -1] = -100
        shifted = shifted_cpu.to(DEV)
        plain = model.fused_loss(tokens, shifted, input_pos=input_pos)
        out = torch.full((4, 4), 7.0, dtype=torch.float64, device=DEV)
        with_scores = model.fused_loss(tokens, shifted, input_pos=input_pos, seq_scores=SeqScores(spans, TOPK, out))
        assert torch.equal(plain, with_scores)
        ref = torch.zeros(4, 4, dtype=torch.float64)
        SeqScores(spans, TOPK, ref).add_logits(logits, shifted_cpu, -100)
        got = out.cpu()
        print(got, ref, sep="\n")
        assert torch.equal(got[:, [0, 2, 3]], ref[:, [0, 2, 3]])
        assert got[:, 0].tolist() == [S - 1 - cut, cut - 1, S - 1 - cut, cut - 1]
        assert ((0 < got[:, 2]) & (got[:, 2] < got[:, 3]) & (got[:, 3] < got[:, 0])).all()
        rel = ((got[:, 1] - ref[:, 1]).abs() / ref[:, 1].abs()).max().item()
        print(f"sum nll, fused against torch, {dtype}: worst relative difference {rel:.3e}")
        assert rel <= (1e-5 if dtype == torch.float32 else 1e-2)
        # with label_metrics beside it: one cross-entropy launch, both reduces, the same loss and the same numbers
        alone = LabelMetrics(ranges, TOPK, torch.device(DEV))
        model.fused_loss(tokens, shifted, input_pos=input_pos, label_metrics=alone)
        both, out2 = LabelMetrics(ranges, TOPK, torch.device(DEV)), torch.zeros(4, 4, dtype=torch.float64, device=DEV)
        loss2 = model.fused_loss(tokens, shifted, input_pos=input_pos, label_metrics=both, seq_scores=SeqScores(spans, TOPK, out2))
        assert torch.equal(loss2, plain) and torch.equal(out2, out) and torch.equal(both.acc, alone.acc)
        assert both.acc[-1, 0] == got[:, 0].sum()
        # a device tensor of spans (how a prefetched batch carries them) is used as it is
        out3 = torch.zeros(4, 4, dtype=torch.float64, device=DEV)
        model.fused_loss(tokens, shifted, input_pos=input_pos, seq_scores=SeqScores(torch.tensor(spans, device=DEV), TOPK, out3))
        assert torch.equal(out3, out)
    model.eval()                                                # eval mode with grad enabled is forward-only too
    assert torch.equal(model.fused_loss(tokens, shifted, input_pos=input_pos, seq_scores=SeqScores(spans, TOPK, out)), plain)


def test_fused_loss_refuses_seq_scores_under_grad_and_with_z_loss():
    from ssi.eval import SeqScores
    model = _model(torch.float32)
    tokens = _model_inputs(False, 96)[0].to(DEV)
    labels = torch.roll(tokens, -1, dims=1)
    scores = SeqScores([(0, 0, 95)], TOPK, torch.zeros(1, 4, dtype=torch.float64, device=DEV))
    model.train()
    with pytest.raises(RuntimeError, match="forward-only"):
        model.fused_loss(tokens, labels, seq_scores=scores)
    with torch.no_grad(), pytest.raises(ValueError, match="z_loss_coeff and seq_scores"):
        model.fused_loss(tokens, labels, seq_scores=scores, z_loss_coeff=1e-4)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_no_leak_between_the_documents_of_a_row(dtype):
    """Replacing every token outside a document (the other document of its row and the whole other row) leaves its four numbers bit-identical:
    attention is block-causal, and the label at a document's last position is ignored."""
    from ssi.eval import SeqScores
    model = _model(dtype)
    tokens, input_pos, cut, S = _packed(dtype)
    spans = _spans(cut, S)
    docs = {(0, 0): (0, slice(0, cut)), (0, 1): (0, slice(cut, S)), (1, 0): (1, slice(0, cut)), (1, 1): (1, slice(cut, S))}
    which = [(1, 1), (0, 0), (0, 1), (1, 0)]                     # the document each entry of spans covers

    def run(tok):
        labels = tok.clone()
        labels[:, 0] = labels[:, cut] = -100                     # each document's first label
        shifted = torch.hstack((labels[:, 1:], torch.full_like(labels[:, -1:], -100))).to(DEV)
        out = torch.zeros(4, 4, dtype=torch.float64, device=DEV)
        with torch.no_grad():
            model.fused_loss(tok.to(DEV), shifted, input_pos=input_pos.to(DEV), seq_scores=SeqScores(spans, TOPK, out))
        return out.cpu()

    base = run(tokens)
    assert (base[:, 0] == torch.tensor([S - 1 - cut, cut - 1, S - 1 - cut, cut - 1])).all() and (base[:, 1] > 0).all()
    other = torch.randint(0, 515, tokens.shape, generator=torch.Generator().manual_seed(77))
    assert (other != tokens).float().mean() > 0.99
    for k, doc in enumerate(which):
        row, cols = docs[doc]
        changed = other.clone()
        changed[row, cols] = tokens[row, cols]
        got = run(changed)
        assert torch.equal(got[k], base[k]), (doc, got[k], base[k])
        assert not torch.equal(got, base)                        # (the others did move: the replacement reached the model)


# ---- score_sequences: packed against alone --------------------------------------------------------------------------------------------------
LENGTHS = [3, 120, 17, 64, 65, 31, 100]                          # 120 + 100 + 31 + 3 in one row of 256, 65 + 64 + 17 in the other


@pytest.mark.parametrize("row_len", [256, 200])                 # 200: the bf16 model right-pads its rows to 256, so row * S_padded + pos is not row * row_len + pos
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_packed_scores_equal_one_sequence_per_row(dtype, row_len):
    from ssi.score import pack_for_scoring, score_sequences
    model = _model(dtype)
    g = torch.Generator().manual_seed(31)
    seqs = [torch.randint(0, 515, (n,), generator=g) for n in LENGTHS]
    assert pack_for_scoring(LENGTHS, row_len) == ([[1, 6, 5, 0], [4, 3, 2]] if row_len == 256 else [[1, 4, 0], [6, 3, 5], [2]])
    kw = dict(pad_id=0, device=DEV, row_len=row_len, topk=TOPK)
    packed = score_sequences(model, seqs, rows_per_batch=1, token_logprobs=True, **kw)       # two batches, each into its slice of the result
    one_batch = score_sequences(model, seqs, rows_per_batch=8, **kw)
    alone = [score_sequences(model, [s], **kw) for s in seqs]
    assert packed.n_tokens.tolist() == [n - 1 for n in LENGTHS] == one_batch.n_tokens.tolist()
    worst = 0.0
    for i, a in enumerate(alone):
        assert int(a.n_tokens[0]) == LENGTHS[i] - 1
        for got in (packed, one_batch):
            rel = abs(float(got.mean_logprob[i]) - float(a.mean_logprob[0])) / abs(float(a.mean_logprob[0]))
            worst = max(worst, rel)
            if dtype == torch.float32:
                assert float(got.logprob[i]) == pytest.approx(float(a.logprob[0]), rel=1e-5), i
            else:
                assert rel <= 1e-2, (i, rel)
        assert float(packed.token_logprobs[i].double().sum()) == pytest.approx(float(packed.logprob[i]), rel=1e-6)
        assert packed.token_logprobs[i].numel() == LENGTHS[i] - 1
    print(f"packed against alone, {dtype}, row_len {row_len}: worst relative difference of mean_logprob {worst:.3e}")
    assert model.training                                        # the mode it came in is restored
    with_context = score_sequences(model, seqs, score_from=[2, 100, 1, 64, 30, 31, 5], rows_per_batch=8, **kw)
    assert with_context.n_tokens.tolist() == [1, 20, 16, 0, 35, 0, 95]
    assert math.isnan(float(with_context.mean_logprob[3])) and float(with_context.logprob[2]) == float(one_batch.logprob[2])


# ---- the script and the trainer -------------------------------------------------------------------------------------------------------------
def _write_pairs(path, vocab=300):
    g = torch.Generator().manual_seed(8)
    with open(path, "w") as f:
        for p in range(6):
            for positive in (True, False):
                n = int(torch.randint(4, 40, (1,), generator=g))
                f.write(json.dumps({"id": f"{p}{'+' if positive else '-'}", "tokens": torch.randint(0, vocab, (n,), generator=g).tolist(),
                                    "pair": p, "positive": positive}) + "\n")


def test_score_script_end_to_end(tmp_path):
    from conftest import PKG
    from ssi.config import compose
    from test_trainer_gpu import SMALL
    spec = importlib.util.spec_from_file_location("score_script", os.path.join(PKG, "scripts", "score.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    _write_pairs(tmp_path / "in.jsonl")
    cfg = compose(os.path.join(PKG, "conf"), "score", [
        "speech.n_dsus=50", "dtype=fp32", "tokenizer.max_seq_len=96", f"output_dir={tmp_path}", f"checkpointer.checkpoint_dir={tmp_path}/none",
        "checkpointer.allow_random_init=true", f"score.input={tmp_path}/in.jsonl", f"score.output={tmp_path}/out.jsonl", "score.rows_per_batch=2"])
    cfg.model_overrides = dict(SMALL)
    summary = script.main(cfg)
    lines = [json.loads(x) for x in open(tmp_path / "out.jsonl")]
    assert len(lines) == 12 == summary["items"] and summary["pair_n"] == 6
    assert summary["tokens"] == sum(x["n_tokens"] for x in lines) > 0
    assert all(x["logprob"] < 0 and x["mean_logprob"] == pytest.approx(x["logprob"] / x["n_tokens"]) for x in lines)
    assert 0.0 <= summary["pair_acc"] <= 1.0 and 0.0 <= summary["pair_acc_mean"] <= 1.0


def test_trainer_logs_pair_accuracy_and_leaves_dev_loss_alone(tmp_path):
    from test_ce_metrics_gpu import _record_of_an_evaluating_step
    _write_pairs(tmp_path / "pairs.jsonl")
    off, _ = _record_of_an_evaluating_step(tmp_path, "off")
    on, _ = _record_of_an_evaluating_step(tmp_path, "on", extra=[f"eval_pairs={tmp_path}/pairs.jsonl"])
    assert set(on) - set(off) == {"dev_pair_acc", "dev_pair_acc_mean", "dev_pair_n"}
    assert on["dev_loss"] == off["dev_loss"]                                                  # bit for bit
    assert on["dev_pair_n"] == 6 and 0.0 <= on["dev_pair_acc"] <= 1.0 and 0.0 <= on["dev_pair_acc_mean"] <= 1.0
