"""GPU: the forward-only cross-entropy that also ranks the label (``ssi_ce_fwd_metrics``), its per-type reduction (``ssi_ce_metrics_reduce``),
``HipLlamaDecoder.fused_loss(label_metrics=...)`` and the trainer's ``eval_token_metrics``.

The reference is torch on the CPU, applied to the very values uploaded: ``rank = #{x > x[label]} + #{c < label: x[c] == x[label]}`` (the label's
position in a stable descending sort of the row) is an exact integer and is compared with ``==``; ``row_loss`` / ``row_lse`` are compared bit for
bit with what ``ops.ce_fwd(..., write_grad=False)`` writes, because ``dev_loss`` must not move when the metrics are switched on."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS = 24
RANGES = {"a": (0, 99), "b": (100, 399), "c": (450, 514), "empty": (515, 600)}  # 400..449 lie in no range
# (vocab, ld, dtype): 515 -> the generic kernel in both dtypes; bf16 with ld = NCH x 8192 chunks -> the register-resident rows (NCH 2, 3, 16, 17);
# fp32 at a register-form shape -> the generic kernel walking many vectors per thread
SHAPES = [(515, 520, torch.float32), (515, 520, torch.bfloat16), (9000, 9216, torch.bfloat16), (9000, 9216, torch.float32),
          (20_000, 20_480, torch.bfloat16), (130_306, 130_560, torch.bfloat16), (133_258, 133_376, torch.bfloat16),
          (133_258, 133_376, torch.float32)]


def rnd(*shape, dtype=torch.float32, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


def ref_rows(logits, labels, vocab, ignore_index=-100):
    """(nll fp32 [rows], rank int32 [rows]) of CPU logits ``[rows, ld]`` by the definition; ignored / out-of-range labels: 0 and -1."""
    x = logits[:, :vocab].float()
    valid = (labels != ignore_index) & (labels >= 0) & (labels < vocab)
    lab = torch.where(valid, labels, torch.zeros_like(labels))
    xl = x.gather(1, lab[:, None])
    below = torch.arange(vocab)[None, :] < lab[:, None]
    rank = ((x > xl).sum(1) + ((x == xl) & below).sum(1)).to(torch.int32)
    nll = torch.logsumexp(x.double(), dim=1).float() - xl[:, 0]
    return torch.where(valid, nll, torch.zeros_like(nll)), torch.where(valid, rank, torch.full_like(rank, -1))


def ranked_labels(logits, vocab):
    """label[r] = the column at position r % 8 of row r's stable descending sort: the reference ranks are exactly r % 8 (random labels never
    come near the top of a row)."""
    order = torch.sort(logits[:, :vocab].float(), dim=1, descending=True, stable=True).indices
    r = torch.arange(logits.shape[0])
    return order[r, r % 8].contiguous()


def run_metrics(ops, logits, labels, vocab, w=None, with_lse=True):
    rows = logits.shape[0]
    dev = logits.to(DEV)
    keep = dev.clone()
    out = {"loss": torch.full((rows,), 7.0, device=DEV), "lse": torch.full((rows,), 7.0, device=DEV) if with_lse else None,
           "nll": torch.full((rows,), 7.0, device=DEV), "rank": torch.full((rows,), 99, dtype=torch.int32, device=DEV)}
    ops.ce_fwd_metrics(dev, labels.to(DEV), vocab, -100, out["loss"], out["lse"], out["nll"], out["rank"],
                       row_weight=None if w is None else w.to(DEV))
    assert torch.equal(dev, keep), "the logits were written"
    return out


def check_against_ce_fwd(ops, logits, labels, vocab, got, w=None):
    rows = logits.shape[0]
    loss, lse = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    ops.ce_fwd(logits.to(DEV), labels.to(DEV), vocab, -100, loss, lse, False, row_weight=None if w is None else w.to(DEV))
    assert torch.equal(got["loss"], loss), "row_loss differs from ce_fwd(write_grad=False)"
    assert torch.equal(got["lse"], lse), "row_lse differs from ce_fwd(write_grad=False)"


@pytest.mark.parametrize("vocab,ld,dtype", SHAPES)
def test_rank_and_nll_against_torch_and_loss_bits_against_ce_fwd(ops, vocab, ld, dtype):
    logits = rnd(ROWS, ld, dtype=dtype, seed=5, scale=3.0)
    labels = ranked_labels(logits, vocab)
    nll_ref, rank_ref = ref_rows(logits, labels, vocab)
    assert torch.equal(rank_ref, torch.arange(ROWS, dtype=torch.int32) % 8)   # the construction: 3 top-1 rows, 15 top-5 rows, 9 beyond
    got = run_metrics(ops, logits, labels, vocab)
    assert torch.equal(got["rank"].cpu(), rank_ref)
    torch.testing.assert_close(got["nll"].cpu(), nll_ref, rtol=1e-5, atol=2e-5)
    check_against_ce_fwd(ops, logits, labels, vocab, got)
    assert torch.equal(got["nll"], got["loss"])                     # no weights: the same subtraction
    # weighted rows (a joined dev batch): row_loss carries the weight as ce_fwd's does, row_nll and row_rank do not see it
    w = 0.97 + 0.06 * torch.rand(ROWS, generator=torch.Generator().manual_seed(6))
    got_w = run_metrics(ops, logits, labels, vocab, w=w)
    check_against_ce_fwd(ops, logits, labels, vocab, got_w, w=w)
    assert torch.equal(got_w["nll"], got["nll"]) and torch.equal(got_w["rank"], got["rank"]) and torch.equal(got_w["lse"], got["lse"])
    again = run_metrics(ops, logits, labels, vocab, w=w)
    assert all(torch.equal(again[k], got_w[k]) for k in again), "not bitwise reproducible"
    no_lse = run_metrics(ops, logits, labels, vocab, with_lse=False)  # row_lse = NULL
    assert torch.equal(no_lse["loss"], got["loss"]) and torch.equal(no_lse["rank"], got["rank"])


def test_many_rows_per_workgroup_with_ignored_stretches(ops):
    """700 rows on at most 256 workgroups: each walks several rows with the next row's loads under the current one; ignored rows singly and in
    a stretch (a workgroup then meets several in a row)."""
    rows, vocab, ld = 700, 9000, 9216
    logits = rnd(rows, ld, dtype=torch.bfloat16, seed=120, scale=4.0)
    labels = ranked_labels(logits, vocab)
    labels[::7] = -100
    labels[300:330] = -100
    nll_ref, rank_ref = ref_rows(logits, labels, vocab)
    got = run_metrics(ops, logits, labels, vocab)
    assert torch.equal(got["rank"].cpu(), rank_ref)
    torch.testing.assert_close(got["nll"].cpu(), nll_ref, rtol=1e-5, atol=2e-5)
    check_against_ce_fwd(ops, logits, labels, vocab, got)


@pytest.mark.parametrize("vocab,ld,dtype", [(515, 520, torch.float32), (515, 520, torch.bfloat16), (20_000, 20_480, torch.bfloat16),
                                            (133_258, 133_376, torch.bfloat16)])
def test_hand_made_rows(ops, vocab, ld, dtype):
    """Ties, the ends of the row, ignored and out-of-range labels, and pad columns that would win every comparison if they counted."""
    far = vocab - 3 if vocab < 8192 else 8192 + 5 * 64 * 8 + 3  # a column of another 8192-column chunk and of another wave than column 10
    rows = []

    def row(label, fill=-1.0, **at):
        x = torch.full((ld,), fill)
        for c, v in at.items():
            x[int(c[1:])] = v
        rows.append((x, label))

    row(10, c10=2.0)                                  # 0: the unique maximum                                  -> rank 0
    row(far, **{"c10": 2.0, f"c{far}": 2.0})         # 1: an equal maximum at a smaller index, far away        -> rank 1
    row(10, **{"c10": 2.0, f"c{far}": 2.0})          # 2: an equal maximum at a larger index, far away         -> rank 0
    row(0, c0=0.5, c7=1.0, c300=1.5)                  # 3: label at column 0, two columns above it               -> rank 2
    row(vocab - 1, **{f"c{vocab - 1}": 0.5, "c7": 1.0})   # 4: label at the last real column                     -> rank 1
    row(vocab - 1, **{f"c{vocab - 1}": 3.0})         # 5: ... and on top there                                  -> rank 0
    row(0)                                            # 6: all columns equal                                     -> rank == label = 0
    row(321)                                          # 7: all columns equal                                     -> 321
    row(vocab - 1)                                    # 8: all columns equal                                     -> vocab - 1
    row(-100, c3=2.0)                                 # 9: ignored                                               -> -1, nll 0
    row(vocab, c3=2.0)                                # 10: out of range above (a pad column's index)            -> -1, nll 0
    row(-5, c3=2.0)                                   # 11: out of range below                                   -> -1, nll 0
    row(9, c9=-0.0, c4=0.0, c12=0.0, fill=-2.0)       # 12: -0.0 == +0.0 as torch's sort and argmax compare them -> rank 1
    logits = torch.stack([x for x, _ in rows])
    logits[:, vocab:] = 1e4                           # pad columns [vocab, ld): must change nothing
    logits = logits.to(dtype)
    labels = torch.tensor([l for _, l in rows])
    want = torch.tensor([0, 1, 0, 2, 1, 0, 0, 321, vocab - 1, -1, -1, -1, 1], dtype=torch.int32)
    nll_ref, rank_ref = ref_rows(logits, labels, vocab)
    assert torch.equal(rank_ref, want)
    argmax_hit = logits[:, :vocab].float().argmax(1) == labels     # torch's first-occurrence rule
    assert torch.equal(argmax_hit[:9], want[:9] == 0)
    got = run_metrics(ops, logits, labels, vocab)
    assert torch.equal(got["rank"].cpu(), want)
    torch.testing.assert_close(got["nll"].cpu(), nll_ref, rtol=1e-5, atol=2e-5)
    assert (got["nll"].cpu()[9:12] == 0).all() and (got["loss"].cpu()[9:12] == 0).all()
    check_against_ce_fwd(ops, logits, labels, vocab, got)
    clean = logits.clone()
    clean[:, vocab:] = -3.0
    got_clean = run_metrics(ops, clean, labels, vocab)
    assert all(torch.equal(got_clean[k], got[k]) for k in got), "the pad columns changed a result"


def reduce_ref(nll, rank, labels, ranges, topk):
    out = torch.zeros(len(ranges) + 1, 4, dtype=torch.float64)
    ok = rank >= 0
    for j, lohi in enumerate(list(ranges.values()) + [None]):
        m = ok if lohi is None else ok & (labels >= lohi[0]) & (labels <= lohi[1])
        out[j] = torch.tensor([m.sum(), nll[m].double().sum(), (m & (rank == 0)).sum(), (m & (rank < topk)).sum()], dtype=torch.float64)
    return out


@pytest.mark.parametrize("topk", [1, 5])
@pytest.mark.parametrize("rows", [ROWS, 2500])
def test_reduce_per_range(ops, topk, rows):
    """Counts exactly; the nll sums against an fp64 sum of the kernel's own fp32 row values (both are fp64 sums of the same numbers)."""
    vocab, ld = 515, 520
    logits = rnd(rows, ld, dtype=torch.float32, seed=40, scale=3.0)
    labels = ranked_labels(logits, vocab)
    labels[3] = 420                                                 # in no range: only the `all` row sees it
    labels[7], labels[8] = -100, 600                                # ignored; out of range (though inside the range `empty`)
    got = run_metrics(ops, logits, labels, vocab)
    nll, rank = got["nll"].cpu(), got["rank"].cpu()
    rt = torch.tensor([v for lohi in RANGES.values() for v in lohi], dtype=torch.int64, device=DEV)
    out = torch.full((len(RANGES) + 1, 4), 123.0, dtype=torch.float64, device=DEV)
    ops.ce_metrics_reduce(got["nll"], got["rank"], labels.to(DEV), rt, topk, out)                     # accumulate = 0 overwrites
    want = reduce_ref(nll, rank, labels, RANGES, topk)
    o = out.cpu().clone()
    assert torch.equal(o[:, [0, 2, 3]], want[:, [0, 2, 3]])
    torch.testing.assert_close(o[:, 1], want[:, 1], rtol=1e-12, atol=0)
    in_no_range = int(((labels >= 400) & (labels <= 449)).sum())                      # row 3 at least: only the `all` row sees these
    assert o[-1, 0] == rows - 2 and o[-1, 0] - o[:-1, 0].sum() == in_no_range >= 1 and o[3, 0] == 0   # (`empty`: the out-of-range 600 does not count)
    assert 0 < o[-1, 2] < o[-1, 0] and (o[-1, 2] < o[-1, 3] if topk > 1 else o[-1, 2] == o[-1, 3])
    ops.ce_metrics_reduce(got["nll"], got["rank"], labels.to(DEV), rt, topk, out, accumulate=True)
    assert torch.equal(out.cpu(), 2 * o)                                                              # accumulate = 1 adds (x2 is exact)
    ops.ce_metrics_reduce(got["nll"], got["rank"], labels.to(DEV), rt, topk, out)
    assert torch.equal(out.cpu(), o), "not bitwise reproducible / accumulate = 0 did not overwrite"
    none = torch.empty(1, 4, dtype=torch.float64, device=DEV)                                         # no ranges at all: the `all` row alone
    ops.ce_metrics_reduce(got["nll"], got["rank"], labels.to(DEV), rt[:0], topk, none)
    assert torch.equal(none.cpu()[0], o[-1])


# ---- model ----------------------------------------------------------------------------------------------------------------------------------
def _model(dtype):
    from oracle import hf_crosscheck as hx
    from ssi.model import HipLlamaDecoder
    params = (dict(vocab_size=515, num_layers=2, num_heads=8, num_kv_heads=2, embed_dim=128, max_seq_len=256, intermediate_dim=256)
              if dtype == torch.float32 else
              dict(vocab_size=515, num_layers=2, num_heads=4, num_kv_heads=2, embed_dim=256, max_seq_len=512, intermediate_dim=512))
    model = HipLlamaDecoder(**params, dtype=dtype, device=DEV)
    model.load_state_dict(hx.seeded_state_dict(params, 52))
    model.set_num_output_chunks(0)
    return model


def _model_inputs(packed, S):
    tokens = torch.randint(0, 515, (2, S), generator=torch.Generator().manual_seed(21))
    input_pos = None
    if packed:                                         # two documents per row: positions restart at 0
        cut = S // 2 - 3
        input_pos = torch.cat([torch.arange(cut), torch.arange(S - cut)]).expand(2, S).contiguous()
    return tokens, input_pos


def _labels_from(logits):
    """Shifted labels ``[B, S]`` placed at positions 0..7 of their rows' sorted logits (a random model would never hit), with -100 runs; the
    columns are spread over the vocabulary, so every range of RANGES and the gap 400..449 occur."""
    B, S, V = logits.shape
    labels = ranked_labels(logits.reshape(B * S, V), V).view(B, S).clone()
    labels[:, -1] = -100
    labels[0, 5:19] = -100
    labels[1, :9] = -100
    return labels


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_loss_with_label_metrics(dtype, packed):
    """``fused_loss(label_metrics=acc)`` under no-grad against the torch arithmetic (``LabelMetrics.add_logits``, itself pinned on the CPU in
    tests/test_label_metrics.py) applied to the logits ``model(tokens, input_pos=...)`` returns: the head GEMM of both calls sees the same
    rows, so those logits are the bits the fused path ranks (the exact counts below would not survive otherwise)."""
    from ssi.eval import LabelMetrics
    model = _model(dtype)
    S = 96 if dtype == torch.float32 else 128
    tokens, input_pos = (None if t is None else t.to(DEV) for t in _model_inputs(packed, S))
    ranges = {k: v for k, v in RANGES.items() if k != "empty"}
    with torch.no_grad():
        logits = model(tokens, input_pos=input_pos).cpu()   # the fp32 copy of the model-dtype logits: exact
        labels_cpu = _labels_from(logits)
        labels = labels_cpu.to(DEV)
        plain = model.fused_loss(tokens, labels, input_pos=input_pos)
        acc = LabelMetrics(ranges, 5, torch.device(DEV))
        with_metrics = model.fused_loss(tokens, labels, input_pos=input_pos, label_metrics=acc)
        assert torch.equal(plain, with_metrics)
        ref = LabelMetrics(ranges, 5, torch.device("cpu"))
        ref.add_logits(logits, labels_cpu, -100)
        got, want = acc.acc.cpu(), ref.acc
        print(got, want, sep="\n")
        assert torch.equal(got[:, [0, 2, 3]], want[:, [0, 2, 3]])
        n_valid = int((labels_cpu != -100).sum())
        assert (got[:3, 0] > 0).all() and got[-1, 0] == n_valid > got[:3, 0].sum()          # three types, and labels in no range
        assert 0 < got[-1, 2] < got[-1, 3] < n_valid                                         # top-1 hits, more top-5 hits, and misses
        torch.testing.assert_close(got[:, 1], want[:, 1], rtol=1e-5, atol=0)
        model.fused_loss(tokens, labels, input_pos=input_pos, label_metrics=acc)             # a second batch ADDS to the accumulator
        assert torch.equal(acc.acc.cpu(), 2 * got)
    model.eval()                                       # eval mode with grad enabled is forward-only too
    assert torch.equal(model.fused_loss(tokens, labels, input_pos=input_pos, label_metrics=LabelMetrics(ranges, 5, torch.device(DEV))), plain)


def test_fused_loss_refuses_label_metrics_while_a_gradient_is_recorded():
    from ssi.eval import LabelMetrics
    model = _model(torch.float32)
    tokens = _model_inputs(False, 96)[0].to(DEV)
    labels = torch.roll(tokens, -1, dims=1)
    model.train()
    with pytest.raises(RuntimeError, match="forward-only"):
        model.fused_loss(tokens, labels, label_metrics=LabelMetrics(RANGES, 5, torch.device(DEV)))


# ---- trainer --------------------------------------------------------------------------------------------------------------------------------
def _record_of_an_evaluating_step(tmp_path, name, dtype="fp32", extra=()):
    from test_trainer_gpu import SMALL, _trainer
    t = _trainer(tmp_path, name, dtype=dtype, model=SMALL, overrides=[
        "max_steps=1", "eval_steps=1", "save_steps=1000", "optimizer.lr=0.0", "data.dev.dataset.n_samples=7", "data.dev.dataset.fixed_len=false", *extra])
    t.train()
    record, types = dict(t.wandb_logger.records[-1]), list(t.token_type_ranges)
    t.cleanup()
    return record, types


def test_trainer_logs_per_type_dev_metrics(tmp_path):
    off, _ = _record_of_an_evaluating_step(tmp_path, "off")
    on, types = _record_of_an_evaluating_step(tmp_path, "on", extra=["eval_token_metrics=true"])
    on0, _ = _record_of_an_evaluating_step(tmp_path, "on0", extra=["eval_token_metrics=true", "eval_join_batches=0", "eval_topk=3"])
    assert not [k for k in off if k.startswith(("dev_loss.", "dev_acc", "dev_n_labels"))]     # off: the reference's record, key for key
    assert on["dev_loss"] == off["dev_loss"]                                                  # bit for bit
    assert set(on) - set(off) == {k for k in on if k.startswith(("dev_loss.", "dev_acc", "dev_n_labels"))}
    seen = [tt for tt in types if on[f"dev_n_labels.{tt}"] > 0]
    assert len(seen) >= 2, on
    for rec, k in ((on, 5), (on0, 3)):
        for tt in types + ["all"]:
            assert rec[f"dev_n_labels.{tt}"] == int(rec[f"dev_n_labels.{tt}"]) >= 0   # (the in-memory logger stores every number as a float)
            keys = {f"dev_loss.{tt}", f"dev_acc.{tt}", f"dev_acc_top{k}.{tt}"}
            if rec[f"dev_n_labels.{tt}"]:
                assert keys <= set(rec) and 0.0 <= rec[f"dev_acc.{tt}"] <= rec[f"dev_acc_top{k}.{tt}"] <= 1.0 and rec[f"dev_loss.{tt}"] > 0
            else:
                assert not keys & set(rec)                                                    # no NaN in the record
        assert sum(rec[f"dev_n_labels.{tt}"] for tt in types) == rec["dev_n_labels.all"] > 0
    # joined (16 dev batches as one) against batch by batch: token-level values do not depend on the batching
    for tt in types + ["all"]:
        assert on[f"dev_n_labels.{tt}"] == on0[f"dev_n_labels.{tt}"]
        if on[f"dev_n_labels.{tt}"]:
            print(tt, on[f"dev_loss.{tt}"], on0[f"dev_loss.{tt}"], on[f"dev_acc.{tt}"], on0[f"dev_acc.{tt}"])
            assert on[f"dev_loss.{tt}"] == pytest.approx(on0[f"dev_loss.{tt}"], rel=1e-5)
