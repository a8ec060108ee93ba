"""``ssi_decode_select_pen`` and ``ssi_decode_sample_pen`` on the GPU against tests/decode_penalty_ref.py: the token, the rank and ``n_kept``
EXACTLY (every committed draw is more than 2 delta clear of its runner-up and every top-p boundary more than eps clear, asserted on the
penalised row), ``logprob`` within ``ssi_decode_select``'s derived bound on the RAW row — both dtypes, the sampler's shapes, every history
of the reference with the penalties, the draws and the masks in turn; neutral arguments bit-equal to the plain kernels; row independence;
unaligned rows; NaN and infinite rows; ids out of range; the refusals and the LDS limit."""
import pytest
import torch

import decode_penalty_ref as P
import decode_sample_ref as S
import decode_select_ref as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", (BF16, F32), ids=("bf16", "fp32"))


def _dev(t):
    return None if t is None else t.to(DEV)


def _hist(hist):
    return {k: _dev(v) for k, v in hist.tensors().items()}


def select_pen(x_dev, vocab, hist, pen, allow=None, early=None, min_new=0, outputs=True):
    from ssi import ops
    rows = x_dev.shape[0]
    tok = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    lp = torch.full((rows,), 7.0, dtype=torch.float32, device=DEV) if outputs else None
    rk = torch.full((rows,), -7, dtype=torch.int32, device=DEV) if outputs else None
    n_bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.decode_select_pen(x_dev, vocab, tok, lp, rk, repetition_penalty=pen[0], frequency_penalty=pen[1], presence_penalty=pen[2], n_bad=n_bad,
                          allow=_dev(D.pack(allow)), allow_early=_dev(D.pack(early)), min_new=min_new, **_hist(hist))
    return (tok, lp, rk), int(n_bad)


def sample_pen(x_dev, vocab, hist, pen, seqs, *, T, top_k=-1, top_p=1.0, seed, step, allow=None, early=None, min_new=0):
    from ssi import ops
    rows = x_dev.shape[0]
    tok = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    lp = torch.full((rows,), 7.0, dtype=torch.float32, device=DEV)
    nk = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    n_bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.decode_sample_pen(x_dev, vocab, tok, lp, nk, temperature=T, top_k=top_k, top_p=top_p, seed=seed, step=step,
                          sequence=S.seq_words(seqs).to(DEV), repetition_penalty=pen[0], frequency_penalty=pen[1], presence_penalty=pen[2],
                          n_bad=n_bad, allow=_dev(D.pack(allow)), allow_early=_dev(D.pack(early)), min_new=min_new, **_hist(hist))
    return (tok, lp, nk), int(n_bad)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return all(torch.equal(_bits(u), _bits(v)) for u, v in zip(a, b))


@DTYPES
@pytest.mark.parametrize("vocab,rows", P.SHAPES, ids=[f"{v}x{r}" for v, r in P.SHAPES])
def test_every_history_at_every_shape(vocab, rows, dtype):
    case, drawn, exps = P.case(vocab, rows, dtype)
    x_dev = case.x.to(DEV)
    for (kind, hist, allow, M, pen, d), dr, e in zip(case.items, drawn, exps):
        what = f"{vocab}x{rows} {kind} r, f, p = {pen} {d}"
        y = P.penalised(case.x, vocab, hist, *pen)
        got, n_bad = select_pen(x_dev, vocab, hist, pen, allow=allow)
        bad_tok, bad_rank, ratio, misses = P.judge_select(got, P.expect_select(case.base, y, M))
        print(f"{what}: select logprob err/bound {ratio:.4f}")
        assert (bad_tok, bad_rank, misses, n_bad) == (0, 0, 0, 0), f"select {what}: {bad_tok} tokens, {bad_rank} ranks, {misses} logprobs, n_bad {n_bad}"
        assert P.clear(e), what                                       # more than 2 delta and more than eps clear, on y
        got, n_bad = sample_pen(x_dev, vocab, hist, pen, case.seqs, seed=case.seed, step=case.step, allow=allow, **d)
        bad_tok, bad_kept, ratio, misses = dr.judge(got, e)
        print(f"{what}: sample logprob err/bound {ratio:.4f}, worst margin {e.worst_margin:.2f} x 2 delta, worst mass {e.worst_mass:.2f} x eps")
        assert (bad_tok, bad_kept, misses, n_bad) == (0, 0, 0, 0), f"sample {what}: {bad_tok} tokens, {bad_kept} n_kept, {misses} logprobs, n_bad {n_bad}"
    bits = torch.int16 if dtype == BF16 else torch.int32
    assert torch.equal(x_dev.cpu().view(bits), case.x.view(bits))                                 # the logits are read only


@DTYPES
def test_every_penalty_setting_alone_and_together(dtype):
    vocab, rows = 2049, 3
    case, _, _ = P.case(vocab, rows, dtype)
    x_dev = case.x.to(DEV)
    kind, hist, allow, M, _, _ = case.items[2]
    assert kind == "edges"
    moved = 0
    for pen in P.PENALTIES:
        y = P.penalised(case.x, vocab, hist, *pen)
        exp = P.expect_select(case.base, y, M)
        got, _ = select_pen(x_dev, vocab, hist, pen, allow=allow)
        assert P.judge_select(got, exp)[:2] == (0, 0) and P.judge_select(got, exp)[3] == 0, pen
        moved += int((exp[3] > case.base.expected(allow)[3]).sum())
        for d in P.DRAWS[:2]:
            dr = P.Drawn(case.base, y, case.seqs, case.seed, case.step)
            e = dr.expected(M, d["T"], d["top_k"], d["top_p"])
            if P.clear(e):                                            # (the committed items are all clear; these extra pairs are judged where they are)
                got, _ = sample_pen(x_dev, vocab, hist, pen, case.seqs, seed=case.seed, step=case.step, allow=allow, **d)
                assert dr.judge(got, e)[:2] == (0, 0) and dr.judge(got, e)[3] == 0, (pen, d)
    assert moved > 0                                                  # a penalty changed a greedy choice somewhere


@DTYPES
def test_neutral_arguments_are_the_plain_kernels_bit_for_bit(dtype):
    from ssi import ops
    for vocab, rows in ((2049, 257), (D.FLAGSHIP[0], 3), (9, 3)):
        case, _, _ = P.case(vocab, rows, dtype)
        x_dev = case.x.to(DEV)
        for i in (2, 3, 5, 6):                                        # edges, repeat300, full, shared: any history
            kind, hist, allow, M, _, d = case.items[i]
            got, _ = select_pen(x_dev, vocab, hist, (1.0, 0.0, 0.0), allow=allow)
            want = [torch.empty_like(t) for t in got]
            ops.decode_select(x_dev, vocab, *want, allow=_dev(D.pack(allow)))
            assert _same(got, want), (vocab, kind)
            for d in P.DRAWS:
                got, _ = sample_pen(x_dev, vocab, hist, (1.0, 0.0, 0.0), case.seqs, seed=case.seed, step=case.step, allow=allow, **d)
                want = [torch.empty_like(t) for t in got]
                ops.decode_sample(x_dev, vocab, *want, temperature=d["T"], top_k=d["top_k"], top_p=d["top_p"], seed=case.seed, step=case.step,
                                  sequence=S.seq_words(case.seqs).to(DEV), allow=_dev(D.pack(allow)))
                assert _same(got, want), (vocab, kind, d)


@DTYPES
def test_row_independence(dtype):
    """A row's outputs do not change with the other rows' logits or histories, nor with its place."""
    vocab, rows = 2049, 257
    case, _, _ = P.case(vocab, rows, dtype)
    kind, hist, allow, M, pen, d = case.items[2]
    first_sel, _ = select_pen(case.x.to(DEV), vocab, hist, pen, allow=allow)
    first_smp, _ = sample_pen(case.x.to(DEV), vocab, hist, pen, case.seqs, seed=case.seed, step=case.step, allow=allow, **d)
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(2)).tolist()
    moved = P.History([hist.prompts[i] for i in perm], [hist.gens[i] for i in perm], hist.ld_gen, ld_prompt=hist.ld_prompt)
    x_p, seq_p, at = case.x[perm].to(DEV), case.seqs[perm], torch.tensor(perm, device=DEV)
    got, _ = select_pen(x_p, vocab, moved, pen, allow=allow)
    assert _same([t[at] for t in first_sel], got)
    got, _ = sample_pen(x_p, vocab, moved, pen, seq_p, seed=case.seed, step=case.step, allow=allow, **d)
    assert _same([t[at] for t in first_smp], got)
    one = P.History([hist.prompts[100]], [hist.gens[100]], hist.ld_gen, ld_prompt=hist.ld_prompt)
    got, _ = select_pen(case.x[100:101].to(DEV), vocab, one, pen, allow=allow)
    assert _same([t[100:101] for t in first_sel], got)
    got, _ = sample_pen(case.x[100:101].to(DEV), vocab, one, pen, case.seqs[100:101], seed=case.seed, step=case.step, allow=allow, **d)
    assert _same([t[100:101] for t in first_smp], got)
    again, _ = sample_pen(case.x.to(DEV), vocab, hist, pen, case.seqs, seed=case.seed, step=case.step, allow=allow, **d)
    assert _same(first_smp, again)                                    # a second launch: bit for bit, whatever order the table filled in


@DTYPES
def test_ids_out_of_range_are_skipped_and_their_rows_counted(dtype):
    vocab, rows = 2049, 257
    case, _, _ = P.case(vocab, rows, dtype)
    kind, hist, allow, M, pen, d = case.items[2]
    bad_rows = [0, 3, 8, 100, 101, 256]
    bad = P.with_bad_ids(hist, vocab, bad_rows)
    assert bad.counts(vocab)[2] == len(bad_rows)
    x_dev = case.x.to(DEV)
    want, zero = select_pen(x_dev, vocab, hist, pen, allow=allow)
    got, n_bad = select_pen(x_dev, vocab, bad, pen, allow=allow)
    assert zero == 0 and n_bad == len(bad_rows) and _same(want, got)
    want, _ = sample_pen(x_dev, vocab, hist, pen, case.seqs, seed=case.seed, step=case.step, allow=allow, **d)
    got, n_bad = sample_pen(x_dev, vocab, bad, pen, case.seqs, seed=case.seed, step=case.step, allow=allow, **d)
    assert n_bad == len(bad_rows) and _same(want, got)
    lines = P.History(hist.prompts[:2], hist.gens, hist.ld_gen, prompt_row=[0, 1, -1, 2] + [1] * (rows - 4), ld_prompt=hist.ld_prompt)
    skipped = P.History([hist.prompts[0], hist.prompts[1], []], hist.gens, hist.ld_gen, prompt_row=[0, 1, 2, 2] + [1] * (rows - 4),
                        ld_prompt=hist.ld_prompt)
    got, n_bad = select_pen(x_dev, vocab, lines, pen, allow=allow)     # a prompt line outside [0, n_prompts): refused like a bad id
    want, _ = select_pen(x_dev, vocab, skipped, pen, allow=allow)
    assert n_bad == 2 and _same(want, got)


@DTYPES
def test_rows_that_are_not_16_byte_aligned_and_min_new(dtype):
    vocab, ld, rows = 515, 517, 5
    x = D.make_logits(rows, vocab, ld, dtype, seed=3)
    assert not D.vec_ok(ld, dtype)
    base = D.Base(x, vocab)
    seqs = torch.arange(rows) + 40
    for i, kind in enumerate(("edges", "congruent", "ld257")):
        allow, M = S.masks_of(("null", "alternating", "complement")[i], vocab, rows)
        hist, pen = P.make_history(kind, x, vocab, allow, seed=i), P.PENALTIES[6 + i]
        y = P.penalised(x, vocab, hist, *pen)
        got, _ = select_pen(x.to(DEV), vocab, hist, pen, allow=allow)
        assert P.judge_select(got, P.expect_select(base, y, M))[:2] == (0, 0)
        dr = P.Drawn(base, y, seqs, 9, 2)
        e = dr.expected(M, 0.7, 50, 0.9)
        assert P.clear(e)
        got, _ = sample_pen(x.to(DEV), vocab, hist, pen, seqs, T=0.7, top_k=50, top_p=0.9, seed=9, step=2, allow=allow)
        bad_tok, bad_kept, _, misses = dr.judge(got, e)
        assert (bad_tok, bad_kept, misses) == (0, 0, 0), kind
    # n_generated picks the early mask AND the length of the history: rows at 3 (early), 4, 0 (early) and 4 generated tokens, min_new 4
    x, allow, early, _, min_new = D.min_new_case(dtype)
    hist = P.History([[77]] * 4, [[5, 6, 7], [77, 77, 77, 77], [], [1, 2, 3, 4]], ld_gen=4)
    n_gen = hist.tensors()["n_generated"]
    M = D.row_masks(4, 515, allow, early, n_gen, min_new).numpy()
    y = P.penalised(x, 515, hist, 1.0, 2.0, 0.0)
    exp = P.expect_select(D.Base(x, 515), y, M)
    got, _ = select_pen(x.to(DEV), 515, hist, (1.0, 2.0, 0.0), allow=allow, early=early, min_new=min_new)
    assert P.judge_select(got, exp)[:2] == (0, 0)
    assert [int(t) == 77 for t in got[0]] == [False, False, False, True]      # early; pushed down by its four occurrences; early; free


@DTYPES
def test_nan_and_infinite_rows(dtype):
    vocab = 515
    x = D.make_logits(5, vocab, D.ld_of(vocab), F32, seed=31)
    allow = D.make_mask("block", vocab)
    x[0, :vocab] = torch.where(allow, torch.tensor(-float("inf")), x[0, :vocab])
    x[1, :vocab] = float("nan")
    x[2, :vocab] = -float("inf")
    x[3, 5:vocab:7] = float("nan")
    x[4, 3:vocab:5] = -float("inf")
    x[4, 140] = float("inf")
    x = x.to(dtype)
    first = int(torch.nonzero(allow)[0])
    hist = P.History([[first, 133, 140, 150]] * 5, [[first, first, 131, 138, 140]] * 5, ld_gen=6)
    M = D.row_masks(5, vocab, allow, None, None, 0).numpy()
    for pen in ((1.3, 0.7, 0.7), (0.8, -0.5, -0.5)):
        y = P.penalised(x, vocab, hist, *pen)
        (tok, _, _), _ = select_pen(x.to(DEV), vocab, hist, pen, allow=allow)
        want = P.expect_select(D.Base(x, vocab), y, M)[0].tolist()    # (the reference's maximum knows no NaN: rows 0, 2 and 4 hold none)
        assert [tok.tolist()[r] for r in (0, 2, 4)] == [want[r] for r in (0, 2, 4)]
        y3 = torch.from_numpy(y[3]).masked_fill(~allow | torch.from_numpy(y[3]).isnan(), -float("inf"))
        assert int(tok[3]) == int(y3.argmax())                        # the first maximum over the allowed numbers of the penalised row
        assert tok.tolist()[:3] == [first] * 3 and int(tok[4]) == 140
        assert bool(allow[tok.cpu()].all()) and not bool(torch.isnan(x[3, int(tok[3])].float()))
        for d in P.DRAWS:
            (tok, _, nk), _ = sample_pen(x.to(DEV), vocab, hist, pen, torch.arange(5), seed=77, step=3, allow=allow, **d)
            assert tok.tolist()[:3] == [first] * 3 and nk.tolist()[:3] == [1] * 3
            assert bool(allow[tok.cpu()].all()) and bool(torch.isfinite(x[3, int(tok[3])].float())) and int(tok[4]) == 140


def test_argument_errors_the_empty_launch_and_the_lds_limit():
    from ssi import _lib, ops
    lib = _lib.load()
    x = torch.zeros(2, 40, device=DEV)
    tok = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    seq = torch.zeros(2, dtype=torch.int32, device=DEV)
    n_gen = torch.zeros(2, dtype=torch.int32, device=DEV)
    plen = torch.zeros(2, dtype=torch.int32, device=DEV)
    pid = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    gid = torch.zeros(2, 4, dtype=torch.int64, device=DEV)
    base = dict(logits=x.data_ptr(), ld=40, rows=2, vocab=33, min_new=0, token=tok.data_ptr(), n_generated=n_gen.data_ptr(),
                prompt_ids=pid.data_ptr(), ld_prompt=3, prompt_len=plen.data_ptr(), n_prompts=2, gen_ids=gid.data_ptr(), ld_gen=4, r=1.2, f=0.1,
                p=0.1, T=1.0, top_p=1.0, sequence=seq.data_ptr())

    def select(**kw):
        a = dict(base, **kw)
        return lib.ssi_decode_select_pen(a["logits"], a["ld"], a["rows"], a["vocab"], None, None, a["n_generated"], a["min_new"], a["token"], None,
                                         None, a["prompt_ids"], a["ld_prompt"], a["prompt_len"], None, a["n_prompts"], a["gen_ids"], a["ld_gen"],
                                         a["r"], a["f"], a["p"], None, _lib.SSI_F32, _lib.stream_ptr())

    def sample(**kw):
        a = dict(base, **kw)
        return lib.ssi_decode_sample_pen(a["logits"], a["ld"], a["rows"], a["vocab"], None, None, a["n_generated"], a["min_new"], a["T"], -1,
                                         a["top_p"], 0, 0, a["sequence"], a["token"], None, None, a["prompt_ids"], a["ld_prompt"], a["prompt_len"],
                                         None, a["n_prompts"], a["gen_ids"], a["ld_gen"], a["r"], a["f"], a["p"], None, _lib.SSI_F32,
                                         _lib.stream_ptr())

    nan, inf = float("nan"), float("inf")
    shared = (dict(r=0.0), dict(r=-1.0), dict(r=inf), dict(r=nan), dict(f=2.5), dict(f=-2.5), dict(f=nan), dict(f=inf), dict(p=2.5), dict(p=-2.5),
              dict(p=nan), dict(n_generated=None), dict(prompt_len=None), dict(gen_ids=None), dict(prompt_ids=None), dict(ld_gen=-1),
              dict(ld_prompt=-1), dict(n_prompts=0), dict(logits=None), dict(token=None), dict(vocab=0), dict(ld=32),
              dict(vocab=2 ** 31, ld=2 ** 31), dict(min_new=-1))
    for kw in shared:
        assert select(**kw) == 1 and sample(**kw) == 1, kw           # SSI_ERR_ARG
    for kw in (dict(T=0.0), dict(T=nan), dict(top_p=0.0), dict(top_p=1.5), dict(sequence=None)):
        assert sample(**kw) == 1, kw
    assert select(rows=0) == 0 and sample(rows=0) == 0
    assert select(gen_ids=None, ld_gen=0) == 0 and select(prompt_ids=None, ld_prompt=0) == 0      # no output yet; no prompt
    torch.cuda.synchronize()
    assert select() == 0 and all(0 <= v < 33 for v in tok.tolist())
    assert sample() == 0 and all(0 <= v < 33 for v in tok.tolist())
    # the LDS limit: 4 ceil(vocab / 32) + 8 Hs <= 57344, refused one step over it and run at it
    assert ops.decode_penalty_lds_bytes(133_376, 256) == 20_768 == lib.ssi_decode_penalty_lds_bytes(133_376, 256)
    for vocab, ld_gen in ((1, 0), (33, 32), (33, 33), (2049, 257), (D.FLAGSHIP[0], 1)):
        assert ops.decode_penalty_lds_bytes(vocab, ld_gen) == lib.ssi_decode_penalty_lds_bytes(vocab, ld_gen) == P.lds_bytes(vocab, ld_gen)
    at = 32 * (_lib.DECODE_PENALTY_LDS_MAX - 8 * 64) // 4
    assert ops.decode_penalty_lds_bytes(at, 4) == _lib.DECODE_PENALTY_LDS_MAX and ops.decode_penalty_lds_bytes(at + 1, 4) == _lib.DECODE_PENALTY_LDS_MAX + 4
    big = torch.zeros(2, at + 8, device=DEV)
    big[0, at - 1], big[1, 17], gid[1, 0] = 1.0, 1.0, 17
    n_gen[1] = 1
    assert select(logits=big.data_ptr(), ld=at + 8, vocab=at + 1) == 2 and sample(logits=big.data_ptr(), ld=at + 8, vocab=at + 1) == 2   # SSI_ERR_UNSUPPORTED
    assert select(logits=big.data_ptr(), ld=at + 8, vocab=at, r=2.0, f=2.0, p=2.0) == 0
    assert tok.tolist() == [at - 1, 0]                               # row 1's only maximum was penalised: 1 / 2 - 4 against zeros
    assert sample(logits=big.data_ptr(), ld=at + 8, vocab=at) == 0
    assert select(ld_gen=2 ** 13, gen_ids=gid.data_ptr(), vocab=33) == 2                          # the table alone is over the limit
