"""``ssi_decode_sample_rows`` and ``ssi_decode_sample_pen_rows`` on the GPU, BITWISE against the scalar entries (which
tests/test_decode_sample_gpu.py and tests/test_decode_penalty_gpu.py hold to the float64 references): row ``r`` of a ``_rows`` launch has the
token, the log-probability and ``n_kept`` of row ``r`` of the scalar entry launched with ``(temperature[r], top_k[r], top_p[r], step[r])``.
6 rows, bf16 and fp32, at the sampler's vocabularies (a vector body, a scalar tail, masked regions); uniform arrays; mixed arrays; each array
NULL in turn; the penalised form on the penalty reference's histories; rows with a refused parameter, which fail alone; the C-level refusals.
Every output starts as NaN / -7, so a row that was not written shows."""
import pytest
import torch

import decode_penalty_ref as P
import decode_sample_ref as S
import decode_select_ref as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", (BF16, F32), ids=("bf16", "fp32"))
ROWS = 6
SEED = (1 << 35) + 11
STEPS = (0, 1, 255, 2 ** 32 - 1, 1, 255)
TEMPS = (0.7, 1.0, 1.3, 1.3, 0.7, 1.0)
TOP_PS = (1.0, 0.9, 1e-6, 0.9, 1.0, 1e-6)
NAN, INF = float("nan"), float("inf")


def top_ks(vocab):
    return (-1, 1, 50, vocab + 1, vocab, 2)


def _dev(t):
    return None if t is None else t.to(DEV)


def _roll(values, by):
    return [values[(i + by) % len(values)] for i in range(len(values))]


def _outputs(rows):
    return (torch.full((rows,), -7, dtype=torch.int64, device=DEV), torch.full((rows,), NAN, dtype=torch.float32, device=DEV),
            torch.full((rows,), -7, dtype=torch.int32, device=DEV))


def _bits(out):
    tok, lp, nk = out
    return tok.tolist(), lp.view(torch.int32).tolist(), nk.tolist()


def _array(name, values):
    """What the wrapper takes for one per-row argument: the tensor of the values, or the one number (the NULL array)."""
    if not isinstance(values, (list, tuple)):
        return values
    if name == "step":
        return S.seq_words(values).to(DEV)
    return torch.tensor(values, dtype=torch.int64 if name == "top_k" else torch.float64, device=DEV)


def _per_row(v, r):
    return v[r] if isinstance(v, (list, tuple)) else v


def launch_rows(x_dev, vocab, seqs, *, T, top_k, top_p, step, hist=None, pen=None, **masks):
    """One ``_rows`` launch; ``T``, ``top_k``, ``top_p``: a list (the array) or a number (NULL, the scalar); ``step``: a list."""
    from ssi import ops
    out = _outputs(x_dev.shape[0])
    kw = dict(temperature=_array("temperature", T), top_k=_array("top_k", top_k), top_p=_array("top_p", top_p), seed=SEED,
              step=_array("step", step), sequence=S.seq_words(seqs).to(DEV), **masks)
    if hist is None:
        ops.decode_sample_rows(x_dev, vocab, *out, **kw)
        return _bits(out), 0
    n_bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.decode_sample_pen_rows(x_dev, vocab, *out, repetition_penalty=pen[0], frequency_penalty=pen[1], presence_penalty=pen[2], n_bad=n_bad,
                               **{k: _dev(v) for k, v in hist.tensors().items()}, **kw)
    return _bits(out), int(n_bad)


def launch_scalar(x_dev, vocab, seqs, *, T, top_k, top_p, step, hist=None, pen=None, **masks):
    """One launch of the scalar entry on all rows."""
    from ssi import ops
    out = _outputs(x_dev.shape[0])
    kw = dict(temperature=T, top_k=top_k, top_p=top_p, seed=SEED, step=step, sequence=S.seq_words(seqs).to(DEV), **masks)
    if hist is None:
        ops.decode_sample(x_dev, vocab, *out, **kw)
    else:
        ops.decode_sample_pen(x_dev, vocab, *out, repetition_penalty=pen[0], frequency_penalty=pen[1], presence_penalty=pen[2],
                              **{k: _dev(v) for k, v in hist.tensors().items()}, **kw)
    return _bits(out)


def each_row_its_own_scalar_launch(x_dev, vocab, seqs, *, T, top_k, top_p, step, **kw):
    """Row r of the scalar entry launched with row r's four values, for every r: what the definition says a ``_rows`` launch gives."""
    want = ([], [], [])
    for r in range(x_dev.shape[0]):
        got = launch_scalar(x_dev, vocab, seqs, T=_per_row(T, r), top_k=_per_row(top_k, r), top_p=_per_row(top_p, r), step=_per_row(step, r), **kw)
        for w, g in zip(want, got):
            w.append(g[r])
    return want


def _case(vocab, dtype):
    x = D.make_logits(ROWS, vocab, D.ld_of(vocab), dtype, seed=7000 + vocab)
    seqs = (torch.arange(ROWS, dtype=torch.int64) * 0x9E3779B1 + 9) & 0xffffffff
    kinds = [k for k in ("null", "alternating", "complement") if D.mask_exists(k, vocab) and (k == "null" or vocab > 1)]
    return x.to(DEV), seqs, [dict(allow=_dev(D.pack(D.make_mask(k, vocab)))) for k in kinds]


@DTYPES
@pytest.mark.parametrize("vocab", S.VOCABS)
def test_uniform_arrays_are_one_scalar_launch(vocab, dtype):
    x_dev, seqs, masks = _case(vocab, dtype)
    for i, m in enumerate(masks):
        T, k, p, step = TEMPS[i], top_ks(vocab)[i + 1], TOP_PS[i + 1], STEPS[i + 2]
        got, _ = launch_rows(x_dev, vocab, seqs, T=[T] * ROWS, top_k=[k] * ROWS, top_p=[p] * ROWS, step=[step] * ROWS, **m)
        assert got == launch_scalar(x_dev, vocab, seqs, T=T, top_k=k, top_p=p, step=step, **m), (vocab, i)
        assert -7 not in got[0] and -7 not in got[2]


@DTYPES
@pytest.mark.parametrize("vocab", S.VOCABS)
def test_mixed_arrays_give_every_row_its_own_scalar_launch(vocab, dtype):
    x_dev, seqs, masks = _case(vocab, dtype)
    for i, m in enumerate(masks):
        for a in range(3):                                        # the values meet in other combinations with every turn
            draw = dict(T=_roll(TEMPS, a), top_k=_roll(top_ks(vocab), 2 * a + i), top_p=_roll(TOP_PS, 3 * a), step=_roll(STEPS, a + i))
            got, _ = launch_rows(x_dev, vocab, seqs, **draw, **m)
            assert got == each_row_its_own_scalar_launch(x_dev, vocab, seqs, **draw, **m), (vocab, i, a)


@DTYPES
@pytest.mark.parametrize("vocab", (9, 257, 2049, D.FLAGSHIP[0]))
@pytest.mark.parametrize("null", ("temperature", "top_k", "top_p"))
def test_each_array_null_in_turn(null, vocab, dtype):
    x_dev, seqs, masks = _case(vocab, dtype)
    draw = dict(T=list(TEMPS), top_k=list(top_ks(vocab)), top_p=list(TOP_PS), step=list(STEPS))
    draw.update({"temperature": dict(T=1.3), "top_k": dict(top_k=50), "top_p": dict(top_p=0.9)}[null])
    for m in masks[:2]:
        got, _ = launch_rows(x_dev, vocab, seqs, **draw, **m)
        assert got == each_row_its_own_scalar_launch(x_dev, vocab, seqs, **draw, **m), (vocab, null)


@DTYPES
@pytest.mark.parametrize("vocab", (257, 2049))
@pytest.mark.parametrize("kind", ("edges", "congruent", "shared", "ld257"))
def test_the_penalised_form_on_the_penalty_histories(kind, vocab, dtype):
    x = D.make_logits(ROWS, vocab, D.ld_of(vocab), dtype, seed=7000 + vocab)
    seqs = (torch.arange(ROWS, dtype=torch.int64) * 0x9E3779B1 + 9) & 0xffffffff
    allow = D.make_mask("complement", vocab)
    hist, x_dev, m = P.make_history(kind, x, vocab, allow, seed=3), x.to(DEV), dict(allow=_dev(D.pack(allow)))
    for a, pen in enumerate((P.PENALTIES[6], P.PENALTIES[7], (1.0, 0.0, 0.0))):
        draw = dict(T=_roll(TEMPS, a), top_k=_roll(top_ks(vocab), a), top_p=_roll(TOP_PS, 2 * a), step=_roll(STEPS, a))
        got, n_bad = launch_rows(x_dev, vocab, seqs, hist=hist, pen=pen, **draw, **m)
        assert n_bad == 0 and got == each_row_its_own_scalar_launch(x_dev, vocab, seqs, hist=hist, pen=pen, **draw, **m), (kind, vocab, pen)
    got, _ = launch_rows(x_dev, vocab, seqs, hist=hist, pen=(1.0, 0.0, 0.0), **draw, **m)      # neutral penalties: the plain _rows entry
    assert got == launch_rows(x_dev, vocab, seqs, **draw, **m)[0]


@DTYPES
@pytest.mark.parametrize("penalised", (False, True), ids=("plain", "pen"))
def test_a_row_with_a_refused_parameter_fails_alone(penalised, dtype):
    vocab = 2049
    x = D.make_logits(ROWS, vocab, D.ld_of(vocab), dtype, seed=7000 + vocab)
    seqs = torch.arange(ROWS) + 70
    kw = dict(hist=P.make_history("edges", x, vocab, None, seed=4), pen=P.PENALTIES[8]) if penalised else {}
    x_dev = x.to(DEV)
    good = dict(T=list(TEMPS), top_k=[50] * ROWS, top_p=[0.9] * ROWS, step=list(STEPS))
    want, _ = launch_rows(x_dev, vocab, seqs, **good, **kw)
    refused = [("T", 0.0), ("T", NAN), ("T", INF), ("top_p", 0.0), ("top_p", 1.5), ("T", -1.0), ("top_p", NAN)]
    for shift in (0, 1):                                          # five refused rows and one good one, which moves
        bad = dict(good, T=list(TEMPS), top_p=[0.9] * ROWS)
        rows_bad = []
        for j, (name, v) in enumerate(refused[2 * shift:2 * shift + 5]):
            r = (j + shift) % ROWS
            bad[name][r] = v
            rows_bad.append(r)
        got, n_bad = launch_rows(x_dev, vocab, seqs, **bad, **kw)
        assert n_bad == 0
        for r in range(ROWS):
            row = [g[r] for g in got]
            assert row == ([-1, 0, -1] if r in rows_bad else [w[r] for w in want]), (shift, r)      # (0: the bits of logprob 0.0)
    assert len(set(range(ROWS)) - set(rows_bad)) == 1


def test_argument_errors_and_the_empty_launch():
    from ssi import _lib, ops
    lib = _lib.load()
    x = torch.zeros(2, 40, device=DEV)
    tok = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    seq, step = torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    temps, ps = torch.ones(2, dtype=torch.float64, device=DEV), torch.ones(2, dtype=torch.float64, device=DEV)
    n_gen, plen = torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    base = dict(logits=x.data_ptr(), ld=40, rows=2, vocab=33, min_new=0, token=tok.data_ptr(), T=1.0, top_p=1.0, step=step.data_ptr(), Ts=None,
                ps=None, sequence=seq.data_ptr())

    def plain(**kw):
        a = dict(base, **kw)
        return lib.ssi_decode_sample_rows(a["logits"], a["ld"], a["rows"], a["vocab"], None, None, None, a["min_new"], a["T"], -1, a["top_p"], 0,
                                          a["step"], a["Ts"], None, a["ps"], a["sequence"], a["token"], None, None, _lib.SSI_F32, _lib.stream_ptr())

    def pen(**kw):
        a = dict(base, **kw)
        return lib.ssi_decode_sample_pen_rows(a["logits"], a["ld"], a["rows"], a["vocab"], None, None, n_gen.data_ptr(), a["min_new"], a["T"], -1,
                                              a["top_p"], 0, a["step"], a["Ts"], None, a["ps"], a["sequence"], a["token"], None, None, None, 0,
                                              plen.data_ptr(), None, 2, None, 0, a.get("r", 1.2), 0.1, 0.1, None, _lib.SSI_F32, _lib.stream_ptr())

    for call in (plain, pen):
        for kw in (dict(logits=None), dict(token=None), dict(vocab=0), dict(ld=32), dict(vocab=2 ** 31, ld=2 ** 31), dict(min_new=-1), dict(T=0.0),
                   dict(T=-1.0), dict(T=INF), dict(T=NAN), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=NAN), dict(sequence=None), dict(step=None)):
            assert call(**kw) == 1, (call.__name__, kw)           # SSI_ERR_ARG
        assert call(rows=0) == 0
    assert pen(r=0.0) == 1
    torch.cuda.synchronize()
    assert tok.tolist() == [-7, -7]                               # nothing was launched, nothing written
    # with its array a scalar is not read
    assert plain(T=0.0, Ts=temps.data_ptr()) == 0 and plain(top_p=1.5, ps=ps.data_ptr()) == 0 and pen(T=NAN, Ts=temps.data_ptr()) == 0
    assert all(0 <= v < 33 for v in tok.tolist())
    out = torch.empty(2, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.HipLibraryError):                      # the wrapper: step is a tensor, arrays are one entry per row of their dtype
        ops.decode_sample_rows(x, 33, out, temperature=1.0, seed=0, step=0, sequence=seq)
    with pytest.raises(_lib.HipLibraryError):
        ops.decode_sample_rows(x, 33, out, temperature=torch.ones(2, device=DEV), seed=0, step=step, sequence=seq)
    with pytest.raises(_lib.HipLibraryError):
        ops.decode_sample_rows(x, 33, out, temperature=1.0, top_k=torch.ones(3, dtype=torch.int64, device=DEV), seed=0, step=step, sequence=seq)
