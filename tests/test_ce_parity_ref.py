"""The cross-entropy parity checker (tests/ce_parity.py) held against itself on the CPU: the fp32 restatements of the two kernel bodies meet
every derived bound in every mode, at every table shape and input family; each planted defect of the restatement misses the bound it is aimed
at; and the gradient tolerance of the older files accepts a gradient row whose non-label columns are all 0, which the derived bound never does."""
import pytest
import torch

import ce_parity as C

ROWS = 4                                         # one row per input family
SELF_MODES = [C.MODES[i] for i in (0, 2, 4, 5, 6, 7)]   # every entry, z of the sign-flipping size, both teachers, row_kl_weight given and not
_WORST: dict[str, float] = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam in sorted(_WORST):
        print(f"\nce-parity restatement worst error/bound  {fam:<22s} {_WORST[fam]:.4f}", end="")
    print()


def _labels(vocab, ld):
    edges = C.label_edges(vocab, ld)
    return torch.tensor([edges[-1], vocab - 1, 0, edges[len(edges) // 2]])   # all valid: every family's row has a gradient


def _case(shape, m, weighted, families=C.FAMILIES, seed=None):
    vocab, ld, dtype, form, _ = shape
    seed = vocab if seed is None else seed
    x = C.make_logits(ROWS, vocab, ld, dtype, seed, families=families)
    labels = _labels(vocab, ld)
    w = torch.tensor([0.37, 1.0, 2.9, 1.7]) if weighted else None
    kw = dict(w=w)
    if m["kind"] == "kl":
        t = C.make_teacher(x, vocab, m["teacher"], seed)
        kw.update(teacher=t, tlse=C.restate_teacher_lse(form, t, labels, vocab), k=torch.tensor([1.5, 0.0, 0.7, 2.0]) if m["kw"] else None)
    return x, labels, kw


def _judge(got, exp, vocab):
    """{output: (worst err / bound, index, misses)}; the rank compares exactly."""
    res = {}
    for name, (ref, bound) in exp.items():
        if name == "row_rank":
            bad = int((got[name] != ref).sum())
            res[name] = (float("inf") if bad else 0.0, (0,), bad)
        elif name == "grad":
            res[name] = C.ratio(got["grad"][:, :vocab].float(), ref, bound)
        else:
            res[name] = C.ratio(got[name], ref, bound)
    return res


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_restatements_meet_every_bound(shape):
    vocab, ld, dtype, form, _ = shape
    base = None
    for i, m in enumerate(SELF_MODES):
        x, labels, kw = _case(shape, m, weighted=i % 2 == 1)
        base = base or C.Base(x, vocab)
        got = C.restate(form, x, labels, vocab, m, **kw)
        res = _judge(got, C.expected(base, labels, m, form, **kw), vocab)
        for name, (worst, idx, misses) in res.items():
            fam = f"{form} {m['kind']} {name}"
            _WORST[fam] = max(_WORST.get(fam, 0.0), worst)
            assert misses == 0 and worst < 1.0, f"{C.mode_id(m)} {name}: {misses} elements miss, worst err / bound {worst:.3f} at {idx}"
        if "grad" in got:
            assert (got["grad"][:, vocab:].float() == 0).all(), "pad columns"
    print(f"{C.shape_id(shape)}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(_WORST.items()) if k.startswith(form)))


def test_rows_without_a_valid_label_are_zero_with_rank_minus_one():
    vocab, ld = 515, 520
    labels = torch.tensor([C.IGNORE, vocab, -7, 3])
    for dtype, form in ((C.BF16, "row"), (C.F32, "generic")):
        x = C.make_logits(ROWS, vocab, ld, dtype, 1)
        for m in (C.MODES[4], C.MODES[5]):
            got = C.restate(form, x, labels, vocab, m)
            exp = C.expected(C.Base(x, vocab), labels, m, form)
            for name, (worst, _, misses) in _judge(got, exp, vocab).items():
                assert misses == 0, name
            for name, v in got.items():
                if name == "row_rank":
                    assert v[:3].tolist() == [-1, -1, -1]
                else:
                    assert (v[:3].float() == 0).all(), name


def _mutant(shape, m, mutant, weighted=False, families=C.FAMILIES):
    vocab = shape[0]
    x, labels, kw = _case(shape, m, weighted, families)
    clean = _judge(C.restate_row_form(x, labels, vocab, m, **kw), C.expected(C.Base(x, vocab), labels, m, "row", **kw), vocab)
    assert all(v[2] == 0 for v in clean.values()), "the restatement itself misses"
    got = C.restate_row_form(x, labels, vocab, m, mutant=mutant, **kw)
    res = _judge(got, C.expected(C.Base(x, vocab), labels, m, "row", **kw), vocab)
    print(f"{mutant}: " + ", ".join(f"{k} misses {v[2]} worst {v[0]:.3g}" for k, v in res.items()))
    return res


PLAIN, SMOOTH, METRICS, KL = C.MODES[0], C.MODES[3], C.MODES[5], C.MODES[7]
S = {C.shape_id(s): s for s in C.SHAPES}


def test_mutant_two_neighbouring_chunks_swapped():
    assert _mutant(S["16384x16384-bf16-row2"], PLAIN, "swap_chunks")["grad"][2] > 0


def test_mutant_a_pad_column_in_the_exp_sum():
    res = _mutant(S["515x520-bf16-row1"], PLAIN, "pad_in_sum", families=("randn",))
    assert res["row_lse"][2] > 0 and res["row_loss"][2] > 0


def test_mutant_the_row_weight_dropped():
    res = _mutant(S["8193x8200-bf16-row2"], PLAIN, "drop_weight", weighted=True)
    assert res["grad"][2] > 0 and res["row_loss"][2] > 0


def test_mutant_the_uniform_part_dropped():
    assert _mutant(S["8193x8200-bf16-row2"], SMOOTH, "drop_wu")["grad"][2] > 0


def test_mutant_the_teacher_chunk_of_an_earlier_slot():
    res = _mutant(S["32768x32768-bf16-row4"], KL, "teacher_early", weighted=True)
    assert res["grad"][2] > 0 and res["row_kl"][2] > 0


def test_mutant_the_gradient_rounded_to_bf16_twice():
    assert _mutant(S["8192x8192-bf16-row1"], SMOOTH, "double_round")["grad"][2] > 0


def test_mutant_the_rank_with_the_wrong_tie_rule():
    assert _mutant(S["8193x8200-bf16-row2"], METRICS, "rank_le", families=("ties",))["row_rank"][2] > 0


def test_mutant_row_u_summed_over_ld():
    assert _mutant(S["515x520-bf16-row1"], SMOOTH, "u_over_ld")["row_u"][2] > 0


def test_the_old_tolerance_hides_a_zeroed_gradient_row_and_the_derived_bound_does_not():
    """At the step's shape the gradient with every non-label column zeroed passes the older files' atol 4e-3 + rtol 1e-2 |ref| on more than
    99.9 % of the non-label elements, and the derived bound on none."""
    shape = S["133258x133376-bf16-row17"]
    vocab = shape[0]
    x, labels, kw = _case(shape, PLAIN, False, families=("randn",))
    ref, bound = C.expected(C.Base(x, vocab), labels, PLAIN, "row")["grad"]
    got = C.restate_row_form(x, labels, vocab, PLAIN, mutant="zero_nonlabel")["grad"][:, :vocab].float()
    nonlabel = torch.ones_like(ref, dtype=torch.bool)
    nonlabel[torch.arange(ROWS), labels] = False
    old = float(C.old_gradient_passes(got, ref, torch.ones(ROWS, dtype=torch.float64))[nonlabel].double().mean())
    new = int(((got.double() - ref).abs() <= bound)[nonlabel].sum())
    print(f"zeroed non-label columns at {C.shape_id(shape)}: the old tolerance passes {100 * old:.3f} % of them, "
          f"the derived bound {new} of {int(nonlabel.sum())}")
    assert old > 0.999 and new == 0
