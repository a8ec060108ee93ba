"""CPU: the checker of ``ssi_attn_decode`` (``decode_ref.py``) checks itself — the recorded bound constant is 8 x what the fp32
restatement is away from fp64, the restatement stays within a quarter of the bound on fresh inputs, and every deliberate mistake a decode
kernel is likely to make exceeds the bound on the test inputs."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_ref as dr  # noqa: E402

DTYPES = (torch.bfloat16, torch.float32)


def test_the_recorded_constants_are_eight_times_the_measurement():
    worst, worst_lse = 0.0, 0.0
    for dt in DTYPES:
        w, wl = dr.measure_c(dr.standard_problems(dt))
        worst, worst_lse = max(worst, w), max(worst_lse, wl)
    print(f"restatement against fp64: {worst:.3e} of the largest |v|, lse {worst_lse:.3e}; recorded C = {dr.C:.3e}, C_LSE = {dr.C_LSE:.3e}")
    # (another CPU sums the fp32 products in another order: the recorded value may sit up to a quarter above 8 x what the CPU at hand measures)
    assert dr.MARGIN * worst <= dr.C <= 1.25 * dr.MARGIN * worst
    assert dr.MARGIN * worst_lse <= dr.C_LSE <= 1.25 * dr.MARGIN * worst_lse


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_the_restatement_stays_within_a_quarter_of_the_bound_on_fresh_inputs(dtype):
    """Another seed than the one C was measured on.  The unrounded restatement within a quarter of the bound; stored in bf16 it adds half a
    bf16 step of its own (2^-9 relative, half of the bound's first term) and must still pass the checker as a kernel would."""
    for p in dr.standard_problems(dtype, dr.SEED + 1):
        ref, re = dr.exact(p), dr.restate(p)
        tol = dr.tolerance(p, ref)
        live = ~ref.dead
        assert bool(((re.out.double() - ref.out).abs()[live] <= 0.25 * tol[live]).all())
        assert bool(((re.lse.double() - ref.lse).abs()[live] <= 0.25 * dr.C_LSE).all())
        assert dr.violations(dr.stored(re.out, dtype), re.lse, p, ref) == []


MISTAKES = {"kv_len one short": dict(kv_delta=-1), "kv_len one long": dict(kv_delta=1), "another row's slot": dict(slot_shift=1),
            "the next kv head": dict(head_shift=1), "no 1/sqrt(head_dim)": dict(scaled=False)}


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("mistake", sorted(MISTAKES))
def test_a_deliberate_mistake_exceeds_the_bound(mistake, dtype):
    """On every problem of the test inputs the mistaken result — exact in fp64 otherwise, rounded to the storage type — breaks the bound.
    The caches are unpoisoned, so that a wrong read finds plausible numbers, not NaN — but for the length one LONG: behind a sink or a
    near-one-hot one more ordinary key weighs e^-10 and less, which no bound on the result can see; the poison behind every row's length
    is what shows it, there and on the GPU (the unpoisoned plain case has a test of its own below).  The wrong kv head needs more than one,
    and a missing 1/sqrt(head_dim) leaves the near-one-hot of ``newest`` a one-hot: in bf16 it passes there, and only there."""
    kw = MISTAKES[mistake]
    seen = 0
    for p in dr.standard_problems(dtype, dr.SEED, kw.get("kv_delta") == 1):
        if "head_shift" in kw and p.geom.n_kv == 1:
            continue
        if "scaled" in kw and p.case == "newest" and dtype == torch.bfloat16:
            continue
        wrong = dr.exact(p, **kw)
        bad = dr.violations(dr.stored(wrong.out, dtype), None, p, dr.exact(p))
        assert any("over the bound" in b or "not finite" in b for b in bad), (mistake, p.geom, bad)
        seen += 1
    assert seen >= 4


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_length_one_long_shows_without_poison_where_the_weights_are_even(dtype):
    for i in (0, 4):                                                            # "gauss" at either geometry
        p = dr.standard_problems(dtype, dr.SEED, False)[i]
        wrong = dr.exact(p, kv_delta=1)
        assert any("over the bound" in b for b in dr.violations(dr.stored(wrong.out, dtype), None, p, dr.exact(p)))


def test_the_off_by_one_is_caught_on_the_row_it_matters_most():
    """``newest``: nearly all of the weight sits on the last live key, so a length one short changes every element of every row longer
    than one key by far more than the bound."""
    p = [q for q in dr.standard_problems(torch.bfloat16, dr.SEED, False)][2]   # (8, 2, 16), "newest"
    ref, wrong = dr.exact(p), dr.exact(p, kv_delta=-1)
    tol = dr.tolerance(p, ref)
    rows = (p.kv_len > 1).nonzero().flatten()
    over = ((wrong.out - ref.out).abs() > tol)[rows]
    assert float(over.double().mean()) > 0.9


def test_dead_rows_and_the_checker_on_them():
    p = dr.make_problem(dr.Geometry(4, 1, 64), torch.bfloat16, [5, 0, 9, 3], "gauss", 16, dead_rows=(2,))
    ref = dr.exact(p)
    assert ref.dead.tolist() == [False, True, True, False]
    good = dr.stored(ref.out, p.dtype)
    assert dr.violations(good, ref.lse, p, ref) == []
    off = good.clone()
    off[1, 0] = 1e-30
    assert any("exact zeros" in b for b in dr.violations(off, ref.lse, p, ref))
    nan = good.clone()
    nan[0, 3] = float("nan")
    assert any("not finite" in b for b in dr.violations(nan, ref.lse, p, ref))


def test_the_edges_follow_the_kernels_lane_layout():
    assert dr.chunk_edges(64, torch.bfloat16) == (8, 16, 64)
    assert dr.chunk_edges(64, torch.float32) == (4, 8, 32)
    assert dr.chunk_edges(16, torch.bfloat16) == (32, 64, 256)
    assert dr.chunk_edges(24, torch.bfloat16) == (16, 32, 128)      # 3 lanes of 16 bytes round up to 4
    assert dr.chunk_edges(128, torch.float32) == (2, 4, 16)
    assert dr.edge_lengths(64, torch.bfloat16, 300) == [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129]
