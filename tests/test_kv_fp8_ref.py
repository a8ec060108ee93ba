"""CPU self-test of kv_fp8_ref.py: the hand-made e4m3 encoder against the code table and against torch's own ``float8_e4m3fn`` cast, the exponent
rule at its edges, exactness of both directions, and every planted defect caught by the comparison the GPU tests make."""
import math

import pytest
import torch

import decode_ref as dr
import kv_fp8_ref as kr

DTYPES = (torch.bfloat16, torch.float32)


def test_every_finite_code_encodes_to_itself_and_the_table_is_e4m3fn():
    t = kr.e4m3_value_table()
    assert float(t[0x7E]) == 448.0 and float(t[0x01]) == 2.0 ** -9 and float(t[0x08]) == 2.0 ** -6 and math.isnan(float(t[0x7F]))
    fin = torch.isfinite(t)
    assert int(fin.sum()) == 254
    assert torch.equal(kr.e4m3_encode(t)[fin], torch.arange(256, dtype=torch.uint8)[fin])
    assert kr.e4m3_encode(torch.tensor([math.nan, math.inf, -math.inf])).tolist() == [0x7F] * 3


def test_the_encoder_agrees_with_torchs_cast_where_that_is_defined():
    if not hasattr(torch, "float8_e4m3fn"):
        pytest.skip("this torch has no float8_e4m3fn")
    g = torch.Generator().manual_seed(0)
    y = (torch.rand(200_000, generator=g, dtype=torch.float64) * 2 - 1) * 448
    y = torch.cat([y, y * 2.0 ** -8, y * 2.0 ** -14, y * 2.0 ** -17]).float()
    t = kr.e4m3_value_table()
    mids = (t[:0x7E] + t[1:0x7F]) / 2                                   # every midpoint between neighbouring codes, both signs
    y = torch.cat([y, mids.float(), -mids.float(), torch.tensor([0.0, -0.0, 448.0, -448.0])])
    assert torch.equal(kr.e4m3_encode(y.double()), y.to(torch.float8_e4m3fn).view(torch.uint8))


def test_ties_go_to_the_even_code_and_half_the_smallest_subnormal_to_zero():
    s = 2.0 ** -9
    y = torch.tensor([17.0, 19.0, 1.5 * s, 2.5 * s, 0.5 * s, -0.5 * s, 0.5078125 * s, 7.5 * s, 15.5 * s], dtype=torch.float64)
    assert kr.e4m3_value_table()[kr.e4m3_encode(y).long()].tolist() == [16.0, 20.0, 2 * s, 2 * s, 0.0, -0.0, s, 8 * s, 16 * s]
    assert int(kr.e4m3_encode(torch.tensor([-0.5 * s], dtype=torch.float64))) == 0x80


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
def test_the_exponent_rule_at_its_edges(dtype):
    lines = kr.edge_lines(16, dtype)
    codes, b = kr.quantise(lines.view(-1, 1, 16))
    b = b.view(-1).tolist()
    name = {n: i for i, n in enumerate(kr.EDGE_NAMES)}
    assert len(kr.EDGE_NAMES) == lines.shape[0]
    assert b[name["zeros"]] == 127 and b[name["all nan"]] == 127 and b[name["subnormal absmax"]] == 0
    assert b[name["m=1.75"]] == 127 - 2 - 8 and b[name["m=1.75-ulp"]] == 127 + 1 - 8 and b[name["m=1.75+ulp"]] == 127 + 4 - 7
    assert (b[name["448"]], b[name["-448*2^-5"]], b[name["-448*2^9"]]) == (127, 122, 136)
    assert bool((codes[name["all nan"]] == 0x7F).all()) and bool((codes[name["zeros"]] == 0).all())
    top = kr.e4m3_value_table()[codes.view(-1, 16).long()].abs().nan_to_num(0.0).amax(dim=1)
    for n in ("m=1.75", "448", "-448*2^-5", "-448*2^9"):                # the largest scaled magnitude is 448 exactly ...
        assert float(top[name[n]]) == 448.0
    live = [i for i, n in enumerate(kr.EDGE_NAMES) if n not in ("zeros", "all nan", "subnormal absmax")]
    assert bool((top[live] >= 224.0).all())                             # ... and never below half of it (224.5 rounds to 224): e is the SMALLEST that fits
    nan_line = codes.view(-1, 16)[name["nan and inf"]]
    assert nan_line[1:4].tolist() == [0x7F] * 3 and int(nan_line[0]) != 0x7F


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
def test_dequantised_values_are_exact_in_the_model_dtype_and_requantise_to_their_own_values(dtype):
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(64, 2, 64, generator=g) * torch.exp2(torch.randint(-20, 20, (64, 2, 1), generator=g).float())).to(dtype)
    codes, b = kr.quantise(x)
    d = kr.dequantise(codes, b)
    assert torch.equal(d.to(dtype).float(), d)                          # four significant bits times a power of two
    c2, b2 = kr.quantise(d.to(dtype))                                   # (the bytes may differ: an absmax that rounded down to m = 1.75 takes e - 1)
    assert torch.equal(kr.dequantise(c2, b2), d)
    step = torch.exp2(b.float() - 127 + 5)[..., None]                   # the widest e4m3 step at that exponent: 2^5 between 256 and 448
    assert bool(((d - x.float()).abs() <= step / 2).all())


@pytest.mark.parametrize("defect", kr.DEFECTS)
def test_every_planted_defect_is_caught(defect):
    """By the store test's comparison (codes and exponent bytes against the reference's) or, where the stored bytes are right and only the reading is
    wrong, by the attention tests' (the dequantised problem differs)."""
    for dtype in DTYPES:
        lines = kr.edge_lines(16, dtype)
        n = lines.shape[0] // 2 * 2
        x = lines[:n].view(-1, 2, 16)                                   # two kv heads per position: a neighbour to confuse with
        codes, b = kr.quantise(x)
        if defect != "k_exp_for_v":
            c2, b2 = kr.quantise(x, defect)
            assert not (torch.equal(c2, codes) and torch.equal(b2, b)), defect
        if defect in ("threshold", "exp_plus_one"):                     # (stored bytes alone show these: no drawn line has a mantissa of exactly
            continue                                                    # 1.75, and one exponent more loses bits only among the subnormal codes)
        p = dr.make_problem(dr.Geometry(4, 2, 16), dtype, [5, 17, 33], "gauss", 40)
        p = p._replace(v_cache=p.v_cache * 8)                           # K and V lines of a position differ in magnitude
        (q, good), (q2, bad) = kr.quantise_problem(p), kr.quantise_problem(p, defect)
        live = kr.live_positions(p)
        same = torch.equal(good.k_cache[live], bad.k_cache[live]) and torch.equal(good.v_cache[live], bad.v_cache[live])
        assert not same, defect
        ref, ref2 = dr.exact(good), dr.exact(bad)
        assert not torch.equal(ref.out, ref2.out), defect


def test_a_problem_keeps_its_poison_and_its_live_lines():
    p = dr.make_problem(dr.Geometry(4, 1, 64), torch.bfloat16, [3, 70, 1], "sink", 80)
    q, d = kr.quantise_problem(p)
    live = kr.live_positions(p)
    assert int(live.sum()) == 74
    assert bool((q.k_codes[~live] == kr.NAN_CODE).all()) and bool((q.v_exp[~live] == kr.POISON_EXP).all())
    assert bool(torch.isnan(d.k_cache[~live].float()).all()) and bool(torch.isfinite(d.v_cache[live].float()).all())
    assert q.k_codes.dtype == torch.uint8 and q.k_exp.shape == (5, 80, 1) and d.k_cache.dtype == torch.bfloat16
    assert dr.violations(dr.stored(dr.restate(d).out, d.dtype), None, d, dr.exact(d)) == []
