"""CPU: the row rule of FP8 weights (tests/weight_fp8_ref.py, a thin restatement over tests/kv_fp8_ref.py) on the rows the GPU tests use — the
exponent bytes the definition names, torch's own e4m3 cast of the scaled rows, the special codes, and that EVERY dequantised value of the test
inputs is exactly a bf16 number (what the bit-equality contract of the ``_w8`` GEMMs stands on)."""
import pytest
import torch

import kv_fp8_ref as kq
import weight_fp8_ref as wq

KS = [64, 192, 2048]


@pytest.mark.parametrize("K", KS)
def test_edge_rows_follow_the_rule(K):
    w, names = wq.edge_rows(K)
    codes, b = wq.quantise(w)
    assert codes.shape == w.shape and codes.dtype == torch.uint8 and b.shape == (w.shape[0],) and b.dtype == torch.uint8
    row = {n: i for i, n in enumerate(names)}
    assert int(b[row["zeros"]]) == 127 and not bool(codes[row["zeros"]].any())
    # absmax 1.75 * 2^-3: the smallest e with absmax * 2^-e <= 448 is -11 (448 exactly); one bf16 step above, -10
    assert int(b[row["m=1.75"]]) == 127 - 11 and int(codes[row["m=1.75"]].max()) == 0xFE      # -448
    assert int(b[row["m=1.75+ulp"]]) == 127 - 10
    assert int(b[row["large last"]]) == 127 - 10                                               # 0.37 = 1.48 * 2^-2
    assert [int(codes[row["minus zero"], k]) for k in (0, K // 2, K - 1)] == [0x80] * 3
    assert int(codes[row["nan"], 5 % K]) == wq.NAN_CODE and int(codes[row["inf"], K - 1]) == wq.NAN_CODE and int(codes[row["inf"], 1]) == wq.NAN_CODE
    # a row is its own line: the exponent of a row does not depend on its neighbours
    for i in range(w.shape[0]):
        ci, bi = wq.quantise(w[i:i + 1])
        assert torch.equal(ci[0], codes[i]) and int(bi[0]) == int(b[i])
    # the largest code of every row with a finite non-zero element lies in [224, 448] (a scaled absmax in (224, 448], rounded): the exponent is
    # the smallest that fits
    val = kq.e4m3_value_table()[codes.long()].abs()
    top = torch.where(torch.isnan(val), torch.zeros_like(val), val).amax(dim=1)
    live = top > 0
    assert bool(((top[live] >= 224) & (top[live] <= 448)).all())


@pytest.mark.parametrize("K", KS)
def test_codes_are_torchs_own_cast_of_the_scaled_row(K):
    w, _ = wq.edge_rows(K)
    codes, b = wq.quantise(w)
    scaled = w.double() * kq._pow2(127 - b.long())[:, None]
    fin = torch.isfinite(scaled)
    ref = scaled.float().to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(codes[fin], ref[fin])


@pytest.mark.parametrize("K", KS)
def test_every_dequantised_value_is_a_bf16_number(K):
    w, _ = wq.edge_rows(K)
    codes, b = wq.quantise(w)
    d = wq.dequantise_bf16(codes, b)            # asserts exactness itself
    f = wq.dequantise(codes, b)
    fin = torch.isfinite(f)
    assert torch.equal(d.float()[fin], f[fin])
    # and it is close to the weight: half a step of the row's grid (the absmax code is at least 224: 2^-4 of the absmax among normals)
    a = torch.where(torch.isfinite(w.float()), w.float().abs(), torch.zeros(())).amax(dim=1, keepdim=True)
    err = (f - w.float()).abs()
    assert bool((err[fin] <= (a.expand_as(err) * 2.0 ** -4)[fin]).all())
    torch.manual_seed(0)
    big = (torch.randn(256, 512) * 0.02).to(torch.bfloat16)
    wq.dequantise_bf16(*wq.quantise(big))
