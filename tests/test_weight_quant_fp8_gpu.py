"""ssi_weight_quant_fp8 (csrc/gemm_wq8.hip) against the CPU restatement of the rule (tests/weight_fp8_ref.py): codes and exponent bytes are EQUAL,
byte for byte, on normal(0, 0.02) rows, a zero row, an absmax of mantissa exactly 1.75 and one bf16 step above, a row whose only large element is the
last (the maximum has to cross the wave), -0.0, a NaN and an infinite element, at K = 64 (8 live lanes), 192 and 2048 (four trips), with packed and
with pitched code rows (the padding bytes stay untouched), on a pitched source, and at a row count that is no multiple of the four rows a workgroup takes."""
import pytest
import torch

import weight_fp8_ref as wq

pytestmark = pytest.mark.gpu

DEV = "cuda"
KS = [64, 192, 2048]
FILL = 0xA5


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


@pytest.fixture(scope="module")
def cases():
    """K -> (rows bf16 [n, K], names, reference codes, reference exponent bytes), computed once."""
    out = {}
    for K in KS:
        w, names = wq.edge_rows(K)
        out[K] = (w, names) + wq.quantise(w)
    return out


@pytest.mark.parametrize("pitch", [0, 64])
@pytest.mark.parametrize("K", KS)
def test_codes_and_exponents_equal_the_reference(ops, cases, K, pitch):
    w, names, ref_c, ref_b = cases[K]
    n = w.shape[0]
    assert n % 4 != 0                                                          # the last workgroup has idle waves
    store = torch.full((n, K + pitch), FILL, dtype=torch.uint8, device=DEV)
    exps = torch.full((n + 3,), FILL, dtype=torch.uint8, device=DEV)
    ops.weight_quant_fp8(w.to(DEV), store[:, :K], exps[:n])
    torch.cuda.synchronize()
    got_c, got_b = store[:, :K].cpu(), exps[:n].cpu()
    for i, name in enumerate(names):
        assert int(got_b[i]) == int(ref_b[i]), (name, int(got_b[i]), int(ref_b[i]))
        bad = (got_c[i] != ref_c[i]).nonzero().flatten()
        assert bad.numel() == 0, (name, bad[:8].tolist(), got_c[i][bad[:8]].tolist(), ref_c[i][bad[:8]].tolist())
    assert bool((store[:, K:] == FILL).all()) and bool((exps[n:] == FILL).all())   # nothing behind a row's K codes or behind exps[n - 1]


def test_a_pitched_source_and_many_rows(ops):
    g = torch.Generator().manual_seed(11)
    N, K, ld = 203, 192, 256
    src = torch.full((N, ld), float("nan"), dtype=torch.bfloat16)
    src[:, :K] = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16)
    ref_c, ref_b = wq.quantise(src[:, :K].contiguous())
    codes = torch.empty((N, K), dtype=torch.uint8, device=DEV)
    exps = torch.empty((N,), dtype=torch.uint8, device=DEV)
    ops.weight_quant_fp8(src.to(DEV)[:, :K], codes, exps)
    assert torch.equal(codes.cpu(), ref_c) and torch.equal(exps.cpu(), ref_b)


def test_refusals(ops):
    w = torch.zeros((4, 96), dtype=torch.bfloat16, device=DEV)                 # K % 64
    with pytest.raises(RuntimeError):
        ops.weight_quant_fp8(w, torch.empty((4, 96), dtype=torch.uint8, device=DEV), torch.empty(4, dtype=torch.uint8, device=DEV))
    w = torch.zeros((4, 64), dtype=torch.bfloat16, device=DEV)
    odd = torch.empty((4, 72), dtype=torch.uint8, device=DEV)[:, :64]          # code rows off 16-byte boundaries
    with pytest.raises(RuntimeError):
        ops.weight_quant_fp8(w, odd, torch.empty(4, dtype=torch.uint8, device=DEV))
