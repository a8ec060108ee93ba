"""The skinny GEMMs on FP8 weights (csrc/gemm_wq8.hip: ssi_gemm_skinny_w8, ssi_gemm_skinny_rope_w8, ssi_gemm_skinny_swiglu_w8) are held to the
property that defines them: the output is BIT-EQUAL to the matching plain entry (ssi_gemm_skinny*, pinned to float64 by tests/test_gemm_skinny_gpu.py)
called on the dequantised matrix stored as bf16.  Weights are normal(0, 0.02) rows quantised by the CPU restatement (tests/weight_fp8_ref.py), so a
failure here is the GEMM's and not the quantiser's; activations are randn, full mantissas.

Shapes: every m-tile count and its edges (M = 1, 15, 16, 17, 32, 33, 64); for the loader that runs two chunks ahead, K with fewer 64-wide chunks
than waves (64; 4-wave form: 64), one chunk per wave (512; 4-wave form: 256 is covered by 320's first round), an odd count per wave (576, 1088; 320,
576) and many (2048).  Every output buffer is one row taller and 16 columns wider than the result and filled with a sentinel on both sides, so
the comparison also shows that nothing outside [M, N] is written; rows of A at and beyond M hold NaN; the exponent bytes are followed by poison
bytes (255: a factor of 2^128) that a read behind exps[N - 1] would pick up.

The issue lists I = 32 for the SwiGLU form; the skinny contract refuses I % 64 (include/ssi_hip.h), so at I = 32 the test asserts that the _w8
entry refuses exactly as its plain sibling does, and the bit-equality cases are I = 64 (two workgroups) and 192."""
import pytest
import torch

import weight_fp8_ref as wq

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
MS = [1, 15, 16, 17, 32, 33, 64]
SENTINEL = -7.25
TLEN = 96
_CACHE: dict = {}


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


@pytest.fixture(scope="module")
def table():
    from ssi.model import llama3_rope_table
    return llama3_rope_table(64, TLEN).to(DEV)


def weights(nw, K, seed=0):
    """(codes, exps followed by poison, dequantised bf16) on the device for a normal(0, 0.02) matrix [nw, K]; cached, never modified."""
    key = (nw, K, seed)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(100 + 7 * nw + K + seed)
        w = (torch.randn(nw, K, generator=g) * 0.02).to(BF)
        codes, b = wq.quantise(w)
        deq = wq.dequantise_bf16(codes, b)
        exps = torch.full((nw + 64,), wq.POISON_EXP, dtype=torch.uint8)
        exps[:nw] = b
        _CACHE[key] = (codes.to(DEV), exps.to(DEV)[:nw], deq.to(DEV))
    return _CACHE[key]


def acts(K, seed=0):
    key = ("a", K, seed)
    if key not in _CACHE:
        _CACHE[key] = torch.randn(65, K, generator=torch.Generator().manual_seed(9 + K + seed)).to(BF).to(DEV)
    return _CACHE[key]


def rows_of(a, M):
    """The first M rows of ``a`` as a view of a buffer whose rows at and beyond M are NaN."""
    buf = a.clone()
    buf[M:] = float("nan")
    return buf[:M]


def out(M, N):
    return torch.full((M + 1, N + 16), SENTINEL, dtype=BF, device=DEV)


def same_bits(got, ref, what):
    ne = got.view(torch.int16) != ref.view(torch.int16)
    if bool(ne.any()):
        bad = ne.nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {ne.numel()} elements differ, first at {bad[0].tolist()}: "
                             f"{float(got[tuple(bad[0])])!r} against {float(ref[tuple(bad[0])])!r}")


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("N,K", [(64, 64), (64, 512), (64, 576), (64, 1088), (2048, 2048), (8192, 64), (8192, 320), (8192, 576)])
def test_plain_and_residual_bit_equal_to_the_plain_entry_on_the_dequantised_matrix(ops, N, K, res):
    codes, exps, deq = weights(N, K)
    a = acts(K)
    r = torch.randn(65, N + 16, generator=torch.Generator().manual_seed(N + K)).to(BF).to(DEV)
    for M in MS:
        x = rows_of(a, M)
        rr = r[:M, :N] if res else None
        c8, c16 = out(M, N), out(M, N)
        ops.gemm_skinny_w8(x, codes, exps, c8[:M, :N], residual=rr)
        ops.gemm_skinny(x, deq, c16[:M, :N], residual=rr)
        same_bits(c8, c16, f"N={N} K={K} M={M} res={res}")
        assert not bool(torch.isnan(c8).any()) and bool((c8[:M, :N] != SENTINEL).any())


@pytest.mark.parametrize("K", [64, 576])
def test_rope_bit_equal(ops, table, K):
    N, rot = 192, 2                                                       # two rotated heads and one that is not
    codes, exps, deq = weights(N, K)
    a = acts(K)
    edge = torch.tensor([0, TLEN - 1, TLEN + 7, 37, -2, 1], dtype=torch.int32)   # first, last, past the table (clamped), negative (clamped)
    for M in MS:
        pos = torch.full((M + 1,), 1 << 30, dtype=torch.int32)            # (the entry behind the last row is never read)
        pos[:M] = edge[torch.arange(M) % edge.numel()]
        pos = pos.to(DEV)[:M]
        x = rows_of(a, M)
        c8, c16 = out(M, N), out(M, N)
        ops.gemm_skinny_rope_w8(x, codes, exps, c8[:M, :N], rot, 64, table, pos)
        ops.gemm_skinny_rope(x, deq, c16[:M, :N], rot, 64, table, pos)
        same_bits(c8, c16, f"rope K={K} M={M}")
        assert not bool(torch.isnan(c8).any())
        if M >= 3:                                                        # a position past the table is the last position
            last = torch.full((M,), TLEN - 1, dtype=torch.int32, device=DEV)
            c_last = out(M, N)
            ops.gemm_skinny_rope_w8(x, codes, exps, c_last[:M, :N], rot, 64, table, last)
            same_bits(c8[2], c_last[2], f"rope clamp K={K} M={M}")


@pytest.mark.parametrize("want_gu", [False, True])
@pytest.mark.parametrize("K", [64, 576])
@pytest.mark.parametrize("inter", [32, 64, 192])
def test_swiglu_bit_equal(ops, inter, K, want_gu):
    g = torch.Generator().manual_seed(inter + K)
    w = (torch.randn(2 * inter, K, generator=g) * 0.05).to(BF)            # (wider than 0.02: the activations are not all near zero)
    codes, b = wq.quantise(w)
    deq = wq.dequantise_bf16(codes, b).to(DEV)
    exps = torch.full((2 * inter + 64,), wq.POISON_EXP, dtype=torch.uint8)
    exps[:2 * inter] = b
    codes, exps = codes.to(DEV), exps.to(DEV)[:2 * inter]
    a = acts(K)
    for M in MS:
        x = rows_of(a, M)
        gu8, gu16, act8, act16 = out(M, 2 * inter), out(M, 2 * inter), out(M, inter), out(M, inter)
        call8 = lambda: ops.gemm_skinny_swiglu_w8(x, codes, exps, gu8[:M, :2 * inter] if want_gu else None, act8[:M, :inter])  # noqa: E731
        call16 = lambda: ops.gemm_skinny_swiglu(x, deq, gu16[:M, :2 * inter] if want_gu else None, act16[:M, :inter])  # noqa: E731
        if inter % 64:                                                    # refused by the skinny contract, by both entries alike, before any launch
            for call, name in ((call8, "ssi_gemm_skinny_swiglu_w8"), (call16, "ssi_gemm_skinny_swiglu")):
                with pytest.raises(RuntimeError, match=name):
                    call()
            assert bool((act8 == SENTINEL).all())
            continue
        call8()
        call16()
        same_bits(act8, act16, f"swiglu act I={inter} K={K} M={M}")
        same_bits(gu8, gu16, f"swiglu gu I={inter} K={K} M={M}")
        assert not bool(torch.isnan(act8).any()) and bool((gu8[:M, :2 * inter] != SENTINEL).any()) == want_gu


@pytest.mark.parametrize("N,K", [(64, 576), (8192, 320)])
def test_a_row_has_the_same_bits_whatever_M_is(ops, N, K):
    codes, exps, _ = weights(N, K)
    a = acts(K)
    got = {}
    for M in (1, 17, 64):
        c = out(M, N)
        ops.gemm_skinny_w8(rows_of(a, M), codes, exps, c[:M, :N])
        got[M] = c[0, :N].clone()
    same_bits(got[17], got[1], f"row 0, M=17 against M=1 (N={N})")
    same_bits(got[64], got[1], f"row 0, M=64 against M=1 (N={N})")


@pytest.mark.parametrize("N,K,n,k", [(64, 576, 37, 575), (8192, 320, 8191, 0)])
def test_a_nan_code_makes_its_own_column_nan_and_moves_no_other(ops, N, K, n, k):
    codes, exps, _ = weights(N, K)
    hit = codes.clone()
    hit[n, k] = wq.NAN_CODE
    a = acts(K)
    for M in (1, 33):
        x = rows_of(a, M)
        c0, c1 = out(M, N), out(M, N)
        ops.gemm_skinny_w8(x, codes, exps, c0[:M, :N])
        ops.gemm_skinny_w8(x, hit, exps, c1[:M, :N])
        assert bool(torch.isnan(c1[:M, n]).all())
        keep = torch.ones(N + 16, dtype=torch.bool, device=DEV)
        keep[n] = False
        same_bits(c1[:, keep], c0[:, keep], f"columns beside {n} (N={N} M={M})")
        assert bool((c1[M] == SENTINEL).all())


def test_refusals_are_the_plain_entries(ops, table):
    codes, exps, deq = weights(64, 64)
    a = acts(64)
    c = out(64, 64)
    # the RoPE refusals, one body for both entries (csrc/gemm_skinny.h): each entry under its own name, before any launch
    pos = torch.zeros(4, dtype=torch.int32, device=DEV)
    for heads, hd, tab in ((1, 128, torch.zeros((TLEN, 64, 2), dtype=torch.float32, device=DEV)),   # head_dim 128 (a table of 64 columns)
                           (2, 64, table)):                                                           # n_heads_rot * 64 > N = 64
        with pytest.raises(RuntimeError, match="ssi_gemm_skinny_rope_w8: head_dim 64"):
            ops.gemm_skinny_rope_w8(a[:4], codes, exps, c[:4, :64], heads, hd, tab, pos)
        with pytest.raises(RuntimeError, match="ssi_gemm_skinny_rope: head_dim 64"):
            ops.gemm_skinny_rope(a[:4], deq, c[:4, :64], heads, hd, tab, pos)
    assert bool((c == SENTINEL).all())
    with pytest.raises(RuntimeError, match="ssi_gemm_skinny_w8"):          # 65 rows
        ops.gemm_skinny_w8(a, codes, exps, torch.empty((65, 64), dtype=BF, device=DEV))
    pitched = torch.zeros((64, 72), dtype=torch.uint8, device=DEV)[:, :64]  # code rows off 16-byte boundaries
    with pytest.raises(RuntimeError, match="ssi_gemm_skinny_w8"):
        ops.gemm_skinny_w8(a[:4], pitched, exps, c[:4, :64])
    w96, e96 = torch.zeros((96, 64), dtype=torch.uint8, device=DEV), torch.zeros(96, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="ssi_gemm_skinny_w8"):          # N % 64
        ops.gemm_skinny_w8(a[:4], w96, e96, torch.empty((4, 96), dtype=BF, device=DEV))
    assert bool((c == SENTINEL).all())
