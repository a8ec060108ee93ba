"""Parity of the skinny bf16 GEMM (csrc/gemm_skinny.hip: ssi_gemm_skinny, ssi_gemm_skinny_rope, ssi_gemm_skinny_swiglu) for 1 to 64 rows, in all
four epilogues (plain, residual, RoPE, SwiGLU forward), at every m-tile count (MT = 1, 2, 4 with full and ragged last tiles, a single row), both
workgroup shapes (16 weight rows and 8 waves below N = 8192, 64 weight rows and 4 waves from there; SwiGLU: 32 gate + 32 up rows) and the K edges of
the split over the waves (one 64-wide chunk, fewer chunks than waves, uneven shares, many chunks, and K = 8192).

Every reference is float64 on the CPU from seeded inputs and EVERY element is compared, in the three kinds of tests/test_gemm_mfma_parity_gpu.py
(helpers restated here):
  1. exact integers (A in [-3, 3], W in [-5, 5], R small integers, K <= 1664: every fp32 operation is exact in any order): bit-equal to the
     float64 result under the documented rounding points, and bit-equal to ops.gemm / ops.gemm_rope / ops.gemm_swiglu_fwd on the same rows padded
     to 256.  RoPE multiplies by the real table, so against float64 its rotated columns get the project's bound for the rotation alone
     (two fp32 products and their sum, one rounding to storage); against the padded call they are bit-equal.
  2. gather probes: one operand holds a single 1 per row at a seeded permutation of k, the other is randn: the output is the selected element bit
     for bit.  The kernel gives lane group g of a 64-wide chunk k = 16 g .. 16 g + 15 instead of the instruction's 8 g .. 8 g + 7: any
     disagreement between the two operands about that shows here on full-mantissa data.
  3. randn against float64, per element: 0.5 ulp_bf16 per rounding to storage + C_ACC K 2^-24 (|A| @ |W|), C_ACC = 1 (Higham's any-order bound
     with correctly rounded adds, derived in that file's docstring).

     The padded comparison of the residual form runs at N = 1024 only: off the 256-tile shapes ops.gemm is the generic kernel, which rounds
     product + residual once, and that is not the kernel this one stands in for.  At the issue's RoPE and SwiGLU widths the padded entries
     run their unfused fallbacks; test_bit_equal_to_the_mfma_tile_kernels_themselves adds N = 512 with 256 rotated columns and I = 256, where
     the fused 256-tile kernels run (IMPL_MFMA forced).

Worst error / bound measured on the MI355X with C_ACC = 1 (pytest -s prints them): plain 0.9976, residual 0.9976, RoPE 0.9969 (the rotation alone,
on exact integer products: 1.0000 to four digits), SwiGLU forward (gate and up; the activation is held bit for bit to ops.swiglu_fwd, which test_row_kernels_gpu.py
pins to float64) 0.9959.

Not testable from here: a NEGATIVE position cannot be refused with SSI_ERR_ARG by the host entry without reading device memory back in the middle of
a decode step; positions are clamped to [0, table_len - 1] on the device on both sides, and that is what the bounds-of-access test checks."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
U32 = 2.0 ** -24
C_ACC = 1
SENTINEL = -7.25
EPIS = ["plain", "res", "rope", "swiglu"]
MS = [1, 2, 15, 16, 17, 31, 32, 33, 48, 63, 64]
KS = [64, 128, 192, 320, 576, 1664]
# output widths per epilogue: plain / residual N (8192: the 64-row workgroup, at K = 64 only); RoPE (N, rotated heads) with 2 to 6 heads of 64, some
# but not all rotated; SwiGLU inter
WIDTHS = {"plain": [64, 128, 320, 1024], "res": [64, 128, 320, 1024], "rope": [(128, 1), (192, 2), (320, 3), (384, 4)], "swiglu": [64, 192]}
WIDE_N = 8192
TLEN = 512

_WORST: dict[str, float] = {}
_CACHE: dict[tuple, tuple] = {}


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from ssi import _lib
    return _lib


@pytest.fixture(scope="module")
def table():
    from ssi.model import llama3_rope_table
    return llama3_rope_table(64, TLEN)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam in sorted(_WORST):
        print(f"\ngemm-skinny worst error/bound (C_ACC = {C_ACC})  {fam:<24s} {_WORST[fam]:.4f}", end="")
    print()


# ---- helpers of tests/test_gemm_mfma_parity_gpu.py, restated ---------------------------------------------------------------------------------
def ints(shape, lim, seed):
    return torch.randint(-lim, lim + 1, shape, generator=torch.Generator().manual_seed(seed)).to(BF)


def rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(BF)


def ulp_bf16(ref):
    _, e = torch.frexp(ref.abs())
    e = torch.where(ref == 0, torch.full_like(e, -1000), e)
    return torch.ldexp(torch.ones_like(ref), (e - 1).clamp(min=-126) - 7)


def r16(v64):
    return v64.float().to(BF).double()


def acc_bound(absS, K):
    return C_ACC * K * U32 * absS


def half_ulp(ref, carried):
    return 0.5 * ulp_bf16(ref.abs() + carried)


def rounded(ref, carried):
    return carried + half_ulp(ref, carried)


def check(family, got, ref, bound, what):
    got64 = got.detach().cpu().double()
    assert got64.shape == ref.shape, f"{what}: shape {tuple(got64.shape)} vs {tuple(ref.shape)}"
    err = (got64 - ref).abs()
    bound = bound.expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ok = err <= bound
    if bool(ok.all()):
        worst = float(ratio.max()) if ratio.numel() else 0.0
        _WORST[family] = max(_WORST.get(family, 0.0), worst)
        return
    bad = (~ok).nonzero()
    fin = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, -1.0))
    w = tuple(int(v) for v in (fin == fin.max()).nonzero()[0])
    raise AssertionError(f"{what}: {bad.shape[0]} of {err.numel()} elements miss their bound; worst at {w}: got {float(got64[w])!r} ref "
                         f"{float(ref[w])!r} err {float(err[w]):.3e} bound {float(bound[w]):.3e} (ratio {float(ratio[w]):.3f}); "
                         f"first at {tuple(int(v) for v in bad[0])}")


def check_bits(got, ref, what):
    got = got.detach().cpu()
    ref16 = ref.to(BF) if ref.dtype != BF else ref.detach().cpu()
    assert got.dtype == BF and got.shape == ref16.shape, f"{what}: {got.dtype} {tuple(got.shape)} vs {tuple(ref16.shape)}"
    ne = got.contiguous().view(torch.int16) != ref16.contiguous().view(torch.int16)
    if not bool(ne.any()):
        return
    bad = ne.nonzero()
    w = tuple(int(v) for v in bad[0])
    rows, cols = sorted({int(v) for v in bad[:, -2]}), sorted({int(v) for v in bad[:, -1]})
    raise AssertionError(f"{what}: {bad.shape[0]} of {ne.numel()} elements differ; first at {w}: got {float(got[w])!r} ref {float(ref16[w])!r}; "
                         f"rows {rows[:6]}.. ({len(rows)}), columns {cols[:6]}.. ({len(cols)})")


def _rope64(p, bp, table, pos, rot_cols):
    """Interleaved rotation of columns [0, rot_cols) of p (float64) in 64-wide heads; bp is the error bound p arrives with."""
    rows = p.shape[0]
    cs = table.double()[pos]
    c, s = cs[:, None, :, 0], cs[:, None, :, 1]
    v, bv = p[:, :rot_cols].reshape(rows, -1, 32, 2), bp[:, :rot_cols].reshape(rows, -1, 32, 2)
    x0, x1, b0, b1 = v[..., 0], v[..., 1], bv[..., 0], bv[..., 1]
    o = torch.stack([x0 * c - x1 * s, x1 * c + x0 * s], -1).reshape(rows, rot_cols)
    m0, m1 = x0.abs() + b0, x1.abs() + b1
    mag = torch.stack([m0 * c.abs() + m1 * s.abs(), m1 * c.abs() + m0 * s.abs()], -1).reshape(rows, rot_cols)
    carried = torch.stack([b0 * c.abs() + b1 * s.abs(), b1 * c.abs() + b0 * s.abs()], -1).reshape(rows, rot_cols)
    return o, rounded(o, carried + 2 * U32 * mag)


# ---- one problem: 64 rows of A, the weights, float64 products, residual, positions; cached, never modified -----------------------------------
def geometry(epi, width):
    """(weight rows, output columns, rotated columns)."""
    if epi == "rope":
        return width[0], width[0], 64 * width[1]
    return (2 * width, 2 * width, 0) if epi == "swiglu" else (width, width, 0)


def problem(epi, width, K, integer):
    key = (epi, width, K, integer)
    if key not in _CACHE:
        nw = geometry(epi, width)[0]
        seed = 1000 * KS.index(K) + 17 * nw + int(integer) if K in KS else 77 + nw + K
        A, W = (ints((64, K), 3, seed), ints((nw, K), 5, seed + 1)) if integer else (rnd((64, K), seed), rnd((nw, K), seed + 1))
        S = A.double() @ W.double().t()
        absS = None if integer else A.double().abs() @ W.double().abs().t()
        R = ints((64, nw), 6, seed + 2) if integer else rnd((64, nw), seed + 2)
        pos = (torch.arange(64) * 37 + 11) % TLEN                       # not monotonic, up to the end of the table
        _CACHE[key] = (A, W, S, absS, R, pos, A.to(DEV), W.to(DEV), R.to(DEV), pos.to(torch.int32).to(DEV))
    return _CACHE[key]


def launch(ops, epi, width, a, w, r, pos, table_dev, out=None, want_gu=True):
    """The skinny entry of `epi` on the rows of `a`: returns the output (SwiGLU: (gu or None, act)), sentinel-filled before the call."""
    M = a.shape[0]
    _, cols, rot = geometry(epi, width)
    new = lambda n: torch.full((M, n), SENTINEL, dtype=BF, device=DEV)   # noqa: E731
    if epi == "swiglu":
        gu, act = (new(cols) if want_gu else None), new(cols // 2)
        ops.gemm_skinny_swiglu(a, w, gu, act)
        return gu, act
    c = new(cols) if out is None else out
    if epi == "rope":
        ops.gemm_skinny_rope(a, w, c, rot // 64, 64, table_dev, pos)
    else:
        ops.gemm_skinny(a, w, c, residual=r if epi == "res" else None)
    return c


def padded_reference(ops, epi, width, a, w, r, pos, table_dev):
    """The 256-tile entry the epilogue stands in for, on the 64 rows padded to 256 (pad rows: zeros, position 0)."""
    _, cols, rot = geometry(epi, width)
    ap = torch.zeros((256, a.shape[1]), dtype=BF, device=DEV)
    ap[:64] = a
    c = torch.full((256, cols), SENTINEL, dtype=BF, device=DEV)
    if epi == "swiglu":
        act = torch.full((256, cols // 2), SENTINEL, dtype=BF, device=DEV)
        ops.gemm_swiglu_fwd(ap, w, c, act)
        return c[:64], act[:64]
    if epi == "rope":
        pp = torch.zeros(256, dtype=torch.int32, device=DEV)
        pp[:64] = pos
        ops.gemm_rope(ap, w, c, 256, rot // 64, 64, table_dev, positions=pp)
    else:
        rp = None
        if epi == "res":
            rp = torch.zeros((256, cols), dtype=BF, device=DEV)
            rp[:64] = r
        ops.gemm(0, ap, w, c, residual=rp)
    return c[:64]


def against_float64(ops, epi, width, K, integer, M, out, table, tag):
    """`out` of the first M rows of problem(epi, width, K, integer) against float64 under the documented rounding points."""
    A, W, S, absS, R, pos, *_ = problem(epi, width, K, integer)
    S, R, pos = S[:M], R[:M].double(), pos[:M]
    _, cols, rot = geometry(epi, width)
    fam = {"plain": "plain", "res": "residual", "rope": "RoPE", "swiglu": "SwiGLU forward"}[epi]
    if epi == "swiglu":
        gu, act = out
        if integer:
            check_bits(gu, r16(S), tag + " gu")
        else:
            check(fam, gu, S, rounded(S, acc_bound(absS[:M], K)), tag + " gu")
        act_ref = torch.full_like(act, SENTINEL)
        ops.swiglu_fwd(gu.contiguous(), act_ref)
        check_bits(act, act_ref, tag + " act against ops.swiglu_fwd(gu)")
        return
    if integer:
        if epi == "plain":
            check_bits(out, r16(S), tag)
        elif epi == "res":
            check_bits(out, r16(r16(S) + R), tag)
        else:
            check_bits(out[:, rot:], r16(S)[:, rot:], tag + " unrotated columns")
            ref, bound = _rope64(r16(S), torch.zeros_like(S), table, pos, rot)
            check("RoPE on exact products", out[:, :rot], ref, bound, tag + " rotated columns")
        return
    bp = rounded(S, acc_bound(absS[:M], K))
    if epi == "plain":
        check(fam, out, S, bp, tag)
    elif epi == "res":
        ref = S + R
        check(fam, out, ref, rounded(ref, bp + U32 * (S.abs() + R.abs())), tag)
    else:
        check(fam, out[:, rot:], S[:, rot:], bp[:, rot:], tag + " unrotated columns")
        ref, bound = _rope64(S, bp, table, pos, rot)
        check(fam, out[:, :rot], ref, bound, tag + " rotated columns")


def rows_of(out, M):
    return tuple(o[:M] for o in out) if isinstance(out, tuple) else out[:M]


def bits_equal(got, ref, what):
    if isinstance(got, tuple):
        for g, r, n in zip(got, ref, ("gu", "act")):
            if g is not None and r is not None:
                check_bits(g, r, f"{what} {n}")
    else:
        check_bits(got, ref, what)


# =====================================================================================================================
# 1 + 3. exact integers and randn, every M x width x K x epilogue
# =====================================================================================================================
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("epi", EPIS)
def test_every_row_count_and_width_against_float64_and_the_256_tile_kernels(ops, table, epi, K):
    tdev = table.to(DEV)
    for width in WIDTHS[epi]:
        for integer in (True, False):
            _, _, _, _, _, _, a, w, r, pos = problem(epi, width, K, integer)
            # (a residual off the 256-tile shapes goes to the generic kernel, which rounds product + residual ONCE: not the kernel this one stands in for)
            pad = padded_reference(ops, epi, width, a, w, r, pos, tdev) if integer and (epi != "res" or width % 256 == 0) else None
            for M in MS:
                tag = f"skinny[{epi},{M}x{width}x{K},{'int' if integer else 'rand'}]"
                out = launch(ops, epi, width, a[:M], w, r[:M], pos[:M].contiguous(), tdev)
                against_float64(ops, epi, width, K, integer, M, out, table, tag)
                if pad is not None:
                    bits_equal(out, rows_of(pad, M), tag + " against the 256-tile entry on the rows padded to 256")


@pytest.mark.parametrize("epi", ["plain", "res"])
def test_the_64_row_workgroup_from_n_8192(ops, table, epi):
    """N = 8192 takes 4 n-tiles per workgroup and 4 waves: one chunk for wave 0 alone (K = 64) and uneven shares (K = 320)."""
    for K in (64, 320):
        for integer in (True, False):
            _, _, _, _, _, _, a, w, r, pos = problem(epi, WIDE_N, K, integer)
            for M in (1, 17, 33, 64):
                out = launch(ops, epi, WIDE_N, a[:M], w, r[:M], None, None)
                against_float64(ops, epi, WIDE_N, K, integer, M, out, table, f"skinny[{epi},{M}x{WIDE_N}x{K},{'int' if integer else 'rand'}]")


@pytest.mark.parametrize("epi", EPIS)
def test_k_8192_the_split_used_for_w2(ops, table, epi):
    """randn only (integers would leave the exact range): 128 chunks, 16 per wave (SwiGLU: 32)."""
    width = {"plain": 128, "res": 128, "rope": (128, 1), "swiglu": 64}[epi]
    _, _, _, _, _, _, a, w, r, pos = problem(epi, width, 8192, False)
    outs = {}
    for M in (1, 33, 64):
        outs[M] = launch(ops, epi, width, a[:M], w, r[:M], pos[:M].contiguous(), table.to(DEV))
        against_float64(ops, epi, width, 8192, False, M, outs[M], table, f"skinny[{epi},{M}x{width}x8192,rand]")
    # 16 chunks a wave: rows have the same bits at every m-tile count
    bits_equal(outs[1], rows_of(outs[64], 1), f"skinny[{epi},K=8192] row 0 alone")
    bits_equal(outs[33], rows_of(outs[64], 33), f"skinny[{epi},K=8192] first 33 rows")
    last = launch(ops, epi, width, a[63:64], w, r[63:64], pos[63:64].contiguous(), table.to(DEV))
    bits_equal(last, tuple(o[63:64] for o in outs[64]) if isinstance(outs[64], tuple) else outs[64][63:64], f"skinny[{epi},K=8192] row 63 alone")


@pytest.mark.parametrize("epi,width,K", [("rope", (512, 4), 1664), ("rope", (512, 4), 256), ("swiglu", 256, 320), ("swiglu", 256, 384),
                                         ("plain", 256, 1024), ("res", 512, 1664)])
def test_bit_equal_to_the_mfma_tile_kernels_themselves(ops, lib, table, epi, width, K):
    """The widths of the issue's list leave ops.gemm_rope and ops.gemm_swiglu_fwd on their unfused fallbacks (the fused tile kernels need N and the
    rotated columns, or I, in multiples of 256).  Here the 256-tile MFMA kernels themselves run — IMPL_MFMA forced, a fallback would be an error:
    RoPE at N = 512 with 256 rotated columns, SwiGLU at I = 256, on the persistent kernel (K % 128 == 0, K >= 256) and on the 8-wave kernel."""
    tdev = table.to(DEV)
    _, _, _, _, _, _, a, w, r, pos = problem(epi, width, K, True)
    prev = ops.set_impl(lib.IMPL_MFMA)
    try:
        pad = padded_reference(ops, epi, width, a, w, r, pos, tdev)
    finally:
        ops.set_impl(prev)
    for M in (1, 17, 33, 64):
        tag = f"skinny[{epi},{M}x{width}x{K},int]"
        out = launch(ops, epi, width, a[:M], w, r[:M], pos[:M].contiguous(), tdev)
        against_float64(ops, epi, width, K, True, M, out, table, tag)
        bits_equal(out, rows_of(pad, M), tag + " against the MFMA tile kernel on the rows padded to 256")


# =====================================================================================================================
# 2. gather probes
# =====================================================================================================================
def pi_map(n, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.randperm(K, generator=g) for _ in range(-(-n // K))])[:n]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("epi", EPIS)
def test_gather_probes(ops, table, epi, K):
    """W one-hot (row n has its 1 at k = pi(n), at least K rows: every k in one launch) against randn A: C[m, n] == A[m, pi(n)]; then A one-hot
    in groups of 64 rows (row m at k = pi(m)) against randn W: C[m, n] == W[n, pi(m)].  Residual: R = 0 adds nothing.  RoPE: the rotated columns
    equal ops.rope_ of the selected elements.  SwiGLU: gu is the selection, act equals ops.swiglu_fwd of it."""
    tdev = table.to(DEV)
    big = -(-K // 64) * 64
    pos = ((torch.arange(64) * 29 + 3) % TLEN).to(torch.int32).to(DEV)

    def expect(sel, M):   # sel: [M, weight rows] bf16 on the CPU = what the contraction must give
        if epi == "swiglu":
            gu = sel.to(DEV)
            act = torch.full((M, sel.shape[1] // 2), SENTINEL, dtype=BF, device=DEV)
            ops.swiglu_fwd(gu, act)
            return gu, act
        if epi == "rope":
            c = sel.to(DEV).clone()
            ops.rope_(c, 64, rot // 64, 64, tdev, positions=pos[:M].contiguous())
            return c
        return sel

    # W one-hot
    nw = 2 * big if epi == "swiglu" else max(big, 128)
    width = nw // 2 if epi == "swiglu" else (nw, 1) if epi == "rope" else nw
    rot = 64 if epi == "rope" else 0
    pi = pi_map(nw, K, 3000 + K)
    assert set(pi.tolist()) == set(range(K))
    W = torch.zeros(nw, K, dtype=BF)
    W[torch.arange(nw), pi] = 1
    A = rnd((64, K), 3001 + K)
    for M in (1, 31, 64):
        out = launch(ops, epi, width, A[:M].to(DEV), W.to(DEV), torch.zeros((M, nw), dtype=BF, device=DEV), pos[:M].contiguous(), tdev)
        bits_equal(out, expect(A[:M][:, pi], M), f"skinny[{epi},M={M},K={K}] gather probe, W one-hot")
    # A one-hot
    nw = 128
    width = 64 if epi == "swiglu" else (128, 1) if epi == "rope" else 128
    W = rnd((nw, K), 3002 + K)
    pi = pi_map(big, K, 3003 + K)
    for g0 in range(0, big, 64):
        A = torch.zeros(64, K, dtype=BF)
        A[torch.arange(64), pi[g0:g0 + 64]] = 1
        out = launch(ops, epi, width, A.to(DEV), W.to(DEV), torch.zeros((64, nw), dtype=BF, device=DEV), pos, tdev)
        bits_equal(out, expect(W[:, pi[g0:g0 + 64]].t().contiguous(), 64), f"skinny[{epi},K={K}] gather probe, A one-hot, k group {g0 // 64}")


# =====================================================================================================================
# row independence, reproducibility
# =====================================================================================================================
@pytest.mark.parametrize("epi", EPIS)
def test_a_row_has_the_same_bits_alone_among_64_and_after_a_permutation_and_in_every_launch(ops, table, epi):
    tdev = table.to(DEV)
    for K in (320, 1664):
        width = {"plain": 320, "res": 320, "rope": (320, 3), "swiglu": 192}[epi]
        _, _, _, _, _, _, a, w, r, pos = problem(epi, width, K, False)
        full = launch(ops, epi, width, a, w, r, pos, tdev)
        bits_equal(launch(ops, epi, width, a, w, r, pos, tdev), full, f"skinny[{epi},K={K}] second launch")
        for row in (0, 15, 16, 31, 47, 63):
            one = launch(ops, epi, width, a[row:row + 1], w, r[row:row + 1], pos[row:row + 1].contiguous(), tdev)
            bits_equal(one, tuple(o[row:row + 1] for o in full) if isinstance(full, tuple) else full[row:row + 1], f"skinny[{epi},K={K}] row {row} alone")
        for M in (17, 33):   # another MT
            bits_equal(launch(ops, epi, width, a[:M], w, r[:M], pos[:M].contiguous(), tdev), rows_of(full, M), f"skinny[{epi},K={K}] first {M} rows")
        perm = torch.randperm(64, generator=torch.Generator().manual_seed(5)).to(DEV)
        shuffled = launch(ops, epi, width, a[perm].contiguous(), w, r[perm].contiguous(), pos[perm].contiguous(), tdev)
        bits_equal(shuffled, tuple(o[perm] for o in full) if isinstance(full, tuple) else full[perm], f"skinny[{epi},K={K}] rows permuted")


def test_swiglu_without_gu_writes_the_same_activation(ops, table):
    _, _, _, _, _, _, a, w, r, pos = problem("swiglu", 192, 320, False)
    for M in (1, 33, 64):
        gu, act = launch(ops, "swiglu", 192, a[:M], w, None, None, None)
        none, act2 = launch(ops, "swiglu", 192, a[:M], w, None, None, None, want_gu=False)
        assert none is None
        check_bits(act2, act, f"skinny[swiglu,M={M}] act with GU = NULL")


# =====================================================================================================================
# bounds of access
# =====================================================================================================================
@pytest.mark.parametrize("M", [1, 17, 63])
@pytest.mark.parametrize("epi", EPIS)
def test_nothing_outside_the_rows_is_read_or_written(ops, lib, table, epi, M):
    """A, R and the positions are the middle of larger buffers whose other rows are NaN (positions: -1) and whose rows are wider than K (N);
    the outputs are windows of sentinel-filled buffers with ld > N and rows before and behind.  Same bits as the plain call, no NaN, nothing
    outside [M, N] written.  A position past the table, and a negative one, are clamped to the table's ends."""
    tdev = table.to(DEV)
    K = 192
    width = {"plain": 128, "res": 128, "rope": (192, 2), "swiglu": 64}[epi]
    _, _, _, _, R, pos_host, a, w, r, pos = problem(epi, width, K, False)
    _, cols, rot = geometry(epi, width)
    ref = launch(ops, epi, width, a[:M], w, r[:M], pos[:M].contiguous(), tdev)

    def inside(t, pad_cols, fill):
        buf = torch.full((M + 3, t.shape[1] + pad_cols), fill, dtype=t.dtype, device=DEV)
        buf[2:2 + M, 8:8 + t.shape[1]] = t
        return buf, buf[2:2 + M, 8:8 + t.shape[1]]

    _, a_in = inside(a[:M], 24, float("nan"))
    pbuf = torch.full((M + 5,), -1, dtype=torch.int32, device=DEV)
    pbuf[4:4 + M] = pos[:M]
    p_in = pbuf[4:4 + M]
    if epi == "swiglu":
        gbuf, gu = inside(torch.full((M, cols), SENTINEL, dtype=BF, device=DEV), 40, SENTINEL)
        abuf, act = inside(torch.full((M, cols // 2), SENTINEL, dtype=BF, device=DEV), 16, SENTINEL)
        ops.gemm_skinny_swiglu(a_in, w, gu, act)
        outs, bufs = (gu, act), ((gbuf, cols), (abuf, cols // 2))
    else:
        cbuf, c = inside(torch.full((M, cols), SENTINEL, dtype=BF, device=DEV), 40, SENTINEL)
        if epi == "rope":
            ops.gemm_skinny_rope(a_in, w, c, rot // 64, 64, tdev, p_in)
        else:
            r_in = None
            if epi == "res":
                rb = torch.full((M + 3, cols + 40), float("nan"), dtype=BF, device=DEV)   # the residual shares C's leading dimension
                rb[2:2 + M, 8:8 + cols] = r[:M]
                r_in = rb[2:2 + M, 8:8 + cols]
            ops.gemm_skinny(a_in, w, c, residual=r_in)
        outs, bufs = c, ((cbuf, cols),)
    bits_equal(outs, ref, f"skinny[{epi},M={M}] operands inside larger buffers")
    for buf, n in bufs:
        host = buf.cpu()
        mask = torch.ones(host.shape, dtype=torch.bool)
        mask[2:2 + M, 8:8 + n] = False
        assert bool((host[mask] == SENTINEL).all()), f"skinny[{epi},M={M}]: {int((host[mask] != SENTINEL).sum())} elements outside [M, N] were written"
        assert not bool(torch.isnan(host[~mask]).any())
    if epi == "rope":
        wild = pos[:M].clone()
        wild[0] = TLEN + 1000
        clamped = pos[:M].clone()
        clamped[0] = TLEN - 1
        if M > 1:
            wild[M - 1], clamped[M - 1] = -5, 0
        check_bits(launch(ops, epi, width, a[:M], w, None, wild, tdev), launch(ops, epi, width, a[:M], w, None, clamped, tdev),
                   "skinny[rope] positions outside the table are clamped to its ends")


# =====================================================================================================================
# refusals
# =====================================================================================================================
def test_refusals_return_their_code_and_leave_the_outputs_alone(lib, table):
    L = lib.load()
    UNS, ARG = 2, 1
    tdev = table.to(DEV)
    a = torch.zeros((80, 136), dtype=BF, device=DEV)
    w = torch.zeros((256, 136), dtype=BF, device=DEV)
    c = torch.full((80, 264), SENTINEL, dtype=BF, device=DEV)
    act = torch.full((80, 136), SENTINEL, dtype=BF, device=DEV)
    af = torch.zeros((8, 128), dtype=torch.float32, device=DEV)
    pos = torch.zeros(80, dtype=torch.int32, device=DEV)
    P = lambda t, off=0: t.data_ptr() + off   # noqa: E731

    def plain(M=8, N=128, K=128, A=P(a), lda=136, W=P(w), ldw=136, C=P(c), ldc=264, R=None, dtype=lib.SSI_BF16):
        return L.ssi_gemm_skinny(M, N, K, A, lda, W, ldw, C, ldc, R, dtype, None)

    def rope(M=8, N=128, K=128, A=P(a), lda=136, W=P(w), ldw=136, C=P(c), ldc=264, heads=1, hd=64, T=P(tdev), tl=TLEN, pp=P(pos), dtype=lib.SSI_BF16):
        return L.ssi_gemm_skinny_rope(M, N, K, A, lda, W, ldw, C, ldc, heads, hd, T, tl, pp, dtype, None)

    def swiglu(M=8, inter=64, K=128, X=P(a), ldx=136, W=P(w), ldw=136, GU=P(c), ldgu=264, ACT=P(act), ldact=136, dtype=lib.SSI_BF16):
        return L.ssi_gemm_skinny_swiglu(M, inter, K, X, ldx, W, ldw, GU, ldgu, ACT, ldact, dtype, None)

    assert plain() == 0 and rope() == 0 and swiglu() == 0 and swiglu(GU=None, ldgu=0) == 0      # the base calls are valid
    torch.cuda.synchronize()
    c.fill_(SENTINEL)
    act.fill_(SENTINEL)
    for f in (plain, rope, swiglu):
        assert f(dtype=lib.SSI_F32) == UNS, f.__name__
        assert f(M=65) == UNS and f(M=-1) == UNS, f.__name__
        assert f(K=96) == UNS, f.__name__
        assert f(M=0) == 0, f.__name__
        assert f(W=None) == ARG and f(ldw=120) == ARG and f(ldw=132) == ARG and f(W=P(w, 2)) == ARG, f.__name__
    assert plain(N=96) == UNS and rope(N=96) == UNS and swiglu(inter=96) == UNS
    assert plain(A=None) == ARG and plain(C=None) == ARG and plain(lda=120) == ARG and plain(ldc=120) == ARG
    assert plain(lda=132) == ARG and plain(ldc=260) == ARG and plain(A=P(a, 2)) == ARG and plain(C=P(c, 4)) == ARG and plain(R=P(c, 6)) == ARG
    assert rope(hd=32) == UNS and rope(hd=128) == UNS and rope(heads=3) == UNS
    assert rope(T=None) == ARG and rope(pp=None) == ARG and rope(tl=0) == ARG and rope(A=None) == ARG and rope(C=P(c, 2)) == ARG
    assert swiglu(X=None) == ARG and swiglu(ACT=None) == ARG and swiglu(ldact=56) == ARG and swiglu(ldgu=120) == ARG and swiglu(ldx=100) == ARG
    assert swiglu(GU=P(c, 2)) == ARG and swiglu(ACT=P(act, 2)) == ARG
    assert L.ssi_gemm_skinny(8, 128, 128, P(af), 128, P(af), 128, P(af), 128, None, lib.SSI_F32, None) == UNS
    torch.cuda.synchronize()
    assert bool((c == SENTINEL).all()) and bool((act == SENTINEL).all()), "a refused call wrote to its output"
