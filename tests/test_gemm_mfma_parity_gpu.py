"""Parity of the bf16 MFMA GEMM (csrc/gemm_mfma.hip with its kernel files gemm_wg8.h and gemm_nt4.h, and its dispatcher in csrc/gemm_generic.hip) at every dispatch branch and K-loop edge:
the 8-wave and the persistent main loops in the NT, NN and TN operand forms, the four epilogues (plain, RoPE, SwiGLU forward / backward), both
split-K schemes with their reduction kernels, the batched form and both tile orders.

Every reference is computed on the CPU in float64 from the same seeded inputs and EVERY element is compared.  Three kinds of comparison:

  1. exact integers.  Operands are integer-valued bf16 (A in [-3, 3], B in [-5, 5]: a swapped or transposed operand shows), alpha is a power
     of two, previous C and R are small integers.  |a b| <= 15 and K <= 1664 keep every partial sum below 2^15 << 2^24, so every fp32
     operation of the kernel is exact in any order and the result is defined by the documented rounding points alone:
     p = bf16(alpha sum), then bf16(float(p) + C_prev + R) when either is present (split-K: the same after the slab sum).  Outputs reach
     several hundred, where bf16 keeps 2-4 integer steps apart: the rounding itself is under test.  Asserted bit for bit, no mask.
  2. gather probes.  One operand is 0/1 with a single 1 per row at k = pi(row), pi a seeded permutation of [0, K) continued periodically (every
     k, hence every residue mod 64, is hit); the other is randn bf16.  One product per output is non-zero, so the output must be the selected
     element of the other operand bit for bit: any k-mapping, swizzle or fragment-order defect shows on full-mantissa data.
  3. randn operands against float64 with a derived bound, evaluated at every element:
       0.5 ulp_bf16(ref)               for each rounding to storage (ulp = 2^(floor(log2 |ref|) - 7), taken at |ref| + the error the value
                                       arrives with: that differs only where this error can lift the value into the next binade), plus
       C_ACC K 2^-24 (|A| @ |B|)       for the fp32 accumulation: bf16 products are exact in fp32, a sum of K terms in ANY order is off by at most
                                       (K - 1) u sum|terms| with u = 2^-24 for correctly rounded adds (Higham, Accuracy and Stability of Numerical
                                       Algorithms, 4.2), plus 2^-24 |x| for each further fp32 add of the epilogue.
     C_ACC = 1 is that bound as it stands; 2 would allow one ulp per add (a truncating adder inside the MFMA).  The value in force and the
     measured worst ratios are stated at C_ACC below.  The half-ulp term dominates, so a partial sum rounded to bf16 anywhere before the epilogue
     (about half an ulp of extra error per rounding) misses the bound at once; integers below 256 cannot see that.

Which kernel a call lands on follows the dispatcher: the persistent kernel takes K % 128 == 0, K >= 256 unless IMPL_MFMA_WG8 is set, both
`accumulate` and a residual are given, or a leading dimension (for the fused SwiGLU forward also the distance from the gate rows to the up rows
of w13) exceeds its 32-bit offsets; split-K goes to the persistent kernel when every slice has
at least 6 K-steps.  `check` prints, for every comparison of kind 3, the largest error as a fraction of its bound; the module prints the worst per
family at its end (pytest -s)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
U32 = 2.0 ** -24
# C_ACC = 1 (Higham's any-order bound with correctly rounded adds) holds on the MI355X for every family.  Worst error/bound measured with it:
# plain 8-wave 0.9984, plain persistent 0.9849, split-K 8-wave 0.9722, split-K persistent 0.9545, batched 0.9894, SwiGLU forward 0.9976,
# SwiGLU backward 0.9975, RoPE 0.9891 (the rotation alone, applied to exact integer products: 1.0000 to four digits), generic kernel 0.9880.
# The ratios sit just under 1 because the half-ulp term dominates and some of the 10^5..10^7 elements of a case always land next to a tie.
C_ACC = 1
SENTINEL = -7.25                    # exact in bf16; no case below can produce it (integers and halves of integers, or randn data)
NT, NN, TN = 0, 1, 2
LAYOUTS = [NT, NN, TN]
LNAME = {NT: "NT", NN: "NN", TN: "TN"}
FAMILIES = ["plain 8-wave", "plain persistent", "split-K 8-wave", "split-K persistent", "batched", "SwiGLU forward", "SwiGLU backward", "RoPE"]

_WORST: dict[str, float] = {}
_REFS: dict[tuple, tuple] = {}


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from ssi import _lib
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam in FAMILIES + sorted(set(_WORST) - set(FAMILIES)):
        if fam in _WORST:
            print(f"\ngemm-parity worst error/bound (C_ACC = {C_ACC})  {fam:<20s} {_WORST[fam]:.4f}", end="")
    print()


class impl:
    """with impl(ops, lib.IMPL_MFMA): ... — the previous implementation is always restored."""
    def __init__(self, ops, which):
        self.ops, self.which = ops, which

    def __enter__(self):
        self.prev = self.ops.set_impl(self.which)

    def __exit__(self, *exc):
        self.ops.set_impl(self.prev)


class tile_order:
    def __init__(self, ops, dynamic):
        self.ops, self.dynamic = ops, dynamic

    def __enter__(self):
        self.ops.set_gemm_tile_order(self.dynamic)

    def __exit__(self, *exc):
        self.ops.set_gemm_tile_order(False)


# =====================================================================================================================
# inputs, references, bounds
# =====================================================================================================================
def ints(shape, lim, seed):
    return torch.randint(-lim, lim + 1, shape, generator=torch.Generator().manual_seed(seed)).to(BF)


def rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(BF)


def operands(M, N, K, integer, seed):
    """(A [M, K], B [K, N], A @ B, |A| @ |B|) in the logical orientation; cached, never modified."""
    key = (M, N, K, integer, seed)
    if key not in _REFS:
        A, B = (ints((M, K), 3, seed), ints((K, N), 5, seed + 1)) if integer else (rnd((M, K), seed), rnd((K, N), seed + 1))
        S = A.double() @ B.double()
        _REFS[key] = (A, B, S, None if integer else A.double().abs() @ B.double().abs())
    return _REFS[key]


def phys(layout, A, B):
    """What ops.gemm takes for C = A @ B in each layout: NT (A, B^T), NN (A, B), TN (A^T, B)."""
    return (A.t().contiguous() if layout == TN else A), (B.t().contiguous() if layout == NT else B)


def window(t, pad, off=8, fill=SENTINEL):
    """t as a column window of a buffer `pad` columns wider, starting `off` elements (16 bytes at 8) into every row; returns (buffer, view)."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype)
    buf[:, off:off + t.shape[1]] = t
    buf = buf.to(DEV)
    return buf, buf[:, off:off + t.shape[1]]


def ulp_bf16(ref):
    _, e = torch.frexp(ref.abs())
    e = torch.where(ref == 0, torch.full_like(e, -1000), e)
    return torch.ldexp(torch.ones_like(ref), (e - 1).clamp(min=-126) - 7)


def r16(v64):
    """Round an fp32-exact float64 value to bf16 (round to nearest even) and return it as float64."""
    return v64.float().to(BF).double()


def acc_bound(absS, K):
    return C_ACC * K * U32 * absS


def half_ulp(ref, carried):
    """The rounding to bf16 of a value that is at most `carried` away from ref: half the spacing at |ref| + carried (the next binade's where
    the error carried in can lift the value over a power of two; 0.5 ulp_bf16(ref) everywhere else)."""
    return 0.5 * ulp_bf16(ref.abs() + carried)


def rounded(ref, carried):
    return carried + half_ulp(ref, carried)


def check(family, got, ref, bound, what):
    """|got - ref| <= bound at EVERY element (NaN/inf fail); names the worst element; records the largest error/bound of the family."""
    got64 = got.detach().cpu().double()
    assert got64.shape == ref.shape, f"{what}: shape {tuple(got64.shape)} vs {tuple(ref.shape)}"
    err = (got64 - ref).abs()
    bound = bound.expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ok = err <= bound
    if bool(ok.all()):
        worst = float(ratio.max()) if ratio.numel() else 0.0
        _WORST[family] = max(_WORST.get(family, 0.0), worst)
        print(f"{what}: max err/bound {worst:.4f}")
        return
    bad = (~ok).nonzero()
    fin = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, -1.0))
    w = tuple(int(v) for v in (fin == fin.max()).nonzero()[0])
    raise AssertionError(f"{what}: {bad.shape[0]} of {err.numel()} elements miss their bound; worst at {w}: got {float(got64[w])!r} ref "
                         f"{float(ref[w])!r} err {float(err[w]):.3e} bound {float(bound[w]):.3e} (ratio {float(ratio[w]):.3f}); "
                         f"first at {tuple(int(v) for v in bad[0])}")


def check_bits(got, ref, what):
    """Bit equality of every bf16 element (ref: float64 holding bf16 values, or a bf16 tensor); names the worst element."""
    got = got.detach().cpu()
    ref16 = ref.to(BF) if ref.dtype != BF else ref.detach().cpu()
    assert got.dtype == BF and got.shape == ref16.shape, f"{what}: {got.dtype} {tuple(got.shape)} vs {tuple(ref16.shape)}"
    if torch.equal(got.contiguous().view(torch.int16), ref16.contiguous().view(torch.int16)):
        return
    g, r = got.double(), ref16.double()
    ne = got.contiguous().view(torch.int16) != ref16.contiguous().view(torch.int16)
    bad = ne.nonzero()
    err = torch.where(ne, (g - r).abs().nan_to_num(nan=float("inf")), torch.zeros_like(g))
    w = tuple(int(v) for v in (err == err.max()).nonzero()[0])
    rows, cols = sorted({int(v) for v in bad[:, -2]}), sorted({int(v) for v in bad[:, -1]})
    raise AssertionError(f"{what}: {bad.shape[0]} of {ne.numel()} elements differ; worst at {w}: got {float(g[w])!r} ref {float(r[w])!r}; "
                         f"first at {tuple(int(v) for v in bad[0])}; rows {rows[:6]}.. ({len(rows)}), columns {cols[:6]}.. ({len(cols)})")


def untouched(buf, keep, what):
    """Every element of the wider buffer outside the window(s) still holds the sentinel, bit for bit."""
    out = buf.detach().cpu()
    mask = torch.ones(out.shape, dtype=torch.bool)
    for rows, cols in keep:
        mask[rows, cols] = False
    assert bool((out[mask] == SENTINEL).all()), f"{what}: {int((out[mask] != SENTINEL).sum())} elements outside the window were written"


# epilogue forms: (accumulate, residual, alpha, alpha_dev); alpha * alpha_dev = 1/2 makes half of the products need rounding below 256 already
FORMS = {"plain": (False, False, 1.0, None), "acc": (True, False, 1.0, None), "res": (False, True, 1.0, None),
         "accres": (True, True, 1.0, None), "alpha": (False, False, 0.25, 2.0), "alpha_acc": (True, False, 2.0, 0.25)}
ALL_FORMS = ["plain", "acc", "res", "accres", "alpha"]


def run_forms(family, what, call, layout, M, N, K, integer, forms, seed, ldc_pad=8, a_pad=0, b_pad=0):
    """call(layout, a, b, c, **kw) on every epilogue form; C and R are windows of buffers ldc_pad wider, A and B windows when a_pad / b_pad."""
    A, B, S, absS = operands(M, N, K, integer, seed)
    a, b = phys(layout, A, B)
    (abuf, a), (bbuf, b) = (window(a, a_pad) if a_pad else (None, a.to(DEV))), (window(b, b_pad) if b_pad else (None, b.to(DEV)))
    c0, r0 = (ints((M, N), 4, seed + 2), ints((M, N), 6, seed + 3)) if integer else (rnd((M, N), seed + 2), rnd((M, N), seed + 3))
    outs = {}
    for form in forms:
        acc, res, alpha, adev = FORMS[form]
        al = alpha * (adev if adev is not None else 1.0)
        cbuf, c = window(c0 if acc else torch.full((M, N), SENTINEL, dtype=BF), ldc_pad)
        rbuf, r = window(r0, ldc_pad) if res else (None, None)
        kw = dict(alpha=alpha, accumulate=acc)
        if adev is not None:
            kw["alpha_dev"] = torch.tensor([adev], device=DEV)
        if res:
            kw["residual"] = r
        call(layout, a, b, c, **kw)
        tag = f"{what}[{LNAME[layout]},{M}x{N}x{K},{form},{'int' if integer else 'rand'}]"
        prev = (c0.double() if acc else 0.0) + (r0.double() if res else 0.0)
        p = al * S
        if integer:
            ref = r16(p)
            if acc or res:
                ref = r16(ref + prev)
            check_bits(c, ref, tag)
        elif acc or res:
            # p is rounded to bf16 (0.5 ulp at p), widened, added to C_prev and R in fp32 (one rounding per add, each of a value no larger
            # than |p| + |C_prev| + |R| in magnitude), and the sum is rounded to storage (0.5 ulp at the result)
            mag = p.abs() + (c0.double().abs() if acc else 0.0) + (r0.double().abs() if res else 0.0)
            ref = p + prev
            check(family, c, ref, rounded(ref, rounded(p, abs(al) * acc_bound(absS, K)) + (int(acc) + int(res)) * U32 * mag), tag)
        else:
            check(family, c, p, rounded(p, abs(al) * acc_bound(absS, K)), tag)
        untouched(cbuf, [(slice(None), slice(8, 8 + N))], tag)
        if res:
            assert torch.equal(rbuf.cpu()[:, 8:8 + N], r0), f"{tag}: the residual was modified"
        outs[form] = c.clone()
    for buf, t, pad in ((abuf, phys(layout, A, B)[0], a_pad), (bbuf, phys(layout, A, B)[1], b_pad)):
        if buf is not None:
            assert torch.equal(buf.cpu()[:, 8:8 + t.shape[1]], t), f"{what}: an input operand was modified"
    return outs


def pi_map(n, K, seed):
    """k = pi(i) for i in [0, n): a seeded permutation of [0, K) repeated with a fresh shuffle per period; n >= K, so every k is hit."""
    assert n >= K
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.randperm(K, generator=g) for _ in range(-(-n // K))])[:n]


def gather_probes(what, call, layout, K, seed, mn=256, ldc_pad=8):
    """A one-hot against randn B: C[m, n] == B[pi(m), n]; then B one-hot against randn A: C[m, n] == A[m, pi(n)].  The one-hot side has
    ceil(K / 256) * 256 rows (columns) so that pi covers [0, K) in one launch."""
    big = -(-K // 256) * 256
    for side in ("A", "B"):
        M, N = (big, mn) if side == "A" else (mn, big)
        if side == "A":
            pi = pi_map(M, K, seed)
            A = torch.zeros(M, K, dtype=BF)
            A[torch.arange(M), pi] = 1
            B = rnd((K, N), seed + 1)
            ref = B[pi, :]
        else:
            pi = pi_map(N, K, seed + 2)
            B = torch.zeros(K, N, dtype=BF)
            B[pi, torch.arange(N)] = 1
            A = rnd((M, K), seed + 3)
            ref = A[:, pi]
        assert set(pi.tolist()) == set(range(K)) and {k % 64 for k in pi.tolist()} == set(range(64))
        a, b = phys(layout, A, B)
        cbuf, c = window(torch.full((M, N), SENTINEL, dtype=BF), ldc_pad)
        call(layout, a.to(DEV), b.to(DEV), c)
        check_bits(c, ref, f"{what}[{LNAME[layout]},K={K}] gather probe, {side} one-hot")


# =====================================================================================================================
# A. ops.gemm: K edges of both main loops, every epilogue form
# =====================================================================================================================
K_8WAVE = [64, 128, 192, 320]     # K/64 = 1 (no second stage) | 2 (no stage(kt + 2)) | 3 (first buffer reuse) | 5 (odd, longer); TN: register-staged loop
K_PERSISTENT = [256, 384, 640]    # 4, 6, 10 K-steps: the fetch stream runs two steps ahead and crosses the unit boundary


@pytest.mark.parametrize("K", K_8WAVE + K_PERSISTENT)
@pytest.mark.parametrize("layout", LAYOUTS, ids=LNAME.get)
def test_gemm_k_edges_every_epilogue_form(ops, lib, layout, K):
    """IMPL_MFMA: the 8-wave kernel at K % 128 != 0 or K < 256 and for `accres` (accumulate and residual together) at every K, the persistent
    kernel otherwise.  Integers exact, randn within the bound, gather probes exact."""
    fam = "plain persistent" if K in K_PERSISTENT else "plain 8-wave"
    with impl(ops, lib.IMPL_MFMA):
        run_forms(fam, "gemm", ops.gemm, layout, 256, 256, K, True, ALL_FORMS + ["alpha_acc"], seed=1000 + K)
        run_forms(fam, "gemm", ops.gemm, layout, 256, 256, K, False, ["plain", "acc", "res", "alpha"], seed=2000 + K)
        run_forms("plain 8-wave", "gemm", ops.gemm, layout, 256, 256, K, False, ["accres"], seed=2000 + K)
        gather_probes("gemm", ops.gemm, layout, K, seed=3000 + K)


@pytest.mark.parametrize("K", K_PERSISTENT)
@pytest.mark.parametrize("layout", LAYOUTS, ids=LNAME.get)
def test_gemm_8wave_kernel_at_the_persistent_k_and_same_bits_as_the_persistent_kernel(ops, lib, layout, K):
    """IMPL_MFMA_WG8 runs the 8-wave kernel at the K the persistent kernel would take: exact, within the bound, and on randn operands the two
    kernels agree bit for bit in every epilogue form (same accumulation order per output element)."""
    with impl(ops, lib.IMPL_MFMA_WG8):
        run_forms("plain 8-wave", "gemm/wg8", ops.gemm, layout, 256, 256, K, True, ALL_FORMS, seed=1000 + K)
        w8 = run_forms("plain 8-wave", "gemm/wg8", ops.gemm, layout, 256, 256, K, False, ALL_FORMS, seed=2000 + K)
        gather_probes("gemm/wg8", ops.gemm, layout, K, seed=3000 + K)
    with impl(ops, lib.IMPL_MFMA):
        w4 = run_forms("plain persistent", "gemm", ops.gemm, layout, 256, 256, K, False, ["plain", "acc", "res", "alpha"], seed=2000 + K)
    for form in w4:
        check_bits(w4[form], w8[form], f"IMPL_MFMA against IMPL_MFMA_WG8 [{LNAME[layout]},K={K},{form}]")


# ---- tile walking -----------------------------------------------------------------------------------------------------
GUARD = 3 * 256   # sentinel rows (TN: columns of A) behind the last tile row: a tile map that leaves the grid is caught, not a fault


def tile_grids(n_cu):
    """(tiles_m, tiles_n) by name.  Fewer tiles than CUs: the grid equals the tile count and G & 7 != 0 (1, 6, 9, 10, 18); tiles_m of 5, 6, 13, 18
    leave the last group of tile_from_t / tile_coords partial (GM = 4); exactly n_cu; between one and two tiles per workgroup; more than two
    (the dynamic order first uses its counters, the static order takes a third round) — the last two not multiples of 8."""
    def pick(lo, hi, tm):
        return next((tm, tn) for tn in range(lo // tm + 1, hi // tm + 1) if (tm * tn) % 8)
    return {"1": (1, 1), "6": (6, 1), "9": (3, 3), "10": (5, 2), "18": (6, 3),
            "n_cu": next((t, n_cu // t) for t in (16, 8, 4, 2, 1) if n_cu % t == 0),
            "between": pick(n_cu + n_cu // 4, 2 * n_cu, 13), "above": pick(2 * n_cu, 2 * n_cu + 72, 18)}


def tile_walk_ref(M, N):
    key = ("walk", M, N)
    if key not in _REFS:
        A, B = ints((M, 256), 3, 41), ints((256, N), 5, 42)
        _REFS[key] = (A, B, r16(A.double() @ B.double()).to(BF))
    return _REFS[key]


@pytest.mark.parametrize("layout", LAYOUTS, ids=LNAME.get)
@pytest.mark.parametrize("grid", ["1", "6", "9", "10", "18", "n_cu", "between", "above"])
def test_gemm_tile_walk_static_and_dynamic_order(ops, lib, grid, layout):
    """K = 256, integers: every tile of the grid is written exactly (an unwritten tile keeps the sentinel, a tile written from the wrong panel
    differs), in the static and the dynamic order of the persistent kernel and, for grids up to n_cu, on the 8-wave kernel."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    tiles_m, tiles_n = tile_grids(n_cu)[grid]
    count = tiles_m * tiles_n
    if grid in ("between", "above"):
        assert count % 8 and (n_cu < count <= 2 * n_cu if grid == "between" else count > 2 * n_cu), (grid, count, n_cu)
    else:
        assert count == n_cu if grid == "n_cu" else count < n_cu, (grid, count, n_cu)
    M, N = tiles_m * 256, tiles_n * 256
    A, B, ref = tile_walk_ref(M, N)
    a, b = phys(layout, A, B)
    # guard band: GUARD more rows of A (NT, NN) or columns of A (TN) and of C, all sentinels
    if layout == TN:
        abuf = torch.full((256, M + GUARD), SENTINEL, dtype=BF)
        abuf[:, :M] = a
        a_dev = abuf.to(DEV)[:, :M]
    else:
        abuf = torch.full((M + GUARD, 256), SENTINEL, dtype=BF)
        abuf[:M] = a
        a_dev = abuf.to(DEV)[:M]
    b_dev, ref_dev = b.to(DEV), ref.to(DEV)
    runs = [("static", lib.IMPL_MFMA, False), ("dynamic", lib.IMPL_MFMA, True)] + ([("8-wave", lib.IMPL_MFMA_WG8, False)] if count <= n_cu else [])
    for name, which, dyn in runs:
        cbuf = torch.full((M + GUARD, N), SENTINEL, dtype=BF, device=DEV)
        with impl(ops, which), tile_order(ops, dyn):
            ops.gemm(layout, a_dev, b_dev, cbuf[:M])
        tag = f"tile walk [{LNAME[layout]},{tiles_m}x{tiles_n} tiles,{name}]"
        if not torch.equal(cbuf[:M].view(torch.int16), ref_dev.view(torch.int16)):
            ne = (cbuf[:M].view(torch.int16) != ref_dev.view(torch.int16)).view(tiles_m, 256, tiles_n, 256).any(3).any(1)
            check_bits(cbuf[:M], ref, f"{tag}: wrong tiles (tm, tn) {[tuple(t) for t in ne.nonzero().tolist()][:12]}")
        assert bool((cbuf[M:] == SENTINEL).all()), f"{tag}: rows behind the last tile row were written"


# =====================================================================================================================
# B. leading dimensions and windows
# =====================================================================================================================
@pytest.mark.parametrize("pad", [8, 264])
@pytest.mark.parametrize("K", [192, 256])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LNAME.get)
def test_gemm_on_column_windows_of_wider_buffers(ops, lib, layout, K, pad):
    """A, B, C and R start 16 bytes into rows `pad` elements longer than they are wide; K = 192 is the 8-wave kernel, K = 256 the persistent one
    (and the 8-wave kernel again under IMPL_MFMA_WG8).  Exact on integers; everything outside C's window keeps the sentinel."""
    for which, fam in ((lib.IMPL_MFMA, "plain persistent" if K == 256 else "plain 8-wave"), (lib.IMPL_MFMA_WG8, "plain 8-wave")):
        with impl(ops, which):
            run_forms(fam, f"gemm/window+{pad}", ops.gemm, layout, 256, 256, K, True, ["plain", "acc", "res", "accres"], seed=50 + K,
                      ldc_pad=pad, a_pad=pad, b_pad=pad)
            run_forms(fam, f"gemm/window+{pad}", ops.gemm, layout, 256, 256, K, False, ["res"], seed=60 + K, ldc_pad=pad, a_pad=pad, b_pad=pad)


@pytest.mark.parametrize("how", ["offset 8 bytes", "ld % 8 != 0"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LNAME.get)
def test_gemm_misaligned_window_takes_the_generic_kernel_or_raises(ops, lib, layout, how):
    """The generic kernel keeps one fp32 fma chain per element in k order and rounds once: exact on integers, and on randn within
    K 2^-24 (|A| @ |B|) + 0.5 ulp.  Forced IMPL_MFMA must refuse."""
    M = N = 256
    K = 192
    off, pad = (4, 8) if how == "offset 8 bytes" else (8, 12)
    for integer in (True, False):
        A, B, S, absS = operands(M, N, K, integer, 70 + int(integer))
        a, b = phys(layout, A, B)
        _, a_dev = window(a, pad, off)
        cbuf, c = window(torch.full((M, N), SENTINEL, dtype=BF), 8)
        assert a_dev.data_ptr() % 16 != 0 or a_dev.stride(0) % 8 != 0
        ops.gemm(layout, a_dev, b.to(DEV), c)
        tag = f"gemm/generic[{LNAME[layout]},{how},{'int' if integer else 'rand'}]"
        if integer:
            check_bits(c, r16(S), tag)
        else:
            check("generic (misaligned)", c, S, rounded(S, K * U32 * absS), tag)
        untouched(cbuf, [(slice(None), slice(8, 8 + N))], tag)
        with impl(ops, lib.IMPL_MFMA), pytest.raises(RuntimeError):
            ops.gemm(layout, a_dev, b.to(DEV), c)


def test_gemm_nt_leading_dimension_beyond_the_32_bit_offsets_takes_the_8wave_kernel(ops, lib):
    """NT, 256 x 256 x 256, A the first 256 columns of an uninitialised [256, 2^22] buffer (2 GiB; 256 rows of it span the 2^31 bytes a buffer
    offset can hold, nt4_ld_ok is false): only the window is written, the result is exact."""
    M = N = K = 256
    A, B, S, _ = operands(M, N, K, True, 80)
    big = torch.empty(M, 2 ** 22, dtype=BF, device=DEV)
    a = big[:, :K]
    a.copy_(A)
    cbuf, c = window(torch.full((M, N), SENTINEL, dtype=BF), 8)
    with impl(ops, lib.IMPL_MFMA):
        ops.gemm(NT, a, B.t().contiguous().to(DEV), c)
    check_bits(c, r16(S), "gemm[NT, lda = 2^22]")
    untouched(cbuf, [(slice(None), slice(8, 8 + N))], "gemm[NT, lda = 2^22]")
    del big


@pytest.mark.parametrize("inter,ldw", [(256, 2 ** 22), (512, 2 ** 21)], ids=["tile-rows", "up-rows"])
def test_gemm_swiglu_forward_w13_beyond_the_32_bit_offsets_takes_the_8wave_kernel(ops, lib, inter, ldw):
    """gemm_swiglu_fwd, M = K = 256, w13 the first 256 columns of an uninitialised [2 inter, ldw] buffer (4 GiB), the smallest shapes at which
    each of the two limits of the persistent kernel's 32-bit loader offsets is passed: at (256, 2^22) 256 rows span 2^31 bytes (nt4_ld_ok is
    false); at (512, 2^21) they do not, but the up rows' distance (inter + 128) ldw 2 = 2.7e9 >= 2^31.  Only the window is written; gu is exact
    on integers and act equals ops.swiglu_fwd(gu) bit for bit.  The dispatch rule (nt4_takes in csrc/gemm_mfma.hip) sends both to the 8-wave
    kernel, which addresses with 64 bits.  Before that rule existed this entry checked neither limit and the persistent kernel's offsets
    wrapped: these cases are not to be run on a checkout older than the rule."""
    M = K = 256
    X, W, S, _ = operands(M, 2 * inter, K, True, 90 + inter)
    big = torch.empty(2 * inter, ldw, dtype=BF, device=DEV)
    w13 = big[:, :K]
    w13.copy_(W.t())
    assert 256 * ldw * 2 >= 2 ** 31 or (inter + 128) * ldw * 2 >= 2 ** 31
    gu = torch.full((M, 2 * inter), SENTINEL, dtype=BF, device=DEV)
    act = torch.full((M, inter), SENTINEL, dtype=BF, device=DEV)
    with impl(ops, lib.IMPL_MFMA):
        ops.gemm_swiglu_fwd(X.to(DEV), w13, gu, act)
    tag = f"gemm_swiglu_fwd[inter = {inter}, ldw = {ldw}]"
    check_bits(gu, r16(S), tag + " gu")
    act_ref = torch.full_like(act, SENTINEL)
    ops.swiglu_fwd(gu, act_ref)
    check_bits(act, act_ref, tag + " act against ops.swiglu_fwd(gu)")
    del big


# =====================================================================================================================
# C. ops.gemm_splitk
# =====================================================================================================================
# (K / 64, splits, K-steps per slice, scheme)
SPLITK_CASES = [(7, 3, [2, 2, 3], "8-wave"), (7, 7, [1] * 7, "8-wave"), (16, 3, [5, 5, 6], "8-wave"), (16, 8, [2] * 8, "8-wave"),
                (12, 2, [6, 6], "persistent"), (20, 3, [6, 6, 8], "persistent"), (26, 4, [6, 6, 6, 8], "persistent")]


def slice_table(nk, splits, scheme):
    """[k_lo, k_hi) in K-steps per slice, by the formulas of the kernels: the 8-wave kernel cuts at floor(s nk / splits); the persistent kernel
    rounds those cuts down to even and ends the last slice at nk."""
    if scheme == "8-wave":
        return [(s * nk // splits, (s + 1) * nk // splits) for s in range(splits)]
    return [((nk * s // splits) & ~1, nk if s + 1 == splits else (nk * (s + 1) // splits) & ~1) for s in range(splits)]


def persistent_splitk_takes(nk, splits):
    return nk % 2 == 0 and nk >= 4 and nk // splits >= 6


@pytest.mark.parametrize("M,N", [(256, 256), (768, 512)], ids=["256x256", "768x512"])
@pytest.mark.parametrize("nk,splits,steps,scheme", SPLITK_CASES, ids=[f"{c[0]}steps/{c[1]}" for c in SPLITK_CASES])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LNAME.get)
def test_gemm_splitk_every_slice_shape_and_reduction_form(ops, lib, layout, nk, splits, steps, scheme, M, N):
    table = slice_table(nk, splits, scheme)
    assert table[0][0] == 0 and table[-1][1] == nk and all(table[i][1] == table[i + 1][0] for i in range(splits - 1)), table
    assert [hi - lo for lo, hi in table] == steps, table
    assert persistent_splitk_takes(nk, splits) == (scheme == "persistent")
    assert scheme == "8-wave" or all(lo % 2 == 0 and hi - lo >= 6 for lo, hi in table)
    K = nk * 64
    ws = torch.empty(splits * M * N, dtype=torch.float32, device=DEV)

    def call(layout, a, b, c, **kw):
        if ws.numel() < splits * c.shape[0] * c.shape[1]:   # the gather probes' one-hot side is taller
            return ops.gemm_splitk(layout, a, b, c, splits, torch.empty(splits * c.shape[0] * c.shape[1], dtype=torch.float32, device=DEV), **kw)
        ws.fill_(float("nan"))
        return ops.gemm_splitk(layout, a, b, c, splits, ws, **kw)

    fam = f"split-K {scheme}"
    with impl(ops, lib.IMPL_MFMA):
        run_forms(fam, f"splitk/{splits}", call, layout, M, N, K, True, ["plain", "acc", "res", "alpha", "alpha_acc"], seed=100 + nk, ldc_pad=24)
        run_forms(fam, f"splitk/{splits}", call, layout, M, N, K, False, ["plain", "acc", "res", "alpha"], seed=200 + nk, ldc_pad=24)
        # accumulate and residual together: the persistent scheme declines, the 8-wave scheme's reduction adds both
        run_forms("split-K 8-wave", f"splitk/{splits}", call, layout, M, N, K, True, ["accres"], seed=100 + nk, ldc_pad=24)
        run_forms("split-K 8-wave", f"splitk/{splits}", call, layout, M, N, K, False, ["accres"], seed=200 + nk, ldc_pad=24)
        if (M, N) == (256, 256):
            gather_probes(f"splitk/{splits}", call, layout, K, seed=300 + nk, ldc_pad=24)


@pytest.mark.parametrize("layout", LAYOUTS, ids=LNAME.get)
def test_gemm_splitk_with_more_splits_than_k_steps_forwards_to_gemm(ops, lib, layout):
    ws = torch.empty(3 * 256 * 256, dtype=torch.float32, device=DEV)
    with impl(ops, lib.IMPL_MFMA):
        run_forms("plain 8-wave", "splitk/3 of 2 steps", lambda lo, a, b, c, **kw: ops.gemm_splitk(lo, a, b, c, 3, ws, **kw), layout, 256, 256, 128,
                  True, ALL_FORMS, seed=400)


# =====================================================================================================================
# D. ops.gemm_batched (TN)
# =====================================================================================================================
def test_gemm_batched_more_units_than_cus_into_a_strided_view(ops, lib):
    """33 problems of 512 x 1024 at K = 256: 264 tiles, more than the CUs whenever n_cu < 264 and never a multiple of n_cu.  C is a strided view
    of a flat sentinel-filled buffer with a gap after every problem."""
    nb, M, N, K, gap = 33, 512, 1024, 256, 1032
    stride = M * N + gap
    for integer in (True, False):
        A = ints((nb, K, M), 3, 90) if integer else rnd((nb, K, M), 92)
        B = ints((nb, K, N), 5, 91) if integer else rnd((nb, K, N), 93)
        S = torch.bmm(A.double().transpose(1, 2), B.double())
        a, b = A.to(DEV), B.to(DEV)
        flat = torch.full((nb * stride,), SENTINEL, dtype=BF, device=DEV)
        c = flat.as_strided((nb, M, N), (stride, N, 1))
        with impl(ops, lib.IMPL_MFMA):
            ops.gemm_batched(TN, a, b, c)
            one = torch.full((nb, M, N), SENTINEL, dtype=BF, device=DEV)
            for i in range(nb):
                ops.gemm(TN, a[i], b[i], one[i])
        tag = f"gemm_batched[{'int' if integer else 'rand'}]"
        if integer:
            check_bits(c, r16(S), tag)
        else:
            check("batched", c, S, rounded(S, acc_bound(torch.bmm(A.double().abs().transpose(1, 2), B.double().abs()), K)), tag)
        check_bits(c, one, tag + " against one ops.gemm per problem")
        gaps = flat.view(nb, stride)[:, M * N:]
        assert bool((gaps == SENTINEL).all()), f"{tag}: the gaps between the problems' outputs were written"


# =====================================================================================================================
# E. fused SwiGLU
# =====================================================================================================================
SWIGLU_K = [64, 128, 192, 320, 256, 384]   # the 8-wave fused kernels at the first four, the persistent kernel at the last two


@pytest.mark.parametrize("M", [256, 512])
@pytest.mark.parametrize("inter", [256, 768])
@pytest.mark.parametrize("K", SWIGLU_K)
def test_gemm_swiglu_forward(ops, lib, K, inter, M):
    """gu = x @ w13^T is exact on integers and within the bound on randn; act equals ops.swiglu_fwd(gu) bit for bit (that kernel is pinned to
    float64 in test_row_kernels_gpu.py); x and w13 as windows of wider buffers give the same bits."""
    for integer in (True, False):
        X, W, S, absS = operands(M, 2 * inter, K, integer, 500 + K + int(integer))
        w13 = W.t().contiguous()
        tag = f"gemm_swiglu_fwd[{M}x{inter}x{K},{'int' if integer else 'rand'}]"
        outs = []
        for pad in (0, 40):
            x_dev, w_dev = (window(X, pad)[1], window(w13, pad + 16)[1]) if pad else (X.to(DEV), w13.to(DEV))
            gu = torch.full((M, 2 * inter), SENTINEL, dtype=BF, device=DEV)
            act = torch.full((M, inter), SENTINEL, dtype=BF, device=DEV)
            with impl(ops, lib.IMPL_MFMA):
                ops.gemm_swiglu_fwd(x_dev, w_dev, gu, act)
            outs.append((gu, act))
        gu, act = outs[0]
        if integer:
            check_bits(gu, r16(S), tag + " gu")
        else:
            check("SwiGLU forward", gu, S, rounded(S, acc_bound(absS, K)), tag + " gu")
        act_ref = torch.full_like(act, SENTINEL)
        ops.swiglu_fwd(gu, act_ref)
        check_bits(act, act_ref, tag + " act against ops.swiglu_fwd(gu)")
        check_bits(outs[1][0], gu, tag + " gu from windows")
        check_bits(outs[1][1], act, tag + " act from windows")


def _swiglu_bwd_case(ops, lib, which, layout, M, inter, K, tag, dact_ws=None):
    DY, W2, S, absS = operands(M, inter, K, False, 600 + K)
    dy, w2 = phys(layout, DY, W2)
    dy, w2 = dy.to(DEV), w2.to(DEV)
    gu = (rnd((M, 2 * inter), 610 + K) * 2).to(BF).to(DEV)
    with impl(ops, which):
        dact = torch.full((M, inter), SENTINEL, dtype=BF, device=DEV)
        ops.gemm(layout, dy, w2, dact)
        dgu = torch.full((M, 2 * inter), SENTINEL, dtype=BF, device=DEV)
        ops.gemm_swiglu_bwd(layout, dy, w2, gu, dgu, dact_ws)
    check("SwiGLU backward", dact, S, rounded(S, acc_bound(absS, K)), tag + " d_act (plain ops.gemm of the same operands)")
    ref = torch.full_like(dgu, SENTINEL)
    ops.swiglu_bwd(dact, gu, ref)
    check_bits(dgu, ref, tag + " dgu against ops.swiglu_bwd(d_act, gu)")


@pytest.mark.parametrize("M,inter", [(256, 256), (512, 768)], ids=["256x256", "512x768"])
@pytest.mark.parametrize("K", SWIGLU_K)
def test_gemm_swiglu_backward_nt(ops, lib, K, M, inter):
    """The 8-wave fused kernel at K it alone takes, the persistent kernel at 256 and 384 and the 8-wave kernel there too (IMPL_MFMA_WG8)."""
    _swiglu_bwd_case(ops, lib, lib.IMPL_MFMA, NT, M, inter, K, f"gemm_swiglu_bwd[NT,{M}x{inter}x{K}]")
    if K in (256, 384):
        _swiglu_bwd_case(ops, lib, lib.IMPL_MFMA_WG8, NT, M, inter, K, f"gemm_swiglu_bwd[NT,{M}x{inter}x{K},wg8]")


@pytest.mark.parametrize("M,inter", [(256, 256), (512, 768)], ids=["256x256", "512x768"])
@pytest.mark.parametrize("K", [256, 384])
def test_gemm_swiglu_backward_nn_fused(ops, lib, K, M, inter):
    _swiglu_bwd_case(ops, lib, lib.IMPL_MFMA, NN, M, inter, K, f"gemm_swiglu_bwd[NN,{M}x{inter}x{K}]")


def test_gemm_swiglu_backward_nn_unfused_fallback_needs_its_workspace(ops, lib):
    """NN at K = 192 is not a shape of the persistent kernel: ops.gemm into dact_ws, then ops.swiglu_bwd; without dact_ws it is an error."""
    M, inter, K = 256, 256, 192
    ws = torch.full((M, inter), SENTINEL, dtype=BF, device=DEV)
    _swiglu_bwd_case(ops, lib, lib.IMPL_MFMA, NN, M, inter, K, "gemm_swiglu_bwd[NN,K=192,fallback]", dact_ws=ws)
    DY, W2, _, _ = operands(M, inter, K, False, 600 + K)
    gu = rnd((M, 2 * inter), 1).to(DEV)
    with pytest.raises(RuntimeError):
        ops.gemm_swiglu_bwd(NN, DY.to(DEV), W2.to(DEV), gu, torch.empty_like(gu), None)


# =====================================================================================================================
# F. ops.gemm_rope
# =====================================================================================================================
def _rope64(p, bp, table, pos, rot_cols):
    """Interleaved rotation of columns [0, rot_cols) of p (float64) in 64-wide heads; bp is the error bound p arrives with.  Each output is two
    fp32 products and their sum or difference (2^-24 of the magnitudes each), then ONE rounding to storage."""
    rows = p.shape[0]
    cs = table.double()[pos]
    c, s = cs[:, None, :, 0], cs[:, None, :, 1]
    v, bv = p[:, :rot_cols].reshape(rows, -1, 32, 2), bp[:, :rot_cols].reshape(rows, -1, 32, 2)
    x0, x1, b0, b1 = v[..., 0], v[..., 1], bv[..., 0], bv[..., 1]
    o = torch.stack([x0 * c - x1 * s, x1 * c + x0 * s], -1).reshape(rows, rot_cols)
    m0, m1 = x0.abs() + b0, x1.abs() + b1                                   # magnitudes of what the kernel really multiplies
    mag = torch.stack([m0 * c.abs() + m1 * s.abs(), m1 * c.abs() + m0 * s.abs()], -1).reshape(rows, rot_cols)
    carried = torch.stack([b0 * c.abs() + b1 * s.abs(), b1 * c.abs() + b0 * s.abs()], -1).reshape(rows, rot_cols)
    return o, rounded(o, carried + 2 * U32 * mag)


@pytest.mark.parametrize("explicit", [False, True], ids=["implicit", "explicit"])
@pytest.mark.parametrize("seq_len", [96, 256, 640])
@pytest.mark.parametrize("N,rot_cols", [(512, 512), (768, 256)], ids=["all 8 heads", "4 of 12 heads"])
@pytest.mark.parametrize("K", [256, 384, 192])
def test_gemm_rope(ops, lib, K, N, rot_cols, seq_len, explicit):
    """M = 768: sequences of 96 (several inside one tile), 256 and 640 rows (one spanning tiles).  Explicit positions restart inside a tile row
    and run past seq_len.  K = 192 is the unfused fallback.  C is a window of a wider sentinel-filled buffer."""
    from ssi.model import llama3_rope_table
    M, tlen = 768, 1024
    table = llama3_rope_table(64, tlen)
    if explicit:
        pos = (torch.arange(M) * 5 + 700) % 901                  # restarts at row 41 and every 181 rows after; up to 900 > seq_len
        pos_dev = pos.to(torch.int32).to(DEV)
    else:
        pos, pos_dev = torch.arange(M) % seq_len, None
    for integer in (True, False):
        A, B, S, absS = operands(M, N, K, integer, 700 + K + int(integer))
        a, b = A.to(DEV), B.t().contiguous().to(DEV)
        cbuf, c = window(torch.full((M, N), SENTINEL, dtype=BF), 72)
        with impl(ops, lib.IMPL_MFMA):
            ops.gemm_rope(a, b, c, seq_len, rot_cols // 64, 64, table.to(DEV), positions=pos_dev)
            two = torch.full((M, N), SENTINEL, dtype=BF, device=DEV)
            ops.gemm(NT, a, b, two)
            ops.rope_(two, seq_len, rot_cols // 64, 64, table.to(DEV), positions=pos_dev)
        tag = f"gemm_rope[{M}x{N}x{K},rot {rot_cols},seq {seq_len},{'explicit' if explicit else 'implicit'},{'int' if integer else 'rand'}]"
        check_bits(c, two, tag + " against ops.gemm then ops.rope_")
        untouched(cbuf, [(slice(None), slice(8, 8 + N))], tag)
        if integer:
            if rot_cols < N:
                check_bits(c[:, rot_cols:], r16(S)[:, rot_cols:], tag + " unrotated columns")
            ref, bound = _rope64(r16(S), torch.zeros_like(S), table, pos, rot_cols)   # the rotation alone, from the exact bf16 product
        else:
            bp = rounded(S, acc_bound(absS, K))
            ref, bound = _rope64(S, bp, table, pos, rot_cols)
            if rot_cols < N:
                check("RoPE", c[:, rot_cols:], S[:, rot_cols:], bp[:, rot_cols:], tag + " unrotated columns")
        check("RoPE" if not integer else "RoPE, rotation of the integer product", c[:, :rot_cols], ref, bound, tag + " rotated columns")
