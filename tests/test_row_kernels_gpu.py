"""Parity of the bandwidth-bound "row" kernels (csrc/elementwise.hip and the head of csrc/embed_ce.hip) at every dispatch branch and
row-loop edge: RMSNorm forward/backward, the dscale column sum, SwiGLU, RoPE, the embedding gather/scatter-add and transpose.

Every reference is float64 on the CPU from the same seeded inputs, with the storage-type roundings at the points the kernels document.
Every element is compared.  Nothing here is tuned: each bound is derived where it is asserted from

  * ulp(ref)   one unit in the last place of the storage type at |ref| for each rounding to storage between the fp32 math and the stored
               value (bf16: 2^(e-7), fp32: 2^(e-23), e = floor(log2 |ref|) held at -126 where the formats go subnormal);
  * U32 = 2^-24  the relative error of one correctly rounded fp32 operation; a sum whose longest chain of additions is n long is off by at
               most n U32 sum|terms| (Higham, Accuracy and Stability of Numerical Algorithms, 4.2: any summation order);
  * data movement and exact arithmetic are compared bit for bit.

`check` prints, for every comparison, the largest error as a fraction of its bound (pytest -s shows them per family at the end)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
MANT = {torch.bfloat16: 7, torch.float32: 23}   # stored mantissa bits
VEC = {torch.bfloat16: 8, torch.float32: 4}     # elements per 16-byte vector
U32 = 2.0 ** -24
TINY = 2.0 ** -126                              # smallest normal of fp32 and of bf16
EPS = 1e-5
SENTINEL = -7.25                                # exact in bf16; no kernel here produces it from the inputs below

_WORST: dict[str, float] = {}


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam in sorted(_WORST):
        print(f"\nrow-kernels worst error/bound  {fam:<28s} {_WORST[fam]:.4f}", end="")
    print()


def rnd(*shape, dtype=torch.float32, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def ulp(ref, dtype):
    """Spacing of `dtype` at |ref| (ref float64): 2^(floor(log2|ref|) - mantissa bits), the subnormal spacing below 2^-126 and at 0."""
    _, e = torch.frexp(ref.abs())                                  # |ref| = m 2^e with m in [0.5, 1)
    e = torch.where(ref == 0, torch.full_like(e, -1000), e)
    return torch.ldexp(torch.ones_like(ref), (e - 1).clamp(min=-126) - MANT[dtype])


def rt(v64, dtype):
    """float64 -> fp32 (where the kernels compute) -> storage type -> float64."""
    return v64.to(torch.float32).to(dtype).double()


def check(family, got, ref, bound, what):
    """|got - ref| <= bound at EVERY element (NaN/inf fail); names the worst element and the rows that miss."""
    got64 = got.detach().cpu().double()
    assert got64.shape == ref.shape, f"{what}: shape {tuple(got64.shape)} vs {tuple(ref.shape)}"
    err = (got64 - ref).abs()
    bound = bound.expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)   # bound 0 and err > 0 -> inf
    ok = err <= bound                                                   # NaN compares false
    finite = ratio[torch.isfinite(ratio)]
    worst = float(finite.max()) if finite.numel() else 0.0
    if bool(ok.all()):
        _WORST[family] = max(_WORST.get(family, 0.0), worst)
        print(f"{what}: max err/bound {worst:.4f}")
        return
    bad = (~ok).nonzero()
    i = tuple(int(v) for v in bad[0])
    rows = sorted({int(r) for r in bad[:, 0]})
    raise AssertionError(f"{what}: {bad.shape[0]} of {err.numel()} elements miss their bound; first at {i}: got {float(got64[i])!r} ref "
                         f"{float(ref[i])!r} err {float(err[i]):.3e} bound {float(bound[i]):.3e}; rows {rows[:8]}{'...' if len(rows) > 8 else ''}")


# =====================================================================================================================
# RMSNorm
# =====================================================================================================================
def _chain(dim, dtype):
    """Longest chain of additions in a one-wave row reduction: a lane adds at most dim/64 + N of its own terms, then 6 xor-shuffle levels."""
    return dim // 64 + VEC[dtype] + 6


def rms_fwd_ref(x, w, dtype):
    """y = (x rstd).type_as(x) * scale, rstd = (mean x^2 + eps)^-1/2; returns (rstd, bound, y, bound) in float64."""
    x64, w64 = x.double(), w.double()
    dim = x.shape[-1]
    rstd = ((x64 * x64).mean(-1, keepdim=True) + EPS).rsqrt()
    # rstd: the sum of squares is off by at most chain U32 sum x^2 (relative chain U32, and eps only dilutes it); the division by dim, the
    # fp32 eps, the addition and rsqrtf (documented at 2 ulp) are 6 U32 more; the -1/2 power halves the sum's share
    e_r = (_chain(dim, dtype) / 2 + 6) * U32
    xn = x64 * rstd
    y = rt(xn, dtype) * w64
    # y: the fp32 product x rstd carries rstd's error and its own rounding, (e_r + U32)|xn|; it is then ROUNDED TO STORAGE (first rounding point:
    # one ulp at xn, which also covers the error above tipping the rounding the other way), multiplied by scale in fp32 (U32 |y|) and STORED
    # (second rounding point: one ulp at y)
    b_y = w64.abs() * (xn.abs() * (e_r + U32) + ulp(xn, dtype)) + U32 * y.abs() + ulp(y, dtype)
    return rstd.squeeze(-1), e_r * rstd.squeeze(-1), y, b_y


def _bwd_blocks(rows):
    return min((rows + 3) // 4, 256)


def rms_bwd_ref(dy, x, w, rstd32, dres, dscale0, dtype):
    """dx = rstd (dy w - xhat c) [+ dres], c = mean(dy w xhat), xhat = x rstd; dscale = [dscale0 +] sum_rows dy xhat.  rstd32 is the fp32
    tensor the kernel is given, so the backward is judged on its own."""
    dy64, x64, w64, rs = dy.double(), x.double(), w.double(), rstd32.double()[:, None]
    rows, dim = x.shape
    xhat, gw = x64 * rs, dy64 * w64
    t = gw * xhat
    c = t.mean(-1, keepdim=True)
    # c: each term is three fp32 roundings (xhat, dy w, their product), the reduction a chain of `chain` additions, the division one more:
    # (chain + 4) U32 sum|terms| / dim
    b_c = (_chain(dim, dtype) + 4) * U32 * t.abs().mean(-1, keepdim=True)
    dx = rs * (gw - xhat * c)
    if dres is not None:
        dx = dx + dres.double()
    # dx: fp32 roundings of dy w (1), xhat (1), xhat c (1), the difference (1), the product with rstd (1): at most 4 U32 |rstd| (|dy w| + |xhat c|);
    # the error of c enters as |rstd xhat| b_c; the residual add and the product's own rounding 2 U32 |dx|; then ONE rounding to storage: ulp(dx)
    b_dx = U32 * (4 * rs.abs() * (gw.abs() + (xhat * c).abs()) + 2 * dx.abs()) + (rs * xhat).abs() * b_c + ulp(dx, dtype)
    q = dy64 * xhat
    ds = q.sum(0)
    nb = _bwd_blocks(rows)
    rpw = -(-rows // (4 * nb))
    # dscale: a wave adds its rows one after the other (rpw), a block its 4 waves (3), the column sum runs 4 chains of nblocks/64 (+3 in the tail),
    # joins them (2) and adds 16 row groups (16); each term has 2 roundings of its own
    depth = rpw + -(-nb // 64) + 24
    b_ds = (depth + 2) * U32 * q.abs().sum(0)
    if dscale0 is not None:
        ds = ds + dscale0.double()
    # [+ the add onto the old value: U32 |dscale|] and ONE rounding to storage
    b_ds = b_ds + U32 * ds.abs() + ulp(ds, dtype)
    return dx, b_dx, ds, b_ds


def _rms_inputs(rows, dim, dtype, seed):
    x = rnd(rows, dim, dtype=dtype, seed=seed)
    w = (1 + 0.1 * rnd(dim, seed=seed + 1)).to(dtype)
    dy = rnd(rows, dim, dtype=dtype, seed=seed + 2)
    dres = rnd(rows, dim, dtype=dtype, seed=seed + 3)
    return x, w, dy, dres


def _run_rms_fwd(ops, x, w, with_rstd=True):
    y = torch.full(x.shape, SENTINEL, dtype=x.dtype, device=DEV)
    rstd = torch.full((x.shape[0],), SENTINEL, dtype=torch.float32, device=DEV) if with_rstd else None
    ops.rmsnorm_fwd(x.to(DEV), w.to(DEV), y, rstd, EPS)
    return y, rstd


def _run_rms_bwd(ops, dy, x, w, rstd32, dres, dscale0, accumulate):
    dx = torch.full(x.shape, SENTINEL, dtype=x.dtype, device=DEV)
    dscale = dscale0.to(DEV).clone()
    ops.rmsnorm_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), rstd32.to(DEV), None if dres is None else dres.to(DEV), dx, dscale, accumulate=accumulate)
    return dx, dscale


# vectors per lane 1 | 2 | 2 + one lane | 3 (a fully masked 4th group) | 4 | 4 + one lane | 6 | 8 | the largest dim the entries take
RMS_DIMS = {torch.bfloat16: [8, 512, 520, 1024, 1032, 1536, 2048, 2056, 4096], torch.float32: [8, 256, 264, 512, 520, 768, 1024, 1032, 2048]}
RMS_CASES = [(dt, d) for dt in DTYPES for d in RMS_DIMS[dt]]


@pytest.mark.parametrize("dtype,dim", RMS_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_rmsnorm_every_vectors_per_lane_branch_and_group_edge(ops, dtype, dim):
    """bf16 dim 4096 is the backward launch that asks for exactly 64 KiB of dynamic LDS."""
    rows = 7
    x, w, dy, dres = _rms_inputs(rows, dim, dtype, seed=100 + dim)
    rstd_ref, b_rstd, y_ref, b_y = rms_fwd_ref(x, w, dtype)
    y, rstd = _run_rms_fwd(ops, x, w)
    check("rmsnorm_fwd rstd", rstd, rstd_ref, b_rstd, f"rmsnorm_fwd[{dtype},{dim}] rstd")
    check("rmsnorm_fwd y", y, y_ref, b_y, f"rmsnorm_fwd[{dtype},{dim}] y")
    y2, _ = _run_rms_fwd(ops, x, w, with_rstd=False)
    assert torch.equal(y, y2), "y must not depend on whether rstd is asked for"
    rstd32 = rstd_ref.float()
    ds0 = rnd(dim, dtype=dtype, seed=7, scale=3.0)   # what accumulate=True adds to; accumulate=False must overwrite it
    for use_dres in (False, True):
        for accumulate in (False, True):
            dx_ref, b_dx, ds_ref, b_ds = rms_bwd_ref(dy, x, w, rstd32, dres if use_dres else None, ds0 if accumulate else None, dtype)
            dx, ds = _run_rms_bwd(ops, dy, x, w, rstd32, dres if use_dres else None, ds0, accumulate)
            tag = f"rmsnorm_bwd[{dtype},{dim},dres={use_dres},acc={accumulate}]"
            check("rmsnorm_bwd dx", dx, dx_ref, b_dx, tag + " dx")
            check("rmsnorm_bwd dscale", ds, ds_ref, b_ds, tag + " dscale")


@pytest.mark.parametrize("dtype,dim", [(torch.bfloat16, 4104), (torch.float32, 2056)], ids=["bf16-4104", "fp32-2056"])
def test_rmsnorm_dim_too_large_is_an_error_and_writes_nothing(ops, dtype, dim):
    rows = 7
    x, w, dy, dres = _rms_inputs(rows, dim, dtype, seed=3)
    y = torch.full(x.shape, SENTINEL, dtype=dtype, device=DEV)
    rstd = torch.full((rows,), SENTINEL, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError):
        ops.rmsnorm_fwd(x.to(DEV), w.to(DEV), y, rstd, EPS)
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()) and bool((rstd == SENTINEL).all())
    dx = torch.full(x.shape, SENTINEL, dtype=dtype, device=DEV)
    ds = torch.full((dim,), SENTINEL, dtype=dtype, device=DEV)
    with pytest.raises(RuntimeError):
        ops.rmsnorm_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), torch.ones(rows, device=DEV), dres.to(DEV), dx, ds)
    torch.cuda.synchronize()
    assert bool((dx == SENTINEL).all()) and bool((ds == SENTINEL).all())


def _row_loop_inputs(rows, dim, dtype, seed):
    """Rows that cannot be mistaken for one another: row r scaled by 2^((r mod 41) - 20) (exact in both types), and one all-zero row, the last
    (in the second register set whenever a wave has a second row)."""
    x, w, dy, dres = _rms_inputs(rows, dim, dtype, seed)
    s = torch.ldexp(torch.ones(rows), (torch.arange(rows) % 41 - 20).to(torch.int32))[:, None]
    x, dy = (x.float() * s).to(dtype), (dy.float() * s).to(dtype)
    x[rows - 1] = 0
    return x, w, dy, dres


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows", [4096, 4097, 8292, 12388])   # grid capped at 1024 blocks = 4096 waves: 1, 1-2, 2-3 and 3-4 rows per wave
def test_rmsnorm_fwd_row_loop_with_both_register_sets(ops, dtype, rows):
    dim = 128
    x, w, _, _ = _row_loop_inputs(rows, dim, dtype, seed=rows)
    rstd_ref, b_rstd, y_ref, b_y = rms_fwd_ref(x, w, dtype)
    assert abs(float(rstd_ref[rows - 1]) - EPS ** -0.5) < 1e-9 and bool((y_ref[rows - 1] == 0).all())   # the zero row: rstd = eps^-1/2, y = 0
    y, rstd = _run_rms_fwd(ops, x, w)
    check("rmsnorm_fwd rstd", rstd[:, None], rstd_ref[:, None], b_rstd[:, None], f"rmsnorm_fwd rows {rows} [{dtype}] rstd")
    check("rmsnorm_fwd y", y, y_ref, b_y, f"rmsnorm_fwd rows {rows} [{dtype}] y")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows", [1024, 1025, 2148, 3172])    # grid capped at 256 blocks = 1024 waves
def test_rmsnorm_bwd_row_loop_with_both_register_sets(ops, dtype, rows):
    dim = 128
    x, w, dy, dres = _row_loop_inputs(rows, dim, dtype, seed=rows)
    rstd32 = rms_fwd_ref(x, w, dtype)[0].float()
    dx_ref, b_dx, ds_ref, b_ds = rms_bwd_ref(dy, x, w, rstd32, dres, None, dtype)
    z = rows - 1   # the zero row: xhat = 0, c = 0, dx = rstd dy w + dres
    torch.testing.assert_close(dx_ref[z], float(rstd32[z]) * dy[z].double() * w.double() + dres[z].double(), rtol=1e-14, atol=0)
    dx, ds = _run_rms_bwd(ops, dy, x, w, rstd32, dres, torch.zeros(dim, dtype=dtype), False)
    check("rmsnorm_bwd dx", dx, dx_ref, b_dx, f"rmsnorm_bwd rows {rows} [{dtype}] dx")
    check("rmsnorm_bwd dscale", ds, ds_ref, b_ds, f"rmsnorm_bwd rows {rows} [{dtype}] dscale")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("dim", [2048, 520])
def test_rmsnorm_bwd_with_the_projection_term_visible(ops, dtype, dim):
    """dy = alpha xhat / w + noise makes c = mean(dy w xhat) about alpha, so - xhat c is as large as dy w: a wrong or missing c is far outside
    the derived bound (with dy ~ N(0,1) it is 0.02 xhat and hides inside a loose bf16 tolerance)."""
    rows, alpha = 5, 1.0
    x, w, noise, dres = _rms_inputs(rows, dim, dtype, seed=dim)
    rstd_ref = rms_fwd_ref(x, w, dtype)[0]
    dy = (alpha * x.double() * rstd_ref[:, None] / w.double() + 0.25 * noise.double()).to(torch.float32).to(dtype)
    rstd32 = rstd_ref.float()
    dx_ref, b_dx, ds_ref, b_ds = rms_bwd_ref(dy, x, w, rstd32, None, None, dtype)
    c = (dy.double() * w.double() * x.double() * rstd32.double()[:, None]).mean(-1)
    assert bool((c > 0.5 * alpha).all())                                   # the term is there ...
    without_c = rstd32.double()[:, None] * dy.double() * w.double()
    assert bool(((without_c - dx_ref).abs() > 16 * b_dx).float().mean() > 0.5)   # ... and dropping it misses the bound by far, in most elements
    dx, ds = _run_rms_bwd(ops, dy, x, w, rstd32, None, torch.zeros(dim, dtype=dtype), False)
    check("rmsnorm_bwd dx", dx, dx_ref, b_dx, f"rmsnorm_bwd projection [{dtype},{dim}] dx")
    check("rmsnorm_bwd dscale", ds, ds_ref, b_ds, f"rmsnorm_bwd projection [{dtype},{dim}] dscale")


# rows = 4 nb - 3 gives nb partial rows: below / at / past the 4-way unrolled loop's condition b + 48 < nblocks for the 16 row groups, one and
# several trips of it, and every tail length; 1024 rows = 256 blocks, the cap
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("nb", [1, 15, 16, 17, 48, 49, 64, 65, 112, 113, 255, 256])
def test_dscale_column_sum_unrolled_loop_and_tails(ops, dtype, nb):
    rows, dim = (1024 if nb == 256 else 4 * nb - 3), 72   # 72 columns: one full 64-column block and one of 8
    assert _bwd_blocks(rows) == nb
    x, w, dy, _ = _rms_inputs(rows, dim, dtype, seed=nb)
    rstd32 = rms_fwd_ref(x, w, dtype)[0].float()
    ds0 = rnd(dim, dtype=dtype, seed=9, scale=3.0)
    for accumulate in (False, True):
        _, _, ds_ref, b_ds = rms_bwd_ref(dy, x, w, rstd32, None, ds0 if accumulate else None, dtype)
        _, ds = _run_rms_bwd(ops, dy, x, w, rstd32, None, ds0, accumulate)
        check("dscale column sum", ds, ds_ref, b_ds, f"colsum[{dtype},nb={nb},acc={accumulate}]")
        _, again = _run_rms_bwd(ops, dy, x, w, rstd32, None, ds0, accumulate)
        assert torch.equal(ds, again), "the column sum adds in a fixed order: two runs must agree bit for bit"


# =====================================================================================================================
# SwiGLU
# =====================================================================================================================
def _swiglu_sigmoid(gu):
    inter = gu.shape[-1] // 2
    g, u = gu[:, :inter].double(), gu[:, inter:].double()
    sig = torch.sigmoid(g)
    # sigmoid in fp32: the bf16 kernels form exp2(g * -log2(e)) with v_exp_f32, whose argument carries the product's rounding and the constant's
    # (|g| log2(e) 1.5 U32 absolute, i.e. 1.5 ln2 |g| log2(e) U32 < 2 |g| U32 relative in the exponential), then v_exp_f32 and v_rcp_f32 at 1 ulp
    # (2 U32) each and the addition (U32); the fp32 kernels use expf (2 ulp) and a division: inside the same 2 |g| + 6
    e_sig = (2 * g.abs() + 6) * U32
    # Where the sigmoid falls below 2^-126 fp32 holds it as a subnormal, or as 0 once 1 + exp(-g) has overflowed to inf (g < -88.7): a value
    # that is off by up to 2^-126 absolute, times whatever multiplies it afterwards.  The same floor for each later product (the TINY terms).
    return g, u, sig, e_sig


def swiglu_fwd_ref(gu, dtype):
    """act = silu(gate).type_as(gate) * up; returns (ref, bound, where the stored bits are pinned)."""
    g, u, sig, e_sig = _swiglu_sigmoid(gu)
    s, ua = g * sig, u.abs()
    e_s = s.abs() * (e_sig + U32)
    act = rt(s, dtype) * u
    # act: the fp32 silu error e_s, ROUNDED TO STORAGE (one ulp at silu), times up; the product's rounding U32 |act|, STORED (one ulp at act)
    b_act = ua * (e_s + ulp(s, dtype)) + U32 * act.abs() + ulp(act, dtype) + (g.abs() * ua + ua + 1) * TINY
    # Sharper where the roundings are unambiguous: if every fp32 value within e_s of silu rounds to the same storage value, and every value within
    # U32 of the product does too, the stored bits are determined: those elements must match bit for bit (bound 0; kept away from the subnormal
    # floor).  Never so in fp32 storage, where e_s is several ulp: not looked for there.
    fixed = torch.zeros_like(s, dtype=torch.bool)
    if dtype == torch.bfloat16:
        fixed = (rt(s - e_s, dtype) == rt(s + e_s, dtype)) & (rt(act * (1 - 2 * U32), dtype) == rt(act * (1 + 2 * U32), dtype))
        fixed &= (s.abs() > 2 ** -100) & (act.abs() > 2 ** -100)
        act = torch.where(fixed, rt(act, dtype), act)
        b_act = torch.where(fixed, torch.zeros_like(b_act), b_act)
    return act, b_act, fixed


def swiglu_bwd_ref(gu, dact, dtype):
    """dgate = dact up sig (1 + gate (1 - sig)); dup = dact gate sig; returns (ref, bound) for [dgate | dup].  Contraction is off in the kernels,
    so operation by operation:"""
    g, u, sig, e_sig = _swiglu_sigmoid(gu)
    d = dact.double()
    d_sig = sig * e_sig                                   # absolute error of sig
    om = 1 - sig
    t = 1 + g * om
    # 1 - sig carries sig's error and the difference's rounding (|1 - sig| <= 1): d_sig + U32; t = 1 + gate (1 - sig): that times |gate|, the
    # product's rounding and the sum's
    d_t = g.abs() * (d_sig + U32) + U32 * ((g * om).abs() + t.abs())
    du, dg = (d * u).abs(), (d * g).abs()
    dgate, dup = d * u * sig * t, d * g * sig
    # dgate = (dact up) (sig t): three products (3 U32) on top of the errors of sig and t; ONE rounding to storage
    b_dgate = du * (t.abs() * d_sig + sig * d_t) + 3 * U32 * dgate.abs() + ulp(dgate, dtype) + (du * t.abs() + du + 1) * TINY
    # dup = dact (gate sig): two products; ONE rounding to storage
    b_dup = dg * d_sig + 2 * U32 * dup.abs() + ulp(dup, dtype) + (dg + d.abs() + 1) * TINY
    return torch.cat([dgate, dup], 1), torch.cat([b_dgate, b_dup], 1)


def _check_swiglu(ops, gu, dact, dtype, what, directions=("fwd", "bwd")):
    rows, inter = dact.shape
    gug, fixed = gu.to(DEV), None
    if "fwd" in directions:
        act_ref, b_act, fixed = swiglu_fwd_ref(gu, dtype)
        act = torch.full((rows, inter), SENTINEL, dtype=dtype, device=DEV)
        ops.swiglu_fwd(gug, act)
        assert bool(torch.isfinite(act.float()).all()), f"{what}: non-finite act"
        check("swiglu_fwd", act, act_ref, b_act, f"swiglu_fwd {what}")
    if "bwd" in directions:
        dgu_ref, b_dgu = swiglu_bwd_ref(gu, dact, dtype)
        dgu = torch.full((rows, 2 * inter), SENTINEL, dtype=dtype, device=DEV)
        ops.swiglu_bwd(dact.to(DEV), gug, dgu)
        assert bool(torch.isfinite(dgu.float()).all()), f"{what}: non-finite dgu"
        check("swiglu_bwd", dgu, dgu_ref, b_dgu, f"swiglu_bwd {what}")
    return fixed


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_swiglu_saturated_sigmoid_ends(ops, dtype):
    """Gate values where exp2 / expf overflow to inf (g < -88.7: the sigmoid must come out 0, not NaN), where the reciprocal is subnormal
    (-88.7 < g < -87.3), where exp underflows (g > 104) and around 0, each with up and dact of both signs."""
    gate = torch.cat([torch.arange(-130.0, 131.0), torch.tensor([-88.5, 88.5, -87.5, 87.5, -103.5, 103.5, -0.5, 0.5, -0.0, -16.5, 16.5])])
    assert all(v in gate.tolist() for v in (87.0, -87.0, 88.5, -88.5, 89.0, -89.0, 104.0, -104.0, 0.0)) and bool((gate.to(dtype).float() == gate).all())
    gate = torch.cat([gate, torch.zeros(-gate.numel() % 8)])
    signs = [(1.5, 0.75), (1.5, -0.75), (-1.5, 0.75), (-1.5, -0.75), (0.37109375, -1.25), (-0.37109375, 1.25)]   # (up, dact), exact in bf16
    inter = gate.numel()
    gu = torch.stack([torch.cat([gate, torch.full((inter,), up)]) for up, _ in signs]).to(dtype)
    dact = torch.stack([torch.full((inter,), d) for _, d in signs]).to(dtype)
    fixed = _check_swiglu(ops, gu, dact, dtype, f"saturation [{dtype}]")
    if dtype == torch.bfloat16:   # pinned bit for bit: what sees a silu that is not rounded to storage.  Not pinned: the quarter of the grid below
        assert float(fixed.float().mean()) > 0.5   # -69 (silu under 2^-100) and products on an exact bf16 tie (odd gate >= 87 times 1.5)


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("dtype,rows", [(torch.float32, 520), (torch.bfloat16, 1030)], ids=["fp32", "bf16"])
def test_swiglu_grid_stride_loop(ops, dtype, rows, direction):
    """More than 8192 * 256 vectors, so threads take a second trip that starts in the middle of a row; in bf16 the vectors per row are odd
    (2049; the fp32 row has 4098)."""
    inter = 16392
    assert rows * inter // VEC[dtype] > 8192 * 256 and (rows * inter // VEC[dtype]) % (8192 * 256) % (inter // VEC[dtype]) != 0
    assert dtype == torch.float32 or (inter // VEC[dtype]) % 2 == 1
    gu = rnd(rows, 2 * inter, dtype=dtype, seed=21, scale=2.0)
    dact = rnd(rows, inter, dtype=dtype, seed=22)
    _check_swiglu(ops, gu, dact, dtype, f"grid-stride [{dtype}]", directions=(direction,))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_swiglu_small_odd_case(ops, dtype):
    gu = rnd(3, 16, dtype=dtype, seed=23, scale=2.0)
    dact = rnd(3, 8, dtype=dtype, seed=24)
    _check_swiglu(ops, gu, dact, dtype, f"3 x 8 [{dtype}]")


# =====================================================================================================================
# RoPE
# =====================================================================================================================
def _rope_ref(x64, table, pos, n_rot, hd, sign):
    """Adjacent pairs: o0 = x0 c - x1 s, o1 = x1 c + x0 s over the first n_rot heads; returns (ref, bound without the storage ulp)."""
    rows = x64.shape[0]
    cs = table.double()[pos]                                   # [rows, hd/2, 2]
    c, s = cs[:, None, :, 0], cs[:, None, :, 1] * sign
    v = x64[:, : n_rot * hd].reshape(rows, n_rot, hd // 2, 2)
    x0, x1 = v[..., 0], v[..., 1]
    o = torch.stack([x0 * c - x1 * s, x1 * c + x0 * s], -1).reshape(rows, n_rot * hd)
    # two fp32 products (U32 each, contraction is off) and their sum or difference (U32 of the result, itself at most the sum of the products)
    mag = torch.stack([(x0 * c).abs() + (x1 * s).abs(), (x1 * c).abs() + (x0 * s).abs()], -1).reshape(rows, n_rot * hd)
    return o, 2 * U32 * mag


@pytest.mark.parametrize("explicit", [False, True], ids=["implicit", "explicit"])
@pytest.mark.parametrize("hd", [8, 16, 64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_rope_on_a_window_of_a_larger_buffer(ops, dtype, hd, explicit):
    from ssi.model import llama3_rope_table
    heads, n_rot, rows, seq, tlen = 3, 2, 301, 19, 64          # 301 rows: several blocks at every head_dim, the last one partly filled
    width, r0, c0 = heads * hd, 2, 16
    ld = width + 40
    assert (r0 * ld + c0) % 8 == 0 and ld % 8 == 0 and (rows * n_rot * hd // VEC[dtype]) % 256 != 0
    table = llama3_rope_table(hd, tlen)
    if explicit:
        pos = (torch.arange(rows) * 37 + 11) % tlen            # not monotonic
        pos[0], pos[1] = tlen - 1, 0                            # the table's last row, then 0
        pos_dev = pos.to(torch.int32).to(DEV)
    else:
        pos, pos_dev = torch.arange(rows) % seq, None
    buf0 = torch.full((rows + 5, ld), SENTINEL, dtype=dtype)
    buf0[r0:r0 + rows, c0:c0 + width] = rnd(rows, width, dtype=dtype, seed=hd)
    buf = buf0.to(DEV)
    x = buf[r0:r0 + rows, c0:c0 + width]
    rot = torch.zeros(buf0.shape, dtype=torch.bool)
    rot[r0:r0 + rows, c0:c0 + n_rot * hd] = True
    ops.rope_(x, seq, n_rot, hd, table.to(DEV), positions=pos_dev)
    fwd = buf.cpu()
    assert torch.equal(fwd[~rot], buf0[~rot]), "sentinels and unrotated columns must stay bit-identical"
    ref, b = _rope_ref(buf0[r0:r0 + rows, c0:c0 + width].double(), table, pos, n_rot, hd, 1.0)
    got = fwd[r0:r0 + rows, c0:c0 + n_rot * hd]
    check("rope", got, ref, b + ulp(ref, dtype), f"rope[{dtype},hd={hd},explicit={explicit}] forward")      # + ONE rounding to storage
    # the inverse, judged against the float64 inverse rotation of the very bits the forward stored
    ops.rope_(x, seq, n_rot, hd, table.to(DEV), inverse=True, positions=pos_dev)
    back = buf.cpu()
    assert torch.equal(back[~rot], buf0[~rot])
    ref_i, b_i = _rope_ref(fwd[r0:r0 + rows, c0:c0 + width].double(), table, pos, n_rot, hd, -1.0)
    got_i = back[r0:r0 + rows, c0:c0 + n_rot * hd]
    check("rope", got_i, ref_i, b_i + ulp(ref_i, dtype), f"rope[{dtype},hd={hd},explicit={explicit}] inverse")
    # ... and as a round trip: the exact inverse of the exact forward is the input, and the inverse is linear with |c| + |s| <= sqrt 2, so what the
    # forward's stored values were off by (at most the larger bound of the pair) comes back at most sqrt 2 times, next to the inverse's own error
    orig = buf0[r0:r0 + rows, c0:c0 + n_rot * hd].double()
    pair_max = (b + ulp(ref, dtype)).reshape(rows, -1, 2).amax(-1, keepdim=True).expand(-1, -1, 2).reshape(rows, -1)
    check("rope round trip", got_i, orig, b_i + ulp(ref_i, dtype) + math.sqrt(2) * pair_max, f"rope[{dtype},hd={hd},explicit={explicit}] round trip")


# =====================================================================================================================
# Embedding gather and scatter-add
# =====================================================================================================================
VOCAB = 1700          # fillers are 100 + t, each seen once (the n == 1 fast path); the small ids are the ones a layout repeats
N_TOKS = [1, 63, 64, 65, 1000, 1537]
LAYOUTS = ["a", "b63", "b64", "b65", "c", "d", "e"]


def _tokens(layout, n_tok):
    t = torch.arange(n_tok)
    tok = 100 + t
    if layout == "a":      # ids 1..7 occurring exactly 1, 2, 7, 8, 9, 16, 17 times inside one 512-position scan window, first hits off the 64-boundaries
        lo = 64 if n_tok >= 600 else 0
        span = min(n_tok - lo, 448)                 # [lo, lo + 448) lies inside the window of any first hit at or after lo
        pool = (lo + torch.randperm(span, generator=torch.Generator().manual_seed(n_tok))).tolist()
        for tid, cnt in zip(range(1, 8), [1, 2, 7, 8, 9, 16, 17]):
            for _ in range(cnt):
                if pool:
                    tok[pool.pop()] = tid
    elif layout[0] == "b":  # one id at t0, t0 + 511 (last of the first window when t0 is 64), t0 + 512 (first of the second) and the last position
        t0 = int(layout[1:])
        for p in (t0, t0 + 511, t0 + 512, n_tok - 1):
            if 0 <= p < n_tok:
                tok[p] = 5
    elif layout == "c":    # one id everywhere: hit lists of exactly 512, then a partial last window (488 hits at 1000, a single one at 1537)
        tok[:] = 3
    elif layout == "d":    # -1, V and 2^40 between valid ids, some of those repeated
        tok = 100 + t % 50
        tok[1::6], tok[3::6], tok[5::6] = -1, VOCAB, 2 ** 40
    elif layout == "e":    # a pad-like run of one id spanning several 64-wide chunks, and once more at the end
        tok = torch.randint(0, VOCAB, (n_tok,), generator=torch.Generator().manual_seed(9))
        tok[n_tok // 10: (4 * n_tok) // 10] = 7
        tok[-1] = 7
    return tok.to(torch.int64)


def _embed_case(ops, tok, dim, dtype, what):
    n_tok, G = tok.numel(), 3
    valid = (tok >= 0) & (tok < VOCAB)
    tv = tok[valid]
    counts = torch.bincount(tv, minlength=VOCAB)
    touched = counts > 0
    # ---- gather: row copies, zeros for ids outside the vocabulary; bit for bit, guard rows of `out` included
    table = rnd(VOCAB, dim, dtype=dtype, seed=8)
    out_full = torch.full((n_tok + 2, dim), SENTINEL, dtype=dtype, device=DEV)
    ops.embed_fwd(tok.to(DEV), table.to(DEV), out_full[1:1 + n_tok], VOCAB)
    exp = torch.full((n_tok + 2, dim), SENTINEL, dtype=dtype)
    exp[1:1 + n_tok] = torch.where(valid[:, None], table[tok.clamp(0, VOCAB - 1)], torch.zeros((), dtype=dtype))
    assert torch.equal(out_full.cpu(), exp), f"{what}: gather"

    def scatter(dout, base):
        full = torch.full((VOCAB + 2 * G, dim), SENTINEL, dtype=dtype)
        full[G:G + VOCAB] = base
        runs = []
        for _ in range(2):
            f = full.to(DEV)
            ops.embed_bwd(tok.to(DEV), dout.to(DEV), f[G:G + VOCAB], VOCAB)   # dtable = the middle rows of a taller buffer
            runs.append(f.cpu())
        assert torch.equal(runs[0], runs[1]), f"{what}: the scatter-add must be bitwise reproducible"
        got = runs[0]
        assert bool((got[:G] == SENTINEL).all()) and bool((got[G + VOCAB:] == SENTINEL).all()), f"{what}: guard rows"
        assert torch.equal(got[G:G + VOCAB][~touched], base[~touched]), f"{what}: vocabulary rows without a token must stay bit-identical"
        return got[G:G + VOCAB]

    # ---- scatter-add on small integers: every sum is an integer of magnitude <= 256, which fp32 and bf16 hold exactly, so any order of
    # additions gives the same bits and the result is compared bit for bit
    amp = 3 if int(counts.max()) <= 20 else 1
    g = torch.Generator().manual_seed(n_tok * 131 + dim)
    dout_i = torch.randint(-amp, amp + 1, (n_tok, dim), generator=g).to(dtype)
    base_i = torch.randint(-8, 9, (VOCAB, dim), generator=g).to(dtype)
    ref_i = base_i.double().index_add(0, tv, dout_i.double()[valid])
    assert float(ref_i.abs().max()) <= 256 and float(base_i.double().abs().index_add(0, tv, dout_i.double().abs()[valid]).max()) < 2 ** 24
    got_i = scatter(dout_i, base_i)
    assert torch.equal(got_i.double(), ref_i), f"{what}: integer scatter-add differs in rows {sorted(set((got_i.double() != ref_i).nonzero()[:, 0].tolist()))[:8]}"
    # ---- scatter-add on random data, relative to the float64 sum
    dout = rnd(n_tok, dim, dtype=dtype, seed=10)
    base = rnd(VOCAB, dim, dtype=dtype, seed=11)
    ref = base.double().index_add(0, tv, dout.double()[valid])
    mag = base.double().abs().index_add(0, tv, dout.double().abs()[valid])
    # count additions in position order plus the one onto the table row: (count + 1) U32 (|old| + sum|terms|); ONE rounding to storage
    bound = (counts[:, None].double() + 1) * U32 * mag + ulp(ref, dtype)
    check("embed scatter-add", scatter(dout, base), ref, bound, f"{what}: random scatter-add")


EMBED_LAYOUT_DIM = {torch.bfloat16: 520, torch.float32: 264}   # two vector groups, the second one lane wide


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("n_tok", N_TOKS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_embedding_token_layouts(ops, dtype, layout, n_tok):
    _embed_case(ops, _tokens(layout, n_tok), EMBED_LAYOUT_DIM[dtype], dtype, f"embed[{dtype},{layout},n_tok={n_tok}]")


# vectors per lane 1 (8 columns: one lane), 1 (half a wave), 2 with one lane in the second group, 2, 4, 8
EMBED_DIMS = {torch.bfloat16: [8, 256, 520, 1024, 2048, 4096], torch.float32: [8, 128, 264, 512, 1024, 2048]}


@pytest.mark.parametrize("layout,n_tok", [("a", 1000), ("c", 1537)])
@pytest.mark.parametrize("dtype,dim", [(dt, d) for dt in DTYPES for d in EMBED_DIMS[dt]], ids=lambda v: str(v).replace("torch.", ""))
def test_embedding_every_vectors_per_lane_branch(ops, dtype, dim, layout, n_tok):
    _embed_case(ops, _tokens(layout, n_tok), dim, dtype, f"embed[{dtype},dim={dim},{layout}]")


@pytest.mark.parametrize("dtype,dim", [(torch.bfloat16, 4104), (torch.float32, 2056)], ids=["bf16-4104", "fp32-2056"])
def test_embedding_bwd_dim_too_large_is_an_error_and_writes_nothing(ops, dtype, dim):
    tok = _tokens("a", 65)
    dtable = torch.full((VOCAB, dim), SENTINEL, dtype=dtype, device=DEV)
    with pytest.raises(RuntimeError):
        ops.embed_bwd(tok.to(DEV), rnd(65, dim, dtype=dtype, seed=1).to(DEV), dtable, VOCAB)
    torch.cuda.synchronize()
    assert bool((dtable == SENTINEL).all())
    table = rnd(VOCAB, dim, dtype=dtype, seed=2)              # the gather has no such limit
    out = torch.empty(65, dim, dtype=dtype, device=DEV)
    ops.embed_fwd(tok.to(DEV), table.to(DEV), out, VOCAB)
    assert torch.equal(out.cpu(), table[tok])


# =====================================================================================================================
# Transpose
# =====================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,cols", [(200, 136), (8, 8), (72, 64)])
def test_transpose_between_windows_of_padded_buffers(ops, dtype, rows, cols):
    src_full = rnd(rows + 3, cols + 24, dtype=dtype, seed=rows)            # ld > extent on both sides, windows at a 16-byte aligned offset
    dst0 = torch.full((cols + 3, rows + 16), SENTINEL, dtype=dtype)
    dst_full = dst0.to(DEV)
    ops.transpose(src_full.to(DEV)[2:2 + rows, 8:8 + cols], dst_full[1:1 + cols, 8:8 + rows])
    exp = dst0.clone()
    exp[1:1 + cols, 8:8 + rows] = src_full[2:2 + rows, 8:8 + cols].t()
    assert torch.equal(dst_full.cpu(), exp)
