"""The generic attention kernels (csrc/attention_generic.hip: ``attn_fwd_generic``, ``attn_bwd_dq_generic``, ``attn_bwd_dkv_generic<DK>``) at
every head geometry they serve, per (token, head) row through ``attn_stress.check_all`` — the criterion of test_attn_stress_gpu.py:

    |got_row - exact_row| <= 8 * E_row,   E_row = max(|restated_row - exact_row|, eps max(|exact_row|, 0.02 rms_row))   for EVERY row

(bf16: ``restated`` and eps 2^-8; fp32: the exact result rounded to fp32 and eps 1e-5; dq: E_row also >= eps x its conditioning on the stored
O), lse within its tolerance, outputs that start as NaN.  Each case runs under ``IMPL_GENERIC`` and under ``IMPL_AUTO``, where the dispatcher
must arrive at these kernels by itself (no MFMA bit in ``attn_last_dispatch()``) and give the same bits.

Geometries (``attn_stress.GEOMETRIES``; the key loop is ``j = j0 + lane; j <= i; j += 64``, the dK/dV loop ``e = lane; e < nq * rep; e += 64``):
head_dim 128 at (2, 192, 6, 2) — Llama-3.2-3B's three query heads per kv head; rows of 1 to 192 keys: one, two and three passes, idle lanes
merged with m = -inf; nq * rep up to 576 — the same packed as documents ((100, 37, 55), (1, 63, 64, 64)), and at (1, 64, 2, 2): rep 1, exactly
one pass; head_dim 16 at (2, 130, 3, 1): rep 3 on one kv head, two lanes into a third pass; head_dim 32 at (1, 65, 8, 1): rep 8, one key in
the second pass, 65 kv waves (a partly filled last workgroup of dK/dV); head_dim 64 at (1, 63, 3, 1), fp32: partly filled last workgroups in
every kernel; head_dim 64 at (2, 128, 6, 2), bf16: the shape the MFMA kernels would take but for rep = 3 — AUTO runs the generic kernels and
``IMPL_MFMA`` refuses without writing.  At the 3B shape also: ``qkv`` / ``dqkv`` as windows of wider buffers (NaN and a sentinel in the pad
columns), the RoPE backward as the second launch with implicit and with document-relative positions, and reproducibility (a second call; a
batch row alone).  ``sink`` runs at the 3B shape only: on the shorter rows the checker would be blind on too many dq rows
(test_attn_stress_ref.py).  The module prints its worst err / E_row per form and block (run with -s); DESIGN.md section 3 has the table.

Measured on the MI355X (margin 8): bf16 at most out 0.72, dq 1.48, dk 2.60 (``sharp`` at the 3B shape, batch row 0, position 88, kv head 0),
dv 0.74; fp32 at most out 0.50, dq 0.25, dk 0.56, dv 0.38; lse at most 0.15 of its tolerance; with the RoPE backward dq 1.36, dk 1.28.
"""
import pytest
import torch

import attn_stress as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = ("bf16", "fp32")
ONLY = {(64, (1, 63, 3, 1)): "fp32", (64, (2, 128, 6, 2)): "bf16"}      # geometries that run in one dtype
PLAIN = [(hd, sh, rows, c, dt) for hd, sh, rows, c in A.GEO_CONFIGS for dt in DTYPES if ONLY.get((hd, sh), dt) == dt]
PLAIN_IDS = [f"{i}-{dt}" for i, (hd, sh, rows, c) in zip(A.GEO_IDS, A.GEO_CONFIGS) for dt in DTYPES if ONLY.get((hd, sh), dt) == dt]
HD3B, SHAPE3B = 128, A.GEO_3B
WORST = {}     # form -> block -> worst err / E_row, printed when the module is done


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for form in sorted(WORST):
        print(f"\nworst err / E_row  {form:40s} " + "  ".join(f"{b} {v:.2f}" for b, v in WORST[form].items()), end="")
    print()


_ON_DEVICE = {}


def _inputs(case, shape, hd, fp32):
    """(qkv, dout) on the device, copied once per (case, shape, head_dim, dtype)."""
    key = (case, shape, hd, fp32)
    if key not in _ON_DEVICE:
        qkv, dout = A.make_inputs(case, *shape, hd=hd)
        _ON_DEVICE[key] = tuple((t.float() if fp32 else t).to(DEV) for t in (qkv, dout))
    return _ON_DEVICE[key]


def _refs(case, shape, hd, rows, fp32):
    ex = A.exact(case, *shape, rows, hd=hd)
    return ex, (A.f32_restated(ex) if fp32 else A.restated(case, *shape, rows, hd=hd))


def _docs(rows, S):
    return (None, None, None) if rows is None else tuple(t.to(DEV) for t in A.doc_arrays([list(r) for r in rows], S))


def _mfma_bits():
    from ssi import _lib
    return 0x10000 | _lib.ATTN_USED_DQ2 | _lib.ATTN_USED_DKV2 | _lib.ATTN_USED_HEAD_SPLIT | _lib.ATTN_USED_PLAN


def _run(ops, impl, x, dout, shape, hd, ds=None, de=None, out=None, d=None, **kw):
    """Forward and backward under ``impl`` into NaN-filled results (or into ``out`` / ``d``): (out, lse, dqkv, attn_last_dispatch())."""
    B, S, H, KV = shape
    prev = ops.set_impl(impl)
    try:
        out = torch.full((B * S, H * hd), float("nan"), dtype=x.dtype, device=DEV) if out is None else out
        lse = torch.full((B * H * S,), float("nan"), dtype=torch.float32, device=DEV)
        ops.attn_fwd(x, out, lse, B, S, H, KV, hd, ds, de)
        d = torch.full_like(x, float("nan")) if d is None else d
        delta = torch.full_like(lse, float("nan"))
        ops.attn_bwd(x, out, dout, lse, d, delta, B, S, H, KV, hd, doc_start=ds, doc_end=de, **kw)
        used = ops.attn_last_dispatch()
        torch.cuda.synchronize()
    finally:
        ops.set_impl(prev)
    return out, lse, d, used


@pytest.mark.parametrize("hd,shape,rows,case,dtype", PLAIN, ids=PLAIN_IDS)
def test_every_row_of_the_generic_kernels(ops, hd, shape, rows, case, dtype):
    """out, lse, dq, dk and dv of the three generic kernels, every row, under IMPL_GENERIC and as IMPL_AUTO dispatches by itself."""
    from ssi import _lib
    fp32 = dtype == "fp32"
    x, dout = _inputs(case, shape, hd, fp32)
    ds, de, _ = _docs(rows, shape[1])
    ex, rs = _refs(case, shape, hd, rows, fp32)
    form = f"hd {hd} {shape[2]}h/{shape[3]}kv S {shape[1]}{' docs' if rows else ''} {dtype}"
    got = {}
    for impl, name in ((_lib.IMPL_GENERIC, "generic"), (_lib.IMPL_AUTO, "auto")):
        out, lse, d, used = got[name] = _run(ops, impl, x, dout, shape, hd, ds, de)
        assert (used & _mfma_bits()) == 0, f"{name}: dispatched {hex(used)}, wanted the generic kernels"
        A.check_all(out.cpu(), lse.cpu(), d.cpu(), ex, rs, *shape, name=f"{name} {form} {case}", eps=A.EPS_F32 if fp32 else A.EPS_BF16, hd=hd,
                    record=WORST.setdefault(form, {}))
    for a, b in zip(got["generic"][:3], got["auto"][:3]):
        assert torch.equal(a, b), "IMPL_AUTO ran other kernels than IMPL_GENERIC"


def test_forced_mfma_refuses_three_heads_per_kv_head_and_writes_nothing(ops):
    """(2, 128, 6, 2) at head_dim 64 in bf16 is an MFMA shape but for rep = 3: forced, both entries raise "unsupported" and leave out and dqkv
    as they were (AUTO on this shape: the generic kernels, in the test above)."""
    from ssi import _lib
    hd, shape = 64, (2, 128, 6, 2)
    B, S, H, KV = shape
    x, dout = _inputs("gauss", shape, hd, False)
    out, lse, _, _ = _run(ops, _lib.IMPL_GENERIC, x, dout, shape, hd)
    prev = ops.set_impl(_lib.IMPL_MFMA)
    try:
        out2, d2 = torch.full_like(out, 3.0), torch.full_like(x, -5.0)
        lse2, delta = torch.full_like(lse, 7.0), torch.full_like(lse, 9.0)
        with pytest.raises(RuntimeError, match="MFMA path forced but unsupported shape"):
            ops.attn_fwd(x, out2, lse2, B, S, H, KV, hd)
        with pytest.raises(RuntimeError, match="MFMA path forced but unsupported shape"):
            ops.attn_bwd(x, out, dout, lse, d2, delta, B, S, H, KV, hd)
        torch.cuda.synchronize()
    finally:
        ops.set_impl(prev)
    assert bool((out2 == 3.0).all()) and bool((lse2 == 7.0).all()) and bool((d2 == -5.0).all()) and bool((delta == 9.0).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pad", (8, 24))
def test_padded_leading_dimension(ops, pad, dtype):
    """``qkv`` and ``dqkv`` as windows of buffers ``pad`` columns wider (NaN in the pad columns of qkv, a sentinel in those of dqkv): the bits of
    the dense call, and the sentinel untouched."""
    from ssi import _lib
    case, fp32 = "ramp8", dtype == "fp32"
    x, dout = _inputs(case, SHAPE3B, HD3B, fp32)
    rows, cols = x.shape
    dense = _run(ops, _lib.IMPL_AUTO, x, dout, SHAPE3B, HD3B)
    wide_x = torch.full((rows, cols + pad), float("nan"), dtype=x.dtype, device=DEV)
    wide_x[:, :cols] = x
    wide_d = torch.full((rows, cols + pad), -640.0, dtype=x.dtype, device=DEV)
    wide_d[:, :cols] = float("nan")
    out, lse, d, used = _run(ops, _lib.IMPL_AUTO, wide_x[:, :cols], dout, SHAPE3B, HD3B, d=wide_d[:, :cols])
    assert d.data_ptr() == wide_d.data_ptr() and d.stride(0) == cols + pad and (used & _mfma_bits()) == 0
    for a, b, what in zip(dense[:3], (out, lse, d), ("out", "lse", "dqkv")):
        assert torch.equal(a, b), f"{what} differs from the dense call at ld = cols + {pad}"
    assert bool((wide_d[:, cols:] == -640.0).all()), "the backward wrote into the pad columns of dqkv"
    assert bool(torch.isnan(wide_x[:, cols:]).all()) and torch.equal(wide_x[:, :cols], x)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("positions", ("implicit", "document-relative"))
def test_fused_rope_backward_at_head_dim_128(ops, positions, dtype):
    """The RoPE backward of the generic path — the second launch, ``ssi_rope_inplace`` inverse — at head_dim 128: dq and dk rows against the
    references rotated in fp64 (``rope_refs``), with the positions 0 .. S - 1 of plain rows and with each document's own of packed rows."""
    from ssi import _lib
    from ssi.model import llama3_rope_table
    case, fp32 = "ramp8", dtype == "fp32"
    B, S, H, KV = SHAPE3B
    rows = A.GEO_DOC_ROWS if positions == "document-relative" else None
    x, dout = _inputs(case, SHAPE3B, HD3B, fp32)
    ds, de, pos = _docs(rows, S)
    ex, rs = _refs(case, SHAPE3B, HD3B, rows, fp32)
    table = llama3_rope_table(HD3B, 256, 500_000, 32)
    hpos = torch.arange(S, dtype=torch.int32).repeat(B) if rows is None else pos.cpu()
    if fp32:
        rot = A.rope_transpose(ex["dqkv"], table, hpos, H, KV, HD3B)
        ref = (rot, rot.float().double())
    else:
        ref = A.rope_refs(ex, rs, table, hpos, H, KV, HD3B)
    kw = {"rope_table": table.to(DEV)}
    if rows is not None:
        kw["positions"] = pos
    _, _, d, used = _run(ops, _lib.IMPL_AUTO, x, dout, SHAPE3B, HD3B, ds, de, **kw)
    assert (used & _mfma_bits()) == 0
    A.check_all(None, None, d.cpu(), ex, rs, *SHAPE3B, name=f"rope {positions} {dtype}", eps=A.EPS_F32 if fp32 else A.EPS_BF16, ref_dqkv=ref,
                hd=HD3B, record=WORST.setdefault(f"hd 128 6h/2kv S 192 +rope {positions} {dtype}", {}))
    plain = _run(ops, _lib.IMPL_AUTO, x, dout, SHAPE3B, HD3B, ds, de)[2]
    lo, _ = A.block_cols("dv", H, KV, HD3B)
    assert torch.equal(d[:, lo:], plain[:, lo:]), "dv is not rotated"


@pytest.mark.parametrize("dtype", DTYPES)
def test_reproducible_and_independent_of_the_other_batch_row(ops, dtype):
    """A second call gives the same bits; batch row 1 alone gives the bits it has inside the batch."""
    from ssi import _lib
    fp32 = dtype == "fp32"
    B, S, H, KV = SHAPE3B
    x, dout = _inputs("sharp", SHAPE3B, HD3B, fp32)
    first = _run(ops, _lib.IMPL_AUTO, x, dout, SHAPE3B, HD3B)
    again = _run(ops, _lib.IMPL_AUTO, x, dout, SHAPE3B, HD3B)
    for a, b in zip(first[:3], again[:3]):
        assert torch.equal(a, b)
    out1, lse1, d1, _ = _run(ops, _lib.IMPL_AUTO, x[S:].contiguous(), dout[S:].contiguous(), (1, S, H, KV), HD3B)
    assert torch.equal(out1, first[0][S:]) and torch.equal(lse1, first[1][H * S:]) and torch.equal(d1, first[2][S:])
