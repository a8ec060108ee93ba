"""Attention parity per (token, head) row, on inputs that move the softmax: every kernel form of the attention path against the two CPU
references of tests/attn_stress.py (fp64 exact; fp32 with the kernels' documented rounding points), through ``row_check``:

    |got_row - exact_row| <= 8 * E_row,   E_row = max(|restated_row - exact_row|, 2^-8 max(|exact_row|, 0.02 rms_row))   for EVERY row

(dq: E_row also >= 2^-8 x the conditioning of dq on the stored O; fp32 forms: 1e-5 for 2^-8 and the exact result rounded to fp32 for the
restated one), lse within 8 x the error of a plain fp32 logsumexp (at least 2e-5), all values finite, the dispatch asserted.  The margin 8 is
twice what a second legitimate restatement needs (test_attn_stress_ref.py holds that, the blind-share cap and the checker's teeth on the CPU).

Cases (attn_stress.make_inputs): ``gauss`` control; ``ramp8`` a rescale of the forward's running maximum on every key tile, the row's largest
scores on the masked keys of the diagonal tile, lse up to 67; ``ramp5`` a stale maximum on alternate tiles, probabilities up to e^5; ``fall``
the maximum in the first tile (in packed rows: on keys of earlier documents, which must contribute nothing); ``sink`` two keys with a large
share of every later row; ``sharp`` near-one-hot rows.  Shapes: (2, 512, 4, 1) — several key tiles per row, two 256-key groups, masked and
unmasked tiles — and (2, 256, 8, 2) — no unmasked 256-key tile, two kv heads.

NOT YET MEASURED: when this file was written no MI355X run of it could be made, so the table of the kernels' worst err / E_row per form and
block is missing here and in DESIGN.md section 3; the module prints it ("worst err / E_row  <form> ...", run with -s) and the first GPU run is to
enter it.  What is known from the CPU: the second restatement of test_attn_stress_ref.py, standing in for a kernel in a dry run of every test
below, reaches out 1.03, dq 2.82, dk 2.45 (with the RoPE transpose), dv 0.99, lse 0.13 of its tolerance.
"""
import pytest
import torch

import attn_stress as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
HD = A.HD
PLAIN = [(c, sh) for sh in A.SHAPES for c in A.CASES]
PLAIN_IDS = [f"{c}-{sh[0]}x{sh[1]}-{sh[2]}h{sh[3]}kv" for c, sh in PLAIN]
DOC_IDS = [f"{c}-{len(rows[0])}docs" for c, rows in A.DOC_CASES]
WORST = {}     # form -> block -> worst err / E_row, printed when the module is done


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for form in sorted(WORST):
        print(f"\nworst err / E_row  {form:34s} " + "  ".join(f"{b} {v:.2f}" for b, v in WORST[form].items()), end="")
    print()


@pytest.fixture
def attn_impl(ops):
    """Switch the attention backward kernels through the ABI's setter (``ssi_set_attn_impl``) and put the previous modes back afterwards."""
    saved = {}

    def choose(which, mode):
        prev = ops.set_attn_impl(which, mode)
        saved.setdefault(which, prev)

    yield choose
    for which, mode in saved.items():
        ops.set_attn_impl(which, mode)


_ON_DEVICE = {}


def _inputs(case, shape, fp32=False):
    """(qkv, dout) on the device, copied once per (case, shape, dtype)."""
    key = (case, shape, fp32)
    if key not in _ON_DEVICE:
        qkv, dout = A.make_inputs(case, *shape)
        _ON_DEVICE[key] = tuple((t.float() if fp32 else t).to(DEV) for t in (qkv, dout))
    return _ON_DEVICE[key]


def _rope(shape, rows=None):
    """The real table (a rotation: row norms are preserved) on the device and the positions of the tokens, on the host."""
    from ssi.model import llama3_rope_table
    B, S = shape[:2]
    table = llama3_rope_table(HD, 512, 500_000, 32)
    pos = torch.arange(S, dtype=torch.int32).repeat(B) if rows is None else A.doc_arrays(rows, S)[2]
    return table, pos


def _forward(ops, impl, x, shape, ds=None, de=None):
    B, S, H, KV = shape
    prev = ops.set_impl(impl)
    try:
        out = torch.full((B * S, H * HD), float("nan"), dtype=x.dtype, device=DEV)
        lse = torch.full((B * H * S,), float("nan"), dtype=torch.float32, device=DEV)
        ops.attn_fwd(x, out, lse, B, S, H, KV, HD, ds, de)
    finally:
        ops.set_impl(prev)
    return out, lse


def _backward(ops, impl, x, dout, out, lse, shape, **kw):
    B, S, H, KV = shape
    prev = ops.set_impl(impl)
    try:
        d = torch.full_like(x, float("nan"))
        delta = torch.full_like(lse, float("nan"))
        ops.attn_bwd(x, out, dout, lse, d, delta, B, S, H, KV, HD, **kw)
        used = ops.attn_last_dispatch()
    finally:
        ops.set_impl(prev)
    return d, used


@pytest.mark.parametrize("form", ["mfma", "generic-bf16", "generic-fp32"])
@pytest.mark.parametrize("case,shape", PLAIN, ids=PLAIN_IDS)
def test_forward(ops, case, shape, form):
    """out and lse of attn_fwd_kernel (the deferred max-rescale: RESCALE_TAU) and of the generic kernel in bf16 and fp32."""
    from ssi import _lib
    fp32 = form == "generic-fp32"
    x, _ = _inputs(case, shape, fp32)
    out, lse = _forward(ops, _lib.IMPL_MFMA if form == "mfma" else _lib.IMPL_GENERIC, x, shape)
    ex = A.exact(case, *shape)
    rs = A.f32_restated(ex) if fp32 else A.restated(case, *shape)
    A.check_all(out.cpu(), lse.cpu(), None, ex, rs, *shape, name=f"fwd {form} {case} {shape}", eps=A.EPS_F32 if fp32 else A.EPS_BF16,
                record=WORST.setdefault(f"forward {form}", {}))


BWD_FORMS = ["dq+dkv128", "dq2+dkv2", "dq2+dkv128-head-split", "generic-bf16", "generic-fp32"]


@pytest.mark.parametrize("fused_rope", [False, True], ids=["plain-epilogue", "fused-rope"])
@pytest.mark.parametrize("form", BWD_FORMS)
@pytest.mark.parametrize("case,shape", PLAIN, ids=PLAIN_IDS)
def test_backward(ops, case, shape, form, fused_rope, attn_impl):
    """dq, dk, dv of: attn_bwd_dq_kernel + the 128-key attn_bwd_dkv_kernel (mode OLD); attn_bwd_dq2_kernel + attn_bwd_dkv2_kernel (mode NEW);
    dq2 + the dK/dV kernel split over the query heads with its reduction (caller-owned workspace); the generic kernels — each also with the
    RoPE backward fused into its epilogues (the references' dq and dk rows through the inverse rotation in fp64)."""
    from ssi import _lib
    B, S, H, KV = shape
    fp32, generic = form == "generic-fp32", form.startswith("generic")
    impl = _lib.IMPL_GENERIC if generic else _lib.IMPL_MFMA
    x, dout = _inputs(case, shape, fp32)
    out, lse = _forward(ops, impl, x, shape)
    kw, want_bits = {}, 0
    if form == "dq+dkv128":
        attn_impl(_lib.ATTN_KERNEL_DQ, _lib.ATTN_MODE_OLD), attn_impl(_lib.ATTN_KERNEL_DKV, _lib.ATTN_MODE_OLD)
        want_bits = 0x10000
    elif form == "dq2+dkv2":
        attn_impl(_lib.ATTN_KERNEL_DQ, _lib.ATTN_MODE_NEW), attn_impl(_lib.ATTN_KERNEL_DKV, _lib.ATTN_MODE_NEW)
        want_bits = 0x10000 | _lib.ATTN_USED_DQ2 | _lib.ATTN_USED_DKV2
    elif form == "dq2+dkv128-head-split":
        attn_impl(_lib.ATTN_KERNEL_DQ, _lib.ATTN_MODE_NEW), attn_impl(_lib.ATTN_KERNEL_DKV, _lib.ATTN_MODE_AUTO)
        need = ops.attn_bwd_workspace_bytes(B, S, H, KV, HD, torch.bfloat16)
        assert need == 4 * B * S * KV * 128 * 4      # one slot per query head of a group
        kw["workspace"] = torch.full((need,), 255, dtype=torch.uint8, device=DEV)
        want_bits = 0x10000 | _lib.ATTN_USED_DQ2 | _lib.ATTN_USED_HEAD_SPLIT
    ex, ref = A.exact(case, *shape), None
    rs = A.f32_restated(ex) if fp32 else A.restated(case, *shape)
    if fused_rope:
        table, pos = _rope(shape)
        kw["rope_table"] = table.to(DEV)
        if fp32:
            rot = A.rope_transpose(ex["dqkv"], table, pos, H, KV)
            ref = (rot, rot.float().double())
        else:
            ref = A.rope_refs(ex, rs, table, pos, H, KV)
    d, used = _backward(ops, impl, x, dout, out, lse, shape, **kw)
    mask = 0x10000 | _lib.ATTN_USED_DQ2 | _lib.ATTN_USED_DKV2 | _lib.ATTN_USED_HEAD_SPLIT | _lib.ATTN_USED_PLAN
    assert (used & mask) == want_bits, f"{form}: dispatched {hex(used)}, wanted {hex(want_bits)}"
    A.check_all(None, None, d.cpu(), ex, rs, *shape, name=f"bwd {form} rope={fused_rope} {case} {shape}", eps=A.EPS_F32 if fp32 else A.EPS_BF16,
                ref_dqkv=ref, record=WORST.setdefault(f"backward {form}{' +rope' if fused_rope else ''}", {}))


@pytest.mark.parametrize("case,shape", PLAIN, ids=PLAIN_IDS)
def test_backward_switches_touch_their_own_blocks_only(ops, case, shape, attn_impl):
    """The dQ switch leaves the dK / dV blocks bit-identical and the dK / dV switch the dQ block, on these inputs too."""
    from ssi import _lib
    B, S, H, KV = shape
    x, dout = _inputs(case, shape)
    out, lse = _forward(ops, _lib.IMPL_MFMA, x, shape)
    res = {}
    for mq in (_lib.ATTN_MODE_OLD, _lib.ATTN_MODE_NEW):
        for mkv in (_lib.ATTN_MODE_OLD, _lib.ATTN_MODE_NEW):
            attn_impl(_lib.ATTN_KERNEL_DQ, mq), attn_impl(_lib.ATTN_KERNEL_DKV, mkv)
            d, used = _backward(ops, _lib.IMPL_MFMA, x, dout, out, lse, shape)
            assert bool(used & _lib.ATTN_USED_DQ2) == (mq == _lib.ATTN_MODE_NEW) and bool(used & _lib.ATTN_USED_DKV2) == (mkv == _lib.ATTN_MODE_NEW)
            res[mq, mkv] = d
    old, new = _lib.ATTN_MODE_OLD, _lib.ATTN_MODE_NEW
    for mkv in (old, new):
        assert torch.equal(res[old, mkv][:, H * HD:], res[new, mkv][:, H * HD:]), "the dK / dV blocks belong to the other kernel"
    for mq in (old, new):
        assert torch.equal(res[mq, old][:, : H * HD], res[mq, new][:, : H * HD]), "the dQ block belongs to the other kernel"


@pytest.mark.parametrize("fused_rope", [False, True], ids=["plain-epilogue", "fused-rope"])
@pytest.mark.parametrize("form", ["varlen", "plan", "plan-split-all"])
@pytest.mark.parametrize("case,rows", A.DOC_CASES, ids=DOC_IDS)
def test_packed_rows(ops, case, rows, form, fused_rope, attn_impl):
    """Packed rows at (2, 512, 4, 1): ssi_attn_varlen_fwd, then the plan-less varlen backward (the round-1..3 kernels with document arrays), the
    plan forms of the pipelined kernels (SSI_ATTN_PLAN_FORCE) and those with every dK/dV chunk split over the query heads
    (SSI_ATTN_PLAN_SPLIT_ALL).  In ``fall`` the keys of earlier documents hold a row's largest scores, in ``ramp8`` the later keys do; ``sink``
    is one document per row through the document forms."""
    from ssi import _lib, attn_plan
    shape = A.SHAPES[0]
    B, S, H, KV = shape
    rows = [list(r) for r in rows]
    docs = tuple(tuple(r) for r in rows)
    x, dout = _inputs(case, shape)
    ds, de, pos = (t.to(DEV) for t in A.doc_arrays(rows, S))
    ex, rs = A.exact(case, *shape, docs), A.restated(case, *shape, docs)
    out, lse = _forward(ops, _lib.IMPL_MFMA, x, shape, ds, de)
    name = f"packed {form} rope={fused_rope} {case}"
    A.check_all(out.cpu(), lse.cpu(), None, ex, rs, *shape, name=name, record=WORST.setdefault("forward mfma packed", {}))
    attn_impl(_lib.ATTN_KERNEL_DQ, _lib.ATTN_MODE_AUTO), attn_impl(_lib.ATTN_KERNEL_DKV, _lib.ATTN_MODE_AUTO)
    kw, ref = {"doc_start": ds, "doc_end": de}, None
    want_bits = 0x10000
    if form != "varlen":
        plan = attn_plan.plan_from_seq_lens(rows, H, KV, force=True, split_all=form == "plan-split-all")
        assert plan is not None and plan.matches(B, S, H, KV) and (plan.workspace_bytes > 0 or form == "plan")
        kw["plan"] = plan.to_device(DEV)
        want_bits |= _lib.ATTN_USED_DQ2 | _lib.ATTN_USED_DKV2 | _lib.ATTN_USED_PLAN | (_lib.ATTN_USED_HEAD_SPLIT if plan.workspace_bytes > 0 else 0)
    if fused_rope:
        table, hpos = _rope(shape, rows)
        kw["rope_table"], kw["positions"] = table.to(DEV), pos
        ref = A.rope_refs(ex, rs, table, hpos, H, KV)
    d, used = _backward(ops, _lib.IMPL_MFMA, x, dout, out, lse, shape, **kw)
    mask = 0x10000 | _lib.ATTN_USED_DQ2 | _lib.ATTN_USED_DKV2 | _lib.ATTN_USED_HEAD_SPLIT | _lib.ATTN_USED_PLAN
    assert (used & mask) == want_bits, f"{form}: dispatched {hex(used)}, wanted {hex(want_bits)}"
    A.check_all(None, None, d.cpu(), ex, rs, *shape, name=name, ref_dqkv=ref,
                record=WORST.setdefault(f"backward packed {form}{' +rope' if fused_rope else ''}", {}))
