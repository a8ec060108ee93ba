"""GPU: the KL term against a frozen teacher inside the cross-entropy kernels (``ssi_ce_fwd_kl``, ``ops.ce_fwd_kl``; ABI v15).

Per valid row, with the student row ``x``, the teacher row ``t``, ``p = softmax(x)``, ``q = softmax(t)``, the row's weight ``w``, its KL weight
``k`` (``row_kl_weight``, or ``w``) and the coefficient ``b``: ``row_loss`` and ``row_lse`` are those of ``ops.ce_fwd`` BIT FOR BIT,
``row_kl = k KL(q || p)`` in fp32 (the coefficient not applied), and the gradient row is ``(w + b k) p - w onehot - b k q``.  ``b = 0`` is
``ops.ce_fwd`` bit for bit.  ``teacher_lse`` is what ``ops.ce_fwd(teacher, ..., write_grad=False)`` writes as ``row_lse``.

The reference is torch in fp64 on the stored values with autograd for the gradient.  Shapes, inputs and gradient tolerances are those of
``tests/test_ce_z_gpu.py``, the atol times ``max(1, w + b k)`` of the row (the magnitude the kernel stores); ``row_kl`` is held to rtol 2e-5 and
atol 2e-5 ``max(1, k)``, the bound ``row_u`` of the smoothing form is held to (the same ``lse - sum`` structure).  Three teachers per shape:
``near`` (the student + 0.5 randn: KL 0.03 to 0.24 per row), ``far`` (an independent 3 randn: KL 5 to 15) and ``same`` (a copy: KL 0).  The two
buffers' pad columns hold different large values."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_ce_z_gpu import ROWS, SHAPES, TOL, is_valid, make_inputs, run_plain

pytestmark = pytest.mark.gpu

DEV = "cuda"
BETAS = (0.1, 2.0)
KL_RTOL, KL_ATOL = 2e-5, 2e-5
TEACHERS = ("near", "far", "same")
NEAR_RANGE = (0.03, 0.24)           # fp64 KL of the valid near rows of SHAPES (24 rows each), worked out on the CPU; asserted on the reference


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


def make_teacher(logits, vocab, kind, seed):
    g = torch.Generator().manual_seed(seed + 1002)           # (with this offset the near rows of every shape of SHAPES lie in NEAR_RANGE)
    if kind == "near":
        t = logits.float() + 0.5 * torch.randn(logits.shape, generator=g)
    elif kind == "far":
        t = 3.0 * torch.randn(logits.shape, generator=g)
    else:
        t = logits.float().clone()
    t[:, vocab:] = -3e4                                      # the teacher's pad columns: another value than the student's 1e4
    return t.to(logits.dtype)


def teacher_lse_of(ops, teacher, labels, vocab):
    rows = teacher.shape[0]
    loss, lse = torch.full((rows,), 7.0, device=DEV), torch.full((rows,), 7.0, device=DEV)
    ops.ce_fwd(teacher, labels.to(DEV), vocab, -100, loss, lse, False)
    return lse


def run_kl(ops, logits, teacher, labels, vocab, w, k, beta, write_grad, with_lse=True, teacher_dev=None):
    """(buffer, row_loss, row_lse, row_kl, the teacher buffer after the call)"""
    rows = logits.shape[0]
    work = logits.to(DEV)
    tdev = teacher.to(DEV) if teacher_dev is None else teacher_dev
    tl = teacher_lse_of(ops, tdev, labels, vocab)
    loss, rk = torch.full((rows,), 7.0, device=DEV), torch.full((rows,), 7.0, device=DEV)
    lse = torch.full((rows,), 7.0, device=DEV) if with_lse else None
    ops.ce_fwd_kl(work, tdev, tl, labels.to(DEV), vocab, -100, beta, loss, lse, rk, write_grad,
                  row_weight=None if w is None else w.to(DEV), row_kl_weight=None if k is None else k.to(DEV))
    return work, loss, lse, rk, tdev


def reference(logits, teacher, labels, vocab, w, k, beta):
    """torch in fp64: (row_kl [rows] with k applied, the row's w + beta k, gradient [rows, vocab] of sum_r w nll + beta k KL); rows without a
    valid label are 0."""
    x = logits[:, :vocab].double().requires_grad_(True)
    t = teacher[:, :vocab].double()
    valid = is_valid(labels, vocab)
    y = torch.where(valid, labels, torch.full_like(labels, -100))
    wd = torch.ones(x.shape[0], dtype=torch.float64) if w is None else w.double()
    kd = wd if k is None else k.double()
    nll = F.cross_entropy(x, y, reduction="none", ignore_index=-100)
    kl = F.kl_div(F.log_softmax(x, dim=1), F.log_softmax(t, dim=1), log_target=True, reduction="none").sum(dim=1)
    ((wd * nll + beta * kd * kl) * valid).sum().backward()
    return torch.where(valid, kd * kl.detach(), torch.zeros_like(kd)), wd + beta * kd, kd, x.grad


def check_kl(got, want, kd, what):
    err = (got.cpu().double() - want).abs()
    bound = KL_ATOL * kd.clamp(min=1.0) + KL_RTOL * want.abs()
    print(f"[{what}] row_kl in [{float(want.min()):.4f}, {float(want.max()):.4f}], max |err| {float(err.max()):.3e}, "
          f"worst err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), what


def check_gradient(got, want, scale, dtype, what):
    rtol, atol = TOL[dtype]
    err = (got.double() - want).abs()
    bound = atol * scale.clamp(min=1.0)[:, None] + rtol * want.abs()
    worst = float((err / bound).max())
    print(f"[{what}] max |err| {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert worst <= 1.0, what


def same_ce(a, b, bits):
    """row_loss / row_lse against ``ops.ce_fwd``'s: bit for bit where both calls take the same form; rtol 2e-5, atol 2e-5 (the bound
    ``tests/test_kernels_gpu.py::test_cross_entropy_with_a_weight_per_row`` holds row_loss to) where the KL call takes the generic form and
    ``ops.ce_fwd`` the register form."""
    if bits:
        return torch.equal(a, b)
    torch.testing.assert_close(a, b, rtol=2e-5, atol=2e-5)
    return True


def check_all(ops, logits, labels, vocab, w, dtype, seed, teacher_of=None, near_floor=False, bits=True):
    """``near_floor``: the inputs are those of SHAPES, whose near rows have a KL inside NEAR_RANGE: the kernel's row_kl with k = 1 is then held
    above 0.02 on every valid row — the term is not rounding error.  (Other inputs, 600 peaked rows among them, have near rows below that.)"""
    valid = is_valid(labels, vocab)
    plain = {wg: run_plain(ops, logits, labels, vocab, w, wg) for wg in (False, True)}
    for kind in TEACHERS:
        teacher = make_teacher(logits, vocab, kind, seed)
        tdev_of = (lambda: None) if teacher_of is None else (lambda: teacher_of(teacher))
        kl64, _, kd, _ = reference(logits, teacher, labels, vocab, w, None, 0.0)
        # beta = 0: the buffer, row_loss and row_lse of ce_fwd for both write_grad; row_kl is still written
        for wg in (False, True):
            work, loss, lse, rk, tdev = run_kl(ops, logits, teacher, labels, vocab, w, None, 0.0, wg, teacher_dev=tdev_of())
            if bits:
                assert torch.equal(work, plain[wg][0]), f"{kind}: beta = 0, write_grad {wg}: the buffer differs from ce_fwd"
            assert same_ce(loss, plain[wg][1], bits) and same_ce(lse, plain[wg][2], bits)
            check_kl(rk, kl64, kd, f"{kind} beta 0 write_grad {wg} weights {w is not None}")
            assert (rk.cpu()[~valid] == 0).all()
        for beta in BETAS:
            kl64, scale, kd, grad64 = reference(logits, teacher, labels, vocab, w, None, beta)
            for wg in (False, True):
                work, loss, lse, rk, tdev = run_kl(ops, logits, teacher, labels, vocab, w, None, beta, wg, teacher_dev=tdev_of())
                assert same_ce(loss, plain[wg][1], bits) and same_ce(lse, plain[wg][2], bits), f"{kind} beta {beta}: row_loss / row_lse differ from ce_fwd"
                assert torch.equal(tdev.cpu(), teacher), "the teacher buffer was written"
                what = f"{kind} beta {beta} write_grad {wg} weights {w is not None}"
                check_kl(rk, kl64, kd, what)
                if kind == "same":
                    assert (rk.cpu().double().abs() <= KL_ATOL * kd.clamp(min=1.0)).all(), "KL of a distribution against itself"
                if kind == "near" and w is None and near_floor:
                    assert (kl64[valid] >= NEAR_RANGE[0]).all() and (kl64[valid] <= NEAR_RANGE[1]).all(), "the inputs are not the ones intended"
                    assert (rk.cpu()[valid] > 0.02).all(), "the near teacher's KL is not above rounding error"
                for out in (loss, lse, rk):
                    assert (out.cpu()[~valid] == 0).all(), "a row without a valid label is not 0 in every output"
                if not wg:
                    assert torch.equal(work.cpu(), logits), "write_grad = 0 wrote the logits"
                    continue
                grad = work.cpu().float()
                check_gradient(grad[:, :vocab], grad64, scale, dtype, what)
                assert (grad[:, vocab:] == 0).all(), "pad columns"
                assert (grad[~valid] == 0).all(), "rows without a valid label"
                again = run_kl(ops, logits, teacher, labels, vocab, w, None, beta, True, teacher_dev=tdev_of())
                assert torch.equal(again[0], work) and torch.equal(again[3], rk), "not bitwise reproducible"
            no_lse = run_kl(ops, logits, teacher, labels, vocab, w, None, beta, True, with_lse=False, teacher_dev=tdev_of())   # row_lse = NULL
            assert torch.equal(no_lse[0], work) and torch.equal(no_lse[1], loss) and torch.equal(no_lse[3], rk)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("vocab,ld,dtype", SHAPES)
def test_kl_forms_against_ce_fwd_bits_and_fp64(ops, vocab, ld, dtype, weighted):
    logits, labels, w = make_inputs(ROWS, vocab, ld, dtype, seed=vocab)
    check_all(ops, logits, labels, vocab, w if weighted else None, dtype, seed=vocab, near_floor=True)


@pytest.mark.parametrize("weighted", [False, True])
def test_many_rows_per_workgroup_with_ignored_stretches(ops, weighted):
    """The layout of ``tests/test_ce_z_gpu.py::test_many_rows_per_workgroup_with_ignored_stretches``: 600 rows, each workgroup walks several, the
    next row's prefetch beside the teacher's loads."""
    rows, vocab, ld, dtype = 600, 515, 520, torch.bfloat16
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert rows >= 2 * cus, f"{rows} rows on {cus} CUs: no workgroup walks several rows"
    logits, labels, w = make_inputs(rows, vocab, ld, dtype, seed=77)
    labels[0], labels[rows - 1] = -100, -100
    labels[::7] = -100
    labels[100:140] = -100
    labels[cus:cus + 3] = -100                               # the second row of the first workgroups
    labels[200], labels[413] = vocab + 2, -1
    check_all(ops, logits, labels, vocab, w if weighted else None, dtype, seed=77)


@pytest.mark.parametrize("vocab,ld,dtype", [(9000, 9216, torch.bfloat16), (515, 520, torch.float32)])
def test_a_teacher_with_its_own_row_stride(ops, vocab, ld, dtype):
    """``ld_teacher != ld``: the teacher is a view of a wider buffer (in bf16 the generic form, where equal strides take the register form)."""
    logits, labels, w = make_inputs(ROWS, vocab, ld, dtype, seed=5)

    def wider(teacher):
        big = torch.full((ROWS, ld + 64), 77.0, dtype=dtype, device=DEV)
        view = big[:, :ld]
        view.copy_(teacher)
        assert view.stride(0) == ld + 64
        return view

    # (in bf16 ``ops.ce_fwd`` on the student alone takes the register form: its row_loss / row_lse are close to the generic form's, not equal)
    check_all(ops, logits, labels, vocab, w, dtype, seed=5, teacher_of=wider, bits=dtype == torch.float32)


@pytest.mark.parametrize("vocab,ld,dtype", SHAPES)
def test_a_kl_weight_per_row(ops, vocab, ld, dtype):
    """``row_kl_weight`` given: w > 0, k = 0 is the pure CE row of beta = 0, bit for bit; w = 0, k > 0 has gradient ``beta k (p - q)`` and
    row_loss 0; both 0 is an all-zero row."""
    beta = 2.0
    logits, labels, w = make_inputs(ROWS, vocab, ld, dtype, seed=vocab)
    teacher = make_teacher(logits, vocab, "far", vocab)
    valid = is_valid(labels, vocab)
    g = torch.Generator().manual_seed(3)
    k = 2.0 * torch.rand(ROWS, generator=g)
    rows_ce, rows_kl, rows_none = (6, 9), (4, 10), (7, 12)   # make_inputs: w[6] = 1, w[4] = w[7] = 0
    for r in rows_ce:
        k[r] = 0.0
    for r in rows_kl:
        w[r], k[r] = 0.0, 1.5
    for r in rows_none:
        w[r], k[r] = 0.0, 0.0
    assert all(bool(valid[r]) and float(w[r]) > 0 for r in rows_ce) and all(bool(valid[r]) for r in rows_kl + rows_none)
    kl64, scale, kd, grad64 = reference(logits, teacher, labels, vocab, w, k, beta)
    work, loss, lse, rk, _ = run_kl(ops, logits, teacher, labels, vocab, w, k, beta, True)
    plain, ploss, plse = run_plain(ops, logits, labels, vocab, w, True)
    assert torch.equal(loss, ploss) and torch.equal(lse, plse)
    check_kl(rk, kl64, kd, "row_kl_weight")
    grad = work.cpu().float()
    check_gradient(grad[:, :vocab], grad64, scale, dtype, "row_kl_weight")
    assert (grad[:, vocab:] == 0).all() and (grad[~valid] == 0).all()
    for r in rows_ce:
        assert torch.equal(work[r], plain[r]), f"row {r}: k = 0 is not the CE row bit for bit"
        assert float(rk[r]) == 0.0
    x, t = logits[:, :vocab].double(), teacher[:, :vocab].double()
    for r in rows_kl:
        want = beta * float(k[r]) * (torch.softmax(x[r], 0) - torch.softmax(t[r], 0))
        check_gradient(grad[r:r + 1, :vocab], want[None], scale[r:r + 1], dtype, f"row {r}: w = 0, k > 0")
        assert float(loss[r]) == 0.0 and float(rk[r]) > 1.0
        assert float(grad[r, :vocab].abs().max()) > 0
    for r in rows_none:
        assert (grad[r] == 0).all() and float(loss[r]) == 0.0 and float(rk[r]) == 0.0


def test_a_hand_made_row_the_tolerance_cannot_hide(ops):
    """vocab 8, fp32, the student all zeros (p = 1/8), the teacher [ln 4, 0, ...] (q = [4/11, 1/11, ...], lse = ln 11), label 1, w = k = beta = 1:
    row_kl = (4/11) ln 4 - ln 11 + ln 8 and the gradient 2/8 - [c == 1] - q[c].  A dropped q term or a wrong sign is off by 0.09 or more."""
    vocab = 8
    logits = torch.zeros(1, vocab)
    teacher = torch.zeros(1, vocab)
    teacher[0, 0] = math.log(4.0)
    labels = torch.tensor([1])
    work, loss, lse, rk, tdev = run_kl(ops, logits, teacher, labels, vocab, None, None, 1.0, True)
    tl = teacher_lse_of(ops, tdev, labels, vocab)
    assert float(tl[0]) == pytest.approx(math.log(11.0), rel=1e-6)
    assert float(lse[0]) == pytest.approx(math.log(8.0), rel=1e-6) and float(loss[0]) == pytest.approx(math.log(8.0), rel=1e-6)
    assert float(rk[0]) == pytest.approx((4.0 / 11.0) * math.log(4.0) - math.log(11.0) + math.log(8.0), rel=1e-6, abs=1e-7)
    q = torch.full((vocab,), 1.0 / 11.0, dtype=torch.float64)
    q[0] = 4.0 / 11.0
    want = 2.0 / 8.0 - q
    want[1] -= 1.0
    print("gradient", work.cpu()[0].tolist(), "want", want.tolist())
    torch.testing.assert_close(work.cpu()[0].double(), want, rtol=1e-6, atol=1e-7)


def test_invalid_arguments_raise_and_launch_nothing(ops):
    vocab, ld = 515, 520
    logits, labels, _ = make_inputs(ROWS, vocab, ld, torch.float32, seed=1)
    teacher = make_teacher(logits, vocab, "near", 1)
    lab = labels.to(DEV)

    def fresh():
        return (logits.to(DEV), teacher.to(DEV), torch.zeros(ROWS, device=DEV), torch.full((ROWS,), 7.0, device=DEV),
                torch.full((ROWS,), 7.0, device=DEV))

    for bad in (-1e-4, float("nan"), float("inf")):
        work, tdev, tl, loss, rk = fresh()
        with pytest.raises(RuntimeError, match="kl_coeff must be finite and >= 0"):
            ops.ce_fwd_kl(work, tdev, tl, lab, vocab, -100, bad, loss, None, rk, True)
        assert torch.equal(work.cpu(), logits) and (loss == 7.0).all() and (rk == 7.0).all(), "a refused call launched"
    work, tdev, tl, loss, rk = fresh()
    with pytest.raises(RuntimeError):                        # teacher == logits
        ops.ce_fwd_kl(work, work, tl, lab, vocab, -100, 0.5, loss, None, rk, True)
    assert torch.equal(work.cpu(), logits) and (loss == 7.0).all() and (rk == 7.0).all()
    from ssi import _lib
    from ssi.ops import ptr, stream_ptr
    lib = _lib.load()

    def raw(teacher_p, tl_p, rk_p, ld_t=ld):
        return lib.ssi_ce_fwd_kl(ptr(work), ld, teacher_p, ld_t, tl_p, ptr(lab), None, None, ROWS, vocab, -100, 0.5, ptr(loss), None, rk_p, 1, 0,
                                 stream_ptr())

    assert raw(None, ptr(tl), ptr(rk)) == 1 and raw(ptr(tdev), None, ptr(rk)) == 1 and raw(ptr(tdev), ptr(tl), None) == 1   # SSI_ERR_ARG
    assert raw(ptr(tdev), ptr(tl), ptr(rk), ld_t=512) == 1, "a teacher stride below the vocabulary"
    torch.cuda.synchronize()
    assert torch.equal(work.cpu(), logits) and (loss == 7.0).all() and (rk == 7.0).all()
    assert raw(ptr(tdev), ptr(tl), ptr(rk)) == 0             # and the same call with every argument in place runs


def test_abi_version():
    from ssi import _lib
    assert _lib.load().ssi_abi_version() >= 15
