"""GPU: the cross-entropy kernels with the auxiliary z-loss ``z * log^2 Z`` (``ssi_ce_fwd_z``, ``ops.ce_fwd_z``; ABI v12).

Per valid row, with ``lse = logsumexp(x[0:vocab])``, ``p = softmax(x)`` and the row's weight ``w``:
``row_loss = w (lse - x[y])`` and ``row_lse`` are those of ``ops.ce_fwd`` BIT FOR BIT, ``row_z = w (lse lse)`` in fp32 (the coefficient not
applied), and the gradient row is ``w (f p - onehot)`` with ``f = 1 + 2 z lse`` — of any sign.  ``z = 0`` is ``ops.ce_fwd`` bit for bit.
The reference is torch in fp64 on the stored values (bf16 inputs upcast).  Gradient tolerances: those of
``tests/test_kernels_gpu.py::test_cross_entropy_with_a_weight_per_row`` (fp32 rtol 5e-5 atol 1e-6, bf16 rtol 1e-2 atol 4e-3), the atol times
``max(1, |f|) max(1, w)`` of the row: the rounding scales with the magnitude the kernel stores."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS = 24
# (vocab, ld, dtype) -> the path taken: generic fp32; register form with 1 chunk; 2 chunks with pad columns ending chunk 0 and filling the whole
# lane range of chunk 1; 2 chunks with pad columns in chunk 1 only; 5 chunks (no register form: the generic kernel in bf16); 17 chunks, the step's form
SHAPES = [(515, 520, torch.float32), (515, 520, torch.bfloat16), (8000, 8200, torch.bfloat16), (9000, 9216, torch.bfloat16),
          (40_000, 40_960, torch.bfloat16), (133_258, 133_376, torch.bfloat16)]
TOL = {torch.float32: (5e-5, 1e-6), torch.bfloat16: (1e-2, 4e-3)}   # (rtol, atol) of test_cross_entropy_with_a_weight_per_row
Z_COEFFS = (1e-4, 0.5)


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


def make_inputs(rows, vocab, ld, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(rows, ld, generator=g) * 3.0)
    logits[:, vocab:] = 1e4                                  # pad columns [vocab, ld): must change nothing
    logits = logits.to(dtype)
    labels = torch.randint(0, vocab, (rows,), generator=g)
    labels[3], labels[rows - 1] = -100, -100
    labels[5], labels[11] = vocab, -7                        # out of range above (a pad column's index) and below
    labels[1], labels[2] = 0, vocab - 1                      # the ends of the row
    w = 3.0 * torch.rand(rows, generator=g)                  # weights in [0, 3], some exactly 0 and 1
    w[4], w[6], w[7], w[8] = 0.0, 1.0, 0.0, 1.0
    return logits, labels, w


def is_valid(labels, vocab):
    return (labels != -100) & (labels >= 0) & (labels < vocab)


def reference(logits, labels, vocab, w, z):
    """fp64: (row_z [rows], f [rows], gradient [rows, vocab]); ignored / out-of-range rows 0 (their f is reported as 1)."""
    x = logits[:, :vocab].double()
    valid = is_valid(labels, vocab)
    lse = torch.logsumexp(x, dim=1)
    p = torch.exp(x - lse[:, None])
    f = 1.0 + 2.0 * z * lse
    onehot = torch.zeros_like(p)
    onehot[valid, labels[valid]] = 1.0
    wd = torch.ones(x.shape[0], dtype=torch.float64) if w is None else w.double()
    grad = wd[:, None] * (f[:, None] * p - onehot)
    grad[~valid] = 0.0
    return torch.where(valid, wd * lse * lse, torch.zeros_like(lse)), torch.where(valid, f, torch.ones_like(f)), grad


def run_plain(ops, logits, labels, vocab, w, write_grad):
    rows = logits.shape[0]
    work = logits.to(DEV)
    loss, lse = torch.full((rows,), 7.0, device=DEV), torch.full((rows,), 7.0, device=DEV)
    ops.ce_fwd(work, labels.to(DEV), vocab, -100, loss, lse, write_grad, row_weight=None if w is None else w.to(DEV))
    return work, loss, lse


def run_z(ops, logits, labels, vocab, w, z, write_grad, with_lse=True):
    rows = logits.shape[0]
    work = logits.to(DEV)
    loss, rz = torch.full((rows,), 7.0, device=DEV), torch.full((rows,), 7.0, device=DEV)
    lse = torch.full((rows,), 7.0, device=DEV) if with_lse else None
    ops.ce_fwd_z(work, labels.to(DEV), vocab, -100, z, loss, lse, rz, write_grad, row_weight=None if w is None else w.to(DEV))
    return work, loss, lse, rz


def check_gradient(got, want, f, w, dtype, what):
    rtol, atol = TOL[dtype]
    scale = f.abs().clamp(min=1.0) * (torch.ones_like(f) if w is None else w.double().clamp(min=1.0))
    err = (got.double() - want).abs()
    bound = atol * scale[:, None] + rtol * want.abs()
    worst = float((err / bound).max())
    print(f"[{what}] max |err| {float(err.max()):.3e}, worst err / bound {worst:.3f}, max |f| {float(f.abs().max()):.3f}")
    assert worst <= 1.0, what


def check_all(ops, logits, labels, vocab, w, dtype):
    """Checks 1-3 of the module docstring on one input, with the row weights ``w`` or without (None)."""
    valid = is_valid(labels, vocab)
    wdev = torch.ones(logits.shape[0], device=DEV) if w is None else w.to(DEV)
    plain = {wg: run_plain(ops, logits, labels, vocab, w, wg) for wg in (False, True)}
    assert torch.equal(plain[False][0].cpu(), logits)
    # 1. z = 0: the buffer, row_loss and row_lse of ce_fwd, for write_grad 0 and 1
    for wg in (False, True):
        work, loss, lse, rz = run_z(ops, logits, labels, vocab, w, 0.0, wg)
        assert torch.equal(work, plain[wg][0]), f"z = 0, write_grad {wg}: the buffer differs from ce_fwd"
        assert torch.equal(loss, plain[wg][1]) and torch.equal(lse, plain[wg][2])
        assert torch.equal(rz, wdev * (lse * lse)), "row_z is written with z = 0 too"
    for z in Z_COEFFS:
        rz64, f64, grad64 = reference(logits, labels, vocab, w, z)
        for wg in (False, True):
            work, loss, lse, rz = run_z(ops, logits, labels, vocab, w, z, wg)
            # 2. the CE outputs do not see z; row_z is w (lse lse) in fp32, in this order
            assert torch.equal(loss, plain[wg][1]) and torch.equal(lse, plain[wg][2]), f"z = {z}: row_loss / row_lse differ from ce_fwd"
            assert torch.equal(rz, wdev * (lse * lse)), f"z = {z}: row_z is not w * (lse * lse) in fp32"
            torch.testing.assert_close(rz.cpu().double(), rz64, rtol=1e-5, atol=0)
            assert (rz.cpu()[~valid] == 0).all() and (loss.cpu()[~valid] == 0).all()
            if not wg:
                assert torch.equal(work.cpu(), logits), "write_grad = 0 wrote the logits"
                continue
            # 3. the gradient against fp64; pad columns and the rows without a valid label exactly 0
            grad = work.cpu().float()
            check_gradient(grad[:, :vocab], grad64, f64, w, dtype, f"z {z} weights {w is not None}")
            assert (grad[:, vocab:] == 0).all(), "pad columns"
            assert (grad[~valid] == 0).all(), "rows without a valid label"
            again = run_z(ops, logits, labels, vocab, w, z, True)
            assert torch.equal(again[0], work) and torch.equal(again[3], rz), "not bitwise reproducible"
        no_lse = run_z(ops, logits, labels, vocab, w, z, True, with_lse=False)   # row_lse = NULL
        assert torch.equal(no_lse[0], work) and torch.equal(no_lse[1], loss) and torch.equal(no_lse[3], rz)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("vocab,ld,dtype", SHAPES)
def test_z_forms_against_ce_fwd_bits_and_fp64(ops, vocab, ld, dtype, weighted):
    logits, labels, w = make_inputs(ROWS, vocab, ld, dtype, seed=vocab)
    check_all(ops, logits, labels, vocab, w if weighted else None, dtype)


@pytest.mark.parametrize("weighted", [False, True])
def test_many_rows_per_workgroup_with_ignored_stretches(ops, weighted):
    """600 rows on one workgroup per CU: each walks several rows, the next row's loads issued under the current row's gradient; stretches of
    ignored labels (a workgroup meets several in a row), the first and the last row among them, and two out-of-range labels."""
    rows, vocab, ld, dtype = 600, 515, 520, torch.bfloat16
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert rows >= 2 * cus, f"{rows} rows on {cus} CUs: no workgroup walks several rows"
    logits, labels, w = make_inputs(rows, vocab, ld, dtype, seed=77)
    labels[0], labels[rows - 1] = -100, -100
    labels[::7] = -100
    labels[100:140] = -100
    labels[cus:cus + 3] = -100                               # the second row of the first workgroups
    labels[200], labels[413] = vocab + 2, -1
    check_all(ops, logits, labels, vocab, w if weighted else None, dtype)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("vocab,ld,dtype", SHAPES)
def test_the_sign_of_f_on_hand_made_rows(ops, vocab, ld, dtype, weighted):
    """z = 0.5, rows of values exact in bf16: ``HOT`` columns at one value (spread over the row: column 0, the last real column, every chunk),
    the rest at -200 (their exp underflows to 0 in fp32), so lse = value + ln(HOT) (or = value exactly with one hot column).
      rows 0, 1: value -5.65625, 64 hot -> lse = -1.4974, f = -0.497 < 0: every hot non-label column is NEGATIVE (label hot / label cold);
      rows 2, 3: one hot column at -1  -> lse = -1 and f = 0 exactly in fp32: 0 off the label and -w on it (label cold / label hot);
      row 4:     value 2, 64 hot       -> f = 7.16 > 0, the plain case."""
    z, hot_n = 0.5, 64
    hot = torch.linspace(0, vocab - 1, hot_n).round().long()
    assert hot[0] == 0 and hot[-1] == vocab - 1 and hot.unique().numel() == hot_n
    cold = int(hot[1]) + 1
    assert cold not in set(hot.tolist())
    x = torch.full((5, ld), -200.0)
    x[0, hot] = x[1, hot] = -5.65625
    x[2, 7] = x[3, 7] = -1.0
    x[4, hot] = 2.0
    x[:, vocab:] = 8192.0                                    # pad columns (exact in bf16): must change nothing
    labels = torch.tensor([int(hot[hot_n // 2]), cold, cold, 7, int(hot[-1])])
    logits = x.to(dtype)
    assert torch.equal(logits.float(), x), "the rows are not exact in this dtype"
    w = torch.tensor([1.0, 2.5, 0.5, 3.0, 1.5]) if weighted else None
    wv = torch.ones(5) if w is None else w
    rz64, f64, grad64 = reference(logits, labels, vocab, w, z)
    print("reference f:", f64.tolist())
    assert f64[0] < -0.49 and f64[1] < -0.49 and f64[2] == 0.0 and f64[3] == 0.0 and f64[4] > 7.0   # the intended signs, before use
    work, loss, lse, rz = run_z(ops, logits, labels, vocab, w, z, True)
    _, loss_plain, lse_plain = run_plain(ops, logits, labels, vocab, w, True)
    assert torch.equal(loss, loss_plain) and torch.equal(lse, lse_plain)
    assert lse.cpu()[2] == -1.0 and lse.cpu()[3] == -1.0, "lse of the f == 0 rows is not exactly -1 in fp32"
    torch.testing.assert_close(rz.cpu().double(), rz64, rtol=1e-5, atol=0)
    grad = work.cpu().float()
    check_gradient(grad[:, :vocab], grad64, f64, w, dtype, f"hand-made rows, weights {weighted}")
    assert (grad[:, vocab:] == 0).all(), "pad columns"
    for r in (0, 1):                                         # f < 0
        others = hot[hot != labels[r]]
        assert (grad[r, others] < 0).all(), f"row {r}: f < 0 but a hot non-label column is not negative"
        assert (grad[r, :vocab] <= 0).all()
    assert float(grad[0, labels[0]]) == pytest.approx(float(wv[0]) * (float(f64[0]) / hot_n - 1.0), rel=1e-2)
    assert float(grad[1, labels[1]]) == -float(wv[1])        # a cold label: p = 0 there
    for r in (2, 3):                                         # f == 0: zero off the label, -w on it
        off = torch.ones(vocab, dtype=torch.bool)
        off[labels[r]] = False
        assert (grad[r, :vocab][off] == 0).all(), f"row {r}: f == 0 but a non-label column is not 0"
        assert float(grad[r, labels[r]]) == -float(wv[r])
    others = hot[hot != labels[4]]
    assert (grad[4, others] > 0).all() and float(grad[4, labels[4]]) < 0


def test_bad_coefficients_raise_with_the_entrys_message(ops):
    logits, labels, _ = make_inputs(ROWS, 515, 520, torch.float32, seed=1)
    for bad in (-1e-4, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="z_coeff must be finite and >= 0"):
            run_z(ops, logits, labels, 515, None, bad, True)


def test_abi_version():
    from ssi import _lib
    assert _lib.load().ssi_abi_version() >= 12
