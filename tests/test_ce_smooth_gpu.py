"""GPU: label smoothing inside the cross-entropy kernels (``ssi_ce_fwd_smooth``, ``ops.ce_fwd_smooth``; ABI v14).

Per valid row, with smoothing ``e``, ``lse = logsumexp(x[0:vocab])``, ``p = softmax(x)``, the row's weight ``w`` and ``f = 1 + 2 z lse``:
``row_loss`` and ``row_lse`` are those of ``ops.ce_fwd`` and ``row_z`` that of ``ops.ce_fwd_z`` BIT FOR BIT, ``row_u = w (lse - mean_c x[c])`` in
fp32 (the coefficient not applied), and the gradient row is ``w (f p - (1 - e) onehot) - w e / vocab`` on the real columns.  ``e = 0`` is
``ops.ce_fwd_z`` bit for bit, and with ``z = 0`` as well ``ops.ce_fwd``.

The reference is torch's own ``F.cross_entropy(x[:, :vocab].double(), y, label_smoothing=e, ignore_index=-100)`` and its autograd gradient on the
stored values (out-of-range labels mapped to ignored), the z part added as ``tests/test_ce_z_gpu.py::reference`` does.  Shapes, inputs and
gradient tolerances are those of ``tests/test_ce_z_gpu.py``; ``row_u`` and the summed loss are held to rtol 2e-5, atol 2e-5, the bound
``tests/test_kernels_gpu.py::test_cross_entropy_with_a_weight_per_row`` holds ``row_loss`` to.  In bf16 the gradient's atol of 4e-3 is 20 to
5000 times ``e / vocab``: ``test_the_uniform_term_exactly_on_hand_made_rows`` is the check that a forgotten ``- e / vocab`` cannot pass."""
import pytest
import torch
import torch.nn.functional as F

from test_ce_z_gpu import ROWS, SHAPES, check_gradient, is_valid, make_inputs, run_plain, run_z

pytestmark = pytest.mark.gpu

DEV = "cuda"
SMOOTHINGS = (0.1, 0.5)
Z_COEFFS = (0.0, 1e-4, 0.5)
U_TOL = dict(rtol=2e-5, atol=2e-5)


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


def run_smooth(ops, logits, labels, vocab, w, e, z, write_grad, with_lse=True, with_z=True):
    rows = logits.shape[0]
    work = logits.to(DEV)
    loss, ru = torch.full((rows,), 7.0, device=DEV), torch.full((rows,), 7.0, device=DEV)
    lse = torch.full((rows,), 7.0, device=DEV) if with_lse else None
    rz = torch.full((rows,), 7.0, device=DEV) if with_z else None
    ops.ce_fwd_smooth(work, labels.to(DEV), vocab, -100, e, z, loss, lse, ru, rz, write_grad, row_weight=None if w is None else w.to(DEV))
    return work, loss, lse, ru, rz


def reference(logits, labels, vocab, w, e, z):
    """torch in fp64: (summed objective without the z part, row_u [rows], f [rows], gradient [rows, vocab] of the objective WITH the z part);
    rows without a valid label are 0 (their f is reported as 1)."""
    x = logits[:, :vocab].double().requires_grad_(True)
    valid = is_valid(labels, vocab)
    y = torch.where(valid, labels, torch.full_like(labels, -100))
    wd = torch.ones(x.shape[0], dtype=torch.float64) if w is None else w.double()
    if w is None:
        total = F.cross_entropy(x, y, reduction="sum", label_smoothing=e, ignore_index=-100)
    else:
        total = (wd * F.cross_entropy(x, y, reduction="none", label_smoothing=e, ignore_index=-100)).sum()
    lse = torch.logsumexp(x, dim=1)
    (total + z * (wd * lse * lse * valid).sum()).backward()
    with torch.no_grad():
        f = 1.0 + 2.0 * z * lse
        u = torch.where(valid, wd * (lse - x.mean(dim=1)), torch.zeros_like(lse))
    return total.detach(), u, torch.where(valid, f, torch.ones_like(f)).detach(), x.grad


def check_all(ops, logits, labels, vocab, w, dtype):
    """Checks 1-3 of the issue on one input, with the row weights ``w`` or without (None)."""
    valid = is_valid(labels, vocab)
    plain = {wg: run_plain(ops, logits, labels, vocab, w, wg) for wg in (False, True)}
    _, u64, _, _ = reference(logits, labels, vocab, w, 0.0, 0.0)
    # 1. the corners: e = 0 is ce_fwd_z bit for bit, for each z and write_grad; e = 0 and z = 0 is ce_fwd; row_u is written in every case
    for z in Z_COEFFS:
        for wg in (False, True):
            zw, zloss, zlse, zrz = run_z(ops, logits, labels, vocab, w, z, wg)
            work, loss, lse, ru, rz = run_smooth(ops, logits, labels, vocab, w, 0.0, z, wg)
            assert torch.equal(work, zw), f"e = 0, z = {z}, write_grad {wg}: the buffer differs from ce_fwd_z"
            assert torch.equal(loss, zloss) and torch.equal(lse, zlse) and torch.equal(rz, zrz)
            if z == 0.0:
                assert torch.equal(work, plain[wg][0]), f"e = 0, z = 0, write_grad {wg}: the buffer differs from ce_fwd"
                assert torch.equal(loss, plain[wg][1]) and torch.equal(lse, plain[wg][2])
            torch.testing.assert_close(ru.cpu().double(), u64, **U_TOL)
            assert (ru.cpu()[~valid] == 0).all()
    for e in SMOOTHINGS:
        for z in Z_COEFFS:
            total64, u64, f64, grad64 = reference(logits, labels, vocab, w, e, z)
            zrz = run_z(ops, logits, labels, vocab, w, z, False)[3]
            for wg in (False, True):
                work, loss, lse, ru, rz = run_smooth(ops, logits, labels, vocab, w, e, z, wg)
                # 2. the outputs: the CE outputs and row_z do not see e; row_u and the summed objective against fp64
                assert torch.equal(loss, plain[wg][1]) and torch.equal(lse, plain[wg][2]), f"e {e} z {z}: row_loss / row_lse differ from ce_fwd"
                assert torch.equal(rz, zrz), f"e {e} z {z}: row_z differs from ce_fwd_z"
                torch.testing.assert_close(ru.cpu().double(), u64, **U_TOL)
                total = (1.0 - e) * loss.cpu().double().sum() + e * ru.cpu().double().sum()
                print(f"[e {e} z {z} weights {w is not None}] summed loss {float(total):.6f} vs torch {float(total64):.6f}")
                torch.testing.assert_close(total, total64, rtol=2e-5, atol=0)
                for out in (loss, lse, ru, rz):
                    assert (out.cpu()[~valid] == 0).all(), "a row without a valid label is not 0 in every output"
                if not wg:
                    assert torch.equal(work.cpu(), logits), "write_grad = 0 wrote the logits"
                    continue
                # 3. the gradient against fp64; pad columns and the rows without a valid label exactly 0; reproducible
                grad = work.cpu().float()
                check_gradient(grad[:, :vocab], grad64, f64, w, dtype, f"e {e} z {z} weights {w is not None}")
                assert (grad[:, vocab:] == 0).all(), "pad columns"
                assert (grad[~valid] == 0).all(), "rows without a valid label"
                again = run_smooth(ops, logits, labels, vocab, w, e, z, True)
                assert all(torch.equal(a, b) for a, b in zip(again, (work, loss, lse, ru, rz))), "not bitwise reproducible"
            no_lse = run_smooth(ops, logits, labels, vocab, w, e, z, True, with_lse=False)   # row_lse = NULL
            assert torch.equal(no_lse[0], work) and torch.equal(no_lse[1], loss) and torch.equal(no_lse[3], ru) and torch.equal(no_lse[4], rz)
        no_z = run_smooth(ops, logits, labels, vocab, w, e, 0.0, True, with_z=False)         # row_z = NULL is allowed with z = 0
        with_z = run_smooth(ops, logits, labels, vocab, w, e, 0.0, True)
        assert torch.equal(no_z[0], with_z[0]) and torch.equal(no_z[1], with_z[1]) and torch.equal(no_z[3], with_z[3])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("vocab,ld,dtype", SHAPES)
def test_smooth_forms_against_the_other_entries_bits_and_torch_fp64(ops, vocab, ld, dtype, weighted):
    logits, labels, w = make_inputs(ROWS, vocab, ld, dtype, seed=vocab)
    check_all(ops, logits, labels, vocab, w if weighted else None, dtype)


@pytest.mark.parametrize("weighted", [False, True])
def test_many_rows_per_workgroup_with_ignored_stretches(ops, weighted):
    """The layout of ``tests/test_ce_z_gpu.py::test_many_rows_per_workgroup_with_ignored_stretches``: 600 rows, each workgroup walks several."""
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


@pytest.mark.parametrize("e", SMOOTHINGS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("vocab,ld,dtype", SHAPES)
def test_the_uniform_term_exactly_on_hand_made_rows(ops, vocab, ld, dtype, weighted, e):
    """The rows of ``tests/test_ce_z_gpu.py::test_the_sign_of_f_on_hand_made_rows`` (z = 0.5; rows 0, 1: f < 0; rows 2, 3: f = 0 exactly; row 4:
    f > 0): every column off the hot ones is at -200, so its p underflows to 0 in fp32 and what the kernel stores there is the constant alone.
    With ``w32``, ``e32`` in fp32, ``wu = w32 * (e32 / float(V))`` and ``ome = 1.f - e32``:
      a cold real column off the label holds exactly ``-wu`` rounded to the dtype; a cold label column exactly ``-(w32 * ome) - wu`` rounded;
      a pad column exactly 0 — for every sign of f."""
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
    w32 = torch.ones(5) if w is None else w
    _, u64, f64, grad64 = reference(logits, labels, vocab, w, e, z)
    print("reference f:", f64.tolist())
    assert f64[0] < -0.49 and f64[1] < -0.49 and f64[2] == 0.0 and f64[3] == 0.0 and f64[4] > 7.0   # the intended signs, before use
    work, loss, lse, ru, rz = run_smooth(ops, logits, labels, vocab, w, e, z, True)
    _, loss_plain, lse_plain = run_plain(ops, logits, labels, vocab, w, True)
    assert torch.equal(loss, loss_plain) and torch.equal(lse, lse_plain)
    assert lse.cpu()[2] == -1.0 and lse.cpu()[3] == -1.0, "lse of the f == 0 rows is not exactly -1 in fp32"
    torch.testing.assert_close(ru.cpu().double(), u64, **U_TOL)
    grad = work.cpu().float()
    check_gradient(grad[:, :vocab], grad64, f64, w, dtype, f"hand-made rows, e {e}, weights {weighted}")
    e32, one = torch.tensor(e, dtype=torch.float32), torch.tensor(1.0, dtype=torch.float32)
    wu = w32 * (e32 / torch.tensor(float(vocab), dtype=torch.float32))      # fp32, in this order
    wl = w32 * (one - e32)
    assert wu.dtype == torch.float32 and wl.dtype == torch.float32 and (wu > 0).all()
    off_want = (-wu).to(dtype).float()
    label_want = (-wl - wu).to(dtype).float()
    assert (off_want < 0).all(), "the constant rounds to 0 in this dtype: the check would be empty"
    assert (grad[:, vocab:] == 0).all(), "pad columns"
    for r in range(5):
        hot_r = torch.zeros(vocab, dtype=torch.bool)
        hot_r[torch.tensor([7]) if r in (2, 3) else hot] = True
        cold_off = ~hot_r
        cold_off[labels[r]] = False
        assert cold_off.sum() >= vocab - hot_n - 1
        got = grad[r, :vocab][cold_off]
        assert (got == off_want[r]).all(), (f"row {r} (f = {float(f64[r]):.3f}): a cold column holds {got[got != off_want[r]][:4].tolist()}, "
                                            f"not -w e / V = {float(off_want[r])!r}")
        if not hot_r[labels[r]]:                             # rows 1 and 2: the label is a cold column
            assert float(grad[r, labels[r]]) == float(label_want[r]), (r, float(grad[r, labels[r]]), float(label_want[r]))
    assert int(labels[1]) == cold and int(labels[2]) == cold  # ... so both cold labels went through the check above (f < 0 and f = 0)
    assert float(grad[3, 7]) == float(label_want[3])         # f = 0, the label hot: f p = 0 exactly, the label's column is the constants alone
    for r in (0, 1):                                         # f < 0: every column is negative
        assert (grad[r, :vocab] < 0).all()
    others = hot[hot != labels[4]]
    assert (grad[4, others] > 0).all() and float(grad[4, labels[4]]) < 0


def test_bad_arguments_raise_with_the_entrys_message(ops):
    logits, labels, _ = make_inputs(ROWS, 515, 520, torch.float32, seed=1)
    for bad in (-0.1, 1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match=r"ce_fwd_smooth: smoothing must be finite and in \[0, 1\)"):
            run_smooth(ops, logits, labels, 515, None, bad, 0.0, True)
    for bad in (-1e-4, float("nan")):
        with pytest.raises(RuntimeError, match="ce_fwd_smooth: z_coeff must be finite and >= 0"):
            run_smooth(ops, logits, labels, 515, None, 0.1, bad, True)


def test_abi_version():
    from ssi import _lib
    assert _lib.load().ssi_abi_version() >= 14
