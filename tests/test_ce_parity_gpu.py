"""GPU: per-element parity of the five cross-entropy entries (``ssi_ce_fwd``, ``_weighted``, ``_z``, ``_smooth``, ``_metrics``, ``_kl``) in both
forms against float64, under the bounds derived in tests/ce_parity.py — every register-form chunk count (1, 2, 3, 4, 8, 16, 17, 18), the
generic fallbacks in bf16 and fp32, both sides of the ``ld - vocab = 8192`` boundary.  Every comparison is made at EVERY element; ``check``
names the worst one and the module prints the worst err / bound per family (form x mode x output; the generic form in fp32 storage apart) at
its end (``pytest -s``).

A case's rows mix the input families (row i: ``ce_parity.MIXED[i % 5]`` — randn at scale 3, randn 3 + 60, randn 10 - 40, one column 30 above the
rest), the student's pad columns hold NaN, 1e4 or +inf by row and the teacher's -3e4 or NaN; labels come from the label table (chunk, lane and
within-register edges, an ignored label, one out of range on either side)."""
import pytest
import torch

import ce_parity as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
_WORST: dict[str, float] = {}
_CACHE: dict = {}


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam in sorted(_WORST):
        print(f"\nce-parity worst error/bound  {fam:<28s} {_WORST[fam]:.4f}", end="")
    print()


def bits(t):
    return t.view(torch.int16 if t.dtype == C.BF16 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def check(family, got, ref, bound, what):
    worst, idx, misses = C.ratio(got, ref, bound)
    print(f"{what} [{family}]: worst err / bound {worst:.4f} at {idx}")
    if misses:
        g = got.detach().cpu().double()
        raise AssertionError(f"{what} [{family}]: {misses} of {ref.numel()} elements miss their bound; worst at {idx}: got {float(g[idx])!r} ref "
                             f"{float(ref[idx])!r} err {abs(float(g[idx]) - float(ref[idx])):.3e} bound {float(bound[idx]):.3e}")
    _WORST[family] = max(_WORST.get(family, 0.0), worst)


def inputs(shape, families=C.MIXED, rows=None):
    """(logits, Base) of a shape, computed once and left unchanged (the latest shape only is kept)."""
    vocab, ld, dtype = shape[:3]
    key = (shape, families, rows)
    if _CACHE.get("key") != key:
        _CACHE.clear()
        x = C.make_logits(rows or C.case_rows(ld), vocab, ld, dtype, seed=vocab, families=families)
        _CACHE.update(key=key, x=x, base=C.Base(x, vocab), teachers={})
    return _CACHE["x"], _CACHE["base"]


def teacher_of(ops, shape, x, kind, labels):
    """(teacher on the host, on the device, teacher_lse as ``ssi_ce_fwd`` writes it forward-only with these labels)."""
    vocab = shape[0]
    if kind not in _CACHE["teachers"]:
        t = C.make_teacher(x, vocab, kind, seed=vocab)
        _CACHE["teachers"][kind] = (t, t.to(DEV))
    t, tdev = _CACHE["teachers"][kind]
    return t, tdev, teacher_lse(ops, tdev, labels, vocab)


def teacher_lse(ops, tdev, labels, vocab):
    rows = tdev.shape[0]
    loss, lse = torch.full((rows,), 7.0, device=DEV), torch.full((rows,), 7.0, device=DEV)
    ops.ce_fwd(tdev, labels.to(DEV), vocab, C.IGNORE, loss, lse, False)
    return lse


def run(ops, m, work, labels, vocab, w, write_grad, tdev=None, tlse=None, k=None):
    """One call of mode ``m``'s entry on the device buffer ``work``: {output: device tensor}."""
    rows = work.shape[0]
    lab = labels.to(DEV)
    wd = None if w is None else w.to(DEV)

    def buf():
        return torch.full((rows,), 7.0, device=DEV)

    out = {"row_loss": buf(), "row_lse": buf()}
    kind = m["kind"]
    if kind == "plain":
        ops.ce_fwd(work, lab, vocab, C.IGNORE, out["row_loss"], out["row_lse"], write_grad, row_weight=wd)
    elif kind == "z":
        out["row_z"] = buf()
        ops.ce_fwd_z(work, lab, vocab, C.IGNORE, m["z"], out["row_loss"], out["row_lse"], out["row_z"], write_grad, row_weight=wd)
    elif kind == "smooth":
        out["row_z"], out["row_u"] = buf(), buf()
        ops.ce_fwd_smooth(work, lab, vocab, C.IGNORE, m["e"], m["z"], out["row_loss"], out["row_lse"], out["row_u"], out["row_z"], write_grad,
                          row_weight=wd)
    elif kind == "metrics":
        out["row_nll"], out["row_rank"] = buf(), torch.full((rows,), 7, dtype=torch.int32, device=DEV)
        ops.ce_fwd_metrics(work, lab, vocab, C.IGNORE, out["row_loss"], out["row_lse"], out["row_nll"], out["row_rank"], row_weight=wd)
    else:
        out["row_kl"] = buf()
        ops.ce_fwd_kl(work, tdev, tlse, lab, vocab, C.IGNORE, m["beta"], out["row_loss"], out["row_lse"], out["row_kl"], write_grad,
                      row_weight=wd, row_kl_weight=None if k is None else k.to(DEV))
    return out


def kl_weights(rows):
    g = torch.Generator().manual_seed(3)
    k = 2.0 * torch.rand(rows, generator=g)
    k[rows // 2] = 0.0
    return k


def check_scalars(form, m, out, exp, what):
    for name, (ref, bound) in exp.items():
        if name == "grad":
            continue
        if name == "row_rank":
            assert torch.equal(out[name].cpu().long(), ref), f"{what}: row_rank {out[name].cpu().tolist()} want {ref.tolist()}"
            continue
        check(f"{form} {m['kind']} {name}", out[name], ref, bound, what)


def parity_case(ops, shape, m, x, base, labels, w, what):
    """All of one (inputs, labels, weights, mode): forward-only, then with the gradient.  Also: write_grad = 0 leaves the buffer bit-identical,
    pad columns and rows without a valid label are 0 (rank -1), the teacher is never written."""
    vocab, ld, dtype, form, _ = shape
    valid = C.is_valid(labels, vocab)
    xdev = x.to(DEV)
    t = tdev = tlse = k = None
    if m["kind"] == "kl":
        t, tdev, tlse = teacher_of(ops, shape, x, m["teacher"], labels)
        k = kl_weights(x.shape[0]) if m["kw"] else None
    exp = C.expected(base, labels, m, form, w=w, teacher=t, tlse=None if tlse is None else tlse.cpu(), k=k)
    fam = form if dtype == C.BF16 else "generic-fp32"    # fp32 storage has no half bf16 ulp to hide in: a family of its own
    for wg in (False, True):
        work = xdev.clone()
        out = run(ops, m, work, labels, vocab, w, wg, tdev, tlse, k)
        check_scalars(fam, m, out, exp, f"{what} write_grad {int(wg)}")
        for name, v in out.items():
            assert (v.cpu()[~valid] == (-1 if name == "row_rank" else 0)).all(), f"{what}: {name} of a row without a valid label"
        if tdev is not None:
            assert same_bits(tdev.cpu(), t), f"{what}: the teacher buffer was written"
        if not wg or m["kind"] == "metrics":
            assert same_bits(work, xdev), f"{what}: write_grad = 0 wrote the logits"
            if m["kind"] == "metrics":
                return
            continue
        grad = work.cpu().float()
        ref, bound = exp["grad"]
        check(f"{fam} {m['kind']} grad", grad[:, :vocab], ref, bound, what)
        assert (grad[:, vocab:] == 0).all(), f"{what}: pad columns"
        assert (grad[~valid] == 0).all(), f"{what}: rows without a valid label"


# ---- 1. parity per mode and form -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", C.MODES, ids=C.mode_id)
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.shape_id)
def test_parity(ops, shape, m):
    vocab, ld = shape[:2]
    x, base = inputs(shape)
    blocks = C.label_blocks(vocab, ld)
    mi = C.MODES.index(m)
    for weighted in (False, True):                       # the label blocks of a shape are dealt over its modes and the two weightings
        labels = blocks[(2 * mi + weighted) % len(blocks)]
        w = C.make_weights(x.shape[0]) if weighted else None
        parity_case(ops, shape, m, x, base, labels, w, f"{C.shape_id(shape)} {C.mode_id(m)} weights {int(weighted)}")


def test_parity_reaches_every_label_block():
    """The dealing above: with 10 modes and two weightings every block of every shape is used (at most 4 blocks at 24 rows)."""
    for vocab, ld, *_ in C.SHAPES:
        n = len(C.label_blocks(vocab, ld))
        assert {(2 * mi + wt) % n for mi in range(len(C.MODES)) for wt in (0, 1)} == set(range(n)), (vocab, ld, n)


# ---- 2. the rank, exact ----------------------------------------------------------------------------------------------------------------------
RANK_SHAPES = [s for s in C.one_per_nch() if s[3] == "row"] + [s for s in C.SHAPES if s[3] == "generic" and s[1] in (520, 8704, 65_544)]


@pytest.mark.parametrize("shape", RANK_SHAPES, ids=C.shape_id)
def test_rank_is_exact_on_tie_heavy_rows(ops, shape):
    vocab, ld, dtype, form, _ = shape
    x, base = inputs(shape, families=("ties",))
    m = C.mode("metrics")
    xdev = x.to(DEV)
    for i, labels in enumerate(C.label_blocks(vocab, ld)):
        exp = C.expected(base, labels, m, form)
        assert int(exp["row_rank"][0].max()) > 1000 or vocab < 5000, "the rows are not tie-heavy"
        work = xdev.clone()
        out = run(ops, m, work, labels, vocab, None, False)
        check_scalars(form, m, out, exp, f"{C.shape_id(shape)} ties block {i}")
        assert same_bits(work, xdev)


# ---- 3. the row walk -------------------------------------------------------------------------------------------------------------------------
WALK_MODES = [C.mode("plain"), C.mode("smooth", e=0.1, z=1e-4), C.mode("kl", beta=2.0, teacher="near", kw=True)]


@pytest.mark.parametrize("m", WALK_MODES, ids=C.mode_id)
@pytest.mark.parametrize("vocab,ld", [(515, 520), (9000, 9216)])
def test_row_walk(ops, vocab, ld, m):
    """Five base rows (content, label, weight; base 3 ignored) repeated cyclically over 1, CUs - 1, CUs, CUs + 1 and 2 CUs + 3 rows; the last
    row and the second row of workgroup 0 are base 3.  Rows of equal base are bit-equal wherever they lie (the next-row loads issued inside the
    gradient loop, the `next < rows ? next : row` tail), and the base rows meet their float64 bounds."""
    shape = (vocab, ld, C.BF16, "row", C.cdiv(ld, C.CHUNK))
    assert C.row_form(C.BF16, ld, vocab)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    x5 = C.make_logits(5, vocab, ld, C.BF16, seed=ld)
    lab5 = torch.tensor([vocab - 1, 0, 8 if ld < C.CHUNK else C.CHUNK, C.IGNORE, vocab // 2])
    w5 = torch.tensor([0.5, 1.0, 2.75, 1.25, 0.0])
    k5 = torch.tensor([1.5, 0.0, 0.25, 1.0, 2.0])
    t5 = C.make_teacher(x5, vocab, "near", seed=ld)
    base = C.Base(x5, vocab)
    for rows in (1, cus - 1, cus, cus + 1, 2 * cus + 3):
        idx = torch.arange(rows) % 5
        if rows >= 5:
            idx[rows - 1] = 3
        if rows > cus:
            idx[cus] = 3
        xdev, labels, w = x5[idx].to(DEV), lab5[idx], w5[idx]
        tdev = tlse = k = None
        if m["kind"] == "kl":
            tdev, k = t5[idx].to(DEV), k5[idx]
            tlse = teacher_lse(ops, tdev, labels, vocab)
        work = xdev.clone()
        out = run(ops, m, work, labels, vocab, w, True, tdev, tlse, k)
        first = {int(j): int((idx == j).nonzero()[0]) for j in idx.unique()}
        src = torch.tensor([first[int(j)] for j in idx], device=DEV)
        assert same_bits(work, work[src]), f"{rows} rows: gradient rows of equal base differ"
        for name, v in out.items():
            assert torch.equal(v, v[src]), f"{rows} rows: {name} of rows of equal base differ"
        if tlse is not None:
            assert torch.equal(tlse, tlse[src])
        # the first occurrence of each base against float64
        sel = torch.tensor([first.get(j, -1) for j in range(5)])
        have = sel >= 0
        tl5 = torch.zeros(5)
        if tlse is not None:
            tl5[have] = tlse.cpu()[sel[have]]
        exp = C.expected(base, lab5, m, "row", w=w5, teacher=t5 if tdev is not None else None, tlse=tl5 if tdev is not None else None,
                         k=k5 if k is not None else None)
        what = f"{vocab}x{ld} {C.mode_id(m)} walk over {rows} rows"
        for name, (ref, bound) in exp.items():
            got = work.cpu().float()[sel[have]][:, :vocab] if name == "grad" else out[name].cpu()[sel[have]]
            check(f"row {m['kind']} {name}", got, ref[have], bound[have], what)
        assert (work.cpu().float()[:, vocab:] == 0).all()


# ---- 4. guard rows ---------------------------------------------------------------------------------------------------------------------------
GUARD_SHAPES = [s for s in C.SHAPES if (s[0], s[1], s[2]) in ((515, 520, C.BF16), (8193, 8200, C.BF16), (139_265, 139_272, C.BF16),
                                                              (40_840, 40_960, C.BF16))]
GUARD_MODES = [C.mode("plain"), C.mode("z", z=0.5), C.mode("smooth", e=0.1, z=1e-4), C.mode("kl", beta=2.0, teacher="far")]


@pytest.mark.parametrize("shape", GUARD_SHAPES, ids=C.shape_id)
def test_guard_rows_stay_untouched(ops, shape):
    """Logits and teacher are rows [1, rows + 1) of buffers whose first and last row hold a sentinel: after every mode with write_grad = 1
    the sentinel rows are bit-identical (the buffer resource's bound drops what lies beyond a row; the generic form's row loop ends at ld)."""
    vocab, ld, dtype, form, _ = shape
    rows = 6
    x = C.make_logits(rows, vocab, ld, dtype, seed=ld)
    labels = torch.tensor([vocab - 1, 0, C.IGNORE, vocab, vocab // 2, vocab - 1])

    def guarded(src):
        big = torch.full((rows + 2, ld), C.SENTINEL, dtype=dtype, device=DEV)
        big[1:rows + 1].copy_(src)
        return big, big[1:rows + 1]

    base = C.Base(x, vocab)
    for m in GUARD_MODES:
        big, work = guarded(x)
        tbig = tdev = tlse = t = None
        if m["kind"] == "kl":
            t = C.make_teacher(x, vocab, m["teacher"], seed=ld)
            tbig, tdev = guarded(t)
            tlse = teacher_lse(ops, tdev, labels, vocab)
        out = run(ops, m, work, labels, vocab, None, True, tdev, tlse)
        torch.cuda.synchronize()
        for b in (big, tbig):
            if b is not None:
                assert (b[0] == C.SENTINEL).all() and (b[rows + 1] == C.SENTINEL).all(), f"{C.mode_id(m)}: a guard row was written"
        if tdev is not None:
            assert same_bits(tdev.cpu(), t)
        exp = C.expected(base, labels, m, form, teacher=t, tlse=None if tlse is None else tlse.cpu())
        check(f"{form} {m['kind']} grad", work.cpu().float()[:, :vocab], *exp["grad"], f"{C.shape_id(shape)} {C.mode_id(m)} guarded")


# ---- 5. which form ran -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s in C.SHAPES if s[1] > s[0]], ids=C.shape_id)
def test_dispatch_signature(ops, shape):
    """No entry reports the form it took; the kernels document one difference: with f < 0 (ssi_ce_fwd_z, z = 0.5, lse < -1) the register form
    leaves -0 in the pad columns (the sign flip of the packed store), the generic form +0.  The rows are randn 10 - 40; where the vocabulary is
    large enough that such a row's lse is not below -3, the row is moved down by the multiple of 16 that puts it there."""
    vocab, ld, dtype, form, _ = shape
    rows = 3
    g = torch.Generator().manual_seed(ld)
    x = 10.0 * torch.randn(rows, ld, generator=g) - 40.0
    lse = torch.logsumexp(x[:, :vocab].double(), 1)
    x -= (16.0 * torch.ceil((lse + 3.0).clamp(min=0) / 16.0)).float()[:, None]
    x[:, vocab:] = 1e4
    x = x.to(dtype)
    labels = torch.tensor([0, vocab - 1, vocab // 2])
    m = C.mode("z", z=0.5)
    f = 1.0 + 2.0 * C.f32(0.5) * torch.logsumexp(x[:, :vocab].double(), 1)
    assert (f < 0).all(), f.tolist()
    work = x.to(DEV)
    run(ops, m, work, labels, vocab, None, True)
    pad = bits(work.cpu())[:, vocab:]
    negative_zero = torch.iinfo(pad.dtype).min           # the sign bit alone
    want = negative_zero if form == "row" else 0
    assert (pad == want).all(), f"{C.shape_id(shape)}: the pad columns do not carry the {form} form's zero"
    assert C.row_form(dtype, ld, vocab) == (form == "row")


# ---- 6. ssi_ce_reduce ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 1023, 1024, 1025, 3000])
def test_ce_reduce_row_loop_edges(ops, rows):
    """Integer row losses in [0, 7]: every fp32 sum is exact in any order.  out[1], out[2], out[3] bit for bit, out[0] the correctly rounded
    quotient."""
    vocab = 515
    g = torch.Generator().manual_seed(rows)
    loss = torch.randint(0, 8, (rows,), generator=g).float()
    labels = torch.randint(0, vocab, (rows,), generator=g)
    labels[1::5] = C.IGNORE
    labels[2::7] = vocab
    labels[3::11] = -3
    valid = C.is_valid(labels, vocab)
    assert bool(valid[0])
    out = torch.full((4,), 7.0, device=DEV)
    ops.ce_reduce(loss.to(DEV), labels.to(DEV), vocab, C.IGNORE, out)
    s, c = loss[valid].sum(), valid.sum().float()
    bad = (~valid & (labels != C.IGNORE)).sum().float()
    want = torch.stack([s / c, s, c, bad])
    assert rows < 5 or (float(bad) > 0 and float(c) < rows)
    assert same_bits(out.cpu(), want), (out.cpu().tolist(), want.tolist())


# ---- a base that is not 16-byte aligned is refused -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [C.BF16, C.F32], ids=["bf16", "fp32"])
def test_a_misaligned_base_is_refused_and_nothing_is_launched(ops, dtype):
    vocab, ld, rows = 515, 520, 4
    x = C.make_logits(rows, vocab, ld, dtype, seed=1, pads=(1e4,))
    labels = torch.tensor([0, 1, 2, 3])
    off = 8 // x.element_size()

    def shifted(src):
        flat = torch.zeros(rows * ld + off, dtype=dtype, device=DEV)
        view = flat[off:].view(rows, ld)
        view.copy_(src)
        assert view.data_ptr() % 16 == 8
        return view

    t = C.make_teacher(x, vocab, "near", seed=1, pads=(-3e4,))
    tlse = teacher_lse(ops, t.to(DEV), labels, vocab)
    for m in (C.mode("plain"), C.mode("z", z=0.5), C.mode("smooth", e=0.1), C.mode("metrics"), C.mode("kl", beta=0.5, teacher="near")):
        for which in ("logits", "teacher") if m["kind"] == "kl" else ("logits",):
            work = shifted(x) if which == "logits" else x.to(DEV)
            tdev = (shifted(t) if which == "teacher" else t.to(DEV)) if m["kind"] == "kl" else None
            before = work.clone()
            for wg in (False, True):
                with pytest.raises(RuntimeError, match="argument check failed"):
                    run(ops, m, work, labels, vocab, None, wg, tdev, tlse)
            torch.cuda.synchronize()
            assert same_bits(work, before), f"{C.mode_id(m)}: a refused call wrote the logits"
    # and the same calls on aligned buffers run
    out = run(ops, C.mode("plain"), x.to(DEV), labels, vocab, None, True)
    assert (out["row_loss"] != 7.0).all()
