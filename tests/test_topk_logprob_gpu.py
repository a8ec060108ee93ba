"""``ssi_topk_logprob`` on the GPU: ``idx`` EXACTLY against a float64 / NumPy restatement (a stable sort of the allowed columns: value
descending, the lower column first among equals, NaN below every number, -1 where fewer than k are allowed), ``idx[:, 0]`` equal to
``ops.decode_select``'s token on the same inputs, ``lse`` and ``lp`` within the bound tests/decode_select_ref.py derives for that kernel's
log-probability (the exp-sum is formed term for term as there: ``Base.dlse`` for lse, ``dlse + U32 |lp|`` for lp = fl(x - lse)).

vocab in {1, 7, 515, 4099, 133 376} with ``ld > vocab`` and the pad columns holding NaN / +inf, k in {1, 3, 8}, both dtypes; masks: none,
sparse, one single allowed column, fewer than k allowed; ties planted at distant columns (two waves, two trips of a thread, the vector / tail
boundary) besides the all-ties family of ``make_logits``; rows holding NaN, and a row of nothing but NaN; an unaligned row length.

The worst lse / lp error over its bound is printed at module end (DESIGN.md §3 records it)."""
import numpy as np
import pytest
import torch

import decode_select_ref as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", (BF16, F32), ids=("bf16", "fp32"))
VOCABS = (1, 7, 515, 4099, 133_376)
KS = (1, 3, 8)
ROWS = 6
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(_WORST):
        print(f"\ntopk-logprob worst error/bound  {k:<10s} {_WORST[k]:.4f}", end="")
    print()


def topk(x_dev, vocab, k, mask=None, with_lse=True):
    from ssi import ops
    rows = x_dev.shape[0]
    idx = torch.full((rows, k), -7, dtype=torch.int32, device=DEV)
    lp = torch.full((rows, k), 7.0, dtype=torch.float32, device=DEV)
    lse = torch.full((rows,), 7.0, dtype=torch.float32, device=DEV) if with_lse else None
    ops.topk_logprob(x_dev, vocab, k, idx, lp, lse, mask=None if mask is None else D.pack(mask).to(DEV))
    torch.cuda.synchronize()
    return idx.cpu(), lp.cpu(), None if lse is None else lse.cpu()


def expected_idx(x, vocab, k, mask):
    """int64 [rows, k]: the stable order said again with NumPy on float64."""
    X = x[:, :vocab].double().numpy()
    allow = np.ones(vocab, dtype=bool) if mask is None else mask.numpy()
    out = np.full((X.shape[0], k), -1, dtype=np.int64)
    cols = np.nonzero(allow)[0]
    for r in range(X.shape[0]):
        v = X[r, cols]
        nan = np.isnan(v)
        order = np.lexsort((cols, np.where(nan, 0.0, -v), nan))              # last key first: numbers before NaN, value descending, column ascending
        best = cols[order[:k]]
        out[r, :len(best)] = best
    return torch.from_numpy(out)


def masks_for(vocab, k, seed):
    g = torch.Generator().manual_seed(seed)
    sparse = torch.rand(vocab, generator=g) < 0.05
    sparse[int(torch.randint(0, vocab, (1,), generator=g))] = True
    single = torch.zeros(vocab, dtype=torch.bool)
    single[vocab * 2 // 3] = True
    few = torch.zeros(vocab, dtype=torch.bool)
    few[torch.randperm(vocab, generator=g)[:max(0, min(k - 1, vocab))]] = True        # fewer than k allowed (none at all for k = 1)
    return {"none": None, "sparse": sparse, "single": single, "few": few}


def check(x, vocab, k, mask, dtype, what, base=None, vec=None):
    x_dev = x.to(DEV)
    idx, lp, lse = topk(x_dev, vocab, k, mask)
    want = expected_idx(x, vocab, k, mask)
    assert torch.equal(idx.long(), want), f"{what}: idx differs at rows {sorted(set((idx.long() != want).nonzero()[:, 0].tolist()))[:5]}"
    none = want < 0
    assert bool((lp[none] == -float("inf")).all()), what
    # idx[:, 0] is decode_select's token
    from ssi import ops
    tok = torch.full((x.shape[0],), -7, dtype=torch.int64, device=DEV)
    ops.decode_select(x_dev, vocab, tok, allow=None if mask is None else D.pack(mask).to(DEV))
    assert torch.equal(tok.cpu(), want[:, 0]), what
    if base is None:
        return idx, lp, lse
    X = base.X
    finite = ~torch.isnan(base.lse)
    elp = X.gather(1, want.clamp(min=0)) - base.lse[:, None]
    e_lse = (lse.double() - base.lse).abs()
    e_lp = (lp.double() - elp).abs()
    b_lp = base.dlse[:, None] + D.U32 * elp.abs()
    live = finite[:, None] & ~none
    assert bool((e_lse[finite] <= base.dlse[finite]).all()), f"{what}: lse off by {float((e_lse / base.dlse)[finite].max()):.3f} x its bound"
    assert bool((e_lp[live] <= b_lp[live]).all()), f"{what}: lp off by {float((e_lp / b_lp)[live].max()):.3f} x its bound"
    key = "bf16" if dtype == BF16 else "fp32"
    for name, ratio in ((key + " lse", (e_lse / base.dlse)[finite]), (key + " lp", (e_lp / b_lp)[live])):
        if ratio.numel():
            _WORST[name] = max(_WORST.get(name, 0.0), float(ratio.max()))
    return idx, lp, lse


def plant_ties(x, vocab):
    """Equal values above everything else at distant columns of rows 0 and 2 (fp32 tensor, before the cast)."""
    if vocab < 515:
        return x
    top = float(x[:, :vocab].max()) + 2.0
    for r, cols in ((0, (512, 0, vocab - 1)), (2, (vocab - 1, 3, 256, 2048 % vocab))):
        for c in cols:
            x[r, c] = top
    return x


@pytest.fixture(scope="module")
def inputs():
    made = {}

    def get(vocab, dtype):
        if (vocab, dtype) not in made:
            ld = D.ld_of(vocab)
            x = plant_ties(D.make_logits(ROWS, vocab, ld, F32, seed=vocab + 1), vocab).to(dtype)
            assert ld > vocab and not bool(torch.isfinite(x[:, vocab:].float()).any())          # the pad columns are poisoned
            made[(vocab, dtype)] = (x, D.Base(x, vocab))
        return made[(vocab, dtype)]
    return get


@DTYPES
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("vocab", VOCABS)
def test_idx_exact_and_logprobs_within_the_bound(inputs, vocab, k, dtype):
    x, base = inputs(vocab, dtype)
    for name, mask in masks_for(vocab, k, seed=vocab + k).items():
        idx, lp, lse = check(x, vocab, k, mask, dtype, f"{vocab} k{k} {name}", base)
        if name == "single":
            assert idx[:, 0].tolist() == [vocab * 2 // 3] * ROWS and bool((idx[:, 1:] == -1).all())
        if name == "few":
            assert bool((idx[:, max(k - 1, 0):] == -1).all()) and (k == 1 or vocab < k or bool((idx[:, :k - 1] >= 0).all()))
    assert torch.equal(x.view(torch.int16 if dtype == BF16 else torch.int32),
                       x.to(DEV).cpu().view(torch.int16 if dtype == BF16 else torch.int32))


@DTYPES
def test_rows_with_nan(dtype):
    vocab, k = 4099, 8
    x = D.make_logits(ROWS, vocab, D.ld_of(vocab), F32, seed=9)
    x[0, :vocab] = float("nan")                                  # nothing but NaN: the lowest columns, in order
    x[1, 5:vocab:3] = float("nan")
    x[2, int(x[2, :vocab].argmax())] = float("nan")              # the maximum of the row becomes a NaN: it ranks last
    x[3, :vocab] = float("nan")
    x[3, [4000, 17, 900]] = torch.tensor([1.0, 1.0, -3.0])       # three numbers, two of them equal, then NaN columns from 0 on
    x = x.to(dtype)
    for name, mask in masks_for(vocab, k, seed=5).items():
        idx, _, _ = check(x, vocab, k, mask, dtype, f"nan {name}")
        if mask is None:
            assert idx[0].tolist() == list(range(8)) and idx[3].tolist() == [17, 4000, 900, 0, 1, 2, 3, 4]


@DTYPES
def test_rows_that_are_not_16_byte_aligned(dtype):
    vocab, ld = 515, 517
    x = D.make_logits(5, vocab, ld, dtype, seed=3)
    assert not D.vec_ok(ld, dtype)
    base = D.Base(x, vocab)
    for k in (2, 4):
        for name, mask in masks_for(vocab, k, seed=k).items():
            check(x, vocab, k, mask, dtype, f"unaligned k{k} {name}", base)


@DTYPES
def test_a_rows_result_does_not_depend_on_other_rows(inputs, dtype):
    x, _ = inputs(4099, dtype)
    idx, lp, lse = topk(x.to(DEV), 4099, 3)
    i1, l1, s1 = topk(x[4:5].to(DEV), 4099, 3)
    assert torch.equal(i1[0], idx[4]) and torch.equal(l1[0], lp[4]) and torch.equal(s1[0], lse[4])
    i2, l2, _ = topk(x.to(DEV), 4099, 3, with_lse=False)         # lse may be NULL
    assert torch.equal(i2, idx) and torch.equal(l2, lp)


def test_refusals_come_before_any_launch():
    from ssi import _lib, ops
    x = torch.zeros(2, 16, device=DEV)
    i32, f32 = torch.full((2, 8), -7, dtype=torch.int32, device=DEV), torch.full((2, 8), 7.0, device=DEV)
    lib = _lib.load()
    p = _lib.ptr
    for k in (0, 9, -1):
        assert lib.ssi_topk_logprob(p(x), 16, 2, 16, k, None, 0, p(i32), p(f32), None, _lib.dtype_code(x.dtype), None) == 1
    with pytest.raises(RuntimeError, match="code 1"):
        ops.topk_logprob(x, 16, 9, torch.zeros(2, 9, dtype=torch.int32, device=DEV), torch.zeros(2, 9, device=DEV))
    assert lib.ssi_topk_logprob(p(x), 16, 2, 16, 2, None, 1, p(i32), p(f32), None, _lib.dtype_code(x.dtype), None) == 1     # a null mask with a length
    assert lib.ssi_topk_logprob(p(x), 16, 2, 16, 2, p(i32), 2, p(i32), p(f32), None, _lib.dtype_code(x.dtype), None) == 1   # a mask of another length
    torch.cuda.synchronize()
    assert bool((i32 == -7).all()) and bool((f32 == 7.0).all())  # nothing was written
    with pytest.raises(RuntimeError):
        ops.topk_logprob(x.cpu(), 16, 2, i32[:, :2].contiguous(), f32[:, :2].contiguous())
