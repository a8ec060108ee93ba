"""GPU: the segmented AdamW with a per-segment DEVICE gradient scale (``ssi_adamw_step_seg_gscale`` through
``ops.adamw_step_seg(seg_scale_dev=...)``; ABI v23).  The oracle is the plain kernel (``ops.adamw_step``, with ``sr_seed`` the stochastic one)
launched per segment on clones with ``grad_scale_dev`` = the product of the launch's scale and the segment's, computed in torch fp32 (one
correctly rounded product); the comparison is bit for bit on all four buffers, on the bit patterns, because frozen gradients hold NaN."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
HP = dict(beta1=0.9, beta2=0.999, eps=1e-8)
LR, WD = 2e-4, 0.01
N = 3 * 2048 + 8 + 5                      # three blocks of 256 bf16 vectors, one more vector, a ragged tail
SEED = (1 << 40) + 12_345
ENDS = (8, 16, 2040, 2048, 2056, 4160, 4224, 6152, N)


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


def _state(n, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g) * 50.0
    m = torch.randn(n, generator=g) * 0.1
    v = torch.rand(n, generator=g) * 0.01
    return [t.to(dtype).to(DEV) for t in (p, grad, m, v)]


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _oracle(ops, bufs, segs, seg_scale, *, step, scale=None, zero_grad=False, sr_seed=None, elem_offset=0):
    """Per segment the plain kernel with the product scale; a frozen segment, or one whose product is not finite, is left alone."""
    out = [t.clone() for t in bufs]
    prod = seg_scale if scale is None else scale * seg_scale       # fp32 on the device: one rounding per product
    finite = torch.isfinite(prod).tolist()
    start = 0
    for k, (end, lr, wd, frozen) in enumerate(segs):
        if not frozen and finite[k] and end > start:
            ops.adamw_step(*[t[start:end] for t in out], lr=lr, weight_decay=wd, step=step, grad_scale_dev=prod[k:k + 1].clone(), zero_grad=zero_grad,
                           sr_seed=sr_seed, elem_offset=elem_offset + start, **HP)
        start = end
    return out


def _gscale(ops, bufs, segs, seg_scale, *, step, scale=None, zero_grad=False, skip=False, sr_seed=None, elem_offset=0):
    out = [t.clone() for t in bufs]
    ops.adamw_step_seg(*out, seg_end=[s[0] for s in segs], seg_lr=[s[1] for s in segs], seg_weight_decay=[s[2] for s in segs],
                       seg_frozen=[s[3] for s in segs], step=step, grad_scale_dev=scale, zero_grad=zero_grad, skip_nonfinite_scale=skip,
                       sr_seed=sr_seed, elem_offset=elem_offset, seg_scale_dev=seg_scale, **HP)
    return out


def _scale():
    return torch.full((1,), 1.0 / 37.0, dtype=F32, device=DEV)


def _seg_scales(n, seed=7):
    # factors whose product with 1/37 needs a rounding; a clip coefficient lies in (0, 1], one of them is exactly 1
    g = torch.Generator().manual_seed(seed)
    s = torch.rand(n, generator=g) * 0.9 + 0.05
    s[n // 2] = 1.0
    return s.to(F32).to(DEV)


def _modes(dtype):
    return ((None, 0), (SEED, 4096)) if dtype == BF16 else ((None, 0),)


def _many(frozen=()):
    return [(e, LR * (1 + 0.5 * k), WD * (k % 3), k in frozen) for k, e in enumerate(ENDS)]


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("n", [0, 8, N])
def test_one_segment(ops, dtype, n):
    bufs = _state(n, dtype)
    ss = torch.full((1,), 0.3, dtype=F32, device=DEV)
    for sr_seed, off in _modes(dtype):
        for scale in (None, _scale()):
            segs = [(n, LR, WD, False)]
            want = _oracle(ops, bufs, segs, ss, step=3, scale=scale, sr_seed=sr_seed, elem_offset=off) if n else [t.clone() for t in bufs]
            got = _gscale(ops, bufs, segs, ss, step=3, scale=scale, sr_seed=sr_seed, elem_offset=off)
            assert _same(got, want)
            assert n == 0 or not _same(got[2:3], bufs[2:3])


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("with_scale", [False, True])
def test_many_segments_at_every_kind_of_boundary(ops, dtype, with_scale):
    bufs = _state(N, dtype, seed=1)
    ss = _seg_scales(len(ENDS))
    scale = _scale() if with_scale else None
    for sr_seed, off in _modes(dtype):
        segs = _many()
        want = _oracle(ops, bufs, segs, ss, step=3, scale=scale, sr_seed=sr_seed, elem_offset=off)
        got = _gscale(ops, bufs, segs, ss, step=3, scale=scale, sr_seed=sr_seed, elem_offset=off)
        assert _same(got, want)
        # the scales matter: all ones is a different result
        assert not _same(got[2:3], _gscale(ops, bufs, segs, torch.ones_like(ss), step=3, scale=scale, sr_seed=sr_seed, elem_offset=off)[2:3])


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_all_ones_is_the_segmented_kernel(ops, dtype):
    bufs = _state(N, dtype, seed=2)
    segs = _many(frozen=(3,))
    ones = torch.ones(len(ENDS), dtype=F32, device=DEV)
    for sr_seed, off in _modes(dtype):
        for scale in (None, _scale()):
            want = [t.clone() for t in bufs]
            ops.adamw_step_seg(*want, seg_end=[s[0] for s in segs], seg_lr=[s[1] for s in segs], seg_weight_decay=[s[2] for s in segs],
                               seg_frozen=[s[3] for s in segs], step=4, grad_scale_dev=scale, sr_seed=sr_seed, elem_offset=off, **HP)
            assert _same(_gscale(ops, bufs, segs, ones, step=4, scale=scale, sr_seed=sr_seed, elem_offset=off), want)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("which", [0, 1, 4, 5, 8])
def test_a_nonfinite_segment_scale_leaves_exactly_that_segment(ops, dtype, bad, which):
    bufs = _state(N, dtype, seed=3)
    start = ENDS[which - 1] if which else 0
    bufs[1][start:ENDS[which]] = float("nan")        # the group whose norm overflowed: its gradient is not to be read
    ss = _seg_scales(len(ENDS))
    ss[which] = bad
    segs = _many()
    for sr_seed, off in _modes(dtype):
        for scale in (None, _scale()):
            want = _oracle(ops, bufs, segs, ss, step=2, scale=scale, zero_grad=True, sr_seed=sr_seed, elem_offset=off)
            got = _gscale(ops, bufs, segs, ss, step=2, scale=scale, zero_grad=True, sr_seed=sr_seed, elem_offset=off)
            assert _same(got, want)
            assert _same([t[start:ENDS[which]] for t in got], [t[start:ENDS[which]] for t in bufs])   # untouched, the NaN gradient included
            s0 = 0
            for k, e in enumerate(ENDS):
                if k != which:
                    assert not got[1][s0:e].float().any() and got[0][s0:e].float().isfinite().all() and not _same([got[2][s0:e]], [bufs[2][s0:e]])
                s0 = e


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_a_nonfinite_launch_scale_with_bit_1_is_a_noop(ops, dtype):
    bufs = _state(N, dtype, seed=4)
    ss = _seg_scales(len(ENDS))
    for value in (float("inf"), float("nan")):
        bad = torch.full((1,), value, dtype=F32, device=DEV)
        for zero in (False, True):
            assert _same(_gscale(ops, bufs, _many(frozen=(2,)), ss, step=1, scale=bad, zero_grad=zero, skip=True), bufs)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("frozen", [(0,), (8,), (0, 1, 7, 8), (0, 1, 4, 5, 8), tuple(range(9))])
def test_frozen_segments_at_both_ends(ops, dtype, frozen):
    bufs = _state(N, dtype, seed=5)
    segs = _many(frozen)
    start = 0
    for k, e in enumerate(ENDS):
        if k in frozen:
            bufs[1][start:e] = float("nan")
        start = e
    ss = _seg_scales(len(ENDS))       # (indexed by segment of the CALL: the launch skips the frozen ends and their scales with them)
    for sr_seed, off in _modes(dtype):
        want = _oracle(ops, bufs, segs, ss, step=2, scale=_scale(), zero_grad=True, sr_seed=sr_seed, elem_offset=off)
        got = _gscale(ops, bufs, segs, ss, step=2, scale=_scale(), zero_grad=True, sr_seed=sr_seed, elem_offset=off)
        assert _same(got, want)


def test_130_segments_split_launches(ops):
    n_segs = 130
    n = 8 * n_segs
    bufs = _state(n, BF16, seed=6)
    segs = [(8 * (k + 1), LR * (1 + k % 7), WD * (k % 2), k % 5 == 3) for k in range(n_segs)]
    ss = _seg_scales(n_segs)
    ss[129] = 0.25                    # the second launch reads ITS slice of the scales
    for sr_seed, off in _modes(BF16):
        want = _oracle(ops, bufs, segs, ss, step=5, scale=_scale(), sr_seed=sr_seed, elem_offset=off)
        assert _same(_gscale(ops, bufs, segs, ss, step=5, scale=_scale(), sr_seed=sr_seed, elem_offset=off), want)
    from ssi import _lib
    out = [t.clone() for t in bufs]
    rc = _lib.load().ssi_adamw_step_seg_gscale(*[t.data_ptr() for t in out], n, (_lib.c_int64 * n_segs)(*[s[0] for s in segs]),
                                               (_lib.c_double * n_segs)(*[s[1] for s in segs]), (_lib.c_double * n_segs)(*[s[2] for s in segs]),
                                               (_lib.c_int32 * n_segs)(*[int(s[3]) for s in segs]), n_segs, 0.9, 0.999, 1e-8, 5, None, 0,
                                               _lib.SSI_BF16, 0, 0, 0, ss.data_ptr(), _lib.stream_ptr())
    assert rc == 2                    # SSI_ERR_UNSUPPORTED
    rc = _lib.load().ssi_adamw_step_seg_gscale(*[t.data_ptr() for t in out], n, (_lib.c_int64 * 1)(n), (_lib.c_double * 1)(LR), (_lib.c_double * 1)(WD),
                                               (_lib.c_int32 * 1)(0), 1, 0.9, 0.999, 1e-8, 5, None, 0, _lib.SSI_BF16, 0, 0, 0, None, _lib.stream_ptr())
    assert rc == 1                    # SSI_ERR_ARG: the scales are never NULL
    torch.cuda.synchronize()
    assert _same(out, bufs)
