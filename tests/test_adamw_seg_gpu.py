"""GPU: AdamW over segments of the flat buffers (``ssi_adamw_step_seg`` through ``ops.adamw_step_seg``; ABI v16).  The oracle is always the
existing kernel (``ops.adamw_step``, with ``sr_seed`` the stochastic one) launched per non-frozen segment on clones, with that segment's lr
and weight decay and ``elem_offset`` + the segment's start; the comparison is bit for bit on all four buffers (on the bit patterns: frozen
gradients hold NaN).

The grid-stride trip of a capped grid (more than 2**20 blocks of 256 vectors: 2**31 bf16 elements) is unreachable at these sizes, as it is for
the existing kernel; it is not faked here."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
HP = dict(beta1=0.9, beta2=0.999, eps=1e-8)
LR, WD = 2e-4, 0.01                       # the reference's optimizer settings (conf/training.yaml)
N = 3 * 2048 + 8 + 5                      # three blocks of 256 bf16 vectors, one more vector, a ragged tail
SEED = (1 << 40) + 12_345


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


def _oracle(ops, bufs, segs, *, step, scale=None, zero_grad=False, skip=False, sr_seed=None, elem_offset=0):
    out = [t.clone() for t in bufs]
    start = 0
    for end, lr, wd, frozen in segs:
        if not frozen and end > start:
            ops.adamw_step(*[t[start:end] for t in out], lr=lr, weight_decay=wd, step=step, grad_scale_dev=scale, zero_grad=zero_grad,
                           skip_nonfinite_scale=skip, sr_seed=sr_seed, elem_offset=elem_offset + start, **HP)
        start = end
    return out


def _segmented(ops, bufs, segs, *, step, scale=None, zero_grad=False, skip=False, sr_seed=None, elem_offset=0):
    out = [t.clone() for t in bufs]
    ops.adamw_step_seg(*out, seg_end=[s[0] for s in segs], seg_lr=[s[1] for s in segs], seg_weight_decay=[s[2] for s in segs],
                       seg_frozen=[s[3] for s in segs], step=step, grad_scale_dev=scale, zero_grad=zero_grad, skip_nonfinite_scale=skip,
                       sr_seed=sr_seed, elem_offset=elem_offset, **HP)
    return out


def _scale():
    return torch.full((1,), 1.0 / 37.0, dtype=F32, device=DEV)


def _modes(dtype):
    return ((None, 0), (SEED, 4096)) if dtype == BF16 else ((None, 0),)


# boundaries: 8; a one-vector segment [8, 16); 2040 and 2056 straddle a block, 2048 is exactly one block's span; 4160 and 4224 lie inside one
# 256-vector span; the last segment [6152, N) is only the ragged tail
ENDS = (8, 16, 2040, 2048, 2056, 4160, 4224, 6152, N)


def _many(frozen=()):
    return [(e, LR * (1 + 0.5 * k), WD * (k % 3), k in frozen) for k, e in enumerate(ENDS)]


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("n", [0, 8, N])
def test_one_segment_is_the_plain_kernel(ops, dtype, n):
    bufs = _state(n, dtype)
    for sr_seed, off in _modes(dtype):
        segs = [(n, LR, WD, False)]
        want = _oracle(ops, bufs, segs, step=3, scale=_scale(), sr_seed=sr_seed, elem_offset=off) if n else [t.clone() for t in bufs]
        got = _segmented(ops, bufs, segs, step=3, scale=_scale(), sr_seed=sr_seed, elem_offset=off)
        assert _same(got, want)
        assert n == 0 or not _same(got[2:3], bufs[2:3])   # (something moved: exp_avg; eight bf16 weights may all round back)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_many_segments_at_every_kind_of_boundary(ops, dtype):
    bufs = _state(N, dtype, seed=1)
    for sr_seed, off in _modes(dtype):
        segs = _many()
        want = _oracle(ops, bufs, segs, step=3, scale=_scale(), sr_seed=sr_seed, elem_offset=off)
        got = _segmented(ops, bufs, segs, step=3, scale=_scale(), sr_seed=sr_seed, elem_offset=off)
        assert _same(got, want)
        # the settings matter: one segment at the first one's values is a different result
        assert not _same(got[:1], _oracle(ops, bufs, [(N, LR, 0.0, False)], step=3, scale=_scale(), sr_seed=sr_seed, elem_offset=off)[:1])


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("frozen", [(0,), (4,), (8,), (0, 1, 4, 5, 8), (1, 2, 3, 4, 5, 6, 7), tuple(range(9))])
def test_frozen_segments_are_neither_read_nor_written(ops, dtype, frozen):
    bufs = _state(N, dtype, seed=2)
    segs = _many(frozen)
    start = 0
    for k, e in enumerate(ENDS):
        if k in frozen:
            bufs[1][start:e] = float("nan")      # a frozen gradient is unspecified
        start = e
    for sr_seed, off in _modes(dtype):
        want = _oracle(ops, bufs, segs, step=2, scale=_scale(), zero_grad=True, sr_seed=sr_seed, elem_offset=off)
        got = _segmented(ops, bufs, segs, step=2, scale=_scale(), zero_grad=True, sr_seed=sr_seed, elem_offset=off)
        assert _same(got, want)
        start = 0
        for k, e in enumerate(ENDS):
            if k in frozen:                          # ... all four buffers as they were, the NaN gradient included (zero_grad leaves it alone)
                assert _same([t[start:e] for t in got], [t[start:e] for t in bufs])
            else:
                assert not got[1][start:e].float().any() and got[0][start:e].float().isfinite().all()
            start = e


@pytest.mark.parametrize("n_segs", [128, 129, 300])
def test_the_table_limit_and_the_split_launch(ops, n_segs):
    """128 segments of 8 elements fill the table; one more and ``ops`` splits the launch at a segment end — still exact.  The library itself
    refuses more than 128."""
    n = 8 * n_segs
    bufs = _state(n, BF16, seed=3)
    segs = [(8 * (k + 1), LR * (1 + k % 7), WD * (k % 2), k % 5 == 3) for k in range(n_segs)]
    for sr_seed, off in _modes(BF16):
        want = _oracle(ops, bufs, segs, step=5, scale=_scale(), sr_seed=sr_seed, elem_offset=off)
        assert _same(_segmented(ops, bufs, segs, step=5, scale=_scale(), sr_seed=sr_seed, elem_offset=off), want)
    if n_segs > 128:
        from ssi import _lib
        out = [t.clone() for t in bufs]
        rc = _lib.load().ssi_adamw_step_seg(*[t.data_ptr() for t in out], n, (_lib.c_int64 * n_segs)(*[s[0] for s in segs]),
                                            (_lib.c_double * n_segs)(*[s[1] for s in segs]), (_lib.c_double * n_segs)(*[s[2] for s in segs]),
                                            (_lib.c_int32 * n_segs)(*[int(s[3]) for s in segs]), n_segs, 0.9, 0.999, 1e-8, 5, None, 0,
                                            _lib.SSI_BF16, 0, 0, 0, _lib.stream_ptr())
        assert rc == 2                                # SSI_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert _same(out, bufs)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_zero_grad_bits(ops, dtype):
    bufs = _state(N, dtype, seed=4)
    segs = _many(frozen=(2, 6))
    got = _segmented(ops, bufs, segs, step=1, scale=_scale(), zero_grad=True)
    assert _same(got, _oracle(ops, bufs, segs, step=1, scale=_scale(), zero_grad=True))
    assert torch.equal(got[1][2040:2048], torch.zeros_like(got[1][2040:2048])) and _same([got[1][16:2040]], [bufs[1][16:2040]])
    inf = torch.full((1,), float("inf"), dtype=F32, device=DEV)
    for zero in (False, True):                        # bit 1: a non-finite scale makes the whole launch a no-op, bit 0 included
        assert _same(_segmented(ops, bufs, segs, step=1, scale=inf, zero_grad=zero, skip=True), bufs)
    nan = torch.full((1,), float("nan"), dtype=F32, device=DEV)
    assert _same(_segmented(ops, bufs, segs, step=1, scale=nan, skip=True), bufs)


def test_argument_errors(ops):
    bufs = _state(64, BF16, seed=5)
    def call(ends, n=64, dtype=BF16, sr_seed=None, elem_offset=0):
        b = [t[:n].to(dtype) for t in bufs]
        ops.adamw_step_seg(*b, seg_end=ends, seg_lr=[LR] * len(ends), seg_weight_decay=[WD] * len(ends), seg_frozen=[False] * len(ends), step=1,
                           sr_seed=sr_seed, elem_offset=elem_offset, **HP)
    call([16, 64])                                    # (the good form)
    for ends in ([12, 64], [32, 16, 64], [32, 32, 64], [32, 56], [32, 72]):
        with pytest.raises((RuntimeError, ValueError)):
            call(ends)
    with pytest.raises(RuntimeError):
        call([16, 64], dtype=F32, sr_seed=SEED)       # fp32 storage has nothing to round
    with pytest.raises(RuntimeError):
        call([16, 64], sr_seed=SEED, elem_offset=4)   # the random bits are per 8-element vector of the global index
    torch.cuda.synchronize()
