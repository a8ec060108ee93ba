"""GPU: sums of squares per group of segments of a flat buffer (``ssi_sumsq_groups`` through ``ops.sumsq_groups``; ABI v23).  The reference is
the sum in float64 of the same stored values.  The three properties the header states are asserted: the same bits in every launch, no bit of a
group's sum moved by any element outside it (NaN, inf and skipped segments included), and the relative bound ``B`` derived from the kernel's own
accumulation depth (``include/ssi_hip.h``, ``DESIGN.md`` section 3):

    B = D u / (1 - D u),  u = 2**-24,  D = 1 + (T E + 1) + n_segs + 12 + 1 + 12

with ``E`` elements per 16-byte vector, ``T = ceil(ceil((n / E) / 256) / 2048)`` tiles per block (1 at these sizes).  The worst fraction of ``B``
reached is printed (run with ``-s``)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
N = 3 * 2048 + 8 + 5                      # three blocks of 256 bf16 vectors, one more vector, a ragged tail (test_adamw_seg_gpu.py's size)
# boundaries: 8; a one-vector segment [8, 16); 2040 and 2056 straddle a block, 2048 is exactly one block's span; 4160 and 4224 lie inside one
# 256-vector span; the last segment [6152, N) is only the ragged tail
ENDS = (8, 16, 2040, 2048, 2056, 4160, 4224, 6152, N)
U = 2.0 ** -24
WORST = {"fraction": 0.0}


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


def bound(n, dtype, n_segs):
    e = 8 if dtype == BF16 else 4
    t = max(1, math.ceil(math.ceil((n // e) / 256) / 2048))
    d = 1 + (t * e + 1) + n_segs + 12 + 1 + 12
    return d * U / (1 - d * U)


def _data(n, dtype, seed=0, wide=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    if wide:   # magnitudes over 2**-20 .. 2**20: small terms meet large partial sums
        x = x * torch.exp2(torch.randint(-20, 21, (n,), generator=g).float())
    return x.to(dtype).to(DEV)


def _ref(x, ends, groups, n_groups):
    ref = [0.0] * n_groups
    xd = x.double().cpu()
    start = 0
    for e, g in zip(ends, groups):
        if g >= 0:
            ref[g] += float((xd[start:e] * xd[start:e]).sum())
        start = e
    return ref


def _run(ops, x, ends, groups, n_groups, out=None):
    out = torch.empty(n_groups, dtype=F32, device=DEV) if out is None else out
    ops.sumsq_groups(x, list(ends), list(groups), n_groups, out)
    return out


def _check(got, ref, b):
    got = got.double().cpu().tolist()
    for g, (a, r) in enumerate(zip(got, ref)):
        err = abs(a - r)
        if r > 0:
            WORST["fraction"] = max(WORST["fraction"], err / (b * r))
        print(f"group {g}: got {a:.9e} ref {r:.9e} |err| {err:.3e} bound {b * r:.3e}")
        assert err <= b * r, (g, a, r, b)


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("n", [0, 8, N])
def test_one_group_over_everything(ops, dtype, n):
    x = _data(n, dtype, seed=n)
    got = _run(ops, x, [n], [0], 1)
    b = bound(n, dtype, 1)
    _check(got, _ref(x, [n], [0], 1), b)
    if n:
        plain = torch.empty(1, dtype=F32, device=DEV)
        ops.sumsq(x, plain)
        r = _ref(x, [n], [0], 1)[0]
        # ssi_sumsq's own depth at this size (one trip, the two trees) is below this kernel's D: it lies within B of float64 as well, and the
        # two agree within B (not in bits: the blocks cut the buffer differently)
        assert abs(float(plain[0]) - r) <= b * r
        assert abs(float(got[0]) - float(plain[0])) <= b * r
    else:
        assert float(got[0]) == 0.0


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("wide", [False, True])
def test_interleaved_groups_nonadjacent_segments_and_an_empty_group(ops, dtype, wide):
    x = _data(N, dtype, seed=1, wide=wide)
    groups = (0, 1, 2, 0, 1, 4, 0, 2, 4)     # group 3 has no segment; 0, 1, 2 and 4 are made of non-adjacent segments
    got = _run(ops, x, ENDS, groups, 5)
    _check(got, _ref(x, ENDS, groups, 5), bound(N, dtype, len(ENDS)))
    assert float(got[3]) == 0.0
    # every segment its own group: every boundary kind decides a sum
    own = tuple(range(len(ENDS)))
    _check(_run(ops, x, ENDS, own, len(ENDS)), _ref(x, ENDS, own, len(ENDS)), bound(N, dtype, len(ENDS)))


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("skipped", [(0,), (8,), (0, 1, 4, 8), (1, 2, 3, 4, 5, 6, 7), tuple(range(9))])
def test_skipped_segments_are_not_read(ops, dtype, skipped):
    x = _data(N, dtype, seed=2)
    groups = [-1 if k in skipped else k % 3 for k in range(len(ENDS))]
    clean = _run(ops, x, ENDS, groups, 3)
    _check(clean, _ref(x, ENDS, groups, 3), bound(N, dtype, len(ENDS)))
    for poison in (float("nan"), float("inf")):
        y = x.clone()
        start = 0
        for k, e in enumerate(ENDS):
            if k in skipped:
                y[start:e] = poison
            start = e
        got = _run(ops, y, ENDS, groups, 3)
        assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(clean))
    if len(skipped) == len(ENDS):
        assert not clean.any()


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_isolation_and_reproducibility(ops, dtype):
    x = _data(N, dtype, seed=3, wide=True)
    groups = (0, 1, 2, 0, 1, 3, 0, 2, 3)
    base = _run(ops, x, ENDS, groups, 4)
    assert torch.equal(_bits(base), _bits(_run(ops, x, ENDS, groups, 4)))   # two launches, equal bits
    start = 0
    for k, e in enumerate(ENDS):
        for value in (3.0, float("nan"), float("-inf")):
            y = x.clone()
            y[start:e] = value
            got = _run(ops, y, ENDS, groups, 4)
            for g in range(4):
                if g != groups[k]:
                    assert _bits(got)[g] == _bits(base)[g], (k, value, g)
            assert value == 3.0 or not math.isfinite(float(got[groups[k]]))
        start = e


def test_out_is_overwritten(ops):
    x = _data(N, BF16, seed=4)
    groups = (0, 1, -1, 0, 1, 2, 0, -1, 2)
    want = _run(ops, x, ENDS, groups, 4)
    out = torch.full((4,), float("nan"), dtype=F32, device=DEV)
    _run(ops, x, ENDS, groups, 4, out=out)
    assert torch.equal(_bits(out), _bits(want))
    out.fill_(1e30)
    _run(ops, x[:0], [0], [0], 4, out=out)       # n == 0 zeroes, too
    assert not out.any()


def test_limits_and_argument_errors(ops):
    from ssi import _lib
    lib = _lib.load()
    n = 8 * 300
    x = _data(n, BF16, seed=5)
    ws = torch.empty(lib.ssi_sumsq_groups_workspace_bytes(n, 256, 64), dtype=torch.uint8, device=DEV)
    out = torch.full((65,), 7.0, dtype=F32, device=DEV)

    def rc(ends, groups, n_groups, n=n, ws_bytes=ws.numel()):
        k = len(ends)
        return lib.ssi_sumsq_groups(x.data_ptr(), n, _lib.SSI_BF16, (_lib.c_int64 * k)(*ends), (_lib.c_int32 * k)(*groups), k, n_groups,
                                    out.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr())

    full = [8 * (k + 1) for k in range(256)]
    assert rc(full[:255] + [n], [k % 64 for k in range(256)], 64) == 0             # the table filled: 256 segments, 64 groups
    ref = _ref(x, full[:255] + [n], [k % 64 for k in range(256)], 64)
    _check(out[:64], ref, bound(n, BF16, 256))
    out.fill_(7.0)
    assert rc([8 * (k + 1) for k in range(256)] + [n], [0] * 257, 1) == 2           # SSI_ERR_UNSUPPORTED: 257 segments
    assert rc([n], [0], 65) == 2                                                    # ... 65 groups
    assert rc([16, n], [0, 2], 2) == 1 and rc([16, n], [-2, 0], 2) == 1             # SSI_ERR_ARG: a group id out of range
    for ends in ([12, n], [32, 16, n], [32, 32, n], [32, n - 8], [32, n + 8]):      # ... bad ends
        assert rc(ends, [0] * len(ends), 1) == 1
    assert rc([16, n], [0, 1], 2, ws_bytes=2048 * 2 * 4 - 1) == 3                   # SSI_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0))                              # a refused call writes nothing
    with pytest.raises(RuntimeError):
        ops.sumsq_groups(x, [16, n], [0, 5], 2, out[:2])


def test_worst_fraction_of_the_bound_is_reported():
    print(f"sumsq_groups: worst |err| / (B ref) over this module's checks: {WORST['fraction']:.4f}")
    assert WORST["fraction"] <= 1.0
