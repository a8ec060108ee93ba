"""``ssi_ema_update`` (``ops.ema_update``): ``ema[i] = fma(decay, ema[i] - p, p)`` in fp32 on bf16 and fp32 parameters.

Inputs of every case: parameters drawn log-uniformly in ``[2^-6, 4)`` with a random sign, the average = the parameter times ``1 + r`` with ``|r|``
log-uniform in ``[2^-10, 1)`` and a random sign, the decays 0.5, 0.999 and 0.9999 rounded to fp32.

Reference: ``(p.double() + float(decay32) * (e - p).double()).float()`` with ``e - p`` first taken in fp32.  The product is exact in fp64 (24 x 24
bits), the fp64 sum is rounded once to 53 bits and then again to 24: it can differ from the kernel's single rounding only where the exact sum
lies within 2^-29 (relative to an fp32 ulp) of a rounding midpoint, about one element in 2^29.  So every element must be within 1 fp32 ulp and
the elements that are not bit-equal must number at most ``max(1, n // 10**5)`` — a cap a wrong arithmetic cannot stay inside: an unfused
multiply-add (product rounded to fp32 first) misses 7 % of these inputs at decay 0.999 and 0.9999 (none at 0.5, where the product is exact).  ``test_reference_against_exact_integers`` (CPU) checks the
reference itself: on 6000 elements per decay it is bit-equal to the exact rational value of ``decay * d + p`` rounded once to fp32 with Python
integers, i.e. inside the cap; and it shows that the unfused form is far outside it.

Sizes: the launch is ``min(ceil((n / 8 + 1) / 256), 2^20)`` blocks of 256 threads, 8 elements per thread and trip, so ONE grid pass covers up to
2^31 elements and none of 1, 7, 8, 9, 255, 2048 + 3, 2^20 + 5 (below one vector, the exact vector, tails, several blocks) reaches the stride
loop's second trip.  The smallest size that does is 2^31 + 8: ``test_beyond_one_grid_pass`` runs 2^31 + 2048 + 3 (bf16 parameters, one decay;
also the first size whose element index passes 2^31), generated and checked in chunks on the device."""
import struct
from fractions import Fraction

import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda"
DECAYS = tuple(struct.unpack("f", struct.pack("f", d))[0] for d in (0.5, 0.999, 0.9999))
SIZES = (1, 7, 8, 9, 255, 2048 + 3, 2 ** 20 + 5)
DTYPES = [torch.bfloat16, torch.float32]
CHUNK = 1 << 26


def _inputs(n, dtype, seed, device):
    """(param in ``dtype``, ema fp32); drawn chunk by chunk on ``device`` so that the largest case needs no fp64 temporaries of its size."""
    g = torch.Generator(device=device).manual_seed(seed)
    p, e = torch.empty(n, dtype=dtype, device=device), torch.empty(n, dtype=torch.float32, device=device)
    for lo in range(0, n, CHUNK):
        k = min(CHUNK, n - lo)

        def rand():
            return torch.rand(k, generator=g, dtype=torch.float32, device=device)

        def sign():
            return torch.where(rand() < 0.5, -1.0, 1.0)

        pc = (torch.exp2(rand() * 8 - 6).clamp(max=3.98) * sign()).to(dtype)
        p[lo:lo + k] = pc
        e[lo:lo + k] = pc.float() * (1 + torch.exp2(rand() * 10 - 10) * sign())
    return p, e


def _reference(p, e, decay32):
    return (p.double() + float(decay32) * (e - p.float()).double()).float()


def _ulps(a, b):
    return (a.view(torch.int32).long() - b.view(torch.int32).long()).abs()


def _check(out, ref, n, what):
    """The acceptance of the module docstring; returns the number of elements that are not bit-equal."""
    assert bool(torch.isfinite(out).all()) and bool((torch.signbit(out) == torch.signbit(ref)).all()), what
    d = _ulps(out, ref)
    worst, off = int(d.max()), int((d != 0).sum())
    assert worst <= 1, (what, worst)
    assert off <= max(1, n // 10 ** 5), (what, off)
    return off


# ---- the reference itself, on the CPU ---------------------------------------------------------------------------------------------------------
def _round_f32(x: Fraction) -> float:
    """``x`` rounded once to the nearest fp32, ties to even (normal range only)."""
    if x == 0:
        return 0.0
    s, a = (-1 if x < 0 else 1), abs(x)
    ex = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** ex > a:
        ex -= 1                                                                           # 2^ex <= a < 2^(ex + 1)
    assert -126 <= ex <= 127
    q = a / Fraction(2) ** (ex - 23)                                                     # in [2^23, 2^24)
    m, r = divmod(q.numerator, q.denominator)
    if 2 * r > q.denominator or (2 * r == q.denominator and m % 2 == 1):
        m += 1
    return s * float(m) * 2.0 ** (ex - 23)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_reference_against_exact_integers(dtype):
    n = 6000
    p, e = _inputs(n, dtype, 3, "cpu")
    for decay in DECAYS:
        ref = _reference(p, e, decay)
        d32 = e - p.float()
        exact = torch.tensor([_round_f32(Fraction(decay) * Fraction(float(d)) + Fraction(float(x))) for d, x in zip(d32.tolist(), p.float().tolist())],
                             dtype=torch.float32)
        assert _check(ref, exact, n, ("reference", decay)) == 0
        unfused = (decay * d32) + p.float()                                                # product rounded to fp32, then the sum
        missed = int((_ulps(unfused, exact) != 0).sum())
        print(f"{dtype} decay {decay!r}: the unfused form misses {missed} of {n}")
        if decay != 0.5:                                                                   # (times a power of two the product is exact either way)
            assert missed > n // 20, "the cap must tell an unfused multiply-add from the fused one"


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_sizes_and_decays_against_the_reference(n, dtype):
    from ssi import ops
    p, e0 = _inputs(n, dtype, 100 + n, DEV)
    p0 = p.clone()
    for decay in DECAYS:
        e = e0.clone()
        ops.ema_update(e, p, decay=decay)
        off = _check(e, _reference(p, e0, decay), n, (n, dtype, decay))
        print(f"n {n} {dtype} decay {decay!r}: {off} of {n} not bit-equal to the reference")
        assert not torch.equal(e, e0) and torch.equal(p, p0)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_slices_leave_their_surroundings_alone(dtype):
    from ssi import ops
    total = 3 * 4096 + 37
    p, e0 = _inputs(total, dtype, 7, DEV)
    for lo, hi in ((8, 8 + 1), (8, 4096 + 13), (64, 64 + 255), (4096, 2 * 4096), (8000, total), (0, total - 1)):
        assert lo % 8 == 0
        e, pc = e0.clone(), p.clone()
        ops.ema_update(e[lo:hi], pc[lo:hi], decay=DECAYS[1])
        _check(e[lo:hi], _reference(p[lo:hi], e0[lo:hi], DECAYS[1]), hi - lo, (lo, hi))
        assert torch.equal(e[:lo], e0[:lo]) and torch.equal(e[hi:], e0[hi:]) and torch.equal(pc.view(torch.uint8), p.view(torch.uint8)), (lo, hi)


@gpu
def test_beyond_one_grid_pass():
    from ssi import ops
    n = 2 ** 31 + 2048 + 3
    need = n * (4 + 4 + 2) + 16 * CHUNK * 8
    if torch.cuda.mem_get_info()[0] < need:
        pytest.fail(f"needs {need / 2 ** 30:.0f} GiB of free device memory")
    decay = DECAYS[1]
    p, e = _inputs(n, torch.bfloat16, 11, DEV)
    e0 = e.clone()
    ops.ema_update(e, p, decay=decay)
    off = 0
    for lo in range(0, n, CHUNK):
        sl = slice(lo, min(lo + CHUNK, n))
        off += _check(e[sl], _reference(p[sl], e0[sl], decay), n, ("chunk at", lo))
    print(f"n {n}: {off} not bit-equal to the reference")
    assert off <= max(1, n // 10 ** 5)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_exact_properties(dtype):
    from ssi import ops
    n = 2048 + 3
    p, e0 = _inputs(n, dtype, 5, DEV)
    e = e0.clone()
    ops.ema_update(e, p, decay=0.0)                                                      # decay 0: the parameter itself
    assert torch.equal(e, p.float())
    for decay in DECAYS:                                                                 # ema == p is a fixed point
        ops.ema_update(e, p, decay=decay)
        assert torch.equal(e, p.float())
    for guard in (float("inf"), float("-inf"), float("nan")):                            # a non-finite guard: nothing moves
        e = e0.clone()
        ops.ema_update(e, p, decay=DECAYS[0], guard_dev=torch.full((1,), guard, dtype=torch.float32, device=DEV))
        assert torch.equal(e, e0)
    plain = e0.clone()
    ops.ema_update(plain, p, decay=DECAYS[0])
    for guard in (1.0, 1e-3):                                                            # a finite one: the plain update, whatever its value
        e = e0.clone()
        ops.ema_update(e, p, decay=DECAYS[0], guard_dev=torch.full((1,), guard, dtype=torch.float32, device=DEV))
        assert torch.equal(e, plain) and not torch.equal(e, e0)
    ops.ema_update(torch.empty(0, dtype=torch.float32, device=DEV), torch.empty(0, dtype=dtype, device=DEV), decay=0.9)   # n = 0 is fine
    torch.cuda.synchronize()


@gpu
def test_errors():
    from ssi import ops
    n = 64
    p, e = _inputs(n, torch.bfloat16, 9, DEV)
    e0 = e.clone()
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(RuntimeError, match="ssi_ema_update failed with code"):
            ops.ema_update(e, p, decay=bad)
    with pytest.raises(RuntimeError, match="ssi_ema_update failed with code"):            # the average 4 bytes off a 16-byte boundary
        ops.ema_update(e[1:33], p[8:40], decay=0.9)
    with pytest.raises(RuntimeError, match="ssi_ema_update failed with code"):            # the parameters 4 bytes off
        ops.ema_update(e[8:40], p[2:34], decay=0.9)
    pf = p.float()
    with pytest.raises(RuntimeError, match="ssi_ema_update failed with code"):
        ops.ema_update(e[8:40], pf[1:33], decay=0.9)
    with pytest.raises(TypeError):
        ops.ema_update(e.to(torch.bfloat16), p, decay=0.9)
    torch.cuda.synchronize()
    assert torch.equal(e, e0)
