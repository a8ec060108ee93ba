"""GPU: bf16 AdamW with stochastic rounding (``ssi_adamw_step_sr``, ``ssi_round_bf16_sr``; ABI v11) against the integer restatement in
``tests/sr_ref.py`` — bit for bit wherever the pre-rounding fp32 value does not depend on how a compiler contracts the expression, within the
two bf16 neighbours of an fp64 evaluation elsewhere — and the reason for the feature: a weight at 1.0 that round-to-nearest never moves."""
import pytest
import torch

import sr_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
N = 2 ** 20 + 3
SEEDS = (42_831, (1 << 40) + 12_345)                   # one above 2**32: the key's second word
ADAMW = dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)   # the reference's optimizer settings (conf/training.yaml)


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _bf16_grads(n, steps, seed):
    """A gradient that changes from step to step around a fixed direction (as tests/test_kernels_gpu.py makes it), bf16, before the scale."""
    base = rnd(n, seed=seed, scale=50.0)
    return [(base + rnd(n, seed=seed + 1 + t, scale=25.0)).to(BF16) for t in range(steps)]


def _from_bits(words):
    b = torch.tensor(words, dtype=torch.int64)
    return torch.where(b >= 2 ** 31, b - 2 ** 32, b).to(torch.int32).view(torch.float32)


_MIXED = {}


def _mixed_f32():
    """N fp32 values of mixed magnitude: the special ones first (so that the short cases meet them), then normals over 2**-140 .. 2**120 (the
    low end denormal), a stretch that bf16 holds exactly, and a stretch just below a power of two (carries into the exponent)."""
    if "x" not in _MIXED:
        g = torch.Generator().manual_seed(5)
        special = torch.cat([torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1.0, -1.0, 1.0 + 2.0 ** -8]),
                             _from_bits([0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0001, 0x7F7F0000, 0x00000001, 0x80000001, 0x0000FFFF, 0x00010000,
                                         0x007FFFFF, 0x3F7FFFFF, 0xBF7FFFFF, 0x3F80FFFF, 0x3F800001])])
        x = torch.randn(N, generator=g) * torch.exp2(torch.randint(-140, 120, (N,), generator=g).float())
        x[:special.numel()] = special
        x[1000:3000] = x[1000:3000].to(BF16).float()
        x[3000:5000] = _from_bits((0x3F7F0000 + torch.randint(0, 65536, (2000,), generator=g)).tolist())
        _MIXED["x"] = x
    return _MIXED["x"]


# ---- G1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, N])
def test_rounding_entry_is_the_restatement_bit_for_bit(ops, n):
    """``ssi_round_bf16_sr``: rounding, generator and indexing in one — two seeds, two steps (one with the top bit of its word set), the three
    tensor ids, element offsets 0, 8, 2**33 + 8 and 2**35 + 16 (the second counter word); short inputs slide over the special values."""
    x = _mixed_f32()
    starts = (0,) if n == N else (0, 2, 4, 7, 9, 13, 1000, 3000)
    checked = 0
    for start in starts:
        src = x[start:start + n].clone()
        dsrc = src.to(DEV)
        for seed in SEEDS:
            for step in (1, 4_000_000_000):
                for tensor in (0, 1, 2):
                    for i, off in enumerate((0, 8, 2 ** 33 + 8, 2 ** 35 + 16)):
                        if n == N and tensor != (i + (step & 1) + (seed & 1)) % 3:
                            continue      # (the long case: every seed x step x offset, the tensor id going round; the short ones: every product)
                        out = torch.full((n,), 7.0, dtype=BF16, device=DEV)
                        ops.round_bf16_sr(dsrc, out, seed=seed, step=step, tensor=tensor, elem_offset=off)
                        ref = sr_ref.round_bf16_sr(src, seed=seed, step=step, tensor=tensor, elem_offset=off)
                        assert sr_ref.same_bf16(out, ref), (n, start, seed, step, tensor, off)
                        checked += 1
    assert checked >= 16


# ---- G2 ---------------------------------------------------------------------------------------------------------------------------------
def _decay_case(n, seed):
    """g = 0 and m = v = 0: the step leaves p * (float)(1 - lr wd) and nothing else, one fp32 multiplication whatever the compiler does."""
    hyper = dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=10.0, step=3)
    p0 = rnd(n, seed=seed, scale=0.02).to(BF16)
    if n > 1000:
        p0[:1000] = 1.0
    pf, mf, vf = sr_ref.adamw_f32(p0, torch.zeros(n), torch.zeros(n), torch.zeros(n), **hyper)
    # the test's own precondition: the fp32 product is the fp64 product (exact: 8 x 24 bits) rounded once
    decay64 = sr_ref.adamw_coefficients(**hyper)["decay"].double()
    assert torch.equal(pf, (p0.double() * decay64).float()) and not bool(mf.any()) and not bool(vf.any())
    return hyper, p0, pf


def test_parameter_stream_through_adamw_bit_for_bit(ops):
    hyper, p0, pf = _decay_case(N, seed=21)
    for seed, off in ((SEEDS[0], 0), (SEEDS[1], 2 ** 33 + 8)):
        want = sr_ref.round_bf16_sr(pf, seed=seed, step=hyper["step"], tensor=sr_ref.TENSOR_PARAM, elem_offset=off)
        moved = float((sr_ref.bf16_bits(want) != sr_ref.bf16_bits(p0)).double().mean())
        print(f"weight decay 10 at lr 2e-4: {moved:.4f} of the weights move (round-to-nearest: {float((pf.to(BF16) != p0).double().mean()):.4f})")
        assert 0.25 < moved < 0.5                      # expected about 0.37: the mean of frac(|p| * 0.002 / ulp) over the weights
        p, g, m, v = p0.to(DEV), torch.zeros(N, dtype=BF16, device=DEV), torch.zeros(N, dtype=BF16, device=DEV), torch.zeros(N, dtype=BF16, device=DEV)
        ops.adamw_step(p, g, m, v, **hyper, sr_seed=seed, elem_offset=off)
        assert sr_ref.same_bf16(p, want)
        assert not bool(m.any()) and not bool(v.any()) and not bool(g.any())
        assert torch.equal(sr_ref.bf16_bits(m.cpu()), torch.zeros(N, dtype=torch.int64))      # +0, not -0


# ---- G3 ---------------------------------------------------------------------------------------------------------------------------------
def test_moment_streams_through_adamw_bit_for_bit(ops):
    """beta1 = 0.75, beta2 = 0.5 and operands whose exponents lie close: m + 0.25 (g - m) and 0.5 v + 0.5 g g are exact in fp32, so the value
    that reaches the rounding cannot depend on contraction, and nearly all of them have bits below the bf16 mantissa."""
    gen = torch.Generator().manual_seed(31)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(N, generator=gen)                     # noqa: E731
    sign = lambda: torch.randint(0, 2, (N,), generator=gen).float() * 2 - 1               # noqa: E731
    m0 = (sign() * u(0.5, 2.0)).to(BF16)
    g0 = (sign() * torch.exp2(u(-6.0, -4.0))).to(BF16)
    v0 = torch.exp2(u(-8.0, -6.0)).to(BF16)
    p0 = rnd(N, seed=32, scale=0.02).to(BF16)
    hyper = dict(lr=2e-4, beta1=0.75, beta2=0.5, eps=1e-8, weight_decay=0.01, step=5)
    _, mf, vf = sr_ref.adamw_f32(p0, g0, m0, v0, **hyper)
    _, m64, v64 = sr_ref.adamw_f32(p0, g0, m0, v0, **hyper, dtype=torch.float64)
    assert torch.equal(mf.double(), m64) and torch.equal(vf.double(), v64)               # precondition: fp32 == fp64, exactly
    low_m = float(((sr_ref.f32_bits(mf) & 0xFFFF) != 0).double().mean())
    low_v = float(((sr_ref.f32_bits(vf) & 0xFFFF) != 0).double().mean())
    print(f"values with bits below the bf16 mantissa: m {low_m:.4f} v {low_v:.4f}")
    assert low_m > 0.9 and low_v > 0.9
    seed, off = SEEDS[1], 16
    p, g, m, v = (t.to(DEV) for t in (p0, g0, m0, v0))
    ops.adamw_step(p, g, m, v, **hyper, sr_seed=seed, elem_offset=off)
    assert sr_ref.same_bf16(m, sr_ref.round_bf16_sr(mf, seed=seed, step=5, tensor=sr_ref.TENSOR_EXP_AVG, elem_offset=off))
    assert sr_ref.same_bf16(v, sr_ref.round_bf16_sr(vf, seed=seed, step=5, tensor=sr_ref.TENSOR_EXP_AVG_SQ, elem_offset=off))
    assert torch.equal(g.cpu(), g0)


# ---- G4 ---------------------------------------------------------------------------------------------------------------------------------
def test_every_store_stays_within_the_two_neighbours(ops):
    """The reference's hyper-parameters, six steps of a changing gradient with the scale 2**-6, every step judged from ITS OWN inputs: an fp64
    evaluation x64 of the kernel's expressions (same fp32 coefficients).  The kernel rounds its fp32 value x32 to one of x32's two bf16
    neighbours, so |stored - x32| < one bf16 step at x32 and |stored - x64| < step + |x32 - x64|.

    The fp32 evaluation error (eps = 2**-24 per operation, relative to that operation's result; the scale 2**-6 is exact), not tuned:
      m: three roundings (g - m, w1 *, m +), each of a result no larger than |g| + |m|:                   d_m <= 4 eps (|g| + |m|)
      v: four roundings of positive terms no larger than the result:                                      d_v <= 4 eps v'
      p: p * decay is one rounding (eps |p|), the subtraction another; the update U = step_size m' / (sqrt(v') / sqrt(bc2) + eps) carries m'
         with its absolute error d_m, sqrt(v') with half of v's relative error plus its own rounding, and three more roundings
         (the product with 1 / sqrt(bc2), the sum, the quotient, the product: 8 eps bounds them all):      d_p <= 2 eps |p| + 8 eps |U| + |U| d_m / |m'|
    The bf16 step is taken at the larger of |x64| and |stored| (x32 may lie across a power of two from x64)."""
    from bf16_dist import bf16_spacing
    n, steps, eps32 = N, 6, 2.0 ** -24
    grads = _bf16_grads(n, steps, seed=20)
    for gb in grads:
        gb[:1000] = 0                                   # m and v of these stay exactly +0, and their U is exactly 0
    p0 = rnd(n, seed=19, scale=0.02).to(BF16)
    p0[:500] = 0                                        # ... and these weights stay exactly 0
    gs = torch.tensor([2.0 ** -6], device=DEV)
    p, m, v = p0.to(DEV), torch.zeros(n, dtype=BF16, device=DEV), torch.zeros(n, dtype=BF16, device=DEV)
    for step, gb in enumerate(grads, 1):
        before = [t.cpu() for t in (p, m, v)]
        gsc = gb.double() * 2.0 ** -6
        x64 = sr_ref.adamw_f32(before[0], gsc, before[1], before[2], **ADAMW, step=step, dtype=torch.float64)
        x32 = sr_ref.adamw_f32(before[0], gsc.float(), before[1], before[2], **ADAMW, step=step)
        ops.adamw_step(p, gb.to(DEV), m, v, **ADAMW, step=step, grad_scale_dev=gs, sr_seed=SEEDS[0], elem_offset=64)
        after = [t.cpu() for t in (p, m, v)]
        p64, m64, v64 = x64
        d_m = 4 * eps32 * (gsc.abs() + before[1].double().abs())
        d_v = 4 * eps32 * v64
        upd = (before[0].double() * sr_ref.adamw_coefficients(**ADAMW, step=step)["decay"].double() - p64).abs()
        d_p = 2 * eps32 * before[0].double().abs() + 8 * eps32 * upd + torch.where(m64 != 0, upd * d_m / m64.abs(), torch.zeros_like(upd))
        for name, got, want, want32, d in (("p", after[0], p64, x32[0], d_p), ("m", after[1], m64, x32[1], d_m), ("v", after[2], v64, x32[2], d_v)):
            assert bool(torch.isfinite(got.float()).all())
            step_bf16 = bf16_spacing(torch.maximum(want.abs(), got.double().abs()))
            over = ((got.double() - want).abs() - d) / step_bf16
            moved = float((sr_ref.bf16_bits(got) != sr_ref.bf16_bits(want.float().to(BF16))).double().mean())
            print(f"step {step} {name}: largest distance from fp64 beyond the fp32 error {float(over.max()):.4f} bf16 steps; "
                  f"differs from round-to-nearest in {moved:.4f} of the elements")
            assert float(over.max()) < 1.0, (step, name)
            # a value bf16 holds exactly (fp32 and fp64 agreeing on it, so there is no doubt about x32) is stored as it is
            exact = (want32.double() == want) & (want == want.float().to(BF16).double())
            assert int(exact.sum()) >= (500 if name == "p" else 1000)
            assert torch.equal(sr_ref.bf16_bits(got)[exact], sr_ref.bf16_bits(want.float().to(BF16))[exact]), (step, name)
    assert not bool(after[1][:1000].any()) and not bool(after[2][:1000].any()) and not bool(after[0][:500].any())


# ---- G5 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_weight_at_one_moves_only_with_stochastic_rounding(ops):
    """p = 1.0, g = 1, lr 2e-4, no weight decay, 64 steps; exact: p = 1 - 64 lr, m = 1 - 0.9**64, v = 1 - 0.999**64.  To nearest, p never
    leaves 1.0 (lr is a twentieth of the bf16 step below 1.0).  Stochastically: each element's walk has std <= 2**-9 sqrt(64) = 0.0156, the
    mean over 2**20 elements 1.5e-5, so 2e-4 is 13 sigma of a displacement of 1.28e-2."""
    n, steps, lr = 2 ** 20, 64, 2e-4
    hyper = dict(lr=lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0)
    out = {}
    for mode, seed in (("nearest", None), ("stochastic", SEEDS[0])):
        p, g = torch.ones(n, dtype=BF16, device=DEV), torch.ones(n, dtype=BF16, device=DEV)
        m, v = torch.zeros(n, dtype=BF16, device=DEV), torch.zeros(n, dtype=BF16, device=DEV)
        for step in range(1, steps + 1):
            ops.adamw_step(p, g, m, v, **hyper, step=step, sr_seed=seed)
        out[mode] = [t.double() for t in (p, m, v)]
    p, m, v = out["nearest"]
    assert bool((p == 1.0).all())                                         # the defect: 64 updates, every one of them dropped
    p, m, v = out["stochastic"]
    still = float((p == 1.0).double().mean())
    print(f"stochastic: mean p {float(p.mean()):.7f} (exact {1 - steps * lr:.7f}) mean m {float(m.mean()):.6f} ({1 - 0.9 ** steps:.6f}) "
          f"mean v {float(v.mean()):.7f} ({1 - 0.999 ** steps:.7f}) still 1.0: {still:.4f}")
    assert abs(float(p.mean()) - (1 - steps * lr)) <= 2e-4
    assert abs(float(m.mean()) - (1 - 0.9 ** steps)) <= 1e-3
    assert abs(float(v.mean()) / (1 - 0.999 ** steps) - 1) <= 1e-2
    assert still < 0.5


# ---- G6 ---------------------------------------------------------------------------------------------------------------------------------
def _state(n, seed):
    return [rnd(n, seed=seed, scale=0.02).to(BF16), _bf16_grads(n, 1, seed=seed + 1)[0], rnd(n, seed=seed + 3, scale=0.2).to(BF16),
            rnd(n, seed=seed + 4, scale=0.5).square().to(BF16)]


def test_slices_with_their_offsets_are_the_whole_call(ops):
    """One call over [0, n) == calls over [0, 8k) and [8k, n) with elem_offset 0 and 8k (buckets, the overlap path, the data-parallel deferred
    range all rest on this); another offset, step or seed gives other bits."""
    n, cut, base = N, 8 * 40_001, 2 ** 33 + 8
    gs = torch.tensor([2.0 ** -6], device=DEV)
    host = _state(n, seed=60)

    def run(pieces, seed=SEEDS[0], step=3, shift=0):
        bufs = [t.to(DEV) for t in host]
        for lo, hi in pieces:
            ops.adamw_step(*(b[lo:hi] for b in bufs), **ADAMW, step=step, grad_scale_dev=gs, sr_seed=seed, elem_offset=base + lo + shift)
        return [sr_ref.bf16_bits(b.cpu()) for b in bufs]

    whole = run([(0, n)])
    for pieces in ([(0, cut), (cut, n)], [(cut, n), (0, cut)], [(0, 8), (8, cut), (cut, n - 3), (n - 3, n)]):
        for a, b in zip(whole, run(pieces)):
            assert torch.equal(a, b), pieces
    assert torch.equal(whole[1], sr_ref.bf16_bits(host[1]))               # g untouched
    for kw in (dict(shift=8), dict(step=4), dict(seed=SEEDS[1])):
        other = run([(0, n)], **kw)
        for name, a, b in zip("pmv", (whole[0], whole[2], whole[3]), (other[0], other[2], other[3])):
            same = float((a == b).double().mean())
            assert same < 0.9, (kw, name, same)                           # (about half of the roundings agree by chance; step also moves the values)


@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_tails_and_guards(ops, n):
    """buf[8:8+n] of a larger buffer (all tail for n < 8, one vector for 8, a vector and a tail for 9): the n elements are the restatement's
    (the g = 0 case, where the fp32 value is one multiplication), the guards on both sides stay bit-identical."""
    hyper, p0, pf = _decay_case(n, seed=80 + n)
    want = sr_ref.round_bf16_sr(pf, seed=SEEDS[0], step=hyper["step"], tensor=sr_ref.TENSOR_PARAM, elem_offset=8)
    bufs = []
    for fill in (p0, torch.zeros(n), torch.zeros(n), torch.zeros(n)):
        b = rnd(n + 24, seed=n + 50, scale=3.0).to(BF16)
        b[8:8 + n] = fill
        bufs.append(b.to(DEV))
    before = [sr_ref.bf16_bits(b.cpu()) for b in bufs]
    ops.adamw_step(*(b[8:8 + n] for b in bufs), **hyper, sr_seed=SEEDS[0], elem_offset=8, zero_grad=True)
    after = [sr_ref.bf16_bits(b.cpu()) for b in bufs]
    for a, b0 in zip(after, before):
        assert torch.equal(a[:8], b0[:8]) and torch.equal(a[8 + n:], b0[8 + n:]), "guards"
    assert torch.equal(after[0][8:8 + n], sr_ref.bf16_bits(want))
    assert not bool(after[1][8:8 + n].any()) and not bool(after[2][8:8 + n].any()) and not bool(after[3][8:8 + n].any())


# ---- G7 ---------------------------------------------------------------------------------------------------------------------------------
def test_flag_bits_and_argument_errors(ops):
    from ssi import _lib
    n = 1003
    host = _state(n, seed=70)

    def mk():
        bufs = []
        for fill in host:
            b = rnd(n + 24, seed=71, scale=3.0).to(BF16)
            b[8:8 + n] = fill
            bufs.append(b.to(DEV))
        return bufs

    bits = lambda t: sr_ref.bf16_bits(t.cpu())             # noqa: E731
    s = torch.tensor([2.0 ** -6], device=DEV)
    call = lambda bufs, scale, **kw: ops.adamw_step(*(b[8:8 + n] for b in bufs), **ADAMW, step=3, grad_scale_dev=scale, sr_seed=SEEDS[0],   # noqa: E731
                                                    elem_offset=8, **kw)
    before = [bits(b) for b in mk()]
    for bad in (float("inf"), float("-inf"), float("nan")):
        bufs = mk()
        call(bufs, torch.tensor([bad], device=DEV), zero_grad=True, skip_nonfinite_scale=True)
        for b, b0 in zip(bufs, before):
            assert torch.equal(bits(b), b0), bad
    bufs = mk()
    call(bufs, s, zero_grad=True, skip_nonfinite_scale=True)
    g = bits(bufs[1])
    assert not bool(g[8:8 + n].any()) and torch.equal(g[:8], before[1][:8]) and torch.equal(g[8 + n:], before[1][8 + n:])
    assert not torch.equal(bits(bufs[0]), before[0])
    plain = mk()
    call(plain, s)
    assert torch.equal(bits(plain[1]), before[1])                          # no zeroing requested: g unchanged
    for i in (0, 2, 3):
        assert torch.equal(bits(plain[i]), bits(bufs[i]))                  # ... and the flag changes nothing else
    # argument errors: fp32 storage, an offset off the vector grid, a step that does not fit the counter word
    f32 = [torch.zeros(16, device=DEV) for _ in range(4)]
    with pytest.raises(RuntimeError, match="ssi_adamw_step_sr failed with code 1:"):
        ops.adamw_step(*f32, **ADAMW, step=3, sr_seed=1)
    b16 = [torch.zeros(16, dtype=BF16, device=DEV) for _ in range(4)]
    for kw in (dict(step=3, elem_offset=4), dict(step=3, elem_offset=-8), dict(step=2 ** 32), dict(step=0)):
        with pytest.raises(RuntimeError, match="ssi_adamw_step_sr failed with code 1:"):
            ops.adamw_step(*b16, **ADAMW, sr_seed=1, **kw)
    ops.adamw_step(*b16, **ADAMW, step=2 ** 32 - 1, sr_seed=1, elem_offset=2 ** 40)     # the largest step, a far offset: fine
    src, dst = torch.zeros(16, device=DEV), torch.zeros(16, dtype=BF16, device=DEV)
    for kw in (dict(step=2 ** 32, tensor=0), dict(step=1, tensor=0, elem_offset=3), dict(step=1, tensor=-1)):
        with pytest.raises(RuntimeError, match="ssi_round_bf16_sr failed with code 1:"):
            ops.round_bf16_sr(src, dst, seed=1, **kw)
    assert _lib.load().ssi_abi_version() >= 11
    torch.cuda.synchronize()
