"""CPU: the integer restatement (``tests/sr_ref.py``) of the stochastic rounding behind ``HipAdamW(stochastic_rounding=True)`` — the generator
against its published known answers, the rounding's properties over ALL 65 536 values of the random bits, and the stagnation that is the
reason for the feature: a bf16 weight at 1.0 that round-to-nearest never moves."""
import math

import pytest
import torch

import sr_ref


def _words(s):
    return [int(w, 16) for w in s.split()]


@pytest.mark.parametrize("counter,key,out", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, out):
    got = [int(w) for w in sr_ref.philox4x32_10(_words(counter), _words(key))]
    assert got == _words(out), [f"{w:08x}" for w in got]


def test_random_bits_follow_the_global_element_index():
    """Element e takes half-word e & 7 of the generator call with counter (e >> 3 low, e >> 3 high, step, tensor) and key (seed low, seed high):
    the same bits whichever slice of the buffer a call sees."""
    seed, step, tensor = (0x299f31d0 << 32) | 0xa4093822, 0x13198a2e, 2
    e0 = ((5 << 32) | 0x243f6a88) << 3                  # vector index with a high word: counter (0x243f6a88, 5, step, tensor)
    r = sr_ref.random_bits(11, seed, step, tensor, elem_offset=e0)
    w = [int(x) for x in sr_ref.philox4x32_10((0x243f6a88, 5, step, tensor), (0xa4093822, 0x299f31d0))]
    assert [int(x) for x in r[:8]] == [w[0] & 0xFFFF, w[0] >> 16, w[1] & 0xFFFF, w[1] >> 16, w[2] & 0xFFFF, w[2] >> 16, w[3] & 0xFFFF, w[3] >> 16]
    w = [int(x) for x in sr_ref.philox4x32_10((0x243f6a89, 5, step, tensor), (0xa4093822, 0x299f31d0))]
    assert [int(x) for x in r[8:]] == [w[0] & 0xFFFF, w[0] >> 16, w[1] & 0xFFFF]
    whole = sr_ref.random_bits(1003, 7, 3, 1, elem_offset=64)
    assert torch.equal(whole[40:], sr_ref.random_bits(1003 - 40, 7, 3, 1, elem_offset=104))
    for other in (sr_ref.random_bits(1003, 8, 3, 1, 64), sr_ref.random_bits(1003, 7, 4, 1, 64), sr_ref.random_bits(1003, 7, 3, 2, 64),
                  sr_ref.random_bits(1003, 7, 3, 1, 72)):
        assert float((other == whole).double().mean()) < 0.01
    assert abs(float(whole.double().mean()) / 65535 - 0.5) < 0.05


def _samples():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4096, generator=g) * torch.exp2(torch.randint(-140, 120, (4096,), generator=g).float())   # denormals to 1e36
    exact = x[:512].to(torch.bfloat16).float()
    big = torch.tensor([0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0001, 0x7F7F0000, 0x00000001, 0x80000001, 0x0000FFFF], dtype=torch.int64)
    big = torch.where(big >= 2 ** 31, big - 2 ** 32, big).to(torch.int32).view(torch.float32)
    return torch.cat([x, exact, big, torch.tensor([0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -23])])


def test_sr_bf16_properties():
    x = _samples()
    u = sr_ref.f32_bits(x)
    low = u & 0xFFFF
    special = torch.tensor([float("inf"), float("-inf"), float("nan"), 0.0, -0.0])
    for r in (0, 1, 0x8000, 0xFFFF):
        out = sr_ref.sr_bf16(special, r)
        assert sr_ref.same_bf16(out, special.to(torch.bfloat16)) and bool(out[2].isnan()), r
        assert torch.equal(sr_ref.bf16_bits(out)[[0, 1, 3, 4]], torch.tensor([0x7F80, 0xFF80, 0x0000, 0x8000])), r
        assert torch.equal(sr_ref.bf16_bits(sr_ref.sr_bf16(x, r))[low == 0], (u >> 16)[low == 0]), "a value bf16 holds must not change"
    down = sr_ref.bf16_bits(sr_ref.sr_bf16(x, 0))
    up = sr_ref.bf16_bits(sr_ref.sr_bf16(x, 0xFFFF))
    assert torch.equal(down, u >> 16)                                                        # r = 0 truncates toward zero
    top = (u >> 16) & 0x7FFF == 0x7F7F                                                       # the largest finite bf16 magnitude: nowhere to go
    inexact = (low != 0) & ~top
    assert torch.equal(up[inexact], (u >> 16)[inexact] + 1) and torch.equal(up[~inexact], (u >> 16)[~inexact])
    assert bool((sr_ref.sr_bf16(x, 0xFFFF).float().abs() >= x.abs())[~top].all())            # ... away from zero, whatever the sign
    assert bool(torch.isfinite(sr_ref.sr_bf16(x, 0xFFFF).float()).all()) and int(top.sum()) >= 4
    # over all 65 536 values of r, exactly (u & 0xFFFF) of them round away from zero
    some = x[::37]
    us = sr_ref.f32_bits(some)
    r_all = torch.arange(65536, dtype=torch.int64)[:, None]
    got = sr_ref.bf16_bits(sr_ref.sr_bf16(some[None, :].expand(65536, -1).contiguous(), r_all))
    away = (got != (us >> 16)[None, :]).sum(0)
    assert bool(((got == (us >> 16)) | (got == (us >> 16) + 1)).all())
    stuck = (us >> 16) & 0x7FFF == 0x7F7F
    assert torch.equal(away[~stuck], (us & 0xFFFF)[~stuck]) and bool((away[stuck] == 0).all())


def test_a_weight_at_one_moves_only_with_stochastic_rounding():
    """p = 1.0, g = 1, lr 2e-4, no weight decay, the reference's betas, 64 steps.  Exact: p = 1 - 64 lr (m-hat / sqrt(v-hat) = 1 at every step),
    m = 1 - 0.9**64, v = 1 - 0.999**64.  Rounded to nearest, p is still 1.0 bit for bit (lr is a twentieth of the bf16 step below 1.0).
    Rounded stochastically every store is unbiased; bounds of the GPU test (n = 2**20: 2e-4 on mean p = 13 sigma of a 64-step random walk of
    bf16 steps 2**-9, 1e-3 on mean m, 1 % on mean v) scaled by sqrt(2**20 / n) for the n used here."""
    n, steps, lr = 2 ** 14, 64, 2e-4
    scale = math.sqrt(2 ** 20 / n)
    hyper = dict(lr=lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0)
    g = torch.ones(n, dtype=torch.bfloat16)
    state = {mode: [torch.ones(n, dtype=torch.bfloat16), torch.zeros(n, dtype=torch.bfloat16), torch.zeros(n, dtype=torch.bfloat16)]
             for mode in ("nearest", "stochastic")}
    for step in range(1, steps + 1):
        state["nearest"] = list(sr_ref.adamw_step_ref(state["nearest"][0], g, *state["nearest"][1:], step=step, **hyper))
        state["stochastic"] = list(sr_ref.adamw_step_ref(state["stochastic"][0], g, *state["stochastic"][1:], step=step, seed=42_831, **hyper))
    p, m, v = state["nearest"]
    assert bool((p == 1.0).all())
    assert float(m.double().mean()) < 1 - 0.9 ** 64 - 1e-2            # exp_avg stalls too (at 0.984375 against 0.99882)
    p, m, v = (t.double() for t in state["stochastic"])
    print(f"stochastic: mean p {p.mean():.6f} (exact {1 - steps * lr:.6f}) mean m {m.mean():.6f} ({1 - 0.9 ** steps:.6f}) "
          f"mean v {v.mean():.7f} ({1 - 0.999 ** steps:.7f}) still 1.0: {float((p == 1.0).double().mean()):.4f}")
    assert abs(float(p.mean()) - (1 - steps * lr)) <= 2e-4 * scale
    assert abs(float(m.mean()) - (1 - 0.9 ** steps)) <= 1e-3 * scale
    assert abs(float(v.mean()) / (1 - 0.999 ** steps) - 1) <= 1e-2 * scale
    assert float((p == 1.0).double().mean()) < 0.5


def test_setup_optimizer_strips_or_refuses_the_keys_for_a_foreign_module():
    """A module without flat buffers goes to torch.optim.AdamW, which knows neither key: off, they are dropped; on, the request is refused."""
    import os
    from conftest import PKG
    from ssi.config import compose
    from ssi.optimizer import setup_optimizer
    cfg = compose(os.path.join(PKG, "conf"), "sft", ["data=sft/mls-speechtokenizer-rvq_0"])
    assert cfg.optimizer.stochastic_rounding is False and cfg.optimizer.stochastic_rounding_seed is None
    model = torch.nn.Linear(4, 4)
    assert type(setup_optimizer(cfg, model)) is torch.optim.AdamW
    cfg = compose(os.path.join(PKG, "conf"), "sft", ["data=sft/mls-speechtokenizer-rvq_0", "optimizer.stochastic_rounding=true",
                                                    "optimizer.stochastic_rounding_seed=7"])
    assert cfg.optimizer.stochastic_rounding is True and cfg.optimizer.stochastic_rounding_seed == 7
    with pytest.raises(ValueError, match="stochastic_rounding"):
        setup_optimizer(cfg, model)
