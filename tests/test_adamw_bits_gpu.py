"""GPU: the bits of the plain AdamW kernels are pinned.  tests/golden/adamw_bits.npz (tests/golden/make_adamw_bits.py) holds inputs and the
p / exp_avg / exp_avg_sq that ``ops.adamw_step`` left on an MI355X, as integer bit patterns, for fp32, bf16 and bf16 with stochastic rounding,
at steps 1, 2 and 1000, with a gradient scale that is no power of two: n = 2048 + 8 + 5 reaches a full block, a second one, a lone vector and
the ragged tail.  Every element of every case must come out bit for bit — the fused-AdamW tests allow 0.1 % of the elements a step aside and
the exact stochastic-rounding tests use inputs on which a contraction cannot matter, so this is what notices that the compiler contracted
or ordered the fp32 arithmetic differently.  The segmented kernels are tied to these bit for bit by tests/test_adamw_seg_gpu.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adamw_bits.npz")
MODES = {"f32": torch.float32, "bf16": torch.bfloat16, "sr": torch.bfloat16}
HYPER = ("lr", "beta1", "beta2", "eps", "weight_decay")


@pytest.fixture(scope="module")
def fx():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


def _tensor(words, dtype):
    return torch.from_numpy(words).view(dtype)


def _inputs(fx, mode, step):
    """(p, g, m, v) of the case as CPU tensors: step 1 starts from zero moments, step 2 from step 1's recorded outputs."""
    dtype, src = MODES[mode], "f32" if mode == "f32" else "bf16"
    g = _tensor(fx[f"{src}/s{step}/g"], dtype)
    if step == 1:
        return _tensor(fx[f"{src}/s1/p"], dtype), g, torch.zeros(g.numel(), dtype=dtype), torch.zeros(g.numel(), dtype=dtype)
    if step == 2:
        p, m, v = (_tensor(fx[f"{mode}/s1/{k}_out"], dtype) for k in "pmv")
        return p, g, m, v
    return tuple(_tensor(fx[f"{src}/s{step}/{k}"], dtype) for k in "pgmv")


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("mode", list(MODES))
def test_adamw_bits_are_the_recorded_ones(ops, fx, mode, step):
    dtype = MODES[mode]
    int_t = torch.int32 if dtype == torch.float32 else torch.int16
    n = int(fx["n"])
    assert n == 2048 + 8 + 5
    p0, g0, m0, v0 = _inputs(fx, mode, step)
    assert p0.numel() == g0.numel() == m0.numel() == v0.numel() == n
    p, g, m, v = (t.clone().to(DEV) for t in (p0, g0, m0, v0))
    gs = _tensor(fx["grad_scale"], torch.float32).to(DEV)
    kw = dict(sr_seed=int(fx["sr_seed"]), elem_offset=int(fx["sr_elem_offset"])) if mode == "sr" else {}
    ops.adamw_step(p, g, m, v, **{k: float(fx[k]) for k in HYPER}, step=step, grad_scale_dev=gs, **kw)
    torch.cuda.synchronize()
    assert torch.equal(g.cpu().view(int_t), g0.view(int_t)), "the gradient was written"
    for name, got in (("p", p), ("m", m), ("v", v)):
        want = torch.from_numpy(fx[f"{mode}/s{step}/{name}_out"])
        got = got.cpu().view(int_t)
        diff = int((got != want).sum())
        print(f"adamw bits {mode} step {step} {name}: {diff} of {n} elements differ")
        assert torch.equal(got, want), (mode, step, name, diff)
    assert not torch.equal(p.cpu().view(int_t), p0.view(int_t))   # (the step did something)
