#!/usr/bin/env python
"""Writes tests/golden/adamw_bits.npz: the bits that ``ops.adamw_step`` leaves in p, exp_avg and exp_avg_sq on an MI355X, with the inputs that
gave them, all as integer bit patterns (nothing depends on a generator's stability).  tests/test_adamw_bits_gpu.py replays the inputs and
compares every element: the pin that a change of the AdamW kernels' source form has not moved a contraction or a rounding.

Record it from the library of the commit BEFORE such a change (build that commit's csrc in a worktree of its own, put the .so under
variants/), on the GPU:

    SSI_HIP_LIB=$PWD/variants/libssi_parent.so python tests/golden/make_adamw_bits.py --out adamw_bits.npz

n = 2048 + 8 + 5: for bf16 one full block of 256 vectors, one more vector and a ragged tail, for fp32 two blocks and a bit (the capped-grid
stride needs 2^31 elements and is not reached).  The reference's hyper-parameters; the gradient scale 1 / 3001 as a device scalar, not a
power of two, so that every product rounds.  Per mode (``f32``, ``bf16``, ``sr``: bf16 with stochastic rounding, which starts from the bf16
inputs) three steps: 1 from zero moments, 2 from step 1's outputs, 1000 from realistic moments (as test_adamw_bf16_at_step_1000 makes them).

Keys: ``<f32|bf16>/s1/{p,g}``, ``/s2/g``, ``/s1000/{p,g,m,v}`` are the inputs, ``<mode>/s<step>/{p,m,v}_out`` the outputs."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "speech-integration_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N = 2048 + 8 + 5
HYPER = dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
GRAD_SCALE = 1.0 / 3001.0
SR_SEED, SR_ELEM_OFFSET = (1 << 40) + 12345, 2 ** 33 + 8
STEPS = (1, 2, 1000)
INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def bits(t):
    return t.detach().cpu().contiguous().view(INT[t.dtype]).numpy().copy()


def rnd(seed, scale):
    return torch.randn(N, generator=torch.Generator().manual_seed(seed)) * scale


def inputs(dtype):
    """{step: {name: CPU tensor}} without step 2's p, m, v, which are step 1's outputs."""
    gtyp = 50.0 * GRAD_SCALE
    grad = lambda seed: (rnd(seed, 50.0) + rnd(seed + 1, 25.0)).to(dtype)  # noqa: E731
    return {1: dict(p=rnd(43, 0.02).to(dtype), g=grad(40)), 2: dict(g=grad(50)),
            1000: dict(p=rnd(63, 0.02).to(dtype), g=grad(60), m=rnd(64, 0.3 * gtyp).to(dtype),
                       v=(rnd(65, gtyp).abs() + 0.05 * gtyp).square().to(dtype))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "adamw_bits.npz"))
    args = ap.parse_args()
    from ssi import _lib, ops
    dev = "cuda:0"
    gs = torch.tensor([GRAD_SCALE], dtype=torch.float32)
    out = {"n": np.int64(N), "grad_scale": bits(gs), "sr_seed": np.int64(SR_SEED), "sr_elem_offset": np.int64(SR_ELEM_OFFSET),
           **{k: np.float64(v) for k, v in HYPER.items()}}
    for mode, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16), ("sr", torch.bfloat16)):
        src = "f32" if mode == "f32" else "bf16"
        ins = inputs(dtype)
        for step, d in ins.items():
            for name, t in d.items():
                out[f"{src}/s{step}/{name}"] = bits(t)
        kw = dict(sr_seed=SR_SEED, elem_offset=SR_ELEM_OFFSET) if mode == "sr" else {}
        state = None
        for step in STEPS:
            d = ins[step]
            if step == 1:
                state = [d["p"].to(dev), torch.zeros(N, dtype=dtype, device=dev), torch.zeros(N, dtype=dtype, device=dev)]
            elif step == 1000:
                state = [d["p"].to(dev), d["m"].to(dev), d["v"].to(dev)]
            g = d["g"].to(dev)
            ops.adamw_step(state[0], g, state[1], state[2], **HYPER, step=step, grad_scale_dev=gs.to(dev), **kw)
            torch.cuda.synchronize()
            assert np.array_equal(bits(g), bits(d["g"]))
            for name, t in zip("pmv", state):
                out[f"{mode}/s{step}/{name}_out"] = bits(t)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes) from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
