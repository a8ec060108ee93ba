"""A fresh process for ``tests/test_gemm_f32_mfma_gpu.py``: the bf16 GEMM under every ``set_impl`` value BEFORE the process has made
any fp32 call, then fp32 calls under every value, then the same bf16 calls again.  Exit code 0 = the bf16 results (and the error a forced
unsupported bf16 shape raises) are what they were before the fp32 path was touched."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "speech-integration_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main() -> int:
    from ssi import _lib, ops
    dev = "cuda"
    impls = (_lib.IMPL_AUTO, _lib.IMPL_GENERIC, _lib.IMPL_MFMA, _lib.IMPL_MFMA_WG8)
    g = torch.Generator().manual_seed(5)
    a = torch.randn(512, 192, generator=g).bfloat16().to(dev)
    b = torch.randn(768, 192, generator=g).bfloat16().to(dev)
    odd_a, odd_b = a[:70, :40].contiguous(), b[:130, :40].contiguous()   # outside the bf16 MFMA rule

    def bf16_round():
        outs, raised = [], []
        for impl in impls:
            prev = ops.set_impl(impl)
            try:
                c = torch.full((512, 768), float("nan"), dtype=torch.bfloat16, device=dev)
                ops.gemm(0, a, b, c)
                outs.append(c)
                c2 = torch.full((70, 130), float("nan"), dtype=torch.bfloat16, device=dev)
                try:
                    ops.gemm(0, odd_a, odd_b, c2)
                    raised.append(False)
                    outs.append(c2)
                except RuntimeError:
                    raised.append(True)
            finally:
                ops.set_impl(prev)
        return outs, raised

    before, raised_before = bf16_round()
    if raised_before != [False, False, True, True]:
        print("bf16 forced-unsupported behaviour before any fp32 call:", raised_before)
        return 1
    fa = torch.randn(200, 96, generator=g).to(dev)
    fb = torch.randn(256, 96, generator=g).to(dev)
    for impl in impls:
        prev = ops.set_impl(impl)
        try:
            ops.gemm(0, fa, fb, torch.empty(200, 256, device=dev))
        finally:
            ops.set_impl(prev)
    after, raised_after = bf16_round()
    torch.cuda.synchronize()
    if raised_after != raised_before or len(after) != len(before):
        print("bf16 forced-unsupported behaviour changed:", raised_before, raised_after)
        return 1
    for n, (x, y) in enumerate(zip(before, after)):
        if not torch.equal(x, y) or bool(torch.isnan(x.float()).any()):
            print(f"bf16 result {n} changed after fp32 calls")
            return 1
    print("ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
