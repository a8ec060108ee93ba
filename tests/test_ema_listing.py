"""CPU, on the BUILT library: the kernel of the parameter average (``ssi_ema_update``) is there — ``ema_update_kernel`` for bf16 and for fp32
parameters — and is a plain streaming pass: no scratch, no matrix instruction, no LDS-DMA.  From the report of ``tools/kernel_lint.py``; no
instruction is inspected here."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "speech-integration_amd", "libssi_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin/llvm-objdump"
# the substrings the other listing tests count kernels by
COUNTED_ELSEWHERE = ("adamw_kernel", "adamw_sr_kernel", "adamw_seg", "round_bf16_sr_kernel", "ce_fwd_kernel", "ce_row_bf16", "ce_fwd_", "ce_kl_",
                     "seq_score_reduce_kernel", "gemm_f32_mfma_kernel", "gemm_nt4dma_kernel", "attn_")

pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(LLVM)), reason="needs the built library and llvm-objdump")


@pytest.fixture(scope="module")
def report():
    import kernel_lint
    return kernel_lint.lint(LIB)


def test_the_average_kernel_is_in_the_library_twice_without_scratch(report):
    import kernel_lint
    errs, rep = report
    assert "ema_update_kernel" in kernel_lint.NO_SCRATCH
    hit = [n for n in rep if "ema_update_kernel" in n]
    assert len(hit) == 2, hit                                                            # bf16 and fp32 parameters
    for n in hit:
        assert rep[n]["scratch"] == 0 and not rep[n]["errors"], (n, rep[n])
        assert rep[n]["mfma"] == 0 and rep[n]["lds_dma"] == 0
        assert not [s for s in COUNTED_ELSEWHERE if s in n], n
    assert not [e for e in errs if "ema_update" in e], errs
    assert not [s for s in COUNTED_ELSEWHERE if s in "ema_update_kernel"]
    assert not errs, errs
