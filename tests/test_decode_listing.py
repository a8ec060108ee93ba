"""CPU, on the BUILT library: the two kernels of generation are there — ``kv_store_kernel`` (``ssi_kv_store``) for bf16 and fp32, and
``kv_decode_kernel`` (``ssi_attn_decode``) for bf16 and fp32 with 1, 2, 4 and 8 query-head registers, nothing else instantiated — and use
no scratch, no matrix instruction and no LDS-DMA.  From the report of ``tools/kernel_lint.py``; no instruction is inspected here."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "speech-integration_amd", "libssi_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin/llvm-objdump"

pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(LLVM)), reason="needs the built library and llvm-objdump")


@pytest.fixture(scope="module")
def report():
    import kernel_lint
    return kernel_lint.lint(LIB)


def test_the_generation_kernels_are_in_the_library_without_scratch(report):
    import kernel_lint
    errs, rep = report
    for name, count in (("kv_store_kernel", 2), ("kv_decode_kernel", 8)):
        assert name in kernel_lint.NO_SCRATCH
        hit = [n for n in rep if name in n]
        assert len(hit) == count, hit
        for n in hit:
            assert rep[n]["scratch"] == 0 and not rep[n]["errors"], (n, rep[n])
            assert rep[n]["mfma"] == 0 and rep[n]["lds_dma"] == 0
    for g in (1, 2, 4, 8):                                  # one decode form per head-register count and storage type
        assert len([n for n in rep if "kv_decode_kernel" in n and f"Li{g}E" in n]) == 2, g
    assert not [e for e in errs if "kv_" in e], errs
