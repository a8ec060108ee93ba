"""CPU, on the BUILT library: the kernels of the segmented AdamW (``ssi_adamw_step_seg``) are there — ``adamw_seg_kernel`` for fp32 and bf16,
``adamw_seg_sr_kernel`` once — and use no scratch (the segment table travels by value in the kernel arguments and is read with wave-uniform
indices only: a per-lane index into it would put its 1.5 KB into private memory, paid in the HBM traffic the kernel is bound by), no matrix
instruction and no LDS-DMA.  From the report of ``tools/kernel_lint.py``; no instruction is inspected here."""
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


def test_the_segmented_kernels_are_in_the_library_without_scratch(report):
    import kernel_lint
    errs, rep = report
    for must, count in (("adamw_seg_kernel", 2), ("adamw_seg_sr_kernel", 1)):
        assert must in kernel_lint.NO_SCRATCH
        hit = [n for n in rep if must in n]
        assert len(hit) == count, f"{must}: {hit}"
        for n in hit:
            assert rep[n]["scratch"] == 0 and not rep[n]["errors"], (n, rep[n])
            assert rep[n]["mfma"] == 0 and rep[n]["lds_dma"] == 0
    assert not [e for e in errs if "adamw_seg" in e], errs
    # the names stay clear of the substrings the plain kernels are counted by
    assert not [n for n in rep if "adamw_seg" in n and ("adamw_kernel" in n or "adamw_sr_kernel" in n)]
