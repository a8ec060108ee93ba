"""CPU, on the BUILT library: the two kernels of the stochastic-rounding AdamW (``ssi_adamw_step_sr``, ``ssi_round_bf16_sr``) are there exactly
once each — the nearest-rounding ``adamw_kernel`` is not a template argument or a runtime branch away from them — and neither uses scratch:
three generator calls per 16-byte vector live in registers next to the four vectors of a memory-bound kernel, and a spill would be paid in
the HBM traffic the kernel is bound by.  From the report of ``tools/kernel_lint.py``; no instruction is inspected here."""
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


def test_both_kernels_are_in_the_library_once_and_without_scratch(report):
    errs, rep = report
    for must in ("adamw_sr_kernel", "round_bf16_sr_kernel"):
        hit = [n for n in rep if must in n]
        assert len(hit) == 1, f"{must}: {hit}"
        assert rep[hit[0]]["scratch"] == 0, (hit[0], rep[hit[0]])
        assert rep[hit[0]]["mfma"] == 0 and rep[hit[0]]["lds_dma"] == 0
    assert not [e for e in errs if "_sr_kernel" in e], errs                     # (they are on the lint's no-scratch list too)
    # the nearest-rounding kernel keeps its two instantiations next to them
    assert len([n for n in rep if "adamw_kernel" in n]) == 2, [n for n in rep if "adamw" in n]
