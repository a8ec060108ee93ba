"""The penalised selection kernels in the disassembly of the BUILT library (no GPU needed), through ``tools/kernel_lint.lint``'s report only:
two forms of each (fp32 and bf16 logits) beside the two of each plain kernel, both on the no-scratch list and without scratch, and nothing
in them that the walks do not need — no matrix instruction, no LDS-DMA."""
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


@pytest.mark.parametrize("name", ("select_pen_kernel", "sample_pen_kernel"))
def test_two_forms_without_scratch(report, name):
    import kernel_lint
    errs, rep = report
    assert name in kernel_lint.NO_SCRATCH
    forms = [n for n in rep if name in n]
    assert len(forms) == 2 and any("IfE" in n for n in forms) and any("IDF16bE" in n for n in forms), forms
    for n in forms:
        assert rep[n]["scratch"] == 0 and rep[n]["mfma"] == 0 and rep[n]["lds_dma"] == 0 and not rep[n]["errors"], (n, rep[n])
    assert not [e for e in errs if name in e]


def test_the_plain_kernels_keep_their_names_and_count(report):
    _, rep = report
    for plain in ("decode_select_kernel", "decode_sample_kernel"):
        assert len([n for n in rep if plain in n]) == 2
    assert not [n for n in rep if "pen_kernel" in n and ("decode_select_kernel" in n or "decode_sample_kernel" in n)]
