"""CPU, on the BUILT library: the label-rank cross-entropy kernels (``ssi_ce_fwd_metrics``) are there for every chunk count the dispatch can ask
for and for both dtypes of the generic form, and none of them uses scratch — a spilled row is the one way the register-resident kernel
silently loses its point (it would still be correct).  From the report of ``tools/kernel_lint.py``; no instruction is inspected here."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "speech-integration_amd", "libssi_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin/llvm-objdump"

pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(LLVM)), reason="needs the built library and llvm-objdump")

ROW_CHUNKS = (1, 2, 3, 4, 8, 16, 17, 18)   # the switch of ssi_ce_fwd_metrics (and of ssi_ce_fwd_weighted)


@pytest.fixture(scope="module")
def report():
    import kernel_lint
    return kernel_lint.lint(LIB)


def test_every_dispatched_metrics_kernel_is_in_the_library_without_scratch(report):
    errs, rep = report
    wanted = [f"ce_row_bf16_metrics_kernelILi{n}EE" for n in ROW_CHUNKS] + ["ce_fwd_metrics_kernelIfE", "ce_fwd_metrics_kernelIDF16bE",
                                                                           "ce_metrics_reduce_kernel"]
    for must in wanted:
        hit = [n for n in rep if must in n]
        assert len(hit) == 1, f"{must}: {hit}"
        assert rep[hit[0]]["scratch"] == 0, (hit[0], rep[hit[0]])
    assert len([n for n in rep if "ce_row_bf16_metrics_kernel" in n]) == len(ROW_CHUNKS)   # nothing instantiated that is never launched
    assert not [e for e in errs if "metrics_kernel" in e], errs                              # (they are on the lint's no-scratch list too)

