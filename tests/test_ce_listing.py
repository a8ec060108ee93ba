"""CPU, on the BUILT library: the cross-entropy kernels of the four entries (``ssi_ce_fwd_weighted``, ``ssi_ce_fwd_z``, ``ssi_ce_fwd_smooth``,
``ssi_ce_fwd_metrics``) are there once for every form their one launcher can launch — the register-resident rows for every chunk count of
the one switch they share, the plain, the z and the smoothing form with and without the gradient, and the generic kernels in both dtypes —
none of them uses scratch (a spilled row is the one way the register-resident kernel silently loses its point: it would still be correct),
and nothing else is instantiated.
From the report of ``tools/kernel_lint.py``; no instruction is inspected here."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "speech-integration_amd", "libssi_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin/llvm-objdump"

pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(LLVM)), reason="needs the built library and llvm-objdump")

ROW_CHUNKS = (1, 2, 3, 4, 8, 16, 17, 18)   # SSI_CE_DISPATCH_CHUNKS, the switch of the four entries


@pytest.fixture(scope="module")
def report():
    import kernel_lint
    return kernel_lint.lint(LIB)


def test_every_dispatched_z_kernel_is_in_the_library_once_without_scratch(report):
    import kernel_lint
    errs, rep = report
    assert "ce_row_bf16_z_kernel" in kernel_lint.NO_SCRATCH and "ce_fwd_z_kernel" in kernel_lint.NO_SCRATCH
    wanted = [f"ce_row_bf16_z_kernelILi{n}ELb{g}EE" for n in ROW_CHUNKS for g in (0, 1)] + ["ce_fwd_z_kernelIfE", "ce_fwd_z_kernelIDF16bE"]
    for must in wanted:
        hit = [n for n in rep if must in n]
        assert len(hit) == 1, f"{must}: {hit}"
        assert rep[hit[0]]["scratch"] == 0, (hit[0], rep[hit[0]])
    assert len([n for n in rep if "ce_row_bf16_z_kernel" in n]) == 2 * len(ROW_CHUNKS)   # nothing instantiated that is never launched
    assert len([n for n in rep if "ce_fwd_z_kernel" in n]) == 2
    assert not [e for e in errs if "z_kernel" in e], errs


def test_every_dispatched_smooth_kernel_is_in_the_library_once_without_scratch(report):
    import kernel_lint
    errs, rep = report
    assert "ce_row_bf16_smooth_kernel" in kernel_lint.NO_SCRATCH and "ce_fwd_smooth_kernel" in kernel_lint.NO_SCRATCH
    wanted = ([f"ce_row_bf16_smooth_kernelILi{n}ELb{g}EE" for n in ROW_CHUNKS for g in (0, 1)]
              + ["ce_fwd_smooth_kernelIfE", "ce_fwd_smooth_kernelIDF16bE"])
    for must in wanted:
        hit = [n for n in rep if must in n]
        assert len(hit) == 1, f"{must}: {hit}"
        assert rep[hit[0]]["scratch"] == 0, (hit[0], rep[hit[0]])
    assert len([n for n in rep if "ce_row_bf16_smooth_kernel" in n]) == 2 * len(ROW_CHUNKS)   # nothing instantiated that is never launched
    assert len([n for n in rep if "ce_fwd_smooth_kernel" in n]) == 2
    assert not [e for e in errs if "smooth_kernel" in e], errs


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


def test_the_plain_and_the_metrics_kernels_are_the_ones_of_before(report):
    """The z and the metrics forms are kernels of their own: the counts of the plain kernels are what they were without them, and none of
    the cross-entropy kernels has scratch."""
    _, rep = report
    assert len([n for n in rep if "ce_row_bf16_kernel" in n]) == 2 * len(ROW_CHUNKS)
    assert len([n for n in rep if "ce_row_bf16_metrics_kernel" in n]) == len(ROW_CHUNKS)
    assert len([n for n in rep if "ce_fwd_kernel" in n]) == 2 and len([n for n in rep if "ce_fwd_metrics_kernel" in n]) == 2
    assert all(rep[n]["scratch"] == 0 for n in rep if "ce_row_bf16" in n or "ce_fwd_" in n)


def test_the_kernels_of_the_other_entries_are_the_ones_of_before(report):
    """The smoothing forms are kernels of their own: the counts of the plain, z and metrics kernels are what they were without them."""
    _, rep = report
    assert len([n for n in rep if "ce_row_bf16_kernel" in n]) == 2 * len(ROW_CHUNKS)
    assert len([n for n in rep if "ce_row_bf16_z_kernel" in n]) == 2 * len(ROW_CHUNKS)
    assert len([n for n in rep if "ce_row_bf16_metrics_kernel" in n]) == len(ROW_CHUNKS)
    assert len([n for n in rep if "ce_fwd_kernel" in n]) == 2 and len([n for n in rep if "ce_fwd_z_kernel" in n]) == 2
    assert len([n for n in rep if "ce_fwd_metrics_kernel" in n]) == 2
    assert all(rep[n]["scratch"] == 0 for n in rep if "ce_row_bf16" in n or "ce_fwd_" in n)
