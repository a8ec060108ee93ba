"""CPU, on the BUILT library: the kernels of FP8 weights are there once each — ``wq8_quant_kernel``, and ``wq8_gemm_kernel`` in the twelve forms of
``skinny_kernel`` (m-tiles 1, 2, 4 times: 16-row workgroup of 8 waves, plain; 64-row workgroup of 4 waves, plain; 16-row workgroup, RoPE; gate +
up workgroup, SwiGLU).  The GEMM forms run on the matrix instructions, none uses scratch (every register index is a compile-time constant) or
LDS-DMA; their names contain nothing the other listing tests count kernels by, and those counts are what they were.  From the report of
``tools/kernel_lint.py``, in the manner of tests/test_gemm_skinny_listing.py; no instruction is inspected here."""
import os
import sys

import pytest

import test_gemm_skinny_listing as sk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "speech-integration_amd", "libssi_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin/llvm-objdump"
GEMM, QUANT = "wq8_gemm_kernel", "wq8_quant_kernel"

pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(LLVM)), reason="needs the built library and llvm-objdump")


@pytest.fixture(scope="module")
def report():
    import kernel_lint
    return kernel_lint.lint(LIB)


def test_the_new_forms_are_in_the_library_once_each_on_the_matrix_cores_without_scratch(report):
    import kernel_lint
    errs, rep = report
    assert GEMM in kernel_lint.NO_SCRATCH and QUANT in kernel_lint.NO_SCRATCH
    hit = [n for n in rep if GEMM in n]
    assert len(hit) == len(sk.FORMS) == 12, hit                                 # nothing instantiated that is never launched
    for form in sk.FORMS:
        assert len([n for n in hit if form in n]) == 1, form
    quant = [n for n in rep if QUANT in n]
    assert len(quant) == 1, quant
    for n in hit + quant:
        assert rep[n]["scratch"] == 0 and not rep[n]["errors"] and rep[n]["lds_dma"] == 0, (n, rep[n])
        assert not [s for s in sk.COUNTED_ELSEWHERE + (sk.KERNEL,) if s in n], n
    for n in hit:
        assert rep[n]["mfma"] > 0, (n, rep[n])
    assert rep[quant[0]]["mfma"] == 0
    for name in (GEMM, QUANT):
        assert not [s for s in sk.COUNTED_ELSEWHERE + (sk.KERNEL, "q8_store_kernel", "q8_decode_kernel") if s in name]
    assert not [e for e in errs if "wq8_" in e], errs


def test_the_other_kernels_are_counted_as_before(report):
    errs, rep = report
    count = lambda s: len([n for n in rep if s in n])   # noqa: E731
    assert count(sk.KERNEL) == 12
    assert count("q8_store_kernel") == 2 and count("q8_decode_kernel") == 8 and count("q8_beam_kernel") == 8
    assert count("q8_split_walk_kernel") == 8 and count("q8_split_beam_kernel") == 8
    assert count("kv_decode_kernel") == 8 and count("kv_store_kernel") == 2 and count("decode_select_kernel") == 2
    assert count("sumsq_partial_kernel") == 2 and count("sumsq_final_kernel") == 1 and count("adamw_seg_kernel") == 2 and count("adamw_seg_sr_kernel") == 1
    assert count("sumsq_groups_partial_kernel") == 2 and count("adamw_gscale_kernel") == 2 and count("adamw_kernel") == 2
    assert count("ce_fwd_kernel") == 2 and count("ce_fwd_z_kernel") == 2 and count("ce_fwd_metrics_kernel") == 2 and count("ema_update_kernel") > 0
    assert count("gemm_nt4dma_kernel") > 0 and count("gemm_f32_mfma_kernel") > 0
    assert not errs, errs
