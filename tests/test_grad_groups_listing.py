"""CPU, on the BUILT library: the kernels of the gradient groups are there — ``sumsq_groups_partial_kernel`` for bf16 and fp32, one
``sumsq_groups_final_kernel``, ``adamw_gscale_kernel`` for bf16 and fp32 and ``adamw_gscale_sr_kernel`` — and are plain streaming passes: no
scratch (the tables are indexed wave-uniformly, never per lane), no matrix instruction, no LDS-DMA.  From the report of
``tools/kernel_lint.py``; no instruction is inspected here."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "speech-integration_amd", "libssi_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin/llvm-objdump"
# the substrings the other listing tests count kernels by
COUNTED_ELSEWHERE = ("adamw_kernel", "adamw_sr_kernel", "adamw_seg", "round_bf16_sr_kernel", "ema_update_kernel", "ce_fwd_kernel", "ce_row_bf16",
                     "ce_fwd_", "ce_kl_", "seq_score_reduce_kernel", "gemm_f32_mfma_kernel", "gemm_nt4dma_kernel", "attn_", "kv_", "beam_",
                     "topk_logprob_kernel", "decode_sample_kernel", "select_pen_kernel", "sample_pen_kernel")
EXPECTED = {"sumsq_groups_partial_kernel": 2, "sumsq_groups_final_kernel": 1, "adamw_gscale_kernel": 2, "adamw_gscale_sr_kernel": 1}

pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(LLVM)), reason="needs the built library and llvm-objdump")


@pytest.fixture(scope="module")
def report():
    import kernel_lint
    return kernel_lint.lint(LIB)


@pytest.mark.parametrize("kernel,count", sorted(EXPECTED.items()))
def test_the_kernels_are_in_the_library_without_scratch(report, kernel, count):
    import kernel_lint
    errs, rep = report
    assert kernel in kernel_lint.NO_SCRATCH
    hit = [n for n in rep if kernel in n]
    assert len(hit) == count, hit
    for n in hit:
        assert rep[n]["scratch"] == 0 and not rep[n]["errors"], (n, rep[n])
        assert rep[n]["mfma"] == 0 and rep[n]["lds_dma"] == 0
        assert not [s for s in COUNTED_ELSEWHERE if s in n], n
    assert not [s for s in COUNTED_ELSEWHERE if s in kernel]
    assert not [e for e in errs if kernel in e], errs


def test_the_plain_sum_and_the_segmented_adamw_are_counted_as_before(report):
    _, rep = report
    assert len([n for n in rep if "sumsq_partial_kernel" in n]) == 2 and len([n for n in rep if "sumsq_final_kernel" in n]) == 1
    assert len([n for n in rep if "adamw_seg_kernel" in n]) == 2 and len([n for n in rep if "adamw_seg_sr_kernel" in n]) == 1
    assert not report[0], report[0]
