"""CPU, on the BUILT library: the unit-BPE kernels are there (the trainer's nine and the encoder in its two forms), without scratch (every
register array is indexed at compile time only), without matrix instructions or LDS-DMA, and under names that none of the older listing tests
counts.  From the report of ``tools/kernel_lint.py``; no instruction is inspected here."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "speech-integration_amd", "libssi_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin/llvm-objdump"
KERNELS = {"bpe_pair_count_kernel": 1, "bpe_sanitise_kernel": 1, "bpe_state_init_kernel": 1, "bpe_best_partial_kernel": 1,
           "bpe_best_final_kernel": 1, "bpe_mark_kernel": 1, "bpe_scan_kernel": 1, "bpe_apply_kernel": 1, "bpe_encode_kernel": 2}
ENCODE_FORMS = ("ILi4E", "ILi16E")   # template argument <ITEMS> as it is mangled
COUNTED_ELSEWHERE = ("adamw_kernel", "adamw_sr_kernel", "adamw_seg", "round_bf16_sr_kernel", "ema_update_kernel", "ce_fwd_kernel", "ce_row_bf16",
                     "ce_fwd_", "ce_kl_", "seq_score_reduce_kernel", "gemm_f32_mfma_kernel", "gemm_nt4dma_kernel", "attn_", "kv_", "beam_",
                     "topk_logprob_kernel", "decode_sample_kernel", "select_pen_kernel", "sample_pen_kernel", "sumsq_", "adamw_gscale",
                     "skinny_kernel", "wq8_", "edit_distance_kernel")

pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(LLVM)), reason="needs the built library and llvm-objdump")


@pytest.fixture(scope="module")
def report():
    import kernel_lint
    return kernel_lint.lint(LIB)


def test_the_bpe_kernels_are_in_the_library_without_scratch(report):
    import kernel_lint
    errs, rep = report
    hit = [n for n in rep if "bpe_" in n]
    assert len(hit) == sum(KERNELS.values()), hit
    for kernel, forms in KERNELS.items():
        assert kernel in kernel_lint.NO_SCRATCH
        assert len([n for n in hit if kernel in n]) == forms, kernel
    for form in ENCODE_FORMS:
        assert len([n for n in hit if "bpe_encode_kernel" + form in n]) == 1, form
    for n in hit:
        assert rep[n]["scratch"] == 0 and not rep[n]["errors"], (n, rep[n])
        assert rep[n]["mfma"] == 0 and rep[n]["lds_dma"] == 0, (n, rep[n])
        assert not [s for s in COUNTED_ELSEWHERE if s in n], n
    assert not [e for e in errs if "bpe_" in e], errs


def test_the_other_kernels_are_counted_as_before(report):
    errs, rep = report
    count = lambda s: len([n for n in rep if s in n])   # noqa: E731
    assert count("gemm_nt4dma_kernel") > 0 and count("gemm_f32_mfma_kernel") > 0 and count("skinny_kernel") == 12
    assert count("kv_decode_kernel") == 8 and count("kv_store_kernel") == 2 and count("decode_select_kernel") == 2
    assert count("seq_score_reduce_kernel") == 1 and count("edit_distance_kernel") == 2 and count("adamw_kernel") == 2
    assert not errs, errs
