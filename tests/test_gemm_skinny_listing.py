"""CPU, on the BUILT library: the skinny GEMM is there in its twelve forms — m-tiles 1, 2, 4 times (16-row workgroup of 8 waves, plain), (64-row
workgroup of 4 waves for wide N, plain), (16-row workgroup, RoPE) and (gate + up workgroup, SwiGLU) — each on the matrix instructions, without scratch (every register index is a
compile-time constant) and without LDS-DMA; its names collide with nothing the other listing tests count, and their counts are what they were.
From the report of ``tools/kernel_lint.py``; no instruction is inspected here."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "speech-integration_amd", "libssi_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin/llvm-objdump"
KERNEL = "skinny_kernel"
# the substrings the other listing tests count kernels by
COUNTED_ELSEWHERE = ("adamw_kernel", "adamw_sr_kernel", "adamw_seg", "round_bf16_sr_kernel", "ema_update_kernel", "ce_fwd_kernel", "ce_row_bf16",
                     "ce_fwd_", "ce_kl_", "seq_score_reduce_kernel", "gemm_f32_mfma_kernel", "gemm_nt4dma_kernel", "attn_", "kv_", "beam_",
                     "topk_logprob_kernel", "decode_sample_kernel", "select_pen_kernel", "sample_pen_kernel", "sumsq_", "adamw_gscale")
# template arguments <MT, NT, WAVES, EPI> as they are mangled: EPI 0 plain (16 rows x 8 waves, 64 x 4), 1 RoPE (16 x 8), 2 SwiGLU (64 x 4)
FORMS = [f"ILi{mt}ELi{nt}ELi{w}ELi{epi}E" for nt, w, epi in ((1, 8, 0), (4, 4, 0), (1, 8, 1), (4, 4, 2)) for mt in (1, 2, 4)]

pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(LLVM)), reason="needs the built library and llvm-objdump")


@pytest.fixture(scope="module")
def report():
    import kernel_lint
    return kernel_lint.lint(LIB)


def test_the_twelve_forms_are_in_the_library_on_the_matrix_cores_without_scratch(report):
    import kernel_lint
    errs, rep = report
    assert KERNEL in kernel_lint.NO_SCRATCH
    hit = [n for n in rep if KERNEL in n]
    assert len(hit) == len(FORMS) == 12, hit                                    # nothing instantiated that is never launched
    for form in FORMS:
        assert len([n for n in hit if form in n]) == 1, form
    for n in hit:
        assert rep[n]["scratch"] == 0 and not rep[n]["errors"], (n, rep[n])
        assert rep[n]["mfma"] > 0 and rep[n]["lds_dma"] == 0, (n, rep[n])
        assert not [s for s in COUNTED_ELSEWHERE if s in n], n
    assert not [s for s in COUNTED_ELSEWHERE if s in KERNEL]
    assert not [e for e in errs if KERNEL in e], errs
    # two matrix instructions per (m-tile, n-tile) pair and 64-wide chunk: the loop is not unrolled over chunks
    for n in hit:
        mt, nt = (int(n.split("skinny_kernelILi")[1][0]), int(n.split("ELi")[1][0]))
        assert rep[n]["mfma"] == 2 * mt * nt, (n, rep[n]["mfma"])


def test_the_other_kernels_are_counted_as_before(report):
    errs, rep = report
    count = lambda s: len([n for n in rep if s in n])   # noqa: E731
    assert count("gemm_nt4dma_kernel") > 0 and count("gemm_f32_mfma_kernel") > 0
    assert count("kv_decode_kernel") == 8 and count("kv_store_kernel") == 2 and count("decode_select_kernel") == 2
    assert count("sumsq_partial_kernel") == 2 and count("sumsq_final_kernel") == 1 and count("adamw_seg_kernel") == 2 and count("adamw_seg_sr_kernel") == 1
    assert count("sumsq_groups_partial_kernel") == 2 and count("adamw_gscale_kernel") == 2 and count("adamw_kernel") == 2
    assert count("ce_fwd_kernel") == 2 and count("ce_fwd_z_kernel") == 2 and count("ce_fwd_metrics_kernel") == 2 and count("ema_update_kernel") > 0
    assert not errs, errs
