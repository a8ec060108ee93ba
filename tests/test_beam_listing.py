"""CPU, on the BUILT library: the two kernels of beam search are there — ``beam_decode_kernel`` (``ssi_attn_decode_beam``) in the 8 forms of
``kv_decode_kernel`` (bf16 and fp32 x 1, 2, 4, 8 query-head registers) and ``topk_logprob_kernel`` (``ssi_topk_logprob``) for bf16 and fp32 with
lists of 1, 2, 4 and 8 candidates — and use no scratch, no matrix instruction and no LDS-DMA.  From the report of ``tools/kernel_lint.py``; no
instruction is inspected here."""
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


def test_the_beam_kernels_are_in_the_library_without_scratch(report):
    import kernel_lint
    errs, rep = report
    for name in ("beam_decode_kernel", "topk_logprob_kernel"):
        assert name in kernel_lint.NO_SCRATCH
        hit = [n for n in rep if name in n]
        assert len(hit) == 8, hit
        for n in hit:
            assert rep[n]["scratch"] == 0 and not rep[n]["errors"], (n, rep[n])
            assert rep[n]["mfma"] == 0 and rep[n]["lds_dma"] == 0
        for g in (1, 2, 4, 8):                              # one form per register count and storage type
            assert len([n for n in hit if f"Li{g}E" in n]) == 2, (name, g)
    assert not [e for e in errs if "beam_decode" in e or "topk_logprob" in e], errs
    assert errs == []                                       # the lint reports nothing for the whole library


def test_the_new_names_leave_the_other_counts_alone(report):
    _, rep = report
    assert len([n for n in rep if "kv_decode_kernel" in n]) == 8 and len([n for n in rep if "kv_store_kernel" in n]) == 2
    assert len([n for n in rep if "decode_select_kernel" in n]) == 2
