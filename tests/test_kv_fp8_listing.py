"""CPU, on the BUILT library: the kernels of the FP8 K/V cache are there once each — ``q8_store_kernel`` for bf16 and fp32, ``q8_decode_kernel``,
``q8_beam_kernel``, ``q8_split_walk_kernel`` and ``q8_split_beam_kernel`` for bf16 and fp32 with 1, 2, 4 and 8 query-head registers — and use no
scratch, no matrix instruction and no LDS-DMA; the split forms bring no merge kernel of their own.  Their names do not contain those of the plain
kernels, which the other listing tests count by substring, and those counts are unchanged.  From the report of ``tools/kernel_lint.py``, in the
manner of tests/test_split_kv_listing.py; no instruction is inspected here."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "speech-integration_amd", "libssi_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin/llvm-objdump"

pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(LLVM)), reason="needs the built library and llvm-objdump")
NEW = (("q8_store_kernel", 2), ("q8_decode_kernel", 8), ("q8_beam_kernel", 8), ("q8_split_walk_kernel", 8), ("q8_split_beam_kernel", 8))
OLD = (("kv_store_kernel", 2), ("kv_decode_kernel", 8), ("beam_decode_kernel", 8), ("split_kv_walk_kernel", 8), ("split_beam_walk_kernel", 8),
       ("split_kv_merge_kernel", 2))


@pytest.fixture(scope="module")
def report():
    import kernel_lint
    return kernel_lint.lint(LIB)


def test_the_fp8_kernels_are_in_the_library_once_each_without_scratch(report):
    import kernel_lint
    errs, rep = report
    for name, count in NEW:
        assert name in kernel_lint.NO_SCRATCH
        hit = [n for n in rep if name in n]
        assert len(hit) == count, hit
        for n in hit:
            assert rep[n]["scratch"] == 0 and not rep[n]["errors"], (n, rep[n])
            assert rep[n]["mfma"] == 0 and rep[n]["lds_dma"] == 0
        if count == 8:
            for g in (1, 2, 4, 8):                                          # one form per head-register count and storage type
                assert len([n for n in hit if f"Li{g}E" in n]) == 2, (name, g)
    assert not [e for e in errs if "q8_" in e], errs


def test_the_plain_kernels_are_still_counted_alone(report):
    _, rep = report
    for old, count in OLD:
        assert len([n for n in rep if old in n]) == count, old
    for name, _ in NEW:
        assert not any(old in name for old, _ in OLD + (("decode_select_kernel", 0),))
