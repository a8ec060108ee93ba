"""CPU: the KL cross-entropy kernels in the built library (``tools/kernel_lint.lint``, as ``tests/test_ce_listing.py``): every kernel the
launcher can launch is there exactly once — the register form for each chunk count of ``SSI_CE_DISPATCH_CHUNKS`` x ``write_grad``, the generic
form in both dtypes — none has scratch, and nothing else is instantiated."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_lint  # noqa: E402


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(kernel_lint.DEFAULT_LIB):
        pytest.fail(f"{kernel_lint.DEFAULT_LIB} is not built")
    errs, rep = kernel_lint.lint(kernel_lint.DEFAULT_LIB)
    assert not errs, errs
    return rep


def _dispatch_chunks():
    text = open(os.path.join(ROOT, "speech-integration_amd", "csrc", "embed_ce.hip")).read()
    body = text[text.index("#define SSI_CE_DISPATCH_CHUNKS"):]
    body = body[:body.index("\n\n")]
    chunks = [int(n) for n in re.findall(r"SSI_CE_CHUNKS_CASE\((\d+),", body)]
    assert chunks == sorted(set(chunks)) and 17 in chunks
    return chunks


def test_the_kl_kernels_join_the_no_scratch_list():
    assert "ce_kl_row_bf16_kernel" in kernel_lint.NO_SCRATCH and "ce_kl_generic_kernel" in kernel_lint.NO_SCRATCH


def test_every_kl_kernel_the_launcher_can_launch_is_there_once_without_scratch(report):
    kl = {name: r for name, r in report.items() if "ce_kl_" in name}
    want = [f"ce_kl_row_bf16_kernelILi{n}ELb{wg}EE" for n in _dispatch_chunks() for wg in (0, 1)]
    want += ["ce_kl_generic_kernelIfE", "ce_kl_generic_kernelIDF16bE"]
    for w in want:
        hits = [name for name in kl if w in name]
        assert len(hits) == 1, (w, hits)
    assert len(kl) == len(want), sorted(kl)
    for name, r in kl.items():
        assert r["scratch"] == 0 and not r["errors"], (name, r)
