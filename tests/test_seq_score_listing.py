"""CPU: the per-sequence reduce kernel in the built library, from ``kernel_lint.lint``'s report alone (no instruction is inspected here):
it is there once, it has no scratch, and the lint's no-scratch rule covers it."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_lint  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(kernel_lint.DEFAULT_LIB), reason="libssi_hip.so not built")


def test_seq_score_reduce_kernel_is_listed_once_without_scratch():
    errs, report = kernel_lint.lint()
    mine = {name: r for name, r in report.items() if "seq_score_reduce_kernel" in name}
    assert len(mine) == 1, sorted(mine)
    (name, r), = mine.items()
    assert r["scratch"] == 0 and not r["errors"], (name, r)
    assert "seq_score_reduce_kernel" in kernel_lint.NO_SCRATCH
    assert not [e for e in errs if "seq_score_reduce_kernel" in e]
    # the substrings by which the other listing tests count kernels do not match it
    assert not [s for s in ("ce_fwd_", "ce_row_bf16", "adamw_sr", "round_bf16_sr") if s in name]
