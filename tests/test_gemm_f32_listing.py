"""The fp32 MFMA GEMM (``csrc/gemm_f32_mfma.hip``) on the disassembly of the BUILT library (no GPU needed): every form of the kernel is there,
uses no scratch, and its steady-state k-loop — one basic block that loops to itself — does its products on the matrix pipe
(``v_mfma_f32_32x32x2_f32`` / ``v_mfma_f32_16x16x4_f32``), none of them quietly on the vector ALU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "speech-integration_amd", "libssi_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin/llvm-objdump"

pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(LLVM)), reason="needs the built library and llvm-objdump")

KERNEL = "gemm_f32_mfma_kernel"
F32_MFMA = ("v_mfma_f32_32x32x2_f32", "v_mfma_f32_16x16x4_f32")
VALU_FMA = ("v_fma_f32", "v_fmac_f32", "v_pk_fma_f32")
# <layout, 16-byte loads>: NT, NN, TN, each with vector loads and with element loads (rows that are not 16-byte aligned)
FORMS = [f"{KERNEL}ILi{layout}ELb{vec}E" for layout in (0, 1, 2) for vec in (1, 0)]


@pytest.fixture(scope="module")
def kernels():
    import tempfile
    import kernel_lint as kl
    found = {}
    with tempfile.TemporaryDirectory() as wd:
        for co in kl.extract(LIB, wd):
            sizes = kl.scratch_sizes(co)
            for k in kl.disassemble(co):
                if KERNEL in k.name:
                    k.scratch_bytes = sizes.get(k.name, 0)
                    found[k.name] = k
    return found


@pytest.fixture(scope="module")
def report():
    import kernel_lint
    return kernel_lint.lint(LIB)


def test_the_lint_covers_the_new_kernel(report):
    import kernel_lint
    errs, rep = report
    assert KERNEL in kernel_lint.NO_SCRATCH
    assert not errs, "\n".join(errs)
    mine = [n for n in rep if KERNEL in n]
    assert len(mine) == len(FORMS) and all(rep[n]["scratch"] == 0 and rep[n]["mfma"] >= 16 and not rep[n]["errors"] for n in mine), {n: rep[n] for n in mine}


@pytest.mark.parametrize("form", FORMS)
def test_every_form_is_built_without_scratch_on_the_f32_matrix_instruction(kernels, form):
    hit = [k for n, k in kernels.items() if form in n]
    assert len(hit) == 1, f"{form}: {sorted(kernels)}"
    k = hit[0]
    assert k.scratch_bytes == 0 and not any(i.op.startswith("scratch_") for i in k.ins)
    assert any(i.op.startswith(F32_MFMA) for i in k.ins)
    other = {i.op for i in k.ins if i.op.startswith("v_mfma") and not i.op.startswith(F32_MFMA)}
    assert not other, other


@pytest.mark.parametrize("form", FORMS)
def test_the_steady_state_loop_is_on_the_matrix_pipe(kernels, form):
    import kernel_lint as kl
    k = next(k for n, k in kernels.items() if form in n)
    index = {i.addr: n for n, i in enumerate(k.ins)}
    loops = []
    for a, b in kl.blocks(k):
        last = k.ins[b]
        if last.target is None or index.get(last.target) != a:
            continue
        body = k.ins[a:b + 1]
        loops.append((sum(1 for i in body if i.op.startswith(F32_MFMA)), sum(1 for i in body if i.op.startswith(VALU_FMA))))
    assert any(m >= 8 and v == 0 for m, v in loops), f"{form}: self-looping blocks (matrix instructions, VALU fma) = {loops}"
