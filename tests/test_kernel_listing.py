"""The hazards of the hand-pipelined kernels, checked on the disassembly of the BUILT library (no GPU needed): ``tools/kernel_lint.py``.

Round 4 found these by reading listings (``profiles/LAB_NOTES.md``): a workgroup that ended with LDS-DMA requests still in flight towards an LDS
that already belonged to the next workgroup; accumulation-register copies that hipcc puts between inline-asm MFMAs without the wait states
they need (an element wrong by 1.2e-1, no fault); accumulators spilled to scratch by a loop that lost its unrolling.  None of them faults and
none shows in a test that happens to pass, so the listing is re-checked whenever the library is rebuilt."""
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
    errs, rep = kernel_lint.lint(LIB)
    return errs, rep


def test_the_listing_has_no_violation(report):
    errs, _ = report
    assert not errs, "\n".join(errs)


def test_the_lint_saw_the_kernels_it_is_meant_for(report):
    """Guards the guard: the pipelined kernels (plain and document-aware forms) are in the library, hold their one-basic-block main loops
    and issue LDS-DMA; the persistent GEMM forms were seen as well."""
    _, rep = report
    names = list(rep)
    for must in ("attn_bwd_dq2_kernelILi8ELb0E", "attn_bwd_dq2_kernelILi4ELb0E", "attn_bwd_dq2_kernelILi2ELb0E", "attn_bwd_dq2_kernelILi0ELb1E",
                 "attn_bwd_dkv2_kernelILb0E", "attn_bwd_dkv2_kernelILb1E", "attn_fwd_kernel", "attn_bwd_dq_kernel", "attn_bwd_dkv_kernel"):
        hit = [n for n in names if must in n]
        assert hit, f"{must} not in the library"
        for n in hit:
            assert rep[n]["mfma"] >= 32 and rep[n]["lds_dma"] > 0 and rep[n]["scratch"] == 0, (n, rep[n])
    gemms = [n for n in names if "gemm_nt4dma_kernel" in n]
    assert len(gemms) >= 15 and all(rep[n]["mfma"] == 512 and rep[n]["scratch"] == 0 for n in gemms)


def test_the_lint_catches_a_missing_drain():
    """The checker itself on a hand-made listing: an LDS-DMA request in a loop whose exit path has no vmcnt(0) is reported, the same
    listing with the wait is clean; a copy of an accumulation register inside a self-looping MFMA block is reported; the comparison of two
    builds reads the literal of a pc-relative address computation as "pc-relative" and every other literal as it stands."""
    import kernel_lint as kl
    def kernel(name, ops):
        k = kl.Kernel(name, 0)
        for n, (op, args, target) in enumerate(ops):
            k.ins.append(kl.Ins(4 * n, op, args, target))
        return k
    body = [("s_mov_b32", "m0, s4", None), ("buffer_load_dwordx4", "v1, s[8:11], s3 offen lds", None), ("s_waitcnt", "vmcnt(2)", None),
            ("s_cbranch_scc1", "65533", 0)]
    bad = kernel("k_lds", body + [("global_store_dword", "v[0:1], v2, off", None), ("s_endpgm", "", None)])
    good = kernel("k_lds", body + [("s_waitcnt", "vmcnt(0)", None), ("s_endpgm", "", None)])
    assert any(e.startswith("R3") for e in kl.lint_kernel(bad)) and not kl.lint_kernel(good)
    loop = [("v_mfma_f32_32x32x16_bf16", "a[0:15], v[0:3], v[4:7], a[0:15]", None)] * 32
    k2 = kernel("attn_bwd_dq2_kernel_x", loop + [("v_accvgpr_mov_b32", "a1, a2", None), ("s_cbranch_scc1", "0", 0), ("s_endpgm", "", None)])
    assert any(e.startswith("R2") for e in kl.lint_kernel(k2))
    k3 = kernel("attn_bwd_dq2_kernel_x", loop + [("s_cbranch_scc1", "0", 0), ("s_endpgm", "", None)])
    assert not kl.lint_kernel(k3)
    # --against: the distance from a kernel to a global moves when a neighbouring kernel changes size; any other literal is the kernel's own
    def pcrel(lit, other):
        return kernel("k_pc", [("s_getpc_b64", "s[14:15]", None), ("s_add_u32", f"s14, s14, {lit}", None), ("s_addc_u32", "s15, s15, 0", None),
                               ("s_add_u32", f"s4, s4, {other}", None), ("s_endpgm", "", None)])
    assert kl.stream(pcrel("0xb14dc", "0x40")) == kl.stream(pcrel("0xb44dc", "0x40"))
    assert kl.stream(pcrel("0xb14dc", "0x40")) != kl.stream(pcrel("0xb14dc", "0x44"))
