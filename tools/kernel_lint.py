#!/usr/bin/env python3
"""Listing lint of the built library (no GPU needed): the hazards of the hand-pipelined kernels that only a look at the
disassembly used to verify (profiles/LAB_NOTES.md, round 4), checked mechanically on the gfx950 code objects inside
``libssi_hip.so``.

Rules
  R1  no scratch: kernels named in ``NO_SCRATCH`` have private_segment_fixed_size == 0 and no ``scratch_*`` instruction;
  R2  main loops keep their registers: a basic block that loops to itself and holds >= ``MAIN_LOOP_MFMAS`` matrix instructions
      (the one-basic-block trips of the pipelined kernels) contains no ``v_accvgpr_mov / _write / _read`` — hipcc's copies of
      accumulation registers between inline-asm MFMAs get no wait states (a dQ element wrong by 1.2e-1, no fault);
  R3  nothing in flight towards LDS at the end: in every kernel that issues LDS-DMA (``buffer_load ... lds``,
      ``global_load_lds_*``) every path from such an instruction to ``s_endpgm`` passes ``s_waitcnt vmcnt(0)`` — the LDS belongs
      to the next workgroup of the CU by then (the round-4 race of attn_bwd_dq2_kernel).

``python tools/kernel_lint.py [lib]`` prints one line per kernel and exits 1 on a violation; ``tests/test_kernel_listing.py``
runs the same checks in the CPU suite.

``python tools/kernel_lint.py [lib] --against OTHER_LIB`` compares the two libraries' gfx950 kernels instead (has a change MOVED device
code or CHANGED it?): the same kernel names on both sides, per kernel the same instruction stream (mnemonic and operands; branch targets as
offsets within the kernel, the literals of pc-relative address computations as "pc-relative") and the same VGPR / AGPR / SGPR counts, LDS bytes and private segment size in the code-object notes.  Exits 1 on
any difference.  Which translation unit a kernel sits in is not compared.  For a kernel whose streams differ it also says where they part against
the kernel's K loops (the loops that hold matrix instructions): the loops' code equal and every difference behind the last of them — an epilogue
moved — or a loop itself or the code ahead of it changed."""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile
from dataclasses import dataclass, field

LLVM = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "speech-integration_amd", "libssi_hip.so")
NO_SCRATCH = ("attn_bwd_dq2_kernel", "attn_bwd_dkv2_kernel", "attn_fwd_kernel", "gemm_nt4dma_kernel", "gemm_f32_mfma_kernel",
              "ce_row_bf16_metrics_kernel", "ce_fwd_metrics_kernel", "ce_row_bf16_z_kernel", "ce_fwd_z_kernel", "ce_row_bf16_smooth_kernel", "ce_fwd_smooth_kernel", "ce_kl_row_bf16_kernel", "ce_kl_generic_kernel", "adamw_sr_kernel", "round_bf16_sr_kernel", "seq_score_reduce_kernel", "edit_distance_kernel",
              "adamw_seg_kernel", "adamw_seg_sr_kernel", "ema_update_kernel", "kv_store_kernel", "kv_decode_kernel", "beam_decode_kernel", "q8_store_kernel", "q8_decode_kernel", "q8_beam_kernel", "q8_split_walk_kernel", "q8_split_beam_kernel","topk_logprob_kernel", "decode_sample_kernel", "select_pen_kernel", "sample_pen_kernel", "sample_rows_kernel", "sample_rows_pen_kernel",
              "sumsq_groups_partial_kernel", "sumsq_groups_final_kernel", "adamw_gscale_kernel", "adamw_gscale_sr_kernel", "skinny_kernel", "wq8_gemm_kernel", "wq8_quant_kernel",
              "split_kv_walk_kernel", "split_beam_walk_kernel", "split_kv_merge_kernel",
              "bpe_pair_count_kernel", "bpe_sanitise_kernel", "bpe_state_init_kernel", "bpe_best_partial_kernel", "bpe_best_final_kernel", "bpe_mark_kernel", "bpe_scan_kernel", "bpe_apply_kernel", "bpe_encode_kernel")
PINNED_LOOPS = ("attn_bwd_dq2_kernel", "attn_bwd_dkv2_kernel")   # kernels whose main loops are inline-asm MFMAs on pinned register classes
MAIN_LOOP_MFMAS = 32

_INS = re.compile(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):")
_SYM = re.compile(r"^([0-9a-f]+) <(\S+)>:")
_TGT = re.compile(r"<(\S+?)\+0x([0-9a-f]+)>\s*$")
_TGT0 = re.compile(r"<(\S+?)>\s*$")


@dataclass
class Ins:
    addr: int
    op: str
    args: str
    target: int | None = None


@dataclass
class Kernel:
    name: str
    addr: int
    ins: list[Ins] = field(default_factory=list)
    scratch_bytes: int = 0
    notes: dict = field(default_factory=dict)


def extract(lib: str, workdir: str) -> list[str]:
    """Code objects of the fat binary: llvm-objdump --offloading writes one file per translation unit next to its input."""
    link = os.path.join(workdir, "lib.so")
    os.symlink(os.path.abspath(lib), link)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", link], check=True, cwd=workdir, stdout=subprocess.DEVNULL)
    return sorted(os.path.join(workdir, f) for f in os.listdir(workdir) if f.endswith("gfx950"))


NOTE_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def kernel_notes(co: str) -> dict[str, dict[str, int]]:
    """NOTE_KEYS of every kernel of a code object, by kernel name."""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, {}
    for line in notes.splitlines() + ["  - ."]:   # a kernel's entry: a list item at indent 2, its own keys at indent 4 (arguments lie deeper)
        m = re.match(r"  [- ] \.(\w+):\s+(\S+)", line)
        if line.startswith("  - ."):
            if "name" in cur:
                out[cur["name"]] = {k: int(cur.get(k, 0)) for k in NOTE_KEYS}
            cur = {}
        if m:
            cur[m.group(1)] = m.group(2)
    return out


def scratch_sizes(co: str) -> dict[str, int]:
    return {name: n["private_segment_fixed_size"] for name, n in kernel_notes(co).items()}


def disassemble(co: str) -> list[Kernel]:
    text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout
    syms, kernels, cur = {}, [], None
    lines = text.splitlines()
    for line in lines:
        m = _SYM.match(line)
        if m:
            syms[m.group(2)] = int(m.group(1), 16)
    for line in lines:
        m = _SYM.match(line)
        if m:
            cur = Kernel(m.group(2), int(m.group(1), 16))
            kernels.append(cur)
            continue
        m = _INS.match(line)
        if not m or cur is None:
            continue
        ins = Ins(int(m.group(3), 16), m.group(1), m.group(2))
        if ins.op.startswith(("s_cbranch", "s_branch")):
            t = _TGT.search(line)
            if t:
                ins.target = syms[t.group(1)] + int(t.group(2), 16)
            else:
                t0 = _TGT0.search(line)
                if t0 and t0.group(1) in syms:
                    ins.target = syms[t0.group(1)]
        cur.ins.append(ins)
    return [k for k in kernels if k.ins]


def blocks(k: Kernel) -> list[tuple[int, int]]:
    """Basic blocks as [first, last] instruction indices."""
    leaders = {0}
    index = {i.addr: n for n, i in enumerate(k.ins)}
    for n, i in enumerate(k.ins):
        if i.op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc")):
            if n + 1 < len(k.ins):
                leaders.add(n + 1)
            if i.target is not None and i.target in index:
                leaders.add(index[i.target])
    ls = sorted(leaders)
    return [(a, (ls[j + 1] - 1) if j + 1 < len(ls) else len(k.ins) - 1) for j, a in enumerate(ls)]


def is_lds_dma(i: Ins) -> bool:
    return i.op.startswith("global_load_lds") or (i.op.startswith("buffer_load") and re.search(r"\blds\b", i.args) is not None)


def drains_vm(i: Ins) -> bool:
    if i.op != "s_waitcnt":
        return False
    if re.search(r"vmcnt\(0\)", i.args):
        return True
    return re.fullmatch(r"(0x)?0+", i.args.strip()) is not None   # raw immediate 0: every counter


def lint_kernel(k: Kernel) -> list[str]:
    errs = []
    short = re.sub(r"^_ZN12_GLOBAL__N_1\d+|^_Z\d+", "", k.name)
    if any(s in k.name for s in NO_SCRATCH):
        if k.scratch_bytes:
            errs.append(f"R1 {short}: {k.scratch_bytes} bytes of scratch")
        n = sum(1 for i in k.ins if i.op.startswith("scratch_"))
        if n:
            errs.append(f"R1 {short}: {n} scratch instructions")
    bl = blocks(k)
    index = {i.addr: n for n, i in enumerate(k.ins)}
    if any(s in k.name for s in PINNED_LOOPS):
        loops = 0
        for a, b in bl:
            last = k.ins[b]
            if last.target is None or index.get(last.target) != a:
                continue
            body = k.ins[a:b + 1]
            if sum(1 for i in body if i.op.startswith("v_mfma")) < MAIN_LOOP_MFMAS:
                continue
            loops += 1
            bad = [i for i in body if i.op.startswith(("v_accvgpr_mov", "v_accvgpr_write", "v_accvgpr_read"))]
            if bad:
                errs.append(f"R2 {short}: {len(bad)} accumulation-register copies inside the main loop at {k.ins[a].addr:#x}")
        if loops == 0:
            errs.append(f"R2 {short}: no one-basic-block main loop found (a trip was split: check the listing)")
    if any(is_lds_dma(i) for i in k.ins):
        # forward may-analysis over the CFG: dirty = an LDS-DMA request may be in flight
        succ: dict[int, list[int]] = {}
        start_of = {a: n for n, (a, _) in enumerate(bl)}
        for n, (a, b) in enumerate(bl):
            last, s = k.ins[b], []
            if last.op.startswith("s_endpgm"):
                pass
            elif last.op.startswith("s_branch"):
                if last.target in index:
                    s.append(start_of[index[last.target]])
            else:
                if last.op.startswith("s_cbranch") and last.target in index:
                    s.append(start_of[index[last.target]])
                if n + 1 < len(bl):
                    s.append(n + 1)
            succ[n] = s
        def transfer(n: int, dirty: bool, report: bool = False) -> bool:
            a, b = bl[n]
            for i in k.ins[a:b + 1]:
                if is_lds_dma(i):
                    dirty = True
                elif drains_vm(i):
                    dirty = False
                elif report and dirty and i.op.startswith("s_endpgm"):
                    errs.append(f"R3 {short}: s_endpgm at {i.addr:#x} reachable with LDS-DMA requests in flight (no s_waitcnt vmcnt(0) on the path)")
            return dirty

        dirty_in = [False] * len(bl)
        work = list(range(len(bl)))
        while work:  # to the fixed point: a block is dirty on entry if any predecessor may leave it dirty
            n = work.pop()
            if transfer(n, dirty_in[n]):
                for s_ in succ[n]:
                    if not dirty_in[s_]:
                        dirty_in[s_] = True
                        work.append(s_)
        for n in range(len(bl)):
            transfer(n, dirty_in[n], report=True)
    return errs


def kernels_of(co: str) -> list[Kernel]:
    notes = kernel_notes(co)
    ks = [k for k in disassemble(co) if k.name in notes]   # (symbols without a kernel descriptor are not kernels)
    for k in ks:
        k.notes = notes[k.name]
        k.scratch_bytes = k.notes["private_segment_fixed_size"]
    return ks


def stream(k: Kernel) -> list[tuple]:
    """A kernel's instructions as compared by --against: (mnemonic, operands, branch target as an offset within the kernel).  The literal of
    a pc-relative address computation (s_getpc_b64 s[n:n+1], then s_add_u32 sn, sn, LIT and s_addc_u32 sn+1, sn+1, LIT within the next
    four instructions: the distance to a global such as g_nt4_sched) reads "pc-relative": it moves when a NEIGHBOURING kernel changes size."""
    ins = list(k.ins)
    while ins and ins[-1].op == "s_nop":  # fill between the last s_endpgm and the next symbol or the end of the section: not the kernel's code
        ins.pop()
    out, pc, since = [], None, 0
    for i in ins:
        args = i.args
        if i.op == "s_getpc_b64":
            m = re.fullmatch(r"s\[(\d+):(\d+)\]", args.strip())
            pc, since = ((f"s{m.group(1)}", f"s{m.group(2)}") if m else None), 0
        elif pc:
            since += 1
            if i.op == "s_add_u32" and args.startswith(f"{pc[0]}, {pc[0]}, "):
                args = f"{pc[0]}, {pc[0]}, pc-relative"
            elif i.op == "s_addc_u32" and args.startswith(f"{pc[1]}, {pc[1]}, "):
                args, pc = f"{pc[1]}, {pc[1]}, pc-relative", None
            if since >= 4:
                pc = None
        out.append((i.op, args, None if i.target is None else i.target - k.addr))
    return out


def k_loops(k: Kernel) -> list[tuple[int, int]]:
    """Loops that hold matrix instructions, as [first, last] instruction indices: from the target of a backward branch to the last branch back to
    it.  R2's main loops (one basic block that loops to itself) are the simplest case; a loop whose body branches (the skinny GEMMs load rows
    under exec masks) spans several blocks."""
    index = {i.addr: n for n, i in enumerate(k.ins)}
    last: dict[int, int] = {}
    for n, i in enumerate(k.ins):
        a = index.get(i.target) if i.target is not None else None
        if a is not None and a <= n:
            last[a] = n
    return [(a, b) for a, b in sorted(last.items()) if any(i.op.startswith("v_mfma") for i in k.ins[a:b + 1])]


def where_against_k_loop(ka: Kernel, kb: Kernel, first: int) -> str:
    """Where two differing streams part, told against the kernels' K loops: a change behind the last loop (an epilogue) leaves the loops alone."""
    la, lb = k_loops(ka), k_loops(kb)
    if not la or not lb:
        return "no loop with matrix instructions on one side"
    sa, sb = stream(ka), stream(kb)
    if [sa[a:b + 1] for a, b in la] != [sb[a:b + 1] for a, b in lb]:
        return "K LOOP DIFFERS"
    end = max(la[-1][1], lb[-1][1])
    return f"K loops equal, every difference after them (the last ends at instruction {end})" if first > end else "DIFFERENCE AHEAD OF THE K LOOP"


def compare(lib: str, other: str) -> tuple[list[str], int]:
    """Differences between the gfx950 kernels of two libraries, and how many kernels `lib` has."""
    def load(path: str) -> dict[str, Kernel]:
        with tempfile.TemporaryDirectory() as wd:
            return {k.name: k for co in extract(path, wd) for k in kernels_of(co)}

    a, b = load(lib), load(other)
    diffs = [f"{n}: only in {lib}" for n in sorted(set(a) - set(b))] + [f"{n}: only in {other}" for n in sorted(set(b) - set(a))]
    if len(a) != len(b):
        diffs.append(f"kernel count {len(a)} against {len(b)}")
    for n in sorted(set(a) & set(b)):
        if a[n].notes != b[n].notes:
            diffs.append(f"{n}: notes {a[n].notes} against {b[n].notes}")
        sa, sb = stream(a[n]), stream(b[n])
        if sa != sb:
            first = next((j for j, (x, y) in enumerate(zip(sa, sb)) if x != y), min(len(sa), len(sb)))
            diffs.append(f"{n}: {len(sa)} against {len(sb)} instructions, first difference at instruction {first}: "
                         f"{sa[first] if first < len(sa) else None} against {sb[first] if first < len(sb) else None}; "
                         f"{where_against_k_loop(a[n], b[n], first)}")
    return diffs, len(a)


def lint(lib: str = DEFAULT_LIB) -> tuple[list[str], dict[str, dict]]:
    errs, report = [], {}
    with tempfile.TemporaryDirectory() as wd:
        for co in extract(lib, wd):
            for k in kernels_of(co):
                e = lint_kernel(k)
                errs += e
                report[k.name] = {"instructions": len(k.ins), "scratch": k.scratch_bytes, "mfma": sum(1 for i in k.ins if i.op.startswith("v_mfma")),
                                  "lds_dma": sum(1 for i in k.ins if is_lds_dma(i)), "errors": e}
    return errs, report


if __name__ == "__main__":
    argv = sys.argv[1:]
    against = None
    if "--against" in argv:
        j = argv.index("--against")
        against = argv[j + 1]
        del argv[j:j + 2]
    lib = argv[0] if argv else DEFAULT_LIB
    if against:
        diffs, n = compare(lib, against)
        for d in diffs:
            print("DIFFERENT", d)
        print(f"{n} gfx950 kernels in {lib}: {'no difference' if not diffs else str(len(diffs)) + ' differences'} against {against}")
        sys.exit(1 if diffs else 0)
    errs, report = lint(lib)
    for name, r in sorted(report.items()):
        if r["mfma"] or r["lds_dma"] or r["scratch"]:
            print(f"{'FAIL' if r['errors'] else 'ok  '} {name[:110]:110s} ins {r['instructions']:6d} mfma {r['mfma']:4d} lds-dma {r['lds_dma']:3d} scratch {r['scratch']}")
    for e in errs:
        print("VIOLATION", e)
    sys.exit(1 if errs else 0)
