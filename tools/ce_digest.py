"""Bits of the cross-entropy kernels, for comparing two builds of the library: one SHA-256 per case over every output buffer of ``ce_fwd``
(``write_grad`` 0 and 1, with and without row weights), ``ce_fwd_z`` (z = 0, 1e-4, 0.5), ``ce_fwd_smooth`` (e = 0, 0.1 at each of these z, and
once without a ``row_z`` at z = 0), ``ce_fwd_metrics``, ``ce_reduce``, ``ce_metrics_reduce`` and ``seq_score_reduce``: all four entries.  Inputs come from the CPU with fixed seeds, so two runs that print the same digests computed
the same bits:  tools/lib_ab.sh "python tools/ce_digest.py" default variants/libssi_<other>.so

Cases: ``make_inputs`` of tests/test_ce_z_gpu.py at its ``SHAPES`` (24 rows: ignored, out-of-range and end labels, weights of 0 and 1; the
generic form in fp32 and bf16, the row form with 1, 2 and 17 chunks), its 600-row case (a workgroup walks several rows), and 8 rows (the
first 8 of such 24) at each remaining chunk count of the row form's dispatch.  Two rows of every case are shifted down by 64 so that their
lse < -1 and, at z = 0.5, f = 1 + 2 z lse < 0 (the sign-flip path of the z form)."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speech-integration_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ssi import ops  # noqa: E402
from test_ce_z_gpu import ROWS, SHAPES, make_inputs  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
OTHER_CHUNKS = [(20_000, 20_480), (32_000, 32_768), (65_000, 65_536), (131_000, 131_072), (147_000, 147_456)]   # 3, 4, 8, 16, 18 chunks
Z_COEFFS = (0.0, 1e-4, 0.5)
SMOOTHINGS = (0.0, 0.1)
TOPK = 5


def cases():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for vocab, ld, dtype in SHAPES:
        yield f"{ROWS}x{vocab}/{ld} {dtype}".replace("torch.", ""), vocab, make_inputs(ROWS, vocab, ld, dtype, seed=vocab)
    logits, labels, w = make_inputs(600, 515, 520, BF16, seed=77)   # test_many_rows_per_workgroup_with_ignored_stretches
    labels[0], labels[599] = -100, -100
    labels[::7] = -100
    labels[100:140] = -100
    labels[cus:cus + 3] = -100
    labels[200], labels[413] = 515 + 2, -1
    yield "600x515/520 bfloat16", 515, (logits, labels, w)
    for vocab, ld in OTHER_CHUNKS:
        yield f"8x{vocab}/{ld} bfloat16", vocab, tuple(t[:8].clone() for t in make_inputs(ROWS, vocab, ld, BF16, seed=vocab))


def digest(vocab, logits, labels, w):
    rows = logits.shape[0]
    shifted = [r for r in (2, 6) if r < rows]
    logits = logits.clone()
    logits[shifted, :vocab] = (logits[shifted, :vocab].float() - 64.0).to(logits.dtype)
    h = hashlib.sha256()

    def add(*tensors):
        torch.cuda.synchronize()
        for t in tensors:
            t = t.detach().cpu().contiguous()
            h.update((t.view(torch.int16) if t.dtype == BF16 else t).numpy().tobytes())

    def buf(dtype=torch.float32):
        return torch.full((rows,), 7, device=DEV, dtype=dtype)   # a row an entry does not write shows in the digest

    dlabels = labels.to(DEV)
    for weights in (None, w.to(DEV)):
        for wg in (False, True):
            work, loss, lse = logits.to(DEV), buf(), buf()
            ops.ce_fwd(work, dlabels, vocab, -100, loss, lse, wg, row_weight=weights)
            add(work, loss, lse)
            out = torch.zeros(4, device=DEV)
            ops.ce_reduce(loss, dlabels, vocab, -100, out)
            add(out)
            for z in Z_COEFFS:
                work, loss, lse, rz = logits.to(DEV), buf(), buf(), buf()
                ops.ce_fwd_z(work, dlabels, vocab, -100, z, loss, lse, rz, wg, row_weight=weights)
                add(work, loss, lse, rz)
                for e in SMOOTHINGS:
                    work, loss, lse, ru, rz = logits.to(DEV), buf(), buf(), buf(), buf()
                    ops.ce_fwd_smooth(work, dlabels, vocab, -100, e, z, loss, lse, ru, rz, wg, row_weight=weights)
                    add(work, loss, lse, ru, rz)
            work, loss, lse, ru = logits.to(DEV), buf(), buf(), buf()
            ops.ce_fwd_smooth(work, dlabels, vocab, -100, SMOOTHINGS[-1], 0.0, loss, lse, ru, None, wg, row_weight=weights)   # z = 0 needs no row_z
            add(work, loss, lse, ru)
        work, loss, lse, nll, rank = logits.to(DEV), buf(), buf(), buf(), buf(torch.int32)
        ops.ce_fwd_metrics(work, dlabels, vocab, -100, loss, lse, nll, rank, row_weight=weights)
        add(work, loss, lse, nll, rank)
    ranges = torch.tensor([0, vocab // 3, vocab // 3 + 1, vocab - 1, 5, 5], device=DEV)
    out = torch.zeros(4, 4, device=DEV, dtype=torch.float64)
    for accumulate in (False, True):
        ops.ce_metrics_reduce(nll, rank, dlabels, ranges, TOPK, out, accumulate=accumulate)
        add(out)
    start = torch.tensor([0, 3, rows // 2, rows, -4], device=DEV)
    end = torch.tensor([3, rows // 2, rows + 9, rows, 2], device=DEV)
    out = torch.zeros(5, 4, device=DEV, dtype=torch.float64)
    ops.seq_score_reduce(nll, rank, rows, start, end, TOPK, out)
    add(out)
    return h.hexdigest()


if __name__ == "__main__":
    for name, vocab, (logits, labels, w) in cases():
        print(f"digest {name}: {digest(vocab, logits, labels, w)}", flush=True)
