#!/usr/bin/env python
"""What learning and applying unit-BPE merges costs (``ssi_bpe_*``, ``ssi/tokenizer/unit_bpe.py``).
    python tools/unit_bpe_bench.py [--json profiles/unit_bpe.json] [--rounds 7] [--sizes 2,16,64] [--n-merges 3000]

corpus   No real units are at hand, so the corpus is drawn: sequences of 1000 ids, each a first-order Markov chain over ``n_base`` = 5000 symbols
         whose transitions out of a state are Zipf-distributed over a state-specific order of the symbols (fixed seed).  Uniform random units
         have flat pair counts, which hides the contention of the count updates; this chain has a few heavy pairs.  The compression ratio it
         gives is recorded and says NOTHING about real units.
train    2 M, 16 M and 64 M ids, 3000 merges, the whole device training (``DeviceTrainer.run``: launches plus a state read every 8 merges)
         behind one synchronise, host clock; ONE process alternates the sizes over ``--rounds`` rounds: median (min - max), total and per
         merge.  The per-merge time is set against the time its unavoidable traffic would take at 5.4 - 6.4 TB/s (the AdamW and EMA passes):
         the ids read and written once (8 bytes per id, at the length the merge starts from) and (n_base + m)^2 counts read once.
split    per kernel, from ``torch.profiler`` over a run of the middle size (device time summed by kernel name): best pair
         (``bpe_best_partial`` + ``bpe_best_final``), mark + scan (``bpe_mark`` + ``bpe_scan``), and ``bpe_apply``, which closes up AND
         updates the counts in one launch: the two are not timed apart.
numpy    the same training restated in NumPy on the host (pair keys, ``bincount``, arg-max with the same tie-break, a vectorised
         left-to-right merge), the first ``--numpy-merges`` merges of the 2 M corpus, whose merges must equal the device's; per merge.
         No earlier number exists: this is the baseline.
encode   up to 4096 sequences of 1000 ids (1999 at the default sizes: what the 2 M corpus holds) through ``encode_many`` (with the copies to and from the device) and through the kernel alone, against
         ``UnitBPE.encode`` on the host over the first 64 of them, in sequences per second, beside the samples per second the headline
         training step consumes (``bench.py``: 8 rows of 2048 tokens in ``--step-ms``).
Nothing is asserted on the times."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speech-integration_amd")
sys.path[:0] = [ROOT, PKG, os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=None)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--sizes", default="2,16,64", help="corpus sizes in M ids")
ap.add_argument("--n-base", type=int, default=5000)
ap.add_argument("--n-merges", type=int, default=3000)
ap.add_argument("--numpy-merges", type=int, default=40)
ap.add_argument("--step-ms", type=float, default=103.7, help="headline training step (bench.py --gpus 1, 8 x 2048 tokens)")
args = ap.parse_args()

from ssi import _lib, ops  # noqa: E402
from ssi.tokenizer import unit_bpe as ub  # noqa: E402

DEV = "cuda:0"
SEQ = 1000


def spread(values, digits=3):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits)}


def draw_corpus(n_ids: int, V: int, seed: int = 1234, alpha: float = 1.2) -> torch.Tensor:
    """``n_ids // SEQ`` chains of SEQ ids, all advanced together on the device, as one flat int32 buffer with -1 between them."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    n_seq = max(n_ids // SEQ, 1)
    p = 1.0 / torch.arange(1, V + 1, device=DEV, dtype=torch.float64) ** alpha
    cdf = torch.cumsum(p / p.sum(), 0).float()
    mult = (2 * torch.randint(0, V // 2, (V,), device=DEV, generator=g) + 1).long()
    out = torch.full((n_seq, SEQ + 1), -1, dtype=torch.int32, device=DEV)
    s = torch.randint(0, V, (n_seq,), device=DEV, generator=g)
    for t in range(SEQ):
        rank = torch.searchsorted(cdf, torch.rand(n_seq, device=DEV, generator=g)).clamp_(max=V - 1)
        s = (s * mult[s] + rank + 1) % V
        out[:, t] = s.int()
    return out.reshape(-1)[:-1].contiguous()


def numpy_train(buf: np.ndarray, n_base: int, n_merges: int, min_frequency: int = 2):
    """The definition in NumPy; returns (merges, counts, seconds per merge)."""
    x = buf.astype(np.int64)
    merges, counts, times = [], [], []
    for m in range(n_merges):
        t0 = time.perf_counter()
        V = n_base + m
        ok = (x[:-1] >= 0) & (x[1:] >= 0)
        key = x[:-1][ok] * V + x[1:][ok]
        c = np.bincount(key, minlength=1)
        best = int(c.argmax())                       # the first maximum: the smallest a V + b
        if c[best] < min_frequency:
            break
        a, b = divmod(best, V)
        hit = np.flatnonzero((x[:-1] == a) & (x[1:] == b))
        if a == b and hit.size:                      # of each run of hits, those at an even offset
            first = np.ones(hit.size, dtype=bool)
            first[1:] = hit[1:] != hit[:-1] + 1
            start = np.maximum.accumulate(np.where(first, np.arange(hit.size), 0))
            hit = hit[(np.arange(hit.size) - start) % 2 == 0]
        x[hit] = V
        keep = np.ones(x.size, dtype=bool)
        keep[hit + 1] = False
        x = x[keep]
        merges.append((a, b))
        counts.append(int(c[best]))
        times.append(time.perf_counter() - t0)
    return merges, counts, times


def train_once(ids: torch.Tensor):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr = ub.DeviceTrainer(ids, args.n_base, args.n_merges, 2, DEV)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    st = tr.run()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return tr, st, t1 - t0, t2 - t1


def main():
    result = {"device": torch.cuda.get_device_name(0), "n_base": args.n_base, "n_merges": args.n_merges, "rounds": args.rounds, "tile": _lib.BPE_TILE,
              "cadence": ub.READBACK_CADENCE, "corpus": f"Zipf(1.2)-Markov chains of {SEQ} ids, seed 1234; says nothing about real units"}
    sizes = [int(float(s) * 1e6) for s in args.sizes.split(",")]
    corpora = {n: draw_corpus(n, args.n_base) for n in sizes}
    timings = {n: {"begin_s": [], "merges_s": []} for n in sizes}
    info = {}
    for r in range(args.rounds + 1):                 # round 0 warms up (allocator, code objects) and is not counted
        for n in sizes:
            tr, st, t_begin, t_merges = train_once(corpora[n])
            if r:
                timings[n]["begin_s"].append(t_begin)
                timings[n]["merges_s"].append(t_merges)
            else:
                merge_list = tr.merge_list.cpu().numpy().reshape(-1, 3)[:st["m"]]
                n_ids = int((corpora[n] >= 0).sum())
                final = tr.buffer()
                ids_after = int((final >= 0).sum())
                info[n] = {"ids": n_ids, "buffer": corpora[n].numel(), "merges_made": st["m"], "ids_after": ids_after, "ratio": round(n_ids / ids_after, 4),
                           "first_counts": merge_list[:3, 2].tolist(), "last_count": int(merge_list[-1, 2]) if st["m"] else None,
                           "first_merges": merge_list[:3, :2].tolist()}
            del tr
    result["train"] = {}
    for n in sizes:
        made = max(info[n]["merges_made"], 1)
        per_merge_us = [1e6 * t / made for t in timings[n]["merges_s"]]
        # the floor: ids read and written once at the length the merge starts from (bounded above by the initial length and below by the final
        # one), and (n_base + m)^2 counts of 4 bytes read once, averaged over the merges
        table_bytes = sum(4 * (args.n_base + m) ** 2 for m in range(made)) / made
        lo = (8 * info[n]["ids_after"] + table_bytes) / 6.4e12 * 1e6
        hi = (8 * info[n]["buffer"] + table_bytes) / 5.4e12 * 1e6
        result["train"][f"{n // 10**6}M"] = {**info[n], "begin_ms": spread([1e3 * t for t in timings[n]["begin_s"]]),
                                              "merges_s": spread(timings[n]["merges_s"], 4), "per_merge_us": spread(per_merge_us, 1),
                                              "traffic_floor_us_per_merge": [round(lo, 1), round(hi, 1)]}
        print(f"train {n // 10**6}M: {result['train'][f'{n // 10**6}M']}", flush=True)

    # per-kernel split at the middle size
    mid = sizes[len(sizes) // 2]
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            tr, st, _, _ = train_once(corpora[mid])
        groups = {"best_pair": ("bpe_best_partial", "bpe_best_final"), "mark_scan": ("bpe_mark", "bpe_scan"), "apply_closeup_and_counts": ("bpe_apply",)}
        per = {}
        for ev in prof.key_averages():
            dev_us = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
            for g, names in groups.items():
                if any(nm in ev.key for nm in names):
                    per[g] = per.get(g, 0.0) + dev_us
        made = max(st["m"], 1)
        result["split"] = {"size": f"{mid // 10**6}M", "per_merge_us": {g: round(v / made, 2) for g, v in per.items()}, "how": "torch.profiler device time by kernel name"}
        del tr
    except Exception as e:   # the profiler is a convenience here, not the measurement
        result["split"] = {"error": repr(e)}
    print(f"split: {result['split']}", flush=True)

    # NumPy baseline on the smallest corpus
    small = sizes[0]
    host = corpora[small].cpu().numpy()
    merges, counts, times = numpy_train(host, args.n_base, args.numpy_merges)
    tr, st, _, _ = train_once(corpora[small])
    dev_merges = tr.merge_list.cpu().numpy().reshape(-1, 3)[:len(merges)]
    same = [tuple(m) for m in dev_merges[:, :2].tolist()] == merges and dev_merges[:, 2].tolist() == counts
    result["numpy"] = {"size": f"{small // 10**6}M", "merges": len(merges), "per_merge_ms": spread([1e3 * t for t in times], 2), "equals_device": bool(same)}
    print(f"numpy: {result['numpy']}", flush=True)

    # encoding
    bpe = ub.UnitBPE(args.n_base, [tuple(m) for m in tr.merge_list.cpu().numpy().reshape(-1, 3)[:st["m"], :2].tolist()])
    del tr
    n_seq = min(4096, (corpora[small].numel() + 1) // (SEQ + 1) - 1)
    seqs = corpora[small].reshape(-1)[: n_seq * (SEQ + 1)].reshape(n_seq, SEQ + 1)[:, :SEQ].contiguous()
    host_seqs = seqs.cpu().numpy()
    tokens = seqs.reshape(-1).contiguous()
    starts = (torch.arange(n_seq, device=DEV, dtype=torch.int64) * SEQ)
    lens = torch.full((n_seq,), SEQ, dtype=torch.int32, device=DEV)
    out, out_len = torch.empty_like(tokens), torch.empty(n_seq, dtype=torch.int32, device=DEV)
    table = bpe.rank_table(DEV)
    enc = {"many_s": [], "kernel_s": [], "host_s": []}
    n_host = 64
    for r in range(args.rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = bpe.encode_many(list(host_seqs), device=DEV)
        t1 = time.perf_counter()
        ops.bpe_encode(tokens, starts, lens, SEQ, table, bpe.vocab_size, bpe.n_base, out, out_len)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        want = [bpe.encode(s) for s in host_seqs[:n_host]]
        t3 = time.perf_counter()
        assert got[:n_host] == want
        if r:
            enc["many_s"].append(t1 - t0); enc["kernel_s"].append(t2 - t1); enc["host_s"].append(t3 - t2)
    mean_after = float(out_len.float().mean())
    step_samples = 8 * 2048 / SEQ / (args.step_ms / 1e3)
    result["encode"] = {"sequences": n_seq, "ids_per_sequence": SEQ, "ids_after_mean": round(mean_after, 1),
                        "encode_many_seq_per_s": spread([n_seq / t for t in enc["many_s"]], 0), "kernel_seq_per_s": spread([n_seq / t for t in enc["kernel_s"]], 0),
                        "host_seq_per_s": spread([n_host / t for t in enc["host_s"]], 1),
                        "training_step_consumes_seq_per_s": round(step_samples, 1), "step_ms": args.step_ms}
    print(f"encode: {result['encode']}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
