#!/usr/bin/env python
"""What the edit-distance kernel costs (``ssi_edit_distance``), and what MBR selection adds to a ``sample`` call.
    python tools/edit_distance_bench.py [--json profiles/edit_distance.json] [--rounds 7] [--no-model]

kernel   four shapes of random ids (an alphabet of 1000; the work does not depend on the ids): 7168 pairs of 40 to 80 ids, 7168 pairs of 256,
         256 pairs of 4096, one pair of 4096.  The span arrays are on the device before the clock starts; a round times ``inner`` launches
         behind one synchronise (host clock) and reports the time per launch.  Against it, on the host, a NumPy restatement of the DISTANCE
         only, vectorised along anti-diagonals (written below), on the first pairs of every shape (7168 pairs of it would take minutes); its
         distances must equal the kernel's.  ONE process alternates kernel and NumPy over ``--rounds`` rounds: median (min - max).
         Reported: time per launch, time per pair, cell updates per second (cells = sum of m * n over the pairs).
mbr      ``sample`` of 256 prompts x 8 candidates x 256 new tokens on the 1B shape (Llama-3.2-1B + 5000 units, bf16, random weights, no stop
         token: every candidate 256 ids, 7168 pairs), once, then ``mbr_select`` on its candidates over the rounds, as a share of that call.
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
ap.add_argument("--no-model", action="store_true", help="the kernel part alone")
args = ap.parse_args()


def numpy_distance(r: np.ndarray, h: np.ndarray) -> int:
    """Edit distance by anti-diagonals: cell (i, j) of diagonal k = i + j needs (i-1, j-1) of k - 2 and (i-1, j), (i, j-1) of k - 1, so a
    whole diagonal is one vector expression.  Diagonals are stored by i."""
    m, n = len(r), len(h)
    if m == 0 or n == 0:
        return m + n
    prev2 = np.zeros(m + 1, dtype=np.int32)       # diagonal k - 2, indexed by i
    prev1 = np.zeros(m + 1, dtype=np.int32)       # diagonal k - 1
    prev1[0], prev1[1] = 1, 1                     # k = 1: (0, 1) and (1, 0)
    cur = np.zeros(m + 1, dtype=np.int32)
    for k in range(2, m + n + 1):
        lo, hi = max(1, k - n), min(m, k - 1)     # interior cells: 1 <= i <= m, 1 <= j = k - i <= n
        if lo <= hi:
            i = np.arange(lo, hi + 1)
            sub = (r[i - 1] != h[k - i - 1]).astype(np.int32)
            cur[lo:hi + 1] = np.minimum(np.minimum(prev2[lo - 1:hi] + sub, prev1[lo - 1:hi] + 1), prev1[lo:hi + 1] + 1)
        if k <= n:
            cur[0] = k                            # (0, k)
        if k <= m:
            cur[k] = k                            # (k, 0)
        prev2, prev1, cur = prev1, cur, prev2
    return int(prev1[m])


def spread(values, digits=3):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits)}


def kernel_part():
    from ssi import ops
    rng = np.random.RandomState(0)
    shapes = {"7168_pairs_of_about_60": ([(int(a), int(b)) for a, b in rng.randint(40, 81, size=(7168, 2))], 20, 64),
              "7168_pairs_of_256": ([(256, 256)] * 7168, 10, 8),
              "256_pairs_of_4096": ([(4096, 4096)] * 256, 3, 1),
              "1_pair_of_4096": ([(4096, 4096)], 3, 1)}
    prepared = {}
    for name, (lens, inner, n_host) in shapes.items():
        seqs = [(rng.randint(0, 1000, size=m).astype(np.int32), rng.randint(0, 1000, size=n).astype(np.int32)) for m, n in lens]
        flat = np.concatenate([x for pair in seqs for x in pair])
        sizes = np.array([len(x) for pair in seqs for x in pair], dtype=np.int64)
        starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        dev = lambda a, dt: torch.tensor(a, dtype=dt).cuda()   # noqa: E731
        bufs = (dev(flat, torch.int32), dev(starts[0::2], torch.int64), dev(sizes[0::2], torch.int32), dev(starts[1::2], torch.int64),
                dev(sizes[1::2], torch.int32), torch.empty((len(lens), 4), dtype=torch.int32, device="cuda"))
        max_len = int(sizes.max())
        launch = lambda bufs=bufs, max_len=max_len: ops.edit_distance(*bufs, max_len)   # noqa: E731
        launch()
        torch.cuda.synchronize()
        prepared[name] = (lens, inner, seqs[:n_host], bufs, launch)
    res = {}
    times = {name: {"kernel_us_per_launch": [], "numpy_ms_per_pair": []} for name in shapes}
    for _ in range(args.rounds):
        for name, (lens, inner, host, bufs, launch) in prepared.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                launch()
            torch.cuda.synchronize()
            times[name]["kernel_us_per_launch"].append((time.perf_counter() - t0) / inner * 1e6)
            t0 = time.perf_counter()
            got = [numpy_distance(r, h) for r, h in host]
            times[name]["numpy_ms_per_pair"].append((time.perf_counter() - t0) / len(host) * 1e3)
            prepared[name] = (lens, inner, host, bufs, launch)
            times[name]["numpy_equals_kernel"] = got == bufs[5][:len(host), 0].cpu().tolist()
    for name, (lens, inner, host, bufs, launch) in prepared.items():
        cells = sum(m * n for m, n in lens)
        host_cells = sum(len(r) * len(h) for r, h in host) / len(host)
        k_us, n_ms = times[name]["kernel_us_per_launch"], times[name]["numpy_ms_per_pair"]
        res[name] = {"pairs": len(lens), "cells": cells, "launches_per_round": inner, "numpy_pairs_per_round": len(host),
                     "kernel_us_per_launch": spread(k_us, 1), "kernel_us_per_pair": spread([t / len(lens) for t in k_us], 3),
                     "kernel_gcells_per_s": spread([cells / t / 1e3 for t in k_us], 2),
                     "numpy_ms_per_pair": spread(n_ms, 3), "numpy_gcells_per_s": spread([host_cells / t / 1e6 for t in n_ms], 4),
                     "numpy_over_kernel_per_pair": round(statistics.median(n_ms) * 1e3 / (statistics.median(k_us) / len(lens)), 1),
                     "numpy_equals_kernel": times[name]["numpy_equals_kernel"]}
        print(name, json.dumps(res[name]), flush=True)
    return res


def mbr_part():
    import copy
    from ssi.generate import mbr_candidate, mbr_select, sample
    from ssi.llama_configs import configllama3_2_1b
    from ssi.model import HipLlamaDecoder
    c = copy.deepcopy(configllama3_2_1b)
    c.n_dsus = 5000
    torch.manual_seed(0)
    model = HipLlamaDecoder(**c.parameters, dtype=torch.bfloat16, device="cuda", rope_cache_len=4096)
    with torch.no_grad():
        flat = model._flat.float().normal_(0.0, 0.02).to(torch.bfloat16)
        model._flat.copy_(flat)
        del flat
        model._view("emb")[model.vocab_size:].zero_()
        for p, name, _ in model._param_src:
            if name.endswith("norm"):
                p.fill_(1.0)
    model.eval()
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(0, model.vocab_size, (int(n),), generator=g) for n in torch.randint(150, 251, (256,), generator=g)]
    kw = dict(n=8, temperature=0.8, top_k=50, top_p=0.9, seed=1, stop_token_ids=[], pad_id=0)
    sample(model, prompts[:4], max_new_tokens=4, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    found = sample(model, prompts, max_new_tokens=256, batch_size=256, **kw)
    torch.cuda.synchronize()
    sample_s = time.perf_counter() - t0
    cands = [[mbr_candidate(x) for x in gs] for gs in found]
    mbr_select(cands[:2], model.device)
    ms = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        order, _ = mbr_select(cands, model.device)
        ms.append((time.perf_counter() - t0) * 1e3)
    res = {"prompts": 256, "n": 8, "max_new_tokens": 256, "pairs": 256 * 28, "sample_call_s_one_run": round(sample_s, 2),
           "mbr_select_ms": spread(ms, 2), "mbr_select_share_of_sample_call": round(statistics.median(ms) / 1e3 / sample_s, 5),
           "prompts_whose_choice_is_not_candidate_0": sum(o[0] != 0 for o in order),
           "note": "mbr_select is host packing of the candidates, the copies, one kernel launch, a few torch ops and one read-back"}
    print("mbr", json.dumps(res), flush=True)
    return res


assert torch.cuda.is_available(), "a measurement needs the GPU"
result = {"what": "ssi_edit_distance, SSI_EDIT_COLS = 4; host clock around launches that end in a synchronise; "
                  f"{args.rounds} rounds alternating kernel and NumPy in one process, median (min - max)",
          "kernel": kernel_part()}
if not args.no_model:
    result["mbr"] = mbr_part()
if args.json:
    with open(args.json, "w") as f:
        json.dump(result, f, indent=1)
