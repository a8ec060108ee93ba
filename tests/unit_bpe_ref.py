"""The definition of byte-pair encoding over speech units (``include/ssi_hip.h``, "Byte-pair encoding over discrete speech units"), restated
in plain Python: lists and dicts, one step at a time, nothing shared with ``ssi/tokenizer/unit_bpe.py`` or the kernels.  Not a test module;
``test_unit_bpe_ref.py`` checks it by hand-worked cases and planted defects, the GPU tests compare the kernels against it.

A corpus is one flat list of symbols in ``[0, V)`` with sequences divided by ``SEP``; a symbol outside ``[0, V)`` other than ``SEP`` is bad:
it acts as a separator, the trainer counts it once and keeps a separator in its place."""
from __future__ import annotations

SEP = -1

# (name, buffer, n_base, n_merges, min_frequency) -> (merges, counts, final buffer), each worked by hand
HAND_CASES = [
    # c(0,0) = 4 -> [1 1 0]; then (1,0) and (1,1) hold one each: below 2
    ("aaaaa", [0, 0, 0, 0, 0], 1, 5, 2, ([(0, 0)], [4], [1, 1, 0])),
    # the same down to one id: (1,0) wins the tie against (1,1) by b -> [1 2]; then (1,2) -> [3]
    ("aaaaa-to-the-end", [0, 0, 0, 0, 0], 1, 5, 1, ([(0, 0), (1, 0), (1, 2)], [4, 1, 1], [3])),
    # (2,3), (0,5), (0,1) hold two each: the smallest a is 0, then the smallest b is 1
    ("tie-by-a-then-b", [2, 3, SEP, 2, 3, SEP, 0, 5, SEP, 0, 5, SEP, 0, 1, SEP, 0, 1], 6, 1, 2,
     ([(0, 1)], [2], [2, 3, SEP, 2, 3, SEP, 0, 5, SEP, 0, 5, SEP, 6, SEP, 6])),
    # without the separators (0,1) would hold two; with them every pair holds one
    ("pair-across-a-separator", [0, SEP, 1, 0, SEP, 1, 2, 2], 3, 4, 2, ([], [], [0, SEP, 1, 0, SEP, 1, 2, 2])),
    # (0,1) twice -> [4 4 2 3]: (4,4), (4,2), (2,3) once each, so the second of five merges is not made
    ("stop-by-min-frequency", [0, 1, 0, 1, 2, 3], 4, 5, 2, ([(0, 1)], [2], [4, 4, 2, 3])),
    # 0 0 0 holds (0,0) twice (overlapping), as many as (1,1) in two sequences: (0,0) wins by a, but only one window merges
    ("overlapping-count-one-merge", [0, 0, 0, 1, 1, SEP, 1, 1], 2, 1, 2, ([(0, 0)], [2], [2, 0, 1, 1, SEP, 1, 1])),
    # an odd run: the leftover a comes last
    ("odd-run", [1, 0, 0, 0, 1], 2, 1, 2, ([(0, 0)], [2], [1, 2, 0, 1])),
]


def flatten(seqs):
    """Sequences as one buffer: a separator between neighbours (none at either end)."""
    out = []
    for k, s in enumerate(seqs):
        if k:
            out.append(SEP)
        out.extend(int(v) for v in s)
    return out


def split(buf):
    seqs, cur = [], []
    for v in buf:
        if v == SEP:
            seqs.append(cur)
            cur = []
        else:
            cur.append(v)
    seqs.append(cur)
    return seqs


def sanitise(buf, V):
    """(buffer with bad ids replaced by the separator, number of bad ids)."""
    out, n_bad = [], 0
    for v in buf:
        if v == SEP or 0 <= v < V:
            out.append(v)
        else:
            out.append(SEP)
            n_bad += 1
    return out, n_bad


def pair_counts(buf, V):
    """``{(a, b): c(a, b)}`` over positions, overlapping ones included; a pair never holds a separator or a bad id."""
    counts = {}
    for i in range(len(buf) - 1):
        a, b = buf[i], buf[i + 1]
        if 0 <= a < V and 0 <= b < V:
            counts[(a, b)] = counts.get((a, b), 0) + 1
    return counts


def best_pair(counts):
    """The largest count; ties by the smallest a, then the smallest b.  ``None`` for no pair at all."""
    best = None
    for (a, b), c in counts.items():
        if best is None or c > best[2] or (c == best[2] and (a, b) < (best[0], best[1])):
            best = (a, b, c)
    return best


def apply_merge(buf, a, b, z):
    """Left to right: where ``(x[i], x[i+1]) == (a, b)`` write ``z`` and continue at ``i + 2``.  Separators stay."""
    out, i, n = [], 0, len(buf)
    while i < n:
        if i + 1 < n and buf[i] == a and buf[i + 1] == b:
            out.append(z)
            i += 2
        else:
            out.append(buf[i])
            i += 1
    return out


def train(buf, n_base, n_merges, min_frequency=2, trace=None):
    """``(merges [(a, b)], counts [c], final buffer, n_bad)``.  ``trace`` (a list) receives the buffer after every merge."""
    buf, n_bad = sanitise(list(buf), n_base)
    merges, counts = [], []
    for m in range(n_merges):
        best = best_pair(pair_counts(buf, n_base + m))
        if best is None or best[2] < min_frequency:
            break
        a, b, c = best
        buf = apply_merge(buf, a, b, n_base + m)
        merges.append((a, b))
        counts.append(c)
        if trace is not None:
            trace.append(list(buf))
    return merges, counts, buf, n_bad


def encode(seq, merges, n_base):
    """Merges 0, 1, ... applied in order."""
    seq = list(seq)
    for r, (a, b) in enumerate(merges):
        seq = apply_merge(seq, a, b, n_base + r)
    return seq


def decode(ids, merges, n_base):
    out, stack = [], list(reversed(list(ids)))
    while stack:
        v = stack.pop()
        if v >= n_base:
            a, b = merges[v - n_base]
            stack.append(b)
            stack.append(a)
        else:
            out.append(v)
    return out


def zipf_markov(n, V, seed, alpha=1.2):
    """``n`` symbols of a first-order Markov chain whose transitions out of every state are Zipf-distributed over a state-specific
    permutation of the symbols: a few pairs carry most of the mass, as in real unit streams (uniform symbols have flat pair counts)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, V + 1) ** alpha
    cdf = np.cumsum(p / p.sum())
    ranks = np.minimum(np.searchsorted(cdf, rng.random(n)), V - 1)
    mult = 2 * rng.integers(0, max(V // 2, 1), size=V) + 1   # target = (state * mult[state] + rank + 1) mod V: a permutation of the ranks per state
    out = np.empty(n, dtype=np.int64)
    s = 0
    for i in range(n):
        s = int((s * int(mult[s]) + int(ranks[i]) + 1) % V)
        out[i] = s
    return out.tolist()
