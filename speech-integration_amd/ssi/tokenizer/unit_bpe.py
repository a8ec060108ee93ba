"""Byte-pair encoding over discrete speech units: learn merges on the device, apply them on the host or the device.

The definition (corpus, pair count, tie-break, left-to-right application, bad ids) is stated once in ``include/ssi_hip.h`` and restated in
``tests/unit_bpe_ref.py``.  A merged unit is one more unit id (``n_base + m``), so everything after the tokens — ``dsu2pua``, the vocabulary
layout with ``speech.n_dsus = n_base + n_merges``, training, scoring, generation — takes it as it is.

* ``train`` runs the trainer kernels (``csrc/unit_bpe.hip``): the ids, the pair-count table, the merge list and a ``done`` word stay on the
  device; the host launches merge after merge and reads the state back every ``READBACK_CADENCE`` merges.
* ``UnitBPE.encode`` is host code (NumPy, lowest rank present first): what a dataset calls per sample.
* ``UnitBPE.encode_many`` encodes many sequences in one launch.

Nothing imports this module unless ``speech.unit_bpe`` is set or it is called directly."""
from __future__ import annotations

import json
import os
from typing import Any, Iterable, Sequence

import numpy as np

SEP = -1
MAX_VOCAB = 16384            # _lib.BPE_MAX_VOCAB: the dense table of the trainer is uint32[MAX_VOCAB ** 2] = 1 GiB at most
READBACK_CADENCE = 8         # merges launched between two reads of the state, as generate's token loop
FILE_VERSION = 1


def flatten(corpus: Any) -> np.ndarray:
    """A list of int sequences as one flat int32 buffer, a separator between neighbours; a flat buffer (1-d array) is taken as it is."""
    if isinstance(corpus, np.ndarray) and corpus.ndim == 1 and corpus.dtype != object:
        return np.ascontiguousarray(corpus, dtype=np.int32)
    if hasattr(corpus, "detach"):   # a torch tensor
        return np.ascontiguousarray(corpus.detach().cpu().numpy().reshape(-1), dtype=np.int32)
    seqs = [np.asarray(s, dtype=np.int32).reshape(-1) for s in corpus]
    if not seqs:
        return np.zeros(0, dtype=np.int32)
    out = np.full(sum(len(s) for s in seqs) + len(seqs) - 1, SEP, dtype=np.int32)
    at = 0
    for s in seqs:
        out[at:at + len(s)] = s
        at += len(s) + 1
    return out


def _corpus_stats(buf: np.ndarray) -> tuple[int, int]:
    """(sequences, ids) of a flat buffer: separators divide, and do not count as ids."""
    n_sep = int((buf == SEP).sum())
    return n_sep + 1, int(buf.size - n_sep)


class UnitBPE:
    def __init__(self, n_base: int, merges: Sequence[Sequence[int]], counts: Sequence[int] | None = None, min_frequency: int = 2,
                 corpus: dict[str, int] | None = None):
        self.n_base = int(n_base)
        self.merges = [(int(a), int(b)) for a, b in merges]
        self.counts = [int(c) for c in counts] if counts is not None else [0] * len(self.merges)
        self.min_frequency = int(min_frequency)
        self.corpus = dict(corpus or {})
        if self.n_base < 1 or len(self.counts) != len(self.merges):
            raise ValueError("UnitBPE: n_base must be positive and counts must match merges")
        for r, (a, b) in enumerate(self.merges):
            if not (0 <= a < self.n_base + r and 0 <= b < self.n_base + r):
                raise ValueError(f"UnitBPE: merge {r} = ({a}, {b}) refers to an id at or above its own, {self.n_base + r}")
        if len(set(self.merges)) != len(self.merges):
            raise ValueError("UnitBPE: a pair is merged twice")
        V = self.vocab_size
        keys = np.array([a * V + b for a, b in self.merges], dtype=np.int64)
        order = np.argsort(keys, kind="stable")
        self._keys, self._ranks = keys[order], order.astype(np.int64)
        self._rank_table = None   # the dense device table of encode_many, built on first use

    @property
    def n_merges(self) -> int:
        return len(self.merges)

    @property
    def vocab_size(self) -> int:
        """``n_base + n_merges``: what ``speech.n_dsus`` must be."""
        return self.n_base + len(self.merges)

    # ---- host encoder --------------------------------------------------------------------------------------------------------------------
    def _pair_ranks(self, x: np.ndarray) -> np.ndarray:
        """Rank of every adjacent pair of ``x`` (int64), ``n_merges`` where there is none.  Ids outside ``[0, V)`` pair with nothing."""
        V, none = self.vocab_size, len(self.merges)
        left, right = x[:-1], x[1:]
        ok = (left >= 0) & (left < V) & (right >= 0) & (right < V)
        key = np.where(ok, left * V + right, -1)
        at = np.minimum(np.searchsorted(self._keys, key), max(len(self._keys) - 1, 0))
        if not len(self._keys):
            return np.full(key.shape, none, dtype=np.int64)
        return np.where(self._keys[at] == key, self._ranks[at], none)

    def encode(self, units: Iterable[int]) -> list[int]:
        """Repeatedly apply the lowest-numbered merge that has an adjacent pair present, left to right (equal to applying merges 0, 1, ... in
        order: see the header).  Separators and ids outside the vocabulary stay and divide."""
        x = np.asarray(list(units) if not isinstance(units, np.ndarray) else units, dtype=np.int64).reshape(-1)
        none = len(self.merges)
        while x.size >= 2:
            ranks = self._pair_ranks(x)
            r = int(ranks.min())
            if r == none:
                break
            at = np.flatnonzero(ranks == r)
            # neighbouring hits are a run of one id (a == b): of each run of hits, those at an even offset start a merge
            first = np.ones(at.size, dtype=bool)
            first[1:] = at[1:] != at[:-1] + 1
            run_start = np.maximum.accumulate(np.where(first, np.arange(at.size), 0))
            at = at[(np.arange(at.size) - run_start) % 2 == 0]
            x = x.copy()
            x[at] = self.n_base + r
            keep = np.ones(x.size, dtype=bool)
            keep[at + 1] = False
            x = x[keep]
        return x.tolist()

    def decode(self, ids: Iterable[int]) -> list[int]:
        out, stack = [], [int(v) for v in ids][::-1]
        top = self.vocab_size
        while stack:
            v = stack.pop()
            if self.n_base <= v < top:
                a, b = self.merges[v - self.n_base]
                stack.append(b)
                stack.append(a)
            else:
                out.append(v)
        return out

    # ---- device encoder ------------------------------------------------------------------------------------------------------------------
    def rank_table(self, device: Any):
        """The dense ``int32[V * V]`` table of the encode kernel (-1: no merge), built once per device."""
        import torch
        device = torch.device(device)
        if self._rank_table is None or self._rank_table.device != device:
            V = self.vocab_size
            table = torch.full((V * V,), -1, dtype=torch.int32, device=device)
            if self.merges:
                keys = torch.tensor([a * V + b for a, b in self.merges], dtype=torch.int64, device=device)
                table[keys] = torch.arange(len(self.merges), dtype=torch.int32, device=device)
            self._rank_table = table
        return self._rank_table

    def encode_many(self, seqs: Sequence[Iterable[int]], device: Any = "cuda") -> list[list[int]]:
        """Every sequence encoded by the kernel, one workgroup per sequence.  Sequences longer than ``_lib.BPE_ENCODE_MAX_LEN`` are refused."""
        import torch
        from .. import _lib, ops
        arrays = [np.asarray(s if isinstance(s, np.ndarray) else list(s), dtype=np.int32).reshape(-1) for s in seqs]
        if not arrays:
            return []
        lens = np.array([a.size for a in arrays], dtype=np.int32)
        max_len = int(lens.max())
        if max_len > _lib.BPE_ENCODE_MAX_LEN:
            raise ValueError(f"encode_many: a sequence of {max_len} ids, above the kernel's {_lib.BPE_ENCODE_MAX_LEN}; use encode")
        starts = np.zeros(len(arrays), dtype=np.int64)
        np.cumsum(lens[:-1], out=starts[1:])
        flat = np.concatenate(arrays) if int(lens.sum()) else np.zeros(0, dtype=np.int32)
        dev = torch.device(device)
        tokens = torch.from_numpy(flat).to(dev)
        out, out_len = torch.empty_like(tokens), torch.empty(len(arrays), dtype=torch.int32, device=dev)
        ops.bpe_encode(tokens, torch.from_numpy(starts).to(dev), torch.from_numpy(lens).to(dev), max_len, self.rank_table(dev), self.vocab_size,
                       self.n_base, out, out_len)
        out_h, len_h = out.cpu().numpy(), out_len.cpu().numpy()
        assert (len_h >= 0).all()
        return [out_h[s:s + n].tolist() for s, n in zip(starts.tolist(), len_h.tolist())]

    # ---- file ----------------------------------------------------------------------------------------------------------------------------
    def to_dict(self) -> dict[str, Any]:
        return {"version": FILE_VERSION, "n_base": self.n_base, "merges": [list(m) for m in self.merges], "counts": list(self.counts),
                "min_frequency": self.min_frequency, "corpus": dict(self.corpus)}

    def save(self, path: Any) -> None:
        with open(path, "w", encoding="utf-8") as f:
            json.dump(self.to_dict(), f)
            f.write("\n")

    @classmethod
    def load(cls, path: Any) -> "UnitBPE":
        with open(path, encoding="utf-8") as f:
            d = json.load(f)
        if d.get("version") != FILE_VERSION:
            raise ValueError(f"{path}: unit BPE file version {d.get('version')!r}, expected {FILE_VERSION}")
        return cls(d["n_base"], d["merges"], d.get("counts"), d.get("min_frequency", 2), d.get("corpus"))

    def __eq__(self, other: object) -> bool:
        return isinstance(other, UnitBPE) and self.to_dict() == other.to_dict()


def load_unit_bpe(spec: Any) -> UnitBPE | None:
    """``speech.unit_bpe`` as the data path takes it: ``None``, a ``UnitBPE``, or the path of a merges file."""
    if spec is None or isinstance(spec, UnitBPE):
        return spec
    return UnitBPE.load(os.fspath(spec))


class DeviceTrainer:
    """The trainer's device state and its launches, one merge at a time (``train`` drives it; the tests look at the table between merges)."""

    def __init__(self, buf: Any, n_base: int, n_merges: int, min_frequency: int = 2, device: Any = "cuda"):
        import torch
        from .. import _lib, ops
        self._ops, self._lib = ops, _lib
        self.n_base, self.n_merges, self.min_frequency = int(n_base), int(n_merges), int(min_frequency)
        self.v_cap = self.n_base + self.n_merges
        if self.v_cap > _lib.BPE_MAX_VOCAB:
            raise ValueError(f"n_base + n_merges = {self.v_cap} is above {_lib.BPE_MAX_VOCAB}")
        if self.n_merges < 1 or self.min_frequency < 1:
            raise ValueError("n_merges and min_frequency must be at least 1")
        dev = torch.device(device)
        ids = (buf if hasattr(buf, "detach") else torch.from_numpy(np.ascontiguousarray(buf, dtype=np.int32))).to(dev, torch.int32).contiguous()
        self.n0 = ids.numel()
        self.bufs = [torch.empty_like(ids), torch.empty_like(ids)]
        self.table = torch.empty(self.v_cap * self.v_cap, dtype=torch.int32, device=dev)
        self.merge_list = torch.zeros(3 * self.n_merges, dtype=torch.int32, device=dev)
        self.state = torch.zeros(_lib.BPE_STATE_WORDS, dtype=torch.int32, device=dev)
        self.workspace = torch.empty(ops.bpe_train_workspace_bytes(self.n0), dtype=torch.uint8, device=dev)
        ops.bpe_train_begin(ids, self.n_base, self.v_cap, self.bufs[0], self.table, self.state)
        self.launched, self.n_upper = 0, self.n0

    def launch(self) -> None:
        """Merge number ``launched``: five launches, nothing read back."""
        assert self.launched < self.n_merges
        self._ops.bpe_merge(self.bufs[0], self.bufs[1], self.n_upper, self.n_base, self.v_cap, self.launched, self.min_frequency, self.table,
                            self.merge_list, self.state, self.workspace)
        self.launched += 1

    def read_state(self) -> dict[str, int]:
        """Read the state back (a synchronisation) and tighten the bound on the length that sizes the next launches."""
        L = self._lib
        s = self.state.cpu().tolist()
        m = s[L.BPE_ST_M]
        self.n_upper = s[L.BPE_ST_LEN + (m & 1)] if (s[L.BPE_ST_DONE] or m == self.launched) else self.n_upper
        return {"done": s[L.BPE_ST_DONE], "m": m, "n_bad": s[L.BPE_ST_NBAD], "n": s[L.BPE_ST_LEN + (m & 1)]}

    def buffer(self):
        """The current ids (after the merges made so far), a view of the device buffer."""
        st = self.read_state()
        return self.bufs[st["m"] & 1][:st["n"]]

    def run(self, cadence: int = READBACK_CADENCE) -> dict[str, int]:
        while self.launched < self.n_merges:
            self.launch()
            if self.launched % cadence == 0 and self.read_state()["done"]:
                break
        return self.read_state()

    def result(self) -> tuple[list[tuple[int, int]], list[int], np.ndarray, int]:
        st = self.read_state()
        ml = self.merge_list.cpu().numpy().reshape(-1, 3)[:st["m"]]
        return [(int(a), int(b)) for a, b, _ in ml], [int(c) for _, _, c in ml], self.bufs[st["m"] & 1][:st["n"]].cpu().numpy(), st["n_bad"]


def check_corpus(buf: np.ndarray, n_base: int, n_merges: int) -> None:
    """The refusals that come before any launch."""
    if n_base + n_merges > MAX_VOCAB:
        raise ValueError(f"n_base + n_merges = {n_base + n_merges} is above {MAX_VOCAB}")
    if buf.size == 0 or not (buf != SEP).any():
        raise ValueError("unit BPE: the corpus is empty")
    if buf.size >= 2 ** 31:
        raise ValueError(f"unit BPE: a corpus of {buf.size} ids; at most 2^31 - 1 in one call (subsample)")
    hi, lo = int(buf.max()), int(buf.min())
    if hi >= n_base or lo < SEP:
        raise ValueError(f"unit BPE: the corpus holds the id {hi if hi >= n_base else lo}, outside [0, n_base = {n_base})")


def train(corpus: Any, n_base: int, n_merges: int, min_frequency: int = 2, device: Any = "cuda", cadence: int = READBACK_CADENCE) -> UnitBPE:
    """Learn up to ``n_merges`` merges over ``corpus`` (a list of int sequences, or a flat buffer with -1 between sequences)."""
    buf = flatten(corpus)
    check_corpus(buf, int(n_base), int(n_merges))
    trainer = DeviceTrainer(buf, n_base, n_merges, min_frequency, device)
    trainer.run(cadence)
    merges, counts, final, _ = trainer.result()
    seqs, ids = _corpus_stats(buf)
    seqs_after, ids_after = _corpus_stats(final)
    return UnitBPE(n_base, merges, counts, min_frequency,
                   {"sequences": seqs, "ids_before": ids, "sequences_after": seqs_after, "ids_after": ids_after})
