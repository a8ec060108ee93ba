"""CPU: the Python restatement of unit BPE (``tests/unit_bpe_ref.py``) on hand-worked cases, planted defects in copies of it that those cases
must catch, and the host side of ``ssi/tokenizer/unit_bpe.py`` (``UnitBPE.encode`` / ``decode`` / file / the refusals before any launch)
against it."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import unit_bpe_ref as ref
from conftest import ROOT
from ssi import _lib
from ssi.tokenizer import unit_bpe as ub

S = ref.SEP
CASES = ref.HAND_CASES


def failing(mod):
    out = []
    for name, buf, n_base, n_merges, min_f, want in CASES:
        merges, counts, final, n_bad = mod.train(buf, n_base, n_merges, min_f)
        if (merges, counts, final) != want or n_bad != 0:
            out.append(name)
    return out


def copy_of_ref(**planted):
    spec = importlib.util.spec_from_file_location("unit_bpe_ref_copy", ref.__file__)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for k, v in planted.items():
        setattr(mod, k, v)
    return mod


def test_hand_worked_cases():
    assert failing(ref) == []


def _counts_overlap_once(buf, V):
    counts, i = {}, 0
    while i < len(buf) - 1:
        a, b = buf[i], buf[i + 1]
        if 0 <= a < V and 0 <= b < V:
            counts[(a, b)] = counts.get((a, b), 0) + 1
            i += 2 if a == b else 1
        else:
            i += 1
    return counts


def _apply_right_to_left(buf, a, b, z):
    return ref.apply_merge(buf[::-1], b, a, z)[::-1]


def _best_larger_b(counts):
    best = None
    for (a, b), c in counts.items():
        if best is None or c > best[2] or (c == best[2] and (a, -b) < (best[0], -best[1])):
            best = (a, b, c)
    return best


def _counts_across_separators(buf, V):
    return ref.pair_counts([v for v in buf if v != S], V)


def _apply_leftover_first(buf, a, b, z):
    if a != b:
        return ref.apply_merge(buf, a, b, z)
    out, i, n = [], 0, len(buf)
    while i < n:
        j = i
        while j < n and buf[j] == a:
            j += 1
        if j > i:
            k = j - i
            out += [a] * (k % 2) + [z] * (k // 2)
            i = j
        else:
            out.append(buf[i])
            i += 1
    return out


@pytest.mark.parametrize("planted,caught_by", [
    ({"pair_counts": _counts_overlap_once}, "overlapping-count-one-merge"),
    ({"apply_merge": _apply_right_to_left}, "odd-run"),
    ({"best_pair": _best_larger_b}, "tie-by-a-then-b"),
    ({"pair_counts": _counts_across_separators}, "pair-across-a-separator"),
    ({"apply_merge": _apply_leftover_first}, "aaaaa"),
], ids=["overlap-counted-once", "right-to-left", "tie-by-larger-b", "across-a-separator", "leftover-first"])
def test_planted_defects_are_caught(planted, caught_by):
    assert caught_by in failing(copy_of_ref(**planted))


def test_bad_ids_divide_and_are_counted_once():
    merges, counts, final, n_bad = ref.train([0, 1, 7, 0, 1, -5, 0, 1], 2, 3, 2)
    assert (merges, counts, final, n_bad) == ([(0, 1)], [3], [2, S, 2, S, 2], 2)


@pytest.fixture(scope="module")
def learned():
    """Merges of the restatement over a small Zipf-Markov corpus: (n_base, merges, counts, sequences)."""
    V = 12
    seqs = [ref.zipf_markov(n, V, seed) for seed, n in enumerate([0, 1, 2, 3, 50, 120, 333, 700, 900])]
    merges, counts, final, n_bad = ref.train(ref.flatten(seqs), V, 40, 2)
    assert len(merges) == 40 and n_bad == 0
    return V, merges, counts, seqs, final


def test_host_encode_equals_in_order_application(learned):
    V, merges, counts, seqs, final = learned
    bpe = ub.UnitBPE(V, merges, counts)
    extra = [ref.zipf_markov(400, V, 100 + k) for k in range(4)] + [[3] * 17, [3] * 16, [0, 0, 0], []]
    for s in seqs + extra:
        want = ref.encode(s, merges, V)
        assert bpe.encode(s) == want
        assert bpe.encode(np.asarray(s, dtype=np.int32)) == want
        assert bpe.decode(want) == list(s) == ref.decode(want, merges, V)
    # the training corpus, sequence by sequence, encodes to the trainer's final buffer
    assert [bpe.encode(s) for s in seqs] == ref.split(final)
    assert any(len(ref.encode(s, merges, V)) < len(s) for s in extra[:4])
    # separators and ids outside the vocabulary stay where they are and divide
    assert bpe.encode(seqs[5] + [S] + seqs[6] + [V + 40] + seqs[5]) == ref.encode(seqs[5], merges, V) + [S] + ref.encode(seqs[6], merges, V) + \
        [V + 40] + ref.encode(seqs[5], merges, V)


def test_file_round_trip(learned, tmp_path):
    V, merges, counts, seqs, final = learned
    bpe = ub.UnitBPE(V, merges, counts, 2, {"sequences": 9, "ids_before": 2109, "sequences_after": 9, "ids_after": 1000})
    path = tmp_path / "merges.json"
    bpe.save(path)
    d = json.loads(path.read_text())
    assert set(d) == {"version", "n_base", "merges", "counts", "min_frequency", "corpus"} and d["version"] == ub.FILE_VERSION
    assert d["n_base"] == V and d["merges"] == [list(m) for m in merges] and d["counts"] == counts and d["min_frequency"] == 2
    back = ub.UnitBPE.load(path)
    assert back == bpe and back.vocab_size == V + 40 and back.encode(seqs[6]) == bpe.encode(seqs[6])
    assert ub.load_unit_bpe(str(path)) == bpe and ub.load_unit_bpe(None) is None and ub.load_unit_bpe(bpe) is bpe
    d["version"] = 99
    path.write_text(json.dumps(d))
    with pytest.raises(ValueError, match="version"):
        ub.UnitBPE.load(path)
    with pytest.raises(ValueError, match="at or above its own"):
        ub.UnitBPE(4, [(0, 4)])


def test_refusals_come_before_any_launch():
    with pytest.raises(ValueError, match="empty"):
        ub.train([], 4, 2)
    with pytest.raises(ValueError, match="empty"):
        ub.train(np.array([S, S], dtype=np.int32), 4, 2)
    with pytest.raises(ValueError, match=str(ub.MAX_VOCAB)):
        ub.train([[0, 1, 0, 1]], 16000, 385)
    with pytest.raises(ValueError, match=r"holds the id 4, outside \[0, n_base = 4\)"):
        ub.train([[0, 1], [2, 4]], 4, 2)
    with pytest.raises(ValueError, match="outside"):
        ub.train(np.array([0, 1, -2], dtype=np.int32), 4, 2)


def test_flatten_and_constants():
    assert ub.flatten([[1, 2], [], [3]]).tolist() == [1, 2, S, S, 3] == ref.flatten([[1, 2], [], [3]])
    assert ub.flatten(np.array([1, S, 2])).tolist() == [1, S, 2]
    header = open(os.path.join(ROOT, "include", "ssi_hip.h")).read()
    define = lambda name: int(re.search(rf"#define {name} \(?(-?\d+)", header).group(1))   # noqa: E731
    assert define("SSI_ABI_VERSION") == _lib.ABI_VERSION >= 30
    assert (define("SSI_BPE_SEP"), define("SSI_BPE_TILE"), define("SSI_BPE_MAX_VOCAB"), define("SSI_BPE_ENCODE_MAX_LEN"), define("SSI_BPE_STATE_WORDS")) == \
        (_lib.BPE_SEP, _lib.BPE_TILE, _lib.BPE_MAX_VOCAB, _lib.BPE_ENCODE_MAX_LEN, _lib.BPE_STATE_WORDS) == (ub.SEP, 4096, ub.MAX_VOCAB, 4096, 8)
