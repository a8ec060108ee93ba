"""GPU: the unit-BPE kernels (``csrc/unit_bpe.hip``) against the Python restatement (``tests/unit_bpe_ref.py``), exactly: merges, counts,
the final buffer and ``n_bad`` are integers, there is no tolerance.  ``T = SSI_BPE_TILE`` ids per workgroup; the training cases aim at its
edges (lengths, separators, the best pair and runs of one symbol across them), the encoding cases at the lengths where the encoder changes
form (``ENCODE_SHORT`` = 1024 ids: four ids per thread below, sixteen above) and at its limit."""
import numpy as np
import pytest
import torch

import unit_bpe_ref as ref
from ssi import _lib, ops
from ssi.tokenizer import unit_bpe as ub

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = _lib.BPE_TILE
S = ref.SEP
CADENCE = ub.READBACK_CADENCE
ENCODE_SHORT = 1024


def device_train(buf, n_base, n_merges, min_frequency=2, cadence=CADENCE):
    tr = ub.DeviceTrainer(np.asarray(buf, dtype=np.int32), n_base, n_merges, min_frequency, DEV)
    tr.run(cadence)
    merges, counts, final, n_bad = tr.result()
    return merges, counts, final.tolist(), n_bad


def check_against_ref(buf, n_base, n_merges, min_frequency=2, cadence=CADENCE):
    want = ref.train(buf, n_base, n_merges, min_frequency)
    got = device_train(buf, n_base, n_merges, min_frequency, cadence)
    assert got[0] == want[0] and got[1] == want[1], (got[0], got[1], want[0], want[1])
    assert got[3] == want[3]
    assert got[2] == want[2], next((i, g, w) for i, (g, w) in enumerate(zip(got[2] + [None], want[2] + [None])) if g != w)
    return want


def corpus(n, V, seed, sep_every=97):
    buf = ref.zipf_markov(n, V, seed)
    for i in range(sep_every - 1, n, sep_every):
        buf[i] = S
    return buf


@pytest.mark.parametrize("case", ref.HAND_CASES, ids=[c[0] for c in ref.HAND_CASES])
def test_hand_worked_cases(case):
    name, buf, n_base, n_merges, min_f, want = case
    assert device_train(buf, n_base, n_merges, min_f) == (*want, 0)


@pytest.mark.parametrize("n", [0, 1, 2, T - 1, T, T + 1, 2 * T + 3])
def test_lengths_around_the_tile(n):
    want = check_against_ref(corpus(n, 7, seed=n), 7, 6)
    assert n < 100 or len(want[0]) == 6


def test_sequences_of_length_0_1_2():
    buf = [S, 3, S, S, 1, 2, S, 1, 2, S, 5, S, 1, 2, S, S, 2, 1, S]
    want = check_against_ref(buf, 6, 3)
    assert want[0] == [(1, 2)] and want[2].count(S) == buf.count(S)


@pytest.mark.parametrize("at", [T - 1, T, 2 * T - 1, 2 * T], ids=["last-of-tile-0", "first-of-tile-1", "last-of-tile-1", "first-of-tile-2"])
def test_separator_at_a_tile_edge(at):
    buf = [0, 1] * (T + 8)               # (0,1) at every even position: a separator at an odd or even place cuts a different pair
    buf[at] = S
    want = check_against_ref(buf, 2, 4)
    assert len(want[0]) >= 3


@pytest.mark.parametrize("edge", [T, 2 * T])
def test_best_pair_straddles_a_tile_edge(edge):
    buf = [2 + v % 5 for v in ref.zipf_markov(2 * T + 50, 5, seed=edge, alpha=0.0)]
    for i in range(7, 2 * T, 8):            # T - 1 and 2T - 1 are among these
        buf[i], buf[i + 1] = 0, 1
    assert (buf[edge - 1], buf[edge]) == (0, 1)
    want = check_against_ref(buf, 7, 5)
    assert want[0][0] == (0, 1)


@pytest.mark.parametrize("offset", [3, 4, T - 1, T])
def test_a_long_run_across_tiles(offset):
    """A run of 2T + 1 equal symbols: which positions merge depends on the parity of the distance to the run's start, up to two tiles to the
    left.  The later merges pair the new ids again, so the parity is carried for them too."""
    buf = [1] * offset + [0] * (2 * T + 1) + [1, 0, 0, 1, 0, 0, 0, S, 0, 0, 0, 0]
    want = check_against_ref(buf, 2, 6, min_frequency=1)
    assert want[0][0] == (0, 0) and want[1][0] == 2 * T + 6 and len(want[0]) == 6


def test_one_symbol_only():
    """The greatest contention (every count update of a merge goes to one address) and the greatest shrink (the buffer halves every time)."""
    n = 3 * T + 5
    want = check_against_ref([0] * n, 1, 10, min_frequency=1)
    assert want[0][:3] == [(0, 0), (1, 1), (2, 2)] and want[1][0] == n - 1


@pytest.mark.parametrize("V,n,n_merges", [(2, 5000, 12), (7, 9000, 20), (300, 3 * T + 11, 24)])
def test_vocabularies(V, n, n_merges):
    want = check_against_ref(corpus(n, V, seed=V), V, n_merges)
    assert len(want[0]) == n_merges and len(want[2]) < n


def test_stop_by_min_frequency_before_n_merges():
    buf = corpus(6000, 7, seed=5)
    want = check_against_ref(buf, 7, 40, min_frequency=120)
    assert 0 < len(want[0]) < 40 and min(want[1]) >= 120
    # later launches after the stop leave everything as it is: the cadence decides how many there are
    for cadence in (1, 3, 64):
        assert device_train(buf, 7, 40, 120, cadence) == want


@pytest.mark.parametrize("n_merges", [CADENCE - 1, CADENCE, CADENCE + 1])
def test_n_merges_around_the_read_back_cadence(n_merges):
    want = check_against_ref(corpus(3000, 7, seed=11), 7, n_merges)
    assert len(want[0]) == n_merges


def test_ids_out_of_range_divide_and_are_counted_once():
    buf = corpus(2 * T + 9, 7, seed=3)
    for i, v in ((5, 7), (T - 1, 9), (T, -2), (T + 500, 2 ** 31 - 1), (2 * T + 8, -2 ** 31)):
        buf[i] = v
    want = check_against_ref(buf, 7, 8)
    assert want[3] == 5
    # the full count alone: the same table as the restatement's, bad ids counted once
    ids = torch.tensor(buf, dtype=torch.int32, device=DEV)
    table, n_bad = torch.zeros(7 * 9, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.bpe_pair_count(ids, 7, 9, table, n_bad)
    counts = ref.pair_counts(ref.sanitise(buf, 7)[0], 7)
    dense = [[counts.get((a, b), 0) for b in range(7)] + [0, 0] for a in range(7)]
    assert table.view(7, 9).cpu().tolist() == dense and int(n_bad) == 5


@pytest.mark.parametrize("name", ["zipf-7", "runs", "one-symbol"])
def test_the_table_equals_a_full_count_after_every_merge(name):
    """The incremental update: after every merge the device table must equal ``ssi_bpe_pair_count`` of the device buffer, and the buffer
    the restatement's."""
    buf, n_base, n_merges = {"zipf-7": (corpus(T + 700, 7, seed=1), 7, 12),
                             "runs": (([0] * 9 + [1] * 4 + [0, 1] * 3 + [S]) * 400, 2, 10),
                             "one-symbol": ([0] * (T + 3), 1, 8)}[name]
    trace = []
    want = ref.train(buf, n_base, n_merges, 1, trace=trace)
    tr = ub.DeviceTrainer(np.asarray(buf, dtype=np.int32), n_base, n_merges, 1, DEV)
    v_cap = n_base + n_merges
    for m in range(len(want[0])):
        tr.launch()
        cur = tr.buffer()
        assert cur.cpu().tolist() == trace[m], m
        full = torch.zeros(v_cap * v_cap, dtype=torch.int32, device=DEV)
        ops.bpe_pair_count(cur.contiguous(), v_cap, v_cap, full)
        assert torch.equal(full, tr.table), (m, (full != tr.table).nonzero().flatten().tolist()[:8])
    assert tr.result()[0] == want[0]


def test_a_second_run_gives_the_same_bytes():
    buf = np.asarray(corpus(3 * T + 77, 40, seed=9), dtype=np.int32)
    runs = []
    for _ in range(2):
        tr = ub.DeviceTrainer(buf, 40, 16, 2, DEV)
        tr.run()
        runs.append((tr.table.cpu(), tr.merge_list.cpu(), tr.state.cpu(), tr.buffer().cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_train_through_the_public_entry():
    seqs = [ref.zipf_markov(n, 12, seed) for seed, n in enumerate([0, 1, 2, 700, 900, 1500])]
    bpe = ub.train(seqs, 12, 30, device=DEV)
    want = ref.train(ref.flatten(seqs), 12, 30)
    assert bpe.merges == want[0] and bpe.counts == want[1] and bpe.n_base == 12 and bpe.vocab_size == 42
    n_after = len([v for v in want[2] if v != S])
    assert bpe.corpus == {"sequences": 6, "ids_before": 3103, "sequences_after": 6, "ids_after": n_after}
    assert ub.train(np.asarray(ref.flatten(seqs), dtype=np.int32), 12, 30, device=DEV) == bpe


def test_refusals_of_the_entries():
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)   # noqa: E731
    with pytest.raises(RuntimeError, match="code 2"):      # SSI_ERR_UNSUPPORTED before any launch: a table above the cap is never touched
        _lib.check(_lib.load().ssi_bpe_train_begin(i32(4).data_ptr(), 4, 16000, _lib.BPE_MAX_VOCAB + 1, i32(4).data_ptr(), i32(4).data_ptr(),
                                                   i32(8).data_ptr(), None), "ssi_bpe_train_begin")
    with pytest.raises(ValueError, match=str(_lib.BPE_MAX_VOCAB)):
        ub.DeviceTrainer(np.zeros(4, dtype=np.int32), 16000, 385, 2, DEV)


# ---- encoding ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def learned():
    V = 12
    seqs = [ref.zipf_markov(n, V, seed) for seed, n in enumerate([0, 1, 2, 3, 63, 64, 65, 700, 900, 2000])]
    flat = ref.flatten(seqs)
    tr = ub.DeviceTrainer(np.asarray(flat, dtype=np.int32), V, 40, 2, DEV)
    tr.run()
    merges, counts, final, _ = tr.result()
    assert (merges, counts, final.tolist()) == ref.train(flat, V, 40)[:3]
    return ub.UnitBPE(V, merges, counts), seqs, final.tolist()


def test_encode_many_of_the_corpus_is_the_trainers_final_buffer(learned):
    bpe, seqs, final = learned
    got = bpe.encode_many(seqs, device=DEV)
    assert got == ref.split(final)
    assert got == [bpe.encode(s) for s in seqs]


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, ENCODE_SHORT - 1, ENCODE_SHORT, ENCODE_SHORT + 1, _lib.BPE_ENCODE_MAX_LEN])
def test_encode_lengths(learned, n):
    bpe, _, _ = learned
    seqs = [ref.zipf_markov(n, 12, 50 + k) for k in range(3)] + [[3] * n, ([5] * 7 + [1])[: max(n, 0)] * (n // 8 + 1)]
    seqs = [s[:n] for s in seqs] + [[2, 2, 2]]          # the short one rides along: the launch's form follows the longest
    got = bpe.encode_many(seqs, device=DEV)
    for s, g in zip(seqs, got):
        assert g == ref.encode(s, bpe.merges, 12) == bpe.encode(s)
        assert bpe.decode(g) == s


def test_encode_refuses_one_more_than_the_limit(learned):
    bpe, _, _ = learned
    n = _lib.BPE_ENCODE_MAX_LEN + 1
    with pytest.raises(ValueError, match=str(_lib.BPE_ENCODE_MAX_LEN)):
        bpe.encode_many([[0] * n], device=DEV)
    tokens = torch.zeros(n, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="code 2"):
        ops.bpe_encode(tokens, torch.zeros(1, dtype=torch.int64, device=DEV), torch.full((1,), n, dtype=torch.int32, device=DEV), n,
                       bpe.rank_table(DEV), bpe.vocab_size, bpe.n_base, torch.empty_like(tokens), torch.empty(1, dtype=torch.int32, device=DEV))


def test_encode_no_merge_present_every_merge_present_and_runs(learned):
    bpe, _, _ = learned
    unmerged = [a for a in range(12) if (a, a) not in bpe.merges]
    nothing = [unmerged[0]] * 50 if unmerged else []
    assert nothing and bpe.encode(nothing) == nothing
    everything = [v for r in range(bpe.n_merges - 1, -1, -1) for v in bpe.decode([bpe.n_base + r]) + [S]]
    runs = [[a] * k for a in range(12) for k in (2, 3, 31, 32, 257)]
    outside = [[0, 1, 2, 52, 0, 1, 2, -7, 0, 1, 2, S, 0, 1, 2, 2 ** 31 - 1, 0, 1]]       # ids outside [0, V) stay and divide
    seqs = [nothing, everything] + runs + outside
    got = bpe.encode_many(seqs, device=DEV)
    assert got[0] == nothing and len(set(got[1]) - {S}) > bpe.n_merges // 2
    for s, g in zip(seqs, got):
        assert g == bpe.encode(s) == ref.encode(s, bpe.merges, 12), s[:20]


def test_a_bad_span_among_good_ones(learned):
    bpe, seqs, _ = learned
    good = [seqs[7], seqs[8], seqs[4]]
    flat = [v for s in good for v in s]
    n = len(flat)
    starts = [0, len(good[0]), -1, len(good[0]) + len(good[1]), n - 5, 0, 0]
    lens = [len(good[0]), len(good[1]), 4, len(good[2]), 6, -1, 901]            # 2: negative start, 4: past the end, 5: negative, 6: above max_len
    tokens = torch.tensor(flat, dtype=torch.int32, device=DEV)
    out, out_len = torch.full_like(tokens, -9), torch.full((len(lens),), -9, dtype=torch.int32, device=DEV)
    ops.bpe_encode(tokens, torch.tensor(starts, dtype=torch.int64, device=DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), 900,
                   bpe.rank_table(DEV), bpe.vocab_size, bpe.n_base, out, out_len)
    out, out_len = out.cpu().tolist(), out_len.cpu().tolist()
    assert [out_len[k] for k in (2, 4, 5, 6)] == [-1] * 4
    for k, s in zip((0, 1, 3), good):
        assert out[starts[k]:starts[k] + out_len[k]] == bpe.encode(s)


def test_the_script_trains_encodes_and_refuses_to_overwrite(tmp_path, capsys):
    import importlib.util
    import json
    import os
    from conftest import PKG
    spec = importlib.util.spec_from_file_location("unit_bpe_script", os.path.join(PKG, "scripts", "unit_bpe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seqs = [ref.zipf_markov(n, 12, seed) for seed, n in enumerate([700, 900, 0, 1500, 800, 5000])]
    data = tmp_path / "units.jsonl"
    data.write_text("\n".join(json.dumps({"id": i, "units": [v for u in s for v in (u, u)]}) for i, s in enumerate(seqs)) + "\n")   # runs: --dedup undoes them
    dedup = [[k for i, k in enumerate(s) if i == 0 or s[i - 1] != k] for s in seqs]
    merges = tmp_path / "merges.json"
    argv = ["train", str(data), "--column", "units", "--n-base", "12", "--n-merges", "30", "--output", str(merges), "--device", DEV]
    got = mod.main(mod.parse_args(argv + ["--max-ids", str(sum(map(len, dedup[:4])) + 5)]))
    assert got["left_out"] == 2 and "left out 2 sequences" in capsys.readouterr().out
    bpe = ub.UnitBPE.load(merges)
    want = ref.train(ref.flatten(dedup[:4]), 12, 30)
    assert bpe.merges == want[0] and bpe.counts == want[1] and bpe.corpus["sequences"] == 4
    with pytest.raises(FileExistsError, match="not overwritten"):
        mod.main(mod.parse_args(argv))
    out = tmp_path / "encoded.jsonl"
    mod.main(mod.parse_args(["encode", str(data), str(merges), "--column", "units", "--output", str(out), "--device", DEV]))
    lines = [json.loads(l) for l in out.read_text().splitlines()]
    assert [l["units"] for l in lines] == [ref.encode(s, bpe.merges, 12) for s in dedup] and [l["id"] for l in lines] == list(range(6))   # 5000 ids: the host encoder
    stats = mod.main(mod.parse_args(["stats", str(data), str(merges), "--column", "units", "--device", DEV]))
    assert stats["ids_before"] == sum(map(len, dedup)) and stats["ids_after"] == sum(len(l["units"]) for l in lines)
