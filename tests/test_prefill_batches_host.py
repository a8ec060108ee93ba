"""CPU: the host packing of ``HipLlamaDecoder.prefill`` (``ssi.score.prefill_batches``) and the placement loop it shares with
``scoring_batches``.

``tests/golden/scoring_batches_layout.npz`` holds what ``scoring_batches`` yielded before the two functions shared that loop, for the inputs of
tests/test_seq_score_host.py (``rows2048``) and for a small case with the dense mask, a context beyond a sequence's end and an empty sequence
(``rows64_mask``); every array as int32 (bool for the mask), keys ``case/batch/key``."""
import os

import numpy as np
import pytest
import torch

LENS, CAP = [5, 17, 1], 40
SCORING_CASES = {
    "rows2048": dict(lengths=[5, 2048, 1, 700, 700, 649, 2], score_from=[1, 1, 1, 300, 1, 649, 5], row_len=2048, rows_per_batch=2, pad_id=7,
                     dense_mask=False),
    "rows64_mask": dict(lengths=[5, 64, 1, 20, 20, 23, 2, 40, 0], score_from=[1, 30, 1, 20, 7, 1, 9, 39, 1], row_len=64, rows_per_batch=2, pad_id=3,
                        dense_mask=True),
}


def _prompts(lens=LENS):
    return [torch.arange(n) + 1000 * (i + 1) for i, n in enumerate(lens)]


def test_a_prompt_longer_than_the_row_raises_as_pack_for_scoring_does():
    from ssi.score import pack_for_scoring, prefill_batches
    with pytest.raises(ValueError, match=r"sequence 1 has 17 tokens, more than row_len = 16"):
        pack_for_scoring(LENS, 16)
    with pytest.raises(ValueError, match=r"sequence 1 has 17 tokens, more than row_len = 16"):
        list(prefill_batches(_prompts(), CAP, 16, 8))


def test_tokens_positions_destinations_and_last_tokens_of_the_hand_case():
    from ssi.score import pack_for_scoring, prefill_batches
    seqs, rows = _prompts(), pack_for_scoring(LENS, 24)
    assert rows == [[1, 0, 2]]                                   # by falling length: 17 + 5 + 1 = 23 of 24 positions, a tail of one
    (tokens, input_pos, dest, last_at, last_of), = prefill_batches(seqs, CAP, 24, 8)
    assert tokens.shape == input_pos.shape == dest.shape == (1, 24) and all(t.dtype == torch.int64 for t in (tokens, input_pos, dest, last_at, last_of))
    at = 0
    for i in rows[0]:
        n = LENS[i]
        assert torch.equal(tokens[0, at:at + n], seqs[i])
        assert torch.equal(input_pos[0, at:at + n], torch.arange(n))          # restarts with every prompt
        for j in range(n):
            assert int(dest[0, at + j]) == i * CAP + j
        at += n
    assert at == 23 and tokens[0, 23:].tolist() == [0]
    assert input_pos[0, 23:].tolist() == [0] and dest[0, 23:].tolist() == [-1]  # the tail: a document of its own, stored nowhere
    assert last_of.tolist() == [1, 0, 2] and last_at.tolist() == [16, 21, 22]
    assert [int(tokens.reshape(-1)[p]) for p in last_at] == [int(seqs[i][-1]) for i in last_of.tolist()]


@pytest.mark.parametrize("lens,row_len,rows_per_batch", [(LENS, 24, 8), ([5, 17, 1, 9, 16, 3, 3], 17, 2), ([4, 4, 4], 4, 1)])
def test_tokens_and_positions_are_those_of_scoring_batches(lens, row_len, rows_per_batch):
    from ssi.score import pack_for_scoring, prefill_batches, scoring_batches
    seqs, rows = _prompts(lens), pack_for_scoring(lens, row_len)
    scoring = list(scoring_batches(seqs, [1] * len(lens), rows, row_len, rows_per_batch, pad_id=0))
    prefill = list(prefill_batches(seqs, CAP, row_len, rows_per_batch))
    assert len(scoring) == len(prefill) == -(-len(rows) // rows_per_batch)
    for s, (tokens, input_pos, dest, last_at, last_of) in zip(scoring, prefill):
        assert torch.equal(tokens, s["tokens"]) and torch.equal(input_pos, s["input_pos"]) and last_of.tolist() == s["seq_index"]
        assert torch.equal(dest >= 0, s["tokens"] != 0)                          # (no token of these prompts is 0: stored = not the tail)


def test_one_row_per_batch_covers_every_prompt_once():
    from ssi.score import pack_for_scoring, prefill_batches
    lens = [10, 9, 8, 3, 2]
    seqs = _prompts(lens)
    assert pack_for_scoring(lens, 12) == [[0, 4], [1, 3], [2]]
    batches = list(prefill_batches(seqs, CAP, 12, 1))
    assert len(batches) == 3 and all(b[0].shape == (1, 12) for b in batches)
    assert sorted(i for b in batches for i in b[4].tolist()) == [0, 1, 2, 3, 4]
    stored = torch.cat([b[2].reshape(-1) for b in batches])
    assert sorted(stored[stored >= 0].tolist()) == sorted(i * CAP + j for i, n in enumerate(lens) for j in range(n))
    for tokens, _, _, last_at, last_of in batches:
        assert [int(tokens.reshape(-1)[p]) for p in last_at] == [int(seqs[i][-1]) for i in last_of.tolist()]


@pytest.mark.parametrize("case", sorted(SCORING_CASES))
def test_scoring_batches_yields_what_it_yielded_before(case, golden_dir):
    from ssi.score import pack_for_scoring, scoring_batches
    c, want = SCORING_CASES[case], np.load(os.path.join(golden_dir, "scoring_batches_layout.npz"))
    seqs = _prompts(c["lengths"])
    rows = pack_for_scoring(c["lengths"], c["row_len"])
    got = list(scoring_batches(seqs, c["score_from"], rows, c["row_len"], c["rows_per_batch"], c["pad_id"], dense_mask=c["dense_mask"], token_logprobs=True))
    assert len(got) == len({k.split("/")[1] for k in want.files if k.startswith(case + "/")})
    for k, batch in enumerate(got):
        assert set(batch) == {key.split("/")[2] for key in want.files if key.startswith(f"{case}/{k}/")}
        for key, v in batch.items():
            ref = want[f"{case}/{k}/{key}"]
            if key == "seq_index":
                assert v == ref.tolist()
            else:
                assert v.dtype == (torch.bool if key == "mask" else torch.int64) and tuple(v.shape) == ref.shape and np.array_equal(v.numpy(), ref), key
