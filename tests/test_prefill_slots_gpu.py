"""``HipLlamaDecoder.prefill(..., slots=[...])`` on the fp32 ``tiny`` model, with both kinds of cache: a prompt enters a cache that holds live
sequences.  Slots 0 and 1 are filled and run three decode steps; slot 1 is poisoned beyond the new prompt's length; then ``prefill([C],
slots=[1])``: slot 0's bytes and length are unchanged, slot 1's first ``len(C)`` positions and the logits are bit-equal to ``prefill([C])``
into a fresh cache, and a following ``decode_step`` with rows of mixed age gives every row the bits of its own sequence run alone.  Packed
and prompt-by-prompt admission of several prompts into scattered slots; the refusals."""
import pytest
import torch

from oracle import hf_crosscheck as hx

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
A, B, C, D = [5, 17, 300, 2, 9, 41, 8], [400, 3, 77, 12], [9, 250, 31, 6, 100], [33, 1, 480, 22, 7, 7, 19, 250, 3]
KINDS = pytest.mark.parametrize("kind", (None, "fp8"), ids=("auto", "fp8"))
CAP, STEPS = 24, 3


@pytest.fixture(scope="module")
def model():
    from ssi.model import HipLlamaDecoder
    params, _, _, seed = hx.CASES["tiny"]
    m = HipLlamaDecoder(**params, dtype=torch.float32, device=DEV)
    m.load_state_dict(hx.seeded_state_dict(params, seed))
    m.eval()
    return m


def _parts(cache):
    return [t for t in (cache.k, cache.v, cache.k_exp, cache.v_exp) if t is not None]


def _slot(cache, s, upto=None):
    """The bytes of slot ``s`` (its first ``upto`` positions) in every tensor of the cache."""
    return [t[:, s, :upto].clone().view(torch.uint8) for t in _parts(cache)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _steps(model, cache, first, n, slots):
    """``n`` greedy decode steps on the rows of ``slots`` (-1: an inert row) from the logits ``first``; the logits of every step as int32 bits."""
    slot = torch.tensor(slots, dtype=torch.int32, device=DEV)
    logits, got = first, []
    for _ in range(n):
        tok = torch.where(slot >= 0, logits[:, :model.vocab_size].argmax(-1), torch.zeros_like(slot, dtype=torch.int64))
        logits = model.decode_step(cache, tok, slot)
        got.append(logits.view(torch.int32).clone())
    return got


def _alone(model, kind, prompt, n, row):
    """A sequence run alone: its prompt into a fresh one-slot cache, then ``n`` greedy steps as row ``row`` of two, the other row inert (no
    other sequence, the launch shapes of the step under test).  Returns the prefill's logits, the slot's bytes after it, the steps' logits."""
    cache = model.new_kv_cache(1, CAP, dtype=kind)
    first = model.prefill(cache, [prompt], max_new_tokens=CAP - len(prompt))
    filled = _slot(cache, 0, len(prompt))
    two = first.new_zeros((2, first.shape[1]))
    two[row] = first[0]
    return first, filled, [g[row] for g in _steps(model, cache, two, n, [0, -1] if row == 0 else [-1, 0])]


@KINDS
def test_a_prompt_enters_a_cache_that_holds_live_sequences(model, kind):
    cache = model.new_kv_cache(3, CAP, dtype=kind)
    first = model.prefill(cache, [A, B], max_new_tokens=CAP - len(A), separate=True)
    mixed = _steps(model, cache, first, STEPS, [0, 1])
    assert cache.lengths.tolist() == [len(A) + STEPS, len(B) + STEPS, 0]
    for t in _parts(cache):                               # poison slot 1 beyond the new prompt's length, and the empty slot 2
        if t.dtype == torch.uint8:                        # (the e4m3 NaN code; for the exponents a byte no store has written)
            t[:, 1, len(C):] = 0x7F if t is cache.k or t is cache.v else 0xFE
            t[:, 2] = 0x7F if t is cache.k or t is cache.v else 0xFE
        else:
            t[:, 1, len(C):] = float("nan")
            t[:, 2] = float("nan")
    slot0, slot2 = _slot(cache, 0), _slot(cache, 2)
    a_first, _, a_steps = _alone(model, kind, A, 2 * STEPS, 0)
    c_first, c_filled, c_steps = _alone(model, kind, C, STEPS, 1)
    assert torch.equal(a_first.view(torch.int32)[0], first.view(torch.int32)[0])
    assert all(torch.equal(mixed[k][0], a_steps[k]) for k in range(STEPS))                        # A beside B was A alone so far
    got_first = model.prefill(cache, [C], max_new_tokens=CAP - len(C), slots=[1])
    assert cache.lengths.tolist() == [len(A) + STEPS, len(C), 0] and int(cache.errors) == 0
    assert _same(_slot(cache, 0), slot0) and _same(_slot(cache, 2), slot2)                        # the other slots: byte for byte
    assert _same(_slot(cache, 1, len(C)), c_filled)                                               # the slot: prefill([C]) into a fresh cache
    assert torch.equal(got_first.view(torch.int32), c_first.view(torch.int32))                    # the logits: bit for bit
    # rows of mixed age in one step: A is STEPS tokens in, C at its first; each has the bits of its own sequence run alone
    logits = torch.stack([mixed[STEPS - 1][0].view(torch.float32), got_first[0]])
    got = _steps(model, cache, logits, STEPS, [0, 1])
    for k in range(STEPS):
        assert torch.equal(got[k][0], a_steps[STEPS + k]) and torch.equal(got[k][1], c_steps[k]), k
    assert cache.lengths.tolist() == [len(A) + 2 * STEPS, len(C) + STEPS, 0] and int(cache.errors) == 0
    assert _same(_slot(cache, 2), slot2)                  # (NaN beyond a slot's length is never read: every logit above is a number)
    assert all(bool(torch.isfinite(g.view(torch.float32)).all()) for g in got)


@KINDS
@pytest.mark.parametrize("separate", (False, True), ids=("packed", "separate"))
def test_several_prompts_into_scattered_slots_come_back_in_prompt_order(model, kind, separate):
    cache = model.new_kv_cache(5, CAP, dtype=kind)
    model.prefill(cache, [A, B, A, B, A], max_new_tokens=2)
    keep1, keep3 = _slot(cache, 1), _slot(cache, 3)
    got = model.prefill(cache, [C, D, B], max_new_tokens=2, slots=[4, 0, 2], separate=separate)
    want_cache = model.new_kv_cache(3, CAP, dtype=kind)
    want = model.prefill(want_cache, [C, D, B], max_new_tokens=2, separate=separate)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))                           # the same forward: only the destinations differ
    assert cache.lengths.tolist() == [len(D), len(B), len(B), len(B), len(C)] and int(cache.errors) == 0
    for i, (s, p) in enumerate(((4, C), (0, D), (2, B))):
        assert _same(_slot(cache, s, len(p)), _slot(want_cache, i, len(p))), s
    assert _same(_slot(cache, 1), keep1) and _same(_slot(cache, 3), keep3)


def test_refusals_come_before_any_launch(model):
    cache = model.new_kv_cache(3, 16)
    model.prefill(cache, [A, B], max_new_tokens=2)
    before, lengths = _slot(cache, 0) + _slot(cache, 1) + _slot(cache, 2), cache.lengths.tolist()
    for slots, match in (([0, 3], "outside"), ([-1, 2], "outside"), ([1, 1], "twice"), ([0], "slots for"), ([0, 1, 2], "slots for")):
        with pytest.raises(ValueError, match=match):
            model.prefill(cache, [C, D], slots=slots)
    with pytest.raises(ValueError, match="cap"):
        model.prefill(cache, [C], max_new_tokens=12, slots=[2])                                 # 5 + 12 > 16
    with pytest.raises(ValueError, match="empty"):
        model.prefill(cache, [[]], slots=[2])
    assert _same(_slot(cache, 0) + _slot(cache, 1) + _slot(cache, 2), before) and cache.lengths.tolist() == lengths and int(cache.errors) == 0
