"""CPU: the host side of beam search — the ABI names the two entries with matching argument counts, the wrappers refuse CPU tensors, the
refusals of ``beam_search`` come before anything is launched (a model stub that fails on any use), the rules said again in plain Python
(tests/beam_ref.py) on hand-made log-probability tables, the JSONL record of ``generate_file`` with ``n_best = 2``, and the configuration."""
import json
import math
import os
import re

import pytest
import torch

import beam_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speech-integration_amd")


def test_the_abi_names_the_two_entries():
    from ssi import _lib, ops
    header = open(os.path.join(ROOT, "include", "ssi_hip.h")).read()
    assert int(re.search(r"#define SSI_ABI_VERSION (\d+)", header).group(1)) >= 20 and _lib.ABI_VERSION >= 20
    assert re.search(r"\* 20: \+ ssi_attn_decode_beam, ssi_topk_logprob", header) and re.search(r"\* 19: \+ ssi_decode_select", header)
    for name, wrapper, n_args in (("ssi_attn_decode_beam", "attn_decode_beam", 24), ("ssi_topk_logprob", "topk_logprob", 12)):
        assert name in _lib.PROTOTYPES and wrapper in ops.__all__ and callable(getattr(ops, wrapper))
        args = re.search(rf"\bint {name}\((.*?)\);", header, re.S).group(1)
        assert len(args.split(",")) == len(_lib.PROTOTYPES[name][1]) == n_args, name


def test_the_wrappers_refuse_cpu_tensors():
    from ssi import _lib, ops
    H, KV, hd = 4, 1, 16
    qkv = torch.zeros(3, (H + 2 * KV) * hd)
    cache = torch.zeros(2, 8, KV * hd)
    i32 = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(_lib.HipLibraryError, match="GPU"):
        ops.attn_decode_beam(qkv, cache, cache.clone(), cache.clone(), cache.clone(), i32, i32, i32, torch.zeros(3, 8, dtype=torch.int32),
                             torch.zeros(3, H * hd), None, H, KV, hd)
    with pytest.raises(_lib.HipLibraryError, match="GPU"):
        ops.topk_logprob(torch.zeros(3, 32), 30, 4, torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, 4))


class _Stub:
    """A model on which any use beyond the host checks fails: no ``prefill``, no cache, no ``eval``."""
    vocab_size, training = 100, False
    device = torch.device("cpu")
    checked = 0

    def check_generation_lengths(self, lens, max_new_tokens, n_slots, cap):
        type(self).checked += 1
        if any(n < 1 for n in lens):
            raise ValueError("prompt is empty")
        if max(lens) + max_new_tokens > 64:
            raise ValueError("exceeds max_seq_len")

    def __getattr__(self, name):
        raise AssertionError(f"the model was used ({name}) before the refusal")


def test_the_refusals_come_before_any_launch():
    from ssi.generate import beam_search
    ok = dict(beam_width=3, max_new_tokens=4, stop_token_ids=[7], pad_id=0)
    for bad, match in ((dict(beam_width=0), "beam_width"), (dict(beam_width=9), "beam_width"), (dict(beam_width=2.0), "beam_width"),
                       (dict(beam_width=True), "beam_width"), (dict(n_best=0), "n_best"), (dict(n_best=4), "n_best"),
                       (dict(length_penalty=-0.5), "length_penalty"), (dict(length_penalty=math.inf), "length_penalty"),
                       (dict(length_penalty=math.nan), "length_penalty"), (dict(length_penalty="1"), "length_penalty"),
                       (dict(min_new_tokens=-1), "min_new_tokens"), (dict(allowed_token_ids=[]), "allows no token"),
                       (dict(allowed_token_ids=[100]), "vocabulary"), (dict(stop_token_ids=[100]), "vocabulary"),
                       (dict(allowed_token_ids=[7], min_new_tokens=1), "besides the stop tokens"),
                       (dict(allowed_token_ids=[7]), "besides the stop tokens"), (dict(max_new_tokens=0), "max_new_tokens"),
                       (dict(batch_size=2), "batch_size")):
        with pytest.raises(ValueError, match=match):
            beam_search(_Stub(), [[1, 2], [3]], **{**ok, **bad})
    before = _Stub.checked
    with pytest.raises(ValueError, match="empty"):
        beam_search(_Stub(), [[1, 2], []], **ok)
    with pytest.raises(ValueError, match="max_seq_len"):
        beam_search(_Stub(), [[1] * 61], **ok)
    assert _Stub.checked == before + 2                                        # the lengths are the last host check
    assert beam_search(_Stub(), [], **ok) == []


# ---- the rules on hand-made tables ---------------------------------------------------------------------------------------------
def table(rows):
    """``step_logprobs`` from {generated tokens (tuple): log-probabilities}; the prompt is one token."""
    return lambda tokens: rows[tuple(tokens[1:])]


NEG = -math.inf


def test_tie_order_is_score_then_beam_then_token():
    # vocabulary of 4, no stop token: at step 0 tokens 1 and 3 tie, then 2; at step 1 every beam offers the same values
    step0 = [NEG, -1.0, -2.0, -1.0]
    same = [-1.0, -1.0, -3.0, -3.0]
    rows = {(): step0, (1,): same, (3,): same, (2,): [-0.5, NEG, NEG, NEG]}
    out = br.beam_search_ref(table(rows), [9], beam_width=3, max_new_tokens=2, stop_token_ids=[], n_best=3, length_penalty=0.0)
    # beams after step 0: (1), (3), (2) with -1, -1, -2.  Step 1: -2 from (1)+0, (1)+1, (3)+0, (3)+1; -2.5 from (2)+0 — beam before token
    assert [h.token_ids for h in out] == [[1, 0], [1, 1], [3, 0]]
    assert [h.score for h in out] == [-2.0, -2.0, -2.0] and all(h.finish_reason == "length" and h.stop_reason is None for h in out)
    assert br.beam_search_ref(table(rows), [9], beam_width=3, max_new_tokens=2, stop_token_ids=[], n_best=1)[0].score == -1.0   # / 2 ** 1


def test_more_stop_candidates_than_the_width_fill_the_pool_in_one_step():
    # tokens 0..2 are stop tokens and lead the first step: all W = 2 first entries are finishers, the pool is full after step 0
    rows = {(): [-0.5, -1.5, -1.0, -4.0, -5.0]}
    tr = {}
    out = br.beam_search_ref(table(rows), [9], beam_width=2, max_new_tokens=5, stop_token_ids=[0, 1, 2], n_best=2, trace=tr)
    assert [(h.token_ids, h.finish_reason, h.stop_reason, h.score) for h in out] == [([0], "stop", 0, -0.5), ([2], "stop", 2, -1.0)]
    assert tr["done_at"] == 0
    # with min_new_tokens = 1 the stop tokens wait a step: the continuations 3 and 4 go on, and stop there
    rows.update({(3,): [-0.1, NEG, NEG, -3.0, NEG], (4,): [-0.2, NEG, NEG, NEG, -3.0]})
    out = br.beam_search_ref(table(rows), [9], beam_width=2, max_new_tokens=5, stop_token_ids=[0, 1, 2], n_best=2, min_new_tokens=1, trace=tr)
    assert [(h.token_ids, h.stop_reason) for h in out] == [([3, 0], 0), ([4, 0], 0)] and tr["done_at"] == 1
    assert out[0].cumulative_logprob == -4.1 and out[0].score == -4.1 / 2


def test_a_finisher_behind_the_width_does_not_join_and_length_ends_the_rest():
    # W = 2: the stop token is third at step 0 (does not join), first at step 1 for beam 0
    rows = {(): [-3.0, -1.0, -2.0], (1,): [-0.1, -5.0, -6.0], (2,): [-9.0, -0.2, -0.3]}
    rows.update({(2, 1): [-9.0, -0.5, -0.6], (2, 2): [-9.0, -0.7, -0.8]})
    out = br.beam_search_ref(table(rows), [9], beam_width=2, max_new_tokens=3, stop_token_ids=[0], n_best=2, length_penalty=1.0)
    # step 1: merged = (1,0) -1.1 [stop], (2,1) -2.2, (2,2) -2.3: one finisher joins; beams (2,1), (2,2).  Step 2: no stop in reach, length.
    assert [(h.token_ids, h.finish_reason) for h in out] == [([1, 0], "stop"), ([2, 1, 1], "length")]
    assert out[0].score == -1.1 / 2 and abs(out[1].score - (-2.7 / 3)) < 1e-12
    allowed = br.beam_search_ref(table(rows), [9], beam_width=2, max_new_tokens=1, stop_token_ids=[0], n_best=2, allowed={2})
    # one allowed continuation: one beam; with it alone ahead, the stop token is second of W = 2 and joins
    assert [(h.token_ids, h.finish_reason, h.score) for h in allowed] == [([2], "length", -2.0), ([0], "stop", -3.0)]


# ---- the file layer ------------------------------------------------------------------------------------------------------------
class _Tok:
    special_tokens = {"<|eot_id|>": 909}
    eos_id, eom_id, eot_id, pad_id = 901, 908, 909, 904

    def decode(self, ids, truncate_at_eos=True, skip_special_tokens=True):
        return "".join(chr(t) for t in ids if t < 900)


def test_generate_file_writes_n_best_entries_per_prompt(tmp_path, monkeypatch):
    from ssi import generate as G
    seen = {}

    def fake_beam_search(model, prompts, **kw):
        seen.update(kw)
        return [[G.Generation([ord("a") + j, 909], "stop", 909, -1.0 - j, len(p), score=-0.5 - j) for j in range(kw["n_best"])] for p in prompts]

    def no_generate(*a, **k):
        raise AssertionError("the greedy loop ran")

    monkeypatch.setattr(G, "beam_search", fake_beam_search)
    monkeypatch.setattr(G, "generate", no_generate)
    out = tmp_path / "g.jsonl"

    class M:
        device = torch.device("cpu")

    summary = G.generate_file(M(), _Tok(), None, str(out), max_new_tokens=5, prompts=[[900, 65], [900]], ids=["x", "y"], beam_width=4,
                              length_penalty=0.5, n_best=2, batch_size=8, logprobs=True, device="cpu", min_new_tokens=1)
    assert summary == {"items": 2, "generated_tokens": 8, "stopped": 4, "beam_width": 4}
    assert seen == dict(max_new_tokens=5, stop_token_ids=[908, 909, 901], beam_width=4, length_penalty=0.5, n_best=2, batch_size=8, pad_id=904,
                        min_new_tokens=1)
    lines = [json.loads(l) for l in out.read_text().splitlines()]
    assert [l["id"] for l in lines] == ["x", "y"]
    for l in lines:
        assert set(l) == {"id", "prompt_token_ids", "prompt", "outputs"} and [o["index"] for o in l["outputs"]] == [0, 1]
        assert [o["text"] for o in l["outputs"]] == ["a", "b"] and [o["cumulative_logprob"] for o in l["outputs"]] == [-1.0, -2.0]
        assert set(l["outputs"][0]) == {"index", "text", "token_ids", "cumulative_logprob", "finish_reason", "stop_reason", "stop_reason_text"}
    with pytest.raises(ValueError, match="n_best"):                           # n_best > 1 needs a beam; refused before the greedy loop
        G.generate_file(M(), _Tok(), None, str(out), max_new_tokens=5, prompts=[[900]], n_best=2)


def test_the_defaults_compose_and_stay_greedy():
    from ssi.config import compose
    from ssi.generate import check_greedy
    cfg = compose(os.path.join(PKG, "conf"), "generate", ["speech.n_dsus=5000", "gen.output_dir=out"])
    assert cfg.gen.beam_width == 1 and cfg.gen.length_penalty == 1.0 and cfg.gen.n_best == 1
    check_greedy(cfg.sampling_params)
    cfg = compose(os.path.join(PKG, "conf"), "generate", ["speech.n_dsus=5000", "gen.output_dir=out", "gen.beam_width=4", "gen.n_best=2"])
    assert cfg.gen.beam_width == 4 and cfg.gen.n_best == 2
    check_greedy(cfg.sampling_params)                                          # beam search is not a sampling parameter
    for key, value in (("n", 4), ("best_of", 4), ("temperature", 0.5), ("beam_width", 4), ("use_beam_search", True)):
        with pytest.raises(NotImplementedError, match=key):
            check_greedy({"n": 1, "temperature": 0.0, **{key: value}})
