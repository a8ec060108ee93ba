"""CPU: the host side of sampled decoding — the ABI names the entry with matching argument counts, the wrapper refuses CPU tensors, the refusals
of ``sample`` come before anything is launched (a model stub that fails on any use), ``check_sampling``, the configuration and the script's
refusals, and the JSONL record and summary of ``generate_file`` with a stubbed ``sample``."""
import importlib.util
import json
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speech-integration_amd")


def test_the_abi_names_the_entry():
    from ssi import _lib, ops
    header = open(os.path.join(ROOT, "include", "ssi_hip.h")).read()
    assert int(re.search(r"#define SSI_ABI_VERSION (\d+)", header).group(1)) >= 21 and _lib.ABI_VERSION >= 21
    assert re.search(r"\* 21: \+ ssi_decode_sample", header)
    assert "ssi_decode_sample" in _lib.PROTOTYPES and "decode_sample" in ops.__all__ and callable(ops.decode_sample)
    args = re.search(r"\bint ssi_decode_sample\((.*?)\);", header, re.S).group(1)
    assert len(args.split(",")) == len(_lib.PROTOTYPES["ssi_decode_sample"][1]) == 19
    makefile = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "decode_sample.hip" in makefile


def test_the_wrapper_refuses_cpu_tensors():
    from ssi import _lib, ops
    with pytest.raises(_lib.HipLibraryError, match="GPU"):
        ops.decode_sample(torch.zeros(3, 32), 30, torch.zeros(3, dtype=torch.int64), temperature=1.0, seed=0, step=0,
                          sequence=torch.zeros(3, dtype=torch.int32))


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
    from ssi.generate import sample
    ok = dict(n=3, temperature=0.8, seed=1, max_new_tokens=4, stop_token_ids=[7], pad_id=0)
    for bad, match in ((dict(n=0), "n = "), (dict(n=9), "n = "), (dict(n=2.0), "n = "), (dict(n=True), "n = "),
                       (dict(temperature=0), "generate"), (dict(temperature=0.0), "generate"), (dict(temperature=-1.0), "temperature"),
                       (dict(temperature=math.inf), "temperature"), (dict(temperature=math.nan), "temperature"), (dict(temperature="1"), "temperature"),
                       (dict(top_p=0.0), "top_p"), (dict(top_p=1.5), "top_p"), (dict(top_p=math.nan), "top_p"), (dict(top_k=2.5), "top_k"),
                       (dict(top_k=True), "top_k"), (dict(seed=-1), "seed"), (dict(seed=1.0), "seed"),
                       (dict(min_new_tokens=-1), "min_new_tokens"), (dict(allowed_token_ids=[]), "allows no token"),
                       (dict(allowed_token_ids=[100]), "vocabulary"), (dict(allowed_token_ids=[7], min_new_tokens=1), "besides the stop tokens"),
                       (dict(max_new_tokens=0), "max_new_tokens"), (dict(batch_size=2), "batch_size")):
        with pytest.raises(ValueError, match=match):
            sample(_Stub(), [[1, 2], [3]], **{**ok, **bad})
    with pytest.raises(TypeError):
        sample(_Stub(), [[1, 2]], beam_width=2, **ok)                         # sample with beam_width is not offered
    before = _Stub.checked
    with pytest.raises(ValueError, match="empty"):
        sample(_Stub(), [[1, 2], []], **ok)
    with pytest.raises(ValueError, match="max_seq_len"):
        sample(_Stub(), [[1] * 61], **ok)
    assert _Stub.checked == before + 2                                        # the lengths are the last host check
    assert sample(_Stub(), [], **ok) == []


def test_check_sampling():
    from ssi.generate import check_greedy, check_sampling
    assert check_sampling({"temperature": 0.8}) == {"n": 1, "temperature": 0.8, "top_k": -1, "top_p": 1.0}
    got = check_sampling({"n": 4, "temperature": 1, "top_k": 50, "top_p": 0.9, "max_tokens": 17, "stop_token_ids": [5], "min_tokens": 2,
                          "allowed_token_ids": [1, 2], "presence_penalty": 0, "frequency_penalty": 0.0, "repetition_penalty": 1})
    assert got == {"n": 4, "temperature": 1.0, "top_k": 50, "top_p": 0.9}
    for key, value in (("presence_penalty", 0.1), ("frequency_penalty", 0.1), ("repetition_penalty", 1.1), ("best_of", 4), ("use_beam_search", True),
                       ("logit_bias", {})):
        with pytest.raises(NotImplementedError, match=key):
            check_sampling({"temperature": 0.8, key: value})
    with pytest.raises(ValueError, match="greedy"):
        check_sampling({"temperature": 0.0})
    with pytest.raises(ValueError, match="greedy"):
        check_sampling({"temperature": 0})
    for bad in ({"n": 2}, {"temperature": None}, {"temperature": -0.5}, {"temperature": 0.8, "n": 0}, {"temperature": 0.8, "n": 9},
                {"temperature": 0.8, "top_p": 0}, {"temperature": 0.8, "top_p": 1.5}, {"temperature": 0.8, "top_k": 2.5},
                {"temperature": 0.8, "min_tokens": -1}):
        with pytest.raises(ValueError):
            check_sampling(bad)
    for key, value in (("temperature", 0.8), ("top_p", 0.9), ("top_k", 50), ("n", 2)):        # check_greedy is what it was
        with pytest.raises(NotImplementedError, match=key):
            check_greedy({"n": 1, "temperature": 0.0, **{key: value}})


def _script():
    spec = importlib.util.spec_from_file_location("generate_script", os.path.join(PKG, "scripts", "generate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_configuration_and_the_scripts_refusals():
    from ssi.config import compose
    from ssi.generate import check_greedy, check_sampling
    conf, base = os.path.join(PKG, "conf"), ["speech.n_dsus=5000", "gen.output_dir=/nonexistent/out"]
    cfg = compose(conf, "generate", base)
    assert cfg.gen.sample is False and cfg.gen.seed == 0
    check_greedy(cfg.sampling_params)
    mod = _script()
    # sampling keys without the switch: refused as before; the switch with the greedy temperature, with a beam, with a penalty: refused
    with pytest.raises(NotImplementedError, match="temperature"):
        mod.main(compose(conf, "generate", base + ["sampling_params.temperature=0.8"]))
    with pytest.raises(ValueError, match="greedy"):
        mod.main(compose(conf, "generate", base + ["gen.sample=true"]))
    with pytest.raises(ValueError, match="beam_width"):
        mod.main(compose(conf, "generate", base + ["gen.sample=true", "sampling_params.temperature=0.8", "gen.beam_width=4"]))
    with pytest.raises(NotImplementedError, match="repetition_penalty"):
        mod.main(compose(conf, "generate", base + ["gen.sample=true", "sampling_params.temperature=0.8", "sampling_params.repetition_penalty=1.2"]))
    with pytest.raises(ValueError, match="n = "):
        mod.main(compose(conf, "generate", base + ["gen.sample=true", "sampling_params.temperature=0.8", "sampling_params.n=9"]))
    assert not os.path.exists("/nonexistent/out")
    cfg = compose(conf, "generate", base + ["gen.sample=true", "gen.seed=7", "sampling_params.temperature=0.8", "sampling_params.top_k=50",
                                            "sampling_params.top_p=0.9", "sampling_params.n=4"])
    assert check_sampling(cfg.sampling_params) == {"n": 4, "temperature": 0.8, "top_k": 50, "top_p": 0.9} and cfg.gen.seed == 7


class _Tok:
    special_tokens = {"<|eot_id|>": 909}
    eos_id, eom_id, eot_id, pad_id = 901, 908, 909, 904

    def decode(self, ids, truncate_at_eos=True, skip_special_tokens=True):
        return "".join(chr(t) for t in ids if t < 900)


def test_generate_file_writes_n_samples_per_prompt(tmp_path, monkeypatch):
    from ssi import generate as G
    seen = {}

    def fake_sample(model, prompts, **kw):
        seen.update(kw)
        return [[G.Generation([ord("a") + j, 909], "stop", 909, -1.0 - j, len(p), n_kept_mean=10.0 + j) for j in range(kw["n"])] for p in prompts]

    def never(*a, **k):
        raise AssertionError("another loop ran")

    monkeypatch.setattr(G, "sample", fake_sample)
    monkeypatch.setattr(G, "generate", never)
    monkeypatch.setattr(G, "beam_search", never)
    out = tmp_path / "g.jsonl"

    class M:
        device = torch.device("cpu")

    summary = G.generate_file(M(), _Tok(), None, str(out), max_new_tokens=5, prompts=[[900, 65], [900]], ids=["x", "y"], sample=True, n=3,
                              temperature=0.8, top_k=50, top_p=0.9, seed=7, batch_size=8, logprobs=True, device="cpu", min_new_tokens=1)
    assert summary == {"items": 2, "generated_tokens": 12, "stopped": 6, "sampled": True, "n": 3, "kept_tokens_mean": 11.0}
    assert seen == dict(max_new_tokens=5, stop_token_ids=[908, 909, 901], n=3, temperature=0.8, top_k=50, top_p=0.9, seed=7, batch_size=8,
                        pad_id=904, min_new_tokens=1)
    lines = [json.loads(l) for l in out.read_text().splitlines()]
    assert [l["id"] for l in lines] == ["x", "y"]
    for l in lines:
        assert set(l) == {"id", "prompt_token_ids", "prompt", "outputs"} and [o["index"] for o in l["outputs"]] == [0, 1, 2]
        assert [o["text"] for o in l["outputs"]] == ["a", "b", "c"] and [o["cumulative_logprob"] for o in l["outputs"]] == [-1.0, -2.0, -3.0]
        assert set(l["outputs"][0]) == {"index", "text", "token_ids", "cumulative_logprob", "finish_reason", "stop_reason", "stop_reason_text"}
    with pytest.raises(ValueError, match="beam_width"):
        G.generate_file(M(), _Tok(), None, str(out), max_new_tokens=5, prompts=[[900]], sample=True, temperature=0.8, seed=0, beam_width=2)
    with pytest.raises(ValueError, match="sample=True"):                      # sampling arguments without the switch
        G.generate_file(M(), _Tok(), None, str(out), max_new_tokens=5, prompts=[[900]], temperature=0.8)
