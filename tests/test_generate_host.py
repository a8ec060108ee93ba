"""CPU: the host side of generation — the ABI names the two entries, prompts are grouped and ordered as documented, the JSONL lines have
the shape the reference's ``wer.py`` reads, the script refuses anything but greedy decoding, and the wrappers refuse CPU tensors."""
import importlib.util
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speech-integration_amd")


def test_the_abi_names_the_two_entries():
    from ssi import _lib, ops
    header = open(os.path.join(ROOT, "include", "ssi_hip.h")).read()
    assert int(re.search(r"#define SSI_ABI_VERSION (\d+)", header).group(1)) >= 18 and _lib.ABI_VERSION >= 18
    for name, wrapper in (("ssi_kv_store", "kv_store"), ("ssi_attn_decode", "attn_decode")):
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.PROTOTYPES and wrapper in ops.__all__ and callable(getattr(ops, wrapper))
    # the argument counts of the header and of the ctypes table agree (test_abi.py compares every entry; this pins the two new ones)
    for name in ("ssi_kv_store", "ssi_attn_decode"):
        args = re.search(rf"\bint {name}\((.*?)\);", header, re.S).group(1)
        assert len(args.split(",")) == len(_lib.PROTOTYPES[name][1]), name


def test_prompts_are_sorted_by_length_and_cut_into_static_groups():
    from ssi.generate import plan_groups
    lens = [7, 3, 9, 3, 1, 12, 7]
    assert plan_groups(lens, 3) == [[4, 1, 3], [0, 6, 2], [5]]            # rising length, ties by index
    assert plan_groups(lens, 256) == [[4, 1, 3, 0, 6, 2, 5]]
    assert plan_groups([], 4) == []
    groups = plan_groups(lens, 2)
    assert sorted(i for g in groups for i in g) == list(range(len(lens))) and all(len(g) <= 2 for g in groups)
    with pytest.raises(ValueError):
        plan_groups(lens, 0)


class _Tok:
    special_tokens = {"<|end_of_text|>": 901, "<|eom_id|>": 908, "<|eot_id|>": 909}
    eos_id, eom_id, eot_id, pad_id = 901, 908, 909, 904

    def encode(self, text, add_bos=True, add_eos=True):
        return ([900] if add_bos else []) + [ord(c) for c in text] + ([901] if add_eos else [])

    def decode(self, ids, truncate_at_eos=True, skip_special_tokens=True):
        assert truncate_at_eos is True and skip_special_tokens is True   # what conf/generate.yaml's tokenizer_decoding says
        return "".join(chr(t) for t in ids if t < 900)


def test_jsonl_lines_have_the_shape_the_wer_script_reads(tmp_path, monkeypatch):
    from ssi import generate as G
    seen = {}

    def fake_generate(model, prompts, **kw):
        seen.update(kw, prompts=prompts)
        return [G.Generation(token_ids=[ord("a") + i, 909] if i != 1 else [ord("z")] * 3, finish_reason="stop" if i != 1 else "length",
                             stop_reason=909 if i != 1 else None, cumulative_logprob=-1.5 * (i + 1), prompt_len=len(p))
                for i, p in enumerate(prompts)]

    monkeypatch.setattr(G, "generate", fake_generate)
    src = tmp_path / "prompts.jsonl"
    src.write_text("\n".join(json.dumps(x) for x in ({"id": "u3", "prompt_tokens": [900, 65, 66]}, {"id": "u1", "prompt": "hi"},
                                                    {"id": "u2", "prompt_tokens": [900]})) + "\n")
    out = tmp_path / "generations.jsonl"
    summary = G.generate_file(object(), _Tok(), str(src), str(out), max_new_tokens=5,
                              tokenizer_decoding={"truncate_at_eos": True, "skip_special_tokens": True}, batch_size=2)
    assert summary == {"items": 3, "generated_tokens": 7, "stopped": 2}
    assert seen["stop_token_ids"] == [908, 909, 901] and seen["pad_id"] == 904 and seen["max_new_tokens"] == 5 and seen["batch_size"] == 2
    assert seen["prompts"] == [[900, 65, 66], [900, ord("h"), ord("i")], [900]]
    lines = [json.loads(l) for l in out.read_text().splitlines()]
    assert [l["id"] for l in lines] == ["u3", "u1", "u2"]                  # input order
    for l in lines:
        assert set(l) == {"id", "prompt_token_ids", "prompt", "outputs"} and len(l["outputs"]) == 1
        assert set(l["outputs"][0]) == {"index", "text", "token_ids", "cumulative_logprob", "finish_reason", "stop_reason", "stop_reason_text"}
        assert l["outputs"][0]["index"] == 0
    assert lines[0]["prompt"] == "AB" and lines[0]["outputs"][0]["text"] == "a" and lines[0]["outputs"][0]["stop_reason_text"] == "<|eot_id|>"
    assert lines[1]["outputs"][0] == {"index": 0, "text": "zzz", "token_ids": [122] * 3, "cumulative_logprob": -3.0, "finish_reason": "length",
                                      "stop_reason": None, "stop_reason_text": None}
    # what the reference's reader does with the file
    assert [l["outputs"][0]["text"] for l in lines] == ["a", "zzz", "c"]
    bad = tmp_path / "bad.jsonl"
    bad.write_text(json.dumps({"id": 1, "prompt": "x", "prompt_tokens": [1]}) + "\n")
    with pytest.raises(ValueError, match="exactly one"):
        G.generate_file(object(), _Tok(), str(bad), str(out), max_new_tokens=5)


def test_only_greedy_sampling_params_pass():
    from ssi.config import compose
    from ssi.generate import check_greedy
    cfg = compose(os.path.join(PKG, "conf"), "generate", ["speech.n_dsus=5000", "gen.output_dir=out"])
    check_greedy(cfg.sampling_params)                                      # the committed defaults are greedy
    assert cfg.gen.output_filename == "generations.jsonl" and cfg.gen.split == "dev" and cfg.gen.input is None
    assert cfg.sampling_params.max_tokens == 256 and cfg.sampling_params.stop_token_ids is None
    assert {k: cfg.tokenizer_decoding[k] for k in cfg.tokenizer_decoding} == {"truncate_at_eos": True, "skip_special_tokens": True}
    for key, value in (("temperature", 0.7), ("top_p", 0.95), ("top_k", 40), ("presence_penalty", 0.1), ("frequency_penalty", 0.1),
                       ("repetition_penalty", 1.1), ("n", 2), ("best_of", 4)):
        with pytest.raises(NotImplementedError, match=key):
            check_greedy({"n": 1, "temperature": 0.0, **{key: value}})
    check_greedy({"temperature": 0, "top_p": 1.0, "max_tokens": 17, "stop_token_ids": [5]})


def test_the_script_refuses_before_it_loads_anything():
    from ssi.config import compose
    spec = importlib.util.spec_from_file_location("generate_script", os.path.join(PKG, "scripts", "generate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cfg = compose(os.path.join(PKG, "conf"), "generate", ["speech.n_dsus=5000", "gen.output_dir=/nonexistent/out", "sampling_params.temperature=0.8"])
    with pytest.raises(NotImplementedError, match="temperature"):
        mod.main(cfg)
    assert not os.path.exists("/nonexistent/out")


def test_the_wrappers_refuse_cpu_tensors():
    from ssi import _lib, ops
    H, KV, hd = 4, 1, 16
    qkv = torch.zeros(3, (H + 2 * KV) * hd)
    cache = torch.zeros(2, 8, KV * hd)
    i32, i64 = torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(_lib.HipLibraryError, match="GPU"):
        ops.kv_store(qkv, i64, cache, cache.clone(), H, KV, hd)
    with pytest.raises(_lib.HipLibraryError, match="GPU"):
        ops.attn_decode(qkv, cache, cache.clone(), i32, i32, torch.zeros(3, H * hd), None, H, KV, hd)
