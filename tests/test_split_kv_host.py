"""CPU: the host side of the split-KV decode attention — the ABI names the four entries, ``takes_split_kv``'s rule, the ``split_kv`` argument reaches
every decode step (and ``prefill``) of the groups that qualify and no other call, ``gen.split_kv`` is in the configuration with default false and is
handed on, the run summary gains ``split_kv_groups`` only with the flag, ``--split-kv`` is an option of the prompt tool, and a split wrapper refuses a
workspace of the wrong dtype or device before anything else (the library is not loaded for it)."""
import importlib.util
import json
import os
import re

import pytest
import torch

import test_small_batch_host as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speech-integration_amd")
ENTRIES = (("ssi_attn_decode_split_span", "attn_decode_split_span"), ("ssi_attn_decode_split_workspace", "attn_decode_split_workspace"),
           ("ssi_attn_decode_split", "attn_decode_split"), ("ssi_attn_decode_beam_split", "attn_decode_beam_split"))


def test_the_abi_names_the_four_entries():
    from ssi import _lib, ops
    header = open(os.path.join(ROOT, "include", "ssi_hip.h")).read()
    assert int(re.search(r"#define SSI_ABI_VERSION (\d+)", header).group(1)) >= 25 and _lib.ABI_VERSION >= 25
    for name, wrapper in ENTRIES:
        args = re.search(rf"\bint(?:64_t)? {name}\((.*?)\);", header, re.S).group(1)
        assert name in _lib.PROTOTYPES and len(args.split(",")) == len(_lib.PROTOTYPES[name][1]), name
        assert wrapper in ops.__all__ and callable(getattr(ops, wrapper))
    plain, split = _lib.PROTOTYPES["ssi_attn_decode"][1], _lib.PROTOTYPES["ssi_attn_decode_split"][1]
    assert split[:len(plain) - 2] == plain[:-2] and split[-2:] == plain[-2:] and len(split) == len(plain) + 4      # the plain arguments, then four, then dtype and stream
    plain, split = _lib.PROTOTYPES["ssi_attn_decode_beam"][1], _lib.PROTOTYPES["ssi_attn_decode_beam_split"][1]
    assert split[:len(plain) - 2] == plain[:-2] and split[-2:] == plain[-2:] and len(split) == len(plain) + 4


def test_takes_split_kv():
    from ssi.model import HipLlamaDecoder

    class M:
        takes_split_kv, split_max_rows, split_span = HipLlamaDecoder.takes_split_kv, HipLlamaDecoder.split_max_rows, HipLlamaDecoder.split_span

    m = M()
    assert M.split_span is None and isinstance(M.split_max_rows, int) and M.split_max_rows >= 0
    m.split_max_rows = 16
    assert [m.takes_split_kv(rows, True) for rows in (0, 1, 5, 16, 17, 256)] == [False, True, True, True, False, False]
    assert not any(m.takes_split_kv(rows, False) for rows in (0, 1, 16, 17))
    m.split_max_rows = 0                                                    # "no row count qualifies": the flag then changes nothing
    assert not any(m.takes_split_kv(rows, True) for rows in (0, 1, 16))
    import inspect
    for fn in (HipLlamaDecoder.decode_step, HipLlamaDecoder.decode_step_beam):
        assert inspect.signature(fn).parameters["split_kv"].default is False


class _Model(sb._Model):
    split_max_rows = 16

    def takes_split_kv(self, rows, split_kv):
        return bool(split_kv) and 1 <= rows <= self.split_max_rows


def test_the_flag_reaches_every_step_of_every_group_and_no_call_without_it():
    m = _Model()
    plain = sb._greedy(m, 5)
    assert plain and all(kw == {} for _, _, kw in plain)
    assert sb._greedy(m, 5, split_kv=False) == plain
    flagged = sb._greedy(m, 5, split_kv=True)
    assert [(n, r) for n, r, _ in flagged] == [(n, r) for n, r, _ in plain]
    assert all(kw == ({"separate": True} if name == "prefill" else {"split_kv": True}) for name, _, kw in flagged)
    both = sb._greedy(m, 5, split_kv=True, small_batch=True)
    assert all(kw == ({"separate": True} if name == "prefill" else {"small_batch": True, "split_kv": True}) for name, _, kw in both)
    # groups of 16 and 4 rows split; a group of 20 rows does not, with or without the other flag taking ITS path
    flagged = sb._greedy(m, 20, split_kv=True, batch_size=16)
    assert [(n, r, kw) for n, r, kw in flagged if n == "prefill"] == [("prefill", 16, {"separate": True}), ("prefill", 4, {"separate": True})]
    flagged = sb._greedy(m, 20, split_kv=True)
    assert [kw for n, _, kw in flagged if n == "prefill"] == [{}] and all(kw == {"split_kv": True} for n, _, kw in flagged if n == "decode_step")
    report = {}
    sb._greedy(m, 20, split_kv=True, small_batch=True, small_batch_report=report)
    assert report == {"small_batch_groups": 1}
    report = {}
    sb._greedy(m, 36, split_kv=True, batch_size=16, small_batch_report=report)
    assert report == {"split_kv_groups": 3}
    report = {}
    sb._greedy(m, 5, small_batch_report=report)
    assert report == {}


@pytest.mark.parametrize("path", ("greedy", "beam", "sample"))
def test_the_summary_key_is_there_only_with_the_flag(tmp_path, monkeypatch, path):
    from ssi import generate as G
    seen = []

    def one(p):
        return G.Generation(token_ids=[65], finish_reason="length", stop_reason=None, cumulative_logprob=-1.0, prompt_len=len(p), n_kept_mean=1.0)

    def loop(wrap):
        def run(model, prompts, **kw):
            seen.append(kw)
            for key in kw.get("small_batch_report", {}):
                kw["small_batch_report"][key] += 3
            return [wrap(one(p)) for p in prompts]
        return run

    monkeypatch.setattr(G, "generate", loop(lambda g: g))
    monkeypatch.setattr(G, "beam_search", loop(lambda g: [g]))
    monkeypatch.setattr(G, "sample", loop(lambda g: [g]))
    extra = {"greedy": {}, "beam": {"beam_width": 4}, "sample": {"sample": True, "n": 2, "temperature": 0.7, "seed": 1}}[path]
    prompts, out = [[900, 65]] * 20, tmp_path / "g.jsonl"
    run = lambda **kw: G.generate_file(_Model(), sb._Tok(), None, str(out), max_new_tokens=2, prompts=prompts, batch_size=32, **extra, **kw)  # noqa: E731
    plain = run()
    assert "split_kv_groups" not in plain and "split_kv" not in seen[-1] and "small_batch_report" not in seen[-1]
    assert run(split_kv=False) == plain and "split_kv" not in seen[-1] and "small_batch_report" not in seen[-1]
    lines_plain = out.read_text()
    on = run(split_kv=True)
    assert seen[-1]["split_kv"] is True and "small_batch" not in seen[-1]
    assert on == dict(plain, split_kv_groups=3)
    both = run(split_kv=True, small_batch=True)
    assert both == dict(plain, split_kv_groups=3, small_batch_groups=3)
    assert run(small_batch=True) == dict(plain, small_batch_groups=3)
    assert out.read_text() == lines_plain
    assert all(set(json.loads(l)) == {"id", "prompt_token_ids", "prompt", "outputs"} for l in lines_plain.splitlines())


def test_gen_split_kv_is_in_the_configuration_and_handed_on(monkeypatch):
    from ssi.config import compose
    text = open(os.path.join(PKG, "conf", "generate.yaml")).read()
    assert re.search(r"^  split_kv: false  # ", text, re.M)
    cfg = compose(os.path.join(PKG, "conf"), "generate", ["speech.n_dsus=5000", "gen.output_dir=out"])
    assert cfg.gen.split_kv is False
    spec = importlib.util.spec_from_file_location("generate_script_skv", os.path.join(PKG, "scripts", "generate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import ssi.trainer

    class FakeTrainer:
        token_type_ranges = {}

        def __init__(self, cfg):
            self.model, self.tokenizer = _Model(), sb._Tok()

        def _setup_model(self):
            pass

        _setup_tokenizer = _setup_model

    seen = []
    monkeypatch.setattr(ssi.trainer, "Trainer", FakeTrainer)
    monkeypatch.setattr(mod, "generate_file", lambda *a, **kw: seen.append(kw) or {"items": 0})
    monkeypatch.setattr(os, "makedirs", lambda *a, **kw: None)
    for flag, want in (("false", False), ("true", True)):
        cfg = compose(os.path.join(PKG, "conf"), "generate", ["speech.n_dsus=5000", "gen.output_dir=out", "gen.input=in.jsonl", "device=cpu",
                                                               f"gen.split_kv={flag}"])
        mod.main(cfg)
        assert ("split_kv" in seen[-1]) is want and "small_batch" not in seen[-1]


def test_the_prompt_tool_takes_the_flag(monkeypatch):
    from ssi import prompting
    seen = []
    monkeypatch.setattr(prompting, "generate", lambda model, prompts, **kw: seen.append(kw) or [])
    prompting.probe(None, sb._Tok(), [[1, 2]], stop_token_ids=[])
    assert "split_kv" not in seen[-1] and seen[-1]["small_batch"] is True
    prompting.probe(None, sb._Tok(), [[1, 2]], stop_token_ids=[], split_kv=True)
    assert seen[-1]["split_kv"] is True
    src = open(os.path.join(PKG, "scripts", "prompt.py")).read()
    assert '"--split-kv"' in src and "split_kv=args.split_kv" in src


def test_a_wrong_workspace_is_refused_before_the_library_is_loaded(monkeypatch):
    from ssi import _lib, ops

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    H, KV, hd = 4, 1, 64
    qkv, cache = torch.zeros(2, (H + 2 * KV) * hd), torch.zeros(2, 8, KV * hd)
    i32, out = torch.zeros(2, dtype=torch.int32), torch.zeros(2, H * hd)
    slot_args = (qkv, cache, cache.clone(), i32, i32, out, None, H, KV, hd)
    beam_args = (qkv, cache, cache.clone(), cache.clone(), cache.clone(), i32, i32, i32, torch.zeros(2, 4, dtype=torch.int32), out, None, H, KV, hd)
    for fn, args in ((ops.attn_decode_split, slot_args), (ops.attn_decode_beam_split, beam_args)):
        for ws in (torch.zeros(4096, dtype=torch.float64), torch.zeros(4096, dtype=torch.bfloat16), torch.zeros(4096, dtype=torch.uint8),
                   torch.zeros(4096, device="meta"), torch.zeros(64, 128)[:, ::2], None):
            with pytest.raises(_lib.HipLibraryError, match="workspace"):
                fn(*args, span=64, workspace=ws)
        for span in (0, -64, 1.5):
            with pytest.raises(_lib.HipLibraryError, match="span"):
                fn(*args, span=span, workspace=torch.zeros(4096))
        with pytest.raises(_lib.HipLibraryError, match="GPU"):              # a good workspace: the plain wrappers' checks come next
            fn(*args, span=64, workspace=torch.zeros(4096))
