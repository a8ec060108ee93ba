"""CPU: the host side of the FP8 K/V cache — the ABI number and the five entries in the header and ``_lib`` (each the plain entry with two more
pointers per cache), the wrappers' refusals before the library is loaded, ``check_kv_cache_dtype``, the argument reaching ``new_kv_cache`` of every
loop only under "fp8", ``gen.kv_cache_dtype`` in the configuration and handed on, ``--kv-cache-dtype`` of the prompt tool, and the summary key."""
import importlib.util
import os
import re

import pytest
import torch

import test_small_batch_host as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speech-integration_amd")
ENTRIES = (("ssi_kv_store_fp8", "kv_store_fp8", "ssi_kv_store", 1), ("ssi_attn_decode_fp8", "attn_decode_fp8", "ssi_attn_decode", 1),
           ("ssi_attn_decode_beam_fp8", "attn_decode_beam_fp8", "ssi_attn_decode_beam", 2),
           ("ssi_attn_decode_split_fp8", "attn_decode_split_fp8", "ssi_attn_decode_split", 1),
           ("ssi_attn_decode_beam_split_fp8", "attn_decode_beam_split_fp8", "ssi_attn_decode_beam_split", 2))


def test_the_abi_is_26_and_names_the_five_entries():
    from ssi import _lib, ops
    header = open(os.path.join(ROOT, "include", "ssi_hip.h")).read()
    assert int(re.search(r"#define SSI_ABI_VERSION (\d+)", header).group(1)) >= 26 and _lib.ABI_VERSION >= 26
    assert int(re.search(r"#define SSI_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    for name, wrapper, plain, caches in ENTRIES:
        args = re.search(rf"\bint {name}\((.*?)\);", header, re.S).group(1)
        assert name in _lib.PROTOTYPES and len(args.split(",")) == len(_lib.PROTOTYPES[name][1]), name
        assert wrapper in ops.__all__ and callable(getattr(ops, wrapper))
        assert len(_lib.PROTOTYPES[name][1]) == len(_lib.PROTOTYPES[plain][1]) + 2 * caches, name       # k_exp and v_exp of every cache
        assert _lib.PROTOTYPES[name][1][-2:] == _lib.PROTOTYPES[plain][1][-2:]
    assert "e4m3" in header and "2^(b - 127)" in header and "2^-116" in header                          # the definition, once


class _Model(sb._Model):
    def __init__(self):
        super().__init__()
        self.opened = []

    def new_kv_cache(self, n_slots, cap, **kw):
        self.opened.append(kw)
        return sb._Cache(n_slots, cap)


def test_check_kv_cache_dtype():
    from ssi.generate import check_kv_cache_dtype
    assert check_kv_cache_dtype(None) is None and check_kv_cache_dtype("auto") is None and check_kv_cache_dtype("fp8") == "fp8"
    for bad in ("FP8", "fp16", "bf16", "", 8, True, torch.uint8):
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            check_kv_cache_dtype(bad)


def test_the_argument_reaches_new_kv_cache_only_under_fp8_and_is_refused_before_any_call():
    m = _Model()
    plain = sb._greedy(m, 5)
    assert m.opened == [{}]
    for value in (None, "auto"):
        m.opened.clear()
        assert sb._greedy(m, 5, kv_cache_dtype=value) == plain and m.opened == [{}]       # new_kv_cache as it was always called
    m.opened.clear()
    assert sb._greedy(m, 5, kv_cache_dtype="fp8") == plain and m.opened == [{"dtype": "fp8"}]      # no decode step takes a new keyword
    m.opened.clear()
    assert sb._greedy(m, 5, kv_cache_dtype="fp8", small_batch=True, batch_size=2)         # three groups, orthogonal to the other flags
    assert m.opened and all(kw == {"dtype": "fp8"} for kw in m.opened)
    from ssi.generate import beam_search, generate, sample
    kw = dict(max_new_tokens=2, stop_token_ids=[], pad_id=0, kv_cache_dtype="int8")
    for run, extra in ((generate, {}), (sample, dict(temperature=0.5, seed=1)), (beam_search, dict(beam_width=2))):
        m.opened.clear()
        m.calls.clear()
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            run(m, [[1, 2]], **extra, **kw)
        assert m.opened == [] and m.calls == []


@pytest.mark.parametrize("path", ("greedy", "beam", "sample"))
def test_the_summary_key_is_there_only_under_fp8(tmp_path, monkeypatch, path):
    from ssi import generate as G
    seen = []

    def one(p):
        return G.Generation(token_ids=[65], finish_reason="length", stop_reason=None, cumulative_logprob=-1.0, prompt_len=len(p), n_kept_mean=1.0)

    def loop(wrap):
        def run(model, prompts, **kw):
            seen.append(kw)
            return [wrap(one(p)) for p in prompts]
        return run

    monkeypatch.setattr(G, "generate", loop(lambda g: g))
    monkeypatch.setattr(G, "beam_search", loop(lambda g: [g]))
    monkeypatch.setattr(G, "sample", loop(lambda g: [g]))
    extra = {"greedy": {}, "beam": {"beam_width": 4}, "sample": {"sample": True, "n": 2, "temperature": 0.7, "seed": 1}}[path]
    out = tmp_path / "g.jsonl"
    run = lambda **kw: G.generate_file(_Model(), sb._Tok(), None, str(out), max_new_tokens=2, prompts=[[900, 65]] * 3, **extra, **kw)  # noqa: E731
    plain = run()
    assert "kv_cache_dtype" not in plain and "kv_cache_dtype" not in seen[-1]
    for value in (None, "auto"):
        assert run(kv_cache_dtype=value) == plain and "kv_cache_dtype" not in seen[-1]
    lines = out.read_text()
    assert run(kv_cache_dtype="fp8") == dict(plain, kv_cache_dtype="fp8") and seen[-1]["kv_cache_dtype"] == "fp8"
    assert out.read_text() == lines
    both = run(kv_cache_dtype="fp8", split_kv=True)
    assert both["kv_cache_dtype"] == "fp8" and "split_kv_groups" in both and seen[-1]["kv_cache_dtype"] == "fp8" and seen[-1]["split_kv"] is True
    n = len(seen)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        run(kv_cache_dtype="fp4")
    assert len(seen) == n


def test_gen_kv_cache_dtype_is_in_the_configuration_and_handed_on(monkeypatch):
    from ssi.config import compose
    text = open(os.path.join(PKG, "conf", "generate.yaml")).read()
    assert re.search(r"^  kv_cache_dtype: auto  # ", text, re.M)
    cfg = compose(os.path.join(PKG, "conf"), "generate", ["speech.n_dsus=5000", "gen.output_dir=out"])
    assert cfg.gen.kv_cache_dtype == "auto"
    spec = importlib.util.spec_from_file_location("generate_script_fp8", os.path.join(PKG, "scripts", "generate.py"))
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
    for value, want in (("auto", None), ("fp8", "fp8")):
        cfg = compose(os.path.join(PKG, "conf"), "generate", ["speech.n_dsus=5000", "gen.output_dir=out", "gen.input=in.jsonl", "device=cpu",
                                                               f"gen.kv_cache_dtype={value}"])
        mod.main(cfg)
        assert seen[-1].get("kv_cache_dtype") == want and "split_kv" not in seen[-1]
    cfg = compose(os.path.join(PKG, "conf"), "generate", ["speech.n_dsus=5000", "gen.output_dir=out", "gen.input=in.jsonl", "device=cpu",
                                                           "gen.kv_cache_dtype=int4"])
    n = len(seen)
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        mod.main(cfg)
    assert len(seen) == n


def test_the_prompt_tool_takes_the_option(monkeypatch):
    from ssi import prompting
    seen = []
    monkeypatch.setattr(prompting, "generate", lambda model, prompts, **kw: seen.append(kw) or [])
    prompting.probe(None, sb._Tok(), [[1, 2]], stop_token_ids=[])
    assert "kv_cache_dtype" not in seen[-1]
    prompting.probe(None, sb._Tok(), [[1, 2]], stop_token_ids=[], kv_cache_dtype="auto")
    assert "kv_cache_dtype" not in seen[-1]
    prompting.probe(None, sb._Tok(), [[1, 2]], stop_token_ids=[], kv_cache_dtype="fp8")
    assert seen[-1]["kv_cache_dtype"] == "fp8"
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        prompting.probe(None, sb._Tok(), [[1, 2]], stop_token_ids=[], kv_cache_dtype="e5m2")
    spec = importlib.util.spec_from_file_location("prompt_script_fp8", os.path.join(PKG, "scripts", "prompt.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.build_parser()
    src = open(os.path.join(PKG, "scripts", "prompt.py")).read()
    assert '"--kv-cache-dtype"' in src and "kv_cache_dtype=args.kv_cache_dtype" in src
    assert {a.dest: a for a in p._actions}["kv_cache_dtype"].default == "auto" and set({a.dest: a for a in p._actions}["kv_cache_dtype"].choices) == {"auto", "fp8"}


def test_wrong_cache_tensors_are_refused_before_the_library_is_loaded(monkeypatch):
    from ssi import _lib, ops

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    H, KV, hd = 4, 1, 64
    qkv = torch.zeros(2, (H + 2 * KV) * hd)
    codes, exps = torch.zeros(2, 8, KV * hd, dtype=torch.uint8), torch.zeros(2, 8, KV, dtype=torch.uint8)
    i32, out = torch.zeros(2, dtype=torch.int32), torch.zeros(2, H * hd)
    good = (codes, codes.clone(), exps, exps.clone())
    bad_caches = [(codes.float(), good[1], exps, good[3]), (codes, good[1], exps.to(torch.int8), good[3]), (codes, good[1], exps[:, :, :0], good[3]),
                  (codes[:, :4], good[1], exps, good[3]), (codes, good[1], torch.zeros(2, 4, KV, dtype=torch.uint8), torch.zeros(2, 4, KV, dtype=torch.uint8)),
                  (codes, good[1], torch.zeros(2, 8, KV * hd, dtype=torch.uint8), good[3]), (codes.to("meta"), good[1], exps, good[3]),
                  (codes, good[1], None, good[3]), (torch.zeros(2, 8, 2 * hd, dtype=torch.uint8)[:, :, :hd], good[1], exps, good[3])]
    ws = torch.zeros(4096)
    anc = torch.zeros(2, 4, dtype=torch.int32)
    dest = torch.zeros(2, dtype=torch.int64)
    for bad in bad_caches:
        calls = ((ops.kv_store_fp8, (qkv, dest, *bad, H, KV, hd), {}),
                 (ops.attn_decode_fp8, (qkv, *bad, i32, i32, out, None, H, KV, hd), {}),
                 (ops.attn_decode_split_fp8, (qkv, *bad, i32, i32, out, None, H, KV, hd), dict(span=64, workspace=ws)),
                 (ops.attn_decode_beam_fp8, (qkv, bad, good, i32, i32, i32, anc, out, None, H, KV, hd), {}),
                 (ops.attn_decode_beam_fp8, (qkv, good, bad, i32, i32, i32, anc, out, None, H, KV, hd), {}),
                 (ops.attn_decode_beam_split_fp8, (qkv, good, bad, i32, i32, i32, anc, out, None, H, KV, hd), dict(span=64, workspace=ws)))
        for fn, args, kw in calls:
            with pytest.raises(_lib.HipLibraryError, match="uint8|one cache"):
                fn(*args, **kw)
    with pytest.raises(_lib.HipLibraryError, match="workspace"):
        ops.attn_decode_split_fp8(qkv, *good, i32, i32, out, None, H, KV, hd, span=64, workspace=torch.zeros(8, dtype=torch.float64))
    with pytest.raises(_lib.HipLibraryError, match="fp32 or bf16"):
        ops.attn_decode_fp8(qkv.half(), *good, i32, i32, out.half(), None, H, KV, hd)
    for fn, args, kw in ((ops.kv_store_fp8, (qkv, dest, *good, H, KV, hd), {}), (ops.attn_decode_fp8, (qkv, *good, i32, i32, out, None, H, KV, hd), {}),
                         (ops.attn_decode_beam_fp8, (qkv, good, good, i32, i32, i32, anc, out, None, H, KV, hd), {})):
        with pytest.raises(_lib.HipLibraryError, match="GPU"):              # good caches: the shared checks come next (no CPU fallback)
            fn(*args, **kw)


def test_new_kv_cache_and_check_cache_know_both_kinds():
    import inspect
    from ssi.model import HipLlamaDecoder, KVCache
    assert inspect.signature(HipLlamaDecoder.new_kv_cache).parameters["dtype"].default is None
    z = torch.zeros(1, 2, 4, 8)
    plain = KVCache(z, z.clone(), torch.zeros(2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    assert plain.dtype == torch.float32 and plain.k_exp is None and len(plain.layer(0)) == 2
    u = torch.zeros(1, 2, 4, 8, dtype=torch.uint8)
    e = torch.zeros(1, 2, 4, 1, dtype=torch.uint8)
    fp8 = KVCache(u, u.clone(), plain.lengths, plain.errors, e, e.clone())
    assert fp8.dtype == "fp8" and len(fp8.layer(0)) == 4 and fp8.layer(0)[2].shape == (2, 4, 1) and (fp8.n_slots, fp8.cap) == (2, 4)

    class M:
        num_layers, num_kv_heads, head_dim, dtype, device = 1, 1, 8, torch.float32, torch.device("cpu")
        _check_cache = HipLlamaDecoder._check_cache

    m = M()
    m._check_cache(plain)
    m._check_cache(fp8)
    m._check_cache(fp8, beside=fp8)
    with pytest.raises(ValueError, match="different kinds"):
        m._check_cache(fp8, beside=plain)
    with pytest.raises(ValueError, match="different kinds"):
        m._check_cache(plain, beside=fp8)
    with pytest.raises(ValueError, match="not this model's"):
        m._check_cache(KVCache(u, u.clone(), plain.lengths, plain.errors, torch.zeros(1, 2, 4, 2, dtype=torch.uint8), e))
    with pytest.raises(ValueError, match="not this model's"):
        m._check_cache(KVCache(u, u.clone(), plain.lengths, plain.errors))                      # uint8 tensors without exponents are no plain cache
