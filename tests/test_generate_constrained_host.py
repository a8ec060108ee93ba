"""CPU: the host side of constrained decoding — the ABI names ``ssi_decode_select``, its wrapper refuses CPU tensors, ``allowed_mask`` and the
refusals of ``generate`` (before any launch, on a model stub), what ``check_greedy`` and ``conf/generate.yaml`` accept, the summary of
``generate_file``, and the kernel in the built library (no scratch, no matrix instruction; from the report of ``tools/kernel_lint.py``)."""
import os
import re
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speech-integration_amd")
LIB = os.path.join(PKG, "libssi_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def test_the_abi_names_the_entry():
    from ssi import _lib, ops
    header = open(os.path.join(ROOT, "include", "ssi_hip.h")).read()
    assert int(re.search(r"#define SSI_ABI_VERSION (\d+)", header).group(1)) >= 19 and _lib.ABI_VERSION >= 19
    assert re.search(r"\* 19: \+ ssi_decode_select", header), "the ABI history names the entry"
    assert re.search(r"\bint ssi_decode_select\(", header)
    assert "ssi_decode_select" in _lib.PROTOTYPES and "decode_select" in ops.__all__ and callable(ops.decode_select)
    args = re.search(r"\bint ssi_decode_select\((.*?)\);", header, re.S).group(1)
    assert len(args.split(",")) == len(_lib.PROTOTYPES["ssi_decode_select"][1]) == 13
    assert "decode_select.hip" in open(os.path.join(PKG, "csrc", "Makefile")).read()


def test_the_wrapper_refuses_cpu_tensors():
    from ssi import _lib, ops
    with pytest.raises(_lib.HipLibraryError, match="GPU"):
        ops.decode_select(torch.zeros(3, 40), 33, torch.zeros(3, dtype=torch.int64), torch.zeros(3), torch.zeros(3, dtype=torch.int32),
                          allow=torch.zeros(2, dtype=torch.int32))


def test_allowed_mask_on_ids_ranges_and_out_of_range_input():
    from ssi.generate import allowed_mask
    m = allowed_mask(40, ids=[0, 39, 7, 7], ranges=[(10, 12), (30, 30)])
    assert m.dtype == torch.bool and m.shape == (40,)
    assert m.nonzero().flatten().tolist() == [0, 7, 10, 11, 12, 30, 39]
    assert not bool(allowed_mask(40).any()) and bool(allowed_mask(40, ranges=[(0, 39)]).all())
    for kw in (dict(ids=[40]), dict(ids=[-1]), dict(ranges=[(5, 40)]), dict(ranges=[(-1, 3)]), dict(ranges=[(7, 6)])):
        with pytest.raises(ValueError, match="vocabulary"):
            allowed_mask(40, **kw)


class _Stub:
    """A model that fails the test on any use beyond its vocabulary size: the refusals come before any launch."""
    vocab_size = 40

    def __getattr__(self, name):
        raise AssertionError(f"generate touched model.{name} before refusing")


@pytest.mark.parametrize("kw,match", [
    (dict(min_new_tokens=-1), "min_new_tokens"),
    (dict(allowed_token_ids=[3, 40]), "vocabulary"),
    (dict(allowed_token_ids=[-2]), "vocabulary"),
    (dict(allowed_token_ids=[3], stop_token_ids=[41]), "vocabulary"),
    (dict(allowed_token_ids=[]), "allows no token"),
    (dict(allowed_token_ids=torch.zeros(40, dtype=torch.bool)), "allows no token"),
    (dict(allowed_token_ids=torch.ones(39, dtype=torch.bool)), "mask"),
    (dict(allowed_token_ids=[5, 6], stop_token_ids=[5, 6], min_new_tokens=1), "besides the stop tokens"),
])
def test_generate_refuses_before_any_launch(kw, match):
    from ssi.generate import generate
    args = dict(max_new_tokens=4, stop_token_ids=[], pad_id=0)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        generate(_Stub(), [[1, 2, 3]], **args)


def test_the_stop_tokens_join_the_allowed_set_and_leave_the_early_one():
    from ssi.generate import _constraint_masks, _mask_words
    assert _constraint_masks(40, None, 0, [5]) is None                        # neither argument: no mask is built
    allow, early = _constraint_masks(40, [1, 2, 5], 3, [5, 9])
    assert allow.nonzero().flatten().tolist() == [1, 2, 5, 9] and early.nonzero().flatten().tolist() == [1, 2]
    allow, early = _constraint_masks(40, None, 2, [5])                        # min_new_tokens alone: everything but the stop tokens
    assert bool(allow.all()) and (~early).nonzero().flatten().tolist() == [5]
    w = _mask_words(allow)
    assert w.dtype == torch.int32 and w.tolist() == [-1, 255]                 # 40 bits: word 0 full, bits 0..7 of word 1
    m = torch.zeros(70, dtype=torch.bool)
    m[[0, 31, 32, 69]] = True
    assert (_mask_words(m).long() & 0xffffffff).tolist() == [1 | 1 << 31, 1, 1 << 5]


def test_check_greedy_accepts_the_two_constraints_and_nothing_else_new():
    from ssi.config import compose
    from ssi.generate import check_greedy
    check_greedy({"temperature": 0.0, "min_tokens": 5, "allowed_token_ids": [1, 2]})
    check_greedy({"min_tokens": 0, "allowed_token_ids": None})
    with pytest.raises(NotImplementedError, match="temperature"):
        check_greedy({"min_tokens": 5, "temperature": 0.7})
    with pytest.raises(NotImplementedError, match="logit_bias"):
        check_greedy({"min_tokens": 5, "logit_bias": {1: 2.0}})
    with pytest.raises(NotImplementedError, match="bad_words"):
        check_greedy({"bad_words": ["x"]})
    for bad in ({"min_tokens": -1}, {"min_tokens": 1.5}, {"min_tokens": None}, {"allowed_token_ids": 3}, {"allowed_token_ids": [1, "a"]},
                {"allowed_token_ids": "12"}):
        with pytest.raises(ValueError):
            check_greedy(bad)
    cfg = compose(os.path.join(PKG, "conf"), "generate", ["speech.n_dsus=5000", "gen.output_dir=out"])
    check_greedy(cfg.sampling_params)                                          # the committed file composes and passes
    assert cfg.sampling_params.min_tokens == 0 and cfg.sampling_params.allowed_token_ids is None and cfg.gen.allowed_token_types is None
    cfg = compose(os.path.join(PKG, "conf"), "generate", ["speech.n_dsus=5000", "gen.output_dir=out", "sampling_params.min_tokens=5",
                                                          "sampling_params.allowed_token_ids=[1,2]", "gen.allowed_token_types=[text,special_text]"])
    check_greedy(cfg.sampling_params)
    assert list(cfg.sampling_params.allowed_token_ids) == [1, 2] and list(cfg.gen.allowed_token_types) == ["text", "special_text"]


def test_the_script_resolves_token_types_to_a_mask():
    import importlib.util
    spec = importlib.util.spec_from_file_location("generate_script_constrained", os.path.join(PKG, "scripts", "generate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ranges = {"text": (0, 9), "special_text": (10, 11), "dsu": (12, 35), "modality": (36, 37)}

    def cfg(kinds, ids):
        return SimpleNamespace(gen={"allowed_token_types": kinds}, sampling_params={"allowed_token_ids": ids})

    assert mod.allowed_tokens(cfg(None, None), ranges, 40) is None             # the defaults: today's call
    m = mod.allowed_tokens(cfg(["text", "special_text"], [36]), ranges, 40)
    assert m.nonzero().flatten().tolist() == list(range(12)) + [36]
    assert mod.allowed_tokens(cfg(None, [3]), ranges, 40).nonzero().flatten().tolist() == [3]
    with pytest.raises(ValueError, match="units"):
        mod.allowed_tokens(cfg(["units"], None), ranges, 40)


class _Tok:
    special_tokens = {}
    eos_id, eom_id, eot_id, pad_id = 31, 38, 39, 34

    def decode(self, ids, **kw):
        return " ".join(str(t) for t in ids)


def test_the_summary_gains_constrained_tokens_only_under_a_constraint(tmp_path, monkeypatch):
    from ssi import generate as G
    seen = {}

    def fake_generate(model, prompts, **kw):
        seen.clear()
        seen.update(kw)
        con = kw.get("allowed_token_ids") is not None or kw.get("min_new_tokens", 0) > 0
        return [G.Generation(token_ids=[5, 6], finish_reason="length", stop_reason=None, cumulative_logprob=-1.0, prompt_len=len(p),
                             n_constrained=i + 1 if con else None) for i, p in enumerate(prompts)]

    monkeypatch.setattr(G, "generate", fake_generate)
    out = tmp_path / "g.jsonl"
    kw = dict(max_new_tokens=2, prompts=[[1], [2, 3], [4]])
    assert G.generate_file(object(), _Tok(), None, str(out), **kw) == {"items": 3, "generated_tokens": 6, "stopped": 0}
    assert "allowed_token_ids" not in seen and "min_new_tokens" not in seen
    got = G.generate_file(object(), _Tok(), None, str(out), allowed_token_ids=[5, 6], **kw)
    assert got == {"items": 3, "generated_tokens": 6, "stopped": 0, "constrained_tokens": 6} and seen["allowed_token_ids"] == [5, 6]
    got = G.generate_file(object(), _Tok(), None, str(out), min_new_tokens=1, **kw)
    assert got["constrained_tokens"] == 6 and seen["min_new_tokens"] == 1
    import json
    for line in out.read_text().splitlines():                                  # the per-line record keeps exactly its keys
        rec = json.loads(line)
        assert set(rec) == {"id", "prompt_token_ids", "prompt", "outputs"}
        assert set(rec["outputs"][0]) == {"index", "text", "token_ids", "cumulative_logprob", "finish_reason", "stop_reason", "stop_reason_text"}
    assert G.Generation([1], "length", None, None, 1).n_constrained is None


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(LLVM)), reason="needs the built library and llvm-objdump")
def test_the_kernel_is_in_the_library_without_scratch_or_matrix_instructions():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_lint
    errs, rep = kernel_lint.lint(LIB)
    hit = [n for n in rep if "decode_select_kernel" in n]
    assert len(hit) == 2, hit                                                 # bf16 and fp32, nothing else instantiated
    for n in hit:
        assert rep[n]["scratch"] == 0 and rep[n]["mfma"] == 0 and rep[n]["lds_dma"] == 0 and not rep[n]["errors"], (n, rep[n])
    assert not [e for e in errs if "decode_select" in e], errs
