"""CPU: the host side of FP8 weights — ABI 27 and the four entries in the header and ``_lib`` (each skinny entry with the exponent pointer more),
``check_weight_dtype`` and the refusals before any call (fp8 without ``small_batch``, an unknown string, a prebuilt object without fp8, an object
of another model, a model that takes no small-batch path), the object reaching exactly the steps of the groups that decode on the skinny path and
being built once, ``gen.weight_dtype`` in the configuration, ``--weight-dtype`` of the prompt tool, and the summary key."""
import importlib.util
import os
import re

import pytest
import torch

import test_small_batch_host as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speech-integration_amd")
ENTRIES = (("ssi_gemm_skinny_w8", "gemm_skinny_w8", "ssi_gemm_skinny"), ("ssi_gemm_skinny_rope_w8", "gemm_skinny_rope_w8", "ssi_gemm_skinny_rope"),
           ("ssi_gemm_skinny_swiglu_w8", "gemm_skinny_swiglu_w8", "ssi_gemm_skinny_swiglu"))


def test_the_abi_is_27_and_names_the_four_entries():
    from ssi import _lib, ops
    header = open(os.path.join(ROOT, "include", "ssi_hip.h")).read()
    assert int(re.search(r"#define SSI_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 27
    for name, wrapper, plain in ENTRIES:
        args = re.search(rf"\bint {name}\((.*?)\);", header, re.S).group(1)
        assert name in _lib.PROTOTYPES and len(args.split(",")) == len(_lib.PROTOTYPES[name][1]), name
        assert len(_lib.PROTOTYPES[name][1]) == len(_lib.PROTOTYPES[plain][1]) + 1, name                # (codes, ld_codes, exps) for (W, ldw)
        assert wrapper in ops.__all__ and callable(getattr(ops, wrapper))
    args = re.search(r"\bint ssi_weight_quant_fp8\((.*?)\);", header, re.S).group(1)
    assert len(args.split(",")) == len(_lib.PROTOTYPES["ssi_weight_quant_fp8"][1]) == 9 and "weight_quant_fp8" in ops.__all__
    section = header[header.index("---- FP8 weights"):header.index("int ssi_weight_quant_fp8(")]
    assert "FP8 K/V cache" in section and "ROW OF A WEIGHT MATRIX" in section and "bf16 normal range" in section and "BIT-EQUAL" in section
    assert section.count("RNE") == 0                                                                     # the rule is referred to, not written again
    sources = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "gemm_wq8.hip" in sources


class _Model(sb._Model):
    built = 0

    def quantize_weights(self, head=True):
        self.built += 1
        return ("qw", self.built)

    def _check_weight_quant(self, qw):
        if qw is not None and qw[0] != "qw":
            raise ValueError("weight_quant is not this model's")
        return qw


def test_check_weight_dtype():
    from ssi.generate import check_weight_dtype
    assert check_weight_dtype(None) is None and check_weight_dtype("auto") is None and check_weight_dtype("fp8") == "fp8"
    assert check_weight_dtype(None, False) is None and check_weight_dtype("auto", False) is None
    with pytest.raises(ValueError, match="small_batch"):
        check_weight_dtype("fp8", False)
    for bad in ("FP8", "int8", "bf16", "", 8, True, torch.uint8):
        with pytest.raises(ValueError, match="weight_dtype"):
            check_weight_dtype(bad)


def test_refusals_come_before_any_call():
    from ssi.generate import beam_search, generate, sample
    m = _Model()
    kw = dict(max_new_tokens=2, stop_token_ids=[], pad_id=0)
    loops = ((generate, {}), (sample, dict(temperature=0.5, seed=1)), (beam_search, dict(beam_width=2)))
    for extra, match in ((dict(weight_dtype="fp8"), "small_batch"), (dict(weight_dtype="fp8", small_batch=False), "small_batch"),
                         (dict(weight_dtype="e5m2", small_batch=True), "weight_dtype"), (dict(weight_quant=("qw", 0), small_batch=True), "without weight_dtype"),
                         (dict(weight_dtype="fp8", small_batch=True, weight_quant=("other", 0)), "not this model's")):
        for run, own in loops:
            m.calls.clear()
            with pytest.raises(ValueError, match=match):
                run(m, [[1, 2]], **own, **extra, **kw)
            assert m.calls == [] and m.built == 0


def test_the_model_refuses_what_it_cannot_quantise_and_what_is_not_its_own():
    from ssi.model import HipLlamaDecoder, QuantWeights

    class M:
        num_layers, device = 2, torch.device("cpu")
        _slices = {f"L{l}.{m}": (0, s) for l in range(2) for m, s in (("wqkv", (96, 64)), ("wo", (64, 64)), ("w13", (128, 64)), ("w2", (64, 64)))}
        _slices["emb"] = (0, (256, 64))
        _quant_names, _check_weight_quant, quantize_weights = HipLlamaDecoder._quant_names, HipLlamaDecoder._check_weight_quant, HipLlamaDecoder.quantize_weights

        def takes_small_batch(self, rows, flag):
            return False

    m = M()
    with pytest.raises(ValueError, match="quantize_weights"):                   # an fp32 model, a geometry off the skinny path
        m.quantize_weights()
    mats = lambda names: {n: (torch.zeros(m._slices[n][1], dtype=torch.uint8), torch.zeros(m._slices[n][1][0], dtype=torch.uint8)) for n in names}  # noqa: E731
    full, no_head = QuantWeights(mats(m._quant_names(True))), QuantWeights(mats(m._quant_names(False)))
    assert full.head and not no_head.head and m._check_weight_quant(full) is full and m._check_weight_quant(no_head) is no_head
    assert m._check_weight_quant(None) is None and full.nbytes() == sum(c.numel() + e.numel() for c, e in full.mats.values())
    one_layer = QuantWeights({n: v for n, v in full.mats.items() if not n.startswith("L1.")})
    wrong_shape = QuantWeights(dict(full.mats, **{"L0.wo": (torch.zeros(64, 128, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8))}))
    elsewhere = QuantWeights({n: (c.to("meta"), e) for n, (c, e) in full.mats.items()})
    for bad in (one_layer, wrong_shape, elsewhere, {"emb": 1}, "fp8"):
        with pytest.raises(ValueError, match="weight_quant"):
            m._check_weight_quant(bad)


def test_the_object_reaches_the_steps_of_the_skinny_groups_alone_and_is_built_once():
    m = _Model()
    plain = sb._greedy(m, 5, small_batch=True)
    for value in (None, "auto"):
        assert sb._greedy(m, 5, small_batch=True, weight_dtype=value) == plain and m.built == 0
    got = sb._greedy(m, 70, small_batch=True, batch_size=64, weight_dtype="fp8")                       # groups of 64 and of 6 rows
    assert m.built == 1
    assert all(kw == {"small_batch": True, "weight_quant": ("qw", 1)} for name, _, kw in got if name == "decode_step")
    assert all(kw == {"separate": True} for name, _, kw in got if name == "prefill")                     # prefill never sees it
    report = {}
    got = sb._greedy(m, 70, small_batch=True, batch_size=256, weight_dtype="fp8", small_batch_report=report)   # one group of 70 rows: untouched
    assert m.built == 1 and report == {} and all(kw == {"small_batch": True} for name, _, kw in got if name == "decode_step")
    report = {}
    got = sb._greedy(m, 70, small_batch=True, batch_size=64, weight_dtype="fp8", weight_quant=("qw", 9), small_batch_report=report)
    assert m.built == 1 and report == {"small_batch_groups": 2, "fp8_weight_groups": 2}
    assert all(kw["weight_quant"] == ("qw", 9) for name, _, kw in got if name == "decode_step")
    off = _Model(mfma=False)
    got = sb._greedy(off, 5, small_batch=True, weight_dtype="fp8")
    assert off.built == 0 and all(kw == {"small_batch": True} for name, _, kw in got if name == "decode_step")


@pytest.mark.parametrize("path", ("greedy", "beam", "sample"))
def test_the_summary_key_is_there_only_under_fp8(tmp_path, monkeypatch, path):
    from ssi import generate as G
    seen = []

    def one(p):
        return G.Generation(token_ids=[65], finish_reason="length", stop_reason=None, cumulative_logprob=-1.0, prompt_len=len(p), n_kept_mean=1.0)

    def loop(wrap):
        def run(model, prompts, **kw):
            seen.append(kw)
            if kw.get("weight_dtype") == "fp8":
                kw["small_batch_report"]["fp8_weight_groups"] += 1
            return [wrap(one(p)) for p in prompts]
        return run

    monkeypatch.setattr(G, "generate", loop(lambda g: g))
    monkeypatch.setattr(G, "beam_search", loop(lambda g: [g]))
    monkeypatch.setattr(G, "sample", loop(lambda g: [g]))
    extra = {"greedy": {}, "beam": {"beam_width": 4}, "sample": {"sample": True, "n": 2, "temperature": 0.7, "seed": 1}}[path]
    out = tmp_path / "g.jsonl"
    run = lambda **kw: G.generate_file(_Model(), sb._Tok(), None, str(out), max_new_tokens=2, prompts=[[900, 65]] * 3, **extra, **kw)  # noqa: E731
    plain, small = run(), run(small_batch=True)
    assert "fp8_weight_groups" not in plain and "fp8_weight_groups" not in small
    for value in (None, "auto"):
        assert run(weight_dtype=value) == plain and run(small_batch=True, weight_dtype=value) == small
        assert "weight_dtype" not in seen[-1] and "weight_quant" not in seen[-1]
    got = run(small_batch=True, weight_dtype="fp8", weight_quant=("qw", 3))
    assert got == dict(small, fp8_weight_groups=1) and seen[-1]["weight_dtype"] == "fp8" and seen[-1]["weight_quant"] == ("qw", 3)
    n = len(seen)
    for bad, match in ((dict(weight_dtype="fp8"), "small_batch"), (dict(weight_dtype="fp4", small_batch=True), "weight_dtype"),
                       (dict(weight_quant=("qw", 3), small_batch=True), "without weight_dtype")):
        with pytest.raises(ValueError, match=match):
            run(**bad)
    assert len(seen) == n


def test_gen_weight_dtype_is_in_the_configuration_and_handed_on(monkeypatch):
    from ssi.config import compose
    text = open(os.path.join(PKG, "conf", "generate.yaml")).read()
    assert re.search(r"^  weight_dtype: auto  # ", text, re.M)
    base = ["speech.n_dsus=5000", "gen.output_dir=out", "gen.input=in.jsonl", "device=cpu"]
    assert compose(os.path.join(PKG, "conf"), "generate", base).gen.weight_dtype == "auto"
    spec = importlib.util.spec_from_file_location("generate_script_w8", os.path.join(PKG, "scripts", "generate.py"))
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
    for extra, want in (([], None), (["gen.weight_dtype=auto", "gen.small_batch=true"], None), (["gen.weight_dtype=fp8", "gen.small_batch=true"], "fp8")):
        mod.main(compose(os.path.join(PKG, "conf"), "generate", base + extra))
        assert seen[-1].get("weight_dtype") == want
    n = len(seen)
    for extra, match in ((["gen.weight_dtype=fp8"], "small_batch"), (["gen.weight_dtype=int4", "gen.small_batch=true"], "weight_dtype")):
        with pytest.raises(ValueError, match=match):
            mod.main(compose(os.path.join(PKG, "conf"), "generate", base + extra))
    assert len(seen) == n


def test_the_prompt_tool_takes_the_option_and_builds_the_object_once(monkeypatch):
    from ssi import prompting
    seen = []
    monkeypatch.setattr(prompting, "generate", lambda model, prompts, **kw: seen.append(kw) or [])
    m = _Model()
    for value in (None, "auto"):
        prompting.probe(m, sb._Tok(), [[1, 2]], stop_token_ids=[], weight_dtype=value)
        assert "weight_dtype" not in seen[-1] and "weight_quant" not in seen[-1] and m.built == 0
    prompting.probe(m, sb._Tok(), [[1, 2], [3]], stop_token_ids=[], weight_dtype="fp8")
    assert seen[-1]["weight_dtype"] == "fp8" and seen[-1]["weight_quant"] == ("qw", 1) and seen[-1]["small_batch"] is True and m.built == 1
    prompting.probe(m, sb._Tok(), [[1, 2]], stop_token_ids=[], weight_dtype="fp8", weight_quant=("qw", 1))      # reused across calls
    assert seen[-1]["weight_quant"] == ("qw", 1) and m.built == 1
    with pytest.raises(ValueError, match="weight_dtype"):
        prompting.probe(m, sb._Tok(), [[1, 2]], stop_token_ids=[], weight_dtype="e5m2")
    spec = importlib.util.spec_from_file_location("prompt_script_w8", os.path.join(PKG, "scripts", "prompt.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    actions = {a.dest: a for a in mod.build_parser()._actions}
    assert actions["weight_dtype"].default == "auto" and set(actions["weight_dtype"].choices) == {"auto", "fp8"}
    src = open(os.path.join(PKG, "scripts", "prompt.py")).read()
    assert '"--weight-dtype"' in src and "weight_dtype=args.weight_dtype" in src
