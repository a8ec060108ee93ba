"""CPU: the prompt tool — ``ssi.prompting.render_prompt`` (exactly one of text, token ids and a Jinja2 template; ids validated against the
vocabulary; the modality variables supplied; ``speech_units`` rendered through ``units_to_text``, with and without deduplication; a clear
refusal without jinja2), ``probe`` (greedy at temperature 0, sampling otherwise, always ``small_batch=True``), the argument parsing of
``scripts/prompt.py`` and its JSONL records.  No checkpoint: a character tokenizer stands in."""
import builtins
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speech-integration_amd")


class Tok:
    """One id per character (its code point, private-use characters included), BOS 1, EOS 2; ids from 0x110000 are out of the vocabulary."""
    vocab_size = 0x110000
    special_tokens = {"<|eot_id|>": 5}
    eos_id, eom_id, eot_id, pad_id = 2, 4, 5, 0

    def encode(self, text, add_bos=True, add_eos=True):
        return ([1] if add_bos else []) + [ord(c) for c in text] + ([2] if add_eos else [])

    def decode(self, ids, **kw):
        return "".join(chr(t) for t in ids if t > 5)


@pytest.fixture(scope="module")
def script():
    spec = importlib.util.spec_from_file_location("prompt_script", os.path.join(PKG, "scripts", "prompt.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_text_and_token_ids():
    from ssi.prompting import render_prompt
    assert render_prompt(Tok(), text="hi") == [1, ord("h"), ord("i")]                  # BOS, no EOS
    assert render_prompt(Tok(), token_ids=[7, 8, 9]) == [7, 8, 9]                     # as they are
    assert render_prompt(Tok(), token_ids=(t for t in (7, 8))) == [7, 8]


def test_the_three_inputs_are_mutually_exclusive():
    from ssi.prompting import render_prompt
    for kw in ({}, {"text": "a", "token_ids": [1]}, {"text": "a", "template": "b"}, {"token_ids": [1], "template": "b"},
               {"text": "a", "token_ids": [1], "template": "b"}):
        with pytest.raises(ValueError, match="exactly one"):
            render_prompt(Tok(), **kw)
    with pytest.raises(ValueError, match="template"):
        render_prompt(Tok(), text="a", variables={"x": 1})
    with pytest.raises(ValueError, match="empty"):
        render_prompt(Tok(), token_ids=[])


def test_token_ids_are_validated_against_the_vocabulary():
    from ssi.prompting import render_prompt
    with pytest.raises(ValueError, match="vocabulary"):
        render_prompt(Tok(), token_ids=[3, Tok.vocab_size])
    with pytest.raises(ValueError, match="vocabulary"):
        render_prompt(Tok(), token_ids=[-1])
    assert render_prompt(Tok(), token_ids=[Tok.vocab_size - 1]) == [Tok.vocab_size - 1]


def test_templates_get_the_modality_tokens_and_the_units_as_text(tmp_path):
    pytest.importorskip("jinja2")
    from ssi.prompting import render_prompt, render_template
    from ssi.tokenizer import MODALITY_TOKEN_SPEECH, MODALITY_TOKEN_TEXT, units_to_text
    tpl = "{{ MODALITY_TOKEN_SPEECH }}{{ speech_units }}{{ MODALITY_TOKEN_TEXT }}{{ lang }}:"
    units = [17, 17, 403, 9, 9, 9, 17]
    want = MODALITY_TOKEN_SPEECH + units_to_text(units) + MODALITY_TOKEN_TEXT + "en:"
    assert render_template(tpl, {"speech_units": units, "lang": "en"}) == want
    dedup = MODALITY_TOKEN_SPEECH + units_to_text([17, 403, 9, 17]) + MODALITY_TOKEN_TEXT + "en:"
    assert render_template(tpl, {"speech_units": units, "lang": "en"}, deduplicate=True) == dedup
    assert render_prompt(Tok(), template=tpl, variables={"speech_units": units, "lang": "en"}) == [1] + [ord(c) for c in want]
    assert render_prompt(Tok(), template=tpl, variables={"speech_units": units, "lang": "en"}, deduplicate=True) == [1] + [ord(c) for c in dedup]
    path = tmp_path / "asr.j2"                                                       # a template named by its path
    path.write_text(tpl, encoding="utf-8")
    assert render_template(str(path), {"speech_units": units, "lang": "en"}) == want
    assert render_template("{{ MODALITY_TOKEN_TEXT }}", {"MODALITY_TOKEN_TEXT": "<t>"}) == "<t>"      # a caller's value wins
    import jinja2
    with pytest.raises(jinja2.UndefinedError):
        render_template(tpl, {"speech_units": units})                                # lang is missing: an error, not an empty string


def test_without_jinja2_a_template_is_refused_and_the_rest_works(monkeypatch):
    from ssi.prompting import render_prompt
    real = builtins.__import__

    def no_jinja(name, *a, **kw):
        if name == "jinja2" or name.startswith("jinja2."):
            raise ImportError("No module named 'jinja2'")
        return real(name, *a, **kw)

    monkeypatch.setattr(builtins, "__import__", no_jinja)
    with pytest.raises(RuntimeError, match="jinja2.*not installed"):
        render_prompt(Tok(), template="{{ x }}", variables={"x": 1})
    assert render_prompt(Tok(), text="a") == [1, 97] and render_prompt(Tok(), token_ids=[9]) == [9]


def test_probe_picks_the_loop_and_sets_small_batch(monkeypatch):
    from ssi import generate as G
    from ssi import prompting as P
    seen = []

    def gen(tokens):
        return G.Generation(token_ids=tokens, finish_reason="stop", stop_reason=5, cumulative_logprob=-2.0, prompt_len=2, n_kept_mean=3.0)

    monkeypatch.setattr(P, "generate", lambda model, prompts, **kw: seen.append(("generate", kw)) or [gen([ord("o"), ord("k"), 5]) for _ in prompts])
    monkeypatch.setattr(P, "sample", lambda model, prompts, **kw: seen.append(("sample", kw)) or [[gen([ord("a") + j, 5]) for j in range(kw["n"])] for _ in prompts])
    found = P.probe(object(), Tok(), [[1, 104], [1, 105]])
    name, kw = seen[-1]
    assert name == "generate" and kw["small_batch"] is True and kw["logprobs"] is True and kw["max_new_tokens"] == 128
    assert kw["stop_token_ids"] == [4, 5, 2] and kw["pad_id"] == 0 and kw["repetition_penalty"] == 1.0
    assert [p.texts for p in found] == [["ok"], ["ok"]] and [p.prompt_ids for p in found] == [[1, 104], [1, 105]]
    found = P.probe(object(), Tok(), [[1, 104]], n=3, temperature=0.7, top_k=40, top_p=0.9, seed=11, max_new_tokens=9, repetition_penalty=1.2)
    name, kw = seen[-1]
    assert name == "sample" and kw["small_batch"] is True and (kw["n"], kw["temperature"], kw["top_k"], kw["top_p"], kw["seed"]) == (3, 0.7, 40, 0.9, 11)
    assert kw["max_new_tokens"] == 9 and kw["repetition_penalty"] == 1.2 and "logprobs" not in kw
    assert found[0].texts == ["a", "b", "c"] and len(found[0].generations) == 3
    with pytest.raises(ValueError, match="temperature 0"):
        P.probe(object(), Tok(), [[1, 104]], n=2)
    # the JSONL records: output_record's keys, one entry per sample
    recs = P.prompt_records(found, Tok())
    assert len(recs) == 1 and set(recs[0]) == {"id", "prompt_token_ids", "prompt", "outputs"} and len(recs[0]["outputs"]) == 3
    assert set(recs[0]["outputs"][0]) == {"index", "text", "token_ids", "cumulative_logprob", "finish_reason", "stop_reason", "stop_reason_text"}
    assert recs[0]["outputs"][1]["text"] == "b" and recs[0]["outputs"][1]["stop_reason_text"] == "<|eot_id|>" and recs[0]["prompt"] == "h"
    assert recs[0] == G.output_record(0, [1, 104], found[0].generations, Tok(), {})
    json.dumps(recs)


def test_the_script_parses_its_arguments(script):
    p = script.build_parser()
    base = ["--checkpoint-dir", "ckpt", "--n-dsus", "5000"]
    a = p.parse_args(base + ["--prompt", "hello"])
    assert (a.checkpoint_dir, a.n_dsus, a.dtype, a.prompt, a.tokens, a.template) == ("ckpt", 5000, "bf16", ["hello"], None, None)
    assert (a.n, a.temperature, a.top_k, a.top_p, a.seed, a.max_new_tokens, a.jsonl) == (1, 0.0, -1, 1.0, 0, 128, None)      # greedy, one sample
    assert (a.repetition_penalty, a.frequency_penalty, a.presence_penalty) == (1.0, 0.0, 0.0)
    assert script.prompts_of(a, Tok()) == [[1] + [ord(c) for c in "hello"]]
    a = p.parse_args(base + ["--tokens", "7, 8 9", "--tokens", "10", "--dtype", "fp32", "-n", "4", "--temperature", "0.8", "--top-k", "50",
                             "--top-p", "0.9", "--seed", "3", "--jsonl", "out.jsonl", "--repetition-penalty", "1.1"])
    assert script.prompts_of(a, Tok()) == [[7, 8, 9], [10]]
    assert (a.dtype, a.n, a.temperature, a.top_k, a.top_p, a.seed, a.jsonl, a.repetition_penalty) == ("fp32", 4, 0.8, 50, 0.9, 3, "out.jsonl", 1.1)
    for bad in (base, base + ["--prompt", "a", "--tokens", "1"], base + ["--prompt", "a", "--template", "t"], ["--prompt", "a"],
                base + ["--prompt", "a", "--dtype", "fp16"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    with pytest.raises(ValueError, match="--template"):
        script.prompts_of(p.parse_args(base + ["--prompt", "a", "--units", "1 2"]), Tok())
    with pytest.raises(ValueError, match="K=V"):
        script.template_variables(p.parse_args(base + ["--template", "t", "--var", "novalue"]))


def test_the_script_refuses_sampling_options_before_it_loads_anything(script, monkeypatch):
    def no_load(args):
        raise AssertionError("the checkpoint was loaded before the options were checked")

    monkeypatch.setattr(script, "load", no_load)
    base = ["--checkpoint-dir", "c", "--n-dsus", "100", "--prompt", "a"]
    for extra in (["-n", "4"], ["--top-k", "40"], ["--top-p", "0.9"], ["--temperature", "-1"], ["--units", "1 2"], ["--max-new-tokens", "0"]):
        with pytest.raises(ValueError):
            script.main(base + extra)
    with pytest.raises(AssertionError, match="loaded"):          # a valid call gets as far as loading
        script.main(base + ["-n", "4", "--temperature", "0.8", "--top-k", "40"])


def test_the_script_renders_a_template_from_its_options(script):
    pytest.importorskip("jinja2")
    from ssi.tokenizer import MODALITY_TOKEN_SPEECH, units_to_text
    a = script.build_parser().parse_args(["--checkpoint-dir", "c", "--n-dsus", "100", "--template", "{{ MODALITY_TOKEN_SPEECH }}{{ speech_units }} {{ k }}",
                                          "--units", "5,5 6", "--dedup", "--var", "k=a=b"])
    assert script.template_variables(a) == {"k": "a=b", "speech_units": [5, 5, 6]}
    assert script.prompts_of(a, Tok()) == [[1] + [ord(c) for c in MODALITY_TOKEN_SPEECH + units_to_text([5, 6]) + " a=b"]]


def test_the_script_prints_the_text_and_writes_the_records(script, monkeypatch, tmp_path, capsys):
    from ssi import generate as G
    from ssi import prompting as P
    monkeypatch.setattr(script, "load", lambda args: (object(), Tok(), {}))
    monkeypatch.setattr(P, "generate", lambda model, prompts, **kw: [G.Generation(token_ids=[ord("y"), 5], finish_reason="stop", stop_reason=5,
                                                                                  cumulative_logprob=-0.5, prompt_len=len(p)) for p in prompts])
    out = tmp_path / "p.jsonl"
    assert script.main(["--checkpoint-dir", "c", "--n-dsus", "100", "--prompt", "one", "--prompt", "two", "--jsonl", str(out)]) == 0
    assert capsys.readouterr().out == "y\ny\n"
    lines = [json.loads(l) for l in out.read_text().splitlines()]
    assert [l["id"] for l in lines] == [0, 1] and lines[1]["prompt"] == "two" and lines[0]["outputs"][0]["text"] == "y"
    assert all(set(l) == {"id", "prompt_token_ids", "prompt", "outputs"} for l in lines)
