"""CPU: the host side of the decode penalties — the ABI number, the prototypes and their argument counts against the header, the wrapper's LDS
formula, ``check_penalties`` and the script's switch (every refusal without ``gen.penalties`` is what it was; acceptance with it; the beam
refusal), the refusals of ``generate`` / ``sample`` / ``beam_search`` before any launch, and — with a stubbed ``ops`` — that neutral penalties
reach neither penalised wrapper nor build a prompt table while a set penalty takes the penalised kernel for every step's token."""
import importlib.util
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "speech-integration_amd")


def test_the_abi_names_the_entries():
    from ssi import _lib, ops
    header = open(os.path.join(ROOT, "include", "ssi_hip.h")).read()
    assert int(re.search(r"#define SSI_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 22
    assert re.search(r"22: \+ ssi_decode_select_pen, ssi_decode_sample_pen", header)
    for name, count, plain in (("ssi_decode_select_pen", 24, "ssi_decode_select"), ("ssi_decode_sample_pen", 30, "ssi_decode_sample")):
        args = re.search(rf"\bint {name}\((.*?)\);", header, re.S).group(1)
        assert len(args.split(",")) == len(_lib.PROTOTYPES[name][1]) == count
        assert len(_lib.PROTOTYPES[name][1]) == len(_lib.PROTOTYPES[plain][1]) + 11        # the same trailing block on both
        head = len(_lib.PROTOTYPES[plain][1]) - 2
        assert _lib.PROTOTYPES[name][1][:head] == _lib.PROTOTYPES[plain][1][:head]          # the plain entry's arguments up to its last output
        assert name[4:] in ops.__all__ and callable(getattr(ops, name[4:]))
    assert _lib.PROTOTYPES["ssi_decode_select"][1] == _lib.PROTOTYPES["ssi_decode_select"][1] and len(_lib.PROTOTYPES["ssi_decode_select"][1]) == 13
    assert len(_lib.PROTOTYPES["ssi_decode_sample"][1]) == 19 and len(_lib.PROTOTYPES["ssi_topk_logprob"][1]) == 12
    assert int(re.search(r"#define SSI_DECODE_PENALTY_LDS_MAX (\d+)", header).group(1)) == _lib.DECODE_PENALTY_LDS_MAX == 57344
    assert "ssi_decode_penalty_lds_bytes" in _lib.PROTOTYPES and "decode_penalty_lds_bytes" in ops.__all__
    lib = _lib.load()
    for vocab, ld_gen in ((1, 0), (32, 1), (33, 32), (33, 33), (2049, 257), (133_376, 256), (133_376, 4096)):
        assert ops.decode_penalty_lds_bytes(vocab, ld_gen) == lib.ssi_decode_penalty_lds_bytes(vocab, ld_gen)
    assert ops.decode_penalty_lds_bytes(133_376, 256) == 20_768


def test_the_wrappers_refuse_cpu_tensors():
    from ssi import _lib, ops
    kw = dict(prompt_ids=None, prompt_len=torch.zeros(3, dtype=torch.int32), gen_ids=None, n_generated=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(_lib.HipLibraryError, match="GPU"):
        ops.decode_select_pen(torch.zeros(3, 32), 30, torch.zeros(3, dtype=torch.int64), **kw)
    with pytest.raises(_lib.HipLibraryError, match="GPU"):
        ops.decode_sample_pen(torch.zeros(3, 32), 30, torch.zeros(3, dtype=torch.int64), temperature=1.0, seed=0, step=0,
                              sequence=torch.zeros(3, dtype=torch.int32), **kw)


def test_check_penalties():
    from ssi.generate import check_greedy, check_penalties, check_sampling
    assert check_penalties({}) == {"repetition_penalty": 1.0, "frequency_penalty": 0.0, "presence_penalty": 0.0}
    got = check_penalties({"repetition_penalty": 1.2, "frequency_penalty": -2, "presence_penalty": 2.0, "temperature": 0.8, "n": 3, "max_tokens": 5})
    assert got == {"repetition_penalty": 1.2, "frequency_penalty": -2.0, "presence_penalty": 2.0}
    for bad in ({"repetition_penalty": 0}, {"repetition_penalty": -1.0}, {"repetition_penalty": math.inf}, {"repetition_penalty": math.nan},
                {"repetition_penalty": "1.2"}, {"repetition_penalty": True}, {"frequency_penalty": 2.5}, {"frequency_penalty": -2.5},
                {"frequency_penalty": math.nan}, {"presence_penalty": 2.5}, {"presence_penalty": -2.5}, {"presence_penalty": math.inf}):
        with pytest.raises(ValueError, match=f"sampling_params.{next(iter(bad))}"):
            check_penalties(bad)
    for key, value in (("presence_penalty", 0.1), ("frequency_penalty", 0.1), ("repetition_penalty", 1.1)):      # the two checks are what they were
        with pytest.raises(NotImplementedError, match=key):
            check_greedy({key: value})
        with pytest.raises(NotImplementedError, match=key):
            check_sampling({"temperature": 0.8, key: value})


def _script():
    spec = importlib.util.spec_from_file_location("generate_script", os.path.join(PKG, "scripts", "generate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_configuration_and_the_scripts_switch(monkeypatch):
    from ssi.config import compose
    conf, base = os.path.join(PKG, "conf"), ["speech.n_dsus=5000", "gen.output_dir=/nonexistent/out"]
    cfg = compose(conf, "generate", base)
    assert cfg.gen.penalties is False
    mod = _script()
    pens = ["sampling_params.repetition_penalty=1.2", "sampling_params.frequency_penalty=0.5"]
    with pytest.raises(NotImplementedError, match="_penalty = "):                             # without the switch: refused as before
        mod.main(compose(conf, "generate", base + pens))
    with pytest.raises(NotImplementedError, match="_penalty = "):
        mod.main(compose(conf, "generate", base + pens + ["gen.sample=true", "sampling_params.temperature=0.8"]))
    with pytest.raises(NotImplementedError, match="repetition_penalty"):
        mod.main(compose(conf, "generate", base + pens[:1] + ["gen.penalties=false"]))
    with pytest.raises(ValueError, match="beam_width"):
        mod.main(compose(conf, "generate", base + pens + ["gen.penalties=true", "gen.beam_width=4"]))
    with pytest.raises(ValueError, match="repetition_penalty"):
        mod.main(compose(conf, "generate", base + ["gen.penalties=true", "sampling_params.repetition_penalty=0"]))
    with pytest.raises(ValueError, match="presence_penalty"):
        mod.main(compose(conf, "generate", base + ["gen.penalties=true", "sampling_params.presence_penalty=3"]))
    with pytest.raises(NotImplementedError, match="temperature"):                             # the rest goes to check_greedy unchanged
        mod.main(compose(conf, "generate", base + pens + ["gen.penalties=true", "sampling_params.temperature=0.8"]))
    with pytest.raises(ValueError, match="n = "):                                             # ... or to check_sampling
        mod.main(compose(conf, "generate", base + pens + ["gen.penalties=true", "gen.sample=true", "sampling_params.temperature=0.8",
                                                          "sampling_params.n=9"]))
    assert not os.path.exists("/nonexistent/out")

    class Accepted(Exception):
        pass

    def loaded(*a, **k):                                    # the first thing after the checks: the switch let the penalties through
        raise Accepted

    import ssi.train_utils
    monkeypatch.setattr(ssi.train_utils, "resolve_n_dsus", loaded)
    for extra in ([], ["gen.sample=true", "sampling_params.temperature=0.8", "sampling_params.n=2"]):
        with pytest.raises(Accepted):
            mod.main(compose(conf, "generate", base + pens + ["gen.penalties=true"] + extra))


class _Stub:
    """A model on which any use beyond the host checks fails."""
    vocab_size, training = 100, False
    device = torch.device("cpu")

    def check_generation_lengths(self, lens, max_new_tokens, n_slots, cap):
        pass

    def __getattr__(self, name):
        raise AssertionError(f"the model was used ({name}) before the refusal")


def test_the_refusals_come_before_any_launch():
    from ssi.generate import beam_search, generate, sample
    g = dict(max_new_tokens=4, stop_token_ids=[7], pad_id=0)
    for bad, match in ((dict(repetition_penalty=0.0), "repetition_penalty"), (dict(repetition_penalty=-1), "repetition_penalty"),
                       (dict(repetition_penalty=math.nan), "repetition_penalty"), (dict(repetition_penalty=math.inf), "repetition_penalty"),
                       (dict(frequency_penalty=2.1), "frequency_penalty"), (dict(frequency_penalty=-2.1), "frequency_penalty"),
                       (dict(presence_penalty=2.1), "presence_penalty"), (dict(presence_penalty="0"), "presence_penalty")):
        with pytest.raises(ValueError, match=match):
            generate(_Stub(), [[1, 2]], **g, **bad)
        with pytest.raises(ValueError, match=match):
            sample(_Stub(), [[1, 2]], temperature=0.8, seed=1, **g, **bad)
        with pytest.raises(ValueError, match=match):
            beam_search(_Stub(), [[1, 2]], beam_width=2, **g, **bad)
    for pen in (dict(repetition_penalty=1.3), dict(frequency_penalty=0.5), dict(presence_penalty=-0.5)):
        with pytest.raises(ValueError, match="beam search"):
            beam_search(_Stub(), [[1, 2]], beam_width=2, **g, **pen)


class _Cache:
    errors = 0


class _Model:
    """Just enough of the decoder for the loops on the CPU: logits that prefer token (last + 1) % V, then (last + 2) % V."""
    vocab_size, training = 16, False
    device = torch.device("cpu")

    def check_generation_lengths(self, *a):
        pass

    def eval(self):
        pass

    def new_kv_cache(self, n_slots, cap):
        return _Cache()

    def _logits(self, last):
        x = torch.zeros(last.numel(), 16)
        x[torch.arange(last.numel()), (last + 1) % 16] = 2.0
        x[torch.arange(last.numel()), (last + 2) % 16] = 1.0
        return x

    def prefill(self, cache, seqs, max_new_tokens=None):
        return self._logits(torch.tensor([int(s[-1]) for s in seqs]))

    def decode_step(self, cache, tok, slot):
        return self._logits(tok)

    def decode_step_beam(self, pcache, bcache, tok, slot, plen, anc, t):
        return self._logits(tok)


def _stub_ops(monkeypatch, calls):
    """``ops`` whose selection wrappers record their call and answer on the CPU: the plain ones the first maximum, the penalised ones the
    SECOND column by value (so a penalised step shows in the tokens)."""
    from ssi import generate as G

    def pick(logits, vocab, token, second):
        order = logits[:, :vocab].argsort(dim=1, descending=True, stable=True)
        token.copy_(order[:, 1 if second else 0])

    def decode_select(logits, vocab, token, logprob=None, rank=None, **kw):
        calls.append(("decode_select", kw))
        pick(logits, vocab, token, False)
        rank.zero_()

    def decode_select_pen(logits, vocab, token, logprob=None, rank=None, **kw):
        calls.append(("decode_select_pen", kw))
        pick(logits, vocab, token, True)
        rank.fill_(1)
        if logprob is not None:
            logprob.fill_(-0.5)

    def decode_sample(logits, vocab, token, logprob, n_kept, **kw):
        calls.append(("decode_sample", kw))
        pick(logits, vocab, token, False)
        logprob.fill_(-1.0)
        n_kept.fill_(3)

    def decode_sample_pen(logits, vocab, token, logprob, n_kept, **kw):
        calls.append(("decode_sample_pen", kw))
        pick(logits, vocab, token, True)
        logprob.fill_(-1.0)
        n_kept.fill_(3)

    for name, fn in (("decode_select", decode_select), ("decode_select_pen", decode_select_pen), ("decode_sample", decode_sample),
                     ("decode_sample_pen", decode_sample_pen)):
        monkeypatch.setattr(G.ops, name, fn)
    built = []
    real = G._prompt_table
    monkeypatch.setattr(G, "_prompt_table", lambda seqs, dev: built.append(len(seqs)) or real(seqs, dev))
    return built


def test_neutral_penalties_reach_no_penalised_wrapper_and_build_no_prompt_table(monkeypatch):
    from ssi import generate as G
    calls = []
    built = _stub_ops(monkeypatch, calls)
    kw = dict(max_new_tokens=3, stop_token_ids=[15], pad_id=0)
    neutral = dict(repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0)
    plain = G.generate(_Model(), [[1], [4, 5]], **kw)
    assert G.generate(_Model(), [[1], [4, 5]], **kw, **neutral) == plain and [g.token_ids for g in plain] == [[2, 3, 4], [6, 7, 8]]
    assert not calls and not built and plain[0].n_constrained is None                      # argmax: no selection kernel at all
    G.generate(_Model(), [[1], [4, 5]], min_new_tokens=1, **kw, **neutral)
    G.sample(_Model(), [[1], [4, 5]], temperature=0.8, seed=3, **kw, **neutral)
    G.sample(_Model(), [[1], [4, 5]], n=2, temperature=0.8, seed=3, **kw, **neutral)
    assert {name for name, _ in calls} == {"decode_select", "decode_sample"} and not built


def test_a_set_penalty_takes_the_penalised_kernel_for_every_token(monkeypatch):
    from ssi import generate as G
    calls = []
    built = _stub_ops(monkeypatch, calls)
    kw = dict(max_new_tokens=3, stop_token_ids=[15], pad_id=0)
    got = G.generate(_Model(), [[1], [4, 5]], repetition_penalty=1.3, frequency_penalty=0.5, logprobs=True, **kw)
    assert [g.token_ids for g in got] == [[3, 5, 7], [7, 9, 11]]                           # the stub's second choice at every step
    assert [g.n_constrained for g in got] == [3, 3] and [g.cumulative_logprob for g in got] == [-1.5, -1.5]
    assert [name for name, _ in calls] == ["decode_select_pen"] * 3 and built == [2]     # one table per group
    first = calls[0][1]
    assert first["repetition_penalty"] == 1.3 and first["frequency_penalty"] == 0.5 and first["presence_penalty"] == 0.0
    assert "allow" not in first and first["n_generated"].dtype == torch.int32 and first["gen_ids"].dtype == torch.int64      # NULL masks
    assert first["prompt_ids"].dtype == torch.int32 and first["prompt_ids"].tolist() == [[1, 0], [4, 5]] and first["prompt_len"].tolist() == [1, 2]
    assert calls[2][1]["gen_ids"][:, :2].tolist() == [[3, 5], [7, 9]] and calls[2][1]["n_generated"].tolist() == [3, 3]      # (the loop's own tensors)
    del calls[:], built[:]
    G.generate(_Model(), [[1]], presence_penalty=0.1, min_new_tokens=2, **kw)
    assert [name for name, _ in calls] == ["decode_select_pen"] * 3 and calls[0][1]["min_new"] == 2 and calls[0][1]["allow"] is not None
    del calls[:], built[:]
    got = G.sample(_Model(), [[1], [4, 5]], n=2, temperature=0.8, seed=3, presence_penalty=-0.5, **kw)
    assert [name for name, _ in calls] == ["decode_sample_pen"] * 3 and built == [2]
    assert calls[0][1]["prompt_row"].tolist() == [0, 0, 1, 1] and calls[0][1]["prompt_ids"].shape == (2, 2)     # a prompt's samples share its line
    assert [[g.token_ids for g in gs] for gs in got] == [[[3, 5, 7]] * 2, [[7, 9, 11]] * 2]


def test_generate_file_reports_the_penalties(tmp_path, monkeypatch):
    from ssi import generate as G

    class Tok:
        special_tokens = {}
        eos_id, eom_id, eot_id, pad_id = 901, 908, 909, 904

        def decode(self, ids, **kw):
            return ""

    seen = {}

    def fake(model, prompts, **kw):
        seen.update(kw)
        return [G.Generation([5, 909], "stop", 909, None, len(p), n_constrained=1) for p in prompts]

    monkeypatch.setattr(G, "generate", fake)
    summary = G.generate_file(object(), Tok(), None, str(tmp_path / "g.jsonl"), max_new_tokens=4, prompts=[[1], [2]], repetition_penalty=1.2,
                              frequency_penalty=0.0, presence_penalty=0.5)
    assert summary == {"items": 2, "generated_tokens": 4, "stopped": 2, "constrained_tokens": 2, "repetition_penalty": 1.2,
                       "frequency_penalty": 0.0, "presence_penalty": 0.5}
    assert seen["repetition_penalty"] == 1.2 and seen["presence_penalty"] == 0.5
    summary = G.generate_file(object(), Tok(), None, str(tmp_path / "g.jsonl"), max_new_tokens=4, prompts=[[1], [2]])
    assert summary == {"items": 2, "generated_tokens": 4, "stopped": 2}
