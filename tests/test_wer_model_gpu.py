"""GPU: the error rates end to end on the small model.  ``scripts/generate.py`` then ``scripts/wer.py`` (as ``test_seq_score_gpu`` drives
``scripts/score.py``): the counts in ``wer.json`` equal the Python restatement (``tests/edit_ref.py``) on the words of the written texts;
with ``gen.mbr`` the outputs are in risk order.  The trainer's ``eval_wer``: the only new keys of an evaluating step are ``dev_ter``,
``dev_wer`` and ``dev_wer_n``, ``dev_loss`` is bit-equal, and ``dev_ter`` equals the restatement on what ``generate`` returns for the same
prompts and weights.

The test configuration has no tokenizer file, so the vocabulary-layout tokenizer is given a ``decode`` and an ``encode`` over made-up words
(id ``t`` reads ``W<t mod 13>,``; the word ``w<k>`` encodes to ``k``): enough for texts with case and punctuation to normalise."""
import importlib.util
import json
import os

import pytest
import torch

import edit_ref

pytestmark = pytest.mark.gpu


def _word_tokenizer(monkeypatch):
    import ssi.tokenizer as T
    from ssi.tokenizer.layout import VocabLayoutTokenizer

    class WordTok(VocabLayoutTokenizer):
        eom_id = property(lambda self: self.special_tokens["<|eom_id|>"])
        eot_id = property(lambda self: self.special_tokens["<|eot_id|>"])

        def decode(self, ids, truncate_at_eos=True, skip_special_tokens=True):
            return " ".join(f"W{int(t) % 13}," for t in ids if int(t) < self.special_offset)

        def encode(self, text, add_bos=True, add_eos=False):
            return [self.bos_id] * bool(add_bos) + [int(w.strip(",").lower()[1:]) for w in text.split()] + [self.eos_id] * bool(add_eos)

    original = T.setup_llama3_tokenizer

    def setup(*args, **kw):
        tok, special = original(*args, **kw)
        tok.__class__ = WordTok
        return tok, special

    monkeypatch.setattr(T, "setup_llama3_tokenizer", setup)


def _script(name):
    from conftest import PKG
    spec = importlib.util.spec_from_file_location(f"{name}_script_wer_model", os.path.join(PKG, "scripts", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _generate_cfg(tmp_path, out, extra=()):
    from conftest import PKG
    from ssi.config import compose
    from test_trainer_gpu import SMALL
    cfg = compose(os.path.join(PKG, "conf"), "generate", [
        "speech.n_dsus=50", "dtype=fp32", "tokenizer.max_seq_len=96", f"output_dir={tmp_path}", f"checkpointer.checkpoint_dir={tmp_path}/none",
        "checkpointer.allow_random_init=true", f"gen.input={tmp_path}/prompts.jsonl", f"gen.output_dir={out}", "sampling_params.max_tokens=12",
        "gen.batch_size=8", *extra])
    cfg.model_overrides = dict(SMALL)
    return cfg


def _write_prompts(path, n=7, vocab=300):
    g = torch.Generator().manual_seed(21)
    with open(path, "w") as f:
        for k in range(n):
            f.write(json.dumps({"id": f"utt{k}", "prompt_tokens": torch.randint(0, vocab, (int(torch.randint(2, 20, (1,), generator=g)),),
                                                                                generator=g).tolist()}) + "\n")


def _restated(refs, hyps, normalizer="basic", level="word"):
    from ssi import wer
    rt, ht = [wer.normalize(t, normalizer) for t in refs], [wer.normalize(t, normalizer) for t in hyps]
    split = (lambda t: t.split()) if level == "word" else list
    counts = [edit_ref.edit_counts(split(r), split(h)) for r, h in zip(rt, ht)]
    n_ref = sum(len(split(r)) for r in rt)
    s, d, i = (sum(c[k] for c in counts) for k in (1, 2, 3))
    return {"wer": (s + d + i) / n_ref, "n_ref": n_ref, "substitutions": s, "deletions": d, "insertions": i, "hits": n_ref - s - d,
            "n_utterances": len(refs), "n_empty_refs": sum(1 for r in rt if not split(r))}


def test_generate_then_wer_scripts_end_to_end(tmp_path, monkeypatch):
    _word_tokenizer(monkeypatch)
    _write_prompts(tmp_path / "prompts.jsonl")
    out = tmp_path / "mls" / "dev"
    summary = _script("generate").main(_generate_cfg(tmp_path, out))
    assert summary["items"] == 7 and "mbr_changed" not in summary
    lines = [json.loads(x) for x in open(out / "generations.jsonl")]
    hyps = [x["outputs"][0]["text"] for x in lines]
    assert all("mbr_risk" not in o for x in lines for o in x["outputs"]) and any(hyps)
    # references: the written texts with words dropped, doubled and replaced, in another case and punctuation; one empty
    refs = []
    for k, text in enumerate(hyps):
        words = text.split()
        edited = [w for j, w in enumerate(words) if (j + k) % 5 != 1] + (["Extra!"] if k % 2 else [])
        refs.append(" ".join(w.upper().replace(",", ";") if j % 3 else "other" for j, w in enumerate(edited)) if k != 3 else "")
    with open(tmp_path / "refs.jsonl", "w") as f:
        for x, r in reversed(list(zip(lines, refs))):                          # matched by id, not by order
            f.write(json.dumps({"id": x["id"], "text": r}) + "\n")
    wer_script = _script("wer")
    for level in ("word", "char"):
        got = wer_script.main(wer_script.parse_args([str(out / "generations.jsonl"), "--references", str(tmp_path / "refs.jsonl"),
                                                     "--normalizer", "basic", "--level", level]))
        want = _restated(refs, hyps, level=level)
        written = json.loads((out / "wer.json").read_text())
        assert written == got and {k: got[k] for k in want} == want, (level, got, want)
        assert got["hits"] > 0 and got["substitutions"] > 0 and got["deletions"] + got["insertions"] > 0 and got["n_empty_refs"] == 1
        with pytest.raises(FileExistsError):
            wer_script.main(wer_script.parse_args([str(out / "generations.jsonl"), "--references", str(tmp_path / "refs.jsonl")]))
        os.remove(out / "wer.json")


def test_generate_script_with_mbr_writes_outputs_in_risk_order(tmp_path, monkeypatch):
    from ssi.generate import Generation, mbr_candidate
    _word_tokenizer(monkeypatch)
    _write_prompts(tmp_path / "prompts.jsonl")
    draw = ["gen.sample=true", "sampling_params.n=4", "sampling_params.temperature=0.9", "gen.seed=3"]
    plain = _script("generate").main(_generate_cfg(tmp_path, tmp_path / "plain", draw))
    mbr = _script("generate").main(_generate_cfg(tmp_path, tmp_path / "mbr", draw + ["gen.mbr=true"]))
    assert set(mbr) - set(plain) == {"mbr_changed"} and {k: mbr[k] for k in plain} == plain
    a = [json.loads(x) for x in open(tmp_path / "plain" / "generations.jsonl")]
    b = [json.loads(x) for x in open(tmp_path / "mbr" / "generations.jsonl")]
    changed = 0
    for x, y in zip(a, b):
        cands = [mbr_candidate(Generation(o["token_ids"], o["finish_reason"], o["stop_reason"], None, 0)) for o in x["outputs"]]
        order, risks = edit_ref.mbr_ref(cands)
        assert [o["index"] for o in y["outputs"]] == order and [o["mbr_risk"] for o in y["outputs"]] == [risks[k] for k in order]
        strip = lambda o: {k: v for k, v in o.items() if k != "mbr_risk"}   # noqa: E731
        assert [strip(o) for o in y["outputs"]] == [x["outputs"][k] for k in order]
        changed += order[0] != 0
    assert mbr["mbr_changed"] == changed


def _write_dev_items(path, texts):
    g = torch.Generator().manual_seed(33)
    prompts = [torch.randint(0, 300, (int(torch.randint(2, 16, (1,), generator=g)),), generator=g).tolist() for _ in range(6)]
    with open(path, "w") as f:
        for k, p in enumerate(prompts):
            n = int(torch.randint(0, 14, (1,), generator=g))
            ref = torch.randint(0, 13, (n,), generator=g).tolist()
            ref_item = {"reference": " ".join(f"w{t}" for t in ref)} if texts else {"reference_tokens": ref}
            f.write(json.dumps(dict({"id": k, "tokens": p}, **ref_item)) + "\n")
    return prompts


def test_trainer_logs_dev_error_rates_and_leaves_dev_loss_alone(tmp_path, monkeypatch):
    from ssi import wer
    from ssi.generate import generate, mbr_candidate
    from test_ce_metrics_gpu import _record_of_an_evaluating_step
    from test_trainer_gpu import SMALL, _trainer
    _word_tokenizer(monkeypatch)
    prompts = _write_dev_items(tmp_path / "dev_text.jsonl", texts=True)
    _write_dev_items(tmp_path / "dev_tokens.jsonl", texts=False)
    more = ["eval_wer_max_new_tokens=10"]
    off, _ = _record_of_an_evaluating_step(tmp_path, "off")
    on, _ = _record_of_an_evaluating_step(tmp_path, "on", extra=[f"eval_wer={tmp_path}/dev_text.jsonl", *more])
    ids_only, _ = _record_of_an_evaluating_step(tmp_path, "ids", extra=[f"eval_wer={tmp_path}/dev_tokens.jsonl", *more])
    assert set(on) - set(off) == {"dev_ter", "dev_wer", "dev_wer_n"} and not set(off) - set(on)
    assert set(ids_only) - set(off) == {"dev_ter", "dev_wer_n"}                # no text, no word error rate
    assert on["dev_loss"] == off["dev_loss"] == ids_only["dev_loss"]          # bit for bit
    assert on["dev_wer_n"] == ids_only["dev_wer_n"] == 6
    # the restatement on what generate returns for the same prompts and weights (lr 0: the step left the seeded weights as they were)
    t = _trainer(tmp_path, "again", model=SMALL, overrides=["optimizer.lr=0.0"])
    tok = t.tokenizer
    found = generate(t.model, prompts, max_new_tokens=10, stop_token_ids=[tok.eom_id, tok.eot_id, tok.eos_id], pad_id=tok.pad_id)
    t.cleanup()
    hyps = [mbr_candidate(g) for g in found]
    for path, rec in ((tmp_path / "dev_text.jsonl", on), (tmp_path / "dev_tokens.jsonl", ids_only)):
        items = [json.loads(x) for x in open(path)]
        refs = [x["reference_tokens"] if "reference_tokens" in x else tok.encode(x["reference"], add_bos=False) for x in items]
        counts = [edit_ref.edit_counts(r, h) for r, h in zip(refs, hyps)]
        assert rec["dev_ter"] == sum(c[0] for c in counts) / sum(len(r) for r in refs)
    want = _restated([x["reference"] for x in map(json.loads, open(tmp_path / "dev_text.jsonl"))], [tok.decode(h) for h in hyps])
    assert on["dev_wer"] == want["wer"] and wer.normalize(tok.decode([5, 18]), "basic") == "w5 w5"
