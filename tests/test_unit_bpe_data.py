"""CPU: unit BPE in the data path.  With ``unit_bpe`` set, an SFT sample and every unit span of an interleaved CPT sample carry exactly the ids
of the encoded span (after deduplication, span by span); without the key the ids are those of today and nothing is imported; a mismatch
between ``speech.n_dsus`` and the merges file is refused with both numbers; the prompt template and ``scripts/unit_bpe.py`` (host side)."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

from conftest import PKG
from ssi.constants import SEED
from ssi.data import SFTDataset, TextCompletionDataset, get_span_idxs_binomial
from ssi.tokenizer import MODALITY_TOKEN_SPEECH, MODALITY_TOKEN_TEXT, deduplicate_units, dsu2pua, dump_tiktoken_bpe, setup_llama3_tokenizer, units_to_text

N_BASE = 50
MERGES = [(1, 2), (50, 3), (7, 7), (4, 5), (53, 6)]
N_UNITS = N_BASE + len(MERGES)
TEXT_MERGES = [b"th", b"he", b"the", b" t", b" the", b"in", b"\n\n", b"er", b"us", b"user", b"as", b"an", b"and", b" and"]
N_TXT = 256 + len(TEXT_MERGES)
UNIT0 = N_TXT
ID_TEXT, ID_SPEECH = N_TXT + N_UNITS, N_TXT + N_UNITS + 1
SYS = "You will act as an automatic speech recognition (ASR) system. "
IKW = {"sampling_rate": 16000, "downsampling_ratio": 320, "mean_seq_len_tokens": 5.0, "binom_prob": 0.4}


def ranks(n_units):
    """A tokenizer file as the test of the data pipeline writes one: bytes, a few text merges, one token per unit, the two modality tokens."""
    out = {bytes([i]): i for i in range(256)}
    for m in TEXT_MERGES:
        out[m] = len(out)
    for k in range(n_units):
        out[dsu2pua(k).encode()] = len(out)
    out[MODALITY_TOKEN_TEXT.encode()] = len(out)
    out[MODALITY_TOKEN_SPEECH.encode()] = len(out)
    return out


@pytest.fixture()
def tok(tmp_path):
    path = tmp_path / "tokenizer.model"
    dump_tiktoken_bpe(ranks(N_UNITS), path)
    return setup_llama3_tokenizer(path, max_seq_len=None, verbose=False)[0]


@pytest.fixture()
def bpe_file(tmp_path):
    from ssi.tokenizer.unit_bpe import UnitBPE
    path = tmp_path / "merges.json"
    UnitBPE(N_BASE, MERGES, [9, 8, 7, 6, 5]).save(path)
    return path


def by_hand(units):
    """MERGES applied in order, left to right, written out for these five."""
    out = list(units)
    for r, (a, b) in enumerate(MERGES):
        i, nxt = 0, []
        while i < len(out):
            if i + 1 < len(out) and (out[i], out[i + 1]) == (a, b):
                nxt.append(N_BASE + r)
                i += 2
            else:
                nxt.append(out[i])
                i += 1
        out = nxt
    return out


ROWS = [{"ID": f"utt{i}", "speech_tokens": [1, 1, 2, 3, 3, 7, 7, 7, 4, 5, 6, 6, (i % 5) + 10, 1, 2, 2, 3, 4, 4, 5, 6, 9, 1, 2], "transcript": "the user and the ant"}
        for i in range(6)]


def sft(tok, **kw):
    args = dict(source=ROWS, model_tokenizer=tok, deduplicate=True, use_modality_tokens=True, train_on_input=True,
                column_map={"input": "speech_tokens", "output": "transcript"}, new_system_prompt=SYS)
    args.update(kw)
    return SFTDataset(**args)


def unit_span(tokens):
    at = tokens.index(ID_SPEECH)
    return tokens[at + 1:tokens.index(ID_TEXT, at)]


def test_by_hand_is_the_host_encoder(bpe_file):
    from ssi.tokenizer.unit_bpe import UnitBPE
    bpe = UnitBPE.load(bpe_file)
    for units in ([1, 2, 3, 7, 7, 7, 4, 5, 6], [7] * 6, [1, 2, 3, 1, 2, 4, 5, 6, 4, 5], []):
        assert bpe.encode(units) == by_hand(units)
    assert by_hand([1, 2, 3, 7, 7, 7, 4, 5, 6]) == [51, 52, 7, 54]


def test_sft_sample_carries_the_encoded_span(tok, bpe_file):
    from ssi.tokenizer.unit_bpe import UnitBPE
    plain = sft(tok)
    for spec in (str(bpe_file), bpe_file, UnitBPE.load(bpe_file)):
        ds = sft(tok, unit_bpe=spec)
        for i in range(len(ROWS)):
            want = by_hand(deduplicate_units(ROWS[i]["speech_tokens"]))
            s, p = ds[i], plain[i]
            assert unit_span(s["tokens"]) == [UNIT0 + u for u in want]
            assert len(want) < len(unit_span(p["tokens"])) and any(u >= N_BASE for u in want)
            # everything around the span is as without the key
            a, b = s["tokens"].index(ID_SPEECH), p["tokens"].index(ID_SPEECH)
            assert s["tokens"][:a] == p["tokens"][:b] and s["tokens"][s["tokens"].index(ID_TEXT):] == p["tokens"][p["tokens"].index(ID_TEXT):]
            assert len(s["tokens"]) == len(s["labels"]) == len(s["mask"])
    # deduplication comes first, and without it the runs are encoded as they are
    nodedup = sft(tok, unit_bpe=bpe_file, deduplicate=False)[0]
    assert unit_span(nodedup["tokens"]) == [UNIT0 + u for u in by_hand(ROWS[0]["speech_tokens"])]
    inference = sft(tok, unit_bpe=bpe_file, inference=True)[2]["tokens"]          # what scripts/generate.py builds its prompts with
    assert unit_span(inference) == [UNIT0 + u for u in by_hand(deduplicate_units(ROWS[2]["speech_tokens"]))]


def test_without_the_key_nothing_changes_and_nothing_is_imported(tok):
    from ssi.config import OmegaConf
    from ssi.train_utils import resolve_n_dsus
    saved = sys.modules.pop("ssi.tokenizer.unit_bpe", None)
    try:
        for ds in (sft(tok), sft(tok, unit_bpe=None)):
            for i in range(len(ROWS)):
                assert unit_span(ds[i]["tokens"]) == [UNIT0 + u for u in deduplicate_units(ROWS[i]["speech_tokens"])]
                assert set(ds[i]) == {"tokens", "mask", "labels"}
        rows = cpt_rows()
        a = TextCompletionDataset(tok, rows, sequence_type="interleaved", deduplicate=True, use_modality_tokens=True, interleave_kwargs=IKW)
        b = TextCompletionDataset(tok, rows, sequence_type="interleaved", deduplicate=True, use_modality_tokens=True, interleave_kwargs=IKW, unit_bpe=None)
        assert [a[i] for i in range(len(rows))] == [b[i] for i in range(len(rows))]
        for speech in ({"n_dsus": N_UNITS}, {"n_dsus": N_UNITS, "unit_bpe": None}):
            cfg = OmegaConf.create({"speech": speech})
            resolve_n_dsus(cfg)
            assert cfg.speech.n_dsus == N_UNITS
        assert "ssi.tokenizer.unit_bpe" not in sys.modules
    finally:
        if saved is not None:
            sys.modules["ssi.tokenizer.unit_bpe"] = saved


def cpt_rows(n=6, words=30):
    rows = []
    for i in range(n):
        w = [("the", "user", "and", "hen", "ant")[(i + j) % 5] for j in range(words)]
        starts = [0.4 * j for j in range(words)]
        ends = [0.4 * j + 0.3 for j in range(words)]
        units = [(1, 2, 1, 2, 3, 4, 5, 6, 1, 2, 7)[(i + j // 2) % 11] for j in range(int(0.4 * words * 50) + 10)]   # 50 units per second
        rows.append({"tokenized": w, "aligned_start_times": starts, "aligned_end_times": ends, "speech_tokens": units})
    return rows


def test_interleaved_cpt_spans_are_encoded_one_by_one(tok, bpe_file):
    rows = cpt_rows()
    ds = TextCompletionDataset(tok, rows, sequence_type="interleaved", deduplicate=True, use_modality_tokens=True, interleave_kwargs=IKW, unit_bpe=bpe_file)
    crossed = 0
    for index, row in enumerate(rows):
        rng = np.random.default_rng((SEED, 0, index))                   # the sample's own draw, by hand: first the coin, then the span lengths
        start_with_text = bool(rng.choice([True, False], p=[0.5, 0.5]))
        spans = get_span_idxs_binomial(5, 0.4, len(row["tokenized"]), rng=rng)
        pieces, whole = [], []
        for k, (a, b) in enumerate(zip(spans[:-1], spans[1:])):
            if (k % 2 == 0) == start_with_text:
                pieces.append(MODALITY_TOKEN_TEXT + " " + " ".join(row["tokenized"][a:b]))
            else:
                lo, hi = int(row["aligned_start_times"][a] * 16000 / 320), int(row["aligned_end_times"][b - 1] * 16000 / 320)
                span = deduplicate_units(row["speech_tokens"][lo:hi])
                whole.append(span)
                pieces.append(MODALITY_TOKEN_SPEECH + " " + units_to_text(by_hand(span)))
        assert ds[index]["tokens"] == tok.encode(" ".join(pieces), add_bos=True, add_eos=True)
        joined = by_hand([u for span in whole for u in span])
        crossed += joined != [u for span in whole for u in by_hand(span)]
    assert crossed > 0      # encoding the utterance's units in one piece would have merged across a text boundary somewhere
    for seq_type in ("concatenated_txt_dsu", "concatenated_dsu_txt"):
        ds = TextCompletionDataset(tok, rows, sequence_type=seq_type, deduplicate=True, use_modality_tokens=True, unit_bpe=bpe_file)
        units = [t - UNIT0 for t in ds[1]["tokens"] if UNIT0 <= t < UNIT0 + N_UNITS]
        assert units == by_hand(deduplicate_units(rows[1]["speech_tokens"]))


def test_a_mismatch_between_n_dsus_and_the_file_is_refused(bpe_file):
    from ssi.config import OmegaConf
    from ssi.train_utils import resolve_n_dsus, validate_train_cfg
    base = {"dtype": "bf16", "gradient_accumulation_steps": 1, "max_steps": 1, "log_interval": 1, "eval_steps": 1, "save_steps": 1}
    for n_dsus in (N_BASE, N_UNITS + 1):
        cfg = OmegaConf.create({"speech": {"n_dsus": n_dsus, "unit_bpe": str(bpe_file)}, **base})
        for check in (resolve_n_dsus, validate_train_cfg):
            with pytest.raises(ValueError, match=rf"speech.n_dsus={n_dsus} .*{N_BASE} \+ {len(MERGES)} = {N_UNITS}"):
                check(cfg)
    cfg = OmegaConf.create({"speech": {"n_dsus": None, "unit_bpe": str(bpe_file)}, "data": {"n_dsus": N_BASE}, **base})
    with pytest.raises(ValueError, match=rf"speech.n_dsus={N_BASE} .*= {N_UNITS}"):      # the data config names the codebook, not the merged count
        resolve_n_dsus(cfg)
    cfg = OmegaConf.create({"speech": {"n_dsus": N_UNITS, "unit_bpe": str(bpe_file)}, **base})
    resolve_n_dsus(cfg)
    validate_train_cfg(cfg)


def test_committed_configuration_keeps_the_key_null():
    from ssi.config import OmegaConf
    common = OmegaConf.load(os.path.join(PKG, "conf", "common.yaml")) if hasattr(OmegaConf, "load") else None
    text = open(os.path.join(PKG, "conf", "common.yaml")).read()
    assert "  unit_bpe: null" in text and (common is None or common.speech.unit_bpe is None)
    for name in ("_sft_base.yaml", "_cpt_base.yaml"):
        lines = open(os.path.join(PKG, "conf", "data", name)).read().splitlines()
        assert sum(l.strip().startswith("# unit_bpe: ${speech.unit_bpe}") for l in lines) == 2 and not any(l.strip().startswith("unit_bpe") for l in lines)


def test_prompt_template_units_are_encoded(bpe_file):
    pytest.importorskip("jinja2")
    from ssi.prompting import render_template
    units = [1, 1, 2, 3, 7, 7, 7, 4, 5, 6]
    template = "{{ MODALITY_TOKEN_SPEECH }}{{ speech_units }}{{ MODALITY_TOKEN_TEXT }}"
    plain = render_template(template, {"speech_units": units}, deduplicate=True)
    assert plain == MODALITY_TOKEN_SPEECH + units_to_text(deduplicate_units(units)) + MODALITY_TOKEN_TEXT
    got = render_template(template, {"speech_units": units}, deduplicate=True, unit_bpe=str(bpe_file))
    assert got == MODALITY_TOKEN_SPEECH + units_to_text(by_hand(deduplicate_units(units))) + MODALITY_TOKEN_TEXT
    assert render_template(template, {"speech_units": units}, unit_bpe=bpe_file) == MODALITY_TOKEN_SPEECH + units_to_text(by_hand(units)) + MODALITY_TOKEN_TEXT


def script():
    spec = importlib.util.spec_from_file_location("unit_bpe_script", os.path.join(PKG, "scripts", "unit_bpe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_encode_and_stats_on_the_host(bpe_file, tmp_path, capsys):
    mod = script()
    data = tmp_path / "units.jsonl"
    data.write_text("\n".join(json.dumps(r) for r in ROWS) + "\n")
    out = tmp_path / "encoded.jsonl"
    mod.main(mod.parse_args(["encode", str(data), str(bpe_file), "--output", str(out), "--host"]))
    lines = [json.loads(l) for l in out.read_text().splitlines()]
    assert [l["speech_tokens"] for l in lines] == [by_hand(deduplicate_units(r["speech_tokens"])) for r in ROWS]
    assert [{k: v for k, v in l.items() if k != "speech_tokens"} for l in lines] == [{k: v for k, v in r.items() if k != "speech_tokens"} for r in ROWS]
    with pytest.raises(FileExistsError, match="not overwritten"):
        mod.main(mod.parse_args(["encode", str(data), str(bpe_file), "--output", str(out), "--host"]))
    nodedup = tmp_path / "nodedup.jsonl"
    mod.main(mod.parse_args(["encode", str(data), str(bpe_file), "--output", str(nodedup), "--host", "--no-dedup"]))
    assert json.loads(nodedup.read_text().splitlines()[0])["speech_tokens"] == by_hand(ROWS[0]["speech_tokens"])
    result = mod.main(mod.parse_args(["stats", str(data), str(bpe_file), "--host"]))
    before = sum(len(deduplicate_units(r["speech_tokens"])) for r in ROWS)
    after = sum(len(l["speech_tokens"]) for l in lines)
    assert (result["sequences"], result["ids_before"], result["ids_after"]) == (len(ROWS), before, after) and result["ratio"] == before / after > 1
    assert sum(result["lengths_before"].values()) == sum(result["lengths_after"].values()) == len(ROWS)
    # train refuses to overwrite before it reads anything
    with pytest.raises(FileExistsError, match="not overwritten"):
        mod.main(mod.parse_args(["train", str(data), "--n-base", "50", "--n-merges", "4", "--output", str(bpe_file)]))
    with pytest.raises(KeyError, match="units"):
        mod.main(mod.parse_args(["stats", str(data), str(bpe_file), "--host", "--column", "units"]))
