"""CPU: the host side of the error rates (``ssi/wer.py``, ``scripts/wer.py``) and of MBR selection: the "basic" normaliser, ``word_ids``, the
aggregation from counts, the files the script reads, its refusal to overwrite ``wer.json``, the refusals of ``mbr`` with one candidate, and the
ABI number."""
import importlib.util
import json
import os
import re

import pytest

from conftest import PKG, ROOT
from ssi import wer


@pytest.mark.parametrize("text,want", [
    ("Hello, World!", "hello world"),
    ("  two\t spaces\nand a line ", "two spaces and a line"),
    ("don't — stop…", "don t stop"),
    ("ＦＵＬＬ width ①", "full width 1"),                    # NFKC: compatibility forms fold
    ("ﬁne ligature", "fine ligature"),
    ("Ünïcode ÉCOLE", "ünïcode école"),
    ("cost: $5 + 3€ = ?", "cost 5 3"),
    ("«quoted» (text) [here]", "quoted text here"),
    ("", ""),
    ("?!...", ""),
])
def test_the_basic_normaliser(text, want):
    assert wer.normalize(text, "basic") == want
    assert wer.normalize(wer.normalize(text, "basic"), "basic") == want          # idempotent


def test_the_other_normalisers():
    assert wer.normalize("As It, Is!", "none") == "As It, Is!" and wer.normalize("As It, Is!", None) == "As It, Is!"
    with pytest.raises(ValueError, match="normalizer"):
        wer.normalize("x", "other")
    try:
        import whisper_normalizer  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="whisper_normalizer.*basic"):
            wer.normalize("x", "whisper")
    else:
        assert wer.normalize("Hello, World!", "whisper") == "hello world"
    assert "NFKC" in wer.normalize.__doc__ and "lower case" in wer.normalize.__doc__


def test_word_ids_share_one_dictionary():
    refs, hyps = wer.word_ids(["a b a", "", "c"], ["b a d", "c", ""])
    assert refs == [[0, 1, 0], [], [2]] and hyps == [[1, 0, 3], [2], []]
    assert wer.word_ids([], []) == ([], [])


def test_aggregate_from_counts():
    got = wer.aggregate([[2, 1, 1, 0], [3, 0, 0, 3], [0, 0, 0, 0]], [4, 0, 5])
    assert got == {"wer": 5 / 9, "n_ref": 9, "substitutions": 1, "deletions": 1, "insertions": 3, "hits": 7, "n_utterances": 3, "n_empty_refs": 1}
    none = wer.aggregate([[2, 0, 0, 2]], [0])
    assert none["wer"] is None and none["n_ref"] == 0 and none["insertions"] == 2 and none["n_empty_refs"] == 1
    assert wer.aggregate([], [])["wer"] is None and wer.aggregate([], [])["n_utterances"] == 0
    with pytest.raises(ValueError):
        wer.aggregate([[1, 1, 0, 0]], [1, 2])
    with pytest.raises(ValueError, match="refused"):
        wer.aggregate([[-1, -1, -1, -1]], [3])
    json.dumps(none)                                                         # no NaN: the result is plain JSON


def test_error_rate_refuses_on_the_host():
    with pytest.raises(ValueError, match="level"):
        wer.error_rate(["a"], ["a"], level="phone")
    with pytest.raises(ValueError, match="references"):
        wer.error_rate(["a", "b"], ["a"])
    from ssi import _lib
    with pytest.raises(ValueError, match=str(_lib.EDIT_MAX_LEN)):
        wer.edit_counts([[0] * (_lib.EDIT_MAX_LEN + 1)], [[0]], "cpu")
    with pytest.raises(_lib.HipLibraryError):                               # CPU tensors are refused through the library, as every op
        wer.edit_counts([[1, 2]], [[1]], "cpu")


def test_reference_files(tmp_path):
    (tmp_path / "r.jsonl").write_text("\n".join(json.dumps(x) for x in (
        {"id": "b", "text": "second"}, {"id": "a", "transcript": "first"}, {"id": "c", "col": "third"})) + "\n")
    assert wer.read_references(str(tmp_path / "r.jsonl"), ["a", "b", "c"], column="col") == ["first", "second", "third"]
    with pytest.raises(ValueError, match="no reference"):
        wer.read_references(str(tmp_path / "r.jsonl"), ["a", "z"], column="col")
    (tmp_path / "r.txt").write_text("one\n\nthree\n")
    assert wer.read_references(str(tmp_path / "r.txt"), [0, 1, 2]) == ["one", "", "three"]
    with pytest.raises(ValueError, match="lines"):
        wer.read_references(str(tmp_path / "r.txt"), [0, 1])
    (tmp_path / "g.jsonl").write_text(json.dumps({"id": 7, "outputs": [{"text": "best"}, {"text": "other"}]}) + "\n")
    assert wer.read_generations(str(tmp_path / "g.jsonl")) == ([7], ["best"])


@pytest.fixture(scope="module")
def script():
    spec = importlib.util.spec_from_file_location("wer_script", os.path.join(PKG, "scripts", "wer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_script_takes_the_reference_arguments_and_two_of_its_own(script):
    args = script.parse_args(["d/s/generations.jsonl"])
    assert (args.dataset, args.split, args.gt_transcript_colname, args.normalizer, args.references, args.level) == \
           (None, None, "transcript", "whisper", None, "word")
    args = script.parse_args(["g.jsonl", "--dataset", "mls", "--split", "dev", "--gt_transcript_colname", "t", "--normalizer", "basic",
                              "--references", "r.txt", "--level", "char"])
    assert (args.dataset, args.split, args.gt_transcript_colname, args.normalizer, str(args.references), args.level) == \
           ("mls", "dev", "t", "basic", "r.txt", "char")


def test_the_script_refuses_to_overwrite_wer_json(script, tmp_path):
    (tmp_path / "generations.jsonl").write_text(json.dumps({"id": 0, "outputs": [{"text": "a"}]}) + "\n")
    (tmp_path / "wer.json").write_text(json.dumps({"wer": 0.25}))
    with pytest.raises(FileExistsError, match="0.25"):
        script.main(script.parse_args([str(tmp_path / "generations.jsonl"), "--references", str(tmp_path / "none.txt")]))
    assert json.loads((tmp_path / "wer.json").read_text()) == {"wer": 0.25}


def test_mbr_is_refused_with_one_candidate():
    from ssi import generate as G
    kw = dict(max_new_tokens=4, stop_token_ids=[1], pad_id=0)
    with pytest.raises(ValueError, match="mbr=True needs at least two candidates"):
        G.sample(object(), [[5]], n=1, temperature=0.8, seed=0, mbr=True, **kw)
    with pytest.raises(ValueError, match="mbr=True needs at least two candidates"):
        G.beam_search(object(), [[5]], beam_width=4, n_best=1, mbr=True, **kw)
    with pytest.raises(ValueError, match="True or False"):
        G.sample(object(), [[5]], n=2, temperature=0.8, seed=0, mbr=1, **kw)
    with pytest.raises(ValueError, match="at least two candidates"):
        G.mbr_select([[[1, 2], [1]], [[3]]], "cpu")
    assert G.mbr_select([], "cpu") == ([], [])
    assert G.Generation([1], "stop", 1, None, 1).mbr_risk is None
    import dataclasses
    assert "mbr_risk" not in dataclasses.asdict(G.Generation([1], "stop", 1, None, 1))     # recorded Generations stay what they were
    assert G.mbr_candidate(G.Generation([4, 5, 1], "stop", 1, None, 1)) == [4, 5] and G.mbr_candidate(G.Generation([4, 5], "length", None, None, 1)) == [4, 5]


def test_the_configuration_and_the_scripts_switch():
    from ssi.config import compose
    conf = os.path.join(PKG, "conf")
    base = ["speech.n_dsus=5000", "gen.output_dir=/nonexistent/out"]
    assert compose(conf, "generate", base).gen.mbr is False
    sft = compose(conf, "sft", ["data=sft/mls-hubert_large_ll60k-layer_22"])
    assert sft.eval_wer is None and sft.eval_wer_max_new_tokens == 256
    spec = importlib.util.spec_from_file_location("generate_script_mbr", os.path.join(PKG, "scripts", "generate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for extra in ([], ["gen.sample=true", "sampling_params.temperature=0.8"], ["gen.beam_width=4"]):      # one candidate per prompt
        with pytest.raises(ValueError, match="gen.mbr=true needs candidates"):
            mod.main(compose(conf, "generate", base + ["gen.mbr=true"] + extra))
    spec = importlib.util.spec_from_file_location("prompt_script_mbr", os.path.join(PKG, "scripts", "prompt.py"))
    prompt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(prompt)
    with pytest.raises(ValueError, match="--mbr"):
        prompt.main(["--checkpoint-dir", "c", "--n-dsus", "100", "--prompt", "x", "--mbr"])


def test_header_and_lib_agree_on_the_abi():
    from ssi import _lib
    header = open(os.path.join(ROOT, "include", "ssi_hip.h")).read()
    assert int(re.search(r"#define SSI_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 29
    assert int(re.search(r"#define SSI_EDIT_MAX_LEN (\d+)", header).group(1)) == _lib.EDIT_MAX_LEN
    assert int(re.search(r"#define SSI_EDIT_COLS (\d+)", header).group(1)) == _lib.EDIT_COLS
    assert {"ssi_edit_distance", "ssi_edit_distance_workspace_bytes"} <= set(_lib.PROTOTYPES)
