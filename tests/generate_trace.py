"""What the generation loops launch and what they return: every call into ``ssi.ops`` of ``generate``, ``sample`` and ``beam_search`` over a fixed
set of scenarios (``launch_trace.Tracer``; the K/V caches a call makes are watched as ``cache.*``), and every field of every ``Generation``.

The model is ``launch_trace.MFMA_PARAMS`` with one layer, bf16, seeded, in ``eval`` mode (the stack's own launches are pinned by
tests/test_decoder_launch_trace_gpu.py; ``takes_small_batch`` needs the MFMA shapes).  Five seeded prompts of 5, 17, 1, 9 and 3 tokens,
``pad_id=0``, ``stop_token_ids=[3, 11]`` and ``max_new_tokens=3`` unless the scenario says otherwise.  Only ``ssi.ops``, the model's
``new_kv_cache`` and the public API of ``ssi.generate`` are touched, so the same file records on any commit.

``run_all()`` returns ``{"traces": {scenario: entries}, "results": {scenario: ...}}``; floats go as ``float.hex()``.
``python tests/generate_trace.py OUT.json`` writes that as JSON: ``entries`` holds every distinct trace entry once, one per line (the decode
steps of a group repeat theirs), and a scenario's trace is a list of indices into it — ``load`` undoes that.
tests/golden/generate_loop_trace.json is such a file, recorded at the commit before the loops were folded into one;
tests/test_generate_loop_trace_gpu.py holds the code to it."""
import dataclasses
import json
import os
import sys

import torch

PROMPT_SEED = 0
PROMPT_LENS = (5, 17, 1, 9, 3)
SAMPLING = dict(temperature=0.8, top_k=50, top_p=0.9, seed=7)
ALLOWED = range(100, 400)
GREEDY, SAMPLE_N3, BEAM = dict(batch_size=4), dict(n=3, batch_size=7, min_new_tokens=2), dict(beam_width=3, n_best=2, batch_size=7, min_new_tokens=1,
                                                                                              allowed_token_ids=ALLOWED)
# scenario: (entry point, its arguments beside the defaults)
SCENARIOS = {
    "greedy": ("generate", dict(GREEDY, max_new_tokens=9)),                              # groups of 4 and 1; a read-back passes and a step follows it
    "greedy.logprobs": ("generate", dict(logprobs=True)),
    "greedy.constrained": ("generate", dict(allowed_token_ids=ALLOWED, min_new_tokens=2, logprobs=True)),
    "greedy.min_new_only": ("generate", dict(min_new_tokens=2)),
    "greedy.penalised": ("generate", dict(repetition_penalty=1.3, frequency_penalty=0.5, presence_penalty=-0.5, logprobs=True)),
    "greedy.penalised.constrained": ("generate", dict(presence_penalty=0.1, min_new_tokens=2)),
    "greedy.early_end": ("generate", dict(stop_token_ids=range(0, 350), max_new_tokens=20)),  # every row stops early: the group ends at a read-back
    "sample.n1": ("sample", dict(SAMPLING)),
    "sample.n3": ("sample", dict(SAMPLING, **SAMPLE_N3, max_new_tokens=9)),             # two prompts per group
    "sample.n3.penalised": ("sample", dict(SAMPLING, n=3, repetition_penalty=1.2)),
    "beam": ("beam_search", dict(BEAM)),
    "small_batch.greedy": ("generate", dict(GREEDY, small_batch=True)),
    "small_batch.sample.n3": ("sample", dict(SAMPLING, **SAMPLE_N3, small_batch=True)),
    "small_batch.beam": ("beam_search", dict(BEAM, small_batch=True)),
}


def _record(gen):
    d = dataclasses.asdict(gen)
    return {k: v.hex() if isinstance(v, float) else v for k, v in d.items()}


def _records(found):
    return [_record(g) if dataclasses.is_dataclass(g) else [_record(h) for h in g] for g in found]


def run_all(prompt_seed=PROMPT_SEED, only=None):
    import launch_trace
    from ssi import generate as G
    tr = launch_trace.Tracer()
    model = tr.watch(launch_trace._model(dict(launch_trace.MFMA_PARAMS, num_layers=1), 31, torch.bfloat16))
    model.eval()
    new_kv_cache = model.new_kv_cache

    def watched_cache(n_slots, cap):
        cache = new_kv_cache(n_slots, cap)
        tr.caches.append(cache)
        return cache

    model.new_kv_cache = watched_cache
    g = torch.Generator().manual_seed(prompt_seed)
    prompts = [torch.randint(0, launch_trace.MFMA_PARAMS["vocab_size"], (n,), generator=g) for n in PROMPT_LENS]
    traces, results = {}, {}
    for name, (entry, args) in SCENARIOS.items():
        if only is not None and name not in only:
            continue
        kw = dict(dict(max_new_tokens=3, stop_token_ids=[3, 11], pad_id=0), **args)
        report = {} if kw.get("small_batch") else None
        if report is not None:
            kw["small_batch_report"] = report
        with tr.scenario():
            found = getattr(G, entry)(model, prompts, **kw)
        traces[name], results[name] = tr.entries, {"generations": _records(found)}
        if report is not None:
            results[name]["small_batch_report"] = report
        if name == "greedy.early_end":      # one group; a decode step is one attn_decode on this one-layer model
            steps = sum(e[0] == "attn_decode" for e in tr.entries)
            assert steps < 19 and (steps + 1) % G.READBACK_EVERY == 0, f"greedy.early_end: {steps} decode steps, so no read-back ended the group"
    return {"traces": traces, "results": results}


def dump(result, path):
    lines, index, traces = [], {}, {}
    for name, entries in result["traces"].items():
        traces[name] = []
        for e in entries:
            line = json.dumps(e)
            if line not in index:
                index[line] = len(lines)
                lines.append(line)
            traces[name].append(index[line])
    with open(path, "w") as f:
        f.write('{"entries": [\n' + ",\n".join("  " + line for line in lines) + '\n ],\n "traces": {\n')
        f.write(",\n".join(f"  {json.dumps(name)}: {json.dumps(idx)}" for name, idx in traces.items()) + '\n },\n "results": {\n')
        f.write(",\n".join(f"  {json.dumps(name)}: {json.dumps(r, sort_keys=True)}" for name, r in result["results"].items()) + "\n }}\n")


def load(path):
    """A file ``dump`` wrote, as ``run_all`` returned it (through JSON: tuples are lists)."""
    with open(path) as f:
        stored = json.load(f)
    return {"traces": {name: [stored["entries"][i] for i in idx] for name, idx in stored["traces"].items()}, "results": stored["results"]}


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "speech-integration_amd")]
    dump(run_all(), sys.argv[1])
