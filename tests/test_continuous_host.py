"""CPU: continuous batching's host code.  ``PoolSchedule`` / ``simulate_pool`` against a brute-force simulation over random length vectors
(every prompt admitted exactly once, no slot double-booked, the admission rule, the read-back cadence); the occupancy arithmetic; termination
when ``admit_min`` exceeds the remaining queue and when the queue is empty; the pool loop itself on a model stub (results in input order and
equal to the static loop's, the per-row bookkeeping, the ``_rows`` wrappers and their per-row arguments); the refusals of ``generate``,
``sample``, ``beam_search``, ``generate_file`` and ``check_continuous``; and without the new keyword arguments the calls of today's path."""
import json
import os
import random
import re

import pytest
import torch

from conftest import PKG, ROOT


# ---- the schedule ----------------------------------------------------------------------------------------------------------------------
def brute_force(generated, order, pool, admit_min, max_new, cadence):
    """The schedule as README and INTEGRATION.md state it, written out step by step with no shared code: rows as dicts, one event list."""
    queue, rows, steps, events, live, admissions = list(order), [None] * pool, 0, [], 0, 0

    def admit():
        nonlocal admissions
        free = [r for r in range(pool) if rows[r] is None]
        alive = pool - len(free)
        if queue and free and (len(free) >= min(admit_min, len(queue)) or alive == 0):
            admissions += 1
            for r in free:
                if queue:
                    i = queue.pop(0)
                    rows[r] = {"prompt": i, "left": generated[i], "since": steps}
                    events.append((steps, i, r))

    admit()
    while queue or any(rows):
        steps += 1
        for row in rows:
            if row is not None and row["left"] > 0:
                row["left"] -= 1
                live += 1
        owned = [row for row in rows if row is not None]
        certain = owned and all(steps - row["since"] >= max_new for row in owned)      # every owned row has run max_new steps: all have ended
        if steps % cadence == 0 or certain:
            for r in range(pool):
                if rows[r] is not None and rows[r]["left"] == 0:
                    rows[r] = None
            admit()
        assert steps < 10 ** 6
    return steps, live, admissions, events


def test_the_schedule_equals_a_brute_force_simulation_over_random_lengths():
    from ssi.generate import PoolSchedule, plan_groups, simulate_pool
    rng = random.Random(5)
    for trial in range(300):
        n, max_new = rng.randint(1, 60), rng.randint(1, 40)
        generated = [rng.randint(1, max_new) for _ in range(n)]
        pool, admit_min, cadence = rng.randint(1, 12), rng.randint(1, 14), rng.choice((1, 3, 8))
        lens = [rng.randint(1, 30) for _ in range(n)]
        order = [i for g in plan_groups(lens, pool) for i in g]
        sched = simulate_pool(generated, order, pool, admit_min, max_new, cadence)
        steps, live, admissions, events = brute_force(generated, order, pool, admit_min, max_new, cadence)
        assert sched.report() == {"decode_steps": steps, "row_steps_live": live, "row_steps_total": steps * pool, "admissions": admissions}
        admitted = [i for pairs in sched.admissions for i, _ in pairs]
        assert admitted == order and sorted(admitted) == list(range(n))              # every prompt exactly once, in the queue's order
        assert [(i, r) for pairs in sched.admissions for i, r in pairs] == [(i, r) for _, i, r in events]
        assert all(sched.slot_of[i] == r for _, i, r in events) and sched.done() and live == sum(generated)
        for pairs in sched.admissions:                                              # no slot double-booked within an admission
            assert len({r for _, r in pairs}) == len(pairs) and all(0 <= r < pool for _, r in pairs)
        busy = {}                                                                    # ... nor across them: [admitted, released) never overlap on a row
        for at, i, r in events:
            assert busy.get(r, 0) <= at, (trial, r)
            busy[r] = at + generated[i]
    with pytest.raises(ValueError):
        PoolSchedule([0, 1], 0, 1, 4)
    with pytest.raises(ValueError):
        PoolSchedule([0, 0], 2, 1, 4)


def test_the_admission_rule_and_termination():
    from ssi.generate import PoolSchedule, simulate_pool
    s = PoolSchedule(range(7), pool=4, admit_min=3, max_new=100, cadence=8)
    assert s.admit() == [(0, 0), (1, 1), (2, 2), (3, 3)] and s.admit() == [] and s.queued == 3
    s.release(2, 5)
    assert s.admit() == []                                 # one free row, three are asked for
    s.release(0, 5)
    assert s.admit() == []
    s.release(3, 5)
    assert s.admit() == [(4, 0), (5, 2), (6, 3)] and s.queued == 0          # the lowest free rows, in the queue's order
    s.release(0, 1)
    assert s.admit() == [] and not s.done()                # the queue is empty: nothing to admit, rows still owned
    for r in (1, 2, 3):
        s.release(r, 1)
    assert s.done() and s.row_steps_live == 19
    with pytest.raises(ValueError):
        s.release(1, 1)
    # admit_min above what is left of the queue: min(admit_min, queued) rows are enough
    s = PoolSchedule(range(5), pool=4, admit_min=3, max_new=100)
    s.admit()
    s.release(1, 2)
    assert s.admit() == [(4, 1)]
    # admit_min above the pool: an admission waits for the empty pool, and the run still ends
    sched = simulate_pool([3, 9, 2, 8, 1], range(5), pool=2, admit_min=50, max_new=9, cadence=8)
    assert sched.done() and [len(p) for p in sched.admissions] == [2, 2, 1] and sched.report()["row_steps_live"] == 23
    # the read-backs: every cadence steps, and at the step by which every owned row must have ended
    s = PoolSchedule(range(2), pool=2, admit_min=1, max_new=5, cadence=8)
    s.admit()
    seen = []
    for _ in range(5):
        s.stepped()
        seen.append(s.reads_back())
    assert seen == [False, False, False, False, True]


def test_the_occupancy_arithmetic_and_the_static_steps():
    from ssi.generate import plan_groups, simulate_pool, static_steps
    # every row runs to max_new: both schedules take the same steps
    n, pool, max_new = 24, 8, 20
    full = simulate_pool([max_new] * n, range(n), pool, 4, max_new)
    assert full.report() == {"decode_steps": 60, "row_steps_live": 480, "row_steps_total": 480, "admissions": 3}
    assert static_steps([max_new] * n, plan_groups([1] * n, pool), max_new) == 60
    # one long row per static group holds its group; the pool keeps refilling beside it
    generated = [max_new if i % pool == 0 else 2 for i in range(n)]
    groups = plan_groups([1] * n, pool)
    assert static_steps(generated, groups, max_new) == 60
    assert static_steps([3] * n, groups, max_new) == 3 * 8                         # a group ends at the first read-back that finds it finished
    sched = simulate_pool(generated, range(n), pool, 1, max_new)
    rep = sched.report()
    assert rep["row_steps_live"] == sum(generated) == 102 and rep["row_steps_total"] == pool * rep["decode_steps"]
    assert rep["decode_steps"] < 60 and rep["row_steps_live"] / rep["row_steps_total"] > 102 / 480
    # geometric lengths, the README's arithmetic in small: fewer steps and a higher live share than the static groups
    rng = random.Random(1)
    gen = [min(1 + int(rng.expovariate(1 / 30.0)), 64) for _ in range(256)]
    static = static_steps(gen, plan_groups([1] * 256, 32), 64)
    pooled = simulate_pool(gen, range(256), 32, 4, 64).report()
    assert pooled["decode_steps"] < static and pooled["row_steps_live"] == sum(gen)
    assert pooled["row_steps_live"] / pooled["row_steps_total"] > sum(gen) / (static * 32)


# ---- the loop on a model stub ---------------------------------------------------------------------------------------------------------------
class _Cache:
    errors = 0


class _Model:
    """Just enough of the decoder for the loops on the CPU: logits that prefer token (last + 1) % V, then (last + 2) % V; it records its calls."""
    vocab_size, training = 16, False
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def check_generation_lengths(self, lens, max_new, n_slots, cap):
        if any(n < 1 for n in lens):
            raise ValueError("prompt is empty")

    def eval(self):
        pass

    def new_kv_cache(self, n_slots, cap):
        self.calls.append(("new_kv_cache", n_slots, cap))
        return _Cache()

    def _logits(self, last):
        x = torch.zeros(last.numel(), 16)
        x[torch.arange(last.numel()), (last + 1) % 16] = 2.0
        x[torch.arange(last.numel()), (last + 2) % 16] = 1.0
        return x

    def prefill(self, cache, seqs, max_new_tokens=None, **kw):
        self.calls.append(("prefill", [int(s[-1]) for s in seqs], kw))
        return self._logits(torch.tensor([int(s[-1]) for s in seqs]))

    def decode_step(self, cache, tok, slot, **kw):
        self.calls.append(("decode_step", slot.tolist(), kw))
        return self._logits(tok)

    def decode_step_beam(self, pcache, bcache, tok, slot, plen, anc, t):
        return self._logits(tok)


def _stub_ops(monkeypatch, calls):
    """Selection wrappers that record their call and answer on the CPU with the first maximum (the penalised ones: the second)."""
    from ssi import generate as G

    def answer(name, second):
        def fn(logits, vocab, token, logprob=None, third=None, **kw):
            calls.append((name, {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}))
            token.copy_(logits[:, :vocab].argsort(dim=1, descending=True, stable=True)[:, 1 if second else 0])
            if logprob is not None:
                logprob.fill_(-1.0)
            if third is not None:
                third.fill_(0 if "select" in name else 3)
        return fn

    for name in ("decode_select", "decode_select_pen", "decode_sample", "decode_sample_pen", "decode_sample_rows", "decode_sample_pen_rows"):
        monkeypatch.setattr(G.ops, name, answer(name, "_pen" in name))


PROMPTS = [[3], [1, 9], [14], [2, 2, 6], [12], [0, 5, 1, 11], [13], [4, 8]]       # a prompt ending in k stops after 15 - k tokens (stop token 15)
KW = dict(max_new_tokens=7, stop_token_ids=[15], pad_id=0)


def _fields(g):
    return g.token_ids, g.finish_reason, g.stop_reason, g.cumulative_logprob, g.prompt_len, g.n_constrained, g.n_kept_mean


def test_the_pool_loop_on_a_stub_gives_the_static_results_in_input_order(monkeypatch):
    from ssi import generate as G
    calls = []
    _stub_ops(monkeypatch, calls)
    static = G.generate(_Model(), PROMPTS, **KW)
    assert [len(g.token_ids) for g in static] == [7, 6, 1, 7, 3, 4, 2, 7] and static[2].finish_reason == "stop" and static[0].finish_reason == "length"
    for pool, admit_min in ((1, 1), (2, 1), (3, 2), (3, None), (8, 1), (50, 4)):
        model, stats = _Model(), {}
        got = G.generate(model, PROMPTS, batch_size=pool, continuous=True, admit_min=admit_min, continuous_report=stats, **KW)
        assert [_fields(g) for g in got] == [_fields(g) for g in static], (pool, admit_min)
        p = min(pool, len(PROMPTS))
        order = [i for g in G.plan_groups([len(q) for q in PROMPTS], p) for i in g]
        sim = G.simulate_pool([len(g.token_ids) for g in static], order, p, G.ADMIT_MIN_DEFAULT if admit_min is None else admit_min, 7)
        assert stats == dict(sim.report(), continuous=True)
        assert [c for c in model.calls if c[0] == "new_kv_cache"] == [("new_kv_cache", p, 4 + 7)]      # ONE cache: pool slots, max(lens) + max_new
        fills = [c for c in model.calls if c[0] == "prefill"]
        assert [c[2]["slots"] for c in fills] == [[r for _, r in pairs] for pairs in sim.admissions]
        assert [c[1] for c in fills] == [[PROMPTS[i][-1] for i, _ in pairs] for pairs in sim.admissions]
        assert all("separate" not in c[2] for c in fills)
        for c in model.calls:                                                       # a free or finished row is inert, a live row decodes on ITS slot
            if c[0] == "decode_step":
                assert all(s in (-1, r) for r, s in enumerate(c[1]))
    assert not calls                                                                # argmax: no selection wrapper
    # under a penalty: the chooser of the static loop, one prompt table for the call, the row's line set on admission
    kw = dict(KW, repetition_penalty=1.3, logprobs=True)
    static = G.generate(_Model(), PROMPTS, **kw)
    del calls[:]
    got = G.generate(_Model(), PROMPTS, batch_size=3, continuous=True, admit_min=1, **kw)
    assert [_fields(g) for g in got] == [_fields(g) for g in static]
    assert {name for name, _ in calls} == {"decode_select_pen"}
    first = calls[0][1]
    assert first["prompt_ids"].shape == (8, 4) and first["prompt_row"].tolist() == [0, 2, 4] and first["n_generated"].tolist() == [0, 0, 0]
    lines = {tuple(kw_["prompt_row"].tolist()) for _, kw_ in calls}
    assert len(lines) > 2 and all(0 <= v < 8 for line in lines for v in line)


def test_the_sampled_pool_runs_on_the_rows_entries_with_per_row_arguments(monkeypatch):
    from ssi import generate as G
    calls = []
    _stub_ops(monkeypatch, calls)
    draw = dict(temperature=0.8, top_k=5, seed=3)
    static = G.sample(_Model(), PROMPTS, **draw, **KW)
    assert {name for name, _ in calls} == {"decode_sample"} and all(isinstance(kw["step"], int) for _, kw in calls)      # today's launches
    del calls[:]
    stats = {}
    got = G.sample(_Model(), PROMPTS, batch_size=3, continuous=True, admit_min=1, continuous_report=stats, **draw, **KW)
    assert [[_fields(g) for g in gs] for gs in got] == [[_fields(g) for g in gs] for gs in static] and stats["admissions"] >= 3
    assert {name for name, _ in calls} == {"decode_sample_rows"}
    for _, kw in calls:
        assert kw["step"].dtype == torch.int32 and kw["temperature"] == 0.8 and kw["top_k"] == 5 and kw["top_p"] == 1.0 and kw["seed"] == 3
    assert calls[0][1]["sequence"].tolist() == [0, 2, 4] and calls[0][1]["step"].tolist() == [0, 0, 0]          # the input index; step 0
    ages = {tuple(kw["step"].tolist()) for _, kw in calls}
    assert any(len(set(a)) > 1 for a in ages)                                          # rows of different ages in one launch
    # per-prompt lists: the _rows entries in either mode, every row with its prompt's values
    temps = [0.5 + 0.1 * i for i in range(8)]
    ks = [-1, 1, 2, 3, 4, 5, 6, 2 ** 70]
    for mode in (dict(), dict(batch_size=3, continuous=True, admit_min=1), dict(n=2, batch_size=6)):
        del calls[:]
        G.sample(_Model(), PROMPTS, temperature=temps, top_k=ks, top_p=0.9, seed=3, **mode, **KW)
        assert {name for name, _ in calls} == {"decode_sample_rows"}
        n = mode.get("n", 1)
        for _, kw in calls:
            seq = kw["sequence"].tolist()
            assert kw["temperature"].dtype == torch.float64 and kw["top_k"].dtype == torch.int64 and kw["top_p"] == 0.9
            if "continuous" not in mode:                                              # (a free row of a pool keeps neutral values)
                assert kw["temperature"].tolist() == [temps[s // n] for s in seq] and kw["top_k"].tolist() == [min(ks[s // n], 2 ** 62) for s in seq]
        if "continuous" in mode:
            assert calls[0][1]["temperature"].tolist() == [temps[0], temps[2], temps[4]] and calls[0][1]["top_k"].tolist() == [-1, 2, 4]
    del calls[:]
    G.sample(_Model(), PROMPTS, temperature=temps, seed=3, presence_penalty=0.5, batch_size=3, continuous=True, **KW)
    assert {name for name, _ in calls} == {"decode_sample_pen_rows"} and calls[0][1]["prompt_row"].tolist() == [0, 2, 4]


# ---- refusals, and today's path ------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    from ssi import generate as G
    model = _Model()
    with pytest.raises(ValueError, match="beam search"):
        G.beam_search(model, PROMPTS, beam_width=2, continuous=True, **KW)
    with pytest.raises(ValueError, match="n = 1"):
        G.sample(model, PROMPTS, n=2, temperature=1.0, seed=0, continuous=True, **KW)
    for bad in (dict(continuous=1), dict(continuous=True, admit_min=0), dict(continuous=True, admit_min=1.5), dict(continuous=True, admit_min=True),
                dict(admit_min=4), dict(continuous=True, batch_size=0)):
        with pytest.raises(ValueError):
            G.generate(model, PROMPTS, **bad, **KW)
        with pytest.raises(ValueError):
            G.sample(model, PROMPTS, temperature=1.0, seed=0, **bad, **KW)
    for bad in (dict(temperature=[1.0] * 7), dict(temperature=[1.0] * 7 + [0.0]), dict(temperature=1.0, top_p=[1.0] * 7 + [1.5]),
                dict(temperature=1.0, top_k=[1] * 7 + [1.5]), dict(temperature=[1.0] * 7 + [float("nan")])):
        with pytest.raises(ValueError):
            G.sample(model, PROMPTS, seed=0, **bad, **KW)
    with pytest.raises(ValueError, match="empty"):
        G.generate(model, [[1], []], continuous=True, **KW)
    assert model.calls == []
    assert G.generate(model, [], continuous=True, **KW) == [] and model.calls == []


def test_check_continuous_and_the_configuration():
    from ssi.generate import check_continuous
    assert check_continuous(None, None) == {} and check_continuous(False, None, beam_width=4, n=3) == {}
    assert check_continuous(True, None) == {"continuous": True} and check_continuous(True, 8) == {"continuous": True, "admit_min": 8}
    with pytest.raises(ValueError, match="gen.continuous=true together with gen.beam_width > 1"):
        check_continuous(True, None, beam_width=2)
    with pytest.raises(ValueError, match="gen.continuous=true together with sampling_params.n > 1"):
        check_continuous(True, None, n=2)
    for bad in ((1, None), ("yes", None), (True, 0), (True, 2.5), (True, False), (False, 4), (None, 4)):
        with pytest.raises(ValueError):
            check_continuous(*bad)
    text = open(os.path.join(PKG, "conf", "generate.yaml")).read()
    assert re.search(r"^  continuous: false\b", text, flags=re.M) and re.search(r"^  admit_min: null\b", text, flags=re.M)
    script = open(os.path.join(PKG, "scripts", "generate.py")).read()
    assert 'check_continuous(cfg.gen.get("continuous"), cfg.gen.get("admit_min")' in script and "constraints.update(pool)" in script
    header = open(os.path.join(ROOT, "include", "ssi_hip.h")).read()
    from ssi import _lib
    assert int(re.search(r"#define SSI_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 28
    assert re.search(r"28: \+ ssi_decode_sample_rows, ssi_decode_sample_pen_rows", header)
    assert len(_lib.PROTOTYPES["ssi_decode_sample_rows"][1]) == len(_lib.PROTOTYPES["ssi_decode_sample"][1]) + 3
    assert len(_lib.PROTOTYPES["ssi_decode_sample_pen_rows"][1]) == len(_lib.PROTOTYPES["ssi_decode_sample_pen"][1]) + 3


class _Tokenizer:
    pad_id, eom_id, eot_id, eos_id = 0, 15, 15, 15
    special_tokens = {}

    def decode(self, ids, **kw):
        return " ".join(str(t) for t in ids)


def test_generate_file_adds_the_summary_keys_under_the_flag_alone(tmp_path, monkeypatch):
    from ssi import generate as G
    _stub_ops(monkeypatch, [])
    out = str(tmp_path / "g.jsonl")
    kw = dict(max_new_tokens=7, stop_token_ids=[15], prompts=PROMPTS)
    plain = G.generate_file(_Model(), _Tokenizer(), None, out, **kw)
    lines = open(out).read()
    assert plain == {"items": 8, "generated_tokens": 37, "stopped": 6}
    assert G.generate_file(_Model(), _Tokenizer(), None, out, continuous=False, admit_min=None, **kw) == plain
    got = G.generate_file(_Model(), _Tokenizer(), None, out, batch_size=3, continuous=True, admit_min=2, **kw)
    assert open(out).read() == lines                                                    # the same generations file
    assert {k: got[k] for k in plain} == plain and got["continuous"] is True and got["row_steps_live"] == 37
    assert set(got) - set(plain) == {"continuous", "decode_steps", "row_steps_live", "row_steps_total", "admissions"}
    assert got["row_steps_total"] == 3 * got["decode_steps"] and got["admissions"] >= 3
    sampled = G.generate_file(_Model(), _Tokenizer(), None, out, sample=True, temperature=0.7, seed=1, batch_size=3, continuous=True, **kw)
    assert sampled["sampled"] is True and sampled["continuous"] is True and [len(json.loads(l)["outputs"]) for l in open(out)] == [1] * 8
    with pytest.raises(ValueError, match="beam search"):
        G.generate_file(_Model(), _Tokenizer(), None, out, beam_width=2, continuous=True, **kw)
    with pytest.raises(ValueError, match="n = 1"):
        G.generate_file(_Model(), _Tokenizer(), None, out, sample=True, n=2, temperature=0.7, seed=1, continuous=True, **kw)
    with pytest.raises(ValueError, match="admit_min"):
        G.generate_file(_Model(), _Tokenizer(), None, out, admit_min=2, **kw)


def test_without_the_new_arguments_the_calls_are_todays(monkeypatch):
    """The static loops never reach the pool loop, the ``_rows`` wrappers or ``prefill(slots=...)``, and call the model as they did."""
    from ssi import generate as G
    calls = []
    _stub_ops(monkeypatch, calls)
    monkeypatch.setattr(G, "_run_pool", lambda *a, **k: pytest.fail("the pool loop ran without continuous=True"))
    monkeypatch.setattr(G, "PoolSchedule", lambda *a, **k: pytest.fail("a schedule was built without continuous=True"))
    model = _Model()
    G.generate(model, PROMPTS, batch_size=3, **KW)
    G.generate(model, PROMPTS, batch_size=3, presence_penalty=0.5, **KW)
    G.sample(model, PROMPTS, temperature=0.8, top_k=4, top_p=0.9, seed=1, batch_size=3, **KW)
    G.sample(model, PROMPTS, n=2, temperature=0.8, seed=1, batch_size=4, frequency_penalty=0.2, **KW)
    assert {name for name, _ in calls} == {"decode_select_pen", "decode_sample", "decode_sample_pen"}
    for name, kw in calls:
        if name.startswith("decode_sample"):
            assert isinstance(kw["step"], int) and isinstance(kw["temperature"], float) and isinstance(kw["top_k"], int)
    fills = [c for c in model.calls if c[0] == "prefill"]
    assert fills and all(c[2] == {} for c in fills)                                     # no slots, no separate: prefill as it was called
    assert all(c[2] == {} for c in model.calls if c[0] == "decode_step")
    caches = [c for c in model.calls if c[0] == "new_kv_cache"]
    assert caches[0] == ("new_kv_cache", 3, 4 + 7)
