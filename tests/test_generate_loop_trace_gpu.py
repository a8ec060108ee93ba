"""The generation loops launch what they launched and return what they returned before ``generate`` and ``sample`` got one token loop and
the three entry points one group runner: every call into ``ssi.ops`` of the scenarios in tests/generate_trace.py (greedy with and without
log-probabilities, constraints and penalties, a group that ends at a read-back, sampling with one and three samples per prompt, beam search,
and the small-batch path of each) against tests/golden/generate_loop_trace.json, entry for entry — function, argument order, keywords, buffer
name, element offset, shape, stride, dtype — and every field of every ``Generation`` exactly, floats by their bits.  The golden file was
recorded with the same helper at the commit before that change, twice, to identical files; it is not to be regenerated from later code."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

SCENARIOS = ("greedy", "greedy.logprobs", "greedy.constrained", "greedy.min_new_only", "greedy.penalised", "greedy.penalised.constrained",
             "greedy.early_end", "sample.n1", "sample.n3", "sample.n3.penalised", "beam", "small_batch.greedy", "small_batch.sample.n3",
             "small_batch.beam")


@pytest.fixture(scope="module")
def golden(golden_dir):
    import generate_trace
    return generate_trace.load(os.path.join(golden_dir, "generate_loop_trace.json"))


@pytest.fixture(scope="module")
def traced():
    import generate_trace
    return json.loads(json.dumps(generate_trace.run_all()))       # (through JSON, as the golden file went: tuples become lists)


def test_the_scenarios_are_the_recorded_ones(golden, traced):
    assert tuple(golden["traces"]) == tuple(traced["traces"]) == SCENARIOS
    assert tuple(golden["results"]) == tuple(traced["results"]) == SCENARIOS


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_every_launch_equals_the_recorded_one(scenario, golden, traced):
    want, got = golden["traces"][scenario], traced["traces"][scenario]
    for k, (w, g) in enumerate(zip(want, got)):
        assert g == w, f"{scenario}: call {k} differs"
    assert len(got) == len(want)


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_every_generation_equals_the_recorded_one(scenario, golden, traced):
    want, got = golden["results"][scenario], traced["results"][scenario]
    assert set(got) == set(want)
    assert got.get("small_batch_report") == want.get("small_batch_report")
    for k, (w, g) in enumerate(zip(want["generations"], got["generations"])):
        assert g == w, f"{scenario}: prompt {k} differs"
    assert len(got["generations"]) == len(want["generations"])
