"""The decoder stack launches what it launched before its forward got one layer body and one table of activation buffers: every call into
``ssi.ops`` of the scenarios in tests/launch_trace.py (training on the generic and the MFMA path, deferred and per-layer weight gradients,
packed rows with a work plan, an eval forward between a training forward and its backward, a KL teacher, prefill and decode steps, and a
five-layer stack forward-only, where the eval and decode buffers come round again) against
tests/golden/decoder_launch_trace.json, entry for entry — function, argument order, buffer name, element offset, shape, stride, dtype — and the
arena's buffers by name, size and dtype.  The golden file was recorded with the same helper at the commit before that change; it is not to be
regenerated from later code.  The order in which buffers are first asked for is free (the table is compared as a dict)."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

SCENARIOS = ("fp32", "mfma.wgrad_group2", "mfma.wgrad_group1", "mfma.plan", "mfma.eval_between", "mfma.teacher_kl", "mfma.generate", "fp32.generate",
             "fp32.deep.eval", "fp32.deep.generate")


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "decoder_launch_trace.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def traced():
    import launch_trace
    return json.loads(json.dumps(launch_trace.run_all()))       # (through JSON, as the golden file went: tuples become lists)


def test_the_scenarios_are_the_recorded_ones(golden, traced):
    assert tuple(golden["traces"]) == tuple(traced["traces"]) == SCENARIOS


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_every_launch_equals_the_recorded_one(scenario, golden, traced):
    want, got = golden["traces"][scenario], traced["traces"][scenario]
    for k, (w, g) in enumerate(zip(want, got)):
        assert g == w, f"{scenario}: call {k} differs"
    assert len(got) == len(want)


def test_the_arena_holds_the_recorded_buffers(golden, traced):
    assert set(traced["arena"]) == set(golden["arena"])
    for model, table in golden["arena"].items():
        assert traced["arena"][model] == table, model
