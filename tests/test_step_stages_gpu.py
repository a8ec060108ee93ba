"""Every stage of the training step on the GPU against an fp64 restatement of that stage, from the values the model stored for the stage's
inputs (tests/step_stages.py holds the capture, the table of stored values, the reference and the bounds; tests/test_step_stages_ref.py its
dry run on the CPU).  Each stage is one kernel deep, so a mis-wiring — a wrong residual, a stale buffer, the wrong layer's activations in a
strided batched launch, write instead of add, a skipped row range — shows at full size in exactly one stage, under the bounds the kernel files
derive.  The shapes are the smallest at which each model-level branch is taken, and the branch is asserted from the capture.

Scenarios: plain (bf16, 3 layers in groups of 2, two micro-batches in a window), per-layer weight gradients, ragged rows padded to whole
tiles, packed rows (plan kernels; varlen kernels), frozen slices, the unfused head and a backward through the hidden states alone, fp32, and
``_gemm``'s tail split directly.

Measured on an MI355X, worst error / bound per stage over all scenarios (the module prints it, run with -s; the attention stages att, dq, dk,
dv are worst err / E_row against attn_stress.MARGIN = 8; an element bound counts a whole ulp per rounding to storage, so a correctly rounded
bf16 store sits at 0.5; tokens, embed and doc_ranges are bit for bit):

  stage     bf16    fp32     stage     bf16    fp32     stage       bf16    fp32
  rstd1     0.1355  0.1471   logits    0.4962  0.0186   dhmid       0.5000  0.4041
  xn1       0.3298  0.2293   row_loss  0.2139  0.1870   datt        0.4955  0.0189
  qkv       0.4962  0.0219   dlogits   0.9991  0.2799   dWo         0.4983  0.0280
  att       1.0972  0.0471   loss      0.0054  0.0012   dq          1.9693  0.1025
  lse       0.0442  0.0415   alpha     0.3086  0.3086   dk          3.5524  0.1171
  hmid      0.4984  0.0176   d_hn      0.4960  0.0433   dv          0.9921  0.0801
  rstd2     0.1480  0.1436   dh final  0.5000  0.3374   dxn attn    0.4938  0.0144
  xn2       0.6507  0.2190   dscale    0.4993  0.0849   dWqkv       0.4988  0.0587
  gu        0.4964  0.0248   dW2       0.4986  0.0475   dh          0.5000  0.3741
  act       0.3200  0.3264   dgu       0.4958  0.2246   dE head     0.4998  0.1410
  h_out     0.4970  0.0172   dxn mlp   0.4842  0.0088   dE scatter  0.5000  0.3659
  rstdf     0.1102  0.1393   dW13      0.4988  0.0358
  hn        0.3298  0.2077

The eleven tests take 7.5 s together (1.7 s the slowest: two micro-batches).
"""
import types

import pytest
import torch

import step_stages as SS
from launch_trace import DEV, MFMA_PARAMS, PLAN_PARAMS, _model

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
WORST = {"bf16": {}, "fp32": {}}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for dt, worst in WORST.items():
        for s, v in worst.items():
            print(f"\nstep-stages worst error / bound  {dt}  {s:<14s} {v:.4f}", end="")
    print()


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


@pytest.fixture(scope="module")
def loss_fn():
    from ssi.loss import CEWithChunkedOutputLoss
    return CEWithChunkedOutputLoss()


_MODELS = {}


def model_of(params, seed, dtype, group=2):
    """One model per (shape, dtype), its window closed and its gradient buffer filled with what the first backward must write over."""
    key = (tuple(params.items()), seed, dtype)
    if key not in _MODELS:
        _MODELS[key] = _model(params, seed, dtype)
    m = _MODELS[key]
    m.set_frozen(None)
    m.zero_grad()
    m.wgrad_group = group
    m._flat_grad.fill_(SS.STALE)
    return m


def run(name, model, params, batches, step):
    """``step(batch)`` for every micro-batch under one capture, then every stage of every micro-batch."""
    cap = SS.Capture()
    cap.watch(model)
    with cap.capture():
        for bt in batches:
            step(bt)
    g = SS.Geom.of(model, params)
    W = g.weights(model._flat)
    mbs = SS.split_micro_batches(cap.calls)
    assert len(mbs) == len(batches)
    ck = SS.Checker(name, WORST["bf16" if model.dtype == BF else "fp32"])
    steps = []
    for i, (calls, bt) in enumerate(zip(mbs, batches)):
        st = SS.Step(calls, g, bt.tokens.numel(), "dh.b.all" in SS.writes_of(calls), bt.head)
        ck.mb = i
        SS.check_step(ck, st, W, bt)
        steps.append(st)
    print(ck.table())
    return cap, steps


def fused(model):
    def step(bt):
        model.fused_loss(bt.tokens.to(DEV), bt.labels.to(DEV)).backward()
    return step


def names(calls, name, layout=None):
    return [c for c in calls if c.name == name and (layout is None or c.enc[1][0] == layout)]


def test_plain_two_micro_batches_in_a_window():
    """Deferred batched dW_o / dW_qkv with one full and one partial group, split-K in ``_gemm`` and in ``wgrad``, the head's dE written before
    the scatter-add; the second micro-batch adds to what the first wrote over a stale buffer."""
    m = model_of(MFMA_PARAMS, 21, BF)
    batches = [SS.seeded(MFMA_PARAMS, 2, 128, 21), SS.seeded(MFMA_PARAMS, 2, 128, 31, accumulate=True)]
    cap, steps = run("plain", m, MFMA_PARAMS, batches, fused(m))
    assert m.num_output_chunks == 8
    for st, acc in zip(steps, (False, True)):
        assert sorted(c.enc[1][3][2][0] for c in names(st.calls, "gemm_batched")) == [1, 1, 2, 2]
        assert names(st.calls, "gemm_splitk", SS.NT) and names(st.calls, "gemm_splitk", SS.NN) and len(names(st.calls, "gemm_splitk", SS.TN)) == 6
        assert all(c.enc[2]["accumulate"] is acc for c in names(st.calls, "gemm_batched") + names(st.calls, "gemm_splitk", SS.TN))
        assert [w[4] for w in st.grad_writes() if w[0] == "emb"] == ["gemm", "embed_bwd"]


def test_per_layer_weight_gradients():
    m = model_of(MFMA_PARAMS, 21, BF, group=1)
    cap, steps = run("per-layer", m, MFMA_PARAMS, [SS.seeded(MFMA_PARAMS, 2, 128, 21)], fused(m))
    assert not names(cap.calls, "gemm_batched") and len(names(cap.calls, "gemm_splitk", SS.TN)) == 12


def test_ragged_rows_padded_to_whole_tiles():
    """Rows of 100, 57 and 1 tokens as the data layer pads a batch (to 100 positions); the model pads on to 256, T = 768: three row tiles in
    every GEMM, pad rows and a row without a label in every stage."""
    m = model_of(MFMA_PARAMS, 21, BF)
    tokens, labels = SS.ragged_batch(MFMA_PARAMS)

    def step(bt):
        m.fused_loss(tokens.to(DEV), labels.to(DEV)).backward()
    cap, steps = run("ragged", m, MFMA_PARAMS, [SS.Batch(*SS.right_pad(tokens, labels, 256))], step)
    assert steps[0]["h.0"].shape[0] == 768


@pytest.mark.parametrize("form", ["plan", "varlen"])
def test_packed_rows(ops, form):
    """Documents ``attn_stress.DOC_ROWS``: host positions with a forced plan run the pipelined kernels, device positions without one the varlen
    kernels; RoPE by document-relative positions, block-causal attention."""
    from ssi import _lib
    m = model_of(PLAN_PARAMS, 22, BF)
    bt, input_pos = SS.packed_batch(PLAN_PARAMS)
    plan = m.build_attn_plan(input_pos, force=True) if form == "plan" else None
    assert (plan is not None) == (form == "plan")

    def step(b):
        m.fused_loss(b.tokens.to(DEV), b.labels.to(DEV), input_pos=input_pos if form == "plan" else input_pos.to(DEV), attn_plan=plan).backward()
    cap, steps = run(f"packed {form}", m, PLAN_PARAMS, [bt], step)
    assert bool(ops.attn_last_dispatch() & _lib.ATTN_USED_PLAN) == (form == "plan")
    assert all((c.enc[2]["plan"] is not None) == (form == "plan") and c.enc[1][11] is not None for c in names(cap.calls, "attn_bwd"))
    assert int(m.position_errors) == 0


def test_frozen_slices():
    """One layer's wqkv (a group of its own: its launch is skipped) and all but rows [256, 512) of the embedding are frozen: the frozen wqkv
    slice keeps the bit pattern it had, the head computes the span alone, everything else is checked."""
    m = model_of(MFMA_PARAMS, 21, BF)
    D = MFMA_PARAMS["embed_dim"]
    o, s = m._slices["L2.wqkv"]
    cuts = [0, 256 * D, 512 * D, m.vocab_pad * D, o, o + s[0] * s[1], m._flat_numel]
    flags = [True, False, True, False, True, False]
    m.set_frozen([types.SimpleNamespace(start=a, end=b, frozen=f) for a, b, f in zip(cuts, cuts[1:], flags) if b > a])
    try:
        assert m._emb_span == (256, 512)
        bt = SS.seeded(MFMA_PARAMS, 2, 128, 21, frozen=("L2.wqkv",), emb_rows=(256, 512))
        run("frozen", m, MFMA_PARAMS, [bt], fused(m))
        assert bool((m._flat_grad[o:o + s[0] * s[1]] == SS.STALE).all()), "the frozen slice was written"
    finally:
        m.set_frozen(None)


def test_unfused_head(loss_fn):
    """``loss_fn(model(tokens), labels)``: the logits leave the model through ``_HeadLogitsFn`` and their gradient comes back from the
    stand-alone cross-entropy."""
    m = model_of(MFMA_PARAMS, 21, BF)

    def step(bt):
        loss_fn(m(tokens=bt.tokens.to(DEV)), bt.labels.to(DEV)).backward()
    cap, steps = run("unfused head", m, MFMA_PARAMS, [SS.seeded(MFMA_PARAMS, 2, 128, 21, head="logits")], step)
    assert not SS.writes_of(cap.calls).get("logits")


def test_backward_through_the_hidden_states_alone():
    """No head in front: the embedding gradient is zeroed before the scatter-add."""
    m = model_of(MFMA_PARAMS, 21, BF)
    w = torch.randn(2, 128, MFMA_PARAMS["embed_dim"], generator=torch.Generator().manual_seed(3)).to(DEV)

    def step(bt):
        (m.forward_hidden(bt.tokens.to(DEV)).float() * w).sum().backward()
    run("hidden only", m, MFMA_PARAMS, [SS.seeded(MFMA_PARAMS, 2, 128, 21, head="hidden")], step)


def test_fp32():
    """The plain scenario in fp32: generic kernels, no deferral, no split."""
    m = model_of(MFMA_PARAMS, 21, F32)
    batches = [SS.seeded(MFMA_PARAMS, 2, 128, 21), SS.seeded(MFMA_PARAMS, 2, 128, 31, accumulate=True)]
    cap, steps = run("fp32", m, MFMA_PARAMS, batches, fused(m))
    assert not names(cap.calls, "gemm_batched") and not names(cap.calls, "gemm_splitk") and "dh.b" in SS.writes_of(steps[0].calls)


@pytest.mark.parametrize("layout", [SS.NT, SS.NN], ids=["NT", "NN"])
def test_gemm_tail_split_directly(layout):
    """M = 257 tile rows of one tile each: one whole round of the 256 CUs and a tail of one tile, which ``_gemm`` gives to a second launch.
    Integer operands in {-3 .. 3}: every fp32 sum is exact (|sum| <= 9 x 256), so the result is defined by the rounding points alone,
    bf16(bf16(sum) + R), and is compared bit for bit against float64."""
    m = model_of(MFMA_PARAMS, 21, BF)
    M, N, K = 257 * 256, 256, 256
    gen = torch.Generator().manual_seed(40 + layout)
    a = torch.randint(-3, 4, (M, K), generator=gen).to(BF)
    b = torch.randint(-3, 4, (N, K) if layout == SS.NT else (K, N), generator=gen).to(BF)
    r = torch.randint(-3, 4, (M, N), generator=gen).to(BF)
    c = torch.full((M, N), -7.25, dtype=BF, device=DEV)
    cap = SS.Capture(values=False)
    cap.watch(m)
    with cap.capture():
        m._gemm(layout, a.to(DEV), b.to(DEV), c, residual=r.to(DEV))
    launches = [e for e in cap.entries if e[0] in ("gemm", "gemm_splitk")]
    assert [e[1][3][1] for e in launches] == [[256 * 256, N], [256, N]], launches
    s = a.double() @ (b.double().t() if layout == SS.NT else b.double())
    ref = (s.float().to(BF).double() + r.double()).float().to(BF)
    assert torch.equal(c.cpu().view(torch.int16), ref.view(torch.int16)), f"{int((c.cpu() != ref).sum())} elements differ"
