"""Which kernels the model launches, on which buffers: a trace of every call into ``ssi.ops`` over a fixed set of scenarios.

``Tracer`` wraps every public function of ``ssi.ops`` while a scenario runs and appends one entry per call: ``[name, [args...], {kwargs}]``.
A tensor argument becomes ``[where, element offset, shape, stride, dtype]``; ``where`` is found from ``data_ptr()``: the arena buffer's name for
that model (a second model's with its prefix), ``param`` (``_flat``), ``grad`` (``_flat_grad``), ``rope``, ``cache.k`` / ``cache.v`` /
``cache.lengths`` / ``cache.errors``; any other tensor is ``["ext", shape, dtype]``.  ``None`` stays null, numbers and bools are literal, floats go as
``float.hex()``.  Only ``ssi.ops`` and the model's public API are touched, so the same file records the trace on any commit.

``run_all()`` runs the scenarios and returns ``{"traces": {scenario: entries}, "arena": {model: {buffer: [numel, dtype]}}}``.
``python tests/launch_trace.py OUT.json`` writes that as JSON, one entry per line; tests/golden/decoder_launch_trace.json is such a file, recorded
at the commit before the decoder stack's forward got one layer body, and tests/test_decoder_launch_trace_gpu.py holds the code to it."""
import contextlib
import inspect
import json
import os
import sys

import torch

DEV = "cuda:0"
MFMA_PARAMS = dict(vocab_size=700, num_layers=3, num_heads=4, num_kv_heads=2, embed_dim=256, max_seq_len=512, intermediate_dim=512)
PLAN_PARAMS = dict(vocab_size=700, num_layers=2, num_heads=8, num_kv_heads=2, embed_dim=512, max_seq_len=512, intermediate_dim=512)


class Tracer:
    def __init__(self):
        self.models = []        # (prefix, model)
        self.caches = []
        self.entries = None

    def watch(self, model, prefix=""):
        self.models.append((prefix, model))
        return model

    def _regions(self):
        for prefix, m in self.models:
            yield prefix + "param", m._flat
            yield prefix + "grad", m._flat_grad
            yield prefix + "rope", m._rope
            for name, t in m._arena.buf.items():
                if t is not None:
                    yield prefix + name, t
        for c in self.caches:
            for name in ("k", "v", "lengths", "errors"):
                yield "cache." + name, getattr(c, name)

    def locate(self, v):
        """(region name, element offset) of a tensor that starts inside one of the watched buffers, else None."""
        if v.numel():
            p = v.data_ptr()
            for where, base in self._regions():
                lo = base.data_ptr()
                if base.device == v.device and lo <= p < lo + base.numel() * base.element_size():
                    return where, (p - lo) // v.element_size()
        return None

    def _enc(self, v):
        if v is None or isinstance(v, (bool, int, str)):
            return v
        if isinstance(v, float):
            return v.hex()
        if isinstance(v, torch.Tensor):
            shape, dtype = list(v.shape), str(v.dtype)
            at = self.locate(v)
            if at is not None:
                return [at[0], at[1], shape, list(v.stride()), dtype]
            return ["ext", shape, dtype]
        if isinstance(v, (list, tuple)):
            return [self._enc(x) for x in v]
        if isinstance(v, (torch.dtype, torch.device)):
            return str(v)
        return {"object": type(v).__name__}

    def traced(self, name, fn, args, kw):
        """One call into ``ssi.ops``: its entry, then the call (``call``: where tests/step_stages.py keeps the tensors' values as well)."""
        self.entries.append([name, [self._enc(a) for a in args], {k: self._enc(x) for k, x in kw.items()}])
        return self.call(name, fn, args, kw)

    def call(self, name, fn, args, kw):
        return fn(*args, **kw)

    @contextlib.contextmanager
    def scenario(self, caches=()):
        """Wrap ``ssi.ops`` for the body; ``self.entries`` is the trace afterwards."""
        from ssi import ops
        self.caches, self.entries = list(caches), []
        names = [n for n, f in vars(ops).items() if inspect.isfunction(f) and f.__module__ == ops.__name__ and not n.startswith("_")]
        saved = {n: getattr(ops, n) for n in names}

        def wrap(name, fn):
            def traced(*args, **kw):
                return self.traced(name, fn, args, kw)
            return traced

        try:
            for n, f in saved.items():
                setattr(ops, n, wrap(n, f))
            yield self
            torch.cuda.synchronize()
        finally:
            for n, f in saved.items():
                setattr(ops, n, f)
            self.caches = []


def _model(params, seed, dtype):
    from oracle import hf_crosscheck as hx
    from ssi.model import HipLlamaDecoder
    m = HipLlamaDecoder(**params, dtype=dtype, device=DEV)
    m.load_state_dict(hx.seeded_state_dict(params, seed))
    m.set_num_output_chunks(8)
    m.train()
    return m


def _batch(params, b, s, seed):
    from oracle import hf_crosscheck as hx
    return {k: v.to(DEV) for k, v in hx.seeded_batch(params["vocab_size"], b, s, seed).items()}


def _generation(tr, model, vocab):
    g = torch.Generator().manual_seed(17)
    prompts = [torch.randint(0, vocab, (n,), generator=g) for n in (5, 17, 1)]
    cache = model.new_kv_cache(4, 40)
    tok = torch.tensor([3, 4, 5], dtype=torch.int64, device=DEV)
    with tr.scenario(caches=[cache]):
        model.prefill(cache, prompts, max_new_tokens=2)
        model.decode_step(cache, tok, torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV))
        model.decode_step(cache, tok, torch.tensor([0, -1, 2], dtype=torch.int32, device=DEV))
        assert int(cache.errors) == 0 and cache.lengths.tolist() == [7, 18, 3, 0]
    return tr.entries


def run_all():
    from oracle import hf_crosscheck as hx
    from ssi.loss import CEWithChunkedOutputLoss, compute_loss
    loss_fn = CEWithChunkedOutputLoss()
    tr, traces = Tracer(), {}
    tiny_params, _, _, tiny_seed = hx.CASES["tiny"]
    tiny = tr.watch(_model(tiny_params, tiny_seed, torch.float32))

    # 1. fp32, generic kernels: the first backward of a window writes, the second accumulates
    batch = _batch(tiny_params, 2, 16, tiny_seed)
    with tr.scenario():
        compute_loss(batch, tiny, loss_fn).backward()
        compute_loss(batch, tiny, loss_fn).backward()
        tiny.zero_grad()
    traces["fp32"] = tr.entries

    # 2. bf16 MFMA shapes, unpacked: 3 layers in groups of 2 (a full and a partial group of deferred weight gradients, split-K), then ungrouped
    mfma = tr.watch(_model(MFMA_PARAMS, 21, torch.bfloat16))
    batch = _batch(MFMA_PARAMS, 2, 128, 21)
    for group in (2, 1):
        mfma.wgrad_group = group
        with tr.scenario():
            compute_loss(batch, mfma, loss_fn).backward()
            mfma.zero_grad()
        traces[f"mfma.wgrad_group{group}"] = tr.entries
    mfma.wgrad_group = 2

    # 3. bf16 MFMA shapes, packed rows with a work plan: three documents per row, one boundary off the 64-row grid
    packed = tr.watch(_model(PLAN_PARAMS, 22, torch.bfloat16), "plan:")
    pbatch = _batch(PLAN_PARAMS, 2, 256, 22)
    pos = torch.stack([torch.cat([torch.arange(n) for n in lens]) for lens in ((64, 100, 92), (128, 64, 64))])
    pbatch["input_pos"] = pos
    pbatch["attn_plan"] = packed.build_attn_plan(pos, force=True)
    assert pbatch["attn_plan"] is not None
    with tr.scenario():
        compute_loss(pbatch, packed, loss_fn).backward()
        packed.zero_grad()
    traces["mfma.plan"] = tr.entries
    tr.models.pop()
    packed_arena = {k: [v.numel(), str(v.dtype)] for k, v in packed._arena.buf.items()}
    del packed, pbatch

    # 4. an eval forward (fused loss and logits) between a training forward and its backward
    with tr.scenario():
        loss = compute_loss(batch, mfma, loss_fn)
        mfma.eval()
        with torch.inference_mode():
            compute_loss(batch, mfma, loss_fn)
            mfma(tokens=batch["tokens"])
        mfma.train()
        loss.backward()
        mfma.zero_grad()
    traces["mfma.eval_between"] = tr.entries

    # 5. KL against a frozen teacher: under grad, and forward-only
    teacher = tr.watch(_model(MFMA_PARAMS, 23, torch.bfloat16), "teacher:")
    teacher.eval()
    with tr.scenario():
        compute_loss(batch, mfma, loss_fn, teacher=teacher, teacher_kl_coeff=0.5).backward()
        with torch.no_grad():
            compute_loss(batch, mfma, loss_fn, teacher=teacher, teacher_kl_coeff=0.5)
        mfma.zero_grad()
    traces["mfma.teacher_kl"] = tr.entries
    tr.models.pop()
    teacher_arena = {k: [v.numel(), str(v.dtype)] for k, v in teacher._arena.buf.items()}
    del teacher

    # 6. generation: prefill of ragged prompts, two decode steps (the second with an inert row); rows padded to 256 on the MFMA shapes only
    traces["mfma.generate"] = _generation(tr, mfma, MFMA_PARAMS["vocab_size"])
    traces["fp32.generate"] = _generation(tr, tiny, tiny_params["vocab_size"])

    # 7. five layers, forward-only: from the fourth layer on the eval forward and the decode step go round their two hidden-state buffers again
    deep_params = dict(tiny_params, num_layers=5)
    deep = tr.watch(_model(deep_params, 24, torch.float32), "deep:")
    with tr.scenario():
        with torch.no_grad():
            deep(tokens=_batch(deep_params, 2, 16, 24)["tokens"])
    traces["fp32.deep.eval"] = tr.entries
    traces["fp32.deep.generate"] = _generation(tr, deep, deep_params["vocab_size"])

    arena = {name: {k: [v.numel(), str(v.dtype)] for k, v in m._arena.buf.items()} for name, m in (("fp32", tiny), ("mfma", mfma), ("deep", deep))}
    arena["plan"], arena["teacher"] = packed_arena, teacher_arena
    return {"traces": traces, "arena": arena}


def dump(result, path):
    with open(path, "w") as f:
        f.write('{"arena": ' + json.dumps(result["arena"], sort_keys=True) + ',\n "traces": {\n')
        blocks = []
        for name, entries in result["traces"].items():
            blocks.append(f'  {json.dumps(name)}: [\n' + ",\n".join("   " + json.dumps(e) for e in entries) + "\n  ]")
        f.write(",\n".join(blocks) + "\n }}\n")


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "speech-integration_amd")]
    dump(run_all(), sys.argv[1])
