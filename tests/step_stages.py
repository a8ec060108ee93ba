"""Every stage of a training step against an fp64 restatement of that stage, computed from the values the model itself stored for the stage's
mathematical inputs (tests/test_step_stages_ref.py on the CPU, tests/test_step_stages_gpu.py on the GPU).  Nothing here calls a kernel.

Three parts:

``Capture``  a ``launch_trace.Tracer`` that also keeps CPU copies of every tensor argument before and after each call into ``ssi.ops``, with the
             buffer name and offset the tracer finds.
``value_table``  THE table that names the captured values by the math (``h.2``, ``dqkv.1``, ...): a value is "the k-th write to buffer X", because
             the backward reuses its buffers across layers.  Gradients are found by their offset in the flat gradient buffer.
``check_step``  the Llama equations of ``oracle/llama_oracle.py`` stage by stage in float64.  Which stored value feeds which stage is decided
             here, never from the arguments the model passed: the residual of ``hmid.l`` is the stored ``h.l`` whatever the GEMM was given.

Every stage is one kernel deep, so its bound is assembled from the pieces the kernel files derive, and nothing is tuned:

  ulp(ref)              once per rounding to storage between the fp32 math and the stored value (test_row_kernels_gpu.ulp)
  K U32 (|A| @ |B|)     an fp32 sum of K terms in any order (Higham 4.2): split-K, batched and tail launches alike; U32 = 2^-24
  GEMM epilogues        as test_gemm_mfma_parity_gpu.run_forms: p = alpha sum ROUNDED, then p + C_prev + R (one U32 each) ROUNDED
  RoPE after the GEMM   as test_gemm_mfma_parity_gpu._rope64: the projection arrives rounded, two products and a sum (2 U32), ROUNDED
  RMSNorm, SwiGLU       test_row_kernels_gpu.rms_fwd_ref / rms_bwd_ref / swiglu_fwd_ref / swiglu_bwd_ref on the stored inputs; the fused SwiGLU
                        backward rounds d act = dh W2 to storage first: that error is carried through d dgu / d dact (the stage is linear in it)
  cross-entropy         ce_parity.expected on the stored logits
  attention             attn_stress.exact_of / restate_of / rope_refs on the stored qkv and d att, judged by attn_stress.row_check with its own
                        MARGIN and EPS, unchanged
  embedding scatter     (count + 1) U32 (|old| + sum |terms|) + ulp, as test_row_kernels_gpu._embed_case
  bit for bit           the gather, untouched rows of the embedding gradient, pad columns and ignored rows of the logits gradient, frozen
                        slices, and every tensor a call only reads (before against after)

``delta`` of the attention backward is a workspace without a contract (include/ssi_hip.h) and is not a stage.
"""
import contextlib
from typing import NamedTuple, Optional

import torch

import attn_stress as A
import ce_parity as C
from launch_trace import Tracer
from test_row_kernels_gpu import EPS as NORM_EPS
from test_row_kernels_gpu import U32, rms_bwd_ref, rms_fwd_ref, swiglu_bwd_ref, swiglu_fwd_ref, ulp

NT, NN, TN = 0, 1, 2
IGNORE = -100
# positional arguments a call writes (ssi/ops.py); a None among them is skipped
OUTPUTS = {"embed_fwd": (2,), "rmsnorm_fwd": (2, 3), "gemm_rope": (2,), "attn_fwd": (1, 2), "gemm": (3,), "gemm_splitk": (3,), "gemm_batched": (3,),
           "gemm_swiglu_fwd": (2, 3), "gemm_swiglu_bwd": (4,), "rmsnorm_bwd": (5, 6), "attn_bwd": (4, 5), "embed_bwd": (2,), "ce_fwd": (0, 4),
           "ce_reduce": (4,)}


# =====================================================================================================================
# capture
# =====================================================================================================================
class Call:
    """One call: ``enc`` the tracer's entry; ``before`` / ``after`` CPU copies of the tensor arguments ([positional list, keyword dict])."""
    def __init__(self, name, args, kw, enc, before):
        self.name, self.args, self.kw, self.enc, self.before, self.after, self.ret = name, args, kw, enc, before, None, None


def _copies(args, kw):
    cp = lambda v: v.detach().cpu().clone() if isinstance(v, torch.Tensor) else None  # noqa: E731
    return [cp(a) for a in args], {k: cp(v) for k, v in kw.items()}


class Capture(Tracer):
    """``with cap.capture(): step`` -> ``cap.calls``.  ``values=False`` keeps the entries alone (operands too large to copy)."""
    def __init__(self, values=True):
        super().__init__()
        self.values, self.calls = values, []

    def call(self, name, fn, args, kw):
        c = Call(name, args, kw, self.entries[-1], _copies(args, kw) if self.values else None)
        ret = fn(*args, **kw)
        if self.values:
            c.after = _copies(args, kw)
            c.ret = _copies(ret if isinstance(ret, tuple) else (ret,), {})[0]
        c.args = c.kw = None          # (no reference to device memory is kept)
        self.calls.append(c)
        return ret

    @contextlib.contextmanager
    def capture(self):
        self.calls = []
        with self.scenario():
            yield self

    def emit(self, name, fn, *args, **kw):
        """A stand-in's call (tests/test_step_stages_ref.py): recorded exactly as a wrapped ``ssi.ops`` function records the model's."""
        if self.entries is None:
            self.entries = []
        return self.traced(name, fn, args, kw)


class Write(NamedTuple):
    call: int
    arg: int
    off: Optional[int]       # element offset in its buffer (None: a tensor outside the watched buffers)
    shape: tuple
    stride: tuple


def writes_of(calls):
    """buffer -> its writes in call order.  A tensor outside the watched buffers goes under ``ext.<op>``."""
    w = {}
    for i, c in enumerate(calls):
        for j in OUTPUTS.get(c.name, ()):
            loc = c.enc[1][j] if j < len(c.enc[1]) else None
            if not isinstance(loc, list) or (c.name == "ce_fwd" and j == 0 and not c.enc[1][6]):
                continue
            if len(loc) == 5:
                w.setdefault(loc[0], []).append(Write(i, j, loc[1], tuple(loc[2]), tuple(loc[3])))
            else:
                w.setdefault("ext." + c.name, []).append(Write(i, j, None, tuple(loc[1]), ()))
    return w


def split_micro_batches(calls):
    """The calls of each micro-batch: one starts at every ``embed_fwd``, or at the ``doc_ranges`` of packed rows just before it."""
    starts = [i - (i > 0 and calls[i - 1].name == "doc_ranges") for i, c in enumerate(calls) if c.name == "embed_fwd"] + [len(calls)]
    return [calls[a:b] for a, b in zip(starts, starts[1:])]


# =====================================================================================================================
# geometry and THE table
# =====================================================================================================================
def _align(n, a):
    return (n + a - 1) // a * a


def flat_layout(p, vocab_pad):
    """name -> (offset, shape) in the flat parameter / gradient buffer: the embedding, every layer's attention projections one after the other,
    every layer's MLP block, the final norm; each slice starts on a multiple of 8 elements (asserted against the model's on the GPU)."""
    D, I, L = p["embed_dim"], p["intermediate_dim"], p["num_layers"]
    hd = D // p["num_heads"]
    qkv = (p["num_heads"] + 2 * p["num_kv_heads"]) * hd
    out, off = {}, 0

    def take(name, shape):
        nonlocal off
        out[name] = (off, shape)
        n = 1
        for s in shape:
            n *= s
        off += _align(n, 8)
    take("emb", (vocab_pad, D))
    for l in range(L):
        take(f"L{l}.wqkv", (qkv, D))
        take(f"L{l}.wo", (D, p["num_heads"] * hd))
    for l in range(L):
        take(f"L{l}.w13", (2 * I, D))
        take(f"L{l}.w2", (D, I))
        take(f"L{l}.sa_norm", (D,))
        take(f"L{l}.mlp_norm", (D,))
    take("norm", (D,))
    return out, off


class Geom:
    def __init__(self, params, dtype, rope, wgrad_group, vocab_pad, eps=NORM_EPS):
        self.L, self.H, self.KV = params["num_layers"], params["num_heads"], params["num_kv_heads"]
        self.D, self.I, self.V, self.Vp = params["embed_dim"], params["intermediate_dim"], params["vocab_size"], vocab_pad
        self.hd = self.D // self.H
        self.Q, self.qkv = self.H * self.hd, (self.H + 2 * self.KV) * self.hd
        self.dtype, self.rope, self.Gp = dtype, rope.detach().cpu(), wgrad_group
        self.slices, self.numel = flat_layout(params, vocab_pad)
        assert self.hd == A.HD and eps == NORM_EPS, "attn_stress is written for head_dim 64, rms_*_ref for eps 1e-5"

    @classmethod
    def of(cls, model, params):
        g = cls(params, model.dtype, model._rope, model.wgrad_group, model.vocab_pad, model.norm_eps)
        assert g.slices == model._slices and g.numel == model._flat_numel, "flat_layout no longer restates the model's parameter layout"
        return g

    def weights(self, flat):
        flat = flat.detach().cpu()
        return {n: flat[o:o + torch.Size(s).numel()].view(s).double() for n, (o, s) in self.slices.items()}


def value_table(g, T, defer, head):
    """name -> ("w", buffer, k, offset, shape): the k-th write of the micro-batch to ``buffer``, which must be ``shape`` at element ``offset``;
    ("arg", buffer, k, which): an argument (as it was BEFORE the call) of the call that made that write — the gradients that arrive from outside.
    ``head``: "fused" (tied head + cross-entropy in the model), "logits" (``_HeadLogitsFn``), "hidden" (``forward_hidden`` alone).
    Layer l is the j-th of the backward, j = L - 1 - l.  Grouped weight gradients (``defer``) keep d hmid and d qkv of layer l in slot l % Gp."""
    L, D, I, Q, X, H = g.L, g.D, g.I, g.Q, g.qkv, g.H
    t = {"h.0": ("w", "h0", 0, 0, (T, D)), "hn": ("w", "hn", 0, 0, (T, D)), "rstdf": ("w", "rstdf", 0, 0, (T,)),
         f"dh.{L}": ("w", "dh.a", 0, 0, (T, D))}
    for l in range(L):
        j = L - 1 - l
        slot = l % g.Gp
        t.update({
            f"xn1.{l}": ("w", "xn1.all", l, l * T * D, (T, D)), f"rstd1.{l}": ("w", f"rstd1.{l}", 0, 0, (T,)),
            f"qkv.{l}": ("w", f"qkv.{l}", 0, 0, (T, X)), f"att.{l}": ("w", "att.all", l, l * T * Q, (T, Q)),
            f"lse.{l}": ("w", f"lse.{l}", 0, 0, (T * H,)), f"hmid.{l}": ("w", f"hmid.{l}", 0, 0, (T, D)),
            f"xn2.{l}": ("w", f"xn2.{l}", 0, 0, (T, D)), f"rstd2.{l}": ("w", f"rstd2.{l}", 0, 0, (T,)),
            f"gu.{l}": ("w", f"gu.{l}", 0, 0, (T, 2 * I)), f"act.{l}": ("w", f"act.{l}", 0, 0, (T, I)),
            f"h.{l + 1}": ("w", f"h{l + 1}", 0, 0, (T, D)),
            f"dgu.{l}": ("w", "dgu", j, 0, (T, 2 * I)), f"dxn2.{l}": ("w", "dxn", 2 * j, 0, (T, D)),
            f"dhmid.{l}": ("w", "dh.b.all", j, slot * T * D, (T, D)) if defer else ("w", "dh.b", j, 0, (T, D)),
            f"datt.{l}": ("w", "datt", j, 0, (T, Q)),
            f"dqkv.{l}": ("w", "dqkv.all", j, slot * T * X, (T, X)) if defer else ("w", "dqkv", j, 0, (T, X)),
            f"dxn1.{l}": ("w", "dxn", 2 * j + 1, 0, (T, D)), f"dh.{l}": ("w", "dh.a", j + 1, 0, (T, D))})
    if head == "fused":
        t.update({"logits": ("w", "logits", 0, 0, (T, g.Vp)), "dlogits": ("w", "logits", 1, 0, (T, g.Vp)), "row_loss": ("w", "row_loss", 0, 0, (T,)),
                  "stats": ("w", "ext.ce_reduce", 0, None, (4,)), "d_hn": ("w", "d_hn", 0, 0, (T, D)), "alpha": ("arg", "d_hn", 0, "alpha_dev")})
    elif head == "logits":
        t.update({"logits": ("w", "ext.gemm", 0, None, (T, g.Vp)), "d_hn": ("w", "d_hn", 0, 0, (T, D)), "dlogits": ("arg", "d_hn", 0, 1)})
    else:
        t["d_hn"] = ("arg", "dh.a", 0, 0)
    return t


class Step:
    """The stored values of one micro-batch, by name; the writes into the gradient buffer in order."""
    def __init__(self, calls, g, T, defer, head):
        self.calls, self.g, self.T = calls, g, T
        self.writes = writes_of(calls)
        self.table = value_table(g, T, defer, head)

    def _write(self, name):
        kind, buf, k, off, shape = self.table[name]
        ws = self.writes.get(buf, [])
        assert k < len(ws), f"stored value {name}: buffer {buf!r} has {len(ws)} writes in this micro-batch, the table wants write {k}"
        w = ws[k]
        assert w.off == off and tuple(w.shape) == tuple(shape), (f"stored value {name}: write {k} to {buf!r} is {w.shape} at {w.off}, "
                                                                 f"the table says {shape} at {off}")
        return w

    def __getitem__(self, name):
        e = self.table[name]
        if e[0] == "arg":
            ws = self.writes.get(e[1], [])
            assert e[2] < len(ws), f"stored value {name}: no write {e[2]} to {e[1]!r}"
            c = self.calls[ws[e[2]].call]
            return c.before[1][e[3]] if isinstance(e[3], str) else c.before[0][e[3]]
        w = self._write(name)
        return self.calls[w.call].after[0][w.arg]

    def grad_writes(self):
        """[(slice name, first row, before, after, op name, call index)] of every chunk a call wrote into the gradient buffer, in order."""
        out = []
        for w in self.writes.get("grad", []):
            c = self.calls[w.call]
            b, a = c.before[0][w.arg], c.after[0][w.arg]
            chunks = [(w.off, b, a)] if len(w.shape) < 3 else [(w.off + i * w.stride[0], b[i], a[i]) for i in range(w.shape[0])]
            for off, bb, aa in chunks:
                name = next(n for n, (o, s) in self.g.slices.items() if o <= off < o + torch.Size(s).numel())
                o, s = self.g.slices[name]
                cols = s[1] if len(s) == 2 else s[0]
                assert (off - o) % cols == 0 and (len(w.shape) == 1 or w.stride[-2] == cols), f"a write into {name} that is not whole rows"
                out.append([name, (off - o) // cols if len(s) == 2 else 0, bb, aa, c.name, w.call])
        return out


# =====================================================================================================================
# checker
# =====================================================================================================================
class StageFailure(AssertionError):
    def __init__(self, stage, layer, message):
        super().__init__(message)
        self.stage, self.layer = stage, layer


class Checker:
    """Judges stage after stage; records the worst error / bound per stage (``worst``) and the blind share of the attention rows (``blind``)."""
    def __init__(self, scenario, worst=None):
        self.scenario, self.worst, self.blind, self.mb = scenario, {} if worst is None else worst, {}, 0

    def _where(self, stage, layer):
        return f"[{self.scenario}] stage {stage}" + ("" if layer is None else f", layer {layer}") + f", micro-batch {self.mb}"

    def _note(self, stage, ratio):
        self.worst[stage] = max(self.worst.get(stage, 0.0), ratio)

    def elem(self, stage, got, ref, bound, layer=None):
        got64 = got.detach().double()
        assert got64.shape == ref.shape, f"{self._where(stage, layer)}: shape {tuple(got64.shape)} vs {tuple(ref.shape)}"
        err = (got64 - ref).abs()
        bound = bound.expand_as(err)
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        if bool((err <= bound).all()):
            self._note(stage, float(ratio.max()) if ratio.numel() else 0.0)
            return
        w = tuple(int(v) for v in torch.unravel_index(ratio.argmax(), ratio.shape))
        raise StageFailure(stage, layer, f"{self._where(stage, layer)}: {int((~(err <= bound)).sum())} of {err.numel()} elements miss their bound; "
                           f"worst at {w}: got {float(got64[w])!r} ref {float(ref[w])!r} err {float(err[w]):.3e} bound {float(bound[w]):.3e}")

    def bits(self, stage, got, ref, layer=None):
        ok = got.shape == ref.shape and got.dtype == ref.dtype and torch.equal(got.contiguous().view(torch.uint8), ref.contiguous().view(torch.uint8))
        if ok:
            self._note(stage, 0.0)
            return
        ne = (got.double() != ref.double()).nonzero() if got.shape == ref.shape else []
        raise StageFailure(stage, layer, f"{self._where(stage, layer)}: not bit for bit ({len(ne)} elements differ in value"
                           + (f", first at {tuple(int(v) for v in ne[0])})" if len(ne) else ")"))

    def zero(self, stage, got, layer=None, where=None):
        """Every element of ``got`` (``where`` given: of its rows ``where``) is 0."""
        bad = (got != 0) if where is None else (got != 0) & where[..., None]
        if bool(bad.any()):
            i = tuple(int(v) for v in bad.nonzero()[0])
            raise StageFailure(stage, layer, f"{self._where(stage, layer)}: {int(bad.sum())} elements that must be 0 are not, first at {i}: "
                               f"{float(got[i])!r}; largest {float(got.double().abs()[bad].max()):.3e}")

    def rows(self, stage, res, layer):
        self._note(stage, res.worst)
        self.blind[(stage, layer, self.mb)] = res.blind
        if not res.ok:
            raise StageFailure(stage, layer, f"{self._where(stage, layer)}: {res.message}")

    def need(self, cond, stage, layer, message):
        if not cond:
            raise StageFailure(stage, layer, f"{self._where(stage, layer)}: {message}")

    def table(self):
        return "\n".join(f"step-stages worst error / bound  {s:<14s} {v:.4f}" for s, v in self.worst.items())


def _up(v, dtype):
    """ulp of the storage type at |v| (taken where the error a value arrives with can have lifted it)."""
    return ulp(v.abs(), dtype)


def gemm_stage(a, b, dtype, alpha=None, prev=()):
    """ref and bound of ``[prev +] alpha a @ b`` (float64 operands holding the stored values; K = a.shape[1] terms per element)."""
    K = a.shape[1]
    p, e = a @ b, K * U32 * (a.abs() @ b.abs())
    if alpha is not None:
        p, e = alpha * p, abs(alpha) * e
        e = e + 2 * U32 * p.abs()                       # alpha and the device scalar: two fp32 products
    e = e + _up(p.abs() + e, dtype)                     # p ROUNDED TO STORAGE
    if not prev:
        return p, e
    ref, mag = p, p.abs()
    for x in prev:
        ref, mag = ref + x, mag + x.abs()
    e = e + len(prev) * U32 * mag                       # one fp32 add per previous value / residual
    return ref, e + _up(ref.abs() + e, dtype)           # ROUNDED TO STORAGE


def rope_stage(p, bp, table, pos, n_rot, dtype, hd=A.HD):
    """Adjacent-pair rotation of the first ``n_rot`` heads of p (which arrives within bp): two fp32 products and their sum or difference, then
    ONE rounding to storage; the other columns pass."""
    rows, rc = p.shape[0], n_rot * hd
    cs = table.double()[pos.long()]
    c, s = cs[:, None, :, 0], cs[:, None, :, 1]
    v, bv = p[:, :rc].reshape(rows, n_rot, hd // 2, 2), bp[:, :rc].reshape(rows, n_rot, hd // 2, 2)
    x0, x1, b0, b1 = v[..., 0], v[..., 1], bv[..., 0], bv[..., 1]
    o = torch.stack([x0 * c - x1 * s, x1 * c + x0 * s], -1).reshape(rows, rc)
    m0, m1 = x0.abs() + b0, x1.abs() + b1
    mag = torch.stack([m0 * c.abs() + m1 * s.abs(), m1 * c.abs() + m0 * s.abs()], -1).reshape(rows, rc)
    car = torch.stack([b0 * c.abs() + b1 * s.abs(), b1 * c.abs() + b0 * s.abs()], -1).reshape(rows, rc) + 2 * U32 * mag
    return torch.cat([o, p[:, rc:]], 1), torch.cat([car + _up(o.abs() + car, dtype), bp[:, rc:]], 1)


class Batch(NamedTuple):
    """What the reference knows of a micro-batch, from the data alone: padded tokens and shifted labels ([B, S]), the documents of every row
    (tuples of lengths, or None), whether the positions are explicit, whether the window already holds gradients, which head ran."""
    tokens: torch.Tensor
    labels: Optional[torch.Tensor]
    docs: Optional[tuple] = None
    accumulate: bool = False
    head: str = "fused"
    frozen: tuple = ()              # names of slices whose gradient nobody reads
    emb_rows: Optional[tuple] = None  # (r0, r1): the only rows of the embedding gradient that mean anything


def right_pad(tokens, labels, S):
    """The reference's batch format: tokens padded with 0, labels with the ignore index, up to S positions."""
    B, S0 = tokens.shape
    if S == S0:
        return tokens, labels
    return (torch.cat([tokens, torch.zeros(B, S - S0, dtype=tokens.dtype)], 1),
            None if labels is None else torch.cat([labels, torch.full((B, S - S0), IGNORE, dtype=labels.dtype)], 1))


STALE = 3.0            # what the tests put into the gradient buffer before a window: the first backward must WRITE over it


def seeded(params, b, s, seed, S=None, accumulate=False, **kw):
    """``hf_crosscheck.seeded_batch`` with its labels shifted, as a ``Batch``."""
    from oracle import hf_crosscheck as hx
    bt = hx.seeded_batch(params["vocab_size"], b, s, seed)
    labels = torch.hstack((bt["labels"][:, 1:], torch.full_like(bt["labels"][:, -1:], IGNORE)))
    return Batch(*right_pad(bt["tokens"], labels, S or s), accumulate=accumulate, **kw)


def ragged_batch(params):
    """Rows of 100, 57 and 1 real tokens; the third row has every label ignored (its one token has no successor)."""
    g = torch.Generator().manual_seed(5)
    tokens = torch.randint(1, params["vocab_size"], (3, 100), generator=g)
    labels = tokens.clone()
    for row, n in enumerate((100, 57, 1)):
        tokens[row, n:], labels[row, n:] = 0, IGNORE
    return tokens, torch.hstack((labels[:, 1:], torch.full_like(labels[:, -1:], IGNORE)))


def packed_batch(params):
    bt = seeded(params, 2, 512, 22, docs=A.DOC_ROWS)
    return bt, torch.stack([A.doc_arrays((row,), 512)[2].long() for row in A.DOC_ROWS])


def check_step(ck, st, W, bt):
    """All stages of one micro-batch, in the order of the data flow: the first stage that misses raises ``StageFailure`` (what it feeds is
    computed from ITS stored value and is not to blame)."""
    g, dt = st.g, st.g.dtype
    L, H, KV, D, I, V = g.L, g.H, g.KV, g.D, g.I, g.V
    B, S = bt.tokens.shape
    T = B * S
    tok = bt.tokens.reshape(-1)
    f64 = lambda name: st[name].double()  # noqa: E731
    bf = dt == torch.bfloat16
    eps = A.EPS_BF16 if bf else A.EPS_F32
    if bt.docs is not None:
        ds, de, pos = A.doc_arrays(bt.docs, S)
        dr = next(c for c in st.calls if c.name == "doc_ranges")
        for name, got, want in zip(("positions", "doc_start", "doc_end"), dr.ret, (pos, ds, de)):
            ck.bits("doc_ranges", got, want)
    else:
        pos = torch.arange(S, dtype=torch.int32).repeat(B)

    # ---- no call changes what it only reads (workspaces aside) ---------------------------------------------------------------------
    for c in st.calls:
        outs = OUTPUTS.get(c.name)
        if outs is None or c.before is None:
            continue
        for j, (b4, after, loc) in enumerate(zip(c.before[0], c.after[0], c.enc[1])):
            scratch = isinstance(loc, list) and len(loc) == 5 and (loc[0].startswith("ws.") or loc[0] in ("dact", "delta"))
            if b4 is not None and j not in outs and not scratch:
                ck.bits("inputs kept", after, b4)
        for k, b4 in c.before[1].items():
            if b4 is not None and k != "workspace":
                ck.bits("inputs kept", c.after[1][k], b4)

    # ---- forward ---------------------------------------------------------------------------------------------------------------------
    ck.bits("tokens", next(c for c in st.calls if c.name == "embed_fwd").before[0][0], tok)
    ck.bits("embed", st["h.0"], W["emb"][tok].to(dt))
    attn = {}
    for l in range(L):
        rstd, b_r, y, b_y = rms_fwd_ref(f64(f"h.{l}"), W[f"L{l}.sa_norm"], dt)
        ck.elem("rstd1", st[f"rstd1.{l}"], rstd, b_r, l)
        ck.elem("xn1", st[f"xn1.{l}"], y, b_y, l)
        p, bp = gemm_stage(f64(f"xn1.{l}"), W[f"L{l}.wqkv"].t(), dt)
        ck.elem("qkv", st[f"qkv.{l}"], *rope_stage(p, bp, g.rope, pos, H + KV, dt), l)
        qkv, datt = st[f"qkv.{l}"], st[f"datt.{l}"]
        ex = A.exact_of(qkv, datt, B, S, H, KV, bt.docs)
        rs = A.restate_of(qkv, datt, B, S, H, KV, bt.docs) if bf else A.f32_restated(ex)
        attn[l] = (ex, rs)
        ck.rows("att", A.row_check(st[f"att.{l}"], ex["out"], rs["out"], "out", B, S, eps=eps, name=f"layer {l}"), l)
        ck.elem("lse", st[f"lse.{l}"], ex["lse"], torch.full_like(ex["lse"], ex["lse_tol"]), l)
        ck.elem("hmid", st[f"hmid.{l}"], *gemm_stage(f64(f"att.{l}"), W[f"L{l}.wo"].t(), dt, prev=(f64(f"h.{l}"),)), l)
        rstd, b_r, y, b_y = rms_fwd_ref(f64(f"hmid.{l}"), W[f"L{l}.mlp_norm"], dt)
        ck.elem("rstd2", st[f"rstd2.{l}"], rstd, b_r, l)
        ck.elem("xn2", st[f"xn2.{l}"], y, b_y, l)
        ck.elem("gu", st[f"gu.{l}"], *gemm_stage(f64(f"xn2.{l}"), W[f"L{l}.w13"].t(), dt), l)
        act, b_act, _ = swiglu_fwd_ref(st[f"gu.{l}"], dt)
        ck.elem("act", st[f"act.{l}"], act, b_act, l)
        ck.elem("h_out", st[f"h.{l + 1}"], *gemm_stage(f64(f"act.{l}"), W[f"L{l}.w2"].t(), dt, prev=(f64(f"hmid.{l}"),)), l)
    rstd, b_r, y, b_y = rms_fwd_ref(f64(f"h.{L}"), W["norm"], dt)
    ck.elem("rstdf", st["rstdf"], rstd, b_r)
    ck.elem("hn", st["hn"], y, b_y)
    alpha = None
    if bt.head != "hidden":
        ck.elem("logits", st["logits"], *gemm_stage(f64("hn"), W["emb"].t(), dt))
    if bt.head == "fused":
        labels = bt.labels.reshape(-1)
        valid = C.is_valid(labels, V)
        n_valid = int(valid.sum())
        exp = C.expected(C.Base(st["logits"], V), labels, C.mode("plain"), "row" if C.row_form(dt, g.Vp, V) else "generic")
        ck.elem("row_loss", st["row_loss"], *exp["row_loss"])
        dl = st["dlogits"]
        ck.elem("dlogits", dl[:, :V], *exp["grad"])
        ck.zero("dlogits pad", dl[:, V:])
        ck.zero("dlogits pad", dl[~valid])
        rl = f64("row_loss")
        stats = f64("stats")
        ck.elem("loss", stats[:1], rl.sum().reshape(1) / n_valid, ((T + 1) * U32 * rl.abs().sum() / n_valid).reshape(1))   # a sum of T terms, one division
        ck.bits("loss", st["stats"][2:], torch.tensor([n_valid, 0], dtype=torch.float32))
        a_ref = torch.tensor([1.0 / n_valid], dtype=torch.float64)
        ck.elem("alpha", st["alpha"], a_ref, 2 * U32 * a_ref)          # one fp32 division, within an ulp
        alpha = float(st["alpha"])

    # ---- backward --------------------------------------------------------------------------------------------------------------------
    grads = st.grad_writes()
    seen = set()

    def grad(name, stage, layer, a, b, al=None):
        """The one write into slice ``name``: [what the window held +] al a^T b."""
        if name in bt.frozen:
            ck.need(not [w for w in grads if w[0] == name], stage, layer, "a frozen slice was written")
            return
        mine = [w for w in grads if w[0] == name]
        ck.need(len(mine) == 1 and tuple(mine[0][3].shape) == tuple(g.slices[name][1]), stage, layer,
                f"{len(mine)} writes into the gradient slice {name}, the step makes one of the whole slice")
        seen.add(name)
        _, _, before, after, _, _ = mine[0]
        ck.elem(stage, after, *gemm_stage(a.t(), b, dt, alpha=al, prev=(before.double(),) if bt.accumulate else ()), layer)

    def norm_bwd(scale, dy, x, rstd, dres, stage, layer, dx_name):
        mine = [w for w in grads if w[0] == scale]
        ck.need(len(mine) == 1, "dscale", layer, f"{len(mine)} writes into {scale}")
        seen.add(scale)
        dx, b_dx, dsc, b_ds = rms_bwd_ref(dy, x, W[scale], rstd, dres, mine[0][2] if bt.accumulate else None, dt)
        ck.elem(stage, st[dx_name], dx, b_dx, layer)
        ck.elem("dscale", mine[0][3], dsc, b_ds, layer)

    if bt.head != "hidden":
        dlog = f64("dlogits")
        ck.elem("d_hn", st["d_hn"], *gemm_stage(dlog, W["emb"], dt, alpha=alpha))
    norm_bwd("norm", st["d_hn"].reshape(T, D), st[f"h.{L}"], st["rstdf"], None, "dh final", None, f"dh.{L}")
    for l in reversed(range(L)):
        dh = f64(f"dh.{l + 1}")
        grad(f"L{l}.w2", "dW2", l, dh, f64(f"act.{l}"))
        # d act = dh W2 is ROUNDED TO STORAGE before the SwiGLU backward, which is linear in it: its error times |d dgu / d dact|
        dact, e_dact = gemm_stage(dh, W[f"L{l}.w2"], dt)
        gu = st[f"gu.{l}"]
        ref, _ = swiglu_bwd_ref(gu, dact, dt)
        _, b_in = swiglu_bwd_ref(gu, dact.abs() + e_dact, dt)          # the kernel's own roundings, at the magnitudes it can see
        deriv, _ = swiglu_bwd_ref(gu, torch.ones_like(dact), dt)
        ck.elem("dgu", st[f"dgu.{l}"], ref, b_in + deriv.abs() * torch.cat([e_dact, e_dact], 1), l)
        ck.elem("dxn mlp", st[f"dxn2.{l}"], *gemm_stage(f64(f"dgu.{l}"), W[f"L{l}.w13"], dt), l)
        grad(f"L{l}.w13", "dW13", l, f64(f"dgu.{l}"), f64(f"xn2.{l}"))
        norm_bwd(f"L{l}.mlp_norm", st[f"dxn2.{l}"], st[f"hmid.{l}"], st[f"rstd2.{l}"], st[f"dh.{l + 1}"], "dhmid", l, f"dhmid.{l}")
        ck.elem("datt", st[f"datt.{l}"], *gemm_stage(f64(f"dhmid.{l}"), W[f"L{l}.wo"], dt), l)
        grad(f"L{l}.wo", "dWo", l, f64(f"dhmid.{l}"), f64(f"att.{l}"))
        ex, rs = attn[l]
        if bf:
            e_d, r_d = A.rope_refs(ex, rs, g.rope, pos, H, KV)
        else:
            e_d = A.rope_transpose(ex["dqkv"], g.rope, pos, H, KV)
            r_d = e_d.float().double()
        dqkv = st[f"dqkv.{l}"]
        for block in A.BLOCKS:
            lo, hi = A.block_cols(block, H, KV)
            # a (batch row, head) whose gradient is 0 in every row of both references (every label that could reach it ignored: d att is 0
            # there) has E_row = 0 throughout: its rows are left out of row_check and must BE 0.  (A single row that is 0 by cancellation —
            # position 0, where P = 1 and dP = delta — sits under the rms floor of its batch row like any other.)
            mag = (e_d[:, lo:hi].abs() + r_d[:, lo:hi].abs()).view(B, S, -1, A.HD).sum((1, 3))
            dead = (mag == 0)[:, None, :].expand(B, S, -1)
            ck.zero(block, dqkv[:, lo:hi].view(B, S, -1, A.HD), l, where=dead)
            ck.rows(block, A.row_check(dqkv[:, lo:hi], e_d[:, lo:hi], r_d[:, lo:hi], block, B, S, eps=eps, exempt=dead,
                                       dq_cond=ex["dq_cond"] if block == "dq" else None, name=f"layer {l}"), l)
        ck.elem("dxn attn", st[f"dxn1.{l}"], *gemm_stage(dqkv.double(), W[f"L{l}.wqkv"], dt), l)
        grad(f"L{l}.wqkv", "dWqkv", l, dqkv.double(), f64(f"xn1.{l}"))
        norm_bwd(f"L{l}.sa_norm", st[f"dxn1.{l}"], st[f"h.{l}"], st[f"rstd1.{l}"], st[f"dhmid.{l}"], "dh", l, f"dh.{l}")

    # ---- the tied embedding: the head's part, then the scatter-add of d h0 on top -------------------------------------------------
    emb = [w for w in grads if w[0] == "emb"]
    seen.add("emb")
    if "emb" in bt.frozen:
        ck.need(not emb, "dE head", None, "the frozen embedding gradient was written")
        return
    r0, r1 = bt.emb_rows or (0, g.Vp)
    head_part, scat = emb[:-1], emb[-1] if emb else None
    ck.need(scat is not None and scat[4] == "embed_bwd" and scat[1] == 0 and scat[3].shape[0] == g.Vp, "dE scatter", None,
            "the last write into the embedding gradient is not the scatter-add over the whole table")
    if bt.head != "hidden":
        rows = sorted((w[1], w[1] + w[3].shape[0]) for w in head_part)
        ck.need(rows and rows[0][0] == r0 and rows[-1][1] == r1 and all(a[1] == b[0] for a, b in zip(rows, rows[1:])), "dE head", None,
                f"the head's launches cover rows {rows} of the embedding gradient, not [{r0}, {r1}) once")
        hn = f64("hn")
        for _, lo, before, after, _, _ in head_part:
            hi = lo + after.shape[0]
            ck.elem("dE head", after, *gemm_stage(dlog[:, lo:hi].t(), hn, dt, alpha=alpha, prev=(before.double(),) if bt.accumulate else ()))
        for _, lo, _, after, _, _ in head_part:
            ck.bits("dE head", scat[2][lo:lo + after.shape[0]], after)   # what the scatter-add found is what the head left
    else:
        ck.need(not head_part, "dE head", None, "a head write without a head")
        if not bt.accumulate:
            ck.zero("dE scatter", scat[2])                               # no head in front: the scatter-add starts from zeros
    before, after = scat[2].double(), scat[3]
    dh0 = f64("dh.0")
    counts = torch.bincount(tok, minlength=g.Vp)
    ref = before.index_add(0, tok, dh0)
    mag = before.abs().index_add(0, tok, dh0.abs())
    ck.elem("dE scatter", after[r0:r1], ref[r0:r1], ((counts[:, None].double() + 1) * U32 * mag + ulp(ref, dt))[r0:r1])
    ck.bits("dE scatter", after[r0:r1][counts[r0:r1] == 0], scat[2][r0:r1][counts[r0:r1] == 0])
    missing = [n for n in g.slices if n not in seen and n not in bt.frozen]
    assert not missing, f"[{ck.scenario}] gradient slices never checked: {missing}"
