"""Dry run of tests/step_stages.py on the CPU: a stand-in for the model — every stage emulated in torch with fp32 math and the documented
roundings to storage, issued call by call through ``Capture.emit`` on named CPU buffers, so that it leaves a capture of the form the model
leaves — goes through the same table and the same checker as the GPU scenarios of tests/test_step_stages_gpu.py.

  * the reference passes: a bound that a correct restatement does not meet is a wrong bound, found here (worst ratios printed, -s);
  * blind share: on the stand-in's stored qkv / d att the share of attention rows whose tolerance would let a wrong value pass is at most
    ``attn_stress.BLIND_CAP`` in every layer.  Measured with the seeded weights as they are (hf_crosscheck.seeded_state_dict, std 0.05):
    at most 1.07 % (dq, layer 1 of the plain scenario; dk, dv and out 0.00 %), printed per scenario and layer at the end of the run (-s);
  * teeth: each planted defect of the composition fails, at the stage that has it.
"""
import copy
import types

import pytest
import torch

import attn_stress as A
import ce_parity as C
import step_stages as SS
from launch_trace import MFMA_PARAMS, PLAN_PARAMS
from oracle import hf_crosscheck as hx

BF, F32 = torch.bfloat16, torch.float32
NT, NN, TN = SS.NT, SS.NN, SS.TN
WORST = {}
BLIND = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for s, v in WORST.items():
        print(f"\nstep-stages (stand-in) worst error / bound  {s:<14s} {v:.4f}", end="")
    for k, v in BLIND.items():
        print(f"\nstep-stages (stand-in) blind share  {k:<24s} {100 * v:.2f} %", end="")
    print()


# =====================================================================================================================
# the stand-in's kernels: fp32 math, one rounding to storage where the kernels document one
# =====================================================================================================================
def docs_of(ds, de, B, S):
    if ds is None:
        return None
    ds, de = ds.view(B, S), de.view(B, S)
    return tuple(tuple(int(de[b, s] - ds[b, s]) for s in range(S) if int(ds[b, s]) == s) for b in range(B))


def _rot(x32, table, pos, n_rot, hd=64):
    rows, rc = x32.shape[0], n_rot * hd
    cs = table[pos.long()]
    c, s = cs[:, None, :, 0], cs[:, None, :, 1]
    v = x32[:, :rc].reshape(rows, n_rot, hd // 2, 2)
    o = torch.stack([v[..., 0] * c - v[..., 1] * s, v[..., 1] * c + v[..., 0] * s], -1).reshape(rows, rc)
    return torch.cat([o, x32[:, rc:]], 1)


class Kernels:
    """The signatures of ``ssi.ops``; ``bug`` plants one defect (the teeth)."""
    def __init__(self, bug=None):
        self.bug = bug

    def embed_fwd(self, tok, table, out, vocab):
        out.copy_(table[tok])

    def rmsnorm_fwd(self, x, scale, y, rstd, eps):
        x32 = x.float()
        r = torch.rsqrt((x32 * x32).mean(-1) + eps)
        rstd.copy_(r)
        y.copy_(((x32 * r[:, None]).to(x.dtype).float() * scale.float()).to(x.dtype))

    def gemm_rope(self, a, b, c, seq_len, n_rot, hd, table, positions=None):
        p = (a.float() @ b.float().t()).to(c.dtype).float()
        pos = positions if positions is not None else torch.arange(a.shape[0]) % seq_len
        c.copy_(_rot(p, table, pos, n_rot, hd).to(c.dtype))

    def attn_fwd(self, qkv, out, lse, B, S, H, KV, hd, ds=None, de=None):
        docs, zero = docs_of(ds, de, B, S), torch.zeros(B * S, H * hd, dtype=qkv.dtype)
        r = A.restate_of(qkv, zero, B, S, H, KV, docs) if qkv.dtype == BF else A.exact_of(qkv, zero, B, S, H, KV, docs)
        out.copy_(r["out"].to(out.dtype))
        lse.copy_(r["lse"].float())

    def attn_bwd(self, qkv, out, dout, lse, dqkv, delta, B, S, H, KV, hd, ds=None, de=None, rope_table=None, positions=None, workspace=None, plan=None):
        docs = docs_of(ds, de, B, S)
        pos = positions if positions is not None else torch.arange(S, dtype=torch.int32).repeat(B)
        d = A.restate_of(qkv, dout, B, S, H, KV, docs)["dqkv_f32"] if qkv.dtype == BF else A.exact_of(qkv, dout, B, S, H, KV, docs)["dqkv"]
        if self.bug != "dqkv_post_rope":
            d = A.rope_transpose(d, rope_table, pos, H, KV)
        dqkv.copy_(d.float().to(dqkv.dtype))

    def gemm(self, layout, a, b, c, *, residual=None, alpha=1.0, alpha_dev=None, accumulate=False):
        a32, b32 = a.float(), b.float()
        s = a32 @ b32.t() if layout == NT else a32 @ b32 if layout == NN else a32.t() @ b32
        al = alpha * (float(alpha_dev) if alpha_dev is not None else 1.0)
        p = (s * al if al != 1.0 else s).to(c.dtype)
        if accumulate or residual is not None:
            p32 = p.float()
            if accumulate:
                p32 = p32 + c.float()
            if residual is not None:
                p32 = p32 + residual.float()
            p = p32.to(c.dtype)
        c.copy_(p)

    def gemm_splitk(self, layout, a, b, c, splits, workspace, **kw):
        self.gemm(layout, a, b, c, **kw)

    def gemm_batched(self, layout, a, b, c, **kw):
        for i in range(c.shape[0]):
            self.gemm(layout, a[i], b[i], c[i], **kw)

    def gemm_swiglu_fwd(self, x, w13, gu, act):
        gu.copy_((x.float() @ w13.float().t()).to(gu.dtype))
        inter = act.shape[1]
        g, u = gu[:, :inter].float(), gu[:, inter:].float()
        act.copy_(((g * torch.sigmoid(g)).to(act.dtype).float() * u).to(act.dtype))

    def gemm_swiglu_bwd(self, layout, dy, w2, gu, dgu, dact_ws):
        assert layout == NN
        d = (dy.float() @ w2.float()).to(dgu.dtype).float()
        inter = d.shape[1]
        g, u = gu[:, :inter].float(), gu[:, inter:].float()
        sig = torch.sigmoid(g)
        dgu.copy_(torch.cat([(d * u) * (sig * (1 + g * (1 - sig))), d * (g * sig)], 1).to(dgu.dtype))

    def rmsnorm_bwd(self, dy, x, scale, rstd, dres, dx, dscale, workspace=None, accumulate=True):
        xhat, gw = x.float() * rstd[:, None], dy.float() * scale.float()
        c = (gw * xhat).mean(-1, keepdim=True)
        v = rstd[:, None] * (gw - xhat * c)
        if dres is not None:
            v = v + dres.float()
        ds = (dy.float() * xhat).sum(0)
        if accumulate:
            ds = ds + dscale.float()
        dx.copy_(v.to(dx.dtype))
        dscale.copy_(ds.to(dscale.dtype))

    def embed_bwd(self, tok, dout, dtable, vocab, workspace=None):
        dtable.copy_(dtable.float().index_add(0, tok, dout.float()).to(dtable.dtype))

    def ce_fwd(self, logits, labels, vocab, ignore_index, row_loss, row_lse, write_grad, row_weight=None):
        form = "row" if C.row_form(logits.dtype, logits.shape[1], vocab) else "generic"
        out = C.restate(form, logits, labels, vocab, C.mode("plain"))
        row_loss.copy_(out["row_loss"])
        logits.copy_(out["grad"])

    def ce_reduce(self, row_loss, labels, vocab, ignore_index, out):
        valid = C.is_valid(labels, vocab)
        s = row_loss.sum()
        out.copy_(torch.stack([s / valid.sum(), s, valid.sum().float(), torch.zeros(())]))

    def doc_ranges(self, input_pos, max_pos, n_clamped=None):
        B, S = input_pos.shape
        rows = tuple(tuple(int(n) for n in torch.diff(torch.cat([(row == 0).nonzero().flatten(), torch.tensor([S])]))) for row in input_pos)
        ds, de, pos = A.doc_arrays(rows, S)
        return pos, ds, de


# =====================================================================================================================
# the stand-in for the model: the step's calls in the order of the equations, on named buffers
# =====================================================================================================================
class StandIn:
    def __init__(self, params, dtype, seed, wgrad_group, bug=None, weight_scale=1.0):
        from ssi.model import llama3_rope_table
        self.p, self.dtype, self.bug, self.k = params, dtype, bug, Kernels(bug)
        V, D = params["vocab_size"], params["embed_dim"]
        self.Vp = SS._align(V, 256)
        self._rope = llama3_rope_table(D // params["num_heads"], params["max_seq_len"])
        self.g = SS.Geom(params, dtype, self._rope, wgrad_group, self.Vp)
        sd = {k: v * (1.0 if k.endswith("scale") else weight_scale) for k, v in hx.seeded_state_dict(params, seed).items()}
        self._flat = torch.zeros(self.g.numel, dtype=dtype)
        self._flat_grad = torch.full((self.g.numel,), SS.STALE, dtype=dtype)
        put = lambda name, t: self.view(name)[: t.shape[0]].copy_(t.to(dtype))  # noqa: E731
        put("emb", sd["tok_embeddings.weight"])
        put("norm", sd["norm.scale"])
        for l in range(params["num_layers"]):
            a, m = f"layers.{l}.attn.", f"layers.{l}.mlp."
            put(f"L{l}.wqkv", torch.cat([sd[a + "q_proj.weight"], sd[a + "k_proj.weight"], sd[a + "v_proj.weight"]]))
            put(f"L{l}.wo", sd[a + "output_proj.weight"])
            put(f"L{l}.w13", torch.cat([sd[m + "w1.weight"], sd[m + "w3.weight"]]))
            put(f"L{l}.w2", sd[m + "w2.weight"])
            put(f"L{l}.sa_norm", sd[f"layers.{l}.sa_norm.scale"])
            put(f"L{l}.mlp_norm", sd[f"layers.{l}.mlp_norm.scale"])
        self._arena = types.SimpleNamespace(buf={})
        self.W = self.g.weights(self._flat)

    def view(self, name, grad=False):
        o, s = self.g.slices[name]
        return (self._flat_grad if grad else self._flat)[o:o + torch.Size(s).numel()].view(s)

    def buf(self, name, shape, dtype=None):
        n = torch.Size(shape).numel()
        if name not in self._arena.buf:
            self._arena.buf[name] = torch.zeros(n, dtype=dtype or self.dtype)
        return self._arena.buf[name][:n].view(shape)

    def step(self, cap, bt, explicit_pos=None):
        """One micro-batch: forward, head, backward.  ``bt``: a ``step_stages.Batch``; ``explicit_pos``: input_pos [B, S] of packed rows."""
        g, k, bug = self.g, self.k, self.bug
        L, H, KV, hd, D, I, Q, X, V, Vp = g.L, g.H, g.KV, g.hd, g.D, g.I, g.Q, g.qkv, g.V, g.Vp
        B, S = bt.tokens.shape
        T, acc, eps = B * S, bt.accumulate, SS.NORM_EPS
        bf = self.dtype == BF
        defer = g.Gp > 1 and bf
        E = lambda name, *a, **kw: cap.emit(name, getattr(k, name), *a, **kw)  # noqa: E731
        tok = bt.tokens.reshape(-1).contiguous()
        pos = ds = de = None
        if explicit_pos is not None:
            pos, ds, de = E("doc_ranges", explicit_pos, self._rope.shape[0] - 1, None)
        xn1_all, att_all = self.buf("xn1.all", (L, T, D)), self.buf("att.all", (L, T, Q))
        h = [self.buf("h0", (T, D))] + [self.buf(f"h{l + 1}", (T, D)) for l in range(L)]
        E("embed_fwd", tok, self.view("emb"), h[0], V)
        lay = []
        for l in range(L):
            b = types.SimpleNamespace(h_in=h[l], xn1=xn1_all[l], rstd1=self.buf(f"rstd1.{l}", (T,), F32), qkv=self.buf(f"qkv.{l}", (T, X)),
                                      att=att_all[l], lse=self.buf(f"lse.{l}", (T * H,), F32), hmid=self.buf(f"hmid.{l}", (T, D)),
                                      xn2=self.buf(f"xn2.{l}", (T, D)), rstd2=self.buf(f"rstd2.{l}", (T,), F32), gu=self.buf(f"gu.{l}", (T, 2 * I)),
                                      act=self.buf(f"act.{l}", (T, I)), h_out=h[l + 1])
            lay.append(b)
            E("rmsnorm_fwd", b.h_in, self.view(f"L{l}.sa_norm"), b.xn1, b.rstd1, eps)
            E("gemm_rope", b.xn1, self.view(f"L{l}.wqkv"), b.qkv, S, H + KV, hd, self._rope, positions=pos)
            E("attn_fwd", b.qkv, b.att, b.lse, B, S, H, KV, hd, ds, de)
            if bug == "hmid_no_residual" and l == L // 2:
                E("gemm", NT, b.att, self.view(f"L{l}.wo"), b.hmid, residual=b.h_in)
                k.gemm(NT, b.att[5:6], self.view(f"L{l}.wo"), b.hmid[5:6])          # row 5 without its residual
                cap.calls[-1].after[0][3][5] = b.hmid[5]
            else:
                E("gemm", NT, b.att, self.view(f"L{l}.wo"), b.hmid, residual=b.h_in)
            E("rmsnorm_fwd", b.hmid, self.view(f"L{l}.mlp_norm"), b.xn2, b.rstd2, eps)
            E("gemm_swiglu_fwd", b.xn2, self.view(f"L{l}.w13"), b.gu, b.act)
            E("gemm", NT, b.act, self.view(f"L{l}.w2"), b.h_out, residual=b.hmid)
            if bug == "h_out_stale" and l == 1:
                b.h_out[7] = h[l - 1][7]                                               # a row of what another h buffer held before
                cap.calls[-1].after[0][3][7] = b.h_out[7]
        hn, rstdf = self.buf("hn", (T, D)), self.buf("rstdf", (T,), F32)
        E("rmsnorm_fwd", h[L], self.view("norm"), hn, rstdf, eps)
        d_hn = self.buf("d_hn", (T, D))
        g_emb = self.view("emb", True)
        if bt.head == "fused":
            labels = bt.labels.reshape(-1).contiguous()
            logits, row_loss, stats = self.buf("logits", (T, Vp)), self.buf("row_loss", (T,), F32), torch.zeros(4)
            E("gemm", NT, hn, self.view("emb"), logits)
            E("ce_fwd", logits, labels, V, SS.IGNORE, row_loss, None, True, row_weight=None)
            E("ce_reduce", row_loss, labels, V, SS.IGNORE, stats)
            alpha = (torch.ones(1) / stats[2:3]).contiguous()
            E("gemm", NN, logits, self.view("emb"), d_hn, alpha_dev=alpha)
            if bug != "dE_no_head":
                if bt.emb_rows:
                    r0, r1 = bt.emb_rows
                    E("gemm", TN, logits[:, r0:r1], hn, g_emb[r0:r1], alpha_dev=alpha, accumulate=acc)
                else:
                    E("gemm", TN, logits, hn, g_emb, alpha_dev=alpha, accumulate=acc)
        elif bt.head == "logits":     # the logits leave the model; their gradient comes back from outside
            logits = torch.zeros(T, Vp, dtype=self.dtype)
            E("gemm", NT, hn, self.view("emb"), logits)
            dlog = (torch.softmax(logits.float(), -1) / T).to(self.dtype)
            dlog[:, V:] = 0
            E("gemm", NN, dlog, self.view("emb"), d_hn, alpha_dev=None)
            E("gemm", TN, dlog, hn, g_emb, alpha_dev=None, accumulate=acc)
        else:
            d_hn = (hn.float() / T).to(self.dtype)
            if not acc:
                g_emb.zero_()
        # ---- backward ----
        gv = lambda name: self.view(name, True)  # noqa: E731

        def wgrad(dy, x, name, a=None):
            if name not in bt.frozen:
                E("gemm_splitk" if bf else "gemm", TN, dy, x, gv(name), *((4, None) if bf else ()), accumulate=acc if a is None else a)

        Gp = g.Gp
        if defer:
            dhmid_all, dqkv_all = self.buf("dh.b.all", (Gp, T, D)), self.buf("dqkv.all", (Gp, T, X))
            lstride = g.slices["L1.wqkv"][0] - g.slices["L0.wqkv"][0] if L > 1 else 0
        dh = self.buf("dh.a", (T, D))
        E("rmsnorm_bwd", d_hn, h[L], self.view("norm"), rstdf, None, dh, gv("norm"), None, accumulate=acc)
        for l in reversed(range(L)):
            b = lay[l]
            wgrad(dh, b.act, f"L{l}.w2", a=False if (bug == "wgrad_write_not_add" and acc and l == 1) else None)
            dgu, dxn = self.buf("dgu", (T, 2 * I)), self.buf("dxn", (T, D))
            E("gemm_swiglu_bwd", NN, dh, self.view(f"L{l}.w2"), b.gu, dgu, None)
            E("gemm", NN, dgu, self.view(f"L{l}.w13"), dxn)
            wgrad(dgu, b.xn2, f"L{l}.w13")
            dhmid = dhmid_all[l % Gp] if defer else self.buf("dh.b", (T, D))
            E("rmsnorm_bwd", dxn, b.hmid, self.view(f"L{l}.mlp_norm"), b.rstd2, dh, dhmid, gv(f"L{l}.mlp_norm"), None, accumulate=acc)
            datt = self.buf("datt", (T, Q))
            E("gemm", NN, dhmid, self.view(f"L{l}.wo"), datt)
            if not defer:
                wgrad(dhmid, b.att, f"L{l}.wo")
            dqkv = dqkv_all[l % Gp] if defer else self.buf("dqkv", (T, X))
            E("attn_bwd", b.qkv, b.att, datt, b.lse, dqkv, self.buf("delta", (T * H,), F32), B, S, H, KV, hd, ds, de,
              rope_table=self._rope, positions=pos, workspace=None, plan=None)
            if bug == "dgrad_tail_stale" and l == 1:
                keep = dxn[T - 256:].clone()
                E("gemm", NN, dqkv, self.view(f"L{l}.wqkv"), dxn)
                dxn[T - 256:] = keep                                                   # the last 256-row tile never written
                cap.calls[-1].after[0][3][T - 256:] = keep
            else:
                E("gemm", NN, dqkv, self.view(f"L{l}.wqkv"), dxn)
            if not defer:
                wgrad(dqkv, b.xn1, f"L{l}.wqkv")
            E("rmsnorm_bwd", dxn, b.h_in, self.view(f"L{l}.sa_norm"), b.rstd1, dhmid, dh, gv(f"L{l}.sa_norm"), None, accumulate=acc)
            if defer and l % Gp == 0:
                n = min(Gp, L - l)
                att_n, xn1_n = att_all[l:l + n], xn1_all[l:l + n]
                if bug == "dWo_wrong_att" and n > 1:
                    att_n = att_all[l:l + 1].expand(n, T, Q)                         # the group's first layer for every layer
                g_o = torch.as_strided(self._flat_grad, (n, D, Q), (lstride, Q, 1), g.slices[f"L{l}.wo"][0])
                g_qkv = torch.as_strided(self._flat_grad, (n, X, D), (lstride, D, 1), g.slices[f"L{l}.wqkv"][0])
                if not all(f"L{i}.wo" in bt.frozen for i in range(l, l + n)):
                    E("gemm_batched", TN, dhmid_all[:n], att_n, g_o, accumulate=acc)
                if not all(f"L{i}.wqkv" in bt.frozen for i in range(l, l + n)):
                    E("gemm_batched", TN, dqkv_all[:n], xn1_n, g_qkv, accumulate=acc)
        if "emb" not in bt.frozen:
            t, d = tok, dh
            if bug == "dE_no_scatter_one":
                rep = next(i for i in range(1, T) if int(tok[i]) in tok[:i].tolist())    # a second occurrence of a token: left out
                keep = torch.arange(T) != rep
                t, d = tok[keep].contiguous(), dh[keep].contiguous()
                cap.emit("embed_bwd", lambda *_: k.embed_bwd(t, d, g_emb, V), tok, dh, g_emb, V, None)
            else:
                E("embed_bwd", tok, dh, g_emb, V, None)


def run_standin(model, batches, **kw):
    """A window of micro-batches -> [(Step, Batch)]."""
    cap = SS.Capture()
    cap.watch(model)
    out = []
    for bt in batches:
        cap.calls = []
        model.step(cap, bt, **kw)
        defer = model.g.Gp > 1 and model.dtype == BF
        out.append((SS.Step(cap.calls, model.g, bt.tokens.numel(), defer, bt.head), bt))
    return out


def check(name, model, steps, worst=WORST):
    ck = SS.Checker(name, worst)
    for i, (st, bt) in enumerate(steps):
        ck.mb = i
        SS.check_step(ck, st, model.W, bt)
    return ck


def _blind(name, ck):
    for (stage, layer, mb), share in ck.blind.items():
        BLIND[f"{name} {stage} L{layer}"] = max(BLIND.get(f"{name} {stage} L{layer}", 0.0), share)
        assert share <= A.BLIND_CAP, f"{name}: blind share of {stage}, layer {layer}: {share:.4f} > {A.BLIND_CAP}"


# =====================================================================================================================
# 1. the reference passes, in every scenario of the GPU file
# =====================================================================================================================
def test_plain_two_micro_batches_in_a_window():
    m = StandIn(MFMA_PARAMS, BF, 21, 2)
    steps = run_standin(m, [SS.seeded(MFMA_PARAMS, 2, 128, 21), SS.seeded(MFMA_PARAMS, 2, 128, 31, accumulate=True)])
    _blind("plain", check("plain", m, steps))


def test_per_layer_weight_gradients():
    m = StandIn(MFMA_PARAMS, BF, 21, 1)
    _blind("per-layer", check("per-layer", m, run_standin(m, [SS.seeded(MFMA_PARAMS, 2, 128, 21)])))


def test_ragged_rows_padded_to_whole_tiles():
    m = StandIn(MFMA_PARAMS, BF, 21, 2)
    bt = SS.Batch(*SS.right_pad(*SS.ragged_batch(MFMA_PARAMS), 256))
    _blind("ragged", check("ragged", m, run_standin(m, [bt])))


def test_packed_rows():
    m = StandIn(PLAN_PARAMS, BF, 22, 2)
    bt, input_pos = SS.packed_batch(PLAN_PARAMS)
    _blind("packed", check("packed", m, run_standin(m, [bt], explicit_pos=input_pos)))


def test_frozen_slices():
    m = StandIn(MFMA_PARAMS, BF, 21, 2)
    bt = SS.seeded(MFMA_PARAMS, 2, 128, 21, frozen=("L2.wqkv",), emb_rows=(256, 512))
    steps = run_standin(m, [bt])
    check("frozen", m, steps)
    assert bool((m.view("L2.wqkv", True) == SS.STALE).all())


@pytest.mark.parametrize("head", ["logits", "hidden"])
def test_unfused_head(head):
    m = StandIn(MFMA_PARAMS, BF, 21, 2)
    check(f"unfused {head}", m, run_standin(m, [SS.seeded(MFMA_PARAMS, 2, 128, 21, head=head)]))


def test_fp32():
    m = StandIn(MFMA_PARAMS, F32, 21, 2)
    steps = run_standin(m, [SS.seeded(MFMA_PARAMS, 2, 128, 21), SS.seeded(MFMA_PARAMS, 2, 128, 31, accumulate=True)])
    check("fp32", m, steps, worst={})


# =====================================================================================================================
# 2. teeth: every planted defect fails, at its own stage
# =====================================================================================================================
TEETH = [("hmid_no_residual", "hmid", 1, 1), ("h_out_stale", "h_out", 1, 1), ("dWo_wrong_att", "dWo", 1, 1), ("wgrad_write_not_add", "dW2", 1, 2),
         ("dE_no_head", "dE head", None, 1), ("dE_no_scatter_one", "dE scatter", None, 1), ("dqkv_post_rope", "dq", 2, 1)]


@pytest.mark.parametrize("bug,stage,layer,n_mb", TEETH, ids=[t[0] for t in TEETH])
def test_a_planted_defect_fails_at_its_stage(bug, stage, layer, n_mb):
    m = StandIn(MFMA_PARAMS, BF, 21, 2, bug=bug)
    batches = [SS.seeded(MFMA_PARAMS, 2, 128, 21), SS.seeded(MFMA_PARAMS, 2, 128, 31, accumulate=True)][:n_mb]
    with pytest.raises(SS.StageFailure) as e:
        check(bug, m, run_standin(m, batches), worst={})
    print(e.value)
    assert (e.value.stage, e.value.layer) == (stage, layer), str(e.value)
    assert f"micro-batch {n_mb - 1}" in str(e.value) and f"[{bug}]" in str(e.value)


def test_a_stale_last_tile_of_a_data_gradient_fails_at_its_stage():
    m = StandIn(MFMA_PARAMS, BF, 21, 2, bug="dgrad_tail_stale")
    with pytest.raises(SS.StageFailure) as e:     # T = 512: the last tile holds two rows with labels (a tile of ignored rows is 0 either way)
        check("tail", m, run_standin(m, [SS.seeded(MFMA_PARAMS, 4, 128, 21)]), worst={})
    assert (e.value.stage, e.value.layer) == ("dxn attn", 1), str(e.value)


def test_a_single_element_4_ulp_off_fails_at_its_stage():
    m = StandIn(MFMA_PARAMS, BF, 21, 2)
    steps = run_standin(m, [SS.seeded(MFMA_PARAMS, 2, 128, 21)])
    for name, stage in (("gu.1", "gu"), ("dxn2.0", "dxn mlp"), ("h.2", "h_out")):
        st = copy.deepcopy(steps[0][0])
        v = st[name]
        x = v[100, 37].double().reshape(1)
        v[100, 37] = (x + 4 * SS.ulp(x, BF)).to(BF)[0]
        with pytest.raises(SS.StageFailure) as e:
            check("4ulp", m, [(st, steps[0][1])], worst={})
        assert e.value.stage == stage and "(100, 37)" in str(e.value), str(e.value)
