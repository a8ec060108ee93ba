"""Llama-3.2 decoder with a DSU-extended, tied vocabulary on hand-written HIP kernels (gfx950).

Replaces what the reference builds at ``/root/reference/ssi/model.py:18-39`` (torchtune ``llama3_2(**params)``) and runs at
``/root/reference/ssi/loss.py:8-14``.  Public surface kept: ``setup_llama3_2_1b(cfg, llama_config, model_state_dict,
dtype_default, device_default)``; the returned module is callable as ``model(tokens=, mask=, encoder_input=,
encoder_mask=, input_pos=)``, has ``set_num_output_chunks``, exposes torchtune-format ``state_dict`` keys
 and populates ``p.grad`` on ``loss.backward()``.

MI355X-first design (not a module-per-op port):
* all parameters live in ONE flat HBM buffer (q/k/v fused to one [3072, D] weight, gate/up fused to one [2I, D] weight;
  the torchtune-named parameters are row-slice views), gradients and AdamW moments in matching flat buffers, so the
  optimizer is a single streaming kernel and data-parallel all-reduce works on contiguous per-layer buckets;
* the embedding table is stored with its row count padded to a multiple of 256 so that the LM-head GEMM, its dgrad and
  its wgrad run on full MFMA tiles (pad rows are zero and stay zero);
* forward/backward are two hand-scheduled kernel sequences over a persistent activation arena (stable pointers, no
  allocator traffic, no autograd graph of small ops) wrapped in three ``torch.autograd.Function`` seams:
  decoder stack, tied head -> logits, tied head + cross-entropy (logits are written once in the model dtype and turned
  into their gradient in place);
* there is no CPU path: constructing the model off-GPU raises.
"""

from __future__ import annotations

import os

import logging
import math
from collections import namedtuple
from dataclasses import make_dataclass
from typing import Any, Optional, Sequence

import torch
from torch import Tensor, nn

from . import _lib, ops
from .constants import CROSS_ENTROPY_IGNORE_IDX, PRECISION_STR_TO_DTYPE
from .llama_configs import ConfigLlama3_2
from .loss import check_loss_options, kl_range_mask
from .ops import GEMM_NN, GEMM_NT, GEMM_TN

LOGGER = logging.getLogger(__name__)

VOCAB_ALIGN = 256  # MFMA tile edge


def _align(n: int, a: int) -> int:
    return (n + a - 1) // a * a


# --------------------------------------------------------------------------------------------------------------------
# RoPE table (torchtune Llama3ScaledRoPE: rope_init / apply_scaling / build_rope_cache).
# Host-side fp32 tensor arithmetic, done once; the rotation itself is the HIP kernel ``ssi_rope_inplace``.
# --------------------------------------------------------------------------------------------------------------------
def llama3_rope_table(head_dim: int, max_seq_len: int, base: float = 500_000, scale_factor: float = 32,
                      low_freq_factor: float = 1, high_freq_factor: float = 4, old_context_len: int = 8192) -> Tensor:
    freqs = 1.0 / (base ** (torch.arange(0, head_dim, 2)[: head_dim // 2].float() / head_dim))
    lo_wl, hi_wl = old_context_len / low_freq_factor, old_context_len / high_freq_factor
    out = []
    for f in freqs:
        wavelen = 2 * math.pi / f
        if wavelen < hi_wl:
            out.append(f)
        elif wavelen > lo_wl:
            out.append(f / scale_factor)
        else:
            smooth = (old_context_len / wavelen - low_freq_factor) / (high_freq_factor - low_freq_factor)
            out.append((1 - smooth) * f / scale_factor + smooth * f)
    theta = torch.stack([t.to(torch.float32) for t in out])
    idx = torch.einsum("i, j -> ij", torch.arange(max_seq_len, dtype=theta.dtype), theta).float()
    return torch.stack([torch.cos(idx), torch.sin(idx)], dim=-1).contiguous()  # [max_seq_len, head_dim/2, 2]


class _Holder(nn.Module):
    """Parameter container so that ``state_dict`` / ``named_parameters`` carry torchtune's dotted names."""


class _Arena:
    """Persistent activation / workspace buffers keyed by name (stable device pointers across steps)."""

    def __init__(self, device: torch.device):
        self.device = device
        self.buf: dict[str, Tensor] = {}

    def get(self, name: str, shape: tuple, dtype: torch.dtype) -> Tensor:
        n = math.prod(shape)
        t = self.buf.get(name)
        if t is None or t.dtype != dtype or t.numel() < n:
            # a buffer that has to GROW (ragged batches: the packed length differs from batch to batch) takes a quarter more than asked, so
            # that a run reaches its largest batch in a few allocations instead of one per new length; fixed shapes never come here twice
            grow = t is not None and t.dtype == dtype
            if grow:
                self.buf[name] = t = None  # (freed BEFORE the larger one is requested: the cached block may serve a smaller sibling)
            t = torch.empty(max(n + n // 4 if grow else n, 1), dtype=dtype, device=self.device)
            self.buf[name] = t
        return t[:n].view(shape)

    def bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.buf.values())


class KVCache:
    """What ``HipLlamaDecoder.new_kv_cache`` returns: ``k`` and ``v`` ``[layers, n_slots, cap, n_kv * head_dim]`` in the model's dtype (K
    after RoPE), ``lengths`` (int32 ``[n_slots]`` on the device: tokens cached per slot) and ``errors`` (int32 ``[1]`` on the device: K / V
    rows or slots the kernels refused — out-of-range destinations, a slot at its cap; 0 in a correct run, read it with whatever is read
    back anyway).  An FP8 cache (``new_kv_cache(..., dtype="fp8")``; the header's "FP8 K/V cache") holds e4m3 codes in ``k`` and ``v`` (uint8, the
    same shape) and one exponent byte per (position, kv head) in ``k_exp`` and ``v_exp`` (uint8 ``[layers, n_slots, cap, n_kv]``).  ``dtype``: "fp8",
    or the torch dtype of a cache in the model's dtype."""

    def __init__(self, k: Tensor, v: Tensor, lengths: Tensor, errors: Tensor, k_exp: Optional[Tensor] = None, v_exp: Optional[Tensor] = None) -> None:
        self.k, self.v, self.lengths, self.errors, self.k_exp, self.v_exp = k, v, lengths, errors, k_exp, v_exp
        self.dtype = "fp8" if k_exp is not None else k.dtype

    def layer(self, l: int) -> tuple:
        """The cache tensors of layer ``l`` as the kernels take them: ``(k, v)``, or ``(k_codes, v_codes, k_exp, v_exp)`` of an fp8 cache."""
        return (self.k[l], self.v[l]) if self.k_exp is None else (self.k[l], self.v[l], self.k_exp[l], self.v_exp[l])

    @property
    def n_slots(self) -> int:
        return self.k.shape[1]

    @property
    def cap(self) -> int:
        return self.k.shape[2]


class QuantWeights:
    """What ``HipLlamaDecoder.quantize_weights`` returns: the projection matrices of every layer (``L{l}.wqkv``, ``.wo``, ``.w13``, ``.w2``) and,
    with ``head``, the tied embedding (``emb``) as e4m3 codes (uint8 ``[N, K]``) with one exponent byte per row (uint8 ``[N]``) — the header's "FP8
    weights".  ``mats``: name -> (codes, exps), plain tensors owned by the caller (not in the arena, not in the flat buffer; the model keeps no
    reference).  A snapshot: weights trained or loaded afterwards are not in it."""

    def __init__(self, mats: dict) -> None:
        self.mats = mats

    @property
    def head(self) -> bool:
        return "emb" in self.mats

    def nbytes(self) -> int:
        return sum(c.numel() + e.numel() for c, e in self.mats.values())


# One decoder layer's activation tensors, views of arena storage; ``HipLlamaDecoder._layer_bufs`` names and shapes them.  The final norm is the
# record of "layer" ``num_layers``: ``h_in`` its input, ``xn1`` its output, ``rstd1`` its rstd, the rest None.  ``lse`` is None in a decode step.
_LayerBufs = namedtuple("_LayerBufs", "h_in xn1 rstd1 qkv att lse hmid xn2 rstd2 gu act h_out", defaults=(None,) * 9)
# What a training forward leaves for its backward; ``h_last`` / ``rstdf``: input (without layers: the embedding's output) and rstd of the final norm.
_Saved = make_dataclass("_Saved", "tok B S gen pos ds de plan layers h_last rstdf".split())


class HipLlamaDecoder(nn.Module):
    def __init__(self, vocab_size: int, num_layers: int, num_heads: int, num_kv_heads: int, embed_dim: int,
                 max_seq_len: int, intermediate_dim: int, attn_dropout: float = 0.0, norm_eps: float = 1e-5,
                 rope_base: int = 500_000, scale_factor: int = 32, *, dtype: torch.dtype = torch.bfloat16,
                 device: torch.device | str = "cuda", rope_cache_len: Optional[int] = None) -> None:
        super().__init__()
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        if device.type != "cuda":
            raise _lib.HipLibraryError(
                f"HipLlamaDecoder runs only on an MI355X GPU through libssi_hip.so (got device={device}); "
                "there is no CPU fallback in the product path")
        _lib.load()
        if attn_dropout != 0.0:
            raise NotImplementedError("attn_dropout must be 0.0 (the reference config, llama_configs.py:136)")
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"unsupported dtype {dtype}")
        if embed_dim % num_heads or num_heads % num_kv_heads or embed_dim % 8 or intermediate_dim % 8:
            raise ValueError("embed_dim must divide into heads, heads into kv heads, and dims must be multiples of 8")
        self.vocab_size, self.num_layers = vocab_size, num_layers
        self.num_heads, self.num_kv_heads = num_heads, num_kv_heads
        self.embed_dim, self.intermediate_dim = embed_dim, intermediate_dim
        self.head_dim = embed_dim // num_heads
        self.max_seq_len, self.norm_eps = max_seq_len, float(norm_eps)
        self.dtype, self.device = dtype, device
        self.vocab_pad = _align(vocab_size, VOCAB_ALIGN)
        self.qkv_dim = (num_heads + 2 * num_kv_heads) * self.head_dim
        self.num_output_chunks = 0
        self.ignore_index = CROSS_ENTROPY_IGNORE_IDX

        D, I, Q, KVD = embed_dim, intermediate_dim, num_heads * self.head_dim, num_kv_heads * self.head_dim
        # ---- flat parameter layout ------------------------------------------------------------------------------
        off = 0
        self._slices: dict[str, tuple[int, tuple]] = {}

        def take(name: str, shape: tuple) -> None:
            nonlocal off
            self._slices[name] = (off, shape)
            off += _align(math.prod(shape), 8)

        # [E_pad | attention weights of every layer: L0.wqkv, L0.wo, L1.wqkv, ... | L0: w13, w2, sa_norm, mlp_norm | L1: ... | norm].
        # The attention projections sit together, one layer after the other at a fixed stride: their weight gradients (64 and 96 output
        # tiles, too few for 256 CUs) are computed for a GROUP of layers in one batched launch (_backward_hidden), which then finishes a
        # contiguous range of the gradient buffer = one data-parallel bucket per group.
        take("emb", (self.vocab_pad, D))
        for l in range(num_layers):
            take(f"L{l}.wqkv", (self.qkv_dim, D))
            take(f"L{l}.wo", (D, Q))
        for l in range(num_layers):
            take(f"L{l}.w13", (2 * I, D))
            take(f"L{l}.w2", (D, I))
            take(f"L{l}.sa_norm", (D,))
            take(f"L{l}.mlp_norm", (D,))
        take("norm", (D,))
        self._flat_numel = off
        self._flat = torch.zeros(off, dtype=dtype, device=device)
        self._flat_grad = torch.zeros(off, dtype=dtype, device=device)
        self._grad_views: dict[str, Tensor] = {}
        # Layers whose attention-projection weight gradients share one batched launch (0 / 1 = every layer on its own, split-K).  8 at the
        # 1B shape: 8 x 64 and 8 x 96 output tiles = 2 and 3 full rounds of the 256 CUs.
        self.wgrad_group = max(1, min(int(os.environ.get("SSI_WGRAD_GROUP", "8")), max(num_layers, 1)))
        # DP buckets in the order backward finishes them: final norm; per layer L-1..0 its MLP block (w13, w2, both norm scales), and
        # behind the lowest layer of every group the attention weights of that group; embedding (tied: finished last)
        self.buckets: list[tuple[str, int, int]] = []
        lo, _ = self._slices["norm"]
        self.buckets.append(("norm", lo, off))
        mlp_lo = lambda l: self._slices[f"L{l}.w13"][0] if l < num_layers else self._slices["norm"][0]  # noqa: E731
        attn_lo = lambda l: self._slices[f"L{l}.wqkv"][0] if l < num_layers else mlp_lo(0)  # noqa: E731
        for l in reversed(range(num_layers)):
            self.buckets.append((f"L{l}.mlp", mlp_lo(l), mlp_lo(l + 1)))
            if l % self.wgrad_group == 0:
                self.buckets.append((f"attn.{l}", attn_lo(l), attn_lo(min(l + self.wgrad_group, num_layers))))
        self.buckets.append(("emb", 0, attn_lo(0) if num_layers else self._slices["norm"][0]))
        self._bucket_by_name = {b[0]: b for b in self.buckets}
        self._bucket_group = self.wgrad_group

        # ---- torchtune-named parameters as views ------------------------------------------------------------------
        def view(name: str, rows: Optional[tuple[int, int]] = None, buf: Optional[Tensor] = None) -> Tensor:
            o, shape = self._slices[name]
            t = (self._flat if buf is None else buf)[o:o + math.prod(shape)].view(shape)
            return t if rows is None else t[rows[0]:rows[1]]

        self._view = view
        self._param_src: list[tuple[nn.Parameter, str, Optional[tuple[int, int]]]] = []

        def param(holder: nn.Module, attr: str, name: str, rows: Optional[tuple[int, int]] = None) -> None:
            p = nn.Parameter(view(name, rows))
            setattr(holder, attr, p)
            self._param_src.append((p, name, rows))

        self.tok_embeddings = _Holder()
        param(self.tok_embeddings, "weight", "emb", (0, vocab_size))
        self.layers = nn.ModuleList()
        for l in range(num_layers):
            layer = _Holder()
            layer.attn = _Holder()
            for nm, rows in (("q_proj", (0, Q)), ("k_proj", (Q, Q + KVD)), ("v_proj", (Q + KVD, Q + 2 * KVD))):
                h = _Holder()
                param(h, "weight", f"L{l}.wqkv", rows)
                setattr(layer.attn, nm, h)
            h = _Holder()
            param(h, "weight", f"L{l}.wo")
            layer.attn.output_proj = h
            layer.mlp = _Holder()
            for nm, src, rows in (("w1", "w13", (0, I)), ("w2", "w2", None), ("w3", "w13", (I, 2 * I))):
                h = _Holder()
                param(h, "weight", f"L{l}.{src}", rows)
                setattr(layer.mlp, nm, h)
            layer.sa_norm = _Holder()
            param(layer.sa_norm, "scale", f"L{l}.sa_norm")
            layer.mlp_norm = _Holder()
            param(layer.mlp_norm, "scale", f"L{l}.mlp_norm")
            self.layers.append(layer)
        self.norm = _Holder()
        param(self.norm, "scale", "norm")
        with torch.no_grad():
            for p, name, _ in self._param_src:
                if name.endswith("norm"):
                    p.fill_(1.0)

        cache_len = min(rope_cache_len or max_seq_len, max_seq_len)
        self._rope = llama3_rope_table(self.head_dim, cache_len, rope_base, scale_factor).to(device)
        self._arena = _Arena(device)
        self._anchor = torch.zeros(1, dtype=torch.float32, device=device, requires_grad=True)
        self._saved: Optional[_Saved] = None     # activations of the forward awaiting its backward
        self._fwd_generation = 0
        self.pending_grad_scale: Optional[Tensor] = None  # lazy scale_grads (device fp32 scalar), consumed by the optimizer
        # Gradient buffer protocol: nothing zeroes the 2.5 GB buffer between optimizer steps.  `_grads_dirty` = the buffer holds the
        # gradients of this accumulation window, the next backward ADDS; not dirty = the next backward WRITES every element (weight
        # gradients by the GEMM's plain epilogue, norm scales by assignment, the tied embedding by the head's weight gradient before the
        # scatter-add), so whatever is in the buffer (`_grads_stale`: left-overs of the last window) never has to be cleared.
        self._grads_dirty = False
        self._grads_stale = False
        self._emb_grad_written = False
        self.label_errors: Optional[Tensor] = None        # device count of out-of-range labels seen by the last fused loss
        self.last_ce_loss: Optional[Tensor] = None        # device scalars of the last fused loss with z_loss_coeff > 0: its cross-entropy part ...
        self.last_z_loss: Optional[Tensor] = None         # ... and its z part (coefficient applied, same normalisation)
        self.last_smooth_loss: Optional[Tensor] = None    # label_smoothing > 0: e x the uniform part (same normalisation); last_ce_loss is set too
        self.bucket_listener = None                       # callable(name, lo, hi) for the NEXT gradient-exchanging backward (see _backward_hidden)
        self.position_errors: Optional[Tensor] = None     # device count of input_pos entries outside the RoPE table in the last forward
        self.grad_sync = None                             # optional ssi.distributed.GradSync
        self.sync_this_backward = False

    # ---- nn.Module plumbing ------------------------------------------------------------------------------------------
    def _apply(self, fn, recurse=True):
        probe = fn(torch.empty(0, dtype=self.dtype, device=self.device))
        if probe.device != self.device or probe.dtype != self.dtype:
            raise NotImplementedError("HipLlamaDecoder is created on its target device/dtype; .to() cannot move it")
        return self

    def set_num_output_chunks(self, num_output_chunks: int) -> None:
        """Kept for API parity (``trainer.py:304``).  The fused loss path never materialises per-chunk logits lists;
        ``forward`` still returns ``num_output_chunks`` sequence chunks when asked for logits."""
        self.num_output_chunks = int(num_output_chunks)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        own = dict(self.named_parameters())
        missing = [k for k in own if k not in state_dict]
        unexpected = [k for k in state_dict if k not in own]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: missing keys {missing}, unexpected keys {unexpected}")
        with torch.no_grad():
            for k, p in own.items():
                if k in state_dict:
                    src = state_dict[k]
                    if tuple(src.shape) != tuple(p.shape):
                        raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(src.shape)} vs model {tuple(p.shape)}")
                    p.copy_(src.to(device=self.device, dtype=self.dtype))
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def attach_grads(self) -> None:
        """Point every ``p.grad`` at its slice of the flat gradient buffer (idempotent)."""
        for p, name, rows in self._param_src:
            if p.grad is None and p.requires_grad:   # (a frozen parameter has no gradient)
                p.grad = self._view(name, rows, self._flat_grad)

    # ---- frozen ranges (ssi/param_groups.py; set by HipAdamW) -------------------------------------------------------------
    def set_frozen(self, segments) -> None:
        """Tell the backward which element ranges of the flat buffer no optimizer will read (``segments``: consecutive ranges with a
        ``frozen`` flag, or None for none).  A weight-gradient launch is skipped when, and only when, every element it writes is frozen;
        a frozen range of the gradient buffer is unspecified from then on, and nothing may read it.  A parameter that is frozen as a whole
        gets ``requires_grad = False`` and ``grad = None``; a partly frozen one (the embedding with some trainable rows) keeps its ``grad``
        view, whose frozen rows mean nothing.  The norm scales' gradients ride in ``rmsnorm_bwd`` with ``dx`` and are written regardless."""
        frozen: list[tuple[int, int]] = []
        for s in segments or ():
            if s.frozen:
                if frozen and frozen[-1][1] == s.start:
                    frozen[-1] = (frozen[-1][0], s.end)
                else:
                    frozen.append((s.start, s.end))
        self._frozen_ranges = frozen
        for p, name, rows in self._param_src:
            o, shape = self._slices[name]
            cols = math.prod(shape[1:])
            lo, hi = (o, o + shape[0] * cols) if rows is None else (o + rows[0] * cols, o + rows[1] * cols)
            is_frozen = self._range_frozen(lo, hi)
            p.requires_grad_(not is_frozen)
            if is_frozen:
                p.grad = None
        # rows of the tied embedding whose gradient the head has to compute: a 256-aligned span around the trainable ones
        D, e_hi = self.embed_dim, self.vocab_pad * self.embed_dim
        self._emb_frozen = self._range_frozen(0, e_hi)
        self._emb_span: Optional[tuple[int, int]] = None
        if frozen and not self._emb_frozen:
            pos, first, last = 0, None, 0   # first and one-past-last trainable element of the embedding
            for lo, hi in frozen + [(e_hi, e_hi)]:
                if lo > pos and pos < e_hi:
                    first, last = (pos if first is None else first), min(lo, e_hi)
                pos = max(pos, hi)
            r0, r1 = first // D // 256 * 256, min(_align(-(-last // D), 256), self.vocab_pad)
            if (r0, r1) != (0, self.vocab_pad):
                self._emb_span = (r0, r1)

    _frozen_ranges: list = []
    _emb_frozen = False
    _emb_span = None

    def _range_frozen(self, lo: int, hi: int) -> bool:
        return any(a <= lo and hi <= b for a, b in self._frozen_ranges)

    def _slice_frozen(self, name: str, count: int = 1, stride: int = 0) -> bool:
        """Is every element of the slice ``name`` (and of the ``count - 1`` slices that follow it ``stride`` elements apart) frozen?"""
        if not self._frozen_ranges:
            return False
        o, shape = self._slices[name]
        n = math.prod(shape)
        return all(self._range_frozen(o + k * stride, o + k * stride + n) for k in range(count))

    def zero_grad(self, set_to_none: bool = True) -> None:
        """With ``set_to_none`` (torch's default) no memory is touched: the next backward overwrites the buffer.  Only a caller who
        keeps the ``p.grad`` views and wants to read zeros pays for a memset."""
        if set_to_none:
            self._grads_stale = self._grads_stale or self._grads_dirty
            for p, _, _ in self._param_src:
                p.grad = None
        elif self._grads_dirty or self._grads_stale:
            self._flat_grad.zero_()
            self._grads_stale = False
        self._grads_dirty = False
        self._emb_grad_written = False  # a head backward whose decoder backward never ran (exception in between) leaves it set
        self.pending_grad_scale = None

    def _window_accumulates(self) -> bool:
        """Does the backward about to run ADD to the gradient buffer (True) or WRITE it (False: first backward of a window)?

        ``_grads_dirty`` alone is not enough: an optimizer the model does not know (``torch.optim.AdamW`` on the parameter views,
        INTEGRATION.md level 2) ends a window with ``optimizer.zero_grad(set_to_none=True)``, which drops every ``p.grad`` without telling
        the model.  Every ``p.grad is None`` therefore opens a new window whatever the flag says — ``torch``'s own meaning of "no
        gradient yet".  Some ``None`` and some not (a caller cleared a subset): those parameters' slices are zeroed and the backward adds,
        which is what autograd's accumulation would give."""
        if not self._grads_dirty:
            return False
        live = [(p, name, rows) for p, name, rows in self._param_src if p.requires_grad]   # (a frozen parameter's grad is always None)
        dropped = [(p, name, rows) for p, name, rows in live if p.grad is None]
        if not dropped:
            return True
        if len(dropped) == len(live):
            self._grads_dirty, self._grads_stale, self._emb_grad_written = False, True, False
            self.pending_grad_scale = None
            return False
        for p, name, rows in dropped:  # re-attached at once: the decoder backward behind a head backward asks again
            p.grad = self._view(name, rows, self._flat_grad).zero_()
        return True

    def _finish_pending_exchange(self) -> None:
        """A data-parallel bucket left in flight (``GradSync.finish(defer_last=True)``) must have landed before a backward writes the
        gradient buffer again; ``HipAdamW.step`` normally does this, a caller that skipped the step must not race the reduction."""
        sync = self.grad_sync
        if sync is not None and hasattr(sync, "finish_deferred"):
            sync.finish_deferred()

    def activation_bytes(self) -> int:
        return self._arena.bytes()

    # ---- batch geometry ----------------------------------------------------------------------------------------------
    def _mfma_shapes(self) -> bool:
        D, I = self.embed_dim, self.intermediate_dim
        return (self.dtype == torch.bfloat16 and D % 256 == 0 and self.qkv_dim % 256 == 0 and (2 * I) % 256 == 0
                and I % 64 == 0 and (self.num_heads * self.head_dim) % 64 == 0)

    def padded_seq_len(self, batch: int, seq: int) -> int:
        """Sequence length after right-padding so that batch*seq fills whole 256-row MFMA tiles.  Right padding is the
        reference's own batch format (pad_id / -100, ``ssi/data/__init__.py:174-199``): causal attention and the ignored
        labels make it numerically inert for the real positions."""
        if not self._mfma_shapes():
            return seq
        g = 256 // math.gcd(batch, 256)
        g = max(g, 128)  # 128: the MFMA attention kernels walk 128-key groups (a ragged batch maximum would otherwise drop to the
        return _align(seq, g)  # generic attention kernels, 5x slower end to end)

    def _padded_rows(self, n: int) -> int:  # n rows that are not sequences (prefill's last tokens, a decode step) as whole MFMA tiles
        return _align(max(n, 1), VOCAB_ALIGN) if self._mfma_shapes() else n

    # the largest row count a ``small_batch`` decode step runs unpadded on the skinny GEMMs (at most ``_lib.GEMM_SKINNY_MAX_ROWS``); how the value
    # was chosen: README, "Small-batch decoding"
    skinny_max_rows = 64

    def takes_small_batch(self, rows: int, small_batch: bool) -> bool:
        """Does a decode step of ``rows`` rows with this flag run on the skinny GEMMs?  (The flag alone never does: fp32 models, shapes off the
        MFMA path, a head_dim other than 64 — the only one ``ssi_gemm_skinny_rope`` rotates — and more rows than the limit keep the tile
        path, launch for launch.)"""
        return bool(small_batch) and self._mfma_shapes() and self.head_dim == 64 and 1 <= rows <= min(self.skinny_max_rows, _lib.GEMM_SKINNY_MAX_ROWS)

    # split-KV decode attention (``decode_step(..., split_kv=True)``): the span in keys a workgroup walks (None: the library's default for the
    # model's head width and dtype, ``ssi_attn_decode_split_span``) and the largest LIVE row count that takes it; how the values were chosen:
    # README, "Split-KV decode attention"
    split_span: Optional[int] = None
    split_max_rows = 16

    def takes_split_kv(self, rows: int, split_kv: bool) -> bool:
        """Does a decode step of ``rows`` live rows with this flag run the split-KV attention?  (Every dtype and head geometry the decode
        attention serves; independent of ``small_batch``.)"""
        return bool(split_kv) and 1 <= rows <= self.split_max_rows

    def _split_kv(self, mode: str, rows: int, keys: int) -> dict:
        """The keywords of a split attention launch of ``rows`` rows over caches of up to ``keys`` keys per row: the span, and the workspace from
        the arena under a name of the step's buffer family."""
        span = int(self.split_span or ops.attn_decode_split_span(self.head_dim, self.dtype))
        n = ops.attn_decode_split_workspace(rows, self.num_heads, self.head_dim, keys, span)
        return {"span": span, "workspace": self._arena.get("ws.splitkv." + mode, (n,), torch.float32)}

    # ---- forward: decoder stack --------------------------------------------------------------------------------------
    @staticmethod
    def _document_ranges(input_pos: Tensor, max_pos: Optional[int] = None) -> tuple[Tensor, Tensor, Tensor]:
        """Torch restatement of ``ops.doc_ranges`` (kept as the checker of that kernel's test; the forward uses the kernel).
        Packed rows (torchtune ``PackedDataset``: ``input_pos`` restarts at 0 with every document of a row) -> int32 [B*S]
        (positions, doc_start, doc_end): a query attends to the keys doc_start <= key <= query of its own row, which is the
        block-causal mask ``padded_collate_packed`` builds from ``seq_lens``.  The padding tail of a pack continues the last
        document's positions and so joins it: no real query sees those keys (causal) and their labels are ignored."""
        B, S = input_pos.shape
        idx = torch.arange(S, device=input_pos.device, dtype=torch.int64).expand(B, S)
        is_start = input_pos == 0
        is_start[:, 0] = True
        doc_start = torch.where(is_start, idx, torch.zeros_like(idx)).cummax(dim=1).values
        nxt = torch.where(is_start, idx, torch.full_like(idx, S))
        nxt = torch.cat([nxt[:, 1:], torch.full_like(nxt[:, :1], S)], dim=1)  # first document start strictly after s
        doc_end = nxt.flip(1).cummin(dim=1).values.flip(1)
        as32 = lambda t: t.to(torch.int32).reshape(-1).contiguous()  # noqa: E731
        return as32(input_pos if max_pos is None else input_pos.clamp(max=max_pos)), as32(doc_start), as32(doc_end)

    # SSI_SPLITK_NT=0 (A/B runs): keep the k-contiguous / data-gradient GEMMs unsplit whatever their output grid
    split_small_grids = os.environ.get("SSI_SPLITK_NT", "1") != "0"

    # SSI_TAIL_SPLIT=0 (A/B runs): a ragged grid is K-split as a whole (the round-4 form) instead of in its last partial round only
    split_tail_only = os.environ.get("SSI_TAIL_SPLIT", "1") != "0"

    def _gemm(self, layout: int, a: Tensor, b: Tensor, c: Tensor, residual: Optional[Tensor] = None) -> None:
        """``ops.gemm`` for the forward projections and the data gradients, with K split where the 256 x 256 output grid leaves CUs idle:
        at the reference's default micro-batches (``conf/data/_sft_base.yaml:21``: 2 x 2048 = 4096 rows) W_o, W2 and the data gradients of
        the N = 2048 projections have 128 tiles for 256 CUs, and a ragged packed length fills its last round badly.  ``ops.splitk_choice``
        weighs the halved rounds against the fp32 partial tiles' traffic (K = 2048: a draw; K = 8192 / 16 384: 1.6-1.8 x).

        Round 5: a grid of MORE than one round (a right-padded batch after the unpadding: T' = 11 520 rows give the N = 2048 projections 360
        tiles = 1.4 rounds) is split in its last, partial round only: the m-tile rows that fill whole rounds run unsplit, the rows behind
        them as a second launch with its own K split — the same time on the matrix cores as the split of the whole grid (1.5 tile times
        either way at 1.4 rounds), but fp32 partial tiles and their reduction pass for 104 tiles instead of 360."""
        M, N = c.shape
        K = a.shape[1]
        mfma = self.split_small_grids and self.dtype == torch.bfloat16 and self._mfma_shapes() and M % 256 == 0 and N % 256 == 0
        if mfma and self.split_tail_only and layout in (GEMM_NT, GEMM_NN):
            tm, tn = M // 256, N // 256
            rounds = (tm * tn) // 256
            m_main = (rounds * 256) // tn  # m-tile rows that fill whole rounds of the 256 CUs
            if rounds >= 1 and 0 < m_main < tm and (tm - m_main) * tn <= 192:
                rows = m_main * 256
                ops.gemm(layout, a[:rows], b, c[:rows], residual=None if residual is None else residual[:rows])
                self._gemm(layout, a[rows:], b, c[rows:], None if residual is None else residual[rows:])  # (fewer than 256 tiles: split as a whole)
                return
        splits = ops.splitk_choice(M, N, K) if mfma else 1
        if splits > 1:
            wsk = self._arena.get("ws.splitk.nt", (splits * M * N,), torch.float32)
            ops.gemm_splitk(layout, a, b, c, splits, wsk, residual=residual)
        else:
            ops.gemm(layout, a, b, c, residual=residual)

    def build_attn_plan(self, input_pos: Tensor, force: bool = False):
        """Work plan of the attention backward for a packed batch (``ssi/attn_plan.py``) from a HOST ``input_pos`` [B, S] — what the data layer
        calls in its prefetch thread; ``None`` where the pipelined kernels do not apply (device tensor, fp32 model, other head ratios, a length
        the model would still have to pad, positions that are not document-relative, batches the library leaves to the round-1..3 kernels)."""
        from . import attn_plan
        if input_pos is None or input_pos.is_cuda or input_pos.dim() != 2 or not self._mfma_shapes() or self.head_dim != 64:
            return None
        B, S = input_pos.shape
        if self.num_heads != 4 * self.num_kv_heads or self.padded_seq_len(B, S) != S or S % 128:
            return None
        return attn_plan.plan_from_input_pos(input_pos, self.num_heads, self.num_kv_heads, force=force)

    def _forward_hidden(self, tokens: Tensor, save: bool, input_pos: Optional[Tensor] = None, attn_plan=None, kv_sink=None) -> Tensor:
        """``kv_sink`` (``prefill``): ``(KVCache, dest)`` with ``dest`` int64 ``[B * S]`` on the device — after every layer's QKV projection
        the k / v columns of row t are stored at ``dest[t]`` of that layer's cache (-1: not stored).  ``None``: not one launch more."""
        B, S = tokens.shape
        pos = ds = de = plan = self.position_errors = None
        if input_pos is not None and save:
            if attn_plan is None and not input_pos.is_cuda:  # host positions: the plan costs no device sync (the trainer's prefetch thread
                attn_plan = self.build_attn_plan(input_pos)   # brings one along with the batch instead)
            if attn_plan is not None and attn_plan.matches(B, S, self.num_heads, self.num_kv_heads) and self._mfma_shapes():
                plan = attn_plan.to_device(tokens.device)
        if input_pos is not None:
            if input_pos.shape != tokens.shape:
                raise ValueError("input_pos must have the shape of tokens")
            if not input_pos.is_cuda and int(input_pos.max()) >= self._rope.shape[0]:  # host tensor: checking costs no device sync
                raise ValueError("input_pos exceeds the RoPE cache")
            # device tensor: no blocking read-back in the step; positions are clamped to the cache instead (the data layer bounds
            # them by tokenizer.max_seq_len <= rope cache, ssi/data/packed.py), so the kernels never index past the table
            # and the clamped positions are COUNTED (position_errors): the trainer raises on them from its one read-back per micro-batch
            self.position_errors = torch.zeros(1, dtype=torch.int32, device=tokens.device)
            pos, ds, de = ops.doc_ranges(input_pos.to(tokens.device), self._rope.shape[0] - 1, self.position_errors)  # one launch
        H, KV, hd = self.num_heads, self.num_kv_heads, self.head_dim
        if pos is None and S > self._rope.shape[0]:  # implicit positions 0 .. S-1; with input_pos the table is indexed by (clamped) positions
            raise ValueError(f"sequence length {S} exceeds the RoPE cache ({self._rope.shape[0]})")
        tok = tokens.reshape(-1).contiguous()
        if save:  # the last saving forward's records hold views of arena storage, and a buffer that has to grow can be freed before the larger
            self._saved = None  # one is requested (_Arena.get) only if nothing refers to it: dropped BEFORE this forward asks the arena for anything

        def attend(l: int, b: _LayerBufs) -> None:
            if kv_sink is not None:
                self._kv_store(kv_sink[0], l, b.qkv, kv_sink[1])
            ops.attn_fwd(b.qkv, b.att, b.lse, B, S, H, KV, hd, ds, de)

        layers, final = self._run_stack("train" if save else "x", tok, B, S, S, pos, attend)  # (eval, no_grad: the ".x" buffers only)
        if save:
            self._fwd_generation += 1
            self._saved = _Saved(tok, B, S, self._fwd_generation, pos, ds, de, plan, layers, final.h_in, final.rstd1)
        return final.xn1

    def _layer_bufs(self, mode: str, l: int, rows: int, B: int, S: int, below: Sequence[_LayerBufs] = ()) -> _LayerBufs:
        """THE table of the stack's activation buffers, the only place that names and shapes them: layer ``l``'s record for ``rows = B * S``.
        ``"train"``: a set per layer, kept for the backward (``qkv.{l}`` ..., ``h0``, ``h{l+1}``; ``xn1`` / ``att`` of all layers in ONE buffer
        each: the batched weight gradients read a group of layers at a stride).  ``"x"`` (eval, teacher, prefill): one set (``qkv.x`` ...),
        ``hx0`` / ``hx1`` in turn.  ``"g"`` (``decode_step``): one set (``qkv.g`` ...), ONE norm output and rstd (``xn.g``, ``rstd.g``), no lse,
        ``h1.g`` / ``h2.g`` in turn.  ``"s"`` (a small-batch ``decode_step``: unpadded rows, skinny GEMMs): ``"g"``'s set under names of its own
        (``qkv.s`` ..., ``xn.s``, ``rstd.s``, ``h1.s`` / ``h2.s``; no ``gu``: nothing reads it in a decode step).  The modes share no buffer:
        a forward of one may run between a training forward and its backward.
        ``below``: the records of layers ``0 .. l - 1``.  In modes ``x`` and ``g`` nothing but ``h_out`` of layers 1 and 2 is looked up again."""
        if mode != "train" and 3 <= l < self.num_layers:
            return below[l - 2]   # (the two h buffers take turns: what layer l - 2 read and wrote)
        A, dt, f32, L, train = self._arena, self.dtype, torch.float32, self.num_layers, mode == "train"
        D, I, Q = self.embed_dim, self.intermediate_dim, self.num_heads * self.head_dim
        nm = (lambda s: f"{s}.{l}") if train else (lambda s: f"{s}.x") if mode == "x" else (lambda s: s.rstrip("12") + "." + mode)
        h_in = below[-1].h_out if below else A.get("h0" if train else nm("h0"), (rows, D), dt)
        if l == L:
            return _LayerBufs(h_in, A.get("hn" if train else "hn.x" if mode == "x" else "xn." + mode, (rows, D), dt),
                              A.get("rstdf" if train else "rstdf.x" if mode == "x" else "rstd." + mode, (rows,), f32))
        h_out = A.get(f"h{l + 1}" if train else f"hx{l & 1}" if mode == "x" else f"h{1 + (l & 1)}.{mode}", (rows, D), dt)
        if below and not train:
            return below[-1]._replace(h_in=h_in, h_out=h_out)
        xn1 = A.get("xn1.all", (L, rows, D), dt)[l] if train else A.get(nm("xn1"), (rows, D), dt)
        att = A.get("att.all", (L, rows, Q), dt)[l] if train else A.get(nm("att"), (rows, Q), dt)
        lse = None if mode in ("g", "s") else A.get(nm("lse"), (B * self.num_heads * S,), f32)
        return _LayerBufs(h_in, xn1, A.get(nm("rstd1"), (rows,), f32), A.get(nm("qkv"), (rows, self.qkv_dim), dt), att, lse,
                          A.get(nm("hmid"), (rows, D), dt), A.get(nm("xn2"), (rows, D), dt), A.get(nm("rstd2"), (rows,), f32),
                          None if mode == "s" else A.get(nm("gu"), (rows, 2 * I), dt), A.get(nm("act"), (rows, I), dt), h_out)

    def _run_stack(self, mode: str, tok: Tensor, B: int, S: int, seq_len: int, pos: Optional[Tensor], attend,
                   weight_quant: Optional["QuantWeights"] = None) -> tuple[list, _LayerBufs]:
        """Embedding, every layer, final norm on ``mode``'s buffers -> (the layers' records, the final norm's).  ``attend(l, record)``: the one step
        in which a forward and a decode step differ.  RoPE (rows of ``seq_len`` positions, or ``pos``) and SwiGLU ride in their GEMMs' epilogues.
        Mode ``"s"``: the four GEMMs are the skinny entries (1 to ``skinny_max_rows`` unpadded rows, ``pos`` required), everything else the same;
        with ``weight_quant`` (mode ``"s"`` only) their ``_w8`` forms on that object's codes and exponents in place of the bf16 weights."""
        weight = self._view
        if mode == "s" and weight_quant is not None:
            weight = lambda name: weight_quant.mats[name]  # noqa: E731
            qkv_gemm = lambda x, w, out: ops.gemm_skinny_rope_w8(x, *w, out, self.num_heads + self.num_kv_heads, self.head_dim, self._rope, pos)  # noqa: E731
            res_gemm = lambda x, w, out, res: ops.gemm_skinny_w8(x, *w, out, residual=res)  # noqa: E731
            mlp_gemm = lambda x, w, gu, act: ops.gemm_skinny_swiglu_w8(x, *w, None, act)  # noqa: E731
        elif mode == "s":
            qkv_gemm = lambda x, w, out: ops.gemm_skinny_rope(x, w, out, self.num_heads + self.num_kv_heads, self.head_dim, self._rope, pos)  # noqa: E731
            res_gemm = lambda x, w, out, res: ops.gemm_skinny(x, w, out, residual=res)  # noqa: E731
            mlp_gemm = lambda x, w, gu, act: ops.gemm_skinny_swiglu(x, w, None, act)  # noqa: E731
        else:
            qkv_gemm = lambda x, w, out: ops.gemm_rope(x, w, out, seq_len, self.num_heads + self.num_kv_heads, self.head_dim, self._rope, positions=pos)  # noqa: E731
            res_gemm = lambda x, w, out, res: self._gemm(GEMM_NT, x, w, out, residual=res)  # noqa: E731
            mlp_gemm = ops.gemm_swiglu_fwd
        layers, b = [], self._layer_bufs(mode, 0, B * S, B, S)
        ops.embed_fwd(tok, self._view("emb"), b.h_in, self.vocab_size)
        for l in range(self.num_layers):
            layers.append(b)
            ops.rmsnorm_fwd(b.h_in, self._view(f"L{l}.sa_norm"), b.xn1, b.rstd1, self.norm_eps)
            qkv_gemm(b.xn1, weight(f"L{l}.wqkv"), b.qkv)
            attend(l, b)
            res_gemm(b.att, weight(f"L{l}.wo"), b.hmid, b.h_in)
            ops.rmsnorm_fwd(b.hmid, self._view(f"L{l}.mlp_norm"), b.xn2, b.rstd2, self.norm_eps)
            mlp_gemm(b.xn2, weight(f"L{l}.w13"), b.gu, b.act)
            res_gemm(b.act, weight(f"L{l}.w2"), b.h_out, b.hmid)
            b = self._layer_bufs(mode, l + 1, B * S, B, S, layers)
        ops.rmsnorm_fwd(b.h_in, self.norm.scale, b.xn1, b.rstd1, self.norm_eps)
        return layers, b

    # ---- backward: decoder stack -------------------------------------------------------------------------------------
    def _saved_for(self, gen: int) -> _Saved:  # the one stale-forward check: the decoder backward's, and the fused loss's before its head
        if (sv := self._saved) is None or sv.gen != gen:
            raise RuntimeError("HipLlamaDecoder: backward called for a forward whose activations were overwritten; "
                               "run backward before the next training forward")
        return sv

    def _backward_hidden(self, d_hn: Tensor, gen: int) -> None:
        sv = self._saved_for(gen)
        B, S, tok, pos, ds, de, plan = sv.B, sv.S, sv.tok, sv.pos, sv.ds, sv.de, sv.plan
        T, D, I = B * S, self.embed_dim, self.intermediate_dim
        H, KV, hd, dt, A = self.num_heads, self.num_kv_heads, self.head_dim, self.dtype, self._arena
        L, G = self.num_layers, self._flat_grad
        self._finish_pending_exchange()   # first: _window_accumulates() may zero slices of the buffer a deferred bucket is still reduced into
        acc = self._window_accumulates()  # False: first backward of the window, every gradient is written, not added
        gv = lambda name: self._view(name, None, G)  # noqa: E731
        ws = A.get("ws.rms", (max(ops.rmsnorm_bwd_workspace_bytes(T, D), 16),), torch.uint8)

        def wgrad(dy: Tensor, x: Tensor, name: str) -> None:
            """dW += dy^T x; split over K = tokens when the [out, in] grid cannot fill the chip (square projections)."""
            if self._slice_frozen(name):
                return   # nobody reads this gradient (set_frozen)
            g = gv(name)
            splits = ops.splitk_choice(g.shape[0], g.shape[1], T) if (dt == torch.bfloat16 and T % 64 == 0) else 1
            if splits > 1:
                wsk = A.get("ws.splitk", (splits * g.shape[0] * g.shape[1],), torch.float32)
                ops.gemm_splitk(GEMM_TN, dy, x, g, splits, wsk, accumulate=acc)
            else:
                ops.gemm(GEMM_TN, dy, x, g, accumulate=acc)

        sync = self.grad_sync if (self.grad_sync is not None and self.sync_this_backward) else None
        # who hears that a bucket's gradients are final: the data-parallel exchange, and / or an optimizer that updates the bucket's parameters
        # under the rest of this backward (HipAdamW.overlap_with_backward, one shot: set for the window's last backward)
        listener, self.bucket_listener = (self.bucket_listener if self.sync_this_backward else None), None

        def announce(name: str) -> None:
            if sync:
                sync.bucket_ready(*self._bucket_by_name[name])
            if listener is not None:
                listener(*self._bucket_by_name[name])

        # Weight gradients of the attention projections (dW_o = d hmid^T att: 64 output tiles; dW_qkv = d qkv^T xn1: 96): deferred until the
        # lowest layer of a group has produced its d qkv, then ONE batched launch per weight covers the group at full K (8 layers: 512 and
        # 768 tiles = 2 and 3 rounds of the 256 CUs) instead of a split-K launch + reduction per layer and weight.  Costs G x T x (D + qkv)
        # elements of HBM for the group's output gradients (1.3 GB at the 1B shape, B x S = 16384) — memory this GPU has.
        Gp = self.wgrad_group
        if sync and Gp != self._bucket_group:
            raise RuntimeError("wgrad_group was changed after construction: the data-parallel buckets were laid out for the old grouping")
        defer = (Gp > 1 and dt == torch.bfloat16 and self._mfma_shapes() and T % 128 == 0 and T >= 256
                 and ops.splitk_choice(D, H * hd, T) > 1 and ops.splitk_choice(self.qkv_dim, D, T) > 1)
        if defer:
            dhmid_all, dqkv_all = A.get("dh.b.all", (Gp, T, D), dt), A.get("dqkv.all", (Gp, T, self.qkv_dim), dt)
            lstride = (self._slices["L1.wqkv"][0] - self._slices["L0.wqkv"][0]) if L > 1 else 0

        def flush_attention_wgrads(l_lo: int) -> None:
            n = min(Gp, L - l_lo)
            # att and xn1 of layers l_lo .. l_lo + n - 1: the saving forward keeps every layer's in ONE buffer, one after the other (_layer_bufs)
            att_n, xn1_n = (x.as_strided((n, *x.shape), (x.numel(), *x.stride())) for x in (sv.layers[l_lo].att, sv.layers[l_lo].xn1))
            g_o = torch.as_strided(G, (n, D, H * hd), (lstride, H * hd, 1), self._slices[f"L{l_lo}.wo"][0])
            g_qkv = torch.as_strided(G, (n, self.qkv_dim, D), (lstride, D, 1), self._slices[f"L{l_lo}.wqkv"][0])
            if not self._slice_frozen(f"L{l_lo}.wo", n, lstride):      # (skipped only when the whole group's weights are frozen)
                ops.gemm_batched(GEMM_TN, dhmid_all[:n], att_n, g_o, accumulate=acc)
            if not self._slice_frozen(f"L{l_lo}.wqkv", n, lstride):
                ops.gemm_batched(GEMM_TN, dqkv_all[:n], xn1_n, g_qkv, accumulate=acc)

        def dgrad(dy: Tensor, name: str, dx: Tensor) -> None:
            """dx = dy @ W  (W = [out, in]) on the untransposed weights: NN form of the persistent GEMM.  In the step its A operand has just
            been written and is served from the Infinity Cache, which makes it as fast as the k-contiguous form on a transposed copy."""
            self._gemm(GEMM_NN, dy, self._view(name), dx)

        # small micro-batches: dK / dV per query head + a reduction, in a workspace of the arena (0 bytes = the launch fills the chip as it is)
        ws_bytes = ops.attn_bwd_workspace_bytes(B, S, H, KV, hd, dt) if T > 0 else 0
        if plan is not None:  # (partial rows of the dK/dV chunks a plan splits over the query heads)
            ws_bytes = max(ws_bytes, plan.workspace_bytes)
        attn_ws = A.get("ws.attn", (ws_bytes,), torch.uint8) if ws_bytes else None
        dh = A.get("dh.a", (T, D), dt)
        ops.rmsnorm_bwd(d_hn, sv.h_last, self.norm.scale, sv.rstdf, None, dh, gv("norm"), ws, accumulate=acc)
        announce("norm")
        for l in reversed(range(L)):
            b = sv.layers[l]
            # MLP: h_out = hmid + act @ w2^T
            wgrad(dh, b.act, f"L{l}.w2")
            dgu = A.get("dgu", (T, 2 * I), dt)
            # d act = dh W2 never reaches memory: the SwiGLU backward rides in the GEMM epilogue
            ops.gemm_swiglu_bwd(GEMM_NN, dh, self._view(f"L{l}.w2"), b.gu, dgu, A.get("dact", (T, I), dt))
            dxn = A.get("dxn", (T, D), dt)
            dgrad(dgu, f"L{l}.w13", dxn)
            wgrad(dgu, b.xn2, f"L{l}.w13")
            dhmid = dhmid_all[l % Gp] if defer else A.get("dh.b", (T, D), dt)
            ops.rmsnorm_bwd(dxn, b.hmid, self._view(f"L{l}.mlp_norm"), b.rstd2, dh, dhmid, gv(f"L{l}.mlp_norm"), ws, accumulate=acc)
            # attention: hmid = h_in + att @ wo^T
            datt = A.get("datt", (T, H * hd), dt)
            dgrad(dhmid, f"L{l}.wo", datt)
            if not defer:
                wgrad(dhmid, b.att, f"L{l}.wo")
            dqkv = dqkv_all[l % Gp] if defer else A.get("dqkv", (T, self.qkv_dim), dt)
            delta = A.get("delta", (B * H * S,), torch.float32)
            # attention backward with the backward of the RoPE rotation fused into its epilogues: dqkv arrives in pre-RoPE space
            ops.attn_bwd(b.qkv, b.att, datt, b.lse, dqkv, delta, B, S, H, KV, hd, ds, de,
                         rope_table=self._rope, positions=pos, workspace=attn_ws, plan=plan)
            dgrad(dqkv, f"L{l}.wqkv", dxn)
            if not defer:
                wgrad(dqkv, b.xn1, f"L{l}.wqkv")
            ops.rmsnorm_bwd(dxn, b.h_in, self._view(f"L{l}.sa_norm"), b.rstd1, dhmid, dh, gv(f"L{l}.sa_norm"), ws, accumulate=acc)
            announce(f"L{l}.mlp")
            if defer and l % Gp == 0:
                flush_attention_wgrads(l)
            if l % self._bucket_group == 0:
                announce(f"attn.{l}")
        ws_e = A.get("ws.emb", (max(_lib.load().ssi_embed_bwd_workspace_bytes(self.vocab_size), 16),), torch.uint8)
        if not self._emb_frozen:
            if not acc and not self._emb_grad_written:  # backward through the hidden states only (no tied head in front): the scatter-add
                gv("emb").zero_()                       # below touches only the rows of this batch's tokens
            ops.embed_bwd(tok, dh, gv("emb"), self.vocab_size, ws_e)
        self._grads_dirty, self._grads_stale, self._emb_grad_written = True, False, False
        announce("emb")
        self._saved = None   # (with it go the records' references to arena storage: a buffer that grows next can be freed first, _Arena.get)
        self.attach_grads()

    # ---- FP8 weights for small-batch decoding (the header's "FP8 weights") -----------------------------------------------------
    def _quant_names(self, head: bool) -> list[str]:
        return [f"L{l}.{m}" for l in range(self.num_layers) for m in ("wqkv", "wo", "w13", "w2")] + (["emb"] if head else [])

    @torch.no_grad()
    def quantize_weights(self, head: bool = True) -> QuantWeights:
        """The present ``wqkv``, ``wo``, ``w13`` and ``w2`` of every layer and, with ``head``, the tied embedding as e4m3 codes with one
        power-of-two exponent per row (``ops.weight_quant_fp8``), for ``decode_step(..., small_batch=True, weight_quant=...)``.  bf16 models on
        the small-batch shapes only (``ValueError`` otherwise: no other step would read the codes).  The codes and exponents are tensors of
        their own, a byte per weight on top of the bf16 weights, which stay: the embedding gather, ``prefill`` and every larger step read them."""
        if not self.takes_small_batch(1, True):
            raise ValueError("quantize_weights: FP8 weights serve the small-batch decode step alone (a bf16 model on the MFMA shapes with head_dim 64)")
        mats = {}
        for name in self._quant_names(head):
            w = self._view(name)
            codes = torch.empty(w.shape, dtype=torch.uint8, device=self.device)
            exps = torch.empty((w.shape[0],), dtype=torch.uint8, device=self.device)
            ops.weight_quant_fp8(w, codes, exps)
            mats[name] = (codes, exps)
        return QuantWeights(mats)

    def _check_weight_quant(self, qw: Optional[QuantWeights]) -> Optional[QuantWeights]:
        """``qw`` if it is this model's (every layer's four matrices, the head or not, in this model's shapes on its device); ``ValueError`` otherwise."""
        if qw is None:
            return None
        if not isinstance(qw, QuantWeights) or set(qw.mats) != set(self._quant_names(qw.head)):
            raise ValueError("weight_quant is not what this model's quantize_weights returns")
        for name, (codes, exps) in qw.mats.items():
            shape = self._slices[name][1]
            if tuple(codes.shape) != tuple(shape) or tuple(exps.shape) != (shape[0],) or codes.device != self.device or exps.device != self.device:
                raise ValueError(f"weight_quant is not this model's: {name} is {tuple(codes.shape)} on {codes.device}, expected {tuple(shape)} on {self.device}")
        return qw

    # ---- generation: K/V cache, prefill, decode step (ssi/generate.py drives them) --------------------------------------------
    def new_kv_cache(self, n_slots: int, cap: int, dtype=None) -> "KVCache":
        """A K/V cache for ``n_slots`` sequences of up to ``cap`` tokens: plain tensors owned by the caller (not arena buffers; the model
        keeps no reference).  Nothing is allocated for generation before this is called.  ``dtype``: None or "auto" — the model's dtype; "fp8" —
        e4m3 codes with a power-of-two exponent per (position, kv head), a quarter (fp32) or half (bf16) of the bytes plus 1 / head_dim: what
        ``prefill`` and the decode steps store is quantised, and the decode steps attend over the quantised values (opt-in: it changes values)."""
        n_slots, cap = int(n_slots), int(cap)
        if n_slots < 1 or cap < 1:
            raise ValueError(f"new_kv_cache: n_slots and cap must be >= 1 (got {n_slots}, {cap})")
        if dtype not in (None, "auto", "fp8"):
            raise ValueError(f"new_kv_cache: dtype is None, 'auto' or 'fp8' (got {dtype!r})")
        shape = (self.num_layers, n_slots, cap, self.num_kv_heads * self.head_dim)
        lengths, errors = torch.zeros(n_slots, dtype=torch.int32, device=self.device), torch.zeros(1, dtype=torch.int32, device=self.device)
        if dtype == "fp8":
            codes, exps = (lambda: torch.zeros(shape, dtype=torch.uint8, device=self.device)), (
                lambda: torch.full(shape[:3] + (self.num_kv_heads,), 127, dtype=torch.uint8, device=self.device))
            return KVCache(codes(), codes(), lengths, errors, exps(), exps())
        return KVCache(torch.zeros(shape, dtype=self.dtype, device=self.device), torch.zeros(shape, dtype=self.dtype, device=self.device),
                       lengths, errors)

    def check_generation_lengths(self, prompt_lens, max_new_tokens: int, n_slots: int, cap: int) -> None:
        """The host refusals of generation, before any launch."""
        if len(prompt_lens) > n_slots:
            raise ValueError(f"{len(prompt_lens)} prompts for {n_slots} cache slots")
        max_new_tokens = int(max_new_tokens)
        if max_new_tokens < 0:
            raise ValueError(f"max_new_tokens = {max_new_tokens}")
        for i, n in enumerate(prompt_lens):
            if n < 1:
                raise ValueError(f"prompt {i} is empty")
            for what, limit in (("the cache's cap", cap), ("the RoPE table", self._rope.shape[0]), ("max_seq_len", self.max_seq_len)):
                if n + max_new_tokens > limit:
                    raise ValueError(f"prompt {i}: {n} tokens + {max_new_tokens} new ones exceed {what} ({limit})")

    PREFILL_ROW_LEN = 2048        # prompts are packed into rows of this many positions ...
    PREFILL_ROWS_PER_BATCH = 8    # ... and run this many rows at a time

    @torch.no_grad()
    def prefill(self, cache: "KVCache", prompts, max_new_tokens: int = 0, separate: bool = False, slots=None) -> Tensor:
        """Prompt ``i`` (a 1-D integer sequence) fills slot ``i`` of ``cache``: the prompts are packed into rows on the host
        (``ssi.score.prefill_batches``: first-fit decreasing, ``input_pos`` restarting with every prompt), the packed forward the dev
        loss and ``ssi.score`` use runs block-causal over them with every layer's K / V scattered into the cache, and the final norm's
        rows of the prompts' LAST tokens alone go through the tied head.  Returns ``[n_prompts, vocab_pad]`` logits (fresh tensor) and
        sets the cache's lengths; slots beyond the prompts are emptied.  ``max_new_tokens``: what ``decode_step`` will add, checked here
        against the cap, the RoPE table and ``max_seq_len`` (``ValueError`` before any launch).
        ``prefill`` always runs on the unquantised weights (FP8 weights, ``quantize_weights``, are read by small-batch decode steps alone), as it
        attends over the unquantised K / V under an fp8 cache.
        ``separate`` (the small-batch loops): every prompt runs as a packed forward of its own, one row that starts at position 0.  Where a
        prompt lies in a packed row, and how many rows the forward has (which picks the K split of its GEMMs), enter the bits of its K / V
        and of its logits; prompt by prompt they are a function of the prompt alone, whatever else is in the group.
        ``slots`` (continuous batching: a prompt enters a cache that holds live sequences): a list of distinct slot numbers, one per prompt;
        prompt ``i`` fills slot ``slots[i]``, every other slot's K / V, exponents and length are left exactly as they were, and the logits
        come in prompt order.  A slot number outside the cache or given twice is a ``ValueError`` before any launch.  ``None``: slots
        ``0 .. n - 1`` and the emptying of the rest, launch for launch as before."""
        from .score import prefill_batches
        seqs = [torch.as_tensor(p, dtype=torch.int64).reshape(-1) for p in prompts]
        lens = [int(s.numel()) for s in seqs]
        n, cap = len(seqs), cache.cap
        self._check_cache(cache)
        if slots is not None:
            slots = [int(v) for v in slots]
            if len(slots) != n:
                raise ValueError(f"prefill: {len(slots)} slots for {n} prompts")
            bad = [v for v in slots if not 0 <= v < cache.n_slots]
            if bad:
                raise ValueError(f"prefill: slots outside the cache's {cache.n_slots}: {bad[:8]}")
            if len(set(slots)) != n:
                raise ValueError(f"prefill: a slot is given twice: {sorted(v for v in set(slots) if slots.count(v) > 1)[:8]}")
        self.check_generation_lengths(lens, max_new_tokens, cache.n_slots, cap)
        if n == 0:
            raise ValueError("prefill: no prompts")
        # rows of PREFILL_ROW_LEN positions; one shorter row where all the prompts together need less, a longer one for a longer prompt
        row_len = min(max(min(self.PREFILL_ROW_LEN, sum(lens)), max(lens)), self._rope.shape[0])
        dev = self.device
        hlast = torch.zeros((self._padded_rows(n), self.embed_dim), dtype=self.dtype, device=dev)   # (pad rows: zeros)

        slot_of = None if slots is None else torch.tensor(slots, dtype=torch.int64)

        def batches():
            if not separate:
                for tokens, input_pos, dest, last_at, last_of in prefill_batches(seqs, cap, row_len, self.PREFILL_ROWS_PER_BATCH):
                    if slot_of is not None:   # slot i of the plan is slot slots[i] of the cache
                        dest = torch.where(dest >= 0, slot_of[dest.clamp(min=0) // cap] * cap + dest % cap, dest)
                    yield tokens, input_pos, dest, last_at, last_of
                return
            for i, s in enumerate(seqs):   # slot 0 of a one-prompt plan is slot i of the cache, or the slot chosen for prompt i
                at = i if slots is None else slots[i]
                for tokens, input_pos, dest, last_at, last_of in prefill_batches([s], cap, min(lens[i], self._rope.shape[0]), 1):
                    yield tokens, input_pos, torch.where(dest >= 0, dest + at * cap, dest), last_at, last_of + i

        for tokens, input_pos, dest, last_at, last_of in batches():
            row_len = tokens.shape[1]
            tokens, input_pos, dest = tokens.to(dev), input_pos.to(dev), dest.to(dev)
            tokens, input_pos, _, _ = self._right_pad(tokens, input_pos)
            B, S = tokens.shape
            if S > row_len:   # the padding is stored nowhere either, and a last token keeps its column in the longer rows
                dest = torch.cat([dest, torch.full((B, S - row_len), -1, dtype=torch.int64, device=dev)], dim=1)
                last_at = last_at + last_at // row_len * (S - row_len)
            hn = self._forward_hidden(tokens, save=False, input_pos=input_pos, kv_sink=(cache, dest.reshape(-1).contiguous()))
            hlast.index_copy_(0, last_of.to(dev), hn.index_select(0, last_at.to(dev)))
        if slots is None:
            cache.lengths.zero_()
            cache.lengths[:n] = torch.tensor(lens, dtype=torch.int32).to(dev)
        else:
            cache.lengths[slot_of.to(dev)] = torch.tensor(lens, dtype=torch.int32).to(dev)
        return self._head_logits(hlast)[:n]

    def _check_cache(self, cache: "KVCache", beside: Optional["KVCache"] = None) -> None:
        """Either kind of cache of this model's shape; ``beside``: the cache it is used with in one launch (prompt and beam cache), which must be
        of the same kind."""
        fp8 = cache.dtype == "fp8"
        want = (self.num_layers, cache.n_slots, cache.cap, self.num_kv_heads * self.head_dim)
        dtype = torch.uint8 if fp8 else self.dtype
        for t in (cache.k, cache.v):
            if tuple(t.shape) != want or t.dtype != dtype or t.device != self.device:
                raise ValueError(f"the K/V cache is not this model's: {tuple(t.shape)} {t.dtype} on {t.device}, expected {want} {dtype} on {self.device}")
        if fp8:
            for t in (cache.k_exp, cache.v_exp):
                if t is None or tuple(t.shape) != want[:3] + (self.num_kv_heads,) or t.dtype != torch.uint8 or t.device != self.device:
                    raise ValueError(f"the fp8 K/V cache's exponents are not this model's: expected uint8 {want[:3] + (self.num_kv_heads,)} on {self.device}")
        if beside is not None and (beside.dtype == "fp8") != fp8:
            raise ValueError(f"a prompt cache and a beam cache of different kinds ({beside.dtype} and {cache.dtype}): both fp8 or both the model's dtype")

    def _kv_store(self, cache: "KVCache", l: int, qkv: Tensor, dest: Tensor) -> None:
        """The K / V columns of ``qkv`` rows into layer ``l`` of ``cache`` at ``dest``, by the store of the cache's kind."""
        store = ops.kv_store_fp8 if cache.dtype == "fp8" else ops.kv_store
        store(qkv, dest, *cache.layer(l), self.num_heads, self.num_kv_heads, self.head_dim, n_bad=cache.errors)

    @torch.no_grad()
    def decode_step(self, cache: "KVCache", tokens: Tensor, slots: Tensor, small_batch: bool = False, split_kv: bool = False,
                    weight_quant: Optional["QuantWeights"] = None) -> Tensor:
        """One new token per live sequence: ``tokens`` (int64 ``[rows]``) and ``slots`` (int32 ``[rows]``; -1 = an inert row: no attention,
        no cache write, a zero attention row) on the device.  Row r runs at position ``cache.lengths[slots[r]]``: its K / V go there, it
        attends over the ``length + 1`` keys of its slot, and the length advances — all on the device, nothing is read back.  Returns the
        ``[rows, vocab_pad]`` logits (fresh tensor).  On the MFMA shapes the rows are padded to a multiple of 256 with inert rows, which
        makes every GEMM of the step one of the training step's tiles; all activations live in arena buffers of their own (``*.g``), so a
        step may run between a training forward and its backward.  A slot whose length has reached the cap is not written (its K / V
        would land in the next slot) and is counted in ``cache.errors``; ``prefill`` refuses what would get there.
        ``small_batch`` (with 1 to ``skinny_max_rows`` rows on the MFMA shapes with head_dim 64; otherwise without effect): the rows are NOT padded, the layer
        GEMMs and the head run on the weight-streaming skinny kernels and the activations live in the ``*.s`` buffers; norms, embedding,
        ``kv_store`` and ``attn_decode`` are the same launches on fewer rows.  A row's logits do not depend on the rows beside it.
        ``split_kv`` (with 1 to ``split_max_rows`` rows; otherwise without effect): ``attn_decode_split`` in place of ``attn_decode``, on the step's
        rows, padded or not, with a span of ``split_span`` keys and a workspace ``ws.splitkv.g`` / ``.s`` from the arena.  A row's logits still
        depend on that row alone, but differ in bits from the unsplit step's once its cache is longer than the span.
        ``weight_quant`` (what ``quantize_weights`` returned; where ``takes_small_batch`` holds, otherwise without effect): the four layer GEMMs and,
        if the object has it, the head read e4m3 codes through the ``_w8`` skinny entries; the logits are bit-equal to a small-batch step of a
        model that holds the dequantised weights.  The embedding gather, the norms, the K/V store and the attention are the same launches."""
        self._check_cache(cache)
        if tokens.dim() != 1 or tokens.dtype != torch.int64 or slots.shape != tokens.shape or slots.dtype != torch.int32:
            raise ValueError("decode_step: tokens is int64 [rows], slots int32 [rows]")
        if not tokens.is_cuda or not slots.is_cuda:
            raise _lib.HipLibraryError("decode_step: tokens and slots must live on the GPU (no CPU fallback)")
        n = tokens.numel()
        small = self.takes_small_batch(n, small_batch)
        wq = self._check_weight_quant(weight_quant) if small else None
        R = n if small else self._padded_rows(n)
        H, KV, hd, dev = self.num_heads, self.num_kv_heads, self.head_dim, self.device
        tok = torch.zeros(R, dtype=torch.int64, device=dev)          # pad rows: token 0, slot -1, position 0
        slot = torch.full((R,), -1, dtype=torch.int32, device=dev)
        tok[:n] = tokens
        slot[:n] = slots
        live = slot >= 0
        length = torch.where(live, cache.lengths[slot.clamp(min=0).long()], torch.zeros_like(slot))
        full = live & (length >= cache.cap)
        cache.errors += full.sum().to(torch.int32)
        write = live & ~full
        dest = torch.where(write, slot.long() * cache.cap + length.long(), torch.full_like(slot, -1, dtype=torch.int64))
        pos = length.clamp(max=self._rope.shape[0] - 1).contiguous()
        kv_len = torch.where(live, length + 1, torch.zeros_like(length)).contiguous()
        mode = "s" if small else "g"
        split = self._split_kv(mode, R, cache.cap) if self.takes_split_kv(n, split_kv) else None
        fp8 = cache.dtype == "fp8"

        def attend(l: int, b: _LayerBufs) -> None:
            self._kv_store(cache, l, b.qkv, dest)
            if split:
                (ops.attn_decode_split_fp8 if fp8 else ops.attn_decode_split)(b.qkv, *cache.layer(l), slot, kv_len, b.att, None, H, KV, hd,
                                                                               n_bad=cache.errors, **split)
            else:
                (ops.attn_decode_fp8 if fp8 else ops.attn_decode)(b.qkv, *cache.layer(l), slot, kv_len, b.att, None, H, KV, hd, n_bad=cache.errors)

        logits = self._head_logits(self._run_stack(mode, tok, R, 1, R, pos, attend, wq)[1].xn1, skinny=small, weight_quant=wq)   # R rows of one position each; RoPE by ``pos``
        cache.lengths.index_add_(0, slot.clamp(min=0).long(), write.to(torch.int32))
        return logits[:n]

    @torch.no_grad()
    def decode_step_beam(self, prompt_cache: "KVCache", beam_cache: "KVCache", tokens: Tensor, prompt_slot: Tensor, prompt_len: Tensor,
                         anc: Tensor, t: int, small_batch: bool = False, split_kv: bool = False,
                         weight_quant: Optional["QuantWeights"] = None) -> Tensor:
        """Step ``t`` of beam search: row ``r`` (one hypothesis) runs ``tokens[r]`` at position ``prompt_len[r] + t``.  Its K / V go to the beam
        cache at ``(r, t)``, and it attends over the ``prompt_len[r]`` keys of slot ``prompt_slot[r]`` of the prompt cache (what ``prefill``
        filled; read only here) and the generated positions ``i <= t`` of the beam cache at slots ``anc[r, i]`` — ``anc`` (int32
        ``[rows, >= t + 1]``, contiguous) is the hypothesis' ancestry and the caller has set ``anc[r, t] = r``.  ``prompt_slot[r] = -1``: an inert
        row.  Everything on the device; rows padded to whole tiles and activations in the ``*.g`` buffers, as ``decode_step``.  Neither cache's
        ``lengths`` are read or changed; refused indices are counted in ``beam_cache.errors``.  Returns ``[rows, vocab_pad]`` logits (fresh).
        ``small_batch``: as in ``decode_step`` (unpadded rows, skinny GEMMs, ``*.s`` buffers, where ``takes_small_batch`` holds).
        ``split_kv``: as in ``decode_step`` (``attn_decode_beam_split`` in place of ``attn_decode_beam``, where ``takes_split_kv`` holds).
        ``weight_quant``: as in ``decode_step`` (the ``_w8`` skinny GEMMs, where ``takes_small_batch`` holds)."""
        self._check_cache(prompt_cache)
        self._check_cache(beam_cache, beside=prompt_cache)
        n, t = tokens.numel(), int(t)
        if tokens.dim() != 1 or tokens.dtype != torch.int64 or any(x.shape != tokens.shape or x.dtype != torch.int32 for x in (prompt_slot, prompt_len)):
            raise ValueError("decode_step_beam: tokens is int64 [rows], prompt_slot and prompt_len int32 [rows]")
        if anc.dim() != 2 or anc.dtype != torch.int32 or anc.shape[0] != n or not anc.is_contiguous():
            raise ValueError("decode_step_beam: anc is a contiguous int32 [rows, width]")
        if not 0 <= t < min(beam_cache.cap, anc.shape[1]) or n > beam_cache.n_slots:
            raise ValueError(f"decode_step_beam: step {t} of {n} rows does not fit a beam cache of {beam_cache.n_slots} slots x {beam_cache.cap} "
                             f"and an ancestry of width {anc.shape[1]}")
        if not all(x.is_cuda for x in (tokens, prompt_slot, prompt_len, anc)):
            raise _lib.HipLibraryError("decode_step_beam: tokens, prompt_slot, prompt_len and anc must live on the GPU (no CPU fallback)")
        small = self.takes_small_batch(n, small_batch)
        wq = self._check_weight_quant(weight_quant) if small else None
        R = n if small else self._padded_rows(n)
        H, KV, hd, dev = self.num_heads, self.num_kv_heads, self.head_dim, self.device
        tok = torch.zeros(R, dtype=torch.int64, device=dev)           # pad rows: token 0, slot -1, position 0
        slot = torch.full((R,), -1, dtype=torch.int32, device=dev)
        plen = torch.zeros(R, dtype=torch.int32, device=dev)
        anc_r = torch.zeros((R, anc.shape[1]), dtype=torch.int32, device=dev)
        tok[:n], slot[:n], plen[:n], anc_r[:n] = tokens, prompt_slot, prompt_len, anc
        live = slot >= 0
        dest = torch.where(live, torch.arange(R, dtype=torch.int64, device=dev) * beam_cache.cap + t, torch.full((R,), -1, dtype=torch.int64, device=dev))
        pos = torch.where(live, plen + t, torch.zeros_like(plen)).clamp(max=self._rope.shape[0] - 1).contiguous()
        gen_len = torch.where(live, torch.full_like(plen, t + 1), torch.zeros_like(plen))
        mode = "s" if small else "g"
        split = self._split_kv(mode, R, prompt_cache.cap + min(beam_cache.cap, anc.shape[1])) if self.takes_split_kv(n, split_kv) else None

        def attend(l: int, b: _LayerBufs) -> None:
            self._kv_store(beam_cache, l, b.qkv, dest)
            if beam_cache.dtype == "fp8":
                (ops.attn_decode_beam_split_fp8 if split else ops.attn_decode_beam_fp8)(
                    b.qkv, prompt_cache.layer(l), beam_cache.layer(l), slot, plen, gen_len, anc_r, b.att, None, H, KV, hd, n_bad=beam_cache.errors,
                    **(split or {}))
            else:
                (ops.attn_decode_beam_split if split else ops.attn_decode_beam)(
                    b.qkv, *prompt_cache.layer(l), *beam_cache.layer(l), slot, plen, gen_len, anc_r, b.att, None, H, KV, hd,
                    n_bad=beam_cache.errors, **(split or {}))

        return self._head_logits(self._run_stack(mode, tok, R, 1, R, pos, attend, wq)[1].xn1, skinny=small, weight_quant=wq)[:n]

    # ---- tied LM head ------------------------------------------------------------------------------------------------
    def _head_logits(self, hn: Tensor, arena_name: Optional[str] = None, skinny: bool = False,
                     weight_quant: Optional["QuantWeights"] = None) -> Tensor:
        """logits [T, vocab_pad] = hn E^T.  Callers of the public ``forward`` get a FRESH tensor (as torchtune returns): logits kept
        from one batch must survive the next forward.  Only the fused loss passes an arena name (its buffer never leaves the model)."""
        T = hn.shape[0]
        if arena_name is None:
            logits = torch.empty((T, self.vocab_pad), dtype=self.dtype, device=self.device)
        else:
            logits = self._arena.get(arena_name, (T, self.vocab_pad), self.dtype)
        if skinny and weight_quant is not None and weight_quant.head:   # (a small-batch decode step on FP8 weights whose object holds the head)
            ops.gemm_skinny_w8(hn, *weight_quant.mats["emb"], logits)
        elif skinny:   # (a small-batch decode step: 1 to skinny_max_rows rows)
            ops.gemm_skinny(hn, self._view("emb"), logits)
        else:
            ops.gemm(GEMM_NT, hn, self._view("emb"), logits)
        return logits

    def _head_backward(self, dlogits: Tensor, hn: Tensor, alpha_dev: Optional[Tensor]) -> Tensor:
        """d_hn = alpha * dlogits @ E ;  dE += alpha * dlogits^T @ hn   (dlogits: [T, vocab_pad], pad columns zero)."""
        T, D = hn.shape
        self._finish_pending_exchange()  # before anything may touch the gradient buffer (see _backward_hidden)
        acc = self._window_accumulates()
        d_hn = self._arena.get("d_hn", (T, D), self.dtype)
        ops.gemm(GEMM_NN, dlogits, self._view("emb"), d_hn, alpha_dev=alpha_dev)
        g_emb = self._view("emb", None, self._flat_grad)
        # dE = dlogits^T hn has vocab_pad / 256 x D / 256 output tiles (521 x 8 = 4168 at V = 133 258): 16 full rounds of the 256 CUs and a
        # 17th with 72 tiles, each a full K = T contraction (~360 us with 184 CUs idle).  The rows of the last partial round go to a second
        # launch that also splits K, so that the tail occupies the chip for a third of a tile's time.
        rows_main = self._head_wgrad_main_rows(T)
        if self._emb_frozen:
            pass   # every row is frozen: no weight gradient at all (set_frozen)
        elif self._emb_span is not None:
            # only some rows are trainable: dE for a 256-aligned span around them, one plain launch on the strided operand the tail launch
            # below uses (about 20 row tiles instead of 521 with the new vocabulary rows alone); the rows outside stay unspecified
            r0, r1 = self._emb_span
            ops.gemm(GEMM_TN, dlogits[:, r0:r1], hn, g_emb[r0:r1], alpha_dev=alpha_dev, accumulate=acc)
        elif rows_main:
            Vp = self.vocab_pad
            ops.gemm(GEMM_TN, dlogits[:, :rows_main], hn, g_emb[:rows_main], alpha_dev=alpha_dev, accumulate=acc)
            tail, splits = Vp - rows_main, self._head_wgrad_tail_splits
            wsk = self._arena.get("ws.splitk.head", (splits * tail * D,), torch.float32)
            ops.gemm_splitk(GEMM_TN, dlogits[:, rows_main:], hn, g_emb[rows_main:], splits, wsk, alpha_dev=alpha_dev, accumulate=acc)
        else:
            ops.gemm(GEMM_TN, dlogits, hn, g_emb, alpha_dev=alpha_dev, accumulate=acc)
        self._emb_grad_written = True  # the decoder backward that follows adds the token rows on top and closes the window
        return d_hn

    _head_wgrad_tail_splits = 3

    def _head_wgrad_main_rows(self, T: int, n_cu: int = 256) -> int:
        """Rows of the embedding gradient computed by the unsplit launch (whole rounds of the CUs); 0 = one launch for everything (not the
        MFMA path, a last round at least half full, or a tail whose split units would not fit one round)."""
        if os.environ.get("SSI_HEAD_WGRAD_TAIL", "1") == "0" or self.dtype != torch.bfloat16 or not self._mfma_shapes() or T % 128 or T < 64 * 6 * self._head_wgrad_tail_splits:
            return 0
        tm, tn = self.vocab_pad // 256, self.embed_dim // 256
        full_rounds = (tm * tn) // n_cu
        if full_rounds == 0 or (full_rounds * n_cu) % tn:
            return 0
        tail_tiles = tm * tn - full_rounds * n_cu
        if tail_tiles == 0 or 2 * tail_tiles >= n_cu or tail_tiles * self._head_wgrad_tail_splits > n_cu:
            return 0
        return full_rounds * n_cu // tn * 256

    # ---- public API --------------------------------------------------------------------------------------------------
    def _check_inputs(self, tokens: Tensor, mask, encoder_input, encoder_mask, input_pos) -> Tensor:
        if encoder_input is not None or encoder_mask is not None:
            raise NotImplementedError("no encoder inputs: the reference's model is decoder-only (ssi/model.py:34)")
        if mask is not None and input_pos is None:
            raise NotImplementedError("a dense attention mask is never materialised: packed batches pass input_pos, from which "
                                      "the block-causal mask follows (ssi/data/packed.py)")
        # mask together with input_pos (torchtune's padded_collate_packed emits both): the block-causal structure is re-derived
        # from input_pos; the dense [B, S, S] tensor itself is not read
        if tokens.dim() != 2 or tokens.dtype != torch.int64:
            raise ValueError("tokens must be an int64 tensor of shape [batch, seq]")
        if not tokens.is_cuda:
            raise _lib.HipLibraryError("tokens must live on the GPU (no CPU fallback)")
        return tokens

    def _right_pad(self, tokens: Tensor, input_pos: Optional[Tensor], labels: Optional[Tensor] = None,
                   ignore_index: int = CROSS_ENTROPY_IGNORE_IDX, weights: Optional[Tensor] = None):
        """Right-pad a [B, S] batch to ``padded_seq_len`` (inert under causal attention): tokens with 0, labels with ``ignore_index``, loss
        weights with 1; positions continue the row's last document (as PackedDataset pads a pack), clamped to the RoPE table."""
        B, S = tokens.shape
        n = self.padded_seq_len(B, S) - S
        if n == 0:
            return tokens, input_pos, labels, weights
        dev = tokens.device
        pad_t = torch.zeros(B, n, dtype=tokens.dtype, device=dev)
        tokens = torch.cat([tokens, pad_t], dim=1)
        if labels is not None:
            labels = torch.cat([labels, torch.full_like(pad_t, ignore_index)], dim=1)
        if weights is not None:
            weights = torch.cat([weights, torch.ones(B, n, dtype=torch.float32, device=dev)], dim=1)
        if input_pos is not None:
            cont = input_pos[:, -1:].to(dev) + torch.arange(1, n + 1, device=dev)
            input_pos = torch.cat([input_pos.to(dev), cont.clamp_(max=self._rope.shape[0] - 1)], dim=1)
        return tokens, input_pos, labels, weights

    def forward_hidden(self, tokens: Tensor, input_pos: Optional[Tensor] = None, attn_plan=None) -> Tensor:
        """Final-normed hidden states [B, S, D] (autograd-aware)."""
        B, S = tokens.shape
        if torch.is_grad_enabled() and self.training:
            hn = _DecoderFn.apply(self, tokens, self._anchor, input_pos, attn_plan)
        else:
            hn = self._forward_hidden(tokens, save=False, input_pos=input_pos)
        return hn.view(B, S, self.embed_dim)

    def forward(self, tokens: Tensor, mask=None, encoder_input=None, encoder_mask=None, input_pos=None):
        """Logits.  ``num_output_chunks > 0``: list of [B, ceil(S/n), V] chunks in the model dtype (torch.chunk rule,
        SURVEY.md Appendix A.4); else one fp32 [B, S, V] tensor — as torchtune's ``TransformerDecoder.forward``."""
        tokens = self._check_inputs(tokens, mask, encoder_input, encoder_mask, input_pos)
        B, S0 = tokens.shape
        tokens, input_pos, _, _ = self._right_pad(tokens, input_pos)  # to whole MFMA tiles; the logits are sliced back below
        S = tokens.shape[1]
        hn = self.forward_hidden(tokens, input_pos).view(B * S, self.embed_dim)
        if torch.is_grad_enabled() and self.training:
            logits = _HeadLogitsFn.apply(self, hn, self._anchor)
        else:
            logits = self._head_logits(hn)
        logits = logits.view(B, S, self.vocab_pad)[:, :S0, : self.vocab_size]
        if self.num_output_chunks > 0:
            return list(logits.chunk(self.num_output_chunks, dim=1))
        return logits.float()

    def fused_loss(self, tokens: Tensor, shifted_labels: Tensor, ignore_index: int = CROSS_ENTROPY_IGNORE_IDX,
                   input_pos: Optional[Tensor] = None, attn_plan=None, loss_weights: Optional[Tensor] = None,
                   label_metrics=None, z_loss_coeff: float = 0.0, seq_scores=None, label_smoothing: float = 0.0,
                   teacher: Optional["HipLlamaDecoder"] = None, teacher_kl_coeff: float = 0.0, teacher_kl_ranges=None) -> Tensor:
        """Mean NLL over non-ignored (already shifted) labels with the LM head + CE fused: equals
        ``CEWithChunkedOutputLoss()(model(tokens, input_pos=...), shifted_labels)`` of the reference for any chunk count.
        ``input_pos`` ([B, S], restarting at 0 with every document): packed rows, block-causal attention.  ``attn_plan``
        (``build_attn_plan(input_pos)`` made on the host beside the batch): the attention backward then runs its pipelined kernels on the
        packed rows; without one (and with ``input_pos`` on the device) the round-1..3 kernels run — same results to rounding.
        ``loss_weights`` (fp32 ``[B, S]``, >= 0, aligned with ``shifted_labels``): the result is ``sum_i w_i nll_i / n_valid`` — how an
        accumulation window that runs as one batch keeps the reference's per-micro-batch normalisation (``ssi/data/window.py``).
        ``label_metrics`` (``ssi.eval.LabelMetrics``; forward-only calls): the cross-entropy launch also ranks every label in its row and the
        per-type sums of nll, top-1 and top-k hits are ADDED to ``label_metrics.acc`` on the device (``ssi_ce_fwd_metrics`` +
        ``ssi_ce_metrics_reduce``); the returned loss is bit-identical with and without it.  ``None``: exactly the launches of before.
        ``z_loss_coeff`` (not in the reference; finite, >= 0): the auxiliary z-loss ``z mean(log^2 Z)`` that keeps the softmax normaliser of
        the extended vocabulary near 1.  ``> 0``: the result is ``(sum_i w_i nll_i + z sum_i w_i lse_i^2) / n_valid`` (same weights and divisor
        for both terms), its gradient comes from the same cross-entropy launch (``ssi_ce_fwd_z``), and two device scalars are left on the
        model as ``label_errors`` is: ``last_ce_loss`` (the cross-entropy part, what a call without the coefficient returns) and
        ``last_z_loss`` (the z part, coefficient applied).  Under grad and without; not together with ``label_metrics`` (the dev set's
        metrics are plain cross-entropy).  ``0.0``: exactly the launches of before.
        ``seq_scores`` (``ssi.eval.SeqScores``; forward-only calls): the sums of nll, top-1 and top-k hits over each of its sequences
        ``(row, start, end)`` of THIS batch are written to ``seq_scores.out`` (``ssi_ce_fwd_metrics`` + ``ssi_seq_score_reduce``).  Its positions
        are those of ``tokens`` as passed; the flat offsets ``row * S_padded + pos`` are made here, after the right-padding.  Combines with
        ``label_metrics`` (one cross-entropy launch feeds both reduces), not with ``z_loss_coeff > 0``; the returned loss is bit-identical
        with and without it.  ``None``: exactly the launches of before.
        ``label_smoothing`` (not in the reference; finite, in ``[0, 1)``): ``e > 0`` trains against ``(1 - e) onehot + e / vocab``, the loss of
        ``F.cross_entropy(label_smoothing=e)``.  The result is ``((1 - e) sum_i w_i nll_i + e sum_i w_i u_i + z sum_i w_i lse_i^2) / n_valid``
        with ``u_i = lse_i - mean_c logits[i, c]``; its gradient comes from one cross-entropy launch (``ssi_ce_fwd_smooth``, with whatever
        ``z_loss_coeff`` is).  Left on the model: ``last_ce_loss`` (what a call without the option returns), ``last_smooth_loss``
        (``e`` x the mean of ``u``) and, with a z-loss, ``last_z_loss``.  Not together with ``label_metrics`` or ``seq_scores`` (plain
        cross-entropy both).  ``0.0``: exactly the launches of before.
        ``teacher`` with ``teacher_kl_coeff`` (not in the reference; finite, >= 0): ``b > 0`` adds the penalty ``b KL(teacher || student)`` on
        the next-token distribution against a frozen second ``HipLlamaDecoder`` of the same vocabulary, padding, device and dtype — what keeps
        a fully fine-tuned model near its starting point, or distils a better checkpoint.  The teacher runs forward-only on the same padded
        batch into ITS OWN arena (no gradient, nothing saved), a forward-only ``ssi_ce_fwd`` gives its lse per row, and ``ssi_ce_fwd_kl`` takes
        the place of the cross-entropy launch: the result is ``(sum_i w_i nll_i + b sum_i k_i KL_i) / n_valid`` and the buffer holds the whole
        objective's gradient.  ``teacher_kl_ranges`` (inclusive ``(lo, hi)`` label-id pairs, as ``get_token_type_ranges`` gives them): ``k_i = w_i``
        where the shifted label lies in one of them and 0 elsewhere, made on the device without a sync; ``None``: every labelled row.  Left on
        the model: ``last_ce_loss`` (what a call without the option returns) and ``last_kl_loss`` (coefficient applied, the same ``n_valid``).
        Under grad and without.  Not together with ``label_metrics``, ``seq_scores``, ``z_loss_coeff > 0`` or ``label_smoothing > 0``: folding
        the KL term into the z and smoothing forms of the kernel is left for later.  ``0.0``: exactly the launches of before; the teacher is
        not run."""
        label_smoothing, z_loss_coeff = check_loss_options("fused_loss", label_smoothing, z_loss_coeff, label_metrics, seq_scores,
                                                           under_grad=torch.is_grad_enabled() and self.training,
                                                           teacher_kl_coeff=teacher_kl_coeff)
        teacher_kl_coeff = float(teacher_kl_coeff)
        if teacher is not None or teacher_kl_coeff > 0.0:
            self._check_teacher(teacher)
        tokens = self._check_inputs(tokens, None, None, None, input_pos)
        if loss_weights is not None:
            if loss_weights.shape != tokens.shape:
                raise ValueError(f"loss_weights {tuple(loss_weights.shape)} vs tokens {tuple(tokens.shape)}")
            loss_weights = loss_weights.to(device=tokens.device, dtype=torch.float32)
        tokens, input_pos, shifted_labels, loss_weights = self._right_pad(tokens, input_pos, shifted_labels, ignore_index, loss_weights)
        labels = shifted_labels.reshape(-1).contiguous()
        weights = None if loss_weights is None else loss_weights.reshape(-1).contiguous()
        kl = None
        if teacher_kl_coeff > 0.0:  # (teacher logits, their lse per row, coefficient, k per row or None) — the teacher's pass comes first
            inside = kl_range_mask(labels, teacher_kl_ranges)
            kl_weights = None if inside is None else (inside.to(torch.float32) if weights is None else weights * inside)
            kl = (*teacher._teacher_rows(tokens, input_pos, labels, ignore_index), teacher_kl_coeff, kl_weights)
        if torch.is_grad_enabled() and self.training:
            return _FusedLossFn.apply(self, tokens, labels, ignore_index, self._anchor, input_pos, attn_plan, weights, z_loss_coeff, label_smoothing,
                                      kl)
        hn = self._forward_hidden(tokens, save=False, input_pos=input_pos)
        seq = None if seq_scores is None else (seq_scores, tokens.shape[1])
        return self._ce_forward(hn, labels, ignore_index, write_grad=False, weights=weights, label_metrics=label_metrics,
                                z_loss_coeff=z_loss_coeff, seq_scores=seq, label_smoothing=label_smoothing, kl=kl)[0]

    def _check_teacher(self, teacher) -> None:
        if not isinstance(teacher, HipLlamaDecoder) or teacher is self:
            raise ValueError("fused_loss: teacher must be another HipLlamaDecoder")
        for what in ("vocab_size", "vocab_pad", "device", "dtype"):
            if getattr(teacher, what) != getattr(self, what):
                raise ValueError(f"fused_loss: the teacher's {what} is {getattr(teacher, what)!r}, the model's {getattr(self, what)!r}")

    @torch.no_grad()
    def _teacher_rows(self, tokens: Tensor, input_pos: Optional[Tensor], labels: Tensor, ignore_index: int) -> tuple[Tensor, Tensor]:
        """This model as a frozen teacher on an already right-padded batch: (logits ``[T, vocab_pad]``, their lse per row), forward-only, in
        this model's own arena.  The lse is a launch of the existing forward-only cross-entropy kernel on the buffer: it reads the row once
        into registers, and ``ssi_ce_fwd_kl`` then needs no online rescaling and no second row in registers."""
        hn = self._forward_hidden(tokens, save=False, input_pos=input_pos)
        logits = self._head_logits(hn, "logits.t")
        T = hn.shape[0]
        row_lse = self._arena.get("row_lse.t", (T,), torch.float32)
        ops.ce_fwd(logits, labels, self.vocab_size, ignore_index, self._arena.get("row_loss.t", (T,), torch.float32), row_lse, False)
        return logits, row_lse

    def _ce_forward(self, hn: Tensor, labels: Tensor, ignore_index: int, write_grad: bool,
                    weights: Optional[Tensor] = None, label_metrics=None, z_loss_coeff: float = 0.0,
                    seq_scores=None, label_smoothing: float = 0.0, kl=None) -> tuple[Tensor, Tensor, Tensor]:
        """Tied head + cross-entropy: (mean loss, stats, logits buffer — which holds softmax - onehot when ``write_grad``).  The same
        three launches as the one-call ABI entry ``ssi_lmhead_ce_fwd`` (``ops.lmhead_ce_fwd``), issued one by one here so that ``bench.py``
        can time the head GEMM on its own.  ``z_loss_coeff > 0``: the z form of the cross-entropy launch (the buffer then holds
        ``f softmax - onehot``, ``f = 1 + 2 z lse``) and a second reduce over its ``row_z``; the loss returned is the sum of both parts.
        ``label_smoothing > 0``: the smoothing form (``ssi_ce_fwd_smooth``, which carries the z-loss too; the buffer then holds
        ``f softmax - (1 - e) onehot - e / vocab``) and one more reduce over its ``row_u``.
        ``kl``: ``(teacher logits, teacher lse, coefficient b, k per row or None)``: the KL form (``ssi_ce_fwd_kl``; the buffer then holds
        ``(w + b k) softmax - w onehot - b k q``) and one more reduce over its ``row_kl``.
        ``seq_scores``: ``(ssi.eval.SeqScores, padded row length)``."""
        T, e, z = hn.shape[0], label_smoothing, z_loss_coeff
        sfx = "" if write_grad else ".x"
        logits = self._head_logits(hn, "logits" + sfx)
        row_loss = self._arena.get("row_loss" + sfx, (T,), torch.float32)
        row_u = self._arena.get("row_u" + sfx, (T,), torch.float32) if e > 0.0 else None
        row_z = self._arena.get("row_z" + sfx, (T,), torch.float32) if z > 0.0 else None
        row_kl = self._arena.get("row_kl" + sfx, (T,), torch.float32) if kl is not None else None
        common = (logits, labels, self.vocab_size, ignore_index)
        if e > 0.0 or z > 0.0 or kl is not None:
            assert label_metrics is None and seq_scores is None
        if kl is not None:
            assert e == 0.0 and z == 0.0
            t_logits, t_lse, b, kl_weights = kl
            ops.ce_fwd_kl(logits, t_logits, t_lse, labels, self.vocab_size, ignore_index, b, row_loss, None, row_kl, write_grad,
                          row_weight=weights, row_kl_weight=kl_weights)
        elif e > 0.0:
            ops.ce_fwd_smooth(*common, e, z, row_loss, None, row_u, row_z, write_grad, row_weight=weights)
        elif z > 0.0:
            ops.ce_fwd_z(*common, z, row_loss, None, row_z, write_grad, row_weight=weights)
        elif label_metrics is None and seq_scores is None:
            ops.ce_fwd(*common, row_loss, None, write_grad, row_weight=weights)
        else:  # forward-only (fused_loss refuses it under grad): the same row losses, plus nll and rank of every label, summed per type / sequence
            assert not write_grad
            row_nll = self._arena.get("row_nll.x", (T,), torch.float32)
            row_rank = self._arena.get("row_rank.x", (T,), torch.int32)
            ops.ce_fwd_metrics(*common, row_loss, None, row_nll, row_rank, row_weight=weights)
            if label_metrics is not None:
                ops.ce_metrics_reduce(row_nll, row_rank, labels, label_metrics.ranges_dev, label_metrics.topk, label_metrics.acc, accumulate=True)
            if seq_scores is not None:
                scores, row_len = seq_scores
                start, end = scores.flat_spans(row_len, self.device)
                ops.seq_score_reduce(row_nll, row_rank, T, start, end, scores.topk, scores.out)
                if scores.keep_rows:
                    scores.row_nll, scores.row_len = row_nll.clone(), row_len
        # one reduce per part of the objective, over the same labels: the same n_valid divides every part.  (row buffer, coefficient, attribute)
        parts = [(row_loss, None, "last_ce_loss")] + [(buf, c, name) for buf, c, name in ((row_u, e, "last_smooth_loss"), (row_z, z, "last_z_loss"),
                                                                            (row_kl, kl[2] if kl is not None else 0.0, "last_kl_loss"))
                                                       if buf is not None]
        out = torch.empty(4 * len(parts), dtype=torch.float32, device=self.device)
        for i, (buf, coeff, name) in enumerate(parts):
            ops.ce_reduce(buf, labels, self.vocab_size, ignore_index, out[4 * i:4 * i + 4])
            if len(parts) > 1:  # (a plain call leaves the attributes of the last call with an option as they are)
                setattr(self, name, out[4 * i] if coeff is None else out[4 * i] * coeff)
        self.label_errors = out[3]  # device scalar: labels outside [0, vocab); the trainer folds it into its one read-back and raises
        loss = out[0]
        if e > 0.0:
            loss = out[0] * (1.0 - e) + self.last_smooth_loss
        if z > 0.0:
            loss = loss + self.last_z_loss
        if kl is not None:
            loss = loss + self.last_kl_loss
        return loss, out[:4], logits


class _DecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model: HipLlamaDecoder, tokens: Tensor, anchor: Tensor, input_pos: Optional[Tensor] = None, attn_plan=None) -> Tensor:
        hn = model._forward_hidden(tokens, save=True, input_pos=input_pos, attn_plan=attn_plan)
        ctx.model, ctx.gen = model, model._fwd_generation
        return hn

    @staticmethod
    def backward(ctx, d_hn: Tensor):
        ctx.model._backward_hidden(d_hn.contiguous(), ctx.gen)
        return None, None, torch.zeros_like(ctx.model._anchor), None, None


class _HeadLogitsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model: HipLlamaDecoder, hn: Tensor, anchor: Tensor) -> Tensor:
        ctx.model = model
        ctx.save_for_backward(hn)
        return model._head_logits(hn)

    @staticmethod
    def backward(ctx, dlogits: Tensor):
        (hn,) = ctx.saved_tensors
        m = ctx.model
        dl = dlogits
        if not dl.is_contiguous() or dl.dtype != m.dtype:
            dl = dl.to(m.dtype).contiguous()
        return None, m._head_backward(dl, hn, None), torch.zeros_like(m._anchor)


class _FusedLossFn(torch.autograd.Function):
    """tokens, shifted labels -> scalar loss; backward runs head + decoder backward and accumulates into the flat
    gradient buffer (so ``p.grad`` is populated exactly as after ``loss.backward()`` in the reference)."""

    @staticmethod
    def forward(ctx, model: HipLlamaDecoder, tokens: Tensor, labels: Tensor, ignore_index: int, anchor: Tensor,
                input_pos: Optional[Tensor] = None, attn_plan=None, weights: Optional[Tensor] = None, z_loss_coeff: float = 0.0,
                label_smoothing: float = 0.0, kl=None) -> Tensor:
        hn = model._forward_hidden(tokens, save=True, input_pos=input_pos, attn_plan=attn_plan)
        loss, stats, dlogits = model._ce_forward(hn, labels, ignore_index, write_grad=True, weights=weights, z_loss_coeff=z_loss_coeff,
                                                 label_smoothing=label_smoothing, kl=kl)
        ctx.model, ctx.gen = model, model._fwd_generation
        ctx.save_for_backward(hn, stats, dlogits)
        return loss.clone()

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        hn, stats, dlogits = ctx.saved_tensors
        m = ctx.model
        m._saved_for(ctx.gen)  # a stale forward raises BEFORE the head backward touches the gradient buffer
        # d loss / d logits = (softmax - onehot) / n_valid ; the 1/n_valid and the upstream scalar ride in alpha_dev (with a z-loss the buffer
        # holds (f softmax - onehot), with label smoothing (f softmax - (1 - e) onehot - e / vocab): every part of the objective shares the divisor)
        alpha = (grad_out.to(torch.float32).reshape(1) / stats[2:3]).contiguous()
        d_hn = m._head_backward(dlogits, hn, alpha)
        m._backward_hidden(d_hn, ctx.gen)
        return None, None, None, None, torch.zeros_like(m._anchor), None, None, None, None, None, None


# --------------------------------------------------------------------------------------------------------------------
# Reference-named entry point
# --------------------------------------------------------------------------------------------------------------------
def get_dtype(dtype: Any) -> torch.dtype:
    if isinstance(dtype, torch.dtype):
        return dtype
    if dtype is None:
        return torch.float32
    if dtype not in PRECISION_STR_TO_DTYPE:
        raise ValueError(f"Dtype {dtype} must be one of {', '.join(PRECISION_STR_TO_DTYPE)}")
    return PRECISION_STR_TO_DTYPE[dtype]


def get_device(device: Any = None) -> torch.device:
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
        torch.cuda.set_device(dev)
    return dev


def validate_expected_param_dtype(named_params, dtype: torch.dtype) -> None:
    for name, param in named_params:
        if param.dtype != dtype:
            raise ValueError(f"Parameter {name} has dtype {param.dtype}, but expected {dtype}")


def setup_llama3_2_1b(cfg, llama_config: ConfigLlama3_2, model_state_dict: Optional[dict[str, Any]],
                      dtype_default: torch.dtype | str | None = None,
                      device_default: torch.device | str | None = None) -> HipLlamaDecoder:
    """Same signature and contract as ``/root/reference/ssi/model.py:18-39``: build the decoder from
    ``llama_config.parameters`` in ``dtype_default`` on ``device_default``, load the (torchtune-key) state dict strictly,
    check every parameter's dtype.  ``cfg.compile`` is accepted and ignored: there is no tracing compiler in this stack."""
    if dtype_default is None:
        dtype_default = torch.get_default_dtype()
    elif isinstance(dtype_default, str):
        dtype_default = get_dtype(cfg.dtype)
    if device_default is None:
        device_default = get_device(None)
    elif isinstance(device_default, str):
        device_default = get_device(cfg.device)
    if cfg is not None and cfg.get("compile", False):
        LOGGER.info("cfg.compile=true ignored: kernels are hand-written HIP, there is nothing to trace-compile")
    model = HipLlamaDecoder(**llama_config.parameters, dtype=dtype_default, device=device_default)
    if model_state_dict is not None:
        model.load_state_dict(model_state_dict)
    validate_expected_param_dtype(model.named_parameters(), dtype=dtype_default)
    return model
