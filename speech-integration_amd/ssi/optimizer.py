"""Optimizer of the training step (reference: ``/root/reference/ssi/optimizer.py:8-17``, ``conf/training.yaml:2-10``).

``setup_optimizer(cfg, model, optimizer_state_dict)`` keeps the reference signature.  :class:`HipAdamW` is a
``torch.optim.Optimizer`` (so ``LambdaLR``, ``param_groups``, ``state_dict`` work unchanged) whose ``step`` is ONE HIP
kernel over the model's flat parameter / gradient / moment buffers: decoupled weight decay, fp32 op-math, a single
rounding on store — the semantics of ``torch.optim.AdamW(fused=True)`` (K13), with ``scale_grads`` (K11) and the
clip coefficient (K12) folded in as a device-side gradient multiplier.  The gradient buffer is not zeroed: the first backward of the
next accumulation window overwrites it (``HipLlamaDecoder`` gradient-buffer protocol).  ``stochastic_rounding`` (bf16 only, off by default,
not in the reference) rounds the three stores stochastically instead of to nearest, with stateless counter-based random bits.
``param_segments`` (config key ``param_groups``, null by default, not in the reference; ``ssi/param_groups.py``) gives consecutive ranges of
the flat buffer their own lr scale, weight decay or a frozen flag: the step is still one launch, of the segmented kernel.
``ema_decay`` (config key of the same name, null by default, not in the reference) keeps an fp32 exponential moving average of the flat
parameter buffer, one more HIP pass chained to every AdamW launch; ``ema_weights()`` evaluates on it, ``ema_state_dict()`` saves it.
``grad_groups`` (config key of the same name, null by default, not in the reference; ``ssi/grad_groups.py``) names groups of the flat gradient
buffer: ``measure_grad_group_sums()`` gives every group's gradient norm in one HIP pass, and with a clip rule each group's coefficient rides
into the segmented AdamW as a per-segment device scale."""

from __future__ import annotations

import contextlib
import math
import struct
import weakref
from typing import Any, Iterable

import torch
from torch import Tensor

from . import ops
from .param_groups import check_segments, model_layout, resolve, trainable_ranges
from .param_groups import clip as clip_segments


def ema_decay_at(step: int, ema_decay: float, warmup: bool = True) -> float:
    """The decay of the parameter average at the 1-based optimizer ``step``: ``ema_decay``, or with ``warmup`` ``min(ema_decay, (1 + step) /
    (10 + step))`` — the first steps do not pin the average to the initial weights (step 1 keeps 2/11 of them, step 10 11/20).  Computed in
    double and rounded to fp32 once, the value the kernel takes.  A function of the step alone: a resume needs no extra state."""
    d = float(ema_decay)
    if warmup:
        d = min(d, (1.0 + int(step)) / (10.0 + int(step)))
    return struct.unpack("f", struct.pack("f", d))[0]


class HipAdamW(torch.optim.Optimizer):
    def __init__(self, params: Iterable, lr: float = 1e-3, betas: tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, amsgrad: bool = False, fused: bool | None = None, *, model=None,
                 stochastic_rounding: bool = False, stochastic_rounding_seed: int | None = None, param_segments=None,
                 ema_decay: float | None = None, ema_warmup: bool = True, grad_groups=None, **unused: Any):
        if amsgrad:
            raise NotImplementedError("amsgrad=True is not supported (reference default: false, conf/training.yaml:8)")
        if unused:
            raise TypeError(f"unsupported AdamW arguments: {sorted(unused)}")
        if model is None or not hasattr(model, "_flat"):
            raise TypeError("HipAdamW needs model=<HipLlamaDecoder> (flat parameter buffers)")
        defaults = dict(lr=float(lr), betas=tuple(float(b) for b in betas), eps=float(eps), weight_decay=float(weight_decay),
                        amsgrad=False, fused=True)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise NotImplementedError("one param group expected (the reference passes model.parameters())")
        # Stochastic rounding of the bf16 stores (not in the reference; off by default).  Round-to-nearest drops every update below half a
        # bf16 step: exp_avg_sq * 0.999 rounds back for every bf16 value, and a weight at 1.0 never moves at lr 2e-4.  The random bits are a
        # pure function of (seed, step, element index in the flat buffer, tensor): slices, ranks and resumes all see the same ones.  Flag
        # and seed belong to the run's configuration, not to the optimizer state: they are kept out of ``param_groups``, which
        # ``load_state_dict`` replaces wholesale, so a state saved either way loads into a run configured either way.
        if stochastic_rounding and model._flat.dtype != torch.bfloat16:
            raise ValueError(f"stochastic_rounding=true needs dtype=bf16: it rounds AdamW's bf16 stores, and the model's parameters are {model._flat.dtype}")
        if stochastic_rounding:
            from .constants import SEED
            self._sr_seed = int(SEED if stochastic_rounding_seed is None else stochastic_rounding_seed)   # the same on every rank
        else:
            self._sr_seed = None
        # Parameter segments (not in the reference; ssi/param_groups.py): consecutive ranges of the flat buffer with their own lr scale, weight
        # decay and frozen flag, applied by ssi_adamw_step_seg in the launches below.  Like the rounding they belong to the run's configuration:
        # ``param_groups`` stays the one torch group, and a state saved under one rule set loads under another (a frozen range's moments
        # simply stay what they were).  The model learns what is frozen, and skips those weight-gradient launches.
        self._segments = None if param_segments is None else check_segments(param_segments, model._flat.numel())
        if self._segments is not None or getattr(model, "_frozen_ranges", None):   # (without segments: only to undo an earlier optimizer's)
            model.set_frozen(self._segments)
        self.model = model
        model._hip_optimizer = weakref.ref(self)  # scale_grads / clip_grad_norm_ may defer their factor only while THIS optimizer consumes it
        self._exp_avg = torch.zeros_like(model._flat)
        self._exp_avg_sq = torch.zeros_like(model._flat)
        self._step_count = 0
        self._views_ready = False
        self._side = None    # stream of the updates that run under the backward (overlap_with_backward)
        self._armed = None
        # Exponential moving average of the parameters (not in the reference; off by default): fp32, the size of the flat buffer (+4 bytes per
        # parameter: 5.0 GB at the 1B shape), started from the parameters as they are now and moved by one ssi_ema_update launch behind every
        # AdamW launch of ``_update`` — so it follows the plain step, the segmented one, the deferred bucket under data parallelism and the
        # buckets updated under the backward alike.  A bf16 run's iterates carry bf16 rounding noise; their fp32 average removes most of it.
        # Like the rounding and the segments, flag and decay belong to the run's configuration, not to ``state_dict()``.
        self._ema, self._ema_stash = None, None
        self._ema_decay, self._ema_warmup = None, bool(ema_warmup)
        if ema_decay is not None:
            d = ema_decay
            if isinstance(d, bool) or not isinstance(d, (int, float)) or not math.isfinite(d) or not 0 <= ema_decay_at(1, d, False) < 1:
                raise ValueError(f"ema_decay must be null or a finite number in [0, 1) (as fp32), got {d!r}")
            self._ema_decay = float(d)
            self._ema = model._flat.to(torch.float32, copy=True)
        self._ema_ranges = None if self._segments is None else trainable_ranges(self._segments)
        # Gradient groups (not in the reference; off by default; ssi/grad_groups.py): a table of segments of the flat gradient buffer with their
        # group, summed per group by ONE ssi_sumsq_groups launch in ``measure_grad_group_sums``; with a clip rule the groups' coefficients become the
        # per-segment device scales of the segmented AdamW over the refined segments.  They belong to the run's configuration like the segments.
        self._groups = grad_groups
        self._group_sums = self._group_ws = self._group_coef = self._group_seg_index = None
        self.group_values = None   # what the last measured window leaves for the log: {"norm": ..., ["clip", "skipped", ["ema"]]} device tensors
        if grad_groups is not None:
            if [s for s, _ in grad_groups.refined] != self._refined_base(grad_groups):
                raise ValueError("grad_groups was resolved against other parameter segments than this optimizer's")
            dev = model._flat.device
            self._group_sums = torch.zeros(grad_groups.n_groups, dtype=torch.float32, device=dev)
            if grad_groups.clip is not None:   # a frozen segment (group -1) takes the factor 1 appended behind the groups': it is never read
                self._group_seg_index = torch.tensor([g if g >= 0 else grad_groups.n_groups for _, g in grad_groups.refined], dtype=torch.int64, device=dev)

    def _refined_base(self, groups) -> list:
        """The refined segments this optimizer expects of ``groups``: its own segments (or one over everything) cut at the group boundaries."""
        from .grad_groups import refine
        return [s for s, _ in refine(self._segments, (groups.names, groups.seg_end, groups.seg_group))]

    # ---- gradient groups ---------------------------------------------------------------------------------------------------------------------
    def measure_grad_group_sums(self) -> Tensor:
        """ONE ``ssi_sumsq_groups`` launch over the flat gradient buffer: the fp32 sum of squares of every group (of the raw gradients: the
        pending scale is not in them).  Under data parallelism the reductions are finished first, as ``clip_grad_norm_`` does."""
        m, gg = self.model, self._groups
        sync = getattr(m, "grad_sync", None)
        if sync is not None and hasattr(sync, "finish_deferred"):
            sync.finish_deferred()   # the norms read every gradient
        if self._group_ws is None:   # (updates armed under the backward only READ the gradients: nothing to wait for)
            from . import _lib
            need = _lib.load().ssi_sumsq_groups_workspace_bytes(m._flat_grad.numel(), len(gg.seg_end), gg.n_groups)
            self._group_ws = torch.empty(need, dtype=torch.uint8, device=m._flat.device)
        ops.sumsq_groups(m._flat_grad, gg.seg_end, gg.seg_group, gg.n_groups, self._group_sums, workspace=self._group_ws)
        return self._group_sums

    def apply_grad_groups(self) -> dict[str, Tensor]:
        """After ``measure_grad_group_sums`` and whatever changes the pending scale (the global clip): the groups' norms as AdamW will see
        the gradients, and with a clip rule the coefficients the next ``step()`` applies.  Returns the window's values for the log."""
        gg, scale = self._groups, self.model.pending_grad_scale
        sums = self._group_sums
        values = {"norm": sums.sqrt() if scale is None else sums.sqrt() * scale.reshape(()).abs()}
        if gg.clip is not None:
            coef = gg.clip.update(sums, scale)
            self._group_coef = torch.cat([coef, torch.ones(1, dtype=torch.float32, device=coef.device)]).index_select(0, self._group_seg_index)
            values["clip"], values["skipped"] = coef, gg.clip.skipped
            if gg.clip.adaptive is not None:
                values["ema"] = gg.clip.gamma
        self.group_values = values
        return values

    def _update(self, lo: int, hi: int, g: dict, step: int, scale: Tensor | None, skip_nonfinite_scale: bool = False) -> None:
        """AdamW on the elements ``[lo, hi)`` of the flat buffers: the plain kernel, or with segments the segmented one on those that reach
        into the slice (nothing at all where every one of them is frozen)."""
        m = self.model
        bufs = (m._flat[lo:hi], m._flat_grad[lo:hi], self._exp_avg[lo:hi], self._exp_avg_sq[lo:hi])
        if self._group_coef is not None:
            refined = self._groups.refined
            a = next(k for k, (s, _) in enumerate(refined) if s.end > lo)
            b = next((k for k, (s, _) in enumerate(refined) if s.start >= hi), len(refined))
            segs = clip_segments([s for s, _ in refined[a:b]], lo, hi)
            if all(s.frozen for s in segs):
                return
            lr, wd = float(g["lr"]), float(g["weight_decay"])
            ops.adamw_step_seg(*bufs, seg_end=[s.end - lo for s in segs], seg_lr=[lr * s.lr_scale for s in segs],
                               seg_weight_decay=[wd if s.weight_decay is None else s.weight_decay for s in segs],
                               seg_frozen=[s.frozen for s in segs], beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"], step=step,
                               grad_scale_dev=scale, zero_grad=False, skip_nonfinite_scale=skip_nonfinite_scale, sr_seed=self._sr_seed,
                               elem_offset=lo, seg_scale_dev=self._group_coef[a:b])
        elif self._segments is None:
            ops.adamw_step(*bufs, lr=float(g["lr"]), beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"], weight_decay=g["weight_decay"],
                           step=step, grad_scale_dev=scale, zero_grad=False, skip_nonfinite_scale=skip_nonfinite_scale,
                           sr_seed=self._sr_seed, elem_offset=lo)
        else:
            segs = clip_segments(self._segments, lo, hi)
            if all(s.frozen for s in segs):
                return   # nothing launched, the average untouched
            lr, wd = float(g["lr"]), float(g["weight_decay"])
            ops.adamw_step_seg(*bufs, seg_end=[s.end - lo for s in segs], seg_lr=[lr * s.lr_scale for s in segs],
                               seg_weight_decay=[wd if s.weight_decay is None else s.weight_decay for s in segs],
                               seg_frozen=[s.frozen for s in segs], beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"], step=step,
                               grad_scale_dev=scale, zero_grad=False, skip_nonfinite_scale=skip_nonfinite_scale, sr_seed=self._sr_seed,
                               elem_offset=lo)
        self._update_ema(lo, hi, step, scale, skip_nonfinite_scale)

    def _update_ema(self, lo: int, hi: int, step: int, scale: Tensor | None, skip_nonfinite_scale: bool) -> None:
        """The average of the elements ``[lo, hi)`` follows their AdamW launch on the same stream: with segments one launch per maximal
        trainable range inside the slice — a frozen element's average is never read or written and stays its initial value."""
        if self._ema is None:
            return
        decay = ema_decay_at(step, self._ema_decay, self._ema_warmup)
        guard = scale if skip_nonfinite_scale else None
        for a, b in ([(lo, hi)] if self._ema_ranges is None else self._ema_ranges):
            a, b = max(a, lo), min(b, hi)
            if b > a:
                ops.ema_update(self._ema[a:b], self.model._flat[a:b], decay=decay, guard_dev=guard)

    # ---- the averaged weights ----------------------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def ema_weights(self):
        """Inside, the model holds the average rounded to nearest in its dtype (evaluate, save); on exit — also on an exception — the
        parameters are back bit for bit.  Costs one stash of the flat buffer in the model's dtype for the time inside.  Not nestable, and not
        while an overlap is armed (its updates would land in the swapped buffer)."""
        if self._ema is None:
            raise RuntimeError("ema_weights() needs an optimizer built with ema_decay")
        if self._ema_stash is not None:
            raise RuntimeError("ema_weights() is already active: it does not nest")
        if self._armed is not None:
            raise RuntimeError("ema_weights() while overlap_with_backward is armed: step() or cancel_overlap() first")
        m = self.model
        if self._side is not None:
            torch.cuda.current_stream(m._flat.device).wait_stream(self._side)
        self._ema_stash = m._flat.clone()
        try:
            with torch.no_grad():
                m._flat.copy_(self._ema)
            yield self
        finally:
            with torch.no_grad():
                m._flat.copy_(self._ema_stash)
            self._ema_stash = None

    def _ema_views(self) -> dict[str, Tensor]:
        if self._ema is None:
            raise RuntimeError("the optimizer was built without ema_decay: there is no average")
        m = self.model
        names = {id(p): n for n, p in m.named_parameters()}
        if self._side is not None:
            torch.cuda.current_stream(m._flat.device).wait_stream(self._side)
        return {names[id(p)]: m._view(name, rows, self._ema) for p, name, rows in m._param_src}

    def ema_state_dict(self) -> dict[str, Tensor]:
        """The fp32 averages by state-dict name (copies)."""
        return {k: v.detach().clone() for k, v in self._ema_views().items()}

    def load_ema_state_dict(self, sd) -> None:
        """Strict on names and shapes; values are taken as fp32."""
        own = self._ema_views()
        missing, unexpected = [k for k in own if k not in sd], [k for k in sd if k not in own]
        if missing or unexpected:
            raise RuntimeError(f"Error(s) in loading the EMA state: missing keys {missing}, unexpected keys {unexpected}")
        for k, v in own.items():
            if tuple(sd[k].shape) != tuple(v.shape):
                raise RuntimeError(f"size mismatch for {k}: EMA state {tuple(sd[k].shape)} vs model {tuple(v.shape)}")
        with torch.no_grad():
            for k, v in own.items():
                v.copy_(sd[k].to(device=v.device, dtype=torch.float32))

    def _ensure_state_views(self) -> None:
        if self._views_ready:
            return
        m = self.model
        for p, name, rows in m._param_src:
            self.state[p] = {
                "step": torch.tensor(float(self._step_count)),
                "exp_avg": m._view(name, rows, self._exp_avg),
                "exp_avg_sq": m._view(name, rows, self._exp_avg_sq),
            }
        self._views_ready = True

    # ---- AdamW under the backward (one GPU, no clipping) -----------------------------------------------------------------------------------
    def overlap_with_backward(self, grad_scale_dev: Tensor) -> bool:
        """Arm the optimizer for the window's LAST backward: every bucket of the flat gradient buffer (``HipLlamaDecoder.buckets``: the final
        norm, each layer's MLP block, each group's attention weights, the tied embedding) is updated on a side stream the moment that backward
        has finished its gradients, while the backward goes on — AdamW is a pure HBM pass (17 GB) and hides partly under the MFMA-bound
        GEMMs.  ``grad_scale_dev`` = the factor ``scale_grads`` would apply afterwards (1 / the window's token count; a DEVICE scalar, so no
        read-back is needed before the backward); ``step()`` then only joins the side stream and counts the step.  The arithmetic per element is
        the one of ``step()`` — same kernel, same scale, same step number — so the parameters come out bit for bit the same.  Not armed (returns
        False: the plain ``step()`` does all the work) under data parallelism (the buckets are still being reduced), or when gradients
        are to be clipped (the global norm needs every gradient first): the caller decides the latter by not calling this.  A window
        without a single label leaves a non-finite scale: the kernel then changes nothing, and the caller, who learns of the empty window
        at its read-back, must not call ``step()`` — exactly the reference's skip."""
        m = self.model
        if getattr(m, "grad_sync", None) is not None or not m._flat.is_cuda:
            return False
        if self._groups is not None and self._groups.clip is not None:
            return False   # a group's coefficient needs every gradient of the group first
        if self._side is None:
            self._side = torch.cuda.Stream(device=m._flat.device)
        self._armed = {"scale": grad_scale_dev.to(torch.float32).reshape(1), "done": [], "step": self._step_count + 1}
        m.bucket_listener = self._bucket_final
        return True

    def _bucket_final(self, name: str, lo: int, hi: int) -> None:
        a, g, m = self._armed, self.param_groups[0], self.model
        if a is None or hi <= lo:
            return
        cur = torch.cuda.current_stream(m._flat.device)
        ev = torch.cuda.Event()
        ev.record(cur)
        with torch.cuda.stream(self._side):
            self._side.wait_event(ev)
            self._update(lo, hi, g, a["step"], a["scale"], skip_nonfinite_scale=True)
        a["done"].append((lo, hi))

    def cancel_overlap(self) -> None:
        """Forget an armed overlap (a window that turned out empty: its updates were no-ops by the kernel's own guard)."""
        if self._armed is not None:
            torch.cuda.current_stream(self.model._flat.device).wait_stream(self._side)
        self._armed = None
        self.model.bucket_listener = None

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        g = self.param_groups[0]
        m = self.model
        if self._armed is not None and self._armed["done"]:
            # the buckets were updated under the backward: join the side stream, update whatever no bucket covered (nothing, by construction)
            a, self._armed = self._armed, None
            m.bucket_listener = None
            torch.cuda.current_stream(m._flat.device).wait_stream(self._side)
            self._step_count += 1
            assert a["step"] == self._step_count
            covered = sorted(a["done"])
            pos, n = 0, m._flat.numel()
            for lo, hi in covered + [(n, n)]:
                if lo > pos:  # a gap between buckets (none in HipLlamaDecoder's layout): the plain update, same scale
                    self._update(pos, lo, g, self._step_count, a["scale"])
                pos = max(pos, hi)
            m.pending_grad_scale = None  # (scale_grads of the caller: already applied, bucket by bucket)
            if self._views_ready:
                for st in self.state.values():
                    st["step"].fill_(float(self._step_count))
            return loss
        self._armed = None
        if all(p.grad is None for p, _, _ in m._param_src if p.requires_grad):   # (a frozen parameter never has a gradient)
            # no backward since the last zero_grad (skipped or failed micro-batches): torch.optim.AdamW skips parameters without a
            # gradient; the never-zeroed buffer still holds the LAST window's gradients, which must not be applied a second time
            sync = getattr(m, "grad_sync", None)
            if sync is not None and hasattr(sync, "finish_deferred"):
                sync.finish_deferred()
            m.pending_grad_scale = None
            return loss
        self._step_count += 1

        def update(lo: int, hi: int) -> None:
            if hi > lo:
                self._update(lo, hi, g, self._step_count, m.pending_grad_scale)

        sync = getattr(m, "grad_sync", None)
        tail = sync.deferred_range() if sync is not None and hasattr(sync, "deferred_range") else None
        n = m._flat.numel()
        if tail is None:
            update(0, n)
        else:  # data parallel: everything but the bucket still being reduced first, that bucket once it has arrived
            lo, hi = tail
            update(0, lo)
            update(hi, n)
            sync.finish_deferred()
            update(lo, hi)
        m.pending_grad_scale = None
        self._group_coef = None   # (a window's coefficients are applied once)
        # the gradients are NOT zeroed (2.5 GB of writes per step for nothing) and the window is NOT closed here: as with torch.optim, a
        # backward that follows a step without a zero_grad in between accumulates; zero_grad (this optimizer's, the model's, or a foreign
        # one that drops every p.grad) ends the window, and the first backward after it overwrites the buffer (model protocol)
        if self._views_ready:
            for st in self.state.values():
                st["step"].fill_(float(self._step_count))
        return loss

    def zero_grad(self, set_to_none: bool = True) -> None:
        # nothing to clear after a step (the next backward overwrites the buffer); the model zeroes only for set_to_none=False
        sync = getattr(self.model, "grad_sync", None)
        if sync is not None and hasattr(sync, "finish_deferred"):
            sync.finish_deferred()  # a step that was skipped must not zero under a reduction in flight
        self.model.zero_grad(set_to_none=set_to_none)

    def state_dict(self):
        self._ensure_state_views()
        return super().state_dict()

    def load_state_dict(self, state_dict) -> None:
        self._ensure_state_views()
        super().load_state_dict(state_dict)
        m = self.model
        step = 0
        for p, name, rows in m._param_src:  # re-home the loaded moments in the flat buffers
            st = self.state[p]
            ea, es = m._view(name, rows, self._exp_avg), m._view(name, rows, self._exp_avg_sq)
            ea.copy_(st["exp_avg"])
            es.copy_(st["exp_avg_sq"])
            st["exp_avg"], st["exp_avg_sq"] = ea, es
            step = int(float(st["step"]))
            st["step"] = torch.tensor(float(step))
        self._step_count = step
        if self._ema is not None:   # the average restarts from what the model now holds; load_ema_state_dict puts a saved one back
            self._ema.copy_(m._flat)


def _to_container(node):
    try:
        from .config import DictConfig, OmegaConf
        if isinstance(node, DictConfig):
            return OmegaConf.to_container(node, resolve=True)
    except Exception:  # pragma: no cover
        pass
    try:
        from omegaconf import OmegaConf as _OC  # type: ignore
        return _OC.to_container(node, resolve=True)
    except Exception:
        return dict(node)


def setup_optimizer(cfg, model, optimizer_state_dict: dict[str, Any] | None = None, *,
                    token_type_ranges: dict[str, tuple[int, int]] | None = None) -> torch.optim.Optimizer:
    optimizer_kwargs = _to_container(cfg.optimizer)
    rules = cfg.get("param_groups") if hasattr(cfg, "get") else None   # (top level: the rules name parameters, not optimizer arguments)
    if rules is not None:
        if not hasattr(model, "_flat"):
            raise ValueError(f"param_groups needs the HIP decoder (ranges of its flat parameter buffer); {type(model).__name__} has none")
        rules = [_to_container(r) if not isinstance(r, dict) else r for r in rules]
        layout, total = model_layout(model)
        optimizer_kwargs["param_segments"] = resolve(rules, layout, total, token_type_ranges)
    stochastic = bool(optimizer_kwargs.pop("stochastic_rounding", False))   # (both keys are this project's, not torch's)
    sr_seed = optimizer_kwargs.pop("stochastic_rounding_seed", None)
    ema_decay = cfg.get("ema_decay") if hasattr(cfg, "get") else None   # (top level, with ema_warmup: the average is the run's, not AdamW's)
    ema_warmup = cfg.get("ema_warmup", True) if hasattr(cfg, "get") else True
    groups = cfg.get("grad_groups") if hasattr(cfg, "get") else None   # (top level, beside param_groups: the same rule language)
    if groups is not None:
        if not hasattr(model, "_flat"):
            raise ValueError(f"grad_groups needs the HIP decoder (ranges of its flat gradient buffer); {type(model).__name__} has none")
        from .grad_groups import GradGroups
        layout, total = model_layout(model)
        groups = GradGroups.from_config(groups, layout, total, token_type_ranges, optimizer_kwargs.get("param_segments"), device=model._flat.device)
    if hasattr(model, "_flat"):
        optimizer = HipAdamW(model.parameters(), model=model, stochastic_rounding=stochastic, stochastic_rounding_seed=sr_seed,
                             ema_decay=ema_decay, ema_warmup=bool(ema_warmup), grad_groups=groups, **optimizer_kwargs)
    else:  # foreign module (tests with stand-in models): the reference's own choice
        if ema_decay is not None:
            raise ValueError("ema_decay needs the HIP decoder (HipAdamW averages its flat parameter buffer); "
                             f"{type(model).__name__} is updated by torch.optim.AdamW, which keeps no average")
        if stochastic:
            raise ValueError("optimizer.stochastic_rounding=true needs the HIP decoder (HipAdamW on its flat buffers); "
                             f"{type(model).__name__} is updated by torch.optim.AdamW, which has no such rounding")
        optimizer_kwargs.pop("fused", None)
        optimizer = torch.optim.AdamW(model.parameters(), **optimizer_kwargs)
    if optimizer_state_dict is not None:
        optimizer.load_state_dict(optimizer_state_dict)
    return optimizer


def _hip_optimizer_of(model):
    """The live :class:`HipAdamW` built on ``model`` (it registers itself), or None when the caller brought its own optimizer."""
    ref = getattr(model, "_hip_optimizer", None)
    return ref() if ref is not None else None


def scale_grads(model, scaler: Tensor | float) -> None:
    """torchtune ``training.scale_grads`` (``trainer.py:404``): ``p.grad *= scaler`` for every parameter.  On the HIP
    decoder the multiplication is deferred: it is folded into the optimizer kernel (and into the clip norm), saving a
    full read+write pass over the 2.5 GB gradient buffer.  Without a :class:`HipAdamW` on the model (INTEGRATION.md level 2: the
    caller's own ``torch.optim`` optimizer on the parameter views) nothing would ever consume a deferred factor, so the
    multiplication happens at once, in place, by the HIP ``scale`` kernel."""
    if hasattr(model, "_flat_grad"):
        # a host scalar becomes a device scalar by a FILL kernel, not by an asynchronous copy out of a temporary host tensor (whose memory the
        # allocator may hand out again while the copy is still queued: round 5 saw one bench.py run in eight end on a slightly different loss)
        dev = model._flat_grad.device
        if torch.is_tensor(scaler) and scaler.is_cuda:
            s = scaler.to(dev, torch.float32).reshape(1)
        else:
            s = torch.full((1,), float(scaler), dtype=torch.float32, device=dev)
        if _hip_optimizer_of(model) is None:  # a foreign optimizer reads p.grad itself: multiply now (one pass over the flat buffer)
            sync = getattr(model, "grad_sync", None)
            if sync is not None and hasattr(sync, "finish_deferred"):
                sync.finish_deferred()
            ops.scale_(model._flat_grad, scale_dev=s)
            return
        model.pending_grad_scale = s if model.pending_grad_scale is None else model.pending_grad_scale * s
        return
    for p in model.parameters():
        if p.grad is not None:
            p.grad *= scaler.to(p.grad.device) if isinstance(scaler, Tensor) else scaler


def clip_grad_norm_from_group_sums(model, max_norm: float, sums: Tensor) -> Tensor:
    """``clip_grad_norm_`` when ``grad_groups`` has already summed the window's gradients per group: the global sum of squares is the fp32 sum
    of the group sums in ascending group order (``other`` included: every trainable element), no second pass over the buffer."""
    out = sums[0:1]
    for k in range(1, sums.numel()):
        out = out + sums[k:k + 1]
    scale = model.pending_grad_scale if model.pending_grad_scale is not None else torch.ones_like(out)
    total_norm = out.sqrt() * scale.abs()
    coef = torch.clamp(float(max_norm) / (total_norm + 1e-6), max=1.0)
    model.pending_grad_scale = scale * coef
    return total_norm.reshape(())


def clip_grad_norm_(model, max_norm: float) -> Tensor:
    """``torch.nn.utils.clip_grad_norm_`` (``trainer.py:405-408``) on the flat gradient buffer: L2 norm by the HIP
    two-stage reduction, clip coefficient ``min(1, max_norm / (norm + 1e-6))`` folded into the pending gradient scale.
    Returns the total norm (device tensor, of the scaled gradients)."""
    if not hasattr(model, "_flat_grad"):
        return torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=float(max_norm))
    sync = getattr(model, "grad_sync", None)
    if sync is not None and hasattr(sync, "finish_deferred"):
        sync.finish_deferred()  # the norm reads every gradient
    out = torch.empty(1, dtype=torch.float32, device=model._flat_grad.device)
    opt = _hip_optimizer_of(model)
    if opt is not None and opt._segments is not None:
        # frozen ranges of the gradient buffer are unspecified (nothing writes them): the norm is over the trainable ranges only, one sum
        # per maximal range, added in ascending order
        ranges = trainable_ranges(opt._segments)
        parts = torch.zeros(max(len(ranges), 1), dtype=torch.float32, device=out.device)
        for k, (lo, hi) in enumerate(ranges):
            ops.sumsq(model._flat_grad[lo:hi], parts[k:k + 1])
        out = parts[0:1].clone()
        for k in range(1, len(ranges)):
            out = out + parts[k:k + 1]
    else:
        ops.sumsq(model._flat_grad, out)
    scale = model.pending_grad_scale if model.pending_grad_scale is not None else torch.ones_like(out)
    total_norm = out.sqrt() * scale.abs()
    coef = torch.clamp(float(max_norm) / (total_norm + 1e-6), max=1.0)
    if _hip_optimizer_of(model) is None:  # nobody will consume a deferred factor (scale is 1 here: scale_grads was eager too)
        ops.scale_(model._flat_grad, scale_dev=(scale * coef).reshape(1).contiguous())
        model.pending_grad_scale = None
    else:
        model.pending_grad_scale = scale * coef
    return total_norm.reshape(())
