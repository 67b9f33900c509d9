"""`Adam` / `AdamW`: torch.optim.Adam (reference train.py:104 `optim.Adam(model.parameters(), lr=args.lr)`, stepped at train.py:139)
and torch.optim.AdamW with the update of ALL parameters in one HIP launch (`tup_adam_step`, csrc/pack_plan.hip) instead of torch's
~13 multi-tensor launches per step.  Drop-in subclasses: same constructor, same `state_dict()` layout (`step`, `exp_avg`,
`exp_avg_sq` per parameter -- a checkpoint written by one loads into the other), same semantics for parameters without a gradient
(skipped: no state, no step).  Weight decay runs in the fused launch too (`tup_adam_step_guarded`, csrc/step_guard.hip:
Adam's ``g += wd * p``, AdamW's ``p *= 1 - lr * wd``).  Options the kernels do not implement (amsgrad, maximize, capturable /
differentiable) and parameters they cannot take (not fp32 / not on the GPU / sparse gradients) fall through to torch's own step,
per parameter group.

Two keyword options guard the step, both decided on the device without a host synchronisation:

* ``max_grad_norm=c``: torch.nn.utils.clip_grad_norm_'s clipping.  The norm is global over every parameter of every group with
  ``grad is not None``; the step uses ``min(1, c / (norm + 1e-6)) * grad``.  The gradients are NOT rewritten: ``p.grad`` keeps the
  unclipped values (clip_grad_norm_ scales them in place).
* ``skip_nonfinite=True``: GradScaler's skipping (reference train.py:136-139).  A step whose gradients hold an inf or a NaN leaves
  every parameter, `exp_avg`, `exp_avg_sq` and `step` as they were.

They are attributes of the optimizer, not param-group keys, so `state_dict()` stays interchangeable with torch's.  With either set,
a group the kernel cannot take raises ValueError (no silent fallback).  ``optimizer.grad_norm`` is a device fp32 scalar with the last
step's pre-clip norm (reading it takes no synchronisation of its own); ``optimizer.guard_stats()`` returns the settled counts
``{"steps", "applied", "clipped", "skipped"}``.

The host computes the bias corrections from `step`, so it has to learn of a skipped step: every guarded step copies the 64-byte
guard record to a pinned slot behind an event, the NEXT `step()` waits for that event (the GPU is then at most one step behind the
host) and takes the skipped step's `step` increments back.  `state_dict()` and `guard_stats()` settle the same way.

``ema_decay=d`` (0 <= d < 1) keeps an exponential moving average of every stepped parameter, updated inside the step's own launch
(`tup_adam_step_ema`, csrc/step_guard.hip): ``e = e + (1 - d_n) * (p_new - e)`` as three rounded fp32 operations, with
``d_n = ema_decay_at(n, d, ema_warmup)`` and n the count of applied updates (``optimizer.ema_updates``).  A step the guard skips on
the device moves neither the weights nor the average nor n.  The buffers live outside ``optimizer.state`` (`state_dict()` stays
torch's); a parameter's buffer is created at its first step as a copy of the parameter before that update, and from then on it is
in every step's table, with a gradient or without (a segment with ``g == NULL``: the average alone moves).  The raw parameters,
`exp_avg` and `exp_avg_sq` are bit-equal to the same run without the option.  Groups that fall through to torch's step update
their averages with the same three torch operations.  ``ema_state_dict(model)`` / ``load_ema_state_dict(model, sd, updates)``
export and load the average in the model's `state_dict()` layout; ``harness.ema_weights(model, optimizer)`` runs the model on it."""
from __future__ import annotations

import math
import struct
from typing import List

import torch

from . import _lib

_CHUNK = 4096
_REC = struct.Struct("<QQQQqffffff")            # AdamSeg of csrc/pack_plan.hip (64 bytes)
_REC_GUARDED = struct.Struct("<QQQQqffffffff")  # AdamWSeg of csrc/step_guard.hip (72 bytes): ..., bc2_sqrt in place of its inverse, wd_l2, decay
_REC_NORM = struct.Struct("<Qq")                # NormSeg (16 bytes): g, n
_REC_EMA = struct.Struct("<QQQQqffffffffQfi")   # AdamEmaSeg (88 bytes): AdamWSeg's fields (bc2: by form), e, ema_w, form (0: _REC's arithmetic, 1: _REC_GUARDED's)
_REC_GUARD = struct.Struct("<ddfifiQQQQ")       # GuardRec (64 bytes): sumsq, norm, coef, apply, norm_f32, clipped, steps, applied, clipped, skipped


def ema_decay_at(n: int, decay: float, warmup: bool = False) -> float:
    """The decay d_n of EMA update n (0-based count of applied updates): `decay`, or with `warmup` timm's schedule
    ``min(decay, (1 + n) / (10 + n))`` (0.1 at n = 0, reaching `decay` and staying there)."""
    decay = float(decay)
    return min(decay, (1 + n) / (10 + n)) if warmup else decay


def _f32(x: float) -> float:
    """x rounded to fp32 (round to nearest, as the record's field holds it)."""
    return struct.unpack("<f", struct.pack("<f", x))[0]


class _EmaBook:
    """The host side of the weight average, shared by the fused step below and harness's torch arm: the options, the buffers (a
    dict parameter -> tensor outside `optimizer.state`), the count of applied updates and the three-op update in torch."""

    def _init_ema(self, ema_decay, ema_warmup) -> None:
        if ema_decay is not None:
            ema_decay = float(ema_decay)
            if not 0.0 <= ema_decay < 1.0:                    # also a NaN
                raise ValueError(f"ema_decay must be in [0, 1) or None, got {ema_decay}")
        self.ema_decay = ema_decay
        self.ema_warmup = bool(ema_warmup)
        self._ema = {}
        self._ema_n = 0
        self._ema_swapped = False                             # harness.ema_weights is active: the parameters hold the averages

    def _ema_settle(self) -> None:
        settle = getattr(self, "_settle", None)
        if settle is not None:
            settle()

    @property
    def ema_updates(self) -> int:
        """The settled count of applied EMA updates (a step skipped on the device is not one)."""
        self._ema_settle()
        return self.__dict__.get("_ema_n", 0)

    def _ema_weight(self) -> float:
        """fp32(1 - d_n) of the next update, rounded from double."""
        return _f32(1.0 - ema_decay_at(self._ema_n, self.ema_decay, self.ema_warmup))

    def _ema_buffer(self, p):
        """p's buffer, created on first use as a copy of p as it is now (before its first update)."""
        e = self._ema.get(p)
        if e is None:
            e = self._ema[p] = p.detach().clone(memory_format=torch.contiguous_format)
        return e

    @staticmethod
    def _ema_torch_update(p, e, w: float) -> None:
        """e = e + w * (p - e): sub, mul, add, each rounded -- the kernel's three operations."""
        d = torch.sub(p.detach(), e)
        d.mul_(w)
        e.add_(d)

    def _ema_check_step(self) -> None:
        if self.__dict__.get("_ema_swapped", False):
            raise RuntimeError("optimizer.step() inside harness.ema_weights(): the parameters hold the averaged weights")

    def ema_state_dict(self, model) -> dict:
        """The averaged weights with exactly ``model.state_dict()``'s keys and order: a parameter's average, or the parameter itself
        where it has no buffer (never stepped: its average is its value); buffers are copied."""
        if self.__dict__.get("ema_decay") is None:
            raise RuntimeError("ema_state_dict(): the optimizer was built without ema_decay")
        self._ema_settle()
        params = dict(model.named_parameters(remove_duplicate=False))
        out = {}
        for k, v in model.state_dict().items():
            p = params.get(k)
            e = None if p is None or self._ema_swapped else self._ema.get(p)
            out[k] = (v if e is None else e).detach().clone()
        return out

    def load_ema_state_dict(self, model, sd, updates: int = 0) -> None:
        """Load averages in the `ema_state_dict` layout (every parameter of `model` gets a buffer) and set the update count."""
        if self.__dict__.get("ema_decay") is None:
            raise RuntimeError("load_ema_state_dict(): the optimizer was built without ema_decay")
        self._ema_check_step()
        self._ema_settle()
        params = dict(model.named_parameters())
        missing = [k for k in params if k not in sd]
        if missing:
            raise KeyError(f"load_ema_state_dict(): no entry for {missing[:3]}{' ...' if len(missing) > 3 else ''}")
        for k, p in params.items():
            v = sd[k]
            if tuple(v.shape) != tuple(p.shape):
                raise ValueError(f"load_ema_state_dict(): {k} has shape {tuple(v.shape)}, the parameter {tuple(p.shape)}")
            self._ema[p] = v.detach().to(device=p.device, dtype=p.dtype, copy=True).contiguous()
        self._ema_n = int(updates)


class _FusedAdamStep(_EmaBook):
    """The step of `Adam` and `AdamW` below (a mix-in in front of the torch class)."""

    def __init__(self, params, *args, max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=False, **kwargs):
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm >= 0.0:                      # negative or NaN
                raise ValueError(f"max_grad_norm must be >= 0 or None, got {max_grad_norm}")
        super().__init__(params, *args, **kwargs)
        self._init_ema(ema_decay, ema_warmup)
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = bool(skip_nonfinite)
        if self._guarded:
            for group in self.param_groups:
                self._require_guardable(group, group["params"])

    @property
    def _guarded(self) -> bool:
        return self.__dict__.get("max_grad_norm") is not None or self.__dict__.get("skip_nonfinite", False)

    def _fusable(self, group) -> bool:
        return (not group.get("amsgrad", False) and not group.get("maximize", False)
                and not group.get("capturable", False) and not group.get("differentiable", False)
                and not torch.is_tensor(group["lr"]) and not torch.is_tensor(group.get("weight_decay", 0))
                and not any(torch.is_tensor(b) for b in group["betas"]))

    def _require_guardable(self, group, params) -> None:
        if not self._fusable(group):
            raise ValueError("max_grad_norm / skip_nonfinite need the fused step: amsgrad, maximize, capturable, differentiable and "
                             "tensor hyper-parameters are not supported with them")
        for p in params:
            if not p.is_cuda or p.dtype != torch.float32 or p.is_sparse:
                raise ValueError(f"max_grad_norm / skip_nonfinite need dense fp32 parameters on the GPU, got {p.dtype} on {p.device}")

    # ---- the guard's host side ----
    def _settle(self) -> None:
        """Wait for the last guarded step's record and, if that step was skipped on the device, take its `step` counts back."""
        pending = self.__dict__.pop("_pending", None)
        if pending is None:
            return
        event, slot, params, ema_counted = pending
        event.synchronize()
        rec = _REC_GUARD.unpack(bytes(slot.numpy().tobytes()))
        self.__dict__["_settled"] = rec
        if rec[3] == 0:                                       # apply == 0: GradScaler's semantics, nothing moved
            if ema_counted:                                   # ... the average included
                self.__dict__["_ema_n"] -= 1
            for p in params:
                st = self.state[p]
                st["step"] -= 1
                if float(st["step"]) == 0.0:                  # state this very step created: torch would not have any
                    del self.state[p]

    def guard_stats(self) -> dict:
        """Settled counts of the guarded steps so far (waits for the last one)."""
        self._settle()
        rec = self.__dict__.get("_settled")
        if rec is None:
            return {"steps": 0, "applied": 0, "clipped": 0, "skipped": 0}
        return {"steps": rec[6], "applied": rec[7], "clipped": rec[8], "skipped": rec[9]}

    @property
    def grad_norm(self):
        """Device fp32 scalar: the global gradient norm of the last guarded step before clipping (None before the first one)."""
        guard = self.__dict__.get("_guard")
        return None if guard is None else guard.view(torch.float32)[6]

    def state_dict(self):
        self._settle()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        self._settle()
        return super().load_state_dict(state_dict)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._ema_check_step()
        guarded = self._guarded
        if guarded:
            self._settle()
        ema = self.__dict__.get("ema_decay") is not None
        ema_w = self._ema_weight() if ema else 0.0
        idle_recs: List[bytes] = []                            # EMA on: parameters with a buffer and no gradient in this step (g = NULL)
        idle_sizes: List[int] = []
        torch_ema: list = []                                   # ... and the parameters whose average torch updates (fall-through groups)
        decoupled_cls = isinstance(self, torch.optim.AdamW)
        recs: List[bytes] = []
        norm_recs: List[bytes] = []                            # the norm pass's (g, n) table, in the order of `recs`
        sizes: List[int] = []
        updated: list = []                                     # parameters the launch writes (their version is bumped below)
        keep: list = []                                        # tensors the asynchronous launch reads: alive until the next step
        device = None
        fallback_groups = []
        # the 72-byte record and tup_adam_step_guarded: under the guard, and wherever a weight decay is set
        extended = guarded or any(group.get("weight_decay", 0) != 0 for group in self.param_groups)
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            idle = [p for p in group["params"] if p.grad is None and p in self._ema] if ema else []
            ok = self._fusable(group) and all(
                p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.grad.dtype == torch.float32
                and not p.grad.is_sparse and p.grad.device == p.device for p in ps)
            if ok and ps:
                if device is None:
                    device = ps[0].device
                ok = all(p.device == device for p in ps)
            if not ok:
                if guarded:
                    self._require_guardable(group, ps)
                    raise ValueError("max_grad_norm / skip_nonfinite need contiguous fp32 parameters with dense fp32 gradients on one GPU")
                fallback_groups.append(group)
                if ema:
                    torch_ema += [(p, self._ema_buffer(p)) for p in ps + idle]
                continue
            for p in idle:                                    # the average still moves (timm, swa_utils.AveragedModel: every update)
                e = self._ema[p]
                if p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and (device is None or p.device == device):
                    device = p.device
                    idle_recs.append(_REC_EMA.pack(p.data_ptr(), 0, 0, 0, p.numel(), 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0,
                                                   e.data_ptr(), ema_w, 0))
                    idle_sizes.append(p.numel())
                else:
                    torch_ema.append((p, e))
            beta1, beta2 = group["betas"]
            wd = float(group.get("weight_decay", 0))
            decoupled = decoupled_cls or bool(group.get("decoupled_weight_decay", False))
            wd_l2 = 0.0 if decoupled else wd
            decay = 1.0 - group["lr"] * wd if decoupled else 1.0
            for p in ps:
                st = self.state[p]
                if len(st) == 0:                              # same lazy state as torch.optim.Adam
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                t = float(st["step"])
                bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                if ema:                                       # the record of either form below, then e, ema_w, form
                    e = self._ema_buffer(p)
                    recs.append(_REC_EMA.pack(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                              p.numel(), group["lr"] / bc1, math.sqrt(bc2) if extended else 1.0 / math.sqrt(bc2), beta2,
                                              1.0 - beta1, 1.0 - beta2, group["eps"], wd_l2 if extended else 0.0,
                                              decay if extended else 1.0, e.data_ptr(), ema_w, 1 if extended else 0))
                elif extended:
                    recs.append(_REC_GUARDED.pack(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                                  p.numel(), group["lr"] / bc1, math.sqrt(bc2), beta2, 1.0 - beta1, 1.0 - beta2,
                                                  group["eps"], wd_l2, decay))
                else:
                    recs.append(_REC.pack(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(),
                                          group["lr"] / bc1, 1.0 / math.sqrt(bc2), beta2, 1.0 - beta1, 1.0 - beta2, group["eps"]))
                if guarded:
                    norm_recs.append(_REC_NORM.pack(g.data_ptr(), p.numel()))
                sizes.append(p.numel())
                updated.append(p)
                if g is not p.grad:
                    keep.append(g)
        n_norm = sum(-(-n // _CHUNK) for n in sizes)           # workgroups of the gradient segments: the norm pass runs on these
        recs += idle_recs                                      # gradient segments first, so that the norm table is the chunk table's head
        sizes += idle_sizes
        ema_counted = ema and bool(recs or torch_ema)
        if recs:
            key = tuple(sizes)
            cache = self.__dict__.setdefault("_chunk_cache", {})
            chunks = cache.get((key, device))
            if chunks is None:                                # (segment, first element) per 4096 elements; changes only with the grad set
                tab = []
                for si, n in enumerate(sizes):
                    tab += [(si, off) for off in range(0, n, _CHUNK)]
                chunks = cache[(key, device)] = torch.tensor(tab, dtype=torch.int32).to(device)
            # gradient pointers change every step: the table goes up through one of two pinned staging buffers (a pageable
            # source would make the copy synchronous and stall the host behind the whole backward)
            raw = b"".join(recs)
            norm_off = len(raw)
            if guarded:                                       # the norm table rides in the same upload
                raw += b"".join(norm_recs)
            stage = self.__dict__.setdefault("_stage", [None, None, 0])
            events = self.__dict__.setdefault("_stage_events", [None, None])
            slot = stage[2] = stage[2] ^ 1
            # the host may run several steps ahead of the GPU (no per-step sync in a training loop): a slot is rewritten only
            # after the asynchronous upload that last read it has executed
            if events[slot] is not None:
                events[slot].synchronize()
            if stage[slot] is None or stage[slot].numel() * 8 < len(raw):
                stage[slot] = torch.empty(len(raw) // 8, dtype=torch.int64).pin_memory()
            host = stage[slot][:len(raw) // 8]
            host.copy_(torch.frombuffer(bytearray(raw), dtype=torch.int64))
            from .ops import _stream
            with torch.cuda.device(device):
                segs = host.to(device, non_blocking=True)
                if events[slot] is None:
                    events[slot] = torch.cuda.Event()
                events[slot].record()
                if guarded and (n_norm or not ema):
                    self._guarded_launches(segs, norm_off, chunks, device, updated, _stream(), n_norm, ema, ema_counted)
                elif ema:                                     # (under the guard: averages alone, no gradient to decide on)
                    _lib.call("tup_adam_step_ema", segs.data_ptr(), chunks.data_ptr(), chunks.shape[0], None, _stream())
                elif extended:
                    _lib.call("tup_adam_step_guarded", segs.data_ptr(), chunks.data_ptr(), chunks.shape[0], None, _stream())
                else:
                    _lib.call("tup_adam_step", segs.data_ptr(), chunks.data_ptr(), chunks.shape[0], _stream())
            keep.append(segs)
            # the launch writes the parameters through raw pointers: tell autograd (saved-tensor checks) and every cache keyed on
            # (data_ptr, _version) -- the models' packed-weight caches -- that they changed, as an in-place torch update would
            for p in updated:
                torch.autograd.graph.increment_version(p)
        self.__dict__["_keep"] = keep
        if fallback_groups:
            saved = self.param_groups
            self.param_groups = fallback_groups
            try:
                super().step()
            finally:
                self.param_groups = saved
        for p, e in torch_ema:
            self._ema_torch_update(p, e, ema_w)
        if ema_counted:
            self._ema_n += 1
        return loss

    def _guarded_launches(self, segs, norm_off, chunks, device, updated, stream, n_norm, ema, ema_counted) -> None:
        """Norm, finish, step; then the record's asynchronous copy to a pinned slot for the next step()'s `_settle`.  The norm pass
        takes the chunk table's first `n_norm` rows (the segments with a gradient; without EMA that is all of them)."""
        d = self.__dict__
        guard = d.get("_guard")
        if guard is None or guard.device != device:
            guard = d["_guard"] = torch.zeros(8, dtype=torch.int64, device=device)          # the 64-byte GuardRec, counters at zero
            d["_guard_slots"] = [torch.zeros(8, dtype=torch.int64).pin_memory() for _ in range(2)]
            d["_guard_events"] = [torch.cuda.Event(), torch.cuda.Event()]
            d["_guard_turn"] = 0
        nchunks = chunks.shape[0]
        partials = d.get("_partials")
        if partials is None or partials.numel() < nchunks or partials.device != device:
            partials = d["_partials"] = torch.empty(max(nchunks, 1024), dtype=torch.float64, device=device)
        max_norm = -1.0 if self.max_grad_norm is None else self.max_grad_norm
        _lib.call("tup_grad_sumsq_partial", segs.data_ptr() + norm_off, chunks.data_ptr(), n_norm, partials.data_ptr(), stream)
        _lib.call("tup_grad_guard_finish", partials.data_ptr(), n_norm, max_norm, int(self.skip_nonfinite), guard.data_ptr(), stream)
        _lib.call("tup_adam_step_ema" if ema else "tup_adam_step_guarded", segs.data_ptr(), chunks.data_ptr(), nchunks, guard.data_ptr(), stream)
        turn = d["_guard_turn"] = d["_guard_turn"] ^ 1
        # the slot's previous content (two steps ago) was consumed by the last step()'s _settle
        d["_guard_slots"][turn].copy_(guard, non_blocking=True)
        d["_guard_events"][turn].record()
        d["_pending"] = (d["_guard_events"][turn], d["_guard_slots"][turn], list(updated), ema_counted)


class Adam(_FusedAdamStep, torch.optim.Adam):
    pass


class AdamW(_FusedAdamStep, torch.optim.AdamW):
    pass
