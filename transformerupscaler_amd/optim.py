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
host) and takes the skipped step's `step` increments back.  `state_dict()` and `guard_stats()` settle the same way."""
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
_REC_GUARD = struct.Struct("<ddfifiQQQQ")       # GuardRec (64 bytes): sumsq, norm, coef, apply, norm_f32, clipped, steps, applied, clipped, skipped


class _FusedAdamStep:
    """The step of `Adam` and `AdamW` below (a mix-in in front of the torch class)."""

    def __init__(self, params, *args, max_grad_norm=None, skip_nonfinite=False, **kwargs):
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm >= 0.0:                      # negative or NaN
                raise ValueError(f"max_grad_norm must be >= 0 or None, got {max_grad_norm}")
        super().__init__(params, *args, **kwargs)
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
        event, slot, params = pending
        event.synchronize()
        rec = _REC_GUARD.unpack(bytes(slot.numpy().tobytes()))
        self.__dict__["_settled"] = rec
        if rec[3] == 0:                                       # apply == 0: GradScaler's semantics, nothing moved
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
        guarded = self._guarded
        if guarded:
            self._settle()
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
                continue
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
                if extended:
                    recs.append(_REC_GUARDED.pack(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                                  p.numel(), group["lr"] / bc1, math.sqrt(bc2), beta2, 1.0 - beta1, 1.0 - beta2,
                                                  group["eps"], wd_l2, decay))
                    if guarded:
                        norm_recs.append(_REC_NORM.pack(g.data_ptr(), p.numel()))
                else:
                    recs.append(_REC.pack(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(),
                                          group["lr"] / bc1, 1.0 / math.sqrt(bc2), beta2, 1.0 - beta1, 1.0 - beta2, group["eps"]))
                sizes.append(p.numel())
                updated.append(p)
                if g is not p.grad:
                    keep.append(g)
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
                if guarded:
                    self._guarded_launches(segs, norm_off, chunks, device, updated, _stream())
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
        return loss

    def _guarded_launches(self, segs, norm_off, chunks, device, updated, stream) -> None:
        """Norm, finish, step; then the record's asynchronous copy to a pinned slot for the next step()'s `_settle`."""
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
        _lib.call("tup_grad_sumsq_partial", segs.data_ptr() + norm_off, chunks.data_ptr(), nchunks, partials.data_ptr(), stream)
        _lib.call("tup_grad_guard_finish", partials.data_ptr(), nchunks, max_norm, int(self.skip_nonfinite), guard.data_ptr(), stream)
        _lib.call("tup_adam_step_guarded", segs.data_ptr(), chunks.data_ptr(), nchunks, guard.data_ptr(), stream)
        turn = d["_guard_turn"] = d["_guard_turn"] ^ 1
        # the slot's previous content (two steps ago) was consumed by the last step()'s _settle
        d["_guard_slots"][turn].copy_(guard, non_blocking=True)
        d["_guard_events"][turn].record()
        d["_pending"] = (d["_guard_events"][turn], d["_guard_slots"][turn], list(updated))


class Adam(_FusedAdamStep, torch.optim.Adam):
    pass


class AdamW(_FusedAdamStep, torch.optim.AdamW):
    pass
