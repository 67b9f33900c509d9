"""`GradAccumulator`: the gradients of a whole mixed-scale training step in one flat fp32 arena, one launch per backward.

The reference's step (train.py:110-146) runs a list of (lr, hr) pairs of different sizes and scales, averages the losses and steps
the optimizer once.  `harness.train_step_samples` runs one backward per group of equal-shaped samples and hands each backward's
gradients to `add()`, which is one `tup_grad_accumulate` launch (csrc/grad_accumulate.hip) for the whole dict instead of one aten
``add_`` per parameter: a parameter's first gradient of the step is copied into its segment (mode 0), later ones are added
(mode 1), so the arena is never zero-filled as a whole.  With ``alpha == 1`` that is torch's own ``grad += g`` to the bit.

    acc = GradAccumulator(module)                 # or GradAccumulator(module, dp.reducer) under data parallelism
    acc.begin(); acc.add(grads_of_group_0); acc.add(grads_of_group_1); acc.finish(); optimizer.step()

`finish()` without a reducer gives every touched parameter ``p.grad`` = its view of the arena; untouched parameters keep
``grad is None``, so Adam skips the scales the step did not use.  With a `dp.GradReducer` the arena has the reducer's
layout, untouched segments are zero-filled (mode 2), and the arena is all-reduced ONCE per step (`GradReducer.reduce_flat`); a
parameter then gets a gradient iff some rank touched it.

The arena is reused across steps and ordered by the stream: the previous step's Adam launch read it on the stream this step's
first launch writes it on.  ``p.grad`` therefore holds a step's gradient until the next step's first `add()`; clone it to keep it.
"""
from __future__ import annotations

import struct
from typing import Dict, List, Optional

import torch

from . import _lib

_CHUNK = 4096
_REC = struct.Struct("<QQqfi")          # AccSeg of csrc/grad_accumulate.hip: dst, src, n, alpha, mode


class SegmentLauncher:
    """`tup_grad_accumulate` for a list of (dst, src, n, alpha, mode): the pointer table changes with every launch, so it goes up
    through one of two pinned staging buffers (as optim.Adam.step does); the chunk table depends on the sizes only and is cached."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._chunks: Dict[tuple, torch.Tensor] = {}
        self._stage = [None, None]
        self._events = [None, None]
        self._slot = 0
        self._keep = None

    def launch(self, segs: List[tuple]) -> None:
        """segs: (dst data_ptr, src data_ptr or 0, n, alpha, mode).  The caller keeps dst / src alive until the launch is issued;
        both were allocated on the current stream, which also orders their reuse."""
        segs = [s for s in segs if s[2] > 0]
        if not segs:
            return
        sizes = tuple(s[2] for s in segs)
        chunks = self._chunks.get(sizes)
        if chunks is None:                                    # (segment, first element) per 4096 elements
            tab = []
            for si, n in enumerate(sizes):
                tab += [(si, off) for off in range(0, n, _CHUNK)]
            chunks = self._chunks[sizes] = torch.tensor(tab, dtype=torch.int32).to(self.device)
        raw = b"".join(_REC.pack(d, s, n, a, m) for d, s, n, a, m in segs)
        slot = self._slot = self._slot ^ 1
        # the host may run ahead of the GPU: a staging slot is rewritten only after the upload that last read it has executed
        if self._events[slot] is not None:
            self._events[slot].synchronize()
        if self._stage[slot] is None or self._stage[slot].numel() * 8 < len(raw):
            self._stage[slot] = torch.empty(max(len(raw) // 8, 1024), dtype=torch.int64).pin_memory()
        host = self._stage[slot][:len(raw) // 8]
        host.copy_(torch.frombuffer(bytearray(raw), dtype=torch.int64))
        from .ops import _stream
        with torch.cuda.device(self.device):
            table = host.to(self.device, non_blocking=True)
            if self._events[slot] is None:
                self._events[slot] = torch.cuda.Event()
            self._events[slot].record()
            _lib.call("tup_grad_accumulate", table.data_ptr(), chunks.data_ptr(), chunks.shape[0], _stream())
        self._keep = table


class GradAccumulator:
    def __init__(self, module, reducer=None):
        """module: any of the trainable plugins; reducer: a dp.GradReducer (its layout is used and `finish()` all-reduces through
        it), or None for a single process (every ``requires_grad`` parameter in ``named_parameters()`` order)."""
        self.module = module
        self.reducer = reducer
        self.params: Dict[str, torch.nn.Parameter] = {n: p for n, p in module.named_parameters() if p.requires_grad}
        if not self.params:
            raise ValueError("GradAccumulator: the module has no trainable parameter")
        first = next(iter(self.params.values()))
        if not first.is_cuda:
            raise ValueError("GradAccumulator: the module must live on the GPU (there is no CPU path)")
        self.device = first.device
        if reducer is not None:
            self.names: List[str] = list(reducer.names)
            missing = [n for n in self.names if n not in self.params]
            if missing:
                raise ValueError(f"GradAccumulator: the reducer's layout names {missing[:3]} which the module does not train")
            self.offset = dict(reducer.offset)
            self.numel = dict(reducer.numel)
            self.total_floats = int(reducer.total_floats)
            for n in self.names:
                if self.numel[n] != self.params[n].numel():
                    raise ValueError(f"GradAccumulator: {n} has {self.params[n].numel()} elements, the reducer's layout {self.numel[n]}")
        else:
            self.names = list(self.params)
            self.offset, self.numel = {}, {}
            cur = 0
            for n in self.names:                              # 64-float (256 B) aligned segments, as dp.GradReducer lays them out
                self.offset[n] = cur
                self.numel[n] = self.params[n].numel()
                cur += (self.numel[n] + 63) // 64 * 64
            self.total_floats = cur
        for n in self.names:
            p = self.params[n]
            if p.dtype != torch.float32 or p.device != self.device:
                raise TypeError(f"GradAccumulator: {n} is {p.dtype} on {p.device}; expected fp32 parameters on {self.device}")
        # zeroed once, so the alignment gaps (all-reduced with the buckets, never read) hold zeros; segments are written per step
        self.arena = torch.zeros(max(self.total_floats, 1), dtype=torch.float32, device=self.device)
        self._base = self.arena.data_ptr()
        # the per-parameter views handed out as p.grad: the arena never moves, so they are built once
        self._views = {n: self.arena[self.offset[n]:self.offset[n] + self.numel[n]].view(self.params[n].shape) for n in self.names}
        self._launcher = SegmentLauncher(self.device)
        self._touched: Optional[set] = None

    def view(self, name: str) -> torch.Tensor:
        return self._views[name]

    def begin(self) -> None:
        """Start a step with nothing touched."""
        self._touched = set()

    def add(self, grads: Dict[str, Optional[torch.Tensor]], alpha: float = 1.0) -> None:
        """Accumulate one backward's gradients ({name: tensor or None}): one launch for the whole dict."""
        if self._touched is None:
            raise RuntimeError("GradAccumulator.add() outside a step: call begin() first")
        segs, keep = [], []
        for n, g in grads.items():
            if g is None:
                continue
            if n not in self.offset:
                raise RuntimeError(f"gradient {n} is not in this accumulator's layout"
                                   + ("" if self.reducer is None else " (the step's scale is outside DataParallel(scales=...))"))
            if g.numel() != self.numel[n]:
                raise ValueError(f"gradient {n}: {tuple(g.shape)} does not match the parameter {tuple(self.params[n].shape)}")
            if not g.is_cuda or g.device != self.device or g.dtype != torch.float32 or g.is_sparse:
                raise TypeError(f"gradient {n}: expected a dense fp32 tensor on {self.device}, got {g.dtype} on {g.device}")
            if not g.is_contiguous():
                g = g.contiguous()
            keep.append(g)
            segs.append((self._base + 4 * self.offset[n], g.data_ptr(), self.numel[n], float(alpha), 1 if n in self._touched else 0))
        self._launcher.launch(segs)
        for n, g in grads.items():
            if g is not None:
                self._touched.add(n)
        del keep

    def finish(self) -> List[str]:
        """Close the step: hand the gradients to the parameters (module docstring); returns the names that got one."""
        if self._touched is None:
            raise RuntimeError("GradAccumulator.finish() outside a step: call begin() first")
        touched, self._touched = self._touched, None
        if self.reducer is None:
            have = [n for n in self.names if n in touched]
        else:
            # what this rank did not produce counts as zeros in the sum
            self._launcher.launch([(self._base + 4 * self.offset[n], 0, self.numel[n], 0.0, 2) for n in self.names if n not in touched])
            have = self.reducer.reduce_flat(self.arena, touched)
        for n in have:
            self.params[n].grad = self._views[n]
        return have
