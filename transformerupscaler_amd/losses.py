"""Training losses on the quantities the scorer reports (metrics.py, ab_test.py): L1 (the reference's nn.L1Loss, train.py:103),
MSE (nn.MSELoss, ab_test.py:96-124) and SSIM (skimage's defaults, inference.py:136-140), with a HIP forward and backward
(csrc/quality_loss.hip).

    loss = quality_loss(out, target, l1=1.0, mse=0.0, ssim=0.0, data_range=1.0)
         = l1 * mean|out - target| + mse * mean (out - target)^2 + ssim * (1 - mean_b SSIM(out[b], target[b]))

SSIM is the quantity ``metrics.ssim`` returns -- the forward runs the scorer's own kernel -- so a model is trained on exactly
the number the A/B driver prints.  `out` and `target` are fp32 planar ``[B][3][H][W]`` GPU tensors of equal shape, H, W >= 7; the
result is a scalar fp32 GPU tensor.  Only `out` receives a gradient: one materialised fp32 tensor, which the model nodes take
through their plain-gradient paths (the fused-L1 hand-off of ``autograd.l1_loss`` is not involved).  Neither direction
synchronises with the host or uses atomics: loss and gradient are bit-identical across runs, and a pixel's gradient does not
depend on the other images of the batch.  There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

import torch

from . import _lib
from .metrics import WIN, _partials
from .ops import _chk, _stream

F32, F64 = torch.float32, torch.float64
L1_BLOCKS = 2048


def _check(out, target, l1, mse, ssim):
    if l1 == 0 and mse == 0 and ssim == 0:
        raise ValueError("quality_loss: all of l1, mse and ssim are 0 -- there is nothing to minimise")
    if out.dim() != 4 or out.shape[1] != 3:
        raise ValueError(f"out: expected fp32 planar [B][3][H][W], got shape {tuple(out.shape)}")
    if target.shape != out.shape:
        raise ValueError(f"target: expected shape {tuple(out.shape)}, got {tuple(target.shape)}")
    B, _, H, W = out.shape
    if H < WIN or W < WIN:
        raise ValueError(f"image of {H}x{W}: SSIM's 7x7 window needs H and W >= 7")
    _chk(out, F32, None, "out")
    _chk(target, F32, out.shape, "target")
    return B, H, W


class _QualityLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, target, l1, mse, ssim, data_range):
        B, H, W = _check(out, target, l1, mse, ssim)
        ctx.save_for_backward(out, target)
        ctx.weights = (float(l1), float(mse), float(ssim), float(data_range))
        s = _stream()
        loss = torch.empty((), dtype=F32, device=out.device)
        qpart = l1part = None
        nparts = 0
        if mse != 0 or ssim != 0:
            nparts = _partials(H, W)
            qpart = torch.empty((B, 3, nparts, 2), dtype=F64, device=out.device)
            _lib.call("tup_quality_f32_partial", out.data_ptr(), target.data_ptr(), qpart.data_ptr(), B, H, W, nparts,
                      float(data_range), s)
        if l1 != 0:
            l1part = torch.empty((L1_BLOCKS,), dtype=F32, device=out.device)
            _lib.call("tup_l1_loss_partial", out.data_ptr(), target.data_ptr(), l1part.data_ptr(), out.numel(), L1_BLOCKS, s)
        _lib.call("tup_quality_loss_reduce", None if qpart is None else qpart.data_ptr(), None if l1part is None else l1part.data_ptr(),
                  loss.data_ptr(), B, H, W, nparts, 0 if l1part is None else L1_BLOCKS, float(l1), float(mse), float(ssim), s)
        return loss

    @staticmethod
    def backward(ctx, g):
        out, target = ctx.saved_tensors
        l1, mse, ssim, data_range = ctx.weights
        B, _, H, W = out.shape
        grad = torch.empty_like(out)
        gs = g.detach().contiguous().float().reshape(1)
        _lib.call("tup_quality_loss_f32_bwd", out.data_ptr(), target.data_ptr(), _chk(gs, F32, None, "grad of the loss"), grad.data_ptr(),
                  B, H, W, l1, mse, ssim, data_range, _stream())
        return grad, None, None, None, None, None


def quality_loss(out: torch.Tensor, target: torch.Tensor, l1: float = 1.0, mse: float = 0.0, ssim: float = 0.0,
                 data_range: float = 1.0) -> torch.Tensor:
    """l1 * L1 + mse * MSE + ssim * (1 - SSIM) of a batch (module docstring).  Terms with weight 0 are not computed."""
    _check(out, target, l1, mse, ssim)          # before autograd records anything
    return _QualityLossFn.apply(out, target, float(l1), float(mse), float(ssim), float(data_range))


class QualityLoss:
    """``QualityLoss(l1=..., mse=..., ssim=...)(out, target)`` = quality_loss(out, target, ...): the callable
    ``harness.train_step(..., loss=)`` takes."""

    def __init__(self, l1: float = 1.0, mse: float = 0.0, ssim: float = 0.0, data_range: float = 1.0):
        if l1 == 0 and mse == 0 and ssim == 0:
            raise ValueError("QualityLoss: all of l1, mse and ssim are 0 -- there is nothing to minimise")
        self.l1, self.mse, self.ssim, self.data_range = float(l1), float(mse), float(ssim), float(data_range)

    def __call__(self, out, target):
        return quality_loss(out, target, self.l1, self.mse, self.ssim, self.data_range)

    def __repr__(self):
        return f"QualityLoss(l1={self.l1}, mse={self.mse}, ssim={self.ssim}, data_range={self.data_range})"
