"""Drop-in plugin module: the reference's A/B baseline (reference models/BicubicInterpolation/model.py), a parameterless
``F.interpolate(x, size=res_out, mode='bicubic', align_corners=False)`` with no clamp, run on the bicubic kernel of
csrc/rt_kernels.hip (``tup_rt_bicubic_sum_fwd`` with ``clamp01 = 0`` and a 1x1 zero second operand, whose bicubic image is
exactly zero)."""
from typing import Tuple

import torch
import torch.nn as nn

from transformerupscaler_amd import ops

__all__ = ["TransformerModel"]


class TransformerModel(nn.Module):
    """Bicubic interpolation of the input (no parameters; ``load_state_dict({})`` is all a checkpoint can hold)."""

    def __init__(self):
        super(TransformerModel, self).__init__()

    def forward(self, x: torch.Tensor, res_out: Tuple[int, int] = (1080, 1920)) -> torch.Tensor:
        """x fp32 [B][3][H][W] on the GPU -> [B][3][res_out[0]][res_out[1]]."""
        B, C = x.shape[0], x.shape[1]
        zero = torch.zeros((B, C, 1, 1), dtype=x.dtype, device=x.device)
        return ops.rt_bicubic_sum(x, zero, (int(res_out[0]), int(res_out[1])), clamp=False)
