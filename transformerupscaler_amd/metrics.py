"""Image-quality metrics on the GPU: SSIM, PSNR and MSE of an image pair in one kernel pass (csrc/metrics.hip).

The quantities are the reference's (inference.py:128-145: ``skimage.metrics.structural_similarity(..., data_range=1,
channel_axis=-1)`` and ``peak_signal_noise_ratio``; ab_test.py:96-124: ``nn.MSELoss``), with skimage's defaults: a 7x7 uniform
window, sample covariance (49/48), K1 = 0.01, K2 = 0.03, and the mean over the interior ``[3:H-3, 3:W-3]``.  Per-image SSIM is
the mean of the three channels' means.

Two input forms, both three-channel:

* fp32 planar ``[B][3][H][W]`` (model outputs, ToTensor targets); ``data_range`` defaults to 1.0;
* uint8 interleaved ``[B][H][W][3]`` (decoded frames); ``data_range`` defaults to 255, so ``ssim(u8)`` is the reference's
  ``img_as_float`` + ``data_range=1`` quantity.

A 3-D input is one image.  Results are float64 GPU tensors of shape ``[B]``; nothing here synchronises with the host.  There is
no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

import torch

from . import _lib
from .ops import _chk, _stream

F64 = torch.float64
STRIP_COLS = 250        # = SO of csrc/metrics.hip: columns a workgroup owns
SEG_ROWS = 96           # = SEG: rows a workgroup owns
WIN = 7


def _partials(H, W):
    return ((W - 6 + STRIP_COLS - 1) // STRIP_COLS) * ((H - 6 + SEG_ROWS - 1) // SEG_ROWS)


def _check_options(win_size, gaussian_weights):
    if win_size is not None and win_size != WIN:
        raise NotImplementedError(f"win_size={win_size}: only skimage's default 7x7 window is implemented")
    if gaussian_weights:
        raise NotImplementedError("gaussian_weights=True is not implemented (uniform window only)")


def _prepare(a, b):
    if a.dim() == 3:
        a = a.unsqueeze(0)
    if b.dim() == 3:
        b = b.unsqueeze(0)
    if a.dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"a: expected torch.float32 ([B][3][H][W]) or torch.uint8 ([B][H][W][3]), got {a.dtype}")
    if a.dim() != 4:
        raise ValueError(f"a: expected a 3-D or 4-D image tensor, got shape {tuple(a.shape)}")
    planar = a.dtype == torch.float32
    B, C, H, W = a.shape if planar else (a.shape[0], a.shape[3], a.shape[1], a.shape[2])
    if C != 3:
        raise ValueError(f"a: expected 3 channels ({'[B][3][H][W]' if planar else '[B][H][W][3]'}), got shape {tuple(a.shape)}")
    if H < WIN or W < WIN:
        raise ValueError(f"image of {H}x{W}: SSIM's 7x7 window needs H and W >= 7")
    _chk(a, a.dtype, None, "a")
    _chk(b, a.dtype, a.shape, "b")
    return a, b, planar, B, H, W


def quality(a: torch.Tensor, b: torch.Tensor, data_range=None, win_size=None, gaussian_weights=False) -> dict:
    """dict(mse=[B], psnr=[B], ssim=[B], ssim_channels=[B, 3]) of the pairs (a[i], b[i]), float64 on the GPU, one kernel pass.
    mse is in the input's units; psnr = 10 log10(data_range^2 / mse), +inf when mse == 0."""
    _check_options(win_size, gaussian_weights)
    a, b, planar, B, H, W = _prepare(a, b)
    if data_range is None:
        data_range = 1.0 if planar else 255.0
    nparts = _partials(H, W)
    work = torch.empty((B, 3, nparts, 2), dtype=F64, device=a.device)
    out = torch.empty((6, B), dtype=F64, device=a.device)
    s = _stream()
    _lib.call("tup_quality_f32_partial" if planar else "tup_quality_u8hwc_partial", a.data_ptr(), b.data_ptr(), work.data_ptr(),
              B, H, W, nparts, float(data_range), s)
    _lib.call("tup_quality_reduce", work.data_ptr(), out.data_ptr(), B, H, W, nparts, float(data_range), s)
    return {"mse": out[0], "psnr": out[1], "ssim": out[2], "ssim_channels": out[3:6].t()}


def ssim(a, b, data_range=None, win_size=None, gaussian_weights=False):
    """Mean SSIM per image, [B] float64 (skimage structural_similarity, channel_axis=-1)."""
    return quality(a, b, data_range, win_size, gaussian_weights)["ssim"]


def psnr(a, b, data_range=None):
    """PSNR per image in dB, [B] float64 (skimage peak_signal_noise_ratio); +inf for identical images."""
    return quality(a, b, data_range)["psnr"]


def mse(a, b):
    """Mean squared error per image in the input's units, [B] float64 (nn.MSELoss per image)."""
    return quality(a, b)["mse"]
