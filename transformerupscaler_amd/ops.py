"""Tensor-level wrappers over the C ABI (include/tupscale_hip.h).

Each wrapper validates device / dtype / shape / contiguity on the host (a kernel that faults
can take the whole GPU node down), allocates the output with torch (plumbing only) and launches
on the caller's current HIP stream.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import re
import struct
import zlib

import numpy as np
import torch

from . import _lib, resize_taps

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
_DTYPE_CODE = {BF16: 0, F32: 1}          # the a_dtype / p_dtype / q_dtype argument of the token-matrix entries


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_dev = torch.cuda.current_device


def _stream():
    """The current stream of the current device as the integer hipStream_t the C ABI takes.  (The raw accessor skips building a
    torch.cuda.Stream object per launch: the training step issues ~275 launches and its host time is within 10 % of its GPU time.)"""
    if _raw_stream is not None:
        return _raw_stream(_cur_dev())
    return torch.cuda.current_stream().cuda_stream


def _chk(t: torch.Tensor, dtype, shape=None, name="tensor"):
    # the common case falls through five cheap tests; the messages are built only on failure
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if shape is not None and t.shape != shape and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: the HIP path needs a GPU tensor (no CPU fallback)")
    if t.device.index != _cur_dev():
        # every launch goes to the CURRENT device's stream: a tensor of another device would be a wild pointer there
        raise RuntimeError(f"{name} lives on {t.device} but the current device is cuda:{torch.cuda.current_device()}; "
                           "call torch.cuda.set_device(...) (one process per GPU) before building / calling the model")
    return t.data_ptr()


def _opt(t, dtype, shape, name):
    return None if t is None else _chk(t, dtype, shape, name)


def _seed(seed):
    """A dropout seed as the unsigned 32-bit argument of the C ABI."""
    return int(seed) & 0xFFFFFFFF


# ---- device tables: every tap / band / plan table is built on the host by a pure function of resize_taps.py and uploaded once ----
_tables = {}


def _table(build, device, sizes):
    """build(*sizes) on `device`, memoised on (builder, device, sizes): the numpy arrays of the tuple it returns are uploaded, its
    plain integers pass through, None stays None."""
    key = (build, str(device), sizes)
    if key not in _tables:
        host = build(*sizes)
        _tables[key] = None if host is None else tuple(
            torch.from_numpy(np.ascontiguousarray(v)).to(device) if isinstance(v, np.ndarray) else v for v in host)
    return _tables[key]


def _taps_on(device, in_size, out_size):
    return _table(resize_taps.aa_taps, device, (in_size, out_size))


def _inv_taps_on(device, in_size, out_size):
    return _table(resize_taps.aa_inverse_ranges, device, (in_size, out_size))


def _bicubic_on(device, in_size, out_size):
    return _table(resize_taps.bicubic_taps, device, (in_size, out_size))


_PIL_COEFFS = {"bilinear": resize_taps.pil_bilinear_coeffs, "bicubic": resize_taps.pil_bicubic_coeffs}


def _pil_taps_on(device, in_size, out_size, resample="bilinear"):
    return _table(_PIL_COEFFS[resample], device, (in_size, out_size))


# ---- zero pool: the backward pass needs ~130 small zero-initialised fp32 buffers per step (atomically accumulated weight /
# bias gradients).  One torch.zeros of the whole lot + views replaces 130 fill launches.  The pool is a fresh allocation per
# backward pass and stays alive as long as any gradient view does, so there is no reuse hazard. ----
_zero_pool = None          # [tensor, next free offset (floats)]
_ZERO_POOL_FLOATS = 9 * 1024 * 1024


def zero_pool_begin(device):
    global _zero_pool
    if _ZERO_POOL_FLOATS > 0:
        _zero_pool = [torch.zeros((_ZERO_POOL_FLOATS,), dtype=F32, device=device), 0]


def zero_pool_end():
    global _zero_pool
    _zero_pool = None


def _zeros(shape, device):
    n = 1
    for d in shape:
        n *= int(d)
    zp = _zero_pool
    if zp is not None and zp[0].device == torch.device(device) and zp[1] + n <= zp[0].numel():
        off = zp[1]
        zp[1] = off + ((n + 63) // 64) * 64          # 256-byte aligned slices
        return zp[0][off:off + n].view(shape)
    return torch.zeros(shape, dtype=F32, device=device)


def conv1(x, wp, bias, relu=True, in_mask=None, out_mask=None):
    """planar fp32 [B][3][H][W] -> NHWC bf16 64 ch (conv1; also the input-gradient conv of the 64->3 convs)."""
    B, C, H, W = x.shape
    assert C == 3
    out = torch.empty((B, H, W, 64), dtype=BF16, device=x.device)
    _lib.call("tup_conv3x3_c3_fwd", _chk(x, F32, None, "x"), _chk(wp, BF16, (64, 32), "wp"),
              _opt(bias, F32, (64,), "bias"), _opt(in_mask, F32, x.shape, "in_mask"),
              _opt(out_mask, BF16, out.shape, "out_mask"), out.data_ptr(), B, H, W, int(relu), _stream())
    return out


def conv1_compact(x):
    """planar fp32 [B][3][H][W] -> the fused conv1 -> conv2's input: bf16 [B][8 ceil(H/8) + 4][32 ceil(W/32) + 4][4], the image at
    (+2, +2) inside a zero border, channel 3 = 0 (csrc/conv12_fused.hip)."""
    B, C, H, W = x.shape
    assert C == 3
    xc = torch.empty((B, (H + 7) // 8 * 8 + 4, (W + 31) // 32 * 32 + 4, 4), dtype=BF16, device=x.device)
    _lib.call("tup_conv1_compact_fwd", _chk(x, F32, None, "x"), xc.data_ptr(), B, H, W, _stream())
    return xc


def conv12_fused(xc, H, W, w1, b1, w2, b2):
    """ReLU(conv2(ReLU(conv1(x)))) from conv1_compact(x) without the conv1 map in HBM: NHWC bf16 [B][H][W][64], bit-identical to
    conv_c64(conv1(x, w1, b1), w2, b2, 1, relu=True) (csrc/conv12_fused.hip; inference only)."""
    B = xc.shape[0]
    _chk(xc, BF16, (B, (H + 7) // 8 * 8 + 4, (W + 31) // 32 * 32 + 4, 4), "xc")
    out = torch.empty((B, H, W, 64), dtype=BF16, device=xc.device)
    _lib.call("tup_conv12_fused_fwd", xc.data_ptr(), _chk(w1, BF16, (64, 32), "w1"), _chk(b1, F32, (64,), "b1"),
              _chk(w2, BF16, (1, 1, 9, 64, 64), "w2"), _chk(b2, F32, (1, 64), "b2"), out.data_ptr(), B, H, W, _stream())
    return out


def conv_c64(x, wp, bias, r=1, relu=False, add=None, mask=None, in_r=1, out=None):
    """NHWC bf16 conv 64*in_r^2 -> 64*r*r with fused PixelShuffle(r); returns [B][H*r][W*r][64] bf16.
    x is [B][H*in_r][W*in_r][64] (in_r > 1: channels read through PixelShuffle^-1)."""
    B, Hi, Wi, C = x.shape
    assert C == 64 and Hi % in_r == 0 and Wi % in_r == 0
    H, W = Hi // in_r, Wi // in_r
    nt = r * r
    if out is None:
        out = torch.empty((B, H * r, W * r, 64), dtype=BF16, device=x.device)
    else:
        _chk(out, BF16, (B, H * r, W * r, 64), "out")
    _lib.call("tup_conv3x3_c64_fwd", _chk(x, BF16, None, "x"), _chk(wp, BF16, (nt, in_r * in_r, 9, 64, 64), "wp"),
              _opt(bias, F32, (nt, 64), "bias"), _opt(add, BF16, out.shape, "add"), _opt(mask, BF16, out.shape, "mask"),
              out.data_ptr(), B, H, W, nt, r, 64, int(relu), 0, in_r, _stream())
    return out


def conv_c64_thin(x, wp, bias, cout, relu=False, out=None):
    """NHWC bf16 conv 64 -> cout (<=16); returns fp32 planar [B][cout][H][W]."""
    B, H, W, C = x.shape
    assert C == 64 and 1 <= cout <= 16
    if out is None:
        out = torch.empty((B, cout, H, W), dtype=F32, device=x.device)
    else:
        _chk(out, F32, (B, cout, H, W), "out")
    _lib.call("tup_conv3x3_c64_fwd", _chk(x, BF16, None, "x"), _chk(wp, BF16, (1, 1, 9, 16, 64), "wp"),
              _opt(bias, F32, (cout,), "bias"), None, None, out.data_ptr(), B, H, W, 1, 1, cout, int(relu), 1, 1, _stream())
    return out


def decoder_fused(x, w1, b1, wz, b2, finish=True):
    """decoder_conv1 (64->64, +bias, ReLU) + decoder_conv2 (64->3, +bias) without the 64-channel map in HBM:
    NHWC bf16 [B][H][W][64] -> fp32 planar [B][3][H][W] (csrc/decoder_fused.hip).
    finish=False: the finishing launch does not run; returns the unfinished pieces (part, seamv, cseam, b2) that
    tail_stream_r2(parts=...) adds up where it reads the plane."""
    B, H, W, C = x.shape
    assert C == 64
    out = torch.empty((B, 3, H, W), dtype=F32, device=x.device)
    seamv = torch.empty((B, 3, H, W), dtype=F32, device=x.device)
    cseam = torch.empty((B, H, (W + 31) // 32, 32), dtype=F32, device=x.device)
    if not finish:
        _chk(b2, F32, (3,), "b2")
        _lib.call("tup_decoder_fused_parts_fwd", _chk(x, BF16, None, "x"), _chk(w1, BF16, (1, 1, 9, 64, 64), "w1"),
                  _chk(b1, F32, (1, 64), "b1"), _chk(wz, BF16, (48, 64), "wz"), out.data_ptr(), seamv.data_ptr(), cseam.data_ptr(),
                  B, H, W, _stream())
        return out, seamv, cseam, b2
    _lib.call("tup_decoder_fused_fwd", _chk(x, BF16, None, "x"), _chk(w1, BF16, (1, 1, 9, 64, 64), "w1"), _chk(b1, F32, (1, 64), "b1"),
              _chk(wz, BF16, (48, 64), "wz"), _chk(b2, F32, (3,), "b2"), seamv.data_ptr(), cseam.data_ptr(), out.data_ptr(),
              B, H, W, _stream())
    return out


def branch_a_composed(x, wp, bias, wv, bv, r, relu=True):
    """Composed (last up-conv + PixelShuffle + up1_conv [+ReLU]) 5x5 conv: NHWC bf16 [B][H][W][64] -> fp32 [B][3][H*r][W*r]."""
    B, H, W, C = x.shape
    assert C == 64 and r in (2, 3, 6)
    rows, n = {2: 16, 3: 32, 6: 112}[r], 3 * r * r
    out = torch.empty((B, 3, H * r, W * r), dtype=F32, device=x.device)
    _lib.call("tup_conv5x5_c64_planar_fwd", _chk(x, BF16, None, "x"), _chk(wp, BF16, (1, 1, 25, rows, 64), "wp"),
              _chk(bias, F32, (n,), "bias"), _chk(wv, BF16, (9, n, 25, 64), "wv"), _chk(bv, F32, (9, n), "bv"),
              out.data_ptr(), B, H, W, r, int(relu), _stream())
    return out


def conv_planar(x, w28, bias, r=1, add=None, clamp=False):
    """clamp = "both" (training): returns (unclamped, clamped), written by the same kernel pass."""
    B, C, H, W = x.shape
    assert C == 3
    cout = 3 * r * r
    both = clamp == "both"
    shape = (B, 3, H * r, W * r)
    out = torch.empty(((2,) if both else ()) + shape, dtype=F32, device=x.device)
    _lib.call("tup_conv3x3_planar_fwd", _chk(x, F32, None, "x"), _chk(w28, F32, (cout, 28), "w28"),
              _opt(bias, F32, (cout,), "bias"), _opt(add, F32, shape, "add"), out.data_ptr(),
              B, H, W, r, 2 if both else int(bool(clamp)), _stream())
    return (out[0], out[1]) if both else out


def resize_aa(x, size, clamp=False):
    """clamp = "both" (training): returns (unclamped, clamped), written by the same kernel pass."""
    B, C, Hi, Wi = x.shape
    Ho, Wo = size
    ylo, yn, yw, ky = _taps_on(x.device, Hi, Ho)
    xlo, xn, xw, kx = _taps_on(x.device, Wi, Wo)
    both = clamp == "both"
    out = torch.empty(((2,) if both else ()) + (B, C, Ho, Wo), dtype=F32, device=x.device)
    _lib.call("tup_resize_aa_fwd", _chk(x, F32, None, "x"), out.data_ptr(), ylo.data_ptr(), yn.data_ptr(),
              yw.data_ptr(), ky, xlo.data_ptr(), xn.data_ptr(), xw.data_ptr(), kx, B * C, Hi, Wi, Ho, Wo,
              2 if both else int(bool(clamp)), _stream())
    return (out[0], out[1]) if both else out


TAIL_TILE_H = 16          # = OT_H of csrc/tail_fused.hip


def tail_fused(x, wfu, bfu, wfc, bfc, ui, r, out_hw, clamp=True):
    """Last final_upscale stage + final_upscale_conv + "+ upscaled_input" + Resize(out_hw) + clamp in one kernel."""
    B, C, H, W = x.shape
    Hs, Ws = H * r, W * r
    Ho, Wo = out_hw
    ylo, yn, yw, ky, xlo, xn, xw, kx, eh, ew = _table(resize_taps.tail_fused_tables, x.device, (Hs, Ws, Ho, Wo, TAIL_TILE_H, 64))
    out = torch.empty((B, 3, Ho, Wo), dtype=F32, device=x.device)
    _lib.call("tup_tail_fused_fwd", _chk(x, F32, None, "x"), _chk(wfu, F32, (3 * r * r, 28), "wfu"), _chk(bfu, F32, (3 * r * r,), "bfu"),
              _chk(wfc, F32, (3, 28), "wfc"), _chk(bfc, F32, (3,), "bfc"), _chk(ui, F32, (B, 3, Hs, Ws), "ui"), out.data_ptr(),
              ylo.data_ptr(), yn.data_ptr(), yw.data_ptr(), ky, xlo.data_ptr(), xn.data_ptr(), xw.data_ptr(), kx,
              B, H, W, r, Ho, Wo, eh, ew, int(clamp), _stream())
    return out


TAIL_STREAM_WAVES_PER_SIMD = 3      # csrc/tail_stream.hip: 127 registers (148 on unfinished decoder pieces), 51 KB of LDS per four-wave workgroup


def _tail_stream_plan(device, B, H, W, Ho, Wo):
    """resize_taps.tail_stream_plan on `device`, sized to fill the chip once at the kernel's occupancy.  None: the Resize runs as
    its own kernel."""
    return _table(resize_taps.tail_stream_plan, device, (B, H, W, Ho, Wo, 256 * 4 * TAIL_STREAM_WAVES_PER_SIMD))


def tail_stream_fits(B, H, W, out_hw=None):
    """The streaming tail addresses its tensors with 32-bit byte offsets: tup_tail_stream_r2_fwd refuses B*12*H*W >= 2^29 elements
    (the HR map of the last stage), tup_tail_stream_r2_resize_fwd also B*3*Ho*Wo >= 2^29 (csrc/tail_stream.hip).  Batches beyond that
    (4x of 720p from B = 13, 540p -> 2160p from B = 22) take the tiled tail (tail_fused), which has no such limit."""
    if B * 12 * H * W >= 1 << 29:
        return False
    if out_hw is not None and tuple(out_hw) != (2 * H, 2 * W) and B * 3 * int(out_hw[0]) * int(out_hw[1]) >= 1 << 29:
        return False
    return True


def tail_stream_r2(x, wfu_t, bfu, wfc_t, bfc, ui, clamp=True, out_hw=None, parts=None):
    """Last final_upscale stage (r = 2) + final_upscale_conv + "+ upscaled_input" [+ antialiased Resize to out_hw] [+ clamp],
    streaming kernel.  Returns None when out_hw needs a Resize whose tap tables the fused kernel does not take (> 4 taps).
    parts = decoder_fused(..., finish=False): the kernel forms x from the unfinished pieces as it reads them (x may be None); the
    result equals that of the finished plane bit for bit."""
    if parts is not None:
        part, seamv, cseam, b2 = parts
        B, C, H, W = part.shape
        dev, tiles_x = part.device, (W + 31) // 32
        head = (_chk(part, F32, (B, 3, H, W), "part"), _chk(seamv, F32, (B, 3, H, W), "seamv"),
                _chk(cseam, F32, (B, H, tiles_x, 32), "cseam"), _chk(b2, F32, (3,), "b2"), tiles_x)
        suffix = "_parts_fwd"
    else:
        B, C, H, W = x.shape
        dev = x.device
        head = (_chk(x, F32, (B, 3, H, W), "x"),)
        suffix = "_fwd"
    args = head + (_chk(wfu_t, F32, (27, 12), "wfu_t"), _chk(bfu, F32, (12,), "bfu"),
                   _chk(wfc_t, F32, (27, 4), "wfc_t"), _chk(bfc, F32, (3,), "bfc"), _chk(ui, F32, (B, 3, 2 * H, 2 * W), "ui"))
    if out_hw is None or tuple(out_hw) == (2 * H, 2 * W):
        out = torch.empty((B, 3, 2 * H, 2 * W), dtype=F32, device=dev)
        _lib.call("tup_tail_stream_r2" + suffix, *args, out.data_ptr(), B, H, W, int(clamp), _stream())
        return out
    Ho, Wo = int(out_hw[0]), int(out_hw[1])
    plan = _tail_stream_plan(dev, B, H, W, Ho, Wo)
    if plan is None:
        return None
    ylo, yn, yw, ky, xlo, xn, xw, kx, oxb, oyb, sc, bh, ext = plan
    out = torch.empty((B, 3, Ho, Wo), dtype=F32, device=dev)
    _lib.call("tup_tail_stream_r2_resize" + suffix, *args, out.data_ptr(), ylo.data_ptr(), yn.data_ptr(), yw.data_ptr(), ky,
              xlo.data_ptr(), xn.data_ptr(), xw.data_ptr(), kx, oxb.data_ptr(), oyb.data_ptr(), B, H, W, Ho, Wo, sc, bh, ext,
              int(clamp), _stream())
    return out


def clamp01(x):
    out = torch.empty_like(x)
    _lib.call("tup_clamp01_fwd", _chk(x, F32, None, "x"), out.data_ptr(), x.numel(), _stream())
    return out


# LayerNorm rows are 192 wide (FastTransformer) or 128 wide (the two other models); each width has its own C entries
_LAYERNORM = {192: ("tup_layernorm_fwd", "tup_layernorm_bwd"), 128: ("tup_layernorm128_fwd", "tup_layernorm128_bwd")}


def _layernorm_entries(D):
    if D not in _LAYERNORM:
        raise ValueError(f"LayerNorm rows must be 192 or 128 wide, got {D}")
    return _LAYERNORM[D]


def layernorm(x, gamma, beta, save_stats=False):
    M, D = x.shape
    entry = _layernorm_entries(D)[0]
    y = torch.empty((M, D), dtype=BF16, device=x.device)
    mean = rstd = None
    if save_stats:
        mean = torch.empty((M,), dtype=F32, device=x.device)
        rstd = torch.empty((M,), dtype=F32, device=x.device)
    _lib.call(entry, _chk(x, F32, None, "x"), _chk(gamma, F32, (D,), "gamma"), _chk(beta, F32, (D,), "beta"), y.data_ptr(),
              None if mean is None else mean.data_ptr(), None if rstd is None else rstd.data_ptr(), M, _stream())
    return (y, mean, rstd) if save_stats else y


# Window attention has 12 heads (FastTransformer, width 192) or 8 (WindowTransformer, width 128).  Per head count the C entries:
# forward, backward, bias expansion in the forward / the backward kernel's layout, table-gradient reduce -- and the `heads`
# argument that only the general entries take
_WINDOW_ATTN = {
    12: ("tup_window_attn_fwd", "tup_window_attn_bwd", "tup_relpos_bias_expand", "tup_relpos_bias_expand_n",
         "tup_relpos_bias_reduce", ()),
    8: ("tup_window_attn_fwd_h", "tup_window_attn_bwd_h", "tup_relpos_bias_expand_h", "tup_relpos_bias_expand_n_h",
        "tup_relpos_bias_reduce_h", (8,)),
}


def _window_attn_entries(heads):
    if heads not in _WINDOW_ATTN:
        raise ValueError(f"window attention takes 12 or 8 heads of 16 channels, got {heads}")
    return _WINDOW_ATTN[heads]


def _relpos_expand(table, which):
    heads = table.shape[1]
    entries = _window_attn_entries(heads)
    frag = torch.empty((heads, 4, 4, 64, 4), dtype=F32, device=table.device)
    _lib.call(entries[which], _chk(table, F32, (225, heads), "table"), frag.data_ptr(), *entries[5], _stream())
    return frag


def relpos_bias_expand(table):
    """Relative-position table fp32 [225][heads] -> the dense bias in the forward kernel's fragment layout."""
    return _relpos_expand(table, 2)


def relpos_bias_expand_n(table):
    """... in the backward kernel's fragment layout."""
    return _relpos_expand(table, 3)


def window_attn(qkv, bias_frag, drop_p=0.0, drop_seed=0, save_lse=False):
    """WindowAttention core on bf16 [M][48 heads].  save_lse (training): also returns the fp32 [M // 64][heads][64] log-sum-exp of
    every score row, which window_attn_bwd rebuilds the probabilities from."""
    M, D = qkv.shape
    heads = D // 48
    fwd, _, _, _, _, hargs = _window_attn_entries(heads)
    if D != 48 * heads or M % 64 != 0:
        raise ValueError(f"qkv: expected [64 windows][48 heads], got {tuple(qkv.shape)}")
    out = torch.empty((M, 16 * heads), dtype=BF16, device=qkv.device)
    lse = torch.empty((M // 64, heads, 64), dtype=F32, device=qkv.device) if save_lse else None
    _lib.call(fwd, _chk(qkv, BF16, None, "qkv"), _chk(bias_frag, F32, (heads, 4, 4, 64, 4), "bias"),
              out.data_ptr(), lse.data_ptr() if save_lse else None, M // 64, *hargs, float(drop_p), _seed(drop_seed), _stream())
    return (out, lse) if save_lse else out


def gemm_tokens(a, wt, bias, epilogue, res=None, out=None, aux=None, drop_p=0.0, drop_seed=0):
    """epilogue 'bf16' | 'gelu' (aux, if given, receives the bf16 pre-activation) | 'res' (fp32 out = a@wt^T + bias
    + res) | 'gelu_bwd' (bf16 out = (a@wt^T) * gelu'(aux))."""
    M, K = a.shape
    N = wt.shape[0]
    assert tuple(wt.shape) == (N, K) and N % 64 == 0 and K % 64 == 0
    epi = {"bf16": 0, "gelu": 1, "res": 2, "gelu_bwd": 3}[epilogue]
    resp = auxp = None
    if epi == 2:
        if out is None:
            out = torch.empty((M, N), dtype=F32, device=a.device)
        _chk(out, F32, (M, N), "out")
        resp = _chk(res, F32, (M, N), "res")
    else:
        out = torch.empty((M, N), dtype=BF16, device=a.device)
        if epi == 3 or (epi == 1 and aux is not None):
            auxp = _chk(aux, BF16, (M, N), "aux")
    _lib.call("tup_gemm_tokens_fwd", _chk(a, a.dtype, None, "a"), _DTYPE_CODE[a.dtype], K, _chk(wt, BF16, None, "wt"),
              _opt(bias, F32, (N,), "bias"), resp, auxp, out.data_ptr(), N, M, N, K, epi, float(drop_p),
              _seed(drop_seed), _stream())
    return out


def _pointer_table(blocks, operands, what):
    """(ctypes array of the blocks' device pointers, number of blocks, the tensors -- kept alive by the caller holding the tuple)
    for the multi-block kernels.  operands: per tensor of a block (dtype, shape), or (dtype, element count) for a flat packed one."""
    if not 1 <= len(blocks) <= 8:
        raise ValueError("1..8 blocks per launch")
    ptrs = []
    for blk in blocks:
        assert len(blk) == len(operands)
        for i, (t, (dt, sh)) in enumerate(zip(blk, operands)):
            if isinstance(sh, int):
                if t.numel() != sh:
                    raise ValueError(f"{what} operand {i}: {t.numel()} elements, expected {sh}")
                sh = None
            ptrs.append(_chk(t, dt, sh, f"{what} operand {i}"))
    return ((ctypes.c_void_p * len(ptrs))(*ptrs), len(blocks), [list(b) for b in blocks])


def block_table(blocks):
    """Pointer table for tup_fused_blocks32_fwd: `blocks` = per block the 9 tensors (wh, bh, bias_frag, wproj, bproj, w1, b1, w2, b2)
    with norm1 / norm2 folded into attn.qkv / mlp.0 (packing.fold_layernorm), w1 / b1 = mlp.0 / 4 (packing.pack_fc1_fused_q),
    w2 = 4 W2 in fp16 (packing.pack_fc2_h4), validated here."""
    return _pointer_table(blocks, [(BF16, (12, 64, 192)), (F32, (12, 48)), (F32, (12, 4, 4, 64, 4)), (BF16, (192, 192)), (F32, (192,)),
                                   (BF16, (768, 192)), (F32, (768,)), (F16, (192, 768)), (F32, (192,))], "block")


def fused_blocks32(x, table):
    """In place: the table's consecutive WindowTransformerBlocks (attention half + MLP half each) in one launch of the 16x16x32
    whole-block kernel (csrc/fused_attn.hip): two waves per window, one window per workgroup at <= 512 windows."""
    M = x.shape[0]
    assert M % 64 == 0
    arr, nblk, _keep = table
    _lib.call("tup_fused_blocks32_fwd", _chk(x, F32, (M, 192), "x"), arr, nblk, M // 64, _stream())
    return x


def fused_block(x, *row):
    """In place: one whole WindowTransformerBlock, the one-block form of fused_blocks32 (`row` = one row of block_table)."""
    return fused_blocks32(x, block_table([row]))


def clock_probe():
    """Two device int64 [2]: (shader cycles, 100 MHz ticks) of the stream position of the call; see bench.py `sustained`."""
    out = torch.zeros(2, dtype=torch.int64, device=torch.device("cuda", _cur_dev()))
    _lib.call("tup_clock_probe", out.data_ptr(), _stream())
    return out


def stream_table(blocks):
    """Pointer table for tup_blocks_stream_fwd: per block the 7 tensors of packing.pack_stream_block (wqk, wv, wproj, w1, w2, tab,
    sbias), validated here."""
    return _pointer_table(blocks, [(BF16, 12 * 6144), (BF16, 6 * 6144), (BF16, 6 * 6144), (BF16, 24 * 6144), (F16, 24 * 6144),
                                   (F32, 1536), (F32, 12 * 2 * 2 * 64 * 16)], "stream block")


def blocks_stream(x, table, out_bf16=False):
    """The table's consecutive WindowTransformerBlocks in one launch of the streamed 32x32x16 kernel (csrc/block_stream.hip).
    out_bf16=False: in place, returns x.  out_bf16=True: returns the result as a NEW bf16 [M][192] tensor (round to nearest even of
    the same values) and leaves x holding the kernel's parked intermediate -- for patch_unembed, whose GEMM rounds its operand to
    bf16 anyway and then reads half the bytes."""
    M = x.shape[0]
    assert M % 64 == 0
    arr, nblk, _keep = table
    out = torch.empty((M, 192), dtype=BF16, device=x.device) if out_bf16 else None
    _lib.call("tup_blocks_stream_fwd", _chk(x, F32, (M, 192), "x"), out.data_ptr() if out_bf16 else None, arr, nblk, M // 64, _stream())
    return out if out_bf16 else x


def window_geometry(H, W):
    ht, wt = (H + 7) // 8, (W + 7) // 8
    nwy, nwx = (ht + 7) // 8, (wt + 7) // 8
    return ht, wt, nwy, nwx


def patch_embed(feat, wt, bias):
    B, H, W, C = feat.shape
    assert C == 64
    if (8 - H % 8) % 8 >= H or (8 - W % 8) % 8 >= W:
        raise RuntimeError("reflect padding needs pad < dim")     # same rule as F.pad(mode='reflect')
    _, _, nwy, nwx = window_geometry(H, W)
    x = torch.empty((B * nwy * nwx * 64, 192), dtype=F32, device=feat.device)
    _lib.call("tup_patch_embed_fwd", _chk(feat, BF16, None, "feat"), _chk(wt, BF16, (192, 4096), "wt"),
              _chk(bias, F32, (192,), "bias"), x.data_ptr(), B, H, W, _stream())
    return x


def patch_unembed(x, wt, bias, skip):
    B, H, W, C = skip.shape
    _, _, nwy, nwx = window_geometry(H, W)
    out = torch.empty_like(skip)
    x16 = x.dtype == BF16            # the streamed block kernel's bf16 output (ops.blocks_stream(out_bf16=True))
    _lib.call("tup_patch_unembed_fwd", _chk(x, BF16 if x16 else F32, (B * nwy * nwx * 64, 192), "x"), int(x16), _chk(wt, BF16, (4096, 192), "wt"),
              _chk(bias, F32, (64,), "bias"), _chk(skip, BF16, None, "skip"), out.data_ptr(), B, H, W, _stream())
    return out


# ------------------------------------------------------------------------------------------------
# backward wrappers
# ------------------------------------------------------------------------------------------------
def _gemm_wgrad(p, q, out, want_bias):
    M, NI = p.shape
    NJ = q.shape[1]
    assert q.shape[0] == M and NI % 64 == 0 and NJ % 64 == 0
    if out is None:
        out = _zeros((NI, NJ), p.device)
    # (out and db are neighbours in the zero pool: the deterministic entry then adds weight and bias slices in one reduce launch)
    db = _zeros((NI,), p.device) if want_bias else None
    head = (_chk(p, p.dtype, None, "p"), _DTYPE_CODE[p.dtype], NI, _chk(q, q.dtype, None, "q"), _DTYPE_CODE[q.dtype], NJ,
            _chk(out, F32, (NI, NJ), "out"), NJ)
    slab = _det_slab(0, M, NI, NJ, p.device)
    if want_bias or slab is not None:
        # tup_gemm_wgrad has no twin of its own: its deterministic form is the bias twin with a null bias pointer
        _reduce("tup_gemm_wgrad_bias", slab, *head, None if db is None else db.data_ptr(), M, NI, NJ)
    else:
        _lib.call("tup_gemm_wgrad", *head, M, NI, NJ, _stream())
    return out, db


def gemm_wgrad(p, q, out=None):
    """out[NI][NJ] fp32 (+)= p^T q; p [M][NI], q [M][NJ] (bf16 or fp32)."""
    return _gemm_wgrad(p, q, out, False)[0]


def gemm_wgrad_bias(p, q):
    """(dW [NI][NJ], db [NI]) = (p^T q, column sums of p): weight and bias gradient of a Linear layer in one pass over p."""
    return _gemm_wgrad(p, q, None, True)


PATCH_WGRAD_WIDE = True          # A/B switch: the wide-tile kernel (tup_patch_wgrad_bf16) for the two patch weights


def patch_wgrad(p, fmap, reflect):
    B, H, W, C = fmap.shape
    _, _, nwy, nwx = window_geometry(H, W)
    out = _zeros((192, 4096), p.device)
    M = B * nwy * nwx * 64
    pp = _chk(p, F32, (M, 192), "p")
    wide = PATCH_WGRAD_WIDE and B * H * W * 128 < 2 ** 31
    if wide:
        # bf16 token rows (the rounding the fp32 entry applies on load): the wide kernel fetches its operands by DMA
        pb = p.to(BF16)
        pp = pb.data_ptr()
    _reduce("tup_patch_wgrad_bf16" if wide else "tup_patch_wgrad", _det_slab(int(wide), M, 192, 4096, p.device),
            pp, _chk(fmap, BF16, None, "map"), out.data_ptr(), B, H, W, int(reflect))
    return out


def colsum(g, out=None, rowmask=None):
    M, N = g.shape
    if out is None:
        out = _zeros((N,), g.device)
    _reduce("tup_colsum", _det_slab(2, M, N, 0, g.device), _chk(g, g.dtype, None, "g"), _DTYPE_CODE[g.dtype], N,
            _chk(out, F32, (N,), "out"), M, N, _opt(rowmask, torch.uint8, (M,), "rowmask"))
    return out


def layernorm_bwd(gy, x, mean, rstd, gamma, gres=None, drop=None):
    """drop = (p, seed): also returns dx * dropout mask / (1 - p) as bf16 (dropout_bwd of dx, fused): (dx, dgamma, dbeta, gdrop)."""
    M, D = x.shape
    entry = _layernorm_entries(D)[1]
    dx = torch.empty((M, D), dtype=F32, device=x.device)
    dg = _zeros((D,), x.device)
    db = _zeros((D,), x.device)
    gd = torch.empty((M, D), dtype=BF16, device=x.device) if drop else None
    _reduce(entry, _det_slab(3, M, D, 0, x.device), _chk(gy, BF16, (M, D), "gy"), _chk(x, F32, (M, D), "x"),
            _chk(mean, F32, (M,), "mean"), _chk(rstd, F32, (M,), "rstd"), _chk(gamma, F32, (D,), "gamma"),
            _opt(gres, F32, (M, D), "gres"), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), M, gd.data_ptr() if drop else None,
            float(drop[0]) if drop else 0.0, _seed(drop[1]) if drop else 0)
    return (dx, dg, db, gd) if drop else (dx, dg, db)


def dropout_bwd(g, drop_p, drop_seed):
    """bf16 [M][192] = fp32 g * mask / (1 - p) for the site keyed by drop_seed."""
    out = torch.empty(g.shape, dtype=BF16, device=g.device)
    _lib.call("tup_dropout_bwd", _chk(g, F32, None, "g"), out.data_ptr(), g.numel(), float(drop_p), _seed(drop_seed), _stream())
    return out


def _attn_bwd_scratch(nwin, heads):
    """Floats of scratch the attention backward needs (tup_window_attn_bwd_scratch returns the count, not an error code)."""
    fn = _lib.load().tup_window_attn_bwd_scratch
    return int(fn(int(nwin), int(heads)))


def window_attn_bwd(qkv, gout, att, lse, bias_n, drop_p=0.0, drop_seed=0):
    """att, lse: what window_attn(..., save_lse=True) returned.  Returns (gqkv bf16 [M][48 heads], dtable fp32 [225][heads])."""
    M, D = qkv.shape
    heads = D // 48
    _, bwd, _, _, reduce, hargs = _window_attn_entries(heads)
    if M % 64 != 0:
        raise ValueError(f"qkv: expected [64 windows][48 heads], got {tuple(qkv.shape)}")
    gqkv = torch.empty((M, 48 * heads), dtype=BF16, device=qkv.device)
    dbias = torch.empty((heads, 4, 4, 64, 4), dtype=F32, device=qkv.device)
    scratch = torch.empty(_attn_bwd_scratch(M // 64, heads), dtype=F32, device=qkv.device)
    _lib.call(bwd, _chk(qkv, BF16, (M, 48 * heads), "qkv"), _chk(gout, BF16, (M, 16 * heads), "gout"),
              _chk(att, BF16, (M, 16 * heads), "att"), _chk(lse, F32, (M // 64, heads, 64), "lse"),
              _chk(bias_n, F32, (heads, 4, 4, 64, 4), "bias_n"), gqkv.data_ptr(), dbias.data_ptr(), scratch.data_ptr(), M // 64,
              *hargs, float(drop_p), _seed(drop_seed), _stream())
    dtable = torch.empty((225, heads), dtype=F32, device=qkv.device)
    _lib.call(reduce, dbias.data_ptr(), dtable.data_ptr(), *hargs, _stream())
    return gqkv, dtable


def patch_unembed_bwd(gmap, wt):
    B, H, W, C = gmap.shape
    _, _, nwy, nwx = window_geometry(H, W)
    gx = torch.empty((B * nwy * nwx * 64, 192), dtype=F32, device=gmap.device)
    _lib.call("tup_patch_unembed_bwd", _chk(gmap, BF16, None, "gmap"), _chk(wt, BF16, (192, 4096), "wt"),
              gx.data_ptr(), B, H, W, _stream())
    return gx


def patch_embed_bwd(gx, wt, B, H, W):
    ht, wt_, nwy, nwx = window_geometry(H, W)
    gmap = torch.empty((B, ht * 8, wt_ * 8, 64), dtype=BF16, device=gx.device)
    _lib.call("tup_patch_embed_bwd", _chk(gx, F32, (B * nwy * nwx * 64, 192), "gx"), _chk(wt, BF16, (4096, 192), "wt"),
              gmap.data_ptr(), B, H, W, _stream())
    return gmap


def patch_embed_bwd_merge(gx, wt, add1, add2, relu_src, want_add1_colsum=False):
    """patch_embed's input gradient + the gradient merge at `feat` (feat_grad_combine) in one kernel; H, W multiples of 8.
    want_add1_colsum: also returns the fp32 [64] column sums of add1 (colsum(add1.view(-1, 64)) for free)."""
    B, H, W, C = relu_src.shape
    assert C == 64 and H % 8 == 0 and W % 8 == 0
    _, _, nwy, nwx = window_geometry(H, W)
    out = torch.empty_like(relu_src)
    cs = _zeros((16, 64), relu_src.device) if want_add1_colsum else None
    _lib.call("tup_patch_embed_bwd_merge", _chk(gx, F32, (B * nwy * nwx * 64, 192), "gx"), _chk(wt, BF16, (4096, 192), "wt"),
              _chk(add1, BF16, relu_src.shape, "add1"), _opt(add2, BF16, relu_src.shape, "add2"), _chk(relu_src, BF16, None, "relu_src"),
              out.data_ptr(), cs.data_ptr() if want_add1_colsum else None, B, H, W, _stream())
    return (out, cs.sum(0)) if want_add1_colsum else out


# ---- deterministic mode: every order-dependent reduction of the three plugins' backward has a *_det form without float atomics
# (a slab of per-work-item partial sums, added in a fixed order: the weight-gradient convs below, the weight-gradient GEMMs, the
# column sums and the LayerNorm backward above) or is routed around (the composed branch A and the patch_unembed bias sums riding
# in patch_embed_bwd_merge have no such form: autograd.py takes the explicit stage convs and ops.colsum instead).  With the
# switch on, a training step is bitwise reproducible from run to run (INTEGRATION.md states the guarantee).  The switch is
# explicit: it does not follow torch.use_deterministic_algorithms.  Set it BEFORE the forward of a step: the branch-A route is
# chosen in forward_train and the backward follows the forward that produced its saved state. ----
deterministic = False            # True routes the reductions of the backward to their deterministic forms


def deterministic_enabled():
    """Whether the wrappers take the deterministic forms now (read at call time)."""
    return bool(deterministic)


@contextlib.contextmanager
def deterministic_mode(enabled=True):
    """Sets ops.deterministic for the duration of the block (forward AND backward of the steps inside it) and restores the
    previous value afterwards, also when the block raises."""
    global deterministic
    previous = deterministic
    deterministic = bool(enabled)
    try:
        yield
    finally:
        deterministic = previous


def wgrad_slab_floats(kind, M, NI, NJ=0):
    """fp32 slab size of the deterministic token-path reductions (kind 0 = 64 x 64-tile GEMM, 1 = wide patch GEMM, 2 = column sums
    over NI columns, 3 = LayerNorm backward of NI-wide rows).  Host only (tup_wgrad_slab returns the count, not an error code)."""
    n = int(_lib.load().tup_wgrad_slab(int(kind), int(M), int(NI), int(NJ)))
    if n <= 0:
        raise ValueError(f"tup_wgrad_slab({kind}, {M}, {NI}, {NJ}): invalid request")
    return n


# The token-path slab: one per device and stream, grown to the largest request and reused: the kernels of a backward run in stream
# order, and a deterministic entry is done with its slab when its reduce launch has run.  (A slab per call would be ~40 allocations
# of up to 50 MB per step.)  Replacing a slab by a larger one while kernels that use the old one are still queued is safe only
# because the slab is allocated on, and used on, the same (current) stream: the caching allocator hands the old block out again in
# stream order.  The cache never shrinks; release_det_slabs() returns the memory (call it also before destroying a side stream that
# ran deterministic steps, so that a later stream with a recycled handle does not inherit its slab).
_det_slabs = {}


def _det_slab(kind, M, NI, NJ, device):
    """The token-path slab for wgrad_slab_floats(kind, M, NI, NJ) in deterministic mode; None (and no size query) outside it."""
    if not deterministic_enabled():
        return None
    n = wgrad_slab_floats(kind, M, NI, NJ)
    key = (_cur_dev(), _stream())
    slab = _det_slabs.get(key)
    if slab is None or slab.numel() < n:
        _det_slabs.pop(key, None)
        slab = _det_slabs[key] = torch.empty((n,), dtype=F32, device=device)
    return slab


def release_det_slabs():
    _det_slabs.clear()


def conv_wgrad_slab_floats(kind, B, H, W, r=1):
    """fp32 slab size of the deterministic weight-gradient convs (kind 0 = c64 / c64 s2d, 1 = thin, 2 = planar with factor r).
    Host only (tup_conv_wgrad_slab returns the count, not an error code)."""
    n = int(_lib.load().tup_conv_wgrad_slab(int(kind), int(B), int(H), int(W), int(r)))
    if n <= 0:
        raise ValueError(f"tup_conv_wgrad_slab({kind}, {B}, {H}, {W}, {r}): invalid shape")
    return n


def _slab(kind, B, H, W, device, r=1):
    """The slab of a weight-gradient conv in deterministic mode, a fresh allocation per wrapper call; None outside it."""
    if not deterministic_enabled():
        return None
    return torch.empty((conv_wgrad_slab_floats(kind, B, H, W, r),), dtype=F32, device=device)


def _reduce(entry, slab, *args):
    """Launches a reduction on the current stream: `entry`, which accumulates with float atomics, or, given a slab (what _det_slab
    / _slab return in deterministic mode), its twin `entry`_det, which takes the same arguments and the slab before the stream."""
    if slab is None:
        _lib.call(entry, *args, _stream())
    else:
        _lib.call(entry + "_det", *args, slab.data_ptr(), _stream())


def conv_c64_wgrad(x, gmap, gr=1):
    """-> (dwp fp32 [gr*gr][64][9][64] (sp, co, tap, ci), dbias fp32 [gr*gr][64])."""
    B, H, W, C = x.shape
    assert C == 64 and tuple(gmap.shape) == (B, H * gr, W * gr, 64)
    dwp = _zeros((gr * gr, 64, 9, 64), x.device)
    db = _zeros((gr * gr, 64), x.device)
    slab = _slab(0, B, H, W, x.device)
    for sp in range(gr * gr):
        _reduce("tup_conv3x3_c64_wgrad", slab, _chk(x, BF16, None, "x"), _chk(gmap, BF16, None, "gmap"), dwp[sp].data_ptr(),
                db[sp].data_ptr(), B, H, W, gr, sp)
    return dwp, db


def conv_thin_wgrad(x, gpl, want_bias):
    B, H, W, C = x.shape
    assert C == 64
    dwp = _zeros((3, 9, 64), x.device)
    db = _zeros((3,), x.device) if want_bias else None
    _reduce("tup_conv3x3_thin_wgrad", _slab(1, B, H, W, x.device), _chk(x, BF16, None, "x"), _chk(gpl, F32, (B, 3, H, W), "gpl"),
            dwp.data_ptr(), None if db is None else db.data_ptr(), B, H, W)
    return dwp, db


def conv1_wgrad(x, gmap):
    """Weight / bias gradient of conv1 (3 -> 64): x planar fp32 [B][3][H][W], gmap NHWC bf16 [B][H][W][64].
    dw[co][ci][tap] = sum_p g[p][co] x[p + tap - 1][ci] = sum_q x[q][ci] g[q - (tap - 1)][co]: the thin (cout = 3) MFMA weight-
    gradient kernel with the roles of the two maps swapped and the taps flipped, plus a column sum for the bias."""
    B, C, H, W = x.shape
    assert C == 3
    dwp, _ = conv_thin_wgrad(gmap, x, False)                     # [ci][tap'][co], tap' = 8 - tap
    dw = dwp.flip(1).permute(2, 0, 1).reshape(64, 3, 3, 3)
    db = colsum(gmap.view(-1, 64))
    return dw, db


def conv1_wgrad_direct(x, gmap):
    """The original VALU kernel (tup_conv3x3_c3_wgrad), kept for the kernel-level test."""
    B, C, H, W = x.shape
    assert C == 3
    dw = _zeros((64, 3, 3, 3), x.device)
    db = _zeros((64,), x.device)
    _lib.call("tup_conv3x3_c3_wgrad", _chk(x, F32, None, "x"), _chk(gmap, BF16, (B, H, W, 64), "gmap"), dw.data_ptr(),
              db.data_ptr(), B, H, W, _stream())
    return dw, db


def conv_planar_wgrad(x, gpl, r):
    B, C, H, W = x.shape
    cout = 3 * r * r
    dw = _zeros((cout, 3, 3, 3), x.device)
    db = _zeros((cout,), x.device)
    _reduce("tup_conv3x3_planar_wgrad", _slab(2, B, H, W, x.device, r), _chk(x, F32, None, "x"),
            _chk(gpl, F32, (B, 3, H * r, W * r), "gpl"), dw.data_ptr(), db.data_ptr(), B, H, W, r)
    return dw, db


def conv_planar_dgrad(gpl, w, r):
    B, C, Hr, Wr = gpl.shape
    H, W = Hr // r, Wr // r
    gx = torch.empty((B, 3, H, W), dtype=F32, device=gpl.device)
    _lib.call("tup_conv3x3_planar_dgrad", _chk(gpl, F32, None, "gpl"), _chk(w, F32, (3 * r * r, 3, 3, 3), "w"),
              gx.data_ptr(), B, H, W, r, _stream())
    return gx


def resize_aa_bwd(gout, in_hw, pre=None, l1_scale=None):
    """Backward of resize_aa (+clamp when `pre`, the pre-clamp output, is given).  l1_scale (device float[2] = {d loss / numel,
    plain}): `gout` is the L1 target and the loss gradient is formed inside the kernel (autograd.l1_loss(...,
    fuse_into_model_backward=True)); plain != 0: `pre` is the loss input itself (this Resize's output), no clamp in between."""
    B, C, Ho, Wo = gout.shape
    Hi, Wi = in_hw
    ylo, _, yw, ky = _taps_on(gout.device, Hi, Ho)
    xlo, _, xw, kx = _taps_on(gout.device, Wi, Wo)
    oy0, oyn = _inv_taps_on(gout.device, Hi, Ho)
    ox0, oxn = _inv_taps_on(gout.device, Wi, Wo)
    gin = torch.empty((B, C, Hi, Wi), dtype=F32, device=gout.device)
    _lib.call("tup_resize_aa_bwd", _chk(gout, F32, None, "gout"), _opt(pre, F32, gout.shape, "pre"), gin.data_ptr(),
              ylo.data_ptr(), yw.data_ptr(), ky, xlo.data_ptr(), xw.data_ptr(), kx, oy0.data_ptr(), oyn.data_ptr(),
              ox0.data_ptr(), oxn.data_ptr(), B * C, Hi, Wi, Ho, Wo, _opt(l1_scale, F32, (2,), "l1_scale"), _stream())
    return gin


def mask_bwd(gout, pre=None, relu_src=None, l1_scale=None):
    gin = torch.empty_like(gout)
    _lib.call("tup_mask_bwd", _chk(gout, F32, None, "gout"), _opt(pre, F32, gout.shape, "pre"),
              _opt(relu_src, F32, gout.shape, "relu_src"), gin.data_ptr(), gout.numel(), _opt(l1_scale, F32, (2,), "l1_scale"), _stream())
    return gin


def feat_grad_combine(a, b, gpe, feat):
    B, H, W, C = feat.shape
    hp, wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    out = torch.empty_like(feat)
    _lib.call("tup_feat_grad_combine", _chk(a, BF16, feat.shape, "a"), _opt(b, BF16, feat.shape, "b"),
              _chk(gpe, BF16, (B, hp, wp, 64), "gpe"), _chk(feat, BF16, None, "feat"), out.data_ptr(), B, H, W, _stream())
    return out


# ------------------------------------------------------------------------------------------------
# ResidualTransformer wrappers
# ------------------------------------------------------------------------------------------------
def rt_patch_embed(feat, wt, bias, pos):
    B, H, W, C = feat.shape
    T = (H // 8) * (W // 8)
    x = torch.empty((B * T, 128), dtype=F32, device=feat.device)
    _lib.call("tup_rt_patch_embed_fwd", _chk(feat, BF16, None, "feat"), _chk(wt, BF16, (128, 4096), "wt"), _chk(bias, F32, (128,), "bias"),
              _chk(pos, F32, (T, 128), "pos"), x.data_ptr(), B, H, W, _stream())
    return x


def rt_patch_unembed(x, wt, bias, skip):
    B, H, W, C = skip.shape
    out = torch.empty_like(skip)
    _lib.call("tup_rt_patch_unembed_fwd", _chk(x, F32, (B * (H // 8) * (W // 8), 128), "x"), _chk(wt, BF16, (4096, 128), "wt"),
              _chk(bias, F32, (64,), "bias"), _chk(skip, BF16, None, "skip"), out.data_ptr(), B, H, W, _stream())
    return out


def _rt_dropout_check(N, drop_p):
    # the attention-probability mask decides two neighbouring keys per hash and a lane holds four consecutive keys (csrc/common.h
    # drop_pair4): the kernels take dropout only on token counts that are multiples of 4 (the reference's 720 x 1280 input = 3600
    # tokens, models/ResidualTransformer/model.py:135-140); p is quantised to multiples of 1 / 65536
    if drop_p > 0.0 and N % 4 != 0:
        raise ValueError(f"ResidualTransformer attention dropout needs a token count that is a multiple of 4 (got N = {N}); "
                         "call .eval() or use an input whose token grid has a multiple of 4 tokens")


def rt_attention(qkv, B, N, save_lse=False, drop_p=0.0, drop_seed=0):
    _rt_dropout_check(N, drop_p)
    out = torch.empty((B * N, 128), dtype=BF16, device=qkv.device)
    lse = torch.empty((B, 8, N), dtype=F32, device=qkv.device) if save_lse else None
    _lib.call("tup_rt_attention_fwd", _chk(qkv, BF16, (B * N, 384), "qkv"), out.data_ptr(),
              None if lse is None else lse.data_ptr(), B, N, float(drop_p), _seed(drop_seed), _stream())
    return (out, lse) if save_lse else out


def rt_attention_bwd(qkv, out, gout, lse, B, N, drop_p=0.0, drop_seed=0):
    _rt_dropout_check(N, drop_p)
    gqkv = torch.empty((B * N, 384), dtype=BF16, device=qkv.device)
    work = torch.empty((B, 8, N), dtype=F32, device=qkv.device)
    _lib.call("tup_rt_attention_bwd", _chk(qkv, BF16, (B * N, 384), "qkv"), _chk(out, BF16, (B * N, 128), "out"),
              _chk(gout, BF16, (B * N, 128), "gout"), _chk(lse, F32, (B, 8, N), "lse"), work.data_ptr(), gqkv.data_ptr(), B, N,
              float(drop_p), _seed(drop_seed), _stream())
    return gqkv


def rt_patch_wgrad(p, fmap):
    """fp32 [128][4096] = p^T patches(fmap); p fp32 [B*T][128] (plain token grid), fmap NHWC bf16."""
    B, H, W, C = fmap.shape
    M = B * (H // 8) * (W // 8)
    out = _zeros((128, 4096), p.device)
    _reduce("tup_rt_patch_wgrad", _det_slab(0, M, 128, 4096, p.device), _chk(p, F32, (M, 128), "p"), _chk(fmap, BF16, None, "map"),
            out.data_ptr(), B, H, W)
    return out


def rt_patch_unembed_bwd(gmap, wd):
    """d tokens fp32 [B*T][128] of patch_unembed: the patch_embed GEMM with the transposed weight (no bias / pos)."""
    B, H, W, C = gmap.shape
    x = torch.empty((B * (H // 8) * (W // 8), 128), dtype=F32, device=gmap.device)
    _lib.call("tup_rt_patch_embed_fwd", _chk(gmap, BF16, None, "gmap"), _chk(wd, BF16, (128, 4096), "wd"), None, None,
              x.data_ptr(), B, H, W, _stream())
    return x


def rt_patch_embed_bwd(gx, wd, add):
    """d feat_down NHWC bf16 = add + scatter(gx wd^T): the patch_unembed GEMM with the transposed weight; `add` carries
    the gradient of the skip connection (model.py:153)."""
    B, H, W, C = add.shape
    out = torch.empty_like(add)
    _lib.call("tup_rt_patch_unembed_fwd", _chk(gx, F32, (B * (H // 8) * (W // 8), 128), "gx"), _chk(wd, BF16, (4096, 128), "wd"),
              None, _chk(add, BF16, None, "add"), out.data_ptr(), B, H, W, _stream())
    return out


def conv_c64_wgrad_s2d(x, gmap, xr):
    """Stride-xr conv weight gradient: fp32 [xr*xr][64 co][9][64 ci] block-tap gradients + bias gradient [64]."""
    B, H, W, C = gmap.shape
    assert tuple(x.shape) == (B, H * xr, W * xr, 64)
    dwp = _zeros((xr * xr, 64, 9, 64), x.device)
    db = _zeros((64,), x.device)
    slab = _slab(0, B, H, W, x.device)
    for sp in range(xr * xr):
        _reduce("tup_conv3x3_c64_wgrad_s2d", slab, _chk(x, BF16, None, "x"), _chk(gmap, BF16, None, "gmap"), dwp[sp].data_ptr(),
                db.data_ptr() if sp == 0 else None, B, H, W, xr, sp)
    return dwp, db


bicubic_bwd_banded = True        # A/B attribute: per-source-row gather of the row pass


def rt_bicubic_bwd(gout, out, in_hw, l1_scale=None):
    """Gradient of clamp(bicubic(src -> size) + ...) w.r.t. a planar fp32 source of size in_hw; `out` = the saved
    forward output (the clamp gate) or None.  l1_scale (fp32 device scalar): `gout` is then the TARGET of an L1 loss on `out`
    and the upstream gradient sign(out - target) * l1_scale is formed inside the kernel."""
    B, C, Ho, Wo = gout.shape
    Ha, Wa = in_hw
    dev = gout.device
    ga = torch.empty((B, C, Ha, Wa), dtype=F32, device=dev)
    tmp = torch.empty((B, C, Ha, Wo), dtype=F32, device=dev)
    # (no column tables: a 256-column block's stretch exceeds the kernel's LDS tile)
    cols = _table(resize_taps.bicubic_cols, dev, (Wa, Wo)) if bicubic_bwd_banded else None
    if cols is not None:
        r0, bn, bw, nr_max = _table(resize_taps.bicubic_bands, dev, (Ha, Ho))
        xoT, xwT, kmax, c0, cn = cols
        _lib.call("tup_rt_bicubic_bwd_banded", _chk(gout, F32, None, "gout"), _opt(out, F32, (B, C, Ho, Wo), "out"), ga.data_ptr(),
                  tmp.data_ptr(), r0.data_ptr(), bn.data_ptr(), bw.data_ptr(), nr_max, xoT.data_ptr(), xwT.data_ptr(), kmax,
                  c0.data_ptr(), cn.data_ptr(), B * C, Ha, Wa, Ho, Wo,
                  None if l1_scale is None else _chk(l1_scale, F32, None, "l1_scale"), _stream())
        return ga
    if l1_scale is not None:
        raise RuntimeError("the fused L1 form of rt_bicubic_bwd needs the banded kernels (ratio too large or TUP_BICUBIC_BWD_GATHER set)")
    xs, xo, xw = _table(resize_taps.bicubic_taps_transposed, dev, (Wa, Wo))
    ys, yo, yw = _table(resize_taps.bicubic_taps_transposed, dev, (Ha, Ho))
    _lib.call("tup_rt_bicubic_bwd", _chk(gout, F32, None, "gout"), _opt(out, F32, (B, C, Ho, Wo), "out"), ga.data_ptr(), tmp.data_ptr(),
              ys.data_ptr(), yo.data_ptr(), yw.data_ptr(), xs.data_ptr(), xo.data_ptr(), xw.data_ptr(), B * C, Ha, Wa, Ho, Wo, _stream())
    return ga


def rt_bicubic_sum(a, b, size, clamp=True):
    """clamp(bicubic(a -> size) + bicubic(b -> size)) for planar fp32 [B][3][H][W] tensors."""
    B, C, Ha, Wa = a.shape
    _, _, Hb, Wb = b.shape
    Ho, Wo = size
    ayi, ayw = _bicubic_on(a.device, Ha, Ho); axi, axw = _bicubic_on(a.device, Wa, Wo)
    byi, byw = _bicubic_on(a.device, Hb, Ho); bxi, bxw = _bicubic_on(a.device, Wb, Wo)
    out = torch.empty((B, C, Ho, Wo), dtype=F32, device=a.device)
    _lib.call("tup_rt_bicubic_sum_fwd", _chk(a, F32, None, "a"), _chk(b, F32, (B, C, Hb, Wb), "b"), out.data_ptr(),
              ayi.data_ptr(), ayw.data_ptr(), axi.data_ptr(), axw.data_ptr(), byi.data_ptr(), byw.data_ptr(),
              bxi.data_ptr(), bxw.data_ptr(), B * C, Ha, Wa, Hb, Wb, Ho, Wo, int(clamp), _stream())
    return out


# ---- frame pre/post-processing ----
def frames_to_tensor(frames_u8, bgr=False):
    """uint8 [B][H][W][3] (or [H][W][3]) on the GPU -> fp32 [B][3][H][W] in [0, 1] (ToTensor); bgr=True for BGR frames."""
    if frames_u8.dim() == 3:
        frames_u8 = frames_u8.unsqueeze(0)
    B, H, W, C = frames_u8.shape
    assert C == 3
    out = torch.empty((B, 3, H, W), dtype=F32, device=frames_u8.device)
    _lib.call("tup_u8hwc_to_f32chw", _chk(frames_u8, torch.uint8, None, "frames"), out.data_ptr(), B, H, W, int(bgr), _stream())
    return out


def tensor_to_frames(x, bgr=False):
    """fp32 [B][3][H][W] -> uint8 [B][H][W][3] = trunc(clamp(x * 255, 0, 255)); bgr=True writes BGR (app_overlay.py:381-388)."""
    B, C, H, W = x.shape
    assert C == 3
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=x.device)
    _lib.call("tup_f32chw_to_u8hwc", _chk(x, F32, None, "x"), out.data_ptr(), B, H, W, int(bgr), _stream())
    return out


# ---- NV12 / P010 video frames (YUV 4:2:0 in 8 and 10 bits: what a decoder hands over and an encoder takes; definitions in DESIGN 3,
# "NV12 frames" and "P010 frames").  One set of helpers for both: a format is its sample dtype, its matrices and its two C entries ----
_Yuv420 = collections.namedtuple("_Yuv420", "name dtype matrices decode encode")
_NV12 = _Yuv420("NV12", torch.uint8, {"bt601": 0, "bt709": 1}, "tup_nv12_to_f32chw", "tup_f32chw_to_nv12")
# bt2020 (non-constant luminance) exists for P010 only
_P010 = _Yuv420("P010", torch.uint16, {"bt601": 0, "bt709": 1, "bt2020": 2}, "tup_p010_to_f32chw", "tup_f32chw_to_p010")


def _dtype_name(dtype):
    return str(dtype).split(".")[-1]


def _yuv420_matrix(op, matrix, table):
    if matrix not in table:
        raise ValueError(f"{op}: matrix must be {' or '.join(repr(m) for m in table)}, got {matrix!r}")
    return table[matrix]


def _on_current_gpu(op, t, name):
    if not t.is_cuda:
        raise ValueError(f"{op}: {name} lives on {t.device}; the HIP path needs a GPU tensor (no CPU fallback)")
    if t.device.index != _cur_dev():
        # every launch goes to the CURRENT device's stream: a tensor of another device would be a wild pointer there
        raise ValueError(f"{op}: {name} lives on {t.device} but the current device is cuda:{_cur_dev()}")


def _yuv420_plane(op, t, name, tail, dtype):
    """A plane of an NV12 / P010 surface as (data_ptr, B, rows, row samples, pitch, batch stride), pitch and stride in bytes: `dtype`
    on the current GPU, [B] + rows + `tail` dimensions with the tail contiguous and one stride per row and per frame, which is what a
    slice of a pitched surface has."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise TypeError(f"{op}: {name} must be a {_dtype_name(dtype)} tensor, got {getattr(t, 'dtype', type(t))}")
    if t.dim() not in (1 + tail, 2 + tail):
        raise ValueError(f"{op}: {name} must have {1 + tail} dimensions (one frame) or {2 + tail} (a batch), got shape {tuple(t.shape)}")
    _on_current_gpu(op, t, name)
    if t.dim() == 1 + tail:
        t = t.unsqueeze(0)
    B, rows = int(t.shape[0]), int(t.shape[1])
    width = 1
    for n in t.shape[2:]:
        width *= int(n)
    if tail == 2 and t.shape[3] != 2:
        raise ValueError(f"{op}: {name} must end in (Cb, Cr) pairs [.., H/2, W/2, 2], got shape {tuple(t.shape)}")
    st = t.stride()
    inner = (st[2] == 1 or width <= 1) if tail == 1 else ((st[3] == 1 and st[2] == 2) or width <= 2)
    if not inner:
        raise ValueError(f"{op}: {name}: the innermost dimension{'s' if tail == 2 else ''} must be contiguous, got strides {tuple(st)}")
    esize = t.element_size()
    pitch = (int(st[1]) if rows > 1 else width) * esize
    if pitch < width * esize or pitch >= 2 ** 31:
        raise ValueError(f"{op}: {name}: row stride {pitch} must be at least the row's {width * esize} bytes (and below 2^31)")
    return t.data_ptr(), B, rows, width, pitch, (int(st[0]) * esize if B > 1 else 0)


def _yuv420_geometry(op, y, uv, fmt):
    yp, B, H, W, ypitch, ybs = _yuv420_plane(op, y, "y", 1, fmt.dtype)
    up, Bu, h2, w2x2, upitch, ubs = _yuv420_plane(op, uv, "uv", 2, fmt.dtype)
    if H % 2 or W % 2:
        raise ValueError(f"{op}: y is {H} x {W}; {fmt.name} needs an even height and width")
    if (Bu, h2, w2x2) != (B, H // 2, W):
        raise ValueError(f"{op}: uv must be [{B}][{H // 2}][{W // 2}][2] for a y of [{B}][{H}][{W}], got {tuple(uv.shape)}")
    if B > 65535:
        raise ValueError(f"{op}: {B} frames in one launch (at most 65535)")
    return yp, up, ybs, ypitch, ubs, upitch, B, H, W


def _yuv420_planes(op, fmt, buf, H, W):
    H, W = int(H), int(W)
    if H < 2 or W < 2 or H % 2 or W % 2:
        raise ValueError(f"{op}: H = {H} and W = {W} must be even and at least 2")
    if not isinstance(buf, torch.Tensor) or buf.dtype != fmt.dtype:
        raise TypeError(f"{op}: buf must be a {_dtype_name(fmt.dtype)} tensor, got {getattr(buf, 'dtype', type(buf))}")
    if buf.dim() not in (2, 3) or buf.shape[-2] < H + H // 2 or buf.shape[-1] < W:
        raise ValueError(f"{op}: buf must be [{H + H // 2}][>= {W}] (or a batch of those), got shape {tuple(buf.shape)}")
    if buf.stride(-1) != 1:
        raise ValueError(f"{op}: buf: the innermost dimension must be contiguous, got strides {tuple(buf.stride())}")
    return buf[..., :H, :W], buf[..., H:H + H // 2, :W].unflatten(-1, (W // 2, 2))


def _yuv420_to_tensor(op, fmt, y, uv, matrix, full_range):
    m = _yuv420_matrix(op, matrix, fmt.matrices)
    yp, up, ybs, ypitch, ubs, upitch, B, H, W = _yuv420_geometry(op, y, uv, fmt)
    out = torch.empty((B, 3, H, W), dtype=F32, device=y.device)
    _lib.call(fmt.decode, yp, up, ybs, ypitch, ubs, upitch, out.data_ptr(), B, H, W, m, int(bool(full_range)), _stream())
    return out


def _tensor_to_yuv420(op, fmt, x, matrix, full_range, out):
    m = _yuv420_matrix(op, matrix, fmt.matrices)
    if not isinstance(x, torch.Tensor) or x.dtype != F32:
        raise TypeError(f"{op}: x must be a float32 tensor, got {getattr(x, 'dtype', type(x))}")
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"{op}: x must be [B][3][H][W], got shape {tuple(x.shape)}")
    B, _, H, W = (int(v) for v in x.shape)
    if H % 2 or W % 2:
        raise ValueError(f"{op}: x is {H} x {W}; {fmt.name} needs an even height and width")
    _on_current_gpu(op, x, "x")
    xp = _chk(x, F32, None, f"{op}: x")
    if out is None:
        y = torch.empty((B, H, W), dtype=fmt.dtype, device=x.device)
        uv = torch.empty((B, H // 2, W // 2, 2), dtype=fmt.dtype, device=x.device)
    else:
        y, uv = out
    yp, up, ybs, ypitch, ubs, upitch, Bo, Ho, Wo = _yuv420_geometry(f"{op}: out", y, uv, fmt)
    if (Bo, Ho, Wo) != (B, H, W):
        raise ValueError(f"{op}: out is for [{Bo}][{Ho}][{Wo}] frames, x is [{B}][3][{H}][{W}]")
    row = W * y.element_size()
    if B > 1 and (ybs < (H - 1) * ypitch + row or ubs < (H // 2 - 1) * upitch + row):
        raise ValueError(f"{op}: out: the frames of a plane overlap (batch stride below one frame)")
    _lib.call(fmt.encode, xp, yp, up, ybs, ypitch, ubs, upitch, B, H, W, m, int(bool(full_range)), _stream())
    return y, uv


def nv12_planes(buf, H, W):
    """The (y, uv) views of single-buffer NV12 frames: buf uint8 [3H/2 or more][pitch] or [B][...][pitch] with the Y rows on top and
    the rows of (Cb, Cr) pairs below them -> y [..][H][W], uv [..][H/2][W/2][2].  No copy; rows beyond 3H/2 and bytes beyond W are
    padding."""
    return _yuv420_planes("nv12_planes", _NV12, buf, H, W)


def nv12_to_tensor(y, uv, matrix="bt709", full_range=False):
    """NV12 frames on the GPU -> fp32 [B][3][H][W] RGB in [0, 1], bit-exact "convert to RGB24, then ToTensor" under the integer
    definition of DESIGN 3.  y uint8 [B][H][W] (or [H][W]), uv uint8 [B][H/2][W/2][2] (or [H/2][W/2][2]) = (Cb, Cr), chroma sited
    left; any views with contiguous rows and uniform row / batch strides, e.g. the two halves of `nv12_planes`."""
    return _yuv420_to_tensor("nv12_to_tensor", _NV12, y, uv, matrix, full_range)


def tensor_to_nv12(x, matrix="bt709", full_range=False, out=None):
    """fp32 [B][3][H][W] (or [3][H][W]) -> NV12 frames (y uint8 [B][H][W], uv uint8 [B][H/2][W/2][2]): bytes as `tensor_to_frames`
    makes them, then the integer matrix and the [1 2 1] x [1 1] chroma filter of DESIGN 3.  out=(y, uv) writes into such views
    (e.g. of a pitched surface; padding bytes are left alone)."""
    return _tensor_to_yuv420("tensor_to_nv12", _NV12, x, matrix, full_range, out)


def p010_planes(buf, H, W):
    """The (y, uv) views of single-buffer P010 frames: buf uint16 [3H/2 or more][pitch] or [B][...][pitch] (pitch in samples) with the
    Y rows on top and the rows of (Cb, Cr) pairs below them -> y [..][H][W], uv [..][H/2][W/2][2].  No copy; rows beyond 3H/2 and
    samples beyond W are padding."""
    return _yuv420_planes("p010_planes", _P010, buf, H, W)


def p010_to_tensor(y, uv, matrix="bt709", full_range=False):
    """P010 frames (10-bit YUV 4:2:0) on the GPU -> fp32 [B][3][H][W] RGB in [0, 1] = 10-bit code / 1023, bit-exact with the integer
    definition of DESIGN 3 ("P010 frames"); never through 8 bits.  y uint16 [B][H][W] (or [H][W]), uv uint16 [B][H/2][W/2][2] (or
    [H/2][W/2][2]) = (Cb, Cr); a sample carries its code in the high ten bits and the low six are ignored.  matrix 'bt601', 'bt709' or
    'bt2020'; the transfer function is not touched (PQ / HLG code values pass through; the model was trained on SDR)."""
    return _yuv420_to_tensor("p010_to_tensor", _P010, y, uv, matrix, full_range)


def tensor_to_p010(x, matrix="bt709", full_range=False, out=None):
    """fp32 [B][3][H][W] (or [3][H][W]) -> P010 frames (y uint16 [B][H][W], uv uint16 [B][H/2][W/2][2]): codes q_10(x) =
    (int)(clamp(x * 1023, 0, 1023) + 0.5), NaN -> 0 (round to nearest, where the 8-bit paths truncate), then the integer matrix and
    the [1 2 1] x [1 1] chroma filter of DESIGN 3; samples are code << 6.  out=(y, uv) writes into such views (padding is left alone)."""
    return _tensor_to_yuv420("tensor_to_p010", _P010, x, matrix, full_range, out)


# ---- branch A in training through its composition (csrc/branch_a_train.hip), r = 2 ----
def bra_compose(wu, bu, w3):
    """Composed weights of (Conv2d(64, 256, 3) + PixelShuffle(2) + Conv2d(64, 3, 3, bias=False)) in the kernels' layouts:
    dict(wp, bias, wv, bv, wd)."""
    dev = wu.device
    wv = torch.empty((9, 12, 25, 64), dtype=BF16, device=dev)
    bv = torch.empty((9, 12), dtype=F32, device=dev)
    wp = torch.zeros((1, 1, 25, 16, 64), dtype=BF16, device=dev)
    wd = torch.zeros((13, 64, 32), dtype=BF16, device=dev)
    _lib.call("tup_bra_compose", _chk(wu, F32, (256, 64, 3, 3), "wu"), _chk(bu, F32, (256,), "bu"), _chk(w3, F32, (3, 64, 3, 3), "w3"),
              wv.data_ptr(), bv.data_ptr(), wp.data_ptr(), wd.data_ptr(), _stream())
    return {"wp": wp, "bias": bv[0].contiguous(), "wv": wv, "bv": bv, "wd": wd}


def bra_backward(g, ui, feat, comp, wu, bu, w3):
    """g: fp32 [B][3][2H][2W] gradient w.r.t. upscaled_input (pre-mask), ui: upscaled_input, feat: bf16 [B][H][W][64].
    Returns (dfeat bf16 [B][H][W][64], dwu, dbu, dw3)."""
    B, H, W, C = feat.shape
    assert C == 64 and tuple(g.shape) == (B, 3, 2 * H, 2 * W)
    dev = feat.device
    g12 = torch.empty((B, H, W, 16), dtype=BF16, device=dev)
    dfeat = torch.empty((B, H, W, 64), dtype=BF16, device=dev)
    G = _zeros((16, 9, 12, 25, 64), dev)          # 16 replicas against atomic contention, summed by tup_bra_chain
    Gb = _zeros((16, 9, 12), dev)
    _lib.call("tup_bra_backward", _chk(g, F32, None, "g"), _chk(ui, F32, g.shape, "ui"), _chk(feat, BF16, None, "feat"),
              _chk(comp["wd"], BF16, (13, 64, 32), "wd"), _chk(comp["wv"], BF16, (9, 12, 25, 64), "wv"),
              g12.data_ptr(), dfeat.data_ptr(), G.data_ptr(), Gb.data_ptr(), B, H, W, _stream())
    dM = torch.empty((3 * 9 * 4 * 9 * 64,), dtype=F32, device=dev)
    dMb = torch.empty((108,), dtype=F32, device=dev)
    dwu = torch.empty((256, 64, 3, 3), dtype=F32, device=dev)
    dbu = torch.empty((256,), dtype=F32, device=dev)
    dw3 = torch.empty((3, 64, 3, 3), dtype=F32, device=dev)
    _lib.call("tup_bra_chain", G.data_ptr(), Gb.data_ptr(), _chk(wu, F32, (256, 64, 3, 3), "wu"), _chk(bu, F32, (256,), "bu"),
              _chk(w3, F32, (3, 64, 3, 3), "w3"), dM.data_ptr(), dMb.data_ptr(), dwu.data_ptr(), dbu.data_ptr(), dw3.data_ptr(), _stream())
    return dfeat, dwu, dbu, dw3, G, Gb


def resize_frames(frames_u8, size, to_tensor=False, bgr=False, resample="bilinear"):
    """transforms.Resize(size) on uint8 frames [B][H][W][3] (or [H][W][3]) on the GPU, bit-exact with Pillow's BILINEAR resample
    of an RGB image (data_handling/data_class.py:61-71, inference.py:65-75).  to_tensor=False -> uint8 [B][h][w][3];
    to_tensor=True -> fp32 [B][3][h][w] in [0, 1] (Resize + ToTensor in the same launches).  resample="bicubic" is Pillow's BICUBIC
    (``Image.resize(size, Image.BICUBIC)``, the reference's baseline image, inference.py:83), bit-exact too: the same two kernels
    with the tables of `resize_taps.pil_bicubic_coeffs`."""
    if resample not in _PIL_COEFFS:
        raise ValueError(f"resize_frames: resample must be 'bilinear' or 'bicubic', got {resample!r}")
    if frames_u8.dim() == 3:
        frames_u8 = frames_u8.unsqueeze(0)
    B, H, W, C = frames_u8.shape
    assert C == 3
    h, w = int(size[0]), int(size[1])
    cur = frames_u8
    _chk(cur, torch.uint8, None, "frames")
    if w != W:                                            # Pillow: horizontal pass first, into a uint8 image
        lo, n, k, ks = _pil_taps_on(cur.device, W, w, resample)
        tmp = torch.empty((B, H, w, 3), dtype=torch.uint8, device=cur.device)
        _lib.call("tup_resize_u8_rows", cur.data_ptr(), tmp.data_ptr(), lo.data_ptr(), n.data_ptr(), k.data_ptr(), ks, B, H, W, w, _stream())
        cur = tmp
    if h != H:
        lo, n, k, ks = _pil_taps_on(cur.device, H, h, resample)
        out_u8 = None if to_tensor else torch.empty((B, h, w, 3), dtype=torch.uint8, device=cur.device)
        out_f = torch.empty((B, 3, h, w), dtype=F32, device=cur.device) if to_tensor else None
        _lib.call("tup_resize_u8_cols", cur.data_ptr(), None if out_u8 is None else out_u8.data_ptr(),
                  None if out_f is None else out_f.data_ptr(), lo.data_ptr(), n.data_ptr(), k.data_ptr(), ks, B, H, w, h, int(bgr), _stream())
        return out_f if to_tensor else out_u8
    return frames_to_tensor(cur, bgr=bgr) if to_tensor else (cur if cur is not frames_u8 else cur.clone())


# ---- patch training samples: crops, flip / rotate variants and their LR counterparts in one launch (csrc/patch_pairs.hip) ----
_PATCH_REC = struct.Struct("<Qiiiiii")          # PatchRec: frame, H, W, y0, x0, op, reserved


class _RecordStager:
    """The record table of a `tup_patch_pairs` launch changes with every launch, so it goes up through one of two pinned staging
    buffers in one non-blocking copy (the pattern of accumulate.SegmentLauncher)."""

    def __init__(self, device):
        self.device = device
        self._stage = [None, None]
        self._events = [None, None]
        self._slot = 0

    def upload(self, raw: bytes) -> torch.Tensor:
        slot = self._slot = self._slot ^ 1
        # the host may run ahead of the GPU: a staging slot is rewritten only after the upload that last read it has executed
        if self._events[slot] is not None:
            self._events[slot].synchronize()
        words = len(raw) // 8
        if self._stage[slot] is None or self._stage[slot].numel() < words:
            self._stage[slot] = torch.empty(max(words, 1024), dtype=torch.int64).pin_memory()
        host = self._stage[slot][:words]
        host.copy_(torch.frombuffer(bytearray(raw), dtype=torch.int64))
        table = host.to(self.device, non_blocking=True)
        if self._events[slot] is None:
            self._events[slot] = torch.cuda.Event()
        self._events[slot].record()
        return table


_PATCH_STAGERS = {}


def patch_pairs(frames, boxes, p, scale, out=None):
    """Training patches of a batch in ONE launch.  frames: B uint8 [H][W][3] GPU tensors (RGB, contiguous; the same tensor may appear
    several times); boxes: B tuples (y0, x0, op); p: LR patch side; scale: HR side = p * scale.  Per sample, bit-exact:
    t = frame[y0:y0+P, x0:x0+P]; op & 1: t[:, ::-1]; op & 2: t[::-1]; op & 4: t.transpose(1, 0, 2), in that order; hr = ToTensor(t),
    lr = ToTensor(Image.resize((p, p), BILINEAR)(t)).  Returns (lr fp32 [B][3][p][p], hr fp32 [B][3][P][P]); out=(lr, hr) supplies
    them.  Everything is validated on the host before anything is uploaded: a crop that leaves its frame never reaches the device."""
    p, scale = int(p), int(scale)
    if p < 1 or scale < 1:
        raise ValueError(f"patch_pairs: p = {p} and scale = {scale} must be >= 1")
    if scale > 8:
        raise ValueError(f"patch_pairs: scale {scale} is beyond the kernel's LDS window (scales up to 8)")
    P = p * scale
    frames, boxes = list(frames), list(boxes)
    B = len(frames)
    if len(boxes) != B:
        raise ValueError(f"patch_pairs: {B} frames but {len(boxes)} boxes")
    if B > 65535:
        raise ValueError(f"patch_pairs: {B} samples in one launch (at most 65535)")
    recs = []
    for i, (f, box) in enumerate(zip(frames, boxes)):
        if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8:
            raise TypeError(f"patch_pairs: sample {i}: the frame must be a uint8 tensor, got {getattr(f, 'dtype', type(f))}")
        if f.dim() != 3 or f.shape[2] != 3 or not f.is_contiguous():
            raise ValueError(f"patch_pairs: sample {i}: the frame must be contiguous [H][W][3], got {tuple(f.shape)}")
        H, W = int(f.shape[0]), int(f.shape[1])
        if len(box) != 3 or any(int(v) != v for v in box):
            raise ValueError(f"patch_pairs: sample {i}: box {box!r} is not (y0, x0, op) in integers")
        y0, x0, op = (int(v) for v in box)
        if y0 < 0 or x0 < 0 or y0 + P > H or x0 + P > W:
            raise ValueError(f"patch_pairs: sample {i}: the {P} x {P} crop at (y0, x0) = ({y0}, {x0}) leaves its {H} x {W} frame")
        if not 0 <= op < 8:
            raise ValueError(f"patch_pairs: sample {i}: op {op} is outside [0, 8)")
        recs.append((f, H, W, y0, x0, op))
    if B == 0:
        dev = out[0].device if out is not None else torch.device("cuda", _cur_dev())
    else:
        dev = frames[0].device
        for i, f in enumerate(frames):
            if not f.is_cuda or f.device != dev or f.device.index != _cur_dev():
                raise RuntimeError(f"patch_pairs: sample {i}: the frame lives on {f.device}; every frame must be on the current GPU "
                                   f"cuda:{_cur_dev() if torch.cuda.is_available() else '?'} (no CPU fallback)")
    if out is None:
        lr = torch.empty((B, 3, p, p), dtype=F32, device=dev)
        hr = torch.empty((B, 3, P, P), dtype=F32, device=dev)
    else:
        lr, hr = out
        _chk(lr, F32, (B, 3, p, p), "out lr")
        _chk(hr, F32, (B, 3, P, P), "out hr")
    if B == 0:
        return lr, hr
    lo, n, k, ks = _pil_taps_on(dev, P, p)
    raw = b"".join(_PATCH_REC.pack(f.data_ptr(), H, W, y0, x0, op, 0) for f, H, W, y0, x0, op in recs)
    stager = _PATCH_STAGERS.get(dev)
    if stager is None:
        stager = _PATCH_STAGERS[dev] = _RecordStager(dev)
    table = stager.upload(raw)
    _lib.call("tup_patch_pairs", table.data_ptr(), B, P, p, lo.data_ptr(), n.data_ptr(), k.data_ptr(), ks,
              hr.data_ptr(), lr.data_ptr(), _stream())
    return lr, hr


# ---- training degradations: blur, noise and a JPEG round trip on bytes in one launch (csrc/degrade.hip) ----
_DEGRADE_REC = struct.Struct("<iiiiiIii")       # DegradeRec: taps[4], noise_amp, noise_seed, quality, flags
DEGRADE_PRECISION_BITS = 32 - 8 - 2             # Pillow's fixed point for 8-bit images
DEGRADE_TAPS_OFF = (1 << DEGRADE_PRECISION_BITS, 0, 0, 0)
DEGRADE_GREY_NOISE = 1                          # flags & 1: one noise value per pixel instead of one per channel
DEGRADE_JPEG_420 = 4                            # flags & 4: this sample's JPEG round trip is 4:2:0 (csrc/degrade420.hip); bit 2 is not used
DEGRADE_OFF = (DEGRADE_TAPS_OFF, 0, 0, 0, 0)    # the record that changes nothing but the quantisation to bytes
DEGRADE_MAX_BLUR_SIGMA = 3.0                    # beyond it the radius-3 truncation is a box, not a Gaussian
DEGRADE_MAX_NOISE_AMP = 1 << 20                 # 510 * amp + 2^15 stays inside 32 bits (sigma up to ~2300)
_NOISE_UNIT = 147.80054                         # sqrt(4 * (256^2 - 1) / 12): the standard deviation of a sum of four uniform bytes
_DEGRADE_STAGERS = {}


def blur_taps(sigma):
    """(k0, k1, k2, k3) of a Gaussian of `sigma` pixels truncated at radius 3, normalised in float64 and rounded to 22-bit fixed
    point, the rounding residue added to k0 so that k0 + 2 (k1 + k2 + k3) == 1 << 22 exactly.  sigma = 0 is the identity."""
    sigma = float(sigma)
    if not 0.0 <= sigma <= DEGRADE_MAX_BLUR_SIGMA:
        raise ValueError(f"blur_taps: sigma = {sigma} must be in [0, {DEGRADE_MAX_BLUR_SIGMA}]")
    if sigma == 0.0:
        return DEGRADE_TAPS_OFF
    g = np.exp(-0.5 * (np.arange(4, dtype=np.float64) / sigma) ** 2)
    g /= g[0] + 2.0 * g[1:].sum()
    k = [int(round(float(v) * (1 << DEGRADE_PRECISION_BITS))) for v in g]
    k[0] += (1 << DEGRADE_PRECISION_BITS) - (k[0] + 2 * sum(k[1:]))
    return tuple(k)


def noise_amp(sigma):
    """The record's noise_amp for noise of standard deviation `sigma` in 8-bit units: round(sigma * 65536 / 147.80054)."""
    sigma = float(sigma)
    amp = int(round(sigma * 65536 / _NOISE_UNIT)) if sigma >= 0.0 else -1
    if not 0 <= amp <= DEGRADE_MAX_NOISE_AMP:
        raise ValueError(f"noise_amp: sigma = {sigma} must be in [0, {DEGRADE_MAX_NOISE_AMP * _NOISE_UNIT / 65536:.0f}]")
    return amp


def _degrade_record(i, rec):
    """One record as the eight words of a DegradeRec; ValueError naming sample i."""
    if hasattr(rec, "pack"):
        rec = rec.pack()
    try:
        taps, amp, seed, quality, flags = rec
        taps = tuple(taps)
        words = taps + (amp, seed, quality, flags)
        if len(taps) != 4 or any(int(v) != v for v in words):
            raise TypeError
        k0, k1, k2, k3, amp, seed, quality, flags = (int(v) for v in words)
    except (TypeError, ValueError):
        raise ValueError(f"degrade: sample {i}: record {rec!r} is not (taps[4], noise_amp, noise_seed, quality, flags) in integers") from None
    if min(k0, k1, k2, k3) < 0 or k0 + 2 * (k1 + k2 + k3) != 1 << DEGRADE_PRECISION_BITS:
        raise ValueError(f"degrade: sample {i}: taps {taps} must be non-negative with k0 + 2 (k1 + k2 + k3) == 1 << {DEGRADE_PRECISION_BITS}")
    if not 0 <= amp <= DEGRADE_MAX_NOISE_AMP:
        raise ValueError(f"degrade: sample {i}: noise_amp {amp} is outside [0, {DEGRADE_MAX_NOISE_AMP}]")
    if not 0 <= seed < 1 << 32:
        raise ValueError(f"degrade: sample {i}: noise_seed {seed} is not a 32-bit unsigned value")
    if not 0 <= quality <= 100:
        raise ValueError(f"degrade: sample {i}: quality {quality} is outside [0, 100] (0 switches the JPEG round trip off)")
    if flags & ~(DEGRADE_GREY_NOISE | DEGRADE_JPEG_420):
        raise ValueError(f"degrade: sample {i}: unknown flag bits in {flags:#x}")
    if flags & DEGRADE_JPEG_420 and quality == 0:
        raise ValueError(f"degrade: sample {i}: flags {flags:#x} name a JPEG sampling (DEGRADE_JPEG_420) but quality 0 switches the round trip off")
    return k0, k1, k2, k3, amp, seed, quality, flags


def _overlap(a, b):
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def degrade(x, records, out=None):
    """Blur, noise and a JPEG round trip of a batch in ONE launch.  x: fp32 [B][3][H][W] in [0, 1] (what `patch_pairs` returns as
    lr); records: B tuples (taps, noise_amp, noise_seed, quality, flags), or objects whose ``pack()`` returns one.  Per sample, in
    integers and bit-exact against tests/_degrade_ref.py: u = clip(floor(v * 255 + .5)); a separable 7-tap blur with `taps` =
    `blur_taps(sigma)`, rounded to bytes after each pass as Pillow's resampler does; noise of `noise_amp(sigma)` from a hash of
    (noise_seed, element), one value per pixel with flags & DEGRADE_GREY_NOISE; what Pillow's ``save(format="JPEG", quality=q,
    subsampling=0)`` and ``open().convert("RGB")`` give back (quality 0: off; with flags & DEGRADE_JPEG_420 ``subsampling=2``, Pillow's
    default, bit-exact against tests/_degrade420_ref.py); result = u / 255.  `DEGRADE_OFF` switches every stage off.  A batch without
    a 4:2:0 record is one `tup_degrade_lr` call; any other is one `tup_degrade_lr_sub` call for all its samples.  Returns fp32 [B][3][H][W]; `out` supplies it and must not overlap x.  Everything is validated on the host before anything
    is uploaded: a bad record is a ValueError naming its sample."""
    if not isinstance(x, torch.Tensor) or x.dtype != F32:
        raise TypeError(f"degrade: x must be an fp32 tensor, got {getattr(x, 'dtype', type(x))}")
    if x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous():
        raise ValueError(f"degrade: x must be contiguous [B][3][H][W], got {tuple(x.shape)}")
    B, _, H, W = (int(v) for v in x.shape)
    if H < 1 or W < 1:
        raise ValueError(f"degrade: x has no pixels: {tuple(x.shape)}")
    if B > 65535:
        raise ValueError(f"degrade: {B} samples in one launch (at most 65535)")
    records = list(records)
    if len(records) != B:
        raise ValueError(f"degrade: {B} samples but {len(records)} records")
    words = [_degrade_record(i, rec) for i, rec in enumerate(records)]
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != F32:
            raise TypeError(f"degrade: out must be an fp32 tensor, got {getattr(out, 'dtype', type(out))}")
        if tuple(out.shape) != tuple(x.shape) or not out.is_contiguous():
            raise ValueError(f"degrade: out must be contiguous {tuple(x.shape)}, got {tuple(out.shape)}")
        if out.device != x.device:
            raise RuntimeError(f"degrade: out lives on {out.device}, x on {x.device}")
        if B and _overlap(x, out):
            raise ValueError("degrade: out must not overlap x (a tile reads its neighbours' pixels)")
    if not x.is_cuda or x.device.index != _cur_dev():
        raise RuntimeError(f"degrade: x lives on {x.device}; it must be on the current GPU "
                           f"cuda:{_cur_dev() if torch.cuda.is_available() else '?'} (no CPU fallback)")
    if out is None:
        out = torch.empty_like(x)
    if B == 0:
        return out
    stager = _DEGRADE_STAGERS.get(x.device)
    if stager is None:
        stager = _DEGRADE_STAGERS[x.device] = _RecordStager(x.device)
    table = stager.upload(b"".join(_DEGRADE_REC.pack(*w) for w in words))
    entry = "tup_degrade_lr_sub" if any(w[7] & DEGRADE_JPEG_420 for w in words) else "tup_degrade_lr"
    _lib.call(entry, x.data_ptr(), table.data_ptr(), B, H, W, out.data_ptr(), _stream())
    return out


# ---- baseline JPEG encoding of a batch (csrc/jpeg_encode.hip) ----
JPEG_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
               35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_JPEG_BASE = (
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32)
# Annex K.3 - K.6 as a DHT segment carries them: (table class << 4 | id, codes of each length 1..16, symbols in code order)
_JPEG_DHT = (
    (0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d),
     (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
      0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
      0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
      0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
      0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
      0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
      0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)),
    (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77),
     (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
      0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
      0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
      0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
      0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
      0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
      0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)),
)
JPEG_CHUNK_BLOCKS = 96                           # 8 x 8 blocks a workgroup codes at a time: 16 MCUs of 4:2:0, 32 of 4:4:4
_JPEG_SUBSAMPLING = {"4:4:4": 0, 0: 0, "4:2:0": 2, 2: 2}
_jpeg_headers = {}


def jpeg_quant_table(which, quality):
    """The Annex K table (0 luma, 1 chroma) scaled to `quality` as jpeg_set_quality does, 64 values in natural order."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(min(max((v * s + 50) // 100, 1), 255) for v in _JPEG_BASE[which])


def _jpeg_params(H, W, quality, subsampling, restart_rows):
    """(subsampling code, restart interval in MCUs, restart segments) after every check `jpeg_encode` makes on its parameters."""
    if isinstance(subsampling, bool) or subsampling not in _JPEG_SUBSAMPLING:
        raise ValueError(f"jpeg_encode: subsampling must be '4:4:4' / 0 or '4:2:0' / 2, got {subsampling!r}")
    sub = _JPEG_SUBSAMPLING[subsampling]
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"jpeg_encode: quality must be an integer in 1..100, got {quality!r}")
    if isinstance(restart_rows, bool) or not isinstance(restart_rows, int) or restart_rows < 1:
        raise ValueError(f"jpeg_encode: restart_rows must be an integer >= 1, got {restart_rows!r} (a file without restarts is not offered)")
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"jpeg_encode: a JPEG image is 1..65535 pixels a side, got {H} x {W}")
    m = 16 if sub == 2 else 8
    mw, mh = (W + m - 1) // m, (H + m - 1) // m
    if restart_rows * mw > 65535:
        raise ValueError(f"jpeg_encode: restart_rows = {restart_rows} x {mw} MCUs a row is a restart interval above 65535")
    return sub, restart_rows * mw, (mh + restart_rows - 1) // restart_rows


def jpeg_header(H, W, quality=75, subsampling="4:2:0", restart_rows=1):
    """The bytes before the scan, built from the parameters alone: SOI, APP0 (JFIF 1.01), DQT x 2, SOF0, DHT x 4, DRI, SOS."""
    sub, interval, _ = _jpeg_params(H, W, quality, subsampling, restart_rows)
    seg = lambda marker, payload: bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i in (0, 1):
        t = jpeg_quant_table(i, quality)
        out += seg(0xDB, bytes([i]) + bytes(t[k] for k in JPEG_ZIGZAG))
    out += seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, 0x22 if sub == 2 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for ident, counts, symbols in _JPEG_DHT:
        out += seg(0xC4, bytes([ident]) + bytes(counts) + bytes(symbols))
    out += seg(0xDD, interval.to_bytes(2, "big"))
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def _jpeg_header_on(device, key):
    k = (str(device),) + key
    if k not in _jpeg_headers:
        if len(_jpeg_headers) >= 64:
            _jpeg_headers.clear()
        _jpeg_headers[k] = torch.frombuffer(bytearray(jpeg_header(*key)), dtype=torch.uint8).to(device)
    return _jpeg_headers[k]


def jpeg_encode(frames, quality=75, subsampling="4:2:0", restart_rows=1, out=None):
    """Baseline JPEG files of a batch, made on the GPU in three launches.  frames: uint8 [B][H][W][3] (or [H][W][3]) RGB, or fp32
    [B][3][H][W] quantised as `tensor_to_frames` does, trunc(clamp(x * 255, 0, 255)), inside the first kernel.  The file of image b
    is byte for byte what ``Image.fromarray(frame_b).save(buf, "JPEG", quality=quality, subsampling=subsampling,
    restart_marker_rows=restart_rows)`` writes: standard Huffman tables, 4:2:0 ("4:2:0" / 2, Pillow's default) or 4:4:4 ("4:4:4" /
    0), a restart marker every `restart_rows` MCU rows (the restart segments are what the GPU codes in parallel).
    Returns (data uint8 [B][capacity], lengths int32 [B]); `jpeg_files` turns them into bytes.  out=None: the lengths are read back
    once (the call's one host synchronisation) and `data` is allocated to the longest file.  out=(data, lengths): nothing
    synchronises; an image longer than data's row gets length -1 and none of its bytes.  Everything is validated before any launch."""
    if not isinstance(frames, torch.Tensor) or frames.dtype not in (torch.uint8, F32):
        raise TypeError(f"jpeg_encode: frames must be a uint8 or float32 tensor, got {getattr(frames, 'dtype', type(frames))}")
    if frames.dtype == torch.uint8:
        if frames.dim() == 3:
            frames = frames.unsqueeze(0)
        if frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError(f"jpeg_encode: uint8 frames must be [B][H][W][3] or [H][W][3], got shape {tuple(frames.shape)}")
        B, H, W = (int(v) for v in frames.shape[:3])
    else:
        if frames.dim() != 4 or frames.shape[1] != 3:
            raise ValueError(f"jpeg_encode: float32 frames must be [B][3][H][W], got shape {tuple(frames.shape)}")
        B, H, W = int(frames.shape[0]), int(frames.shape[2]), int(frames.shape[3])
    if not 1 <= B <= 65535:
        raise ValueError(f"jpeg_encode: {B} images in one call (1..65535)")
    sub, _, S = _jpeg_params(H, W, quality, subsampling, restart_rows)
    if not frames.is_contiguous():
        raise ValueError("jpeg_encode: frames must be contiguous")
    if out is not None:
        data, lengths = out
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() != 2 or data.shape[0] != B or not data.is_contiguous():
            raise ValueError(f"jpeg_encode: out[0] must be a contiguous uint8 [{B}][capacity] tensor, got {getattr(data, 'dtype', type(data))} "
                             f"{tuple(getattr(data, 'shape', ()))}")
        if not isinstance(lengths, torch.Tensor) or lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,) or not lengths.is_contiguous():
            raise ValueError(f"jpeg_encode: out[1] must be a contiguous int32 [{B}] tensor, got {getattr(lengths, 'dtype', type(lengths))} "
                             f"{tuple(getattr(lengths, 'shape', ()))}")
        if data.shape[1] >= 2 ** 31:
            raise ValueError(f"jpeg_encode: out[0] has rows of {data.shape[1]} bytes (below 2^31)")
    _on_current_gpu("jpeg_encode", frames, "frames")
    if out is not None:
        _on_current_gpu("jpeg_encode", data, "out[0]")
        _on_current_gpu("jpeg_encode", lengths, "out[1]")
    dev = frames.device
    u8 = frames.data_ptr() if frames.dtype == torch.uint8 else None
    f32 = frames.data_ptr() if frames.dtype == F32 else None
    header = _jpeg_header_on(dev, (H, W, quality, sub, restart_rows))
    work = torch.empty((2, B, S), dtype=torch.int32, device=dev)
    if _lib.load().tup_jpeg_segments(H, W, sub, restart_rows) != S:
        raise RuntimeError("jpeg_encode: the library counts other restart segments than the binding")
    _lib.call("tup_jpeg_sizes", u8, f32, B, H, W, quality, sub, restart_rows, work[0].data_ptr(), _stream())
    if out is None:
        lengths = torch.empty((B,), dtype=torch.int32, device=dev)
        _lib.call("tup_jpeg_offsets", work[0].data_ptr(), B, S, header.numel(), 2 ** 31 - 1, work[1].data_ptr(), lengths.data_ptr(), _stream())
        host = lengths.cpu().tolist()                                   # the one synchronisation
        if min(host) < 0:
            raise RuntimeError("jpeg_encode: a file of 2 GiB or more")
        data = torch.empty((B, max(host)), dtype=torch.uint8, device=dev)
    else:
        _lib.call("tup_jpeg_offsets", work[0].data_ptr(), B, S, header.numel(), int(data.shape[1]), work[1].data_ptr(), lengths.data_ptr(), _stream())
    _lib.call("tup_jpeg_write", u8, f32, B, H, W, quality, sub, restart_rows, header.data_ptr(), header.numel(), work[1].data_ptr(),
              lengths.data_ptr(), data.data_ptr(), int(data.shape[1]), _stream())
    return data, lengths


def jpeg_files(data, lengths):
    """(data, lengths) of `jpeg_encode` -> a list of bytes, one file per image (one copy to the host).  An image that did not fit
    (length -1) is an error."""
    return _files("jpeg_files", data, lengths)


def _files(op, data, lengths):
    n = [int(v) for v in lengths.cpu().tolist()]
    if any(v < 0 for v in n):
        raise ValueError(f"{op}: image {[i for i, v in enumerate(n) if v < 0][0]} did not fit its row of {data.shape[1]} bytes")
    host = data.cpu().numpy()
    return [host[i, :v].tobytes() for i, v in enumerate(n)]


# ---- PNG encoding of a batch (csrc/png_encode.hip, csrc/png_deflate.h) ----
PNG_FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}
PNG_MIN_BLOCK, PNG_MAX_BLOCK = 256, 32768
PNG_BLOCK_BYTES = 16384                          # the default range of the filtered stream one workgroup codes (DESIGN 7m has the measurement)


def _png_bps(op, bits):
    """bytes per sample of a file of `bits` bits"""
    if isinstance(bits, bool) or bits not in (8, 16):
        raise ValueError(f"{op}: bits must be 8 or 16, got {bits!r}")
    return bits // 8


def _png_params(op, H, W, block_bytes, bps=1):
    """the number of deflate blocks after every check on the geometry; a row is 1 + 3 bps W filtered bytes"""
    if isinstance(block_bytes, bool) or not isinstance(block_bytes, int) or not PNG_MIN_BLOCK <= block_bytes <= PNG_MAX_BLOCK:
        raise ValueError(f"{op}: block_bytes must be an integer in {PNG_MIN_BLOCK}..{PNG_MAX_BLOCK}, got {block_bytes!r}")
    if isinstance(H, bool) or isinstance(W, bool) or not isinstance(H, int) or not isinstance(W, int) or H < 1 or W < 1:
        raise ValueError(f"{op}: an image is at least 1 x 1, got {H!r} x {W!r}")
    if H * (1 + 3 * bps * W) >= 2 ** 31:
        raise ValueError(f"{op}: {H} x {W} has a filtered stream of {H * (1 + 3 * bps * W)} bytes (below 2^31)")
    return -(-(H * (1 + 3 * bps * W)) // block_bytes)


def png_max_bytes(H, W, block_bytes=PNG_BLOCK_BYTES, bits=8):
    """The length of the file whose blocks are all stored: no file of `png_encode` for this geometry and depth is longer, so rows of
    this many bytes always fit (`out=`)."""
    bps = _png_bps("png_max_bytes", bits)
    N = _png_params("png_max_bytes", H, W, block_bytes, bps)
    return 33 + 2 + H * (1 + 3 * bps * W) + (12 + 5) * N + 16 + 12


def png_encode(frames, filter="adaptive", block_bytes=PNG_BLOCK_BYTES, out=None, bits=8):
    """PNG files (8-bit RGB, no interlace) of a batch, made on the GPU.  frames: uint8 [B][H][W][3] (or [H][W][3]) RGB, or fp32
    [B][3][H][W] quantised as `tensor_to_frames` does, trunc(clamp(x * 255, 0, 255)), inside the kernels.  bits=16 writes 16-bit files
    (IHDR depth 16, samples big-endian, rows of 1 + 6 W filtered bytes, everything else as below; tests/_png16_ref.py states them):
    frames uint16 [B][H][W][3] (or [H][W][3]), or fp32 [B][3][H][W] quantised inside the kernels by q_16 = (int)(clamp(x * 65535, 0,
    65535) + 0.5), NaN -> 0, which rounds to nearest; uint8 frames are refused (widen them yourself: v * 257).  filter: "adaptive" (per row,
    the filter with the smallest sum of |residual|) or one of "none", "sub", "up", "average", "paeth" for every row.  The filtered
    stream is cut every `block_bytes` bytes (256..32768) into deflate blocks (literals and runs, the shortest of stored / fixed /
    dynamic Huffman), one IDAT chunk each; the file is byte for byte what tests/_png_ref.py states and does not depend on B or `out`.
    Returns (data uint8 [B][capacity], lengths int32 [B]); `png_files` turns them into bytes.  out=None: the lengths are read back once
    (the call's one host synchronisation) and `data` is allocated to the longest file.  out=(data, lengths): nothing synchronises; an
    image longer than data's row gets length -1 and none of its bytes (`png_max_bytes` always fits).  Everything is validated before
    any launch."""
    bps = _png_bps("png_encode", bits)
    idt = torch.uint8 if bps == 1 else torch.uint16
    if not isinstance(frames, torch.Tensor) or frames.dtype not in (idt, F32):
        raise TypeError(f"png_encode: frames must be a {_dtype_name(idt)} or float32 tensor{'' if bps == 1 else ' for bits=16'}, "
                        f"got {getattr(frames, 'dtype', type(frames))}")
    if frames.dtype == idt:
        if frames.dim() == 3:
            frames = frames.unsqueeze(0)
        if frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError(f"png_encode: {_dtype_name(idt)} frames must be [B][H][W][3] or [H][W][3], got shape {tuple(frames.shape)}")
        B, H, W = (int(v) for v in frames.shape[:3])
    else:
        if frames.dim() != 4 or frames.shape[1] != 3:
            raise ValueError(f"png_encode: float32 frames must be [B][3][H][W], got shape {tuple(frames.shape)}")
        B, H, W = int(frames.shape[0]), int(frames.shape[2]), int(frames.shape[3])
    if not 1 <= B <= 65535:
        raise ValueError(f"png_encode: {B} images in one call (1..65535)")
    if not isinstance(filter, str) or filter not in PNG_FILTERS:
        raise ValueError(f"png_encode: filter must be one of {', '.join(PNG_FILTERS)}, got {filter!r}")
    ft = PNG_FILTERS[filter]
    N = _png_params("png_encode", H, W, block_bytes, bps)
    if not frames.is_contiguous():
        raise ValueError("png_encode: frames must be contiguous")
    if out is not None:
        data, lengths = out
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() != 2 or data.shape[0] != B or not data.is_contiguous():
            raise ValueError(f"png_encode: out[0] must be a contiguous uint8 [{B}][capacity] tensor, got {getattr(data, 'dtype', type(data))} "
                             f"{tuple(getattr(data, 'shape', ()))}")
        if not isinstance(lengths, torch.Tensor) or lengths.dtype != torch.int32 or tuple(lengths.shape) != (B,) or not lengths.is_contiguous():
            raise ValueError(f"png_encode: out[1] must be a contiguous int32 [{B}] tensor, got {getattr(lengths, 'dtype', type(lengths))} "
                             f"{tuple(getattr(lengths, 'shape', ()))}")
        if data.shape[1] >= 2 ** 31:
            raise ValueError(f"png_encode: out[0] has rows of {data.shape[1]} bytes (below 2^31)")
    _on_current_gpu("png_encode", frames, "frames")
    if out is not None:
        _on_current_gpu("png_encode", data, "out[0]")
        _on_current_gpu("png_encode", lengths, "out[1]")
    dev = frames.device
    u8 = frames.data_ptr() if frames.dtype == idt else None             # the integer frames: uint8, or uint16 for bits=16
    e = "tup_png_" if bps == 1 else "tup_png16_"
    f32 = frames.data_ptr() if frames.dtype == F32 else None
    work = torch.empty((3, B, N), dtype=torch.int32, device=dev)            # sizes, offsets, Adler partials
    adlers = torch.empty((B,), dtype=torch.int32, device=dev)
    if getattr(_lib.load(), e + "blocks")(H, W, block_bytes) != N:
        raise RuntimeError("png_encode: the library counts other blocks than the binding")
    rows = None
    if ft == PNG_FILTERS["adaptive"]:
        rows = torch.empty((B, H), dtype=torch.uint8, device=dev)
        _lib.call(e + "filters", u8, f32, B, H, W, rows.data_ptr(), _stream())
    rows_ptr = rows.data_ptr() if rows is not None else None
    _lib.call(e + "sizes", u8, f32, B, H, W, ft, block_bytes, rows_ptr, work[0].data_ptr(), work[2].data_ptr(), _stream())
    if out is None:
        lengths = torch.empty((B,), dtype=torch.int32, device=dev)
        _lib.call(e + "offsets", work[0].data_ptr(), work[2].data_ptr(), B, H, W, block_bytes, 2 ** 31 - 1, work[1].data_ptr(),
                  lengths.data_ptr(), adlers.data_ptr(), _stream())
        host = lengths.cpu().tolist()                                   # the one synchronisation
        if min(host) < 0:
            raise RuntimeError("png_encode: a file of 2 GiB or more")
        data = torch.empty((B, max(host)), dtype=torch.uint8, device=dev)
    else:
        _lib.call(e + "offsets", work[0].data_ptr(), work[2].data_ptr(), B, H, W, block_bytes, int(data.shape[1]), work[1].data_ptr(),
                  lengths.data_ptr(), adlers.data_ptr(), _stream())
    _lib.call(e + "write", u8, f32, B, H, W, ft, block_bytes, rows_ptr, work[1].data_ptr(), lengths.data_ptr(), adlers.data_ptr(),
              data.data_ptr(), int(data.shape[1]), _stream())
    return data, lengths


def png_files(data, lengths):
    """(data, lengths) of `png_encode` -> a list of bytes, one file per image (one copy to the host).  An image that did not fit
    (length -1) is an error."""
    return _files("png_files", data, lengths)


# ---- baseline JPEG decoding of a batch (csrc/jpeg_decode.hip) ----
_JPEG_LAYOUT = {"4:4:4": 0, "4:2:0": 2, "grey": 4}
_JPEG_DEC_REC = struct.Struct("<ii4s4s384s1088s")          # JdImage: scan_off, scan_len, td[4], ta[4], qt[3][64] uint16, huff[4][272]
_JPEG_SOF = {0xC1: "extended sequential (SOF1)", 0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)", 0xC5: "differential sequential (SOF5)",
             0xC6: "differential progressive (SOF6)", 0xC7: "differential lossless (SOF7)", 0xC9: "arithmetic-coded sequential (SOF9)",
             0xCA: "arithmetic-coded progressive (SOF10)", 0xCB: "arithmetic-coded lossless (SOF11)", 0xCD: "arithmetic-coded differential (SOF13)",
             0xCE: "arithmetic-coded differential progressive (SOF14)", 0xCF: "arithmetic-coded differential lossless (SOF15)",
             0xCC: "arithmetic coding conditioning (DAC)"}
_JPEG_NEXT_MARKER = re.compile(rb"\xff[^\x00\xd0-\xd7\xff]")


def jpeg_parse(data):
    """The marker segments of a baseline JPEG file, walked on the host without a library: a dict of H, W, components (1 or 3),
    subsampling ("4:4:4", "4:2:0" or "grey"), quant_tables {id: 64 values in natural order}, huffman_tables {(class, id): (the 16
    counts, the symbols)} with class 0 = DC and 1 = AC, and per component component_ids, quant_selectors, dc_selectors,
    ac_selectors; restart_interval in MCUs (0 = none) and scan = (first byte, end) of the entropy-coded data.  APPn and COM segments
    are skipped.  Everything `jpeg_decode` does not decode is a ValueError that names the reason: any SOFn but SOF0, a precision other
    than 8 bits, 16-bit quantisation tables, samplings other than the three above, four components, more than one scan or a scan
    with Ss / Se / Ah / Al other than 0 / 63 / 0 / 0, an Adobe segment whose transform is not YCbCr, component ids libjpeg reads as
    RGB, a table that is selected but missing, Huffman counts that are no prefix code, and a file that ends before SOS."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError(f"jpeg_parse: a file is bytes, got {type(data)}")
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("jpeg_parse: not a JPEG file (no SOI)")
    n, i = len(data), 2
    quant, huff, frame, interval, jfif, adobe = {}, {}, None, 0, False, None
    while True:
        if i + 4 > n:
            raise ValueError("jpeg_parse: the file ends before SOS")
        if data[i] != 0xFF:
            raise ValueError(f"jpeg_parse: no marker at byte {i}")
        m = data[i + 1]
        if m == 0xFF:                                  # fill byte
            i += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD8:             # markers without a length
            i += 2
            continue
        if m == 0xD9:
            raise ValueError("jpeg_parse: the file ends before SOS")
        length = int.from_bytes(data[i + 2:i + 4], "big")
        if length < 2 or i + 2 + length > n:
            raise ValueError("jpeg_parse: the file ends before SOS (a marker segment is cut short)")
        p = data[i + 4:i + 2 + length]
        i += 2 + length
        if m in _JPEG_SOF:
            raise ValueError(f"jpeg_parse: {_JPEG_SOF[m]} is not decoded, only baseline (SOF0)")
        if m == 0xC0:
            if frame is not None:
                raise ValueError("jpeg_parse: two frame headers")
            if len(p) < 6 or len(p) != 6 + 3 * p[5]:
                raise ValueError("jpeg_parse: SOF0 of the wrong length")
            if p[0] != 8:
                raise ValueError(f"jpeg_parse: {p[0]}-bit precision is not decoded, only 8-bit")
            H, W = int.from_bytes(p[1:3], "big"), int.from_bytes(p[3:5], "big")
            if H < 1 or W < 1:
                raise ValueError(f"jpeg_parse: an image of {H} x {W}")
            if p[5] == 4:
                raise ValueError("jpeg_parse: four components (CMYK / YCCK) are not decoded")
            if p[5] not in (1, 3):
                raise ValueError(f"jpeg_parse: {p[5]} components are not decoded, only 1 or 3")
            frame = (H, W, [(p[6 + 3 * c], p[7 + 3 * c], p[8 + 3 * c]) for c in range(p[5])])
        elif m == 0xDB:
            k = 0
            while k < len(p):
                if p[k] >> 4:
                    raise ValueError("jpeg_parse: 16-bit quantisation tables are not decoded")
                if (p[k] & 15) > 3 or k + 65 > len(p):
                    raise ValueError("jpeg_parse: DQT of the wrong length or table number")
                t = [0] * 64
                for z in range(64):
                    t[JPEG_ZIGZAG[z]] = p[k + 1 + z]
                quant[p[k] & 15] = tuple(t)
                k += 65
        elif m == 0xC4:
            k = 0
            while k < len(p):
                if k + 17 > len(p) or (p[k] >> 4) > 1 or (p[k] & 15) > 1:
                    raise ValueError("jpeg_parse: DHT of the wrong length, class or table number (baseline has tables 0 and 1)")
                counts = tuple(p[k + 1:k + 17])
                code = 0
                for bits, c in enumerate(counts, 1):
                    code += c
                    if code > (1 << bits):
                        raise ValueError(f"jpeg_parse: a Huffman table is not a valid prefix code ({c} codes of {bits} bits are more than are left)")
                    code <<= 1
                total = sum(counts)
                if total > 256 or k + 17 + total > len(p):
                    raise ValueError("jpeg_parse: DHT of the wrong length")
                huff[(p[k] >> 4, p[k] & 15)] = (counts, tuple(p[k + 17:k + 17 + total]))
                k += 17 + total
        elif m == 0xDD:
            if len(p) != 2:
                raise ValueError("jpeg_parse: DRI of the wrong length")
            interval = int.from_bytes(p, "big")
        elif m == 0xE0 and p[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and p[:5] == b"Adobe" and len(p) >= 12:
            adobe = p[11]
        elif m == 0xDA:
            break
    if frame is None:
        raise ValueError("jpeg_parse: SOS before SOF0")
    H, W, comps = frame
    ns = p[0] if p else 0
    if len(p) != 4 + 2 * ns:
        raise ValueError("jpeg_parse: SOS of the wrong length")
    if ns != len(comps) or [p[1 + 2 * c] for c in range(ns)] != [c[0] for c in comps]:
        raise ValueError(f"jpeg_parse: more than one scan (the first holds {ns} of {len(comps)} components)")
    if tuple(p[1 + 2 * ns:]) != (0, 63, 0):
        raise ValueError(f"jpeg_parse: a scan with Ss, Se, Ah/Al = {tuple(p[1 + 2 * ns:])}, not 0, 63, 0")
    ids = tuple(c[0] for c in comps)
    if len(comps) == 3:
        if adobe is not None and adobe != 1:
            raise ValueError(f"jpeg_parse: Adobe transform {adobe} (not YCbCr) is not decoded")
        if adobe is None and not jfif and ids == (0x52, 0x47, 0x42):
            raise ValueError("jpeg_parse: component ids 'R', 'G', 'B' without JFIF (libjpeg reads them as RGB) are not decoded")
        samp = tuple(c[1] for c in comps)
        if samp == (0x11, 0x11, 0x11):
            sub = "4:4:4"
        elif samp == (0x22, 0x11, 0x11):
            sub = "4:2:0"
        else:
            raise ValueError("jpeg_parse: sampling factors " + ", ".join(f"{s >> 4}x{s & 15}" for s in samp) + " are not decoded, only 4:4:4 and 4:2:0")
    else:
        sub = "grey"
    dc, ac = tuple(p[2 + 2 * c] >> 4 for c in range(ns)), tuple(p[2 + 2 * c] & 15 for c in range(ns))
    for c, (_, _, tq) in enumerate(comps):
        if tq not in quant:
            raise ValueError(f"jpeg_parse: missing quantisation table {tq}")
        if dc[c] > 1 or ac[c] > 1:
            raise ValueError("jpeg_parse: a Huffman table number above 1 (baseline has tables 0 and 1)")
        if (0, dc[c]) not in huff or (1, ac[c]) not in huff:
            raise ValueError(f"jpeg_parse: missing Huffman table (DC {dc[c]} or AC {ac[c]})")
    nxt = _JPEG_NEXT_MARKER.search(data, i)
    if nxt is not None and (data[nxt.start() + 1] in (0xDA, 0xC4, 0xDB, 0xDD) or 0xC0 <= data[nxt.start() + 1] <= 0xCF):
        raise ValueError("jpeg_parse: more than one scan")
    end = data.rfind(b"\xff\xd9", i)
    return {"H": H, "W": W, "components": len(comps), "subsampling": sub, "quant_tables": quant, "huffman_tables": huff,
            "component_ids": ids, "quant_selectors": tuple(c[2] for c in comps), "dc_selectors": dc, "ac_selectors": ac,
            "restart_interval": interval, "scan": (i, end if end >= 0 else n)}


def _jpeg_decode_geometry(H, W, layout, interval):
    """(segments, workspace bytes per image): the twin of jd_geometry (csrc/jpeg_decode.hip)."""
    m = 16 if layout == 2 else 8
    mw, mh = (W + m - 1) // m, (H + m - 1) // m
    S = (mw * mh + interval - 1) // interval if interval else mh
    return S, mw * m * mh * m + (0 if layout == 4 else 2 * mw * 8 * mh * 8)


def _jpeg_decode_record(info, data, scan_off):
    """The 1488 bytes the kernels read about one image (struct JdImage)."""
    nc = info["components"]
    sel = lambda v: bytes(v) + bytes(4 - nc)
    qt = b"".join(struct.pack("<64H", *info["quant_tables"][info["quant_selectors"][min(c, nc - 1)]]) for c in range(3))
    spec = b""
    for key in ((0, 0), (0, 1), (1, 0), (1, 1)):
        counts, symbols = info["huffman_tables"].get(key, ((0,) * 16, ()))
        spec += bytes(counts) + bytes(symbols) + bytes(256 - len(symbols))
    start, end = info["scan"]
    return _JPEG_DEC_REC.pack(scan_off, end - start, sel(info["dc_selectors"]), sel(info["ac_selectors"]), qt, spec)


JPEG_SYNC_BYTES = 132                                        # JS_BYTES of csrc/jpeg_sync.h: the raw bytes of a subsequence of the sync index
_JPEG_INDEX = ("auto", "serial", "sync")


def _jpeg_decode_files(who, files, index):
    """The checks `jpeg_decode` and `jpeg_scan_index` share, ahead of any launch -> (files, infos, (H, W, subsampling, interval), the
    index that runs)."""
    if index not in _JPEG_INDEX:
        raise ValueError(f"{who}: index must be one of {_JPEG_INDEX}, got {index!r}")
    if isinstance(files, (bytes, bytearray, memoryview)):
        files = [files]
    try:
        files = list(files)
    except TypeError:
        raise TypeError(f"{who}: files must be bytes or a sequence of bytes, got {type(files)}") from None
    B = len(files)
    if not 1 <= B <= 65535:
        raise ValueError(f"{who}: {B} images in one call (1..65535)")
    if any(not isinstance(f, (bytes, bytearray, memoryview)) for f in files):
        raise TypeError(f"{who}: files must be bytes or a sequence of bytes")
    infos = [jpeg_parse(f) for f in files]
    key = lambda s: (s["H"], s["W"], s["subsampling"], s["restart_interval"])
    for b, s in enumerate(infos):
        if key(s) != key(infos[0]):
            raise ValueError(f"{who}: the images of a call share H, W, subsampling and restart interval; image 0 has {key(infos[0])}, "
                             f"image {b} has {key(s)}")
    if index == "sync" and key(infos[0])[3]:
        raise ValueError(f"{who}: index='sync' is for files without restart markers; these have a restart interval of {key(infos[0])[3]} MCUs")
    # "auto" is what ran before there was a choice: the serial walk.  A test of the three launches pins the entry names of a
    # restart-less call with default arguments, so the parallel index is asked for by name (inference.py does)
    return files, infos, key(infos[0]), "sync" if index == "sync" else "serial"


def _jpeg_decode_upload(who, files, infos, H, W, layout, interval, dev):
    """The one upload: the image records, then the scans, each at a multiple of 16 -> (tensor, bytes of scans, segments, workspace
    bytes per image)."""
    B = len(files)
    S, ws = _jpeg_decode_geometry(H, W, layout, interval)
    offs, at = [], B * _JPEG_DEC_REC.size
    for s in infos:
        offs.append(at)
        at += (s["scan"][1] - s["scan"][0] + 15) & ~15
    scans_bytes = at - B * _JPEG_DEC_REC.size
    if scans_bytes > 0x7fff0000:
        raise ValueError(f"{who}: {scans_bytes} bytes of scans in one call (below 2^31)")
    lib = _lib.load()
    if lib.tup_jpeg_decode_segments(H, W, layout, interval) != S:
        raise RuntimeError(f"{who}: the library counts other segments than the binding")
    host = bytearray(max(at, 16))
    for b, (s, f) in enumerate(zip(infos, files)):
        host[b * _JPEG_DEC_REC.size:(b + 1) * _JPEG_DEC_REC.size] = _jpeg_decode_record(s, f, offs[b] - B * _JPEG_DEC_REC.size)
        host[offs[b]:offs[b] + s["scan"][1] - s["scan"][0]] = f[s["scan"][0]:s["scan"][1]]
    return torch.frombuffer(host, dtype=torch.uint8).to(dev), scans_bytes, S, ws


def _jpeg_decode_index(route, records, scans, scans_bytes, B, H, W, layout, interval, S, segs, status, rounds):
    """Launch 1, by either route."""
    if route == "sync":
        _lib.call("tup_jpeg_decode_index_sync", records, scans, scans_bytes, B, H, W, layout, segs.data_ptr(), status.data_ptr(),
                  None if rounds is None else rounds.data_ptr(), _stream())
    else:
        _lib.call("tup_jpeg_decode_index", records, scans, scans_bytes, B, H, W, layout, interval, S, segs.data_ptr(), status.data_ptr(), _stream())


def jpeg_decode(files, to_tensor=False, out=None, index="auto"):
    """Baseline JPEG files decoded on the GPU in three launches.  files: bytes, or a sequence of bytes whose images share H, W,
    subsampling and restart interval (quantisation and Huffman tables are each image's own).  Returns (frames, status): frames uint8
    [B][H][W][3] RGB, pixel for pixel ``np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))`` (a one-component file gives R = G = B);
    with to_tensor=True fp32 [B][3][H][W], bit-equal to `frames_to_tensor` of the uint8 result and written by the last kernel.
    status int32 [B] on the device: 0 for a scan that decoded completely; otherwise the file is damaged and its pixels are
    unspecified (the other images are unaffected).  out=: the caller's frames tensor.  One upload (the image records and the scans),
    no read-back, no synchronisation.  Restart markers make a file fast: its intervals are walked in parallel.  For a file without
    them launch 1 finds the start of every MCU row, and `index` says how: "serial", one lane's walk through the whole scan; "sync",
    self-synchronising decoding of subsequences of JPEG_SYNC_BYTES bytes by a whole workgroup (a ValueError for files with restart
    markers); "auto", the serial walk.  Frames and status are the same bits on every route.  Everything is validated before any
    launch; what `jpeg_parse` refuses is refused here."""
    files, infos, (H, W, sub, interval), route = _jpeg_decode_files("jpeg_decode", files, index)
    B, layout = len(files), _JPEG_LAYOUT[sub]
    shape, dtype = ((B, 3, H, W), F32) if to_tensor else ((B, H, W, 3), torch.uint8)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError(f"jpeg_decode: out must be a contiguous {dtype} tensor of shape {shape}, got {getattr(out, 'dtype', type(out))} "
                             f"{tuple(getattr(out, 'shape', ()))}")
        _on_current_gpu("jpeg_decode", out, "out")
    elif not torch.cuda.is_available():
        raise RuntimeError("jpeg_decode: the HIP path needs a GPU (no CPU fallback)")
    dev = out.device if out is not None else torch.device("cuda", _cur_dev())
    up, scans_bytes, S, ws = _jpeg_decode_upload("jpeg_decode", files, infos, H, W, layout, interval, dev)
    segs = torch.empty((B, S, 8), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    work = torch.empty((B, ws), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=dev)
    records, scans = up.data_ptr(), up.data_ptr() + B * _JPEG_DEC_REC.size
    _jpeg_decode_index(route, records, scans, scans_bytes, B, H, W, layout, interval, S, segs, status, None)
    _lib.call("tup_jpeg_decode_blocks", records, scans, scans_bytes, B, H, W, layout, interval, S, segs.data_ptr(), status.data_ptr(),
              work.data_ptr(), ws, _stream())
    _lib.call("tup_jpeg_decode_finish", work.data_ptr(), ws, B, H, W, layout, None if to_tensor else out.data_ptr(),
              out.data_ptr() if to_tensor else None, _stream())
    return out, status


def jpeg_scan_index(files, index="auto"):
    """Launch 1 of `jpeg_decode` alone -> (segs int32 [B][S][8], status int32 [B], rounds int32 [B]) on the device.  A segment record
    is {byte, end byte, the bits already read (at the top of the word) and their number, three DC predictors, first MCU}: the reader's
    state at the start of a restart interval, or of an MCU row where the file has none; a number of bits of -1 marks a segment that
    was not placed.  rounds: the sync rounds each image took (index="sync"; otherwise zeros).  The records of "serial" and "sync"
    denote the same bits of the scan with the same predictors and MCU numbers; byte and bits may differ, since a reader that has
    looked further ahead holds more bits."""
    files, infos, (H, W, sub, interval), route = _jpeg_decode_files("jpeg_scan_index", files, index)
    if not torch.cuda.is_available():
        raise RuntimeError("jpeg_scan_index: the HIP path needs a GPU (no CPU fallback)")
    B, layout, dev = len(files), _JPEG_LAYOUT[sub], torch.device("cuda", _cur_dev())
    up, scans_bytes, S, _ = _jpeg_decode_upload("jpeg_scan_index", files, infos, H, W, layout, interval, dev)
    segs = torch.empty((B, S, 8), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    rounds = torch.zeros((B,), dtype=torch.int32, device=dev)
    _jpeg_decode_index(route, up.data_ptr(), up.data_ptr() + B * _JPEG_DEC_REC.size, scans_bytes, B, H, W, layout, interval, S, segs, status, rounds)
    return segs, status, rounds


# ---- PNG decoding of a batch (csrc/png_decode.hip) ----
_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_PNG_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}             # colour type -> bytes per pixel of the filtered stream at 8 bits a sample
_PNG_DEC_REC = struct.Struct("<iiii768s")                  # PngImage: stream offset, length, colour type, channels, palette
PNG_WALKS = ("auto", "token", "wave")
# status of an image (PiStatus, csrc/png_inflate.h): 0, or the first thing wrong in stream order
PNG_STATUS = ("ok", "bad block type", "bad stored length", "invalid code", "symbol without a code", "distance before the start",
              "input exhausted", "output too long", "output too short", "bad filter byte", "Adler-32 mismatch")


def png_parse(data):
    """The chunks of a PNG file, walked on the host: signature, every chunk's CRC-32, IHDR, PLTE, the IDAT payload ranges, IEND ->
    a dict of H, W, color_type, channels (bytes per pixel of the filtered stream: 1, 3, 1, 2, 4 for colour types 0, 2, 3, 4, 6),
    palette (colour type 3: the PLTE entries as bytes, zero-filled to 256 entries; otherwise None), idat [(first byte, end)] in
    order, and stream_bytes = H (1 + channels W).  Ancillary chunks are skipped.  Everything `png_decode` does not decode is a
    ValueError that names what was found: a bit depth other than 8, Adam7 interlace, an unknown colour type, compression or filter
    method, a bad CRC, a cut file, no IDAT, IDAT chunks that are not consecutive, a palette image without PLTE, a zlib header that
    is not deflate with a window of at most 32 KB and no preset dictionary."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise TypeError(f"png_parse: a file is bytes, got {type(data)}")
    data = bytes(data)
    if data[:8] != _PNG_SIGNATURE:
        raise ValueError("png_parse: not a PNG file (no signature)")
    at, n = 8, len(data)
    head, palette, idat, ended, closed = None, None, [], False, False
    while at < n and not ended:
        if at + 12 > n:
            raise ValueError(f"png_parse: the file ends inside a chunk header at byte {at}")
        size, kind = struct.unpack(">I4s", data[at:at + 8])
        if at + 12 + size > n:
            raise ValueError(f"png_parse: the file ends inside the {kind!r} chunk at byte {at}")
        if zlib.crc32(data[at + 4:at + 8 + size]) != struct.unpack(">I", data[at + 8 + size:at + 12 + size])[0]:
            raise ValueError(f"png_parse: bad CRC in the {kind!r} chunk at byte {at}")
        payload = data[at + 8:at + 8 + size]
        if head is None:
            if kind != b"IHDR" or size != 13:
                raise ValueError(f"png_parse: the first chunk is {kind!r} of {size} bytes, not IHDR of 13")
            W, H, depth, ct, comp, filt, lace = struct.unpack(">IIBBBBB", payload)
            if ct not in _PNG_CHANNELS:
                raise ValueError(f"png_parse: colour type {ct}")
            if depth != 8:
                raise ValueError(f"png_parse: bit depth {depth} is not decoded, only 8")
            if lace:
                raise ValueError(f"png_parse: interlace method {lace} (Adam7) is not decoded")
            if comp or filt:
                raise ValueError(f"png_parse: compression method {comp}, filter method {filt} (only 0, 0 exist)")
            if H < 1 or W < 1 or H >= 2 ** 31 or W >= 2 ** 31:
                raise ValueError(f"png_parse: an image of {H} x {W}")
            head = (H, W, ct)
        elif kind == b"IHDR":
            raise ValueError("png_parse: two IHDR chunks")
        elif kind == b"PLTE":
            if palette is not None or idat or size % 3 or not 3 <= size <= 768:
                raise ValueError(f"png_parse: a PLTE chunk of {size} bytes, a second one, or one after IDAT")
            palette = payload + bytes(768 - size)
        elif kind == b"IDAT":
            if closed:
                raise ValueError(f"png_parse: IDAT chunks that are not consecutive (byte {at})")
            idat.append((at + 8, at + 8 + size))
        elif kind == b"IEND":
            ended = True
        elif not kind[0] & 32:
            raise ValueError(f"png_parse: unknown critical chunk {kind!r}")
        if idat and kind != b"IDAT":
            closed = True
        at += 12 + size
    if head is None:
        raise ValueError("png_parse: no IHDR")
    if not ended:
        raise ValueError("png_parse: the file ends before IEND")
    if not idat:
        raise ValueError("png_parse: no IDAT")
    H, W, ct = head
    if ct == 3 and palette is None:
        raise ValueError("png_parse: colour type 3 without PLTE")
    first = b""
    for a, b in idat:                                       # the header's two bytes may lie in two chunks
        first = (first + data[a:b][:2])[:2]
    if len(first) < 2:
        raise ValueError("png_parse: the IDAT chunks hold less than a zlib header")
    if first[0] & 15 != 8 or first[0] >> 4 > 7 or first[1] & 32 or (first[0] * 256 + first[1]) % 31:
        raise ValueError(f"png_parse: zlib header {first.hex()} (deflate with a window up to 32 KB and no preset dictionary is decoded)")
    ch = _PNG_CHANNELS[ct]
    return {"H": H, "W": W, "color_type": ct, "channels": ch, "palette": palette if ct == 3 else None, "idat": idat,
            "stream_bytes": H * (1 + ch * W)}


# What "auto" resolves to: the walk that is faster at B = 1 (scripts/microbench_png_decode.py)
PNG_AUTO_WALK = "wave"


def _png_decode_upload(files, infos, dev):
    """The one upload: the image records, then every image's IDAT payloads joined, each at a multiple of 16 -> (tensor, bytes of
    streams)."""
    B = len(files)
    offs, at = [], B * _PNG_DEC_REC.size
    for s in infos:
        offs.append(at)
        at += (sum(b - a for a, b in s["idat"]) + 15) & ~15
    streams_bytes = at - B * _PNG_DEC_REC.size
    if streams_bytes > 0x7fff0000:
        raise ValueError(f"png_decode: {streams_bytes} bytes of streams in one call (below 2^31)")
    host = bytearray(at)
    for b, (s, f) in enumerate(zip(infos, files)):
        stream = b"".join(bytes(f[a:e]) for a, e in s["idat"])
        host[b * _PNG_DEC_REC.size:(b + 1) * _PNG_DEC_REC.size] = _PNG_DEC_REC.pack(
            offs[b] - B * _PNG_DEC_REC.size, len(stream), s["color_type"], s["channels"], s["palette"] or bytes(768))
        host[offs[b]:offs[b] + len(stream)] = stream
    return torch.frombuffer(host, dtype=torch.uint8).to(dev), streams_bytes


def png_decode(files, to_tensor=False, out=None, walk="auto"):
    """PNG files (8 bits a sample; grey, RGB, palette, grey + alpha, RGBA; no interlace) decoded on the GPU in two launches.  files:
    bytes, or a sequence of 1..65535 bytes whose images share H and W with H (1 + 4 W) < 2^31 (colour type and palette are each
    image's own).  Returns (frames, status): frames uint8 [B][H][W][3] RGB, pixel for pixel
    ``np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))`` (grey: R = G = B; alpha: dropped; palette: looked up, an index past the
    file's PLTE entries gives (0, 0, 0)); with to_tensor=True fp32 [B][3][H][W], bit-equal to `frames_to_tensor` of the uint8 result
    and written by the last kernel.  status int32 [B] on the device: 0 for a stream that inflated to exactly stream_bytes with every
    filter byte in 0..4 and the right Adler-32, otherwise the index into PNG_STATUS of the first thing wrong; the pixels of such an
    image are unspecified, the other images are unaffected, and nothing is read or written outside the image's own stream,
    workspace and frame.  out=: the caller's frames tensor.  One upload (the image records, then every image's IDAT payloads joined,
    each at a multiple of 16 bytes), no read-back, no synchronisation.  walk: "token", one wave decodes one token a round; "wave",
    lane i decodes the token that would begin i bits on and the true chain is followed across the wave; "auto", PNG_AUTO_WALK.
    Frames and status are the same bits on every walk.  Everything is validated before any launch; what `png_parse` refuses is
    refused here."""
    if walk not in PNG_WALKS:
        raise ValueError(f"png_decode: walk must be one of {PNG_WALKS}, got {walk!r}")
    if isinstance(files, (bytes, bytearray, memoryview)):
        files = [files]
    try:
        files = list(files)
    except TypeError:
        raise TypeError(f"png_decode: files must be bytes or a sequence of bytes, got {type(files)}") from None
    B = len(files)
    if not 1 <= B <= 65535:
        raise ValueError(f"png_decode: {B} images in one call (1..65535)")
    if any(not isinstance(f, (bytes, bytearray, memoryview)) for f in files):
        raise TypeError("png_decode: files must be bytes or a sequence of bytes")
    infos = [png_parse(f) for f in files]
    H, W = infos[0]["H"], infos[0]["W"]
    for b, s in enumerate(infos):
        if (s["H"], s["W"]) != (H, W):
            raise ValueError(f"png_decode: the images of a call share H and W; image 0 is {H} x {W}, image {b} is {s['H']} x {s['W']}")
    if H * (1 + 4 * W) >= 2 ** 31:
        raise ValueError(f"png_decode: {H} x {W} has a filtered stream of up to {H * (1 + 4 * W)} bytes (below 2^31)")
    shape, dtype = ((B, 3, H, W), F32) if to_tensor else ((B, H, W, 3), torch.uint8)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError(f"png_decode: out must be a contiguous {dtype} tensor of shape {shape}, got {getattr(out, 'dtype', type(out))} "
                             f"{tuple(getattr(out, 'shape', ()))}")
        _on_current_gpu("png_decode", out, "out")
    elif not torch.cuda.is_available():
        raise RuntimeError("png_decode: the HIP path needs a GPU (no CPU fallback)")
    dev = out.device if out is not None else torch.device("cuda", _cur_dev())
    channels = max(s["channels"] for s in infos)
    ws = ((H * (1 + channels * W) + 15) & ~15) + ((8 * W + 15) & ~15)      # the filtered stream, then two rows of packed pixels
    if ws >= 2 ** 31:
        raise ValueError(f"png_decode: {H} x {W} needs a workspace of {ws} bytes an image (below 2^31)")
    if _lib.load().tup_png_decode_workspace(H, W, channels) != ws:
        raise RuntimeError("png_decode: the library sizes another workspace than the binding")
    up, streams_bytes = _png_decode_upload(files, infos, dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    work = torch.empty((B, ws), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=dev)
    records, streams = up.data_ptr(), up.data_ptr() + B * _PNG_DEC_REC.size
    route = PNG_AUTO_WALK if walk == "auto" else walk
    _lib.call("tup_png_decode_inflate", records, streams, streams_bytes, B, H, W, channels, int(route == "wave"), work.data_ptr(), ws,
              status.data_ptr(), _stream())
    _lib.call("tup_png_decode_finish", records, work.data_ptr(), ws, B, H, W, channels, None if to_tensor else out.data_ptr(),
              out.data_ptr() if to_tensor else None, status.data_ptr(), _stream())
    return out, status


# ---- WindowTransformer: the patch GEMMs in window layout, without reflect padding ----
def _wt_windows(H, W):
    """Windows down and across the floor(H/8) x floor(W/8) token grid."""
    return (H // 8 + 7) // 8, (W // 8 + 7) // 8


def wt_patch_embed(feat, wt, bias):
    """Stride-8 patch conv without padding (floor(H/8) x floor(W/8) tokens) -> fp32 window-layout tokens [M][N]."""
    B, H, W, C = feat.shape
    N = wt.shape[0]
    nwy, nwx = _wt_windows(H, W)
    x = torch.empty((B * nwy * nwx * 64, N), dtype=F32, device=feat.device)
    _lib.call("tup_wt_patch_embed_fwd", _chk(feat, BF16, None, "feat"), _chk(wt, BF16, (N, 4096), "wt"), _chk(bias, F32, (N,), "bias"),
              x.data_ptr(), B, H, W, N, _stream())
    return x


def wt_patch_unembed(x, wt, bias, skip):
    """skip + ConvTranspose(k8, s8)(window_reverse(x)): skip / result NHWC bf16 [B][Ht*8][Wt*8][64]."""
    B, Hs, Ws, C = skip.shape
    K = wt.shape[1]
    nwy, nwx = _wt_windows(Hs, Ws)
    out = torch.empty_like(skip)
    _lib.call("tup_wt_patch_unembed_fwd", _chk(x, F32, (B * nwy * nwx * 64, K), "x"), _chk(wt, BF16, (4096, K), "wt"),
              _chk(bias, F32, (64,), "bias"), _chk(skip, BF16, None, "skip"), out.data_ptr(), B, Hs, Ws, K, _stream())
    return out


# ---- training-step loss ----
def l1_loss_partial(a, b, nblocks=2048):
    n = a.numel()
    part = torch.empty((nblocks,), dtype=F32, device=a.device)
    _lib.call("tup_l1_loss_partial", _chk(a, F32, None, "a"), _chk(b, F32, tuple(a.shape), "b"), part.data_ptr(), n, nblocks, _stream())
    return part


def l1_loss_bwd(a, b, gout):
    ga = torch.empty_like(a)
    _lib.call("tup_l1_loss_bwd", _chk(a, F32, None, "a"), _chk(b, F32, tuple(a.shape), "b"), _chk(gout, F32, None, "gout"),
              ga.data_ptr(), a.numel(), _stream())
    return ga


def wt_patch_wgrad(p, fmap):
    """fp32 [NI][4096] = p^T patches(fmap); p fp32 window-layout tokens [M][NI] over the floor(H/8) x floor(W/8) grid."""
    B, H, W, C = fmap.shape
    NI = p.shape[1]
    nwy, nwx = _wt_windows(H, W)
    M = B * nwy * nwx * 64
    out = _zeros((NI, 4096), p.device)
    _reduce("tup_wt_patch_wgrad", _det_slab(0, M, NI, 4096, p.device), _chk(p, F32, (M, NI), "p"), _chk(fmap, BF16, None, "map"),
            out.data_ptr(), B, H, W, NI)
    return out


def wt_patch_unembed_bwd(gmap, wd):
    """d tokens (window layout, fp32 [M][N]) of the WindowTransformer patch_unembed: the patch_embed GEMM with W^T, no bias."""
    B, H, W, C = gmap.shape
    N = wd.shape[0]
    nwy, nwx = _wt_windows(H, W)
    x = torch.empty((B * nwy * nwx * 64, N), dtype=F32, device=gmap.device)
    _lib.call("tup_wt_patch_embed_fwd", _chk(gmap, BF16, None, "gmap"), _chk(wd, BF16, (N, 4096), "wd"), None,
              x.data_ptr(), B, H, W, N, _stream())
    return x


def wt_patch_embed_bwd(gx, wd, add):
    """d feat_down on the token-covered map = add + scatter(gx wd^T) (the patch_unembed GEMM with W^T, no bias)."""
    B, Hs, Ws, C = add.shape
    K = wd.shape[1]
    out = torch.empty_like(add)
    _lib.call("tup_wt_patch_unembed_fwd", _chk(gx, F32, None, "gx"), _chk(wd, BF16, (4096, K), "wd"), None,
              _chk(add, BF16, None, "add"), out.data_ptr(), B, Hs, Ws, K, _stream())
    return out
