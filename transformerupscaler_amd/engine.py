"""Forward orchestration of the FastTransformer path over the HIP kernels.

Mirrors TransformerModel.forward (reference models/FastTransformer/model.py:231-327) stage by
stage; every stage is one C-ABI launch (ops.py).  Activations: NHWC bf16 for the 64-channel
maps, fp32 planar for the 3-channel images, fp32 residual stream for the tokens.
"""
from __future__ import annotations

import contextlib
import os

import math
from typing import Dict, Optional, Tuple

import torch

from . import ops
from .blocks_train import blocks_infer
from .weights import BLOCKS, VALID_SCALES, upsampler_layout


# Optional per-stage timing hook (bench.py installs one): callable(name) -> context manager.
stage_timer = None


_NO_TIMER = contextlib.nullcontext()


def stage(timer, name: str):
    """Context manager around one timed stage: timer(name), or nothing when no timer is installed (autograd_rt has its own hook)."""
    return timer(name) if timer is not None else _NO_TIMER


def _stage(name: str):
    return stage(stage_timer, name)


def resolve_scale(h: int, w: int, res_out, upscale_factor: Optional[int]):
    """model.py:245-248 + the ValueError of utils.py:96-97."""
    if upscale_factor is not None:
        res_out = (h * upscale_factor, w * upscale_factor)
    else:
        upscale_factor = math.ceil(max(res_out[0] / h, res_out[1] / w))
    if upscale_factor not in VALID_SCALES:
        raise ValueError(f"Requested scale={upscale_factor} was not built.")
    return (int(res_out[0]), int(res_out[1])), int(upscale_factor)


blocks_in_one_launch = True     # constant: both block kernels run the six blocks as one launch; bench.py reads it for its launch count
# inference (A/B attribute): large launches take the streamed 32x32x16 kernel (csrc/block_stream.hip); False = the 16x16x32 whole-block
# kernel (csrc/fused_attn.hip) at every size
stream_blocks = True
# the streamed kernel's workgroup carries four windows (one workgroup per CU): launches that would leave most CUs without one stay on the
# 16x16x32 kernel, whose small-launch form runs one window per workgroup (the 720p -> 4K overlay frame: 240 windows; config 4: 540)
STREAM_MIN_WINDOWS = 512
# the streamed kernel hands its result to patch_unembed as bf16 tokens (the rounding that GEMM applies on load anyway; A/B attribute)
stream_bf16_tokens = True
fuse_blocks = True      # inference: the six blocks in one launch of a whole-block kernel; False = one kernel per op (blocks_infer)
fuse_tail = True        # inference: fused output tail (csrc/tail_fused.hip)
stream_tail = True     # A/B attribute; last stage x2: the register-streaming tail (csrc/tail_stream.hip) [+ separable Resize]
# inference (A/B attribute): decoder_conv1 + decoder_conv2 as one conv with decoder_conv2 in its epilogue plus a finishing launch
# (csrc/decoder_fused.hip); the 64-channel map between them never reaches HBM.  Rides on fuse_tail so that the unfused arm of the
# fused-vs-unfused tests runs the two-kernel decoder.
fuse_decoder = True
# inference (A/B attribute): conv1 recomputed per conv2 tile inside conv2's idle wave group from a compact bf16 copy of the input
# (csrc/conv12_fused.hip); the 64-channel conv1 map never reaches HBM
fuse_conv12 = True
# inference (A/B attribute): at scale 2 the streaming tail reads `residual` straight from the fused decoder, so the decoder's finishing
# launch does not run and the tail adds the unfinished pieces where it reads them (csrc/tail_stream.hip, PARTS).  Bit-identical.
fuse_decoder_finish = True


def _block_operands(pk, i, bias_frags):
    """One row of ops.block_table: the whole-block kernels take norm1 / norm2 folded into attn.qkv / mlp.0 (packing.fold_layernorm)."""
    return (pk[f"b{i}.qkv.whn"], pk[f"b{i}.qkv.bhn"], bias_frags[i], pk[f"b{i}.proj.wpp"], pk[f"b{i}.proj.b"],
            pk[f"b{i}.fc1.wfqn"], pk[f"b{i}.fc1.bqn"], pk[f"b{i}.fc2.wh4"], pk[f"b{i}.fc2.b"])


def transformer_blocks(pk: Dict[str, torch.Tensor], x: torch.Tensor, bias_frags, capture=None, bf16_out: bool = False):
    """x: fp32 [M][192] window layout, updated in place.  model.py:153-172 x6.  Three routes: the streamed kernel for large launches,
    the 16x16x32 whole-block kernel below that, one kernel per op when fuse_blocks is off or `capture` wants the intermediates.
    bf16_out (the caller feeds the result to patch_unembed, whose GEMM rounds its operand to bf16 anyway): the streamed kernel then
    returns the tokens as a bf16 tensor (the same rounding, half the bytes to write and to read back); every other route ignores it."""
    if not fuse_blocks or capture is not None:
        return blocks_infer(pk, x, ("qkv", "proj"), lambda i, qkv: ops.window_attn(qkv, bias_frags[i]), nblocks=BLOCKS, capture=capture)
    if stream_blocks and x.shape[0] // 64 >= STREAM_MIN_WINDOWS:
        # all six blocks in ONE launch of the streamed kernel (csrc/block_stream.hip)
        table = ops.stream_table([tuple(pk[f"b{i}.stream.{j}"] for j in range(7)) for i in range(BLOCKS)])
        return ops.blocks_stream(x, table, out_bf16=bf16_out and stream_bf16_tokens)
    # all six blocks in ONE launch (csrc/fused_attn.hip)
    return ops.fused_blocks32(x, ops.block_table([_block_operands(pk, i, bias_frags) for i in range(BLOCKS)]))


def forward(pk: Dict[str, torch.Tensor], bias_frags, x: torch.Tensor, scale: int, res_out: Tuple[int, int],
            require_ratio: bool = True, capture: Optional[dict] = None, fuse_branch_a: bool = True) -> torch.Tensor:
    cap = capture
    x = x.contiguous().float()
    B, _, H, W = x.shape
    # (measured and dropped in round 4: conv1 -> conv2 and decoder_conv1 -> decoder_conv2 one or two images at a time, so that the
    # 118 MB-per-image map between them would come back from the 256 MB memory-side cache: 0.693 -> 0.74-0.80 ms and 0.675 ->
    # 0.70-0.72 ms per forward -- the consumers are not faster on cache-resident input, and eight small launches cost their tails)
    if fuse_conv12 and cap is None:
        with _stage("conv1"):
            xc = ops.conv1_compact(x)
        with _stage("conv2"):
            feat = ops.conv12_fused(xc, H, W, pk["conv1.w"], pk["conv1.b"], pk["conv2.w"], pk["conv2.b"])
        del xc
    else:
        with _stage("conv1"):
            feat1 = ops.conv1(x, pk["conv1.w"], pk["conv1.b"], relu=True)
        with _stage("conv2"):
            feat = ops.conv_c64(feat1, pk["conv2.w"], pk["conv2.b"], 1, relu=True)
        del feat1
    # branch A: Upsampler + up1_conv (conv, no bias, ReLU)
    stages = upsampler_layout(scale)
    up = feat
    if fuse_branch_a and "bra.w" in pk:
        # all but the last stage explicitly; the last conv + PixelShuffle + up1_conv as one composed 5x5 conv
        for si, (_, r) in enumerate(stages[:-1]):
            up = ops.conv_c64(up, pk[f"up1.{si}.w"], pk[f"up1.{si}.b"], r, relu=False)
        with _stage("branch_a"):
            upscaled_input = ops.branch_a_composed(up, pk["bra.w"], pk["bra.b"], pk["bra.wv"], pk["bra.bv"], stages[-1][1])
    else:
        for si, (_, r) in enumerate(stages):
            with _stage(f"up1.{si}"):
                up = ops.conv_c64(up, pk[f"up1.{si}.w"], pk[f"up1.{si}.b"], r, relu=False)
        upscaled_input = ops.conv_c64_thin(up, pk["up1_conv.w"], None, 3, relu=True)
        if cap is not None:
            cap["up1"] = up
    if cap is not None:
        cap["feat"] = feat; cap["upscaled_input"] = upscaled_input
    del up
    # branch B: tokens
    with _stage("patch_embed"):
        xw = ops.patch_embed(feat, pk["pe.w"], pk["pe.b"])
    if cap is not None:
        cap["win_in"] = xw.clone()
    with _stage("blocks"):
        xw = transformer_blocks(pk, xw, bias_frags, cap, bf16_out=cap is None)
    with _stage("unembed"):
        combined = ops.patch_unembed(xw, pk["pu.w"], pk["pu.b"], feat)
    hs, ws = H * scale, W * scale
    # model.py:323: `res_out != (out.shape[2], out.shape[2])` -- the (H, H) quirk is kept; Resize to an
    # identical size is the identity.
    needs_resize = bool(require_ratio) and tuple(res_out) != (hs, hs) and tuple(res_out) != (hs, ws)
    fu = upsampler_layout(scale)
    tail_out_hw = tuple(res_out) if needs_resize else None
    parts = None
    if fuse_decoder and fuse_tail and cap is None and "dec2.wz" in pk:
        # the streaming tail is the decoder's only reader (one final_upscale stage of x2): it takes the unfinished pieces
        unfinished = (fuse_decoder_finish and stream_tail and len(fu) == 1 and fu[0][1] == 2 and "tail.wfu_t" in pk
                      and ops.tail_stream_fits(B, H, W, tail_out_hw))
        with _stage("decoder"):
            residual = ops.decoder_fused(combined, pk["dec1.w"], pk["dec1.b"], pk["dec2.wz"], pk["dec2.b"], finish=not unfinished)
        if unfinished:
            parts, residual = residual, residual[0]
    else:
        with _stage("dec1"):
            dec = ops.conv_c64(combined, pk["dec1.w"], pk["dec1.b"], 1, relu=True)
        with _stage("dec2"):
            residual = ops.conv_c64_thin(dec, pk["dec2.w"], pk["dec2.b"], 3, relu=False)
    if cap is not None:
        cap["combined"] = combined; cap["dec"] = dec; cap["residual"] = residual
    t = residual
    if fuse_tail and cap is None:
        for si, (_, r) in enumerate(fu[:-1]):
            t = ops.conv_planar(t, pk[f"fu.{si}.w"], pk[f"fu.{si}.b"], r)
        li = len(fu) - 1
        if (stream_tail and fu[li][1] == 2 and "tail.wfu_t" in pk
                and ops.tail_stream_fits(t.shape[0], t.shape[2], t.shape[3], tail_out_hw)):
            # (parts: `t` is then the unfinished `part` plane, which the kernel reads with the other pieces; they stay referenced
            # by `parts` until the tail is enqueued)
            with _stage("tail"):
                out = ops.tail_stream_r2(t, pk["tail.wfu_t"], pk[f"fu.{li}.b"], pk["tail.wfc_t"], pk["fuc.b"], upscaled_input,
                                         clamp=True, out_hw=tail_out_hw, parts=parts)
                if out is None:        # a Resize with more than 4 taps per output: pre-resize sums, then the separable Resize kernel
                    out = ops.tail_stream_r2(t, pk["tail.wfu_t"], pk[f"fu.{li}.b"], pk["tail.wfc_t"], pk["fuc.b"], upscaled_input,
                                             clamp=False, parts=parts)
                    out = ops.resize_aa(out, tuple(res_out), clamp=True)
            return out
        assert parts is None       # the unfinished pieces go to the streaming tail only
        with _stage("tail"):
            out = ops.tail_fused(t, pk[f"fu.{li}.w"], pk[f"fu.{li}.b"], pk["fuc.w"], pk["fuc.b"], upscaled_input, fu[li][1],
                                 tuple(res_out) if needs_resize else (hs, ws), clamp=True)
        return out
    for si, (_, r) in enumerate(fu):
        t = ops.conv_planar(t, pk[f"fu.{si}.w"], pk[f"fu.{si}.b"], r)
    out = ops.conv_planar(t, pk["fuc.w"], pk["fuc.b"], 1, add=upscaled_input, clamp=not needs_resize)
    if cap is not None:
        cap["sum"] = out
    if needs_resize:
        out = ops.resize_aa(out, res_out, clamp=True)
    return out
