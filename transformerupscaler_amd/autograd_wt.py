"""Training path of the WindowTransformer plugin: forward that keeps what the hand-written backward needs, and the
backward itself -- every gradient the reference gets from ``loss.backward()`` through models/WindowTransformer/model.py:
225-305, computed by the HIP kernels of include/tupscale_hip.h; torch.autograd sees one node per model call.  The blocks,
the decoder head, the stride-2 stem and the node's backward are blocks_train.py's; this file holds what is WindowTransformer's
own: 8x8 window attention at width 128 / 8 heads, the pad to even sizes, the crop to whole patches, the bicubic global residual.
"""
from __future__ import annotations

from typing import Dict

import torch

from . import ops
from .blocks_train import (blocks_backward, blocks_forward, conv_tail_backward, decoder_backward, downsample_backward, node_backward,
                           stem_forward, token_rowmask, window_block_spec)
from .window_transformer import pad_to_even


def forward_train(pk, frags_t, x, res_out, drop_p: float, seed: int):
    B, _, H, W = x.shape
    x = x.contiguous().float()
    sv = {"x": x, "drop_p": drop_p, "seed": seed}
    # odd sizes: + one zero row / column before the stride-2 conv; the skip is cropped to whole patches
    sv["feat1"], sv["feat"], sv["feat_down"], skip = stem_forward(pk, x, pad=pad_to_even, crop=True)
    sv["skip"] = skip
    xw = ops.wt_patch_embed(sv["feat_down"], pk["pe.w"], pk["pe.b"])
    xw, sv["blocks"] = blocks_forward(window_block_spec(512, frags_t), pk, pk["nblocks"], xw, drop_p, seed)
    sv["xw_out"] = xw
    comb = ops.wt_patch_unembed(xw, pk["pu.w"], pk["pu.b"], skip)
    dec = ops.conv_c64(comb, pk["dec1.w"], pk["dec1.b"], 1, relu=True)
    residual = ops.conv_c64_thin(dec, pk["dec2.w"], pk["dec2.b"], 3, relu=False)
    out = ops.rt_bicubic_sum(x, residual, tuple(int(v) for v in res_out), clamp=True)
    sv["comb"], sv["dec"], sv["out"] = comb, dec, out
    return out, sv


def backward_train(pk, frags_t, frags_n, sv, gout, reducer=None) -> Dict[str, torch.Tensor]:
    g: Dict[str, torch.Tensor] = {}

    def ready(*names):
        if reducer is not None:
            reducer.on_ready(list(names), g)

    x = sv["x"]
    B, _, H, W = x.shape
    hd, wd = (H + 1) // 2, (W + 1) // 2
    hs, ws = sv["skip"].shape[1], sv["skip"].shape[2]
    gout = gout.contiguous().float()
    g_res = ops.rt_bicubic_bwd(gout, sv["out"], (hs, ws))
    g_comb = decoder_backward(pk, sv, g, ready, g_res)
    # ---- patch_unembed (+ cropped skip) ----
    g["patch_unembed.bias"] = ops.colsum(g_comb.view(-1, 64))
    g["patch_unembed.weight"] = ops.wt_patch_wgrad(sv["xw_out"], g_comb).view(128, 8, 8, 64).permute(0, 3, 1, 2)
    g_x = ops.wt_patch_unembed_bwd(g_comb, pk["pu.wd"])
    ready("patch_unembed.weight", "patch_unembed.bias")
    # ---- window blocks (reverse) ----
    g_x = blocks_backward(window_block_spec(512, frags_t, frags_n), pk, sv["blocks"], g, ready, g_x, sv["drop_p"], sv["seed"])
    # ---- patch_embed (real tokens only: the zero pad carries no bias, model.py:256-263) ----
    g["patch_embed.bias"] = ops.colsum(g_x, rowmask=token_rowmask(B, hd // 8, wd // 8, x.device))
    g["patch_embed.weight"] = ops.wt_patch_wgrad(g_x, sv["feat_down"]).view(128, 8, 8, 64).permute(0, 3, 1, 2)
    g_fd = ops.wt_patch_embed_bwd(g_x, pk["pe.wd"], add=g_comb)                  # + skip gradient, on the cropped map
    del g_x, g_comb
    ready("patch_embed.weight", "patch_embed.bias")
    # ---- downsample (stride-2 conv; zero-fills what the crop cut, trims what the pad appended), conv2, conv1 ----
    g_feat = downsample_backward(pk, sv, g, ready, g_fd)
    del g_fd
    conv_tail_backward(pk, sv, g, ready, g_feat)
    return g


class _WindowTransformerFn(torch.autograd.Function):
    # no fused L1: backward_train above takes no L1 target, so autograd.l1_loss always hands this node a materialised gradient.
    # Accepting the hand-off would change what a training step launches; the node's shared backward only keeps what was there.
    accepts_fused_l1 = False

    @staticmethod
    def forward(ctx, module, x, res_out, names, *params):
        pk, frags_t, frags_n = module.packed(backward=True)
        drop_p, seed = module._next_dropout()
        out, sv = forward_train(pk, frags_t, x, res_out, drop_p, seed)
        ctx.module, ctx.names, ctx.sv, ctx.pk, ctx.frags = module, names, sv, pk, (frags_t, frags_n)
        return out

    @staticmethod
    def backward(ctx, gout):
        def run(gout, reducer, l1_scale):
            return backward_train(ctx.pk, ctx.frags[0], ctx.frags[1], ctx.sv, gout, reducer)
        return (None, None, None, None) + node_backward(ctx, gout, run, _WindowTransformerFn.accepts_fused_l1)[1]


def window_transformer_function(module, x, res_out):
    named = dict(module.named_parameters())
    names = [n for n, p in named.items() if p.requires_grad]
    return _WindowTransformerFn.apply(module, x, tuple(res_out), names, *[named[n] for n in names])
