"""Training path of the ResidualTransformer plugin (BASELINE.json config 5): forward that keeps what the hand-written
backward needs, and the backward itself -- every gradient the reference gets from ``loss.backward()`` through
models/ResidualTransformer/model.py:121-165 (train.py:138), computed by the HIP kernels of include/tupscale_hip.h.

torch.autograd sees one node per model call.  The blocks, the decoder head, the stride-2 stem and the node's backward are
blocks_train.py's; this file holds what is ResidualTransformer's own: global attention over the 3600 tokens, pos_embed, the
bicubic global residual.
"""
from __future__ import annotations

from typing import Dict

import torch

from . import ops
from .blocks_train import (BlockSpec, blocks_backward, blocks_forward, conv_tail_backward, decoder_backward, downsample_backward,
                           node_backward, stem_forward)
from .engine import stage

# Optional timing hook (bench.py --mode rt installs one): callable(name) -> context manager around the attention launches
# ("rt_attn_fwd" = rt_attention_kernel, "rt_attn_bwd" = the dq + dkv pair).
stage_timer = None


def _block_spec(B, N):
    """ResidualTransformer's block for blocks_train: nn.MultiheadAttention at width 128 -- packed in_proj / out_proj, global
    attention, no relative-position table and no dropout behind the out-projection."""
    def attn_fwd(i, qkv, drop_p, seed):
        with stage(stage_timer, "rt_attn_fwd"):
            return ops.rt_attention(qkv, B, N, save_lse=True, drop_p=drop_p, drop_seed=seed)

    def attn_bwd(i, s, g_att, drop_p, seed):
        with stage(stage_timer, "rt_attn_bwd"):
            return ops.rt_attention_bwd(s["qkv"], s["att"], g_att, s["lse"], B, N, drop_p=drop_p, drop_seed=seed)
    return BlockSpec(
        attn_fwd=attn_fwd, attn_bwd=attn_bwd,
        hidden=512, keys=("in", "out"),
        names=(".attn.in_proj_weight", ".attn.in_proj_bias", ".attn.out_proj.weight", ".attn.out_proj.bias"),
        prefix="transformer_blocks", proj_drop=False, table_grad=False)


def forward_train(pk, x, res_out, drop_p: float, seed: int):
    B, _, H, W = x.shape
    x = x.contiguous().float()
    sv = {"x": x, "drop_p": drop_p, "seed": seed}
    sv["feat1"], sv["feat"], sv["feat_down"], _ = stem_forward(pk, x)
    feat_down = sv["feat_down"]
    xw = ops.rt_patch_embed(feat_down, pk["pe.w"], pk["pe.b"], pk["pos"])
    xw, sv["blocks"] = blocks_forward(_block_spec(B, xw.shape[0] // B), pk, pk["nblocks"], xw, drop_p, seed)
    sv["xw_out"] = xw
    comb = ops.rt_patch_unembed(xw, pk["pu.w"], pk["pu.b"], feat_down)
    dec = ops.conv_c64(comb, pk["dec1.w"], pk["dec1.b"], 1, relu=True)
    residual = ops.conv_c64_thin(dec, pk["dec2.w"], pk["dec2.b"], 3, relu=False)
    out = ops.rt_bicubic_sum(x, residual, tuple(int(v) for v in res_out), clamp=True)
    sv["comb"], sv["dec"], sv["out"] = comb, dec, out          # the clamp gate is read back from the output itself
    return out, sv


def backward_train(pk, sv, gout, reducer=None, l1_scale=None) -> Dict[str, torch.Tensor]:
    g: Dict[str, torch.Tensor] = {}

    def ready(*names):
        if reducer is not None:
            reducer.on_ready(list(names), g)

    x = sv["x"]
    B, _, H, W = x.shape
    hd, wd = H // 2, W // 2
    N = (hd // 8) * (wd // 8)
    # ---- clamp + bicubic (only the residual branch carries parameters); l1_scale: gout is the target of an L1 loss on the
    #      output and the loss gradient is formed inside the kernel (autograd.l1_loss(..., fuse_into_model_backward=True)) ----
    gout = gout.contiguous().float()
    g_res = ops.rt_bicubic_bwd(gout, sv["out"], (hd, wd), l1_scale=None if l1_scale is None else l1_scale[:1])
    g_comb = decoder_backward(pk, sv, g, ready, g_res)
    # ---- patch_unembed (+ skip) ----
    g["patch_unembed.bias"] = ops.colsum(g_comb.view(-1, 64))
    g["patch_unembed.weight"] = ops.rt_patch_wgrad(sv["xw_out"], g_comb).view(128, 8, 8, 64).permute(0, 3, 1, 2)
    g_x = ops.rt_patch_unembed_bwd(g_comb, pk["pu.wd"])
    ready("patch_unembed.weight", "patch_unembed.bias")
    # ---- transformer blocks (reverse) ----
    g_x = blocks_backward(_block_spec(B, N), pk, sv["blocks"], g, ready, g_x, sv["drop_p"], sv["seed"])
    # ---- pos_embed, patch_embed ----
    g["pos_embed"] = g_x.view(B, N, 128).sum(0, keepdim=True)
    g["patch_embed.bias"] = ops.colsum(g_x)
    g["patch_embed.weight"] = ops.rt_patch_wgrad(g_x, sv["feat_down"]).view(128, 8, 8, 64).permute(0, 3, 1, 2)
    g_fd = ops.rt_patch_embed_bwd(g_x, pk["pe.wd"], add=g_comb)            # + skip gradient
    del g_x, g_comb
    ready("pos_embed", "patch_embed.weight", "patch_embed.bias")
    # ---- downsample (stride-2 conv), conv2, conv1 ----
    g_feat = downsample_backward(pk, sv, g, ready, g_fd)
    del g_fd
    conv_tail_backward(pk, sv, g, ready, g_feat)
    return g


class _ResidualTransformerFn(torch.autograd.Function):
    accepts_fused_l1 = True          # autograd.l1_loss may hand (target, scale) to this node instead of a gradient tensor

    @staticmethod
    def forward(ctx, module, x, res_out, names, *params):
        pk = module.packed(backward=True)
        drop_p, seed = module._next_dropout()
        out, sv = forward_train(pk, x, res_out, drop_p, seed)
        ctx.module, ctx.names, ctx.sv, ctx.pk = module, names, sv, pk
        return out

    @staticmethod
    def backward(ctx, gout):
        def run(gout, reducer, l1_scale):
            return backward_train(ctx.pk, ctx.sv, gout, reducer, l1_scale=l1_scale)
        return (None, None, None, None) + node_backward(ctx, gout, run, _ResidualTransformerFn.accepts_fused_l1)[1]


def residual_transformer_function(module, x, res_out):
    named = dict(module.named_parameters())
    names = [n for n, p in named.items() if p.requires_grad]
    return _ResidualTransformerFn.apply(module, x, tuple(res_out), names, *[named[n] for n in names])
