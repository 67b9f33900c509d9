"""What the three training paths (autograd.py = FastTransformer, autograd_rt.py = ResidualTransformer, autograd_wt.py =
WindowTransformer) have in common, once: the transformer-block forward and backward, the decoder backward head, the
conv2 / conv1 backward tail, the stride-2 stem of the two 128-wide models, and the backward of the autograd node.

A model describes its block to blocks_forward / blocks_backward with a BlockSpec (a plain record, DESIGN.md "Shared training
blocks"); everything else a model does differently stays in its own file.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, NamedTuple, Tuple

import torch

from . import ops, packing

BF16 = torch.bfloat16


class BlockSpec(NamedTuple):
    attn_fwd: Callable          # (i, qkv, drop_p, seed) -> (att, lse); closed over the bias fragments or (B, N)
    attn_bwd: Callable          # (i, s, g_att, drop_p, seed) -> g_qkv, or (g_qkv, g_table) when table_grad; None in a forward-only spec
    hidden: int                 # MLP hidden width
    keys: Tuple[str, str]       # packed-weight keys of the two attention projections: ("qkv", "proj") | ("in", "out")
    names: Tuple[str, str, str, str]      # reference names (below the block prefix) of their in-weight, in-bias, out-weight, out-bias
    prefix: str                 # "window_blocks" | "transformer_blocks"
    proj_drop: bool             # dropout behind the output projection (nn.MultiheadAttention has none)
    table_grad: bool            # attn_bwd also returns the relative-position table gradient


def window_block_spec(hidden, frags_t, frags_n=None):
    """The 8x8-window block of FastTransformer (width 192 / 12 heads) and WindowTransformer (128 / 8; ops.window_attn reads the
    head count off qkv): relative-position bias, all three dropout sites.  frags_n: the backward's bias fragments."""
    return BlockSpec(
        attn_fwd=lambda i, qkv, drop_p, seed: ops.window_attn(qkv, frags_t[i], drop_p, seed, save_lse=True),
        attn_bwd=lambda i, s, g_att, drop_p, seed: ops.window_attn_bwd(s["qkv"], g_att, s["att"], s["lse"], frags_n[i], drop_p, seed),
        hidden=hidden, keys=("qkv", "proj"),
        names=(".attn.qkv.weight", ".attn.qkv.bias", ".attn.proj.weight", ".attn.proj.bias"),
        prefix="window_blocks", proj_drop=True, table_grad=True)


def site_seed(seed: int, block: int, site: int) -> int:
    """Per-dropout-site seed (site 0 = attn_drop, 1 = proj_drop, 2 = MLP dropout of block `block`)."""
    return (seed * 0x9E3779B9 + (3 * block + site + 1) * 0x85EBCA6B) & 0xFFFFFFFF


def next_dropout(module):
    """(p, seed) for the next training forward of `module`: p = 0 in eval mode; the seed advances every call and is
    offset by torch's seed and the data-parallel rank so replicas draw different masks."""
    if not module.training or module.dropout_p <= 0.0:
        return 0.0, 0
    module._dropout_calls += 1
    base = (torch.initial_seed() + 7919 * int(os.environ.get("RANK", "0"))) & 0x7FFFFFFF
    return module.dropout_p, (base * 2654435761 + module._dropout_calls) & 0xFFFFFFFF


_ROWMASK_CACHE = {}


def token_rowmask(B, ht, wt, device):
    """uint8 [M]: 1 for the rows of the window-layout token matrix that are real tokens of the ht x wt grid (not window padding)."""
    key = (B, ht, wt, str(device))
    if key not in _ROWMASK_CACHE:
        nwy, nwx = (ht + 7) // 8, (wt + 7) // 8
        ty = (torch.arange(nwy).view(-1, 1, 1, 1) * 8 + torch.arange(8).view(1, 1, -1, 1))
        tx = (torch.arange(nwx).view(1, -1, 1, 1) * 8 + torch.arange(8).view(1, 1, 1, -1))
        m = ((ty < ht) & (tx < wt)).expand(nwy, nwx, 8, 8).reshape(1, -1).expand(B, -1).reshape(-1)
        _ROWMASK_CACHE[key] = m.to(torch.uint8).contiguous().to(device)
    return _ROWMASK_CACHE[key]


# ---- transformer blocks ----
def blocks_forward(spec: BlockSpec, pk, nblocks, xw, drop_p, seed):
    """The training forward of `nblocks` blocks on the token matrix xw.  Returns (xw, what each block's backward needs)."""
    k_in, k_out = spec.keys
    blocks = []
    for i in range(nblocks):
        b = f"b{i}."
        s = {"x_in": xw}
        s["y1"], s["mean1"], s["rstd1"] = ops.layernorm(xw, pk[b + "norm1.w"], pk[b + "norm1.b"], save_stats=True)
        s["qkv"] = ops.gemm_tokens(s["y1"], pk[b + k_in + ".w"], pk[b + k_in + ".b"], "bf16")
        s["att"], s["lse"] = spec.attn_fwd(i, s["qkv"], drop_p, site_seed(seed, i, 0))
        if spec.proj_drop:
            xm = ops.gemm_tokens(s["att"], pk[b + k_out + ".w"], pk[b + k_out + ".b"], "res", res=xw,
                                 drop_p=drop_p, drop_seed=site_seed(seed, i, 1))
        else:
            xm = ops.gemm_tokens(s["att"], pk[b + k_out + ".w"], pk[b + k_out + ".b"], "res", res=xw)
        s["x_mid"] = xm
        s["y2"], s["mean2"], s["rstd2"] = ops.layernorm(xm, pk[b + "norm2.w"], pk[b + "norm2.b"], save_stats=True)
        s["hpre"] = torch.empty((xm.shape[0], spec.hidden), dtype=BF16, device=xm.device)
        s["hid"] = ops.gemm_tokens(s["y2"], pk[b + "fc1.w"], pk[b + "fc1.b"], "gelu", aux=s["hpre"])
        xw = ops.gemm_tokens(s["hid"], pk[b + "fc2.w"], pk[b + "fc2.b"], "res", res=xm,
                             drop_p=drop_p, drop_seed=site_seed(seed, i, 2))
        blocks.append(s)
    return xw, blocks


def blocks_backward(spec: BlockSpec, pk, blocks, g, ready, g_x, drop_p, seed):
    """The blocks in reverse: their parameter gradients into `g` (announced per block through `ready`); returns the gradient of
    the first block's input."""
    k_in, k_out = spec.keys
    w_in, b_in, w_out, b_out = spec.names
    announce = (".mlp.2.bias", ".mlp.2.weight", ".mlp.0.bias", ".mlp.0.weight", ".norm2.weight", ".norm2.bias", b_out, w_out) \
        + ((".attn.relative_position_bias_table",) if spec.table_grad else ()) + (b_in, w_in, ".norm1.weight", ".norm1.bias")
    g_xd = None
    for i in reversed(range(len(blocks))):
        s, p, b = blocks[i], f"{spec.prefix}.{i}", f"b{i}."
        # gradient entering mlp.2's output: through the MLP dropout mask (the residual path keeps g_x itself); from the second
        # block of the loop on the previous LayerNorm1 backward has written it already (fused dropout_bwd)
        if g_xd is not None:
            g_o, g_xd = g_xd, None
        else:
            g_o = ops.dropout_bwd(g_x, drop_p, site_seed(seed, i, 2)) if drop_p > 0 else g_x
        g[p + ".mlp.2.weight"], g[p + ".mlp.2.bias"] = ops.gemm_wgrad_bias(g_o, s["hid"])
        g_h = ops.gemm_tokens(g_o, pk[b + "fc2.wd"], None, "gelu_bwd", aux=s["hpre"])
        del g_o
        g[p + ".mlp.0.weight"], g[p + ".mlp.0.bias"] = ops.gemm_wgrad_bias(g_h, s["y2"])
        g_y2 = ops.gemm_tokens(g_h, pk[b + "fc1.wd"], None, "bf16")
        del g_h
        if spec.proj_drop and drop_p > 0:          # + proj_drop's backward of the result (bf16), in the same pass
            g_xm, g[p + ".norm2.weight"], g[p + ".norm2.bias"], g_o = ops.layernorm_bwd(
                g_y2, s["x_mid"], s["mean2"], s["rstd2"], pk[b + "norm2.w"], gres=g_x, drop=(drop_p, site_seed(seed, i, 1)))
        else:
            g_xm, g[p + ".norm2.weight"], g[p + ".norm2.bias"] = ops.layernorm_bwd(
                g_y2, s["x_mid"], s["mean2"], s["rstd2"], pk[b + "norm2.w"], gres=g_x)
            g_o = g_xm
        g[p + w_out], g[p + b_out] = ops.gemm_wgrad_bias(g_o, s["att"])
        g_att = ops.gemm_tokens(g_o, pk[b + k_out + ".wd"], None, "bf16")
        del g_o
        if spec.table_grad:
            g_qkv, g[p + ".attn.relative_position_bias_table"] = spec.attn_bwd(i, s, g_att, drop_p, site_seed(seed, i, 0))
        else:
            g_qkv = spec.attn_bwd(i, s, g_att, drop_p, site_seed(seed, i, 0))
        g[p + w_in], g[p + b_in] = ops.gemm_wgrad_bias(g_qkv, s["y1"])
        g_y1 = ops.gemm_tokens(g_qkv, pk[b + k_in + ".wd"], None, "bf16")
        del g_qkv, g_att
        if drop_p > 0 and i > 0:          # + the MLP dropout's backward for the block below
            g_x, g[p + ".norm1.weight"], g[p + ".norm1.bias"], g_xd = ops.layernorm_bwd(
                g_y1, s["x_in"], s["mean1"], s["rstd1"], pk[b + "norm1.w"], gres=g_xm, drop=(drop_p, site_seed(seed, i - 1, 2)))
        else:
            g_x, g[p + ".norm1.weight"], g[p + ".norm1.bias"] = ops.layernorm_bwd(
                g_y1, s["x_in"], s["mean1"], s["rstd1"], pk[b + "norm1.w"], gres=g_xm)
        ready(*[p + sfx for sfx in announce])
    return g_x


def blocks_infer(pk, xw, keys, attn, nblocks=None, capture=None):
    """The dropout-free, nothing-saved form of blocks_forward, one kernel per op: xw is updated in place.  The inference route of the
    two 128-wide models, and FastTransformer's when engine.fuse_blocks is off or intermediates are captured.
    attn: (i, qkv) -> att.  nblocks: the block count where pk carries no "nblocks".  capture: a dict that receives, per block,
    block{i} (a copy of xw after the block), block{i}_qkv and block{i}_attn_out."""
    k_in, k_out = keys
    for i in range(pk["nblocks"] if nblocks is None else nblocks):
        b = f"b{i}."
        y = ops.layernorm(xw, pk[b + "norm1.w"], pk[b + "norm1.b"])
        qkv = ops.gemm_tokens(y, pk[b + k_in + ".w"], pk[b + k_in + ".b"], "bf16")
        att = attn(i, qkv)
        ops.gemm_tokens(att, pk[b + k_out + ".w"], pk[b + k_out + ".b"], "res", res=xw, out=xw)
        y = ops.layernorm(xw, pk[b + "norm2.w"], pk[b + "norm2.b"])
        hid = ops.gemm_tokens(y, pk[b + "fc1.w"], pk[b + "fc1.b"], "gelu")
        ops.gemm_tokens(hid, pk[b + "fc2.w"], pk[b + "fc2.b"], "res", res=xw, out=xw)
        if capture is not None:
            capture[f"block{i}"] = xw.clone()
            capture[f"block{i}_qkv"] = qkv
            capture[f"block{i}_attn_out"] = att
    return xw


# ---- the convolutions around the blocks ----
def decoder_backward(pk, sv, g, ready, g_res):
    """decoder_conv2 (64 -> 3), decoder_conv1's ReLU and decoder_conv1 (64 -> 64), from the gradient of the planar residual.
    Returns the gradient of decoder_conv1's input (`comb`)."""
    dwp, db = ops.conv_thin_wgrad(sv["dec"], g_res, True)
    g["decoder_conv2.weight"], g["decoder_conv2.bias"] = dwp.permute(0, 2, 1).reshape(3, 64, 3, 3), db
    g_dec = ops.conv1(g_res, pk["dec2.wd"], None, relu=False, out_mask=sv["dec"])
    ready("decoder_conv2.weight", "decoder_conv2.bias")
    dwp, db = ops.conv_c64_wgrad(sv["comb"], g_dec, 1)
    g["decoder_conv1.weight"], g["decoder_conv1.bias"] = packing.unpack_conv_c64_wgrad(dwp, db, 1)
    g_comb = ops.conv_c64(g_dec, pk["dec1.wd"], None, 1)
    del g_dec
    ready("decoder_conv1.weight", "decoder_conv1.bias")
    return g_comb


def conv_tail_backward(pk, sv, g, ready, g_feat):
    """conv2 and conv1, from the gradient of `feat` (conv2's ReLU already applied).  Returns the gradient of `feat1`."""
    dwp, db = ops.conv_c64_wgrad(sv["feat1"], g_feat, 1)
    g["conv2.weight"], g["conv2.bias"] = packing.unpack_conv_c64_wgrad(dwp, db, 1)
    g_f1 = ops.conv_c64(g_feat, pk["conv2.wd"], None, 1, mask=sv["feat1"])
    g["conv1.weight"], g["conv1.bias"] = ops.conv1_wgrad(sv["x"], g_f1)
    ready("conv2.weight", "conv2.bias", "conv1.weight", "conv1.bias")
    return g_f1


def stem_forward(pk, x, pad=None, crop=False):
    """conv1, conv2 and the stride-2 downsample of the two 128-wide models.  pad: applied to `feat` before the stride-2 conv
    (window_transformer.pad_to_even for odd sizes); crop: the skip connection is feat_down cut to whole 8x8 patches.
    Returns (feat1, feat, feat_down, skip)."""
    feat1 = ops.conv1(x, pk["conv1.w"], pk["conv1.b"], relu=True)
    feat = ops.conv_c64(feat1, pk["conv2.w"], pk["conv2.b"], 1, relu=True)
    if pad is not None:
        feat = pad(feat)
    feat_down = ops.conv_c64(feat, pk["ds.w"], pk["ds.b"], 1, relu=False, in_r=2)
    skip = feat_down
    if crop:
        hd, wd = feat_down.shape[1:3]
        hs, ws = (hd // 8) * 8, (wd // 8) * 8
        if (hs, ws) != (hd, wd):
            skip = feat_down[:, :hs, :ws, :].contiguous()
    return feat1, feat, feat_down, skip


def downsample_backward(pk, sv, g, ready, g_fd):
    """The stride-2 downsample conv, from the gradient of (the possibly cropped) feat_down.  Returns the gradient of `feat`
    at conv2's output size, conv2's ReLU applied."""
    B, hd, wd, _ = sv["feat_down"].shape
    if tuple(g_fd.shape[1:3]) != (hd, wd):          # rows / columns the stride-8 conv and the crop never read get no gradient
        full = torch.zeros((B, hd, wd, 64), dtype=g_fd.dtype, device=g_fd.device)
        full[:, :g_fd.shape[1], :g_fd.shape[2], :] = g_fd
        g_fd = full
    dwp, db = ops.conv_c64_wgrad_s2d(sv["feat"], g_fd, 2)
    g["downsample.weight"], g["downsample.bias"] = packing.unpack_conv_c64_stride2_wgrad(dwp), db
    g_feat = ops.conv_c64(g_fd, pk["ds.wd"], None, 2, mask=sv["feat"])      # 4 sub-pixel tiles -> HR grid, conv2's ReLU
    del g_fd
    if g_feat.shape[1:3] != sv["feat1"].shape[1:3]:          # odd input size: drop the zero row / column the forward's pad appended
        g_feat = g_feat[:, :sv["feat1"].shape[1], :sv["feat1"].shape[2], :].contiguous()
    ready("downsample.weight", "downsample.bias")
    return g_feat


# ---- the autograd node ----
def node_backward(ctx, gout, run, accepts_fused_l1):
    """The backward of a model's autograd node around run(gout, reducer, l1_scale) -> {parameter name: gradient}.
    ctx carries .module, .names and .sv.  Returns (what `run` returned, the gradients in ctx.names order -- through the
    module's gradient reducer, if it has one)."""
    # the fused-L1 hand-off is validated BEFORE the reducer opens its episode: a refusal here must not leave it open
    fused = getattr(ctx, "_fused_l1", None) if accepts_fused_l1 else None
    l1_scale = None
    if fused is not None:
        target, l1_scale, stand_in = fused
        ctx._fused_l1 = None
        if gout.data_ptr() != stand_in.data_ptr() or any(st != 0 for st in gout.stride()):
            raise RuntimeError("l1_loss(..., fuse_into_model_backward=True): the model output has a consumer besides the loss "
                               "(its gradient is not the loss's stand-in); call l1_loss without the fusion")
        gout = target
    reducer = getattr(ctx.module, "_grad_reducer", None)
    if reducer is not None:
        reducer.begin(ctx.names)          # raises if this step's parameters are not in the reducer's layout
    ops.zero_pool_begin(gout.device)
    try:
        own = run(gout, reducer, l1_scale)
    except BaseException:
        if reducer is not None:
            reducer._abort()
        raise
    finally:
        ops.zero_pool_end()
    grads = own if reducer is None else reducer.finish()          # averaged over ranks (views of the flat bucket buffer)
    ctx.sv = None
    outs = []
    for n in ctx.names:
        gr = grads.get(n)
        outs.append(None if gr is None else gr.contiguous())      # reducer: views of this episode's own flat buffer (dp.py)
    return own, tuple(outs)
