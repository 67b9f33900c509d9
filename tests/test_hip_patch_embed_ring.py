"""patch_embed_kernel's operand rings (csrc/gemm_tokens.hip).

The kernel streams one patch pixel (64 channels) per K-step: token tiles two steps ahead in a three-slot LDS ring, weight tiles one
step ahead in a two-slot ring, the DMA pieces of both issued between the step's MFMAs, a counted vmcnt in front of one barrier per
step and a vmcnt(0) for the last step alone.  What can go wrong is a stage in the wrong slot, a stage read one step early, or a
wait that lets a reader in before the DMA has landed.

Operands are the integers of tests/_gemm_exact_ref.py (amplitude 7, every sum an integer below 2**24): the fp32 result is exact in
any summation order, so every comparison is torch.equal against torch on the CPU.  Per shape one dense case (every patch pixel and
channel of map and weights is an independent draw, so a stage that reaches the MFMAs from the wrong slot changes the result), then
the weights live in ONE K-step only, swept over steps 0, 1, 2, 3 (prologue, first wrap of the weight ring at 2 and of the token
ring at 3) and the last two (the step that issues no token stage and the vmcnt(0) tail): the result is then exactly the product of
that step's token stage with that step's weight stage, and any other stage read in its place gives zeros or a foreign product.

Shapes: (1, 8, 8) one valid token in one workgroup beside 63 zero rows; (2, 19, 70) reflect padding and partial windows on both
axes; (1, 72, 136) two workgroups, the second with 128 of its 256 rows; (3, 64, 64) no padding at all.

The A_BF16 instances (plain bf16 rows, N = 192, M >= 4096) run nk = 9 and nk = 12 steps through ops.gemm_tokens at K = 576 and 768."""
import pytest
import torch
import torch.nn.functional as F

import _exact_ref as R          # tests/ is on sys.path (rootdir-less test modules)
import _gemm_exact_ref as G

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
EMBED_SHAPES = [(1, 8, 8), (2, 19, 70), (1, 72, 136), (3, 64, 64)]
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else None


def ring_steps(nk):
    return [0, 1, 2, 3, nk - 2, nk - 1]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from transformerupscaler_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _pack(w2d, dev):
    from transformerupscaler_amd import packing
    return packing.pack_linear(w2d).to(dev)


def _embed_ref(m, w, b):
    """ops.patch_embed in fp64: reflect padding to multiples of 8, stride-8 conv + bias, window layout with zero rows for padded tokens."""
    H, W = m.shape[2:]
    ph, pw = -H % 8, -W % 8
    mp = F.pad(m.double(), (0, pw, 0, ph), mode="reflect") if (ph or pw) else m.double()
    return G.to_windows(F.conv2d(mp, w.double(), b.double(), stride=8).permute(0, 2, 3, 1))


@pytest.mark.parametrize("shape", EMBED_SHAPES, ids=ids)
def test_patch_embed_every_stage(dev, shape):
    from transformerupscaler_amd import ops
    B, H, W = shape
    s = 9500 + H
    m, w, b = G.ints((B, 64, H, W), s, G.AMP), G.ints((192, 64, 8, 8), s + 1, G.AMP), G.ints((192,), s + 2, G.AMP)
    feat, bias = R.nhwc_bf16(m).to(dev), b.to(dev)
    rows = B * (((H + 7) // 8 + 7) // 8) * (((W + 7) // 8 + 7) // 8) * 64
    for kc in [None] + ring_steps(64):
        wk = w
        if kc is not None:                      # K-step kc = patch pixel (kc >> 3, kc & 7)
            wk = torch.zeros_like(w)
            wk[:, :, kc >> 3, kc & 7] = w[:, :, kc >> 3, kc & 7]
        ref = _embed_ref(m, wk, b)
        assert ref.shape == (rows, 192) and float(ref.abs().max()) < 2 ** 24
        got = ops.patch_embed(feat, _pack(wk.permute(0, 2, 3, 1).reshape(192, 4096), dev), bias).cpu()      # k = (i*8+j)*64 + c
        bad = got != ref.float()
        assert torch.equal(got, ref.float()), \
            f"patch_embed {shape}, weights live in K-step {kc}: {int(bad.sum())} of {bad.numel()} differ, first at {bad.nonzero()[:4].tolist()}"


@pytest.mark.parametrize("K", [576, 768])
def test_long_k_linear_every_stage(dev, K):
    """patch_embed_kernel<3, A_BF16, E_BF16 / E_RES_F32>: nk = K / 64 = 9 and 12; 17 workgroups, the last with 37 rows."""
    from transformerupscaler_amd import ops
    M, N, nk = 4133, 192, K // 64
    a, w, b, res = G.ints((M, K), 9600 + K, G.AMP), G.ints((N, K), 9601 + K, G.AMP), G.ints((N,), 9602 + K, G.AMP), G.ints((M, N), 9603 + K, G.AMP)
    a16, bias, resd = a.to(BF16).to(dev), b.to(dev), res.to(dev)
    for kc in [None] + ring_steps(nk):
        wk = w
        if kc is not None:
            wk = torch.zeros_like(w)
            wk[:, kc * 64:(kc + 1) * 64] = w[:, kc * 64:(kc + 1) * 64]
        y = a.double() @ wk.double().t() + b.double()
        got = ops.gemm_tokens(a16, _pack(wk, dev), bias, "res", res=resd)
        assert torch.equal(got.cpu(), (y + res.double()).float()), f"gemm_tokens res K={K}, weights live in K-step {kc}"
        if kc is None:
            assert 0.05 < R.share_above_256(y) < 0.95               # the bf16 epilogue really rounds
            got = ops.gemm_tokens(a16, _pack(wk, dev), bias, "bf16")
            assert torch.equal(got.cpu(), y.to(BF16)), f"gemm_tokens bf16 K={K}"
