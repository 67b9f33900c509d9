"""The fused inference conv1 -> conv2 (csrc/conv12_fused.hip: ops.conv1_compact + ops.conv12_fused) against the two kernels it
replaces (ops.conv1, then ops.conv_c64 with ReLU) on random weights.  The fused kernel feeds conv1's MFMA the same operands in the
same K order and rounds its output the same way, so the results must be bit-identical."""
import pytest
import torch

from transformerupscaler_amd import ops, packing

pytestmark = pytest.mark.gpu


def _weights(seed):
    g = torch.Generator().manual_seed(seed)
    w1 = torch.randn(64, 3, 3, 3, generator=g) / 4
    b1 = torch.randn(64, generator=g) * 0.2
    w2 = torch.randn(64, 64, 3, 3, generator=g) / 24
    b2 = torch.randn(64, generator=g) * 0.1
    p2, pb2 = packing.pack_conv_c64(w2, b2, 1)
    return packing.pack_conv1(w1).cuda(), b1.float().cuda(), p2.cuda(), pb2.cuda()


def _input(B, H, W, seed):
    return torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.mark.parametrize("B,H,W", [(1, 3, 7), (1, 5, 20), (1, 13, 45), (3, 13, 45), (1, 41, 70), (2, 24, 96), (2, 720, 1280)])
def test_conv12_fused_equals_two_kernels(B, H, W):
    w1, b1, w2, b2 = _weights(B * 1000 + H + W)
    x = _input(B, H, W, H * W)
    with torch.no_grad():
        ref = ops.conv_c64(ops.conv1(x, w1, b1, relu=True), w2, b2, 1, relu=True)
        got = ops.conv12_fused(ops.conv1_compact(x), H, W, w1, b1, w2, b2)
    torch.cuda.synchronize()
    assert got.shape == ref.shape == (B, H, W, 64)
    assert torch.equal(got, ref), (got.float() - ref.float()).abs().max().item()


def test_conv12_fused_batch_equals_single():
    w1, b1, w2, b2 = _weights(11)
    H, W = 37, 70
    x = _input(3, H, W, 5)
    with torch.no_grad():
        yb = ops.conv12_fused(ops.conv1_compact(x), H, W, w1, b1, w2, b2)
        ys = torch.cat([ops.conv12_fused(ops.conv1_compact(x[i:i + 1].contiguous()), H, W, w1, b1, w2, b2) for i in range(3)])
    assert torch.equal(yb, ys)


@pytest.mark.parametrize("B,H,W", [(1, 3, 7), (2, 13, 45), (1, 40, 96)])
def test_conv1_compact_matches_torch(B, H, W):
    x = _input(B, H, W, 3) * 4 - 2
    with torch.no_grad():
        xc = ops.conv1_compact(x)
    Hp, Wp = (H + 7) // 8 * 8 + 4, (W + 31) // 32 * 32 + 4
    ref = torch.zeros((B, Hp, Wp, 4), dtype=torch.bfloat16, device=x.device)
    ref[:, 2:2 + H, 2:2 + W, :3] = x.permute(0, 2, 3, 1).to(torch.bfloat16)
    assert xc.shape == ref.shape
    assert torch.equal(xc, ref)


@pytest.mark.parametrize("scale", [2, 3])
def test_engine_routes_conv12(det_sd, scale):
    """engine.fuse_conv12 on / off over the whole forward: the same output, bit for bit."""
    import importlib
    from transformerupscaler_amd import engine
    model = importlib.import_module("models.FastTransformer.model").TransformerModel()
    model.load_state_dict(det_sd, strict=False)
    model = model.cuda().eval()
    x = torch.rand((2, 3, 40, 72), generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad():
        y_f = model(x, upscale_factor=scale)
        engine.fuse_conv12 = False
        try:
            y_u = model(x, upscale_factor=scale)
        finally:
            engine.fuse_conv12 = True
    assert torch.equal(y_f, y_u)
