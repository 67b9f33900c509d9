"""The fused inference decoder (csrc/decoder_fused.hip, ops.decoder_fused) against the two-kernel decoder (decoder_conv1 by
tup_conv3x3_c64_fwd out_mode 0, decoder_conv2 by out_mode 1) on random weights.  Both round the 64-channel map to bf16 the same
way; only the fp32 summation order of decoder_conv2 differs, so the bound is tight."""
import pytest
import torch

from transformerupscaler_amd import ops, packing

pytestmark = pytest.mark.gpu


def _weights(seed):
    g = torch.Generator().manual_seed(seed)
    w1 = torch.randn(64, 64, 3, 3, generator=g) / 24
    b1 = torch.randn(64, generator=g) * 0.1
    w2 = torch.randn(3, 64, 3, 3, generator=g) / 24
    b2 = torch.randn(3, generator=g)
    p1, pb1 = packing.pack_conv_c64(w1, b1, 1)
    return (p1.cuda(), pb1.cuda(), packing.pack_conv_c64_thin(w2).cuda(), b2.float().cuda(),
            packing.pack_dec2_scatter(w2).cuda())


def _two_kernel(x, p1, pb1, p2, b2):
    dec = ops.conv_c64(x, p1, pb1, 1, relu=True)
    return ops.conv_c64_thin(dec, p2, b2, 3, relu=False)


@pytest.mark.parametrize("B,H,W", [(1, 13, 45), (3, 13, 45), (1, 5, 20), (3, 24, 96), (1, 41, 70), (2, 720, 1280)])
def test_decoder_fused_matches_two_kernels(B, H, W):
    p1, pb1, p2, b2, wz = _weights(B * 1000 + H)
    x = torch.randn(B, H, W, 64, generator=torch.Generator().manual_seed(H * W)).to(torch.bfloat16).cuda()
    with torch.no_grad():
        ref = _two_kernel(x, p1, pb1, p2, b2)
        got = ops.decoder_fused(x, p1, pb1, wz, b2)
    torch.cuda.synchronize()
    assert got.shape == ref.shape == (B, 3, H, W)
    assert torch.isfinite(got).all()
    rng = (ref.max() - ref.min()).item()
    err = (got - ref).abs().max().item()
    assert err <= 1e-5 * rng, (err, rng)


def test_decoder_fused_batch_equals_single():
    p1, pb1, _, b2, wz = _weights(7)
    x = torch.randn(3, 37, 70, 64, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).cuda()
    with torch.no_grad():
        yb = ops.decoder_fused(x, p1, pb1, wz, b2)
        ys = torch.cat([ops.decoder_fused(x[i:i + 1].contiguous(), p1, pb1, wz, b2) for i in range(3)])
    assert torch.equal(yb, ys)


def test_engine_routes_decoder(det_sd):
    """engine.fuse_decoder on / off over the whole forward: same output to the fused decoder's rounding."""
    import importlib
    from transformerupscaler_amd import engine
    model = importlib.import_module("models.FastTransformer.model").TransformerModel()
    model.load_state_dict(det_sd, strict=False)
    model = model.cuda().eval()
    x = torch.rand((2, 3, 40, 72), generator=torch.Generator().manual_seed(2)).cuda()
    with torch.no_grad():
        y_f = model(x, upscale_factor=2)
        engine.fuse_decoder = False
        try:
            y_u = model(x, upscale_factor=2)
        finally:
            engine.fuse_decoder = True
    assert (y_f - y_u).abs().max().item() <= 1e-4
