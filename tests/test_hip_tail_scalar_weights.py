"""The streaming output tail with its 420 wave-uniform weights as scalar operands (csrc/tail_stream.hip, SW = true: the default arm)
against the LDS-ring arm it replaces (ops.tail_stream_weight_source("lds")).  The FMA operands and their order are the same in both
arms, so every output must be bit-identical: torch.equal, with weights whose 420 values are all distinct so that a mis-indexed
weight shows.

Shapes (B, H, W); bands are 12 LR rows at these sizes (TS_BAND_MIN), strips 60 LR columns (fewer with Resize):
  (1, 12, 60)   one band, one strip, exactly full
  (2, 25, 61)   bands of 12 + 12 + 1 (a remainder that is no multiple of 3), a second strip of one column, a batch
  (1, 40, 130)  three strips, four bands
The first two rows of every band run stage B only (no weights of the 3 -> 3 conv are requested), every later row hands the ring from
stage B to stage C; the band and strip seams read values formed by the neighbouring wave's first / last rows and halo lanes.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from transformerupscaler_amd import ops, packing

pytestmark = pytest.mark.gpu

SHAPES = [(1, 12, 60), (2, 25, 61), (1, 40, 130)]


def _resized(H, W):
    return (H * 3 // 2, W * 3 // 2)          # 0.75 x the HR map: at most 4 taps per output


@pytest.fixture
def arms():
    """Runs fn under both arms; the default arm is in force again afterwards, whatever happens."""
    def both(fn):
        try:
            ops.tail_stream_weight_source("lds")
            lds = fn()
            ops.tail_stream_weight_source("scalar")
            scalar = fn()
        finally:
            ops.tail_stream_weight_source("scalar")
        return scalar, lds
    return both


@functools.lru_cache(maxsize=None)
def _weights():
    g = torch.Generator().manual_seed(420)
    w_fu, b_fu = torch.randn(12, 3, 3, 3, generator=g) * 0.05, torch.randn(12, generator=g) * 0.1
    w_fc, b_fc = torch.randn(3, 3, 3, 3, generator=g) * 0.2, torch.randn(3, generator=g) * 0.1
    assert torch.cat([t.flatten() for t in (w_fu, b_fu, w_fc, b_fc)]).unique().numel() == 420
    return w_fu, b_fu, w_fc, b_fc


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    """Inputs, the finished LR plane and the decoder's unfinished pieces of one shape: computed once, shared, never written to."""
    g = torch.Generator().manual_seed(B * 1000 + H * W)
    w1 = torch.randn(64, 64, 3, 3, generator=g) / 24
    b1 = torch.randn(64, generator=g) * 0.1
    w2 = torch.randn(3, 64, 3, 3, generator=g) / 24
    b2 = torch.randn(3, generator=g)
    p1, pb1 = packing.pack_conv_c64(w1, b1, 1)
    dec = (p1.cuda(), pb1.cuda(), packing.pack_dec2_scatter(w2).cuda(), b2.float().cuda())
    w_fu, b_fu, w_fc, b_fc = _weights()
    tail = (packing.pack_planar_t(w_fu).cuda(), b_fu.cuda(), packing.pack_planar_t(w_fc).cuda(), b_fc.cuda())
    x = torch.randn(B, H, W, 64, generator=g).to(torch.bfloat16).cuda()
    ui = (torch.rand(B, 3, 2 * H, 2 * W, generator=g) * 0.6 + 0.2).cuda()
    with torch.no_grad():
        residual = ops.decoder_fused(x, *dec)
        parts = ops.decoder_fused(x, *dec, finish=False)
    torch.cuda.synchronize()
    return ui, tail, residual, parts


@pytest.mark.parametrize("from_parts", [False, True], ids=["plane", "parts"])
@pytest.mark.parametrize("clamp", [True, False], ids=["clamp", "noclamp"])
@pytest.mark.parametrize("resize", [False, True], ids=["x2", "resize"])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_scalar_weight_arm_equals_lds_arm(arms, B, H, W, resize, clamp, from_parts):
    ui, tail, residual, parts = _case(B, H, W)
    out_hw = _resized(H, W) if resize else None

    def run():
        with torch.no_grad():
            if from_parts:
                return ops.tail_stream_r2(None, *tail, ui, clamp=clamp, out_hw=out_hw, parts=parts)
            return ops.tail_stream_r2(residual, *tail, ui, clamp=clamp, out_hw=out_hw)

    scalar, lds = arms(run)
    assert scalar is not None and lds is not None           # the 0.75 x Resize is one the fused kernel takes
    assert tuple(scalar.shape) == (B, 3) + (out_hw if resize else (2 * H, 2 * W))
    assert torch.isfinite(lds).all()
    assert torch.equal(scalar, lds)
    if clamp:
        assert 0.02 < lds.mean().item() < 0.98              # not clamped away


def test_scalar_weight_arm_vs_float64_torch():
    """The default arm against final_upscale + final_upscale_conv + "+ upscaled_input" restated in float64 (models/FastTransformer:
    utils.py:62-63,74-75, model.py:316-320), unclamped, at (2, 25, 61).  Tolerance: the 2e-5 of
    tests/test_hip_kernels.py::test_tail_stream_r2_vs_torch_and_unfused."""
    B, H, W = 2, 25, 61
    ui, tail, residual, _ = _case(B, H, W)
    w_fu, b_fu, w_fc, b_fc = (t.double() for t in _weights())
    ops.tail_stream_weight_source("scalar")
    with torch.no_grad():
        got = ops.tail_stream_r2(residual, *tail, ui, clamp=False)
        t1 = F.pixel_shuffle(F.conv2d(residual.cpu().double(), w_fu, b_fu, padding=1), 2)
        ref = F.conv2d(t1, w_fc, b_fc, padding=1) + ui.cpu().double()
    assert got.shape == ref.shape
    err = (got.cpu().double() - ref).abs().max().item()
    assert err <= 2e-5, err


def test_weight_source_switch_refuses_unknown_values():
    from transformerupscaler_amd import _lib
    with pytest.raises(ValueError):
        ops.tail_stream_weight_source("registers")
    with pytest.raises(RuntimeError):
        _lib.call("tup_tail_stream_weight_source", 2)
    ops.tail_stream_weight_source("scalar")


def test_scalar_weight_arm_refuses_misaligned_weight_pointers():
    """The scalar loads are 16-byte reads: a weight tensor that does not start on a 16-byte boundary is an error, not a slow path."""
    ui, tail, residual, _ = _case(1, 12, 60)
    wfu_t, bfu, wfc_t, bfc = tail
    shifted = torch.zeros(16, device=bfu.device)[1:13].copy_(bfu)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    ops.tail_stream_weight_source("scalar")
    with pytest.raises(RuntimeError):
        ops.tail_stream_r2(residual, wfu_t, shifted, wfc_t, bfc, ui)
    try:
        ops.tail_stream_weight_source("lds")
        lds = ops.tail_stream_r2(residual, wfu_t, shifted, wfc_t, bfc, ui)
    finally:
        ops.tail_stream_weight_source("scalar")
    assert torch.equal(lds, ops.tail_stream_r2(residual, wfu_t, bfu, wfc_t, bfc, ui))
