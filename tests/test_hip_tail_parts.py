"""The decoder's finishing pass folded into the streaming output tail (csrc/tail_stream.hip PARTS, csrc/decoder_fused.hip
tup_decoder_fused_parts_fwd; engine.fuse_decoder_finish): the tail forms every LR value from the unfinished pieces in
decoder_finish_kernel's order of fp32 additions, so nothing may differ from the finished path -- the reference everywhere is
ops.decoder_fused(finish=True) followed by ops.tail_stream_r2(x=residual), the comparison torch.equal.

Shapes (B, H, W); the launcher and ops._tail_stream_plan give bands of 12 LR rows at these sizes (TS_BAND_MIN; the band height only
grows once B * strips * bands exceeds the 3072 resident waves), so H = 13 .. 41 is two to four bands:
  (1, 5, 20)    one decoder tile, no column seam, rows without a seam partner at both ends
  (1, 13, 45)   two tile columns, odd H (the last row has no partner), W no multiple of 4 or 32
  (3, 24, 96)   exact tile multiples, two bands, a batch
  (2, 41, 70)   two 60-column strips: the halo lanes form their values across a strip boundary
  (1, 27, 150)  three strips; with Resize the strip stride is below 60, so the tile-edge lanes differ from strip to strip
"""
import functools
import importlib

import pytest
import torch

from transformerupscaler_amd import ops, packing

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 20), (1, 13, 45), (3, 24, 96), (2, 41, 70), (1, 27, 150)]


def _resized(H, W):
    return (H * 3 // 2, W * 3 // 2)          # 1.5 x the LR size = 3/4 of the HR map: at most 4 taps per output


def _weights(seed):
    g = torch.Generator().manual_seed(seed)
    w1 = torch.randn(64, 64, 3, 3, generator=g) / 24
    b1 = torch.randn(64, generator=g) * 0.1
    w2 = torch.randn(3, 64, 3, 3, generator=g) / 24
    b2 = torch.randn(3, generator=g)
    p1, pb1 = packing.pack_conv_c64(w1, b1, 1)
    w_fu, b_fu = torch.randn(12, 3, 3, 3, generator=g) * 0.05, torch.randn(12, generator=g) * 0.1
    w_fc, b_fc = torch.randn(3, 3, 3, 3, generator=g) * 0.2, torch.randn(3, generator=g) * 0.1
    dec = (p1.cuda(), pb1.cuda(), packing.pack_dec2_scatter(w2).cuda(), b2.float().cuda())
    tail = (packing.pack_planar_t(w_fu).cuda(), b_fu.cuda(), packing.pack_planar_t(w_fc).cuda(), b_fc.cuda())
    return dec, tail


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    """Inputs, the finished plane and the unfinished pieces of one shape: computed once, shared by the tests, never written to."""
    dec, tail = _weights(B * 1000 + H)
    g = torch.Generator().manual_seed(H * W)
    x = torch.randn(B, H, W, 64, generator=g).to(torch.bfloat16).cuda()
    ui = (torch.rand(B, 3, 2 * H, 2 * W, generator=g) * 0.6 + 0.2).cuda()
    with torch.no_grad():
        residual = ops.decoder_fused(x, *dec)
        parts = ops.decoder_fused(x, *dec, finish=False)
    torch.cuda.synchronize()
    return x, ui, dec, tail, residual, parts


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("resize", [False, True])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_tail_on_unfinished_pieces_equals_finished_path(B, H, W, resize, clamp):
    x, ui, dec, tail, residual, parts = _case(B, H, W)
    part, seamv, cseam, b2 = parts
    assert part.shape == residual.shape and b2 is dec[3]
    assert not torch.equal(part, residual)                  # the pieces really are unfinished
    out_hw = _resized(H, W) if resize else None
    with torch.no_grad():
        ref = ops.tail_stream_r2(residual, *tail, ui, clamp=clamp, out_hw=out_hw)
        got = ops.tail_stream_r2(None, *tail, ui, clamp=clamp, out_hw=out_hw, parts=parts)
    assert ref is not None and got is not None              # the 1.5 x Resize is one the fused kernel takes
    assert tuple(got.shape) == (B, 3) + (out_hw if resize else (2 * H, 2 * W))
    assert torch.isfinite(ref).all()
    assert torch.equal(got, ref)
    if clamp and H * W > 100:
        assert 0.02 < ref.mean().item() < 0.98              # not clamped away


def test_tail_on_unfinished_pieces_batch_equals_single():
    B, H, W = 3, 24, 96
    x, ui, dec, tail, _, parts = _case(B, H, W)
    out_hw = _resized(H, W)
    with torch.no_grad():
        yb = ops.tail_stream_r2(None, *tail, ui, clamp=True, out_hw=out_hw, parts=parts)
        ys = []
        for i in range(B):
            pi = ops.decoder_fused(x[i:i + 1].contiguous(), *dec, finish=False)
            ys.append(ops.tail_stream_r2(None, *tail, ui[i:i + 1].contiguous(), clamp=True, out_hw=out_hw, parts=pi))
    assert torch.equal(yb, torch.cat(ys))


@pytest.fixture(scope="module")
def model(det_sd):
    m = importlib.import_module("models.FastTransformer.model").TransformerModel()
    m.load_state_dict(det_sd, strict=False)
    return m.cuda().eval()


# scale 2 with and without the fused Resize, and a Resize of more than 4 taps (144 -> 50 columns), which the fused kernel declines:
# the tail then runs unclamped on the pieces and resize_aa follows.  Scale 4 and the 3 x output keep the finishing kernel
# (conv_planar / tail_fused read `residual`), so the toggle changes nothing there.
@pytest.mark.parametrize("kw", [dict(upscale_factor=2), dict(res_out=(60, 108)), dict(res_out=(44, 50)),
                                dict(upscale_factor=4), dict(res_out=(120, 216))], ids=str)
def test_engine_toggle_is_bit_identical(model, kw, monkeypatch):
    from transformerupscaler_amd import engine
    x = torch.rand((2, 3, 40, 72), generator=torch.Generator().manual_seed(2)).cuda()
    if kw.get("res_out") == (44, 50):
        assert ops._tail_stream_plan(x.device, 2, 40, 72, 44, 50) is None
    seen = []
    real = ops.decoder_fused
    monkeypatch.setattr(ops, "decoder_fused", lambda *a, finish=True: seen.append(finish) or real(*a, finish=finish))
    assert engine.fuse_decoder_finish in (True, False)
    with torch.no_grad():
        monkeypatch.setattr(engine, "fuse_decoder_finish", True)
        y_on = model(x, **kw)
        monkeypatch.setattr(engine, "fuse_decoder_finish", False)
        y_off = model(x, **kw)
    scale2 = kw.get("upscale_factor") == 2 or kw.get("res_out") in ((60, 108), (44, 50))
    assert seen == [not scale2, True]                        # only the scale-2 route skips the finishing launch
    assert torch.equal(y_on, y_off)
