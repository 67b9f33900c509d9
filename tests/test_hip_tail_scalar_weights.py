"""The streaming output tail (csrc/tail_stream.hip): its 420 wave-uniform weights are scalar operands fetched through an asm-managed
ring of scalar registers.  A mis-indexed weight or a changed order of additions must show, so the bits are pinned by two references,
neither of them the kernel:
  x2 instances       integer operands: every partial sum is an integer below 2**24, hence exact in fp32 in ANY order, and the
                     output must be bit-equal to the float64 torch restatement (the style of tests/_exact_ref.py)
  Resize instances   no Resize the planner accepts with more than two taps has dyadic tap weights, so the bits are a recorded result:
                     tests/golden/tail_stream_resize_digests.json, SHA-256 of the output bytes (how it was made: see the file)
Plane input only: tests/test_hip_tail_parts.py pins the PARTS instances to the plane ones bit for bit.

Shapes (B, H, W); bands are 12 LR rows at these sizes (TS_BAND_MIN), strips 60 LR columns (fewer with Resize):
  (1, 12, 60)   one band, one strip, exactly full
  (2, 25, 61)   bands of 12 + 12 + 1 (a remainder that is no multiple of 3), a second strip of one column, a batch
  (1, 40, 130)  three strips, four bands
The first two rows of every band run stage B only (the first group of the 3 -> 3 conv is requested and drained unused), every later
row hands the ring from stage B to stage C; the band and strip seams read values formed by the neighbouring wave's first / last rows
and halo lanes.
"""
import functools
import hashlib
import json
import os

import pytest
import torch
import torch.nn.functional as F

import _exact_ref as R          # tests/ is on sys.path (rootdir-less test modules)
from transformerupscaler_amd import ops, packing

pytestmark = pytest.mark.gpu

SHAPES = [(1, 12, 60), (2, 25, 61), (1, 40, 130)]
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tail_stream_resize_digests.json")


def _resized(H, W):
    return (H * 3 // 2, W * 3 // 2)          # 0.75 x the HR map: at most 4 taps per output


def _packed(w_fu, b_fu, w_fc, b_fc):
    return packing.pack_planar_t(w_fu).cuda(), b_fu.cuda(), packing.pack_planar_t(w_fc).cuda(), b_fc.cuda()


def _tail64(x, w_fu, b_fu, w_fc, b_fc, ui):
    """final_upscale + final_upscale_conv + "+ upscaled_input" restated in float64 (models/FastTransformer: utils.py:62-63,74-75,
    model.py:316-320), unclamped."""
    w_fu, b_fu, w_fc, b_fc = (t.double() for t in (w_fu, b_fu, w_fc, b_fc))
    t1 = F.pixel_shuffle(F.conv2d(x.cpu().double(), w_fu, b_fu, padding=1), 2)
    return F.conv2d(t1, w_fc, b_fc, padding=1) + ui.cpu().double()


@functools.lru_cache(maxsize=None)
def _weights():
    g = torch.Generator().manual_seed(420)
    w_fu, b_fu = torch.randn(12, 3, 3, 3, generator=g) * 0.05, torch.randn(12, generator=g) * 0.1
    w_fc, b_fc = torch.randn(3, 3, 3, 3, generator=g) * 0.2, torch.randn(3, generator=g) * 0.1
    assert torch.cat([t.flatten() for t in (w_fu, b_fu, w_fc, b_fc)]).unique().numel() == 420
    return w_fu, b_fu, w_fc, b_fc


# ------------------------------------------------------------------------------------------------
# x2: exact integer operands
# ------------------------------------------------------------------------------------------------
X_AMP, UI_AMP = 3, 3


@functools.lru_cache(maxsize=None)
def _int_weights():
    """420 distinct integers: the 84 values of the 3 -> 3 conv a permutation of +-1 .. +-42, the 336 of the 3 -> 12 conv of +-43 ..
    +-210.  The bound of every partial sum, in any order, from sum |w| max |x| per output channel: asserted here, on the CPU."""
    g = torch.Generator().manual_seed(421)

    def perm(lo, hi):
        mag = torch.arange(lo, hi + 1)
        v = torch.cat([mag, -mag])
        return v[torch.randperm(v.numel(), generator=g)].float()

    fu, fc = perm(43, 210), perm(1, 42)
    w_fu, b_fu, w_fc, b_fc = fu[:324].view(12, 3, 3, 3), fu[324:], fc[:81].view(3, 3, 3, 3), fc[81:]
    assert torch.cat([fu, fc]).unique().numel() == 420
    t1_top = (w_fu.abs().sum(dim=(1, 2, 3)) * X_AMP + b_fu.abs()).max().item()
    out_top = (w_fc.abs().sum(dim=(1, 2, 3)) * t1_top + b_fc.abs()).max().item() + UI_AMP
    assert out_top < 2 ** 24, (t1_top, out_top)
    return w_fu, b_fu, w_fc, b_fc


@functools.lru_cache(maxsize=None)
def _int_case(B, H, W):
    """Integer plane and upscaled_input with the float64 reference: computed once, shared, never written to."""
    x = R.ints((B, 3, H, W), 4200 + H, X_AMP)
    ui = R.ints((B, 3, 2 * H, 2 * W), 4300 + H, UI_AMP)
    ref = _tail64(x, *_int_weights(), ui)
    R.assert_exact_preconditions(ref)
    assert 0.2 < (ref < 0).double().mean().item() < 0.8 and 0.2 < (ref > 1).double().mean().item() < 0.8      # the clamp has work on both sides
    return x.cuda(), ui.cuda(), ref


@pytest.mark.parametrize("clamp", [True, False], ids=["clamp", "noclamp"])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_x2_exact_integer_operands(B, H, W, clamp):
    x, ui, ref = _int_case(B, H, W)
    with torch.no_grad():
        got = ops.tail_stream_r2(x, *_packed(*_int_weights()), ui, clamp=clamp)
    want = ref.clamp(0, 1) if clamp else ref
    R.assert_bit_equal(got, want.float(), tile=(12, 60), r=2, what=f"tail_stream_r2 x2 {(B, H, W)} clamp={clamp}", layout="nchw")


# ------------------------------------------------------------------------------------------------
# Resize: recorded digests
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _float_case(B, H, W):
    """Plane and upscaled_input from the CPU generator (not from the decoder: the recorded digests depend on the tail alone)."""
    g = torch.Generator().manual_seed(B * 1000 + H * W)
    x = torch.randn(B, 3, H, W, generator=g)
    ui = torch.rand(B, 3, 2 * H, 2 * W, generator=g) * 0.6 + 0.2
    return x.cuda(), ui.cuda()


def _resize_digest(B, H, W, clamp):
    x, ui = _float_case(B, H, W)
    with torch.no_grad():
        out = ops.tail_stream_r2(x, *_packed(*_weights()), ui, clamp=clamp, out_hw=_resized(H, W))
    assert out is not None and tuple(out.shape) == (B, 3) + _resized(H, W)          # the 0.75 x Resize is one the fused kernel takes
    return hashlib.sha256(out.cpu().contiguous().numpy().tobytes()).hexdigest()


def _digest_key(B, H, W, clamp):
    return f"{B}x{H}x{W}-{'clamp' if clamp else 'noclamp'}"


@pytest.mark.parametrize("clamp", [True, False], ids=["clamp", "noclamp"])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_resize_recorded_digests(B, H, W, clamp):
    with open(DIGESTS) as f:
        recorded = json.load(f)["sha256"]
    assert _resize_digest(B, H, W, clamp) == recorded[_digest_key(B, H, W, clamp)]


# ------------------------------------------------------------------------------------------------
# float operands against float64; the entry's refusals
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    """Inputs and the decoder's finished LR plane of one shape: computed once, shared, never written to."""
    g = torch.Generator().manual_seed(B * 1000 + H * W)
    w1 = torch.randn(64, 64, 3, 3, generator=g) / 24
    b1 = torch.randn(64, generator=g) * 0.1
    w2 = torch.randn(3, 64, 3, 3, generator=g) / 24
    b2 = torch.randn(3, generator=g)
    p1, pb1 = packing.pack_conv_c64(w1, b1, 1)
    dec = (p1.cuda(), pb1.cuda(), packing.pack_dec2_scatter(w2).cuda(), b2.float().cuda())
    x = torch.randn(B, H, W, 64, generator=g).to(torch.bfloat16).cuda()
    ui = (torch.rand(B, 3, 2 * H, 2 * W, generator=g) * 0.6 + 0.2).cuda()
    with torch.no_grad():
        residual = ops.decoder_fused(x, *dec)
    torch.cuda.synchronize()
    return ui, _packed(*_weights()), residual


def test_scalar_weight_arm_vs_float64_torch():
    """The kernel against the float64 restatement, unclamped, at (2, 25, 61).  Tolerance: the 2e-5 of
    tests/test_hip_kernels.py::test_tail_stream_r2_vs_torch_and_unfused."""
    B, H, W = 2, 25, 61
    ui, tail, residual = _case(B, H, W)
    with torch.no_grad():
        got = ops.tail_stream_r2(residual, *tail, ui, clamp=False)
    ref = _tail64(residual, *_weights(), ui)
    assert got.shape == ref.shape
    err = (got.cpu().double() - ref).abs().max().item()
    assert err <= 2e-5, err


def test_scalar_weight_arm_refuses_misaligned_weight_pointers():
    """The scalar loads are 16-byte reads: a weight tensor that does not start on a 16-byte boundary is an error, not a slow path."""
    ui, tail, residual = _case(1, 12, 60)
    wfu_t, bfu, wfc_t, bfc = tail
    shifted = torch.zeros(16, device=bfu.device)[1:13].copy_(bfu)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    with pytest.raises(RuntimeError):
        ops.tail_stream_r2(residual, wfu_t, shifted, wfc_t, bfc, ui)


if __name__ == "__main__":          # regenerates the golden file from the kernel as it is: PYTHONPATH=. python3 tests/test_hip_tail_scalar_weights.py
    with open(DIGESTS) as f:
        doc = json.load(f)
    doc["sha256"] = {_digest_key(*s, c): _resize_digest(*s, c) for s in SHAPES for c in (True, False)}
    with open(DIGESTS, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
