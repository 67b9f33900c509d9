"""Exact-operand references for the conv kernels (tests/test_conv_exact_cpu.py, tests/test_hip_conv_exact.py).  No tests here.

Every kernel of the conv family is a linear map plus ReLU, masks and clamps; its operands are bf16 (or fp32 planes it rounds to
bf16) and it accumulates in fp32.  With small INTEGER operands every product and every partial sum is an integer whose magnitude
is at most sum |x| |w| < 2**24, so the fp32 result is exact in any summation order (MFMA or VALU, atomics or slabs, any split of
K) and a kernel must equal the torch reference bit for bit; an indexing error changes some output by at least 1.  A bf16 output
is the exact integer passed through .to(torch.bfloat16): for |value| <= 256 that is the integer itself (bf16 holds 8 significant
bits), whatever the rounding mode; above 256 it is torch's round-to-nearest-even, which csrc/common.h's f32_to_bf16 promises too.

The references are torch on the CPU (F.conv2d, F.pixel_shuffle, F.relu, autograd) in a dtype the caller chooses: fp64 is the
reference proper, fp32 is shown equal to it on the CPU (test_conv_exact_cpu.py) and used where fp64 would be slow."""
import torch
import torch.nn.functional as F

TILE = (8, 32)                       # TH x TW of csrc/conv3x3_c64.hip and its relatives
TILE_ROWS = (8, 28)                  # the row-GEMM kernels (thin cout <= 4, branch A r = 2): 28 output columns per tile

# (B, H, W) of the LR map.  Tile counts below are for 8 x 32 tiles; the row-GEMM kernels count 8 x 28 ones.
SHAPES = [
    (1, 1, 1),          # everything is border
    (1, 3, 7),          # one partial tile
    (1, 8, 32),         # exactly one tile
    (2, 9, 33),         # a one-pixel second tile in both directions, and the batch stride
    (2, 19, 70),        # 3 x 3 tiles per image, partial last ones: interior seams on all four sides
]
# the persistent kernels' schedules: grid = min(tiles, 256) workgroups of two groups; (gridDim & 7) == 0 takes XCD bands, else round robin
SCHED_LARGE = [
    (3, 60, 345),       # 8 x 11 x 3 = 264 tiles (8x28: 8 x 13 x 3 = 312): grid 256, bands of 33, ragged last band, second tiles
    (3, 117, 440),      # 15 x 14 x 3 = 630 tiles (8x28: 15 x 16 x 3 = 720): several tiles per group, carries across row and image
]
SCHED_SMALL = [
    (1, 19, 45),        # 3 x 2 = 6 tiles (8x28: 6): grid 6, 6 & 7 != 0 -> round robin
    (3, 19, 45),        # 18 tiles (8x28: 18): grid 18, 18 & 7 != 0 -> round robin, batch carry
    (1, 13, 45),        # 2 x 2 = 4 tiles (8x28: 4): grid 4 -> round robin
    (1, 16, 128),       # 2 x 4 = 8 tiles (8x28: 2 x 5 = 10): grid 8, 8 & 7 == 0 -> bands of one tile each (round robin for 8x28)
]
SCHEDULES = SCHED_LARGE + SCHED_SMALL
BRA_EXTRA = [(1, 1, 5), (1, 2, 2), (1, 6, 6)]          # branch A: the ring is most or all of the image
DECODER_SHAPES = SHAPES + [(3, 117, 440)]              # seamv / cseam are per 32-column tile: many tiles, several per group
BRA_BWD_MIN = 6                                        # tup_bra_backward refuses H < 6 or W < 6
# feat_grad_combine folds the gradient of a reflect padding to the next multiple of 8 back onto the map.  Reflect padding is defined
# (in torch and in the reference model) only where the padding is smaller than the side, which (1, 1, 1) and (1, 3, 7) are not:
# the shapes below are the default ones where the operation exists, plus a small one with padding on both sides.
FGC_SHAPES = [(1, 8, 32), (2, 9, 33), (2, 19, 70), (1, 5, 12)]


def ref_dtype(shape):
    """fp64 is the reference; the large maps take fp32, which test_conv_exact_cpu.py shows equal to it case by case."""
    B, H, W = shape
    return torch.float32 if B * H * W > 20000 else torch.float64


def ints(shape, seed, amp=1, density=1.0):
    """fp32 tensor of integers in [-amp, amp]; a (1 - density) share are zeros, the rest uniform over the non-zero values."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.randint(1, amp + 1, tuple(shape), generator=g)
    sign = torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1
    keep = torch.rand(tuple(shape), generator=g) < density
    return (mag * sign * keep).float()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nhwc_bf16(t):
    return nhwc(t).to(torch.bfloat16)


def bf16_round(t):
    """What a kernel's bf16 store makes of t (round-to-nearest-even), back in t's dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def _c(t, dtype):
    return None if t is None else t.to(dtype)


# ------------------------------------------------------------------------------------------------
# forward references (NCHW in, the kernel's output layout out)
# ------------------------------------------------------------------------------------------------
def conv_c64_ref(x, w, b, r, relu=False, add=None, mask=None, dtype=torch.float64):
    """tup_conv3x3_c64_fwd out_mode 0: (PixelShuffle_r(conv(x) + b) [relu] + add) * (mask > 0), NHWC [B][Hr][Wr][64]."""
    y = F.pixel_shuffle(F.conv2d(x.to(dtype), w.to(dtype), _c(b, dtype), padding=1), r)
    if relu:
        y = F.relu(y)
    if add is not None:
        y = y + add.to(dtype)
    if mask is not None:
        y = y * (mask > 0)
    return nhwc(y)


def conv_thin_ref(x, w, b, relu=False, dtype=torch.float64):
    """tup_conv3x3_c64_fwd out_mode 1: conv 64 -> cout (+ b) [relu], planar."""
    y = F.conv2d(x.to(dtype), w.to(dtype), _c(b, dtype), padding=1)
    return F.relu(y) if relu else y


def conv1_ref(x, w, b, relu=True, in_mask=None, out_mask=None, dtype=torch.float64):
    """tup_conv3x3_c3_fwd: conv(x * (in_mask > 0)) + b [relu], * (out_mask > 0); NHWC [B][H][W][64]."""
    x = x.to(dtype)
    if in_mask is not None:
        x = x * (in_mask > 0)
    y = F.conv2d(x, w.to(dtype), _c(b, dtype), padding=1)
    if relu:
        y = F.relu(y)
    if out_mask is not None:
        y = y * (out_mask > 0)
    return nhwc(y)


def conv12_ref(x, w1, b1, w2, b2, dtype=torch.float64):
    """conv1_compact -> conv12_fused: relu(conv2(bf16(relu(conv1(x))))); returns (NHWC result, conv1's map before its rounding)."""
    mid = F.relu(F.conv2d(x.to(dtype), w1.to(dtype), b1.to(dtype), padding=1))
    y = F.relu(F.conv2d(bf16_round(mid), w2.to(dtype), b2.to(dtype), padding=1))
    return nhwc(y), mid


def decoder_ref(x, w1, b1, w2, b2, dtype=torch.float64):
    """decoder_fused: conv -> relu -> bf16 -> conv + bias, planar fp32; returns (result, the 64-channel map before its rounding)."""
    mid = F.relu(F.conv2d(x.to(dtype), w1.to(dtype), b1.to(dtype), padding=1))
    return F.conv2d(bf16_round(mid), w2.to(dtype), b2.to(dtype), padding=1), mid


def branch_a_ref(feat, wu, bu, w3, r, relu=True, dtype=torch.float64):
    """The explicit chain the composed 5x5 conv stands for: conv 64 -> 64rr (+ bias) -> PixelShuffle(r) -> conv 64 -> 3 (no bias)
    [-> relu]; planar [B][3][Hr][Wr].  Nothing is rounded in between: the composed kernel never forms the middle map."""
    y = F.conv2d(F.pixel_shuffle(F.conv2d(feat.to(dtype), wu.to(dtype), bu.to(dtype), padding=1), r), w3.to(dtype), None, padding=1)
    return F.relu(y) if relu else y


def branch_a_weights(r, seed, amp_u=1, density_u=0.25):
    """(wu, bu, w3) whose composition is exact in bf16 BY CONSTRUCTION: w3 has exactly 4 non-zero +-1 input channels per (output,
    tap), wu is integer with |wu| <= amp_u, and a composed weight is a sum over at most 9 HR taps of sum_ch w3[c, ch, tap] wu[ch..]:
    |Wc| <= 9 * 4 * amp_u = 36 amp_u <= 256 for amp_u <= 7, an integer that bf16 holds exactly (so do |bias| <= 36 amp_b in fp32)."""
    wu = ints((64 * r * r, 64, 3, 3), seed, amp_u, density_u)
    bu = ints((64 * r * r,), seed + 1, 2, 1.0)
    g = torch.Generator().manual_seed(seed + 2)
    w3 = torch.zeros(3, 9, 64)
    for c in range(3):
        for tap in range(9):
            ch = torch.randperm(64, generator=g)[:4]
            w3[c, tap, ch] = (torch.randint(0, 2, (4,), generator=g) * 2 - 1).float()
    return wu, bu, w3.permute(0, 2, 1).reshape(3, 64, 3, 3).contiguous()


def ring_mask(Hs, Ws, width=1):
    m = torch.ones(Hs, Ws, dtype=torch.bool)
    if Hs > 2 * width and Ws > 2 * width:
        m[width:-width, width:-width] = False
    return m


# ------------------------------------------------------------------------------------------------
# backward references (autograd)
# ------------------------------------------------------------------------------------------------
def _leaf(t, dtype):
    """A fresh autograd leaf (a copy: .to() of a tensor that already has the dtype would hand back the operand itself)."""
    return t.detach().to(dtype).clone().requires_grad_(True)


def conv_grads(x, w, b, gy, r=1, stride=1, dtype=torch.float64):
    """(dx, dw, db) of PixelShuffle_r(conv2d(x, w, b, stride, padding=1)) for the output gradient gy (all NCHW)."""
    x, w = _leaf(x, dtype), _leaf(w, dtype)
    b = None if b is None else _leaf(b, dtype)
    y = F.conv2d(x, w, b, stride=stride, padding=1)
    if r > 1:
        y = F.pixel_shuffle(y, r)
    y.backward(gy.to(dtype))
    return x.grad, w.grad, (None if b is None else b.grad)


def feat_grad_combine_ref(a, b, gpe, feat, dtype=torch.float64):
    """tup_feat_grad_combine: (a [+ b] + fold of the reflect padding's gradient gpe) * (feat > 0); NHWC."""
    H, W = feat.shape[2:]
    hp, wp = gpe.shape[2:]
    f = _leaf(feat, dtype)
    fp = F.pad(f, (0, wp - W, 0, hp - H), mode="reflect") if (hp > H or wp > W) else f * 1
    fp.backward(gpe.to(dtype))
    s = a.to(dtype) + f.grad
    if b is not None:
        s = s + b.to(dtype)
    return nhwc(s * (feat > 0))


def branch_a_grads(feat, wu, bu, w3, g, dtype=torch.float64):
    """Backward of relu(branch_a) at r = 2 for the gradient g w.r.t. its output: (ui, dfeat, dwu, dbu, dw3), gated by ui > 0."""
    feat, wu, bu, w3 = (_leaf(t, dtype) for t in (feat, wu, bu, w3))
    ui = F.relu(F.conv2d(F.pixel_shuffle(F.conv2d(feat, wu, bu, padding=1), 2), w3, None, padding=1))
    ui.backward(g.to(dtype))
    return ui.detach(), feat.grad, wu.grad, bu.grad, w3.grad


# ------------------------------------------------------------------------------------------------
# the checks
# ------------------------------------------------------------------------------------------------
def assert_exact_preconditions(ref64, bf16_out=False, default_case=True):
    """The reference is integer-valued and below 2**24 (exact in fp32 in any summation order); a bf16 output of a default case also
    stays within 256, where bf16 holds every integer and the comparison does not depend on the rounding mode."""
    ref64 = ref64.double()
    assert bool(torch.isfinite(ref64).all())
    assert torch.equal(ref64, ref64.round()), "the reference is not integer-valued"
    top = ref64.abs().max().item() if ref64.numel() else 0.0
    assert top < 2 ** 24, top
    if bf16_out and default_case:
        assert top <= 256, f"bf16 output reaches {top}: the default cases stay within 256"


def share_above_256(ref64):
    return (ref64.abs() > 256).double().mean().item()


def _describe(bad, tile, r, layout):
    idx = bad.nonzero()
    n = idx.shape[0]
    if bad.dim() != 4 or layout is None:
        return f"{n} of {bad.numel()} differ; first at {[tuple(i.tolist()) for i in idx[:6]]}"
    if layout == "nchw":
        idx = idx[:, [0, 2, 3, 1]]
        Hs, Ws = bad.shape[2], bad.shape[3]
    else:
        Hs, Ws = bad.shape[1], bad.shape[2]
    th, tw = tile
    y, x = idx[:, 1], idx[:, 2]
    ly, lx = y // r, x // r
    border = (y == 0) | (y == Hs - 1) | (x == 0) | (x == Ws - 1)
    iy, ix = ly % th, lx % tw
    seam = (iy == 0) | (iy == th - 1) | (ix == 0) | (ix == tw - 1)
    where = []
    for k in range(min(n, 6)):
        b, yy, xx, c = idx[k].tolist()
        where.append(f"(b {b}, y {yy}, x {xx}, c {c}: tile ({ly[k].item() // th}, {lx[k].item() // tw}) at ({iy[k].item()}, {ix[k].item()})"
                     f" sub-pixel ({yy % r}, {xx % r}))")
    place = ("all on the image border" if bool(border.all()) else
             "all on a tile seam" if bool(seam.all()) else
             "all on the image border or a tile seam" if bool((border | seam).all()) else
             f"{int(border.sum())} on the image border, {int((seam & ~border).sum())} more on a tile seam, the rest inside tiles")
    return f"{n} of {bad.numel()} differ, {place}; first: " + "; ".join(where)


def assert_bit_equal(got, ref, tile=TILE, r=1, what="", layout="nhwc", region=None):
    """torch.equal(got, ref) with a failure message that places the mismatches: (b, y, x, c), the tile and the position inside it
    (tile is in LR pixels, r the PixelShuffle factor of the output), the sub-pixel, and whether all of them lie on the image
    border or on a tile seam.  layout: "nhwc" / "nchw" for images, None for anything else.  region: a [Y][X] bool mask; only
    pixels inside it are compared (the ring and the interior of branch A are asserted separately)."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.dtype == ref.dtype, f"{what}: dtype {got.dtype} vs reference {ref.dtype}"
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs reference {tuple(ref.shape)}"
    if region is not None:
        m = region.view(1, 1, *region.shape) if layout == "nchw" else region.view(1, *region.shape, 1)
        zero = torch.zeros((), dtype=got.dtype)
        got, ref = torch.where(m, got, zero), torch.where(m, ref, zero)
    if torch.equal(got, ref):
        return
    bad = ~(got == ref)                     # NaN counts as a mismatch
    d = (got.double() - ref.double()).abs()
    raise AssertionError(f"{what}: not bit-equal to the reference: {_describe(bad, tile, r, layout)}; max |diff| {d[bad].max().item():g}")


def out_of(ref, bf16_out):
    """The tensor a kernel must produce from the exact reference: bf16 by round-to-nearest-even, or fp32."""
    return ref.to(torch.bfloat16) if bf16_out else ref.float()


# ------------------------------------------------------------------------------------------------
# the case tables: operands and references of every comparison of tests/test_hip_conv_exact.py; tests/test_conv_exact_cpu.py
# walks the same tables and shows each reference exact (fp32 == fp64, the preconditions) without a GPU
# ------------------------------------------------------------------------------------------------
class Case:
    """operands: name -> CPU fp32 tensor (NCHW); refs(dtype) -> name -> reference in the kernel's output layout; bf16: the names
    of the outputs (and middle maps) a kernel stores as bf16; rounding: a case whose bf16 outputs are meant to exceed 256."""

    def __init__(self, ident, operands, refs, bf16=(), rounding=False):
        self.id, self.operands, self.refs, self.bf16, self.rounding = ident, operands, refs, frozenset(bf16), rounding
        self.share_key = bf16[0] if rounding else None          # the output whose share above 256 a rounding case asserts

    def expected(self, dtype):
        return {k: out_of(v, k in self.bf16) for k, v in self.refs(dtype).items()}


def _sid(shape):
    return "x".join(str(v) for v in shape)


def c64_case(shape, r, want=("plain", "relu", "addmask"), rounding=False):
    """conv_c64 forward.  Default operands: x in +-2 (half zeros), w ternary (half zeros), |b| <= 3: K = 576 products of variance
    0.625 give |y| ~ 19 rms, far inside 256.  Rounding: x in +-8, w in +-4, dense: |y| ~ 330 rms."""
    B, H, W = shape
    s = 1000 + 10 * r
    o = {"x": ints((B, 64, H, W), s, 8 if rounding else 2, 1.0 if rounding else 0.5),
         "w": ints((64 * r * r, 64, 3, 3), s + 1, 4 if rounding else 1, 1.0 if rounding else 0.5),
         "b": ints((64 * r * r,), s + 2, 3)}
    if "addmask" in want:
        o["add"] = ints((B, 64, H * r, W * r), s + 3, 3)
        o["mask"] = ints((B, 64, H * r, W * r), s + 4, 1, 0.66)          # +1, 0 and -1, a third each

    def refs(dtype):
        y = F.pixel_shuffle(F.conv2d(o["x"].to(dtype), o["w"].to(dtype), o["b"].to(dtype), padding=1), r)
        out = {}
        if "plain" in want:
            out["plain"] = nhwc(y)
        if "relu" in want:
            out["relu"] = nhwc(F.relu(y))
        if "addmask" in want:
            out["addmask"] = nhwc((F.relu(y) + o["add"].to(dtype)) * (o["mask"] > 0))
        return out
    return Case(f"c64-r{r}-{_sid(shape)}" + ("-rounding" if rounding else ""), o, refs, bf16=want, rounding=rounding)


def thin_case(shape, cout):
    B, H, W = shape
    s = 2000 + cout
    o = {"x": ints((B, 64, H, W), s, 2, 0.5), "w": ints((cout, 64, 3, 3), s + 1, 2, 0.5), "b": ints((cout,), s + 2, 3)}

    def refs(dtype):
        y = F.conv2d(o["x"].to(dtype), o["w"].to(dtype), None, padding=1)
        yb = y + o["b"].to(dtype).view(1, -1, 1, 1)
        return {"b0r0": y, "b0r1": F.relu(y), "b1r0": yb, "b1r1": F.relu(yb)}
    return Case(f"thin{cout}-{_sid(shape)}", o, refs)


def conv1_case(shape, rounding=False):
    """conv1 (3 -> 64) on integer fp32 planes.  Default: |x| <= 3, |w| <= 2: at most 27 * 6 + 3 = 165 <= 256 by construction."""
    B, H, W = shape
    s = 3000
    o = {"x": ints((B, 3, H, W), s, 24 if rounding else 3, 1.0 if rounding else 0.8),
         "w": ints((64, 3, 3, 3), s + 1, 6 if rounding else 2, 1.0 if rounding else 0.7), "b": ints((64,), s + 2, 3),
         "in_mask": ints((B, 3, H, W), s + 3, 1, 0.66), "out_mask": ints((B, 64, H, W), s + 4, 1, 0.66)}

    def refs(dtype):
        return {"plain": conv1_ref(o["x"], o["w"], o["b"], False, dtype=dtype),
                "relu": conv1_ref(o["x"], o["w"], o["b"], True, dtype=dtype),
                "masked": conv1_ref(o["x"], o["w"], o["b"], False, o["in_mask"], o["out_mask"], dtype=dtype)}
    return Case(f"conv1-{_sid(shape)}" + ("-rounding" if rounding else ""), o, refs, bf16=("plain", "relu", "masked"), rounding=rounding)


def conv12_case(shape, rounding=False):
    """conv1_compact -> conv12_fused.  Default: conv1's map is at most 27 * 2 + 2 = 56; conv2 ternary with 1/8 non-zeros."""
    B, H, W = shape
    s = 4000
    o = {"x": ints((B, 3, H, W), s, 8 if rounding else 2, 1.0 if rounding else 0.5),
         "w1": ints((64, 3, 3, 3), s + 1, 4 if rounding else 1, 1.0 if rounding else 0.5), "b1": ints((64,), s + 2, 2),
         "w2": ints((64, 64, 3, 3), s + 3, 2 if rounding else 1, 1.0 if rounding else 0.125), "b2": ints((64,), s + 4, 3)}

    def refs(dtype):
        y, mid = conv12_ref(o["x"], o["w1"], o["b1"], o["w2"], o["b2"], dtype)
        return {"out": y, "mid": mid}
    return Case(f"conv12-{_sid(shape)}" + ("-rounding" if rounding else ""), o, refs, bf16=("out", "mid"), rounding=rounding)


def decoder_case(shape):
    """decoder_fused: the 64-channel map (bf16 in the kernel) stays within 256; the fp32 result only has to stay below 2**24."""
    B, H, W = shape
    s = 5000
    o = {"x": ints((B, 64, H, W), s, 2, 0.5), "w1": ints((64, 64, 3, 3), s + 1, 1, 0.5), "b1": ints((64,), s + 2, 3),
         "w2": ints((3, 64, 3, 3), s + 3, 2, 0.5), "b2": ints((3,), s + 4, 3)}

    def refs(dtype):
        y, mid = decoder_ref(o["x"], o["w1"], o["b1"], o["w2"], o["b2"], dtype)
        return {"out": y, "mid": mid}
    return Case(f"decoder-{_sid(shape)}", o, refs, bf16=("mid",))


def bra_case(shape, r):
    B, H, W = shape
    s = 6000 + r
    wu, bu, w3 = branch_a_weights(r, s)
    o = {"feat": ints((B, 64, H, W), s + 5, 2, 0.5), "wu": wu, "bu": bu, "w3": w3}

    def refs(dtype):
        y = branch_a_ref(o["feat"], wu, bu, w3, r, relu=False, dtype=dtype)
        return {"plain": y, "relu": F.relu(y)}
    return Case(f"bra-r{r}-{_sid(shape)}", o, refs)


def c64_bwd_case(shape, r, rounding=False):
    """Backward of conv 64 -> 64rr + PixelShuffle(r): dx (bf16, the forward kernel with in_r = r) sums 576 rr products, so the
    output gradient gets sparser with r (about 1.4 / rr non-zeros) to keep |dx| within 256; dw, db are fp32."""
    B, H, W = shape
    s = 7000 + r
    o = {"x": ints((B, 64, H, W), s, 2, 0.5), "w": ints((64 * r * r, 64, 3, 3), s + 1, 4 if rounding else 1, 1.0 if rounding else 0.5),
         "b": ints((64 * r * r,), s + 2, 2),
         "gy": ints((B, 64, H * r, W * r), s + 3, 8 if rounding else 1, 1.0 if rounding else min(0.5, 1.4 / (r * r)))}
    if r == 1:
        o["add"] = ints((B, 64, H, W), s + 4, 3)
        o["mask"] = ints((B, 64, H, W), s + 5, 1, 0.66)

    def refs(dtype):
        dx, dw, db = conv_grads(o["x"], o["w"], o["b"], o["gy"], r, dtype=dtype)
        out = {"dx": nhwc(dx), "dw": dw, "db": db}
        if r == 1:
            out["dx_addmask"] = nhwc((dx + o["add"].to(dtype)) * (o["mask"] > 0))
        return out
    return Case(f"c64bwd-r{r}-{_sid(shape)}" + ("-rounding" if rounding else ""), o, refs, bf16=("dx", "dx_addmask"), rounding=rounding)


def s2d_case(shape):
    """Weight gradient of Conv2d(64, 64, 3, stride=2, padding=1): x is [B][64][2H][2W], the output gradient [B][64][H][W]."""
    B, H, W = shape
    s = 7100
    o = {"x": ints((B, 64, 2 * H, 2 * W), s, 2, 0.5), "w": ints((64, 64, 3, 3), s + 1, 1, 0.5), "b": ints((64,), s + 2, 2),
         "gy": ints((B, 64, H, W), s + 3, 2, 0.5)}

    def refs(dtype):
        _, dw, db = conv_grads(o["x"], o["w"], o["b"], o["gy"], 1, stride=2, dtype=dtype)
        return {"dw": dw, "db": db}
    return Case(f"s2d-{_sid(shape)}", o, refs)


def thin_bwd_case(shape):
    """Backward of the 64 -> 3 conv: dw / db (thin weight-gradient kernel) and dx (bf16, the conv1 kernel on the flipped weights),
    plain and with both masks: the gradient gated by (m > 0) on the way in and by (z > 0) on the way out."""
    B, H, W = shape
    s = 7200
    o = {"x": ints((B, 64, H, W), s, 2, 0.5), "w": ints((3, 64, 3, 3), s + 1, 2, 0.5), "b": ints((3,), s + 2, 2),
         "gy": ints((B, 3, H, W), s + 3, 3, 0.8), "m": ints((B, 3, H, W), s + 4, 1, 0.66), "z": ints((B, 64, H, W), s + 5, 1, 0.66)}

    def refs(dtype):
        dx, dw, db = conv_grads(o["x"], o["w"], o["b"], o["gy"], dtype=dtype)
        dxm, _, _ = conv_grads(o["x"], o["w"], o["b"], o["gy"] * (o["m"] > 0), dtype=dtype)
        return {"dw": dw, "db": db, "dx": nhwc(dx), "dx_masked": nhwc(dxm * (o["z"] > 0))}
    return Case(f"thinbwd-{_sid(shape)}", o, refs, bf16=("dx", "dx_masked"))


def conv1_wgrad_case(shape):
    B, H, W = shape
    s = 7300
    o = {"x": ints((B, 3, H, W), s, 3, 0.8), "w": ints((64, 3, 3, 3), s + 1, 1), "b": ints((64,), s + 2, 1),
         "gy": ints((B, 64, H, W), s + 3, 2, 0.5)}

    def refs(dtype):
        _, dw, db = conv_grads(o["x"], o["w"], o["b"], o["gy"], dtype=dtype)
        return {"dw": dw, "db": db}
    return Case(f"conv1wgrad-{_sid(shape)}", o, refs)


def planar_bwd_case(shape, r):
    B, H, W = shape
    s = 7400 + r
    o = {"x": ints((B, 3, H, W), s, 3, 0.8), "w": ints((3 * r * r, 3, 3, 3), s + 1, 3, 0.8), "b": ints((3 * r * r,), s + 2, 1),
         "gy": ints((B, 3, H * r, W * r), s + 3, 3, 0.8)}

    def refs(dtype):
        dx, dw, db = conv_grads(o["x"], o["w"], o["b"], o["gy"], r, dtype=dtype)
        return {"dx": dx, "dw": dw, "db": db}
    return Case(f"planarbwd-r{r}-{_sid(shape)}", o, refs)


def fgc_case(shape, rounding=False):
    """feat_grad_combine: three bf16 maps added (the third folded back through the reflect padding to a multiple of 8) and gated."""
    B, H, W = shape
    s = 7500
    hp, wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
    amp = 256 if rounding else 20
    o = {"a": ints((B, 64, H, W), s, amp), "b": ints((B, 64, H, W), s + 1, amp), "gpe": ints((B, 64, hp, wp), s + 2, amp),
         "feat": ints((B, 64, H, W), s + 3, 1, 0.66)}

    def refs(dtype):
        return {"two": feat_grad_combine_ref(o["a"], o["b"], o["gpe"], o["feat"], dtype),
                "one": feat_grad_combine_ref(o["a"], None, o["gpe"], o["feat"], dtype)}
    return Case(f"fgc-{_sid(shape)}" + ("-rounding" if rounding else ""), o, refs, bf16=("two", "one"), rounding=rounding)


def bra_bwd_case(shape, rounding=False):
    """Backward of the composed branch A at r = 2, gated by the reference's own ui: dfeat is bf16, dwu / dbu / dw3 fp32."""
    B, H, W = shape
    s = 7600
    wu, bu, w3 = branch_a_weights(2, s, 2 if rounding else 1, 0.5 if rounding else 0.25)
    o = {"feat": ints((B, 64, H, W), s + 5, 2, 0.5), "wu": wu, "bu": bu, "w3": w3,
         "g": ints((B, 3, 2 * H, 2 * W), s + 6, 8 if rounding else 1, 1.0 if rounding else 0.25)}

    def refs(dtype):
        ui, dfeat, dwu, dbu, dw3 = branch_a_grads(o["feat"], wu, bu, w3, o["g"], dtype)
        return {"ui": ui, "dfeat": nhwc(dfeat), "dwu": dwu, "dbu": dbu, "dw3": dw3}
    return Case(f"brabwd-{_sid(shape)}" + ("-rounding" if rounding else ""), o, refs, bf16=("dfeat",), rounding=rounding)


THIN3_EXTRA = [(4, 117, 440)]          # 15 x 16 x 4 = 960 tiles of 8 x 28 > the thin-rows kernel's 768 workgroups: second tiles there
THIN_SCHEDULES = [(sh, co) for sh in SCHEDULES for co in (3, 16)] + [(sh, 3) for sh in THIN3_EXTRA]
ROUNDING_SHAPE = (2, 19, 70)


def all_cases():
    """name (= Case.id) -> builder of every case the GPU file runs (built lazily: the large ones hold hundreds of MB)."""
    t = {}
    sid = _sid
    for sh in SHAPES:
        for r in (1, 2, 3, 6):
            t[f"c64-r{r}-{sid(sh)}"] = lambda sh=sh, r=r: c64_case(sh, r, want=("plain", "relu", "addmask") if r <= 2 else ("plain", "relu"))
            t[f"c64bwd-r{r}-{sid(sh)}"] = lambda sh=sh, r=r: c64_bwd_case(sh, r)
            t[f"planarbwd-r{r}-{sid(sh)}"] = lambda sh=sh, r=r: planar_bwd_case(sh, r)
        for co in (3, 16):
            t[f"thin{co}-{sid(sh)}"] = lambda sh=sh, co=co: thin_case(sh, co)
        for prefix, fn in (("conv1", conv1_case), ("conv12", conv12_case), ("s2d", s2d_case), ("thinbwd", thin_bwd_case),
                           ("conv1wgrad", conv1_wgrad_case)):
            t[f"{prefix}-{sid(sh)}"] = lambda sh=sh, fn=fn: fn(sh)
        if min(sh[1:]) >= BRA_BWD_MIN:
            t[f"brabwd-{sid(sh)}"] = lambda sh=sh: bra_bwd_case(sh)
    for sh in DECODER_SHAPES:
        t[f"decoder-{sid(sh)}"] = lambda sh=sh: decoder_case(sh)
    for sh in FGC_SHAPES:
        t[f"fgc-{sid(sh)}"] = lambda sh=sh: fgc_case(sh)
    for sh in SHAPES + BRA_EXTRA + SCHEDULES:
        for r in ((2,) if sh in SCHEDULES else (2, 3, 6)):
            t[f"bra-r{r}-{sid(sh)}"] = lambda sh=sh, r=r: bra_case(sh, r)
    for sh in SCHEDULES:
        t[f"c64-r1-{sid(sh)}"] = lambda sh=sh: c64_case(sh, 1, want=("addmask",))
        t[f"c64-r2-{sid(sh)}"] = lambda sh=sh: c64_case(sh, 2, want=("plain",))
        t[f"conv12-{sid(sh)}"] = lambda sh=sh: conv12_case(sh)           # conv12_fused_kernel and decoder_fused_kernel walk the
        t[f"decoder-{sid(sh)}"] = lambda sh=sh: decoder_case(sh)         # same two-group schedule (csrc/conv_pingpong.h)
    for sh, co in THIN_SCHEDULES:
        t[f"thin{co}-{sid(sh)}"] = lambda sh=sh, co=co: thin_case(sh, co)
    rs = sid(ROUNDING_SHAPE)
    t[f"c64-r1-{rs}-rounding"] = lambda: c64_case(ROUNDING_SHAPE, 1, rounding=True)
    t[f"c64bwd-r2-{rs}-rounding"] = lambda: c64_bwd_case(ROUNDING_SHAPE, 2, rounding=True)
    for prefix, fn in (("conv1", conv1_case), ("conv12", conv12_case), ("fgc", fgc_case), ("brabwd", bra_bwd_case)):
        t[f"{prefix}-{rs}-rounding"] = lambda fn=fn: fn(ROUNDING_SHAPE, rounding=True)
    return t
