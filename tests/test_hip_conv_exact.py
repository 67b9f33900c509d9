"""Exact-operand tests of the conv kernels on the MI355X: csrc/conv3x3_c64.hip, conv_thin.hip, conv12_fused.hip, decoder_fused.hip,
conv_bwd.hip and branch_a_train.hip against torch on the CPU, bit for bit.

The operands are small integers (tests/_exact_ref.py): every product and partial sum is an integer below 2**24, the fp32 result is
exact in any summation order, and an indexing error (a tap from the wrong neighbour on a border row, one sub-pixel of a
PixelShuffle, a tile seam, a tile the persistent schedule hands to the wrong group) changes some output by at least 1.  So every
comparison here is torch.equal with the torch reference, never with another HIP kernel and never within a bound;
tests/test_conv_exact_cpu.py shows without a GPU that each reference used here is itself exact.

Shapes: _exact_ref.SHAPES (all border; one partial tile; exactly one tile; a one-pixel second tile both ways + the batch stride;
3 x 3 tiles with seams on all sides) for every operation, _exact_ref.SCHEDULES for the persistent kernels (grid 256 with ragged
XCD bands and second tiles; several tiles per group with carries across rows and images; the round-robin branch), and the shapes
named at the tests for single operations."""
import pytest
import torch

import _exact_ref as R          # tests/ is on sys.path (rootdir-less test modules)

pytestmark = pytest.mark.gpu

ids = R._sid


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from transformerupscaler_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _expected(case, shape):
    return case.expected(R.ref_dtype(shape))


def _check_share(case, shape):
    """A rounding case really rounds: between 5 % and 95 % of the reference exceed 256."""
    share = R.share_above_256(case.refs(R.ref_dtype(shape))[case.share_key])
    assert 0.05 <= share <= 0.95, share


# ------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------
def _run_c64(dev, case, shape, r):
    from transformerupscaler_amd import ops, packing
    o, exp = case.operands, _expected(case, shape)
    x = R.nhwc_bf16(o["x"]).to(dev)
    wp, bp = (t.to(dev) for t in packing.pack_conv_c64(o["w"], o["b"], r))
    what = f"conv_c64 r={r} {shape}"
    if "plain" in exp:
        R.assert_bit_equal(ops.conv_c64(x, wp, bp, r, relu=False), exp["plain"], r=r, what=what)
        out = torch.full(tuple(exp["plain"].shape), -31744.0, dtype=torch.bfloat16, device=dev)          # sentinel, exact in bf16
        assert ops.conv_c64(x, wp, bp, r, relu=False, out=out) is out
        R.assert_bit_equal(out, exp["plain"], r=r, what=what + " out=")
    if "relu" in exp:
        R.assert_bit_equal(ops.conv_c64(x, wp, bp, r, relu=True), exp["relu"], r=r, what=what + " relu")
    if "addmask" in exp:
        add, mask = R.nhwc_bf16(o["add"]).to(dev), R.nhwc_bf16(o["mask"]).to(dev)
        R.assert_bit_equal(ops.conv_c64(x, wp, bp, r, relu=True, add=add, mask=mask), exp["addmask"], r=r, what=what + " relu + add + mask")


@pytest.mark.parametrize("r", [1, 2, 3, 6])
@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_conv_c64_forward(dev, shape, r):
    """conv_c64 with bias, relu off and on, out= over a sentinel, and at r = 1, 2 relu + add + mask (mask +1 / 0 / -1)."""
    _run_c64(dev, R.c64_case(shape, r, want=("plain", "relu", "addmask") if r <= 2 else ("plain", "relu")), shape, r)


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("shape", R.SCHEDULES, ids=ids)
def test_conv_c64_schedules(dev, shape, r):
    """The persistent schedule of conv_c64_persistent_kernel<4, NHWC>: r = 1 with relu + add + mask, r = 2 plain (four weight passes
    over the same tiles).  Tile counts per shape: _exact_ref.SCHED_LARGE / SCHED_SMALL."""
    _run_c64(dev, R.c64_case(shape, r, want=("addmask",) if r == 1 else ("plain",)), shape, r)


def _run_thin(dev, shape, cout):
    from transformerupscaler_amd import ops, packing
    case = R.thin_case(shape, cout)
    o, exp = case.operands, _expected(case, shape)
    x = R.nhwc_bf16(o["x"]).to(dev)
    wp, b = packing.pack_conv_c64_thin(o["w"]).to(dev), o["b"].to(dev)
    tile = R.TILE_ROWS if cout <= 4 else R.TILE
    for bias in (False, True):
        for relu in (False, True):
            got = ops.conv_c64_thin(x, wp, b if bias else None, cout, relu=relu)
            R.assert_bit_equal(got, exp[f"b{int(bias)}r{int(relu)}"], tile=tile, layout="nchw", what=f"thin cout={cout} bias={bias} relu={relu} {shape}")
    out = torch.full(tuple(exp["b1r0"].shape), -7777.0, device=dev)
    assert ops.conv_c64_thin(x, wp, b, cout, relu=False, out=out) is out
    R.assert_bit_equal(out, exp["b1r0"], tile=tile, layout="nchw", what=f"thin cout={cout} out= {shape}")


@pytest.mark.parametrize("cout", [3, 16])
@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_conv_c64_thin(dev, shape, cout):
    """conv_c64_thin: cout = 3 is conv3_thin_rows_kernel (8 x 28 tiles), cout = 16 the persistent kernel <1, PLANAR>."""
    _run_thin(dev, shape, cout)


@pytest.mark.parametrize("shape,cout", R.THIN_SCHEDULES, ids=lambda v: ids(v) if isinstance(v, tuple) else str(v))
def test_conv_c64_thin_schedules(dev, shape, cout):
    """cout = 16 walks the two-group schedule of 8 x 32 tiles; cout = 3 walks up to 768 one-group workgroups of 8 x 28 tiles, which
    only (4, 117, 440) (960 tiles, cout = 3 alone) makes take a second tile."""
    _run_thin(dev, shape, cout)


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_conv1(dev, shape):
    """conv1 on integer fp32 planes: relu off and on, and in_mask / out_mask."""
    from transformerupscaler_amd import ops, packing
    case = R.conv1_case(shape)
    o, exp = case.operands, _expected(case, shape)
    x, wp, b = o["x"].to(dev), packing.pack_conv1(o["w"]).to(dev), o["b"].to(dev)
    R.assert_bit_equal(ops.conv1(x, wp, b, relu=False), exp["plain"], what=f"conv1 {shape}")
    R.assert_bit_equal(ops.conv1(x, wp, b, relu=True), exp["relu"], what=f"conv1 relu {shape}")
    got = ops.conv1(x, wp, b, relu=False, in_mask=o["in_mask"].to(dev), out_mask=R.nhwc_bf16(o["out_mask"]).to(dev))
    R.assert_bit_equal(got, exp["masked"], what=f"conv1 masks {shape}")


def _run_conv12(dev, case, shape):
    from transformerupscaler_amd import ops, packing
    o, exp = case.operands, _expected(case, shape)
    B, H, W = shape
    w2, b2 = (t.to(dev) for t in packing.pack_conv_c64(o["w2"], o["b2"], 1))
    got = ops.conv12_fused(ops.conv1_compact(o["x"].to(dev)), H, W, packing.pack_conv1(o["w1"]).to(dev), o["b1"].to(dev), w2, b2)
    R.assert_bit_equal(got, exp["out"], what=f"conv12_fused {shape}")


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_conv12_fused(dev, shape):
    """conv1_compact -> conv12_fused against torch relu(conv(relu(conv))) with the middle map rounded to bf16."""
    _run_conv12(dev, R.conv12_case(shape), shape)


@pytest.mark.parametrize("shape", R.SCHEDULES, ids=ids)
def test_conv12_fused_schedules(dev, shape):
    """conv12_fused_kernel walks the two-group schedule of csrc/conv_pingpong.h: XCD bands with second tiles, round robin, one tile
    per XCD, groups with 0, 1 and 2 tiles (tile counts per shape: _exact_ref.SCHED_LARGE / SCHED_SMALL)."""
    _run_conv12(dev, R.conv12_case(shape), shape)


def _run_decoder(dev, shape):
    from transformerupscaler_amd import ops, packing
    case = R.decoder_case(shape)
    o, exp = case.operands, _expected(case, shape)
    p1, pb1 = (t.to(dev) for t in packing.pack_conv_c64(o["w1"], o["b1"], 1))
    got = ops.decoder_fused(R.nhwc_bf16(o["x"]).to(dev), p1, pb1, packing.pack_dec2_scatter(o["w2"]).to(dev), o["b2"].to(dev))
    R.assert_bit_equal(got, exp["out"], layout="nchw", what=f"decoder_fused {shape}")


@pytest.mark.parametrize("shape", R.DECODER_SHAPES, ids=ids)
def test_decoder_fused(dev, shape):
    """decoder_fused(finish=True) against torch conv -> relu -> bf16 -> conv + bias; (3, 117, 440) for the per-tile seam buffers."""
    _run_decoder(dev, shape)


@pytest.mark.parametrize("shape", R.SCHEDULES, ids=ids)
def test_decoder_fused_schedules(dev, shape):
    """decoder_fused_kernel over the same schedules as test_conv12_fused_schedules."""
    _run_decoder(dev, shape)


def _run_bra(dev, shape, r):
    from transformerupscaler_amd import ops, packing
    case = R.bra_case(shape, r)
    o, exp = case.operands, _expected(case, shape)
    B, H, W = shape
    feat = R.nhwc_bf16(o["feat"]).to(dev)
    packs = {"pack_branch_a": tuple(t.to(dev) for t in packing.pack_branch_a(o["wu"], o["bu"], o["w3"], r))}
    if r == 2:
        comp = ops.bra_compose(o["wu"].to(dev), o["bu"].to(dev), o["w3"].to(dev))
        packs["bra_compose"] = (comp["wp"], comp["bias"], comp["wv"], comp["bv"])
        for got, want, name in zip(packs["bra_compose"], packs["pack_branch_a"], ("wp", "bias", "wv", "bv")):
            R.assert_bit_equal(got, want, layout=None, what=f"bra_compose {name} vs packing.pack_branch_a")
    ring = R.ring_mask(H * r, W * r)
    tile = R.TILE_ROWS if r == 2 else R.TILE
    for name, (wp, bias, wv, bv) in packs.items():
        for relu in (True, False):
            got = ops.branch_a_composed(feat, wp, bias, wv, bv, r, relu=relu)
            ref = exp["relu" if relu else "plain"]
            what = f"branch_a_composed r={r} relu={relu} ({name}) {shape}"
            R.assert_bit_equal(got, ref, tile=tile, r=r, layout="nchw", region=ring, what=what + ", RING")
            R.assert_bit_equal(got, ref, tile=tile, r=r, layout="nchw", region=~ring, what=what + ", INTERIOR")


@pytest.mark.parametrize("r", [2, 3, 6])
@pytest.mark.parametrize("shape", R.SHAPES + R.BRA_EXTRA, ids=ids)
def test_branch_a_composed(dev, shape, r):
    """The composed 5 x 5 conv against the explicit chain conv -> PixelShuffle -> conv [-> relu]; the outermost HR ring (the border
    variants) and the interior asserted separately.  (1, 1, 5), (1, 2, 2), (1, 6, 6): the ring is most or all of the image."""
    _run_bra(dev, shape, r)


@pytest.mark.parametrize("shape", R.SCHEDULES, ids=ids)
def test_branch_a_composed_schedules(dev, shape):
    """bra_rows_persistent_kernel (r = 2) over 8 x 28 tiles: 312 and 720 tiles on 256 workgroups, and the round-robin shapes."""
    _run_bra(dev, shape, 2)


# ------------------------------------------------------------------------------------------------
# backward.  Every weight-gradient op runs twice: with float atomics and, inside ops.deterministic_mode(), through its slab form;
# both must equal the reference bit for bit, and so each other.
# ------------------------------------------------------------------------------------------------
def _modes():
    from transformerupscaler_amd import ops
    import contextlib
    return (("atomics", contextlib.nullcontext), ("deterministic", ops.deterministic_mode))


def _run_c64_bwd(dev, case, shape, r):
    from transformerupscaler_amd import ops, packing
    o, exp = case.operands, _expected(case, shape)
    gy, x = R.nhwc_bf16(o["gy"]).to(dev), R.nhwc_bf16(o["x"]).to(dev)
    wd = packing.pack_conv_c64_dgrad(o["w"], r).to(dev)
    R.assert_bit_equal(ops.conv_c64(gy, wd, None, 1, in_r=r), exp["dx"], what=f"conv_c64 dgrad in_r={r} {shape}")
    if "dx_addmask" in exp:
        got = ops.conv_c64(gy, wd, None, 1, add=R.nhwc_bf16(o["add"]).to(dev), mask=R.nhwc_bf16(o["mask"]).to(dev))
        R.assert_bit_equal(got, exp["dx_addmask"], what=f"conv_c64 dgrad + add + mask {shape}")
    for mode, ctx in _modes():
        with ctx():
            dwp, db = ops.conv_c64_wgrad(x, gy, r)
        dw, dbb = packing.unpack_conv_c64_wgrad(dwp, db, r)
        R.assert_bit_equal(dw, exp["dw"], layout=None, what=f"conv_c64_wgrad gr={r} ({mode}) {shape}")
        R.assert_bit_equal(dbb, exp["db"], layout=None, what=f"conv_c64_wgrad gr={r} bias ({mode}) {shape}")


@pytest.mark.parametrize("r", [1, 2, 3, 6])
@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_conv_c64_backward(dev, shape, r):
    """dgrad through pack_conv_c64_dgrad with in_r = r (r = 1 also with add + mask) and conv_c64_wgrad(gr = r)."""
    _run_c64_bwd(dev, R.c64_bwd_case(shape, r), shape, r)


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_conv_c64_wgrad_s2d(dev, shape):
    """conv_c64_wgrad_s2d at xr = 2: the weight gradient of the stride-2 conv ((B, H, W) is the gradient's map, x is twice that)."""
    from transformerupscaler_amd import ops, packing
    case = R.s2d_case(shape)
    o, exp = case.operands, _expected(case, shape)
    x, gy = R.nhwc_bf16(o["x"]).to(dev), R.nhwc_bf16(o["gy"]).to(dev)
    for mode, ctx in _modes():
        with ctx():
            dwp, db = ops.conv_c64_wgrad_s2d(x, gy, 2)
        R.assert_bit_equal(packing.unpack_conv_c64_stride2_wgrad(dwp), exp["dw"], layout=None, what=f"conv_c64_wgrad_s2d ({mode}) {shape}")
        R.assert_bit_equal(db, exp["db"], layout=None, what=f"conv_c64_wgrad_s2d bias ({mode}) {shape}")


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_conv_thin_backward(dev, shape):
    """conv_thin_wgrad with and without bias, and the thin dgrad through conv1, plain and with both masks."""
    from transformerupscaler_amd import ops, packing
    case = R.thin_bwd_case(shape)
    o, exp = case.operands, _expected(case, shape)
    x, gy = R.nhwc_bf16(o["x"]).to(dev), o["gy"].to(dev)
    for mode, ctx in _modes():
        for want_bias in (True, False):
            with ctx():
                dwp, db = ops.conv_thin_wgrad(x, gy, want_bias)
            R.assert_bit_equal(dwp.permute(0, 2, 1).reshape(3, 64, 3, 3), exp["dw"], layout=None, what=f"conv_thin_wgrad bias={want_bias} ({mode}) {shape}")
            if want_bias:
                R.assert_bit_equal(db, exp["db"], layout=None, what=f"conv_thin_wgrad bias ({mode}) {shape}")
            else:
                assert db is None
    wd = packing.pack_conv_thin_dgrad(o["w"]).to(dev)
    R.assert_bit_equal(ops.conv1(gy, wd, None, relu=False), exp["dx"], what=f"thin dgrad {shape}")
    got = ops.conv1(gy, wd, None, relu=False, in_mask=o["m"].to(dev), out_mask=R.nhwc_bf16(o["z"]).to(dev))
    R.assert_bit_equal(got, exp["dx_masked"], what=f"thin dgrad, both masks {shape}")


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_conv1_wgrad(dev, shape):
    """conv1_wgrad (the thin MFMA kernel with the maps swapped + a column sum) and conv1_wgrad_direct (fp32 VALU)."""
    from transformerupscaler_amd import ops
    case = R.conv1_wgrad_case(shape)
    o, exp = case.operands, _expected(case, shape)
    x, gy = o["x"].to(dev), R.nhwc_bf16(o["gy"]).to(dev)
    for mode, ctx in _modes():
        for name, fn in (("conv1_wgrad", ops.conv1_wgrad), ("conv1_wgrad_direct", ops.conv1_wgrad_direct)):
            with ctx():
                dw, db = fn(x, gy)
            R.assert_bit_equal(dw.contiguous(), exp["dw"], layout=None, what=f"{name} ({mode}) {shape}")
            R.assert_bit_equal(db, exp["db"], layout=None, what=f"{name} bias ({mode}) {shape}")


@pytest.mark.parametrize("r", [1, 2, 3, 6])
@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_conv_planar_backward(dev, shape, r):
    from transformerupscaler_amd import ops
    case = R.planar_bwd_case(shape, r)
    o, exp = case.operands, _expected(case, shape)
    x, gy = o["x"].to(dev), o["gy"].to(dev)
    for mode, ctx in _modes():
        with ctx():
            dw, db = ops.conv_planar_wgrad(x, gy, r)
        R.assert_bit_equal(dw, exp["dw"], layout=None, what=f"conv_planar_wgrad r={r} ({mode}) {shape}")
        R.assert_bit_equal(db, exp["db"], layout=None, what=f"conv_planar_wgrad r={r} bias ({mode}) {shape}")
    R.assert_bit_equal(ops.conv_planar_dgrad(gy, o["w"].to(dev), r), exp["dx"], layout="nchw", what=f"conv_planar_dgrad r={r} {shape}")


def _run_fgc(dev, case, shape):
    from transformerupscaler_amd import ops
    o, exp = case.operands, _expected(case, shape)
    a, b, gpe, feat = (R.nhwc_bf16(o[k]).to(dev) for k in ("a", "b", "gpe", "feat"))
    R.assert_bit_equal(ops.feat_grad_combine(a, b, gpe, feat), exp["two"], what=f"feat_grad_combine {shape}")
    R.assert_bit_equal(ops.feat_grad_combine(a, None, gpe, feat), exp["one"], what=f"feat_grad_combine, b = None {shape}")


@pytest.mark.parametrize("shape", R.FGC_SHAPES, ids=ids)
def test_feat_grad_combine(dev, shape):
    """The default shapes on which the reflect padding it folds back is defined (see _exact_ref.FGC_SHAPES), and (1, 5, 12)."""
    _run_fgc(dev, R.fgc_case(shape), shape)


def _run_bra_bwd(dev, case, shape):
    from transformerupscaler_amd import ops
    o, exp = case.operands, _expected(case, shape)
    B, H, W = shape
    wu, bu, w3 = (o[k].to(dev) for k in ("wu", "bu", "w3"))
    comp = ops.bra_compose(wu, bu, w3)
    # gated by the REFERENCE's ui, so that only the backward kernels are compared
    dfeat, dwu, dbu, dw3, _, _ = ops.bra_backward(o["g"].to(dev), exp["ui"].to(dev), R.nhwc_bf16(o["feat"]).to(dev), comp, wu, bu, w3)
    ring = R.ring_mask(H, W, 3)                       # bra_dgrad_ring_kernel: three LR rows / columns on every side
    R.assert_bit_equal(dwu, exp["dwu"], layout=None, what=f"bra_backward dwu {shape}")
    R.assert_bit_equal(dbu, exp["dbu"], layout=None, what=f"bra_backward dbu {shape}")
    R.assert_bit_equal(dw3, exp["dw3"], layout=None, what=f"bra_backward dw3 {shape}")
    R.assert_bit_equal(dfeat, exp["dfeat"], region=~ring, what=f"bra_backward dfeat {shape}, INTERIOR")
    R.assert_bit_equal(dfeat, exp["dfeat"], region=ring, what=f"bra_backward dfeat {shape}, RING")


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_bra_backward(dev, shape):
    """bra_backward at r = 2 (it has no deterministic form: autograd.py routes around it in that mode).  The wrapper refuses maps
    with a side below 6 with an error code; that refusal is what the two smallest shapes assert."""
    from transformerupscaler_amd import ops
    if min(shape[1:]) < R.BRA_BWD_MIN:
        B, H, W = shape
        z = lambda *s: torch.zeros(s, device=dev)
        comp = ops.bra_compose(z(256, 64, 3, 3), z(256), z(3, 64, 3, 3))
        with pytest.raises(RuntimeError, match="tup_bra_backward failed"):
            ops.bra_backward(z(B, 3, 2 * H, 2 * W), z(B, 3, 2 * H, 2 * W), torch.zeros((B, H, W, 64), dtype=torch.bfloat16, device=dev),
                             comp, z(256, 64, 3, 3), z(256), z(3, 64, 3, 3))
        return
    _run_bra_bwd(dev, R.bra_bwd_case(shape), shape)


# ------------------------------------------------------------------------------------------------
# rounding: one case per kernel with a bf16 output, operands raised until a visible share of the outputs exceeds 256, where bf16
# no longer holds every integer: the kernel's f32_to_bf16 (csrc/common.h promises round-to-nearest-even) against torch's cast
# ------------------------------------------------------------------------------------------------
def test_rounding_conv_c64(dev):
    case = R.c64_case(R.ROUNDING_SHAPE, 1, rounding=True)
    _check_share(case, R.ROUNDING_SHAPE)
    _run_c64(dev, case, R.ROUNDING_SHAPE, 1)


def test_rounding_conv_c64_dgrad(dev):
    """in_r = 2 takes conv3x3_c64_kernel, not the persistent one."""
    case = R.c64_bwd_case(R.ROUNDING_SHAPE, 2, rounding=True)
    _check_share(case, R.ROUNDING_SHAPE)
    _run_c64_bwd(dev, case, R.ROUNDING_SHAPE, 2)


def test_rounding_conv1(dev):
    from transformerupscaler_amd import ops, packing
    case = R.conv1_case(R.ROUNDING_SHAPE, rounding=True)
    _check_share(case, R.ROUNDING_SHAPE)
    o, exp = case.operands, _expected(case, R.ROUNDING_SHAPE)
    x, wp, b = o["x"].to(dev), packing.pack_conv1(o["w"]).to(dev), o["b"].to(dev)
    R.assert_bit_equal(ops.conv1(x, wp, b, relu=False), exp["plain"], what="conv1, rounding")
    R.assert_bit_equal(ops.conv1(x, wp, b, relu=True), exp["relu"], what="conv1 relu, rounding")


def test_rounding_conv12_fused(dev):
    case = R.conv12_case(R.ROUNDING_SHAPE, rounding=True)
    _check_share(case, R.ROUNDING_SHAPE)
    _run_conv12(dev, case, R.ROUNDING_SHAPE)


def test_rounding_feat_grad_combine(dev):
    case = R.fgc_case(R.ROUNDING_SHAPE, rounding=True)
    _check_share(case, R.ROUNDING_SHAPE)
    _run_fgc(dev, case, R.ROUNDING_SHAPE)


def test_rounding_bra_backward(dev):
    """The ring of dfeat (three LR rows / columns at the border) is summed by two kernels; it must still be rounded to bf16 once:
    bra_dgrad_ring_kernel forms the frame pixel's whole sum in fp32 (adding its share to the bf16 value bra_dgrad_kernel had stored
    rounded twice: 2507 of 170240 ring values were off by one bf16 step at this shape)."""
    case = R.bra_bwd_case(R.ROUNDING_SHAPE, rounding=True)
    _check_share(case, R.ROUNDING_SHAPE)
    _run_bra_bwd(dev, case, R.ROUNDING_SHAPE)
