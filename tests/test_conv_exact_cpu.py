"""Exact-operand tests of the conv family, the part that runs without a GPU.

This file exists because of test_unit_change_of_one_tap_is_rejected_exactly_and_accepted_by_the_tolerance: a conv whose single
weight tap is off passes the tolerance comparison of tests/test_hip_kernels.py (the tap's whole contribution is inside the bound),
while on integer operands the smallest such fault changes an output by at least 1 and a bit-for-bit comparison sees it.

The rest shows, case by case and with none skipped, that the references tests/test_hip_conv_exact.py compares the kernels with
are themselves exact: the fp32 torch reference equals the fp64 one, every value is an integer below 2**24, and bf16 outputs of
the default cases stay within 256 (tests/_exact_ref.py states why those two bounds).  The CPU emulations of the packing
(test_boundary._emulate_conv_c64, packing.compose_branch_a) are held to the same equality."""
import pytest
import torch
import torch.nn.functional as F

import _exact_ref as R          # tests/ is on sys.path (rootdir-less test modules)

CASES = R.all_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_reference_is_exact(name):
    case = CASES[name]()
    r64, r32 = case.refs(torch.float64), case.refs(torch.float32)
    assert set(r64) == set(r32)
    for key, ref in r64.items():
        assert ref.dtype == torch.float64 and r32[key].dtype == torch.float32
        assert torch.equal(r32[key].double(), ref), f"{name}/{key}: the fp32 reference differs from the fp64 one"
        R.assert_exact_preconditions(ref, bf16_out=key in case.bf16, default_case=not case.rounding)
    for key, t in case.operands.items():          # the operands themselves survive the cast to bf16
        assert torch.equal(t.to(torch.bfloat16).float(), t), f"{name}: operand {key} is not exact in bf16"
    if case.rounding:
        share = R.share_above_256(r64[case.share_key])
        assert 0.05 <= share <= 0.95, f"{name}/{case.share_key}: {share:.3f} of the outputs exceed 256"
        ties = (r64[case.share_key].abs() > 256) & (r64[case.share_key] % 2 == 1)          # odd integers in (256, 512) are exact ties
        assert bool(ties.any()), "no value for round-to-nearest-even to break a tie on"


def test_case_tables_cover_what_the_issue_lists():
    names = set(CASES)
    for sh in R.SHAPES:
        s = R._sid(sh)
        for r in (1, 2, 3, 6):
            assert {f"c64-r{r}-{s}", f"c64bwd-r{r}-{s}", f"planarbwd-r{r}-{s}"} <= names
        assert {f"thin3-{s}", f"thin16-{s}", f"conv1-{s}", f"conv12-{s}", f"decoder-{s}", f"s2d-{s}", f"thinbwd-{s}",
                f"conv1wgrad-{s}"} <= names
    for sh in R.SHAPES + R.BRA_EXTRA:
        assert {f"bra-r{r}-{R._sid(sh)}" for r in (2, 3, 6)} <= names
    for sh in R.SCHEDULES:
        s = R._sid(sh)
        assert {f"c64-r1-{s}", f"c64-r2-{s}", f"thin3-{s}", f"thin16-{s}", f"bra-r2-{s}", f"conv12-{s}", f"decoder-{s}"} <= names
    assert "decoder-3x117x440" in names
    assert sum(n.endswith("-rounding") for n in names) == 6
    # tile counts the schedule comments promise (8 x 32 tiles; grid = min(tiles, 256); bands when grid % 8 == 0)
    tiles = lambda sh, tw=32: sh[0] * ((sh[1] + 7) // 8) * ((sh[2] + tw - 1) // tw)
    assert [tiles(sh) for sh in R.SCHED_LARGE] == [264, 630] and [tiles(sh, 28) for sh in R.SCHED_LARGE] == [312, 720]
    assert [tiles(sh) for sh in R.SCHED_SMALL] == [6, 18, 4, 8] and [tiles(sh, 28) for sh in R.SCHED_SMALL] == [6, 18, 4, 10]
    assert tiles(R.THIN3_EXTRA[0], 28) == 960


def test_branch_a_weights_compose_exactly_in_bf16():
    """The bound of _exact_ref.branch_a_weights: |Wc| <= 9 * 4 * amp_u, integer, so the bf16 packing of the composition is exact."""
    from transformerupscaler_amd import packing
    for r, amp in ((2, 1), (3, 1), (6, 1), (2, 2)):
        wu, bu, w3 = R.branch_a_weights(r, 6000 + r, amp, 0.5)
        assert int((w3 != 0).sum(1).max()) == 4 and int((w3 != 0).sum(1).min()) == 4 and float(w3.abs().max()) == 1
        wp, bias, wv, bv = packing.pack_branch_a(wu, bu, w3, r)
        for rm in range(3):
            for cm in range(3):
                wc, bc = packing.compose_branch_a(wu, bu, w3, r, rm, cm)
                assert torch.equal(wc, wc.round()) and float(wc.abs().max()) <= 36 * amp
                assert torch.equal(wv[rm * 3 + cm].float(), wc.reshape(3 * r * r, 25, 64))
                assert torch.equal(bv[rm * 3 + cm], bc) and torch.equal(bc, bc.round())


@pytest.mark.parametrize("r", [1, 2, 3, 6])
def test_emulated_conv_c64_packing_is_exact(r):
    """test_boundary._emulate_conv_c64 (what conv3x3_c64_kernel computes from pack_conv_c64's operands) on integer operands
    equals the reference exactly; the old test allows 1e-4."""
    from test_boundary import _emulate_conv_c64
    from transformerupscaler_amd import packing
    case = R.c64_case((2, 5, 7), r, want=("plain",))
    o = case.operands
    wp, bp = packing.pack_conv_c64(o["w"], o["b"], r)
    got = _emulate_conv_c64(R.nhwc(o["x"]), wp, bp, r)
    R.assert_bit_equal(got, case.refs(torch.float64)["plain"].float(), r=r, what=f"emulated conv_c64 r={r}")


@pytest.mark.parametrize("r", [2, 3, 6])
def test_compose_branch_a_is_exact(r):
    """packing.compose_branch_a, all 9 border variants, applied pixel by pixel as the kernels apply them, equals the explicit chain
    conv -> PixelShuffle -> conv exactly on a small map (3 x 4 LR: every variant occurs, the interior too)."""
    from transformerupscaler_amd import packing
    H, W = 3, 4
    case = R.bra_case((1, H, W), r)
    o = case.operands
    ref = case.refs(torch.float64)["plain"]
    var = {(rm, cm): packing.compose_branch_a(o["wu"], o["bu"], o["w3"], r, rm, cm) for rm in range(3) for cm in range(3)}
    fp = F.pad(o["feat"], (2, 2, 2, 2)).double()
    Hs, Ws = H * r, W * r
    out = torch.zeros_like(ref)
    used = set()
    for Y in range(Hs):
        for X in range(Ws):
            rm = 1 if Y == 0 else (2 if Y == Hs - 1 else 0)
            cm = 1 if X == 0 else (2 if X == Ws - 1 else 0)
            used.add((rm, cm))
            wc, bc = var[(rm, cm)]
            y, si, x, sj = Y // r, Y % r, X // r, X % r
            win = fp[0, :, y:y + 5, x:x + 5].permute(1, 2, 0)            # [5][5][64]
            n = torch.arange(3) * r * r + si * r + sj
            out[0, :, Y, X] = (wc[n].double() * win).sum((1, 2, 3)) + bc[n].double()
    assert len(used) == 9
    R.assert_bit_equal(out, ref, r=r, layout="nchw", what=f"composed branch A r={r}")


def _old_rnd(shape, seed, scale=1.0):
    """The operands of tests/test_hip_kernels.py (its rnd(), restated)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def test_unit_change_of_one_tap_is_rejected_exactly_and_accepted_by_the_tolerance():
    """One weight tap (one input channel, one of the 3 x 3 positions) of one output channel is off by the smallest amount the
    operands can express.
    Integer operands: the tap gains 1.  The reference then changes exactly in the outputs that tap reaches (that output channel,
    the pixels whose neighbour at the tap's offset is a non-zero input), by that input's value, at least 1, and assert_bit_equal
    rejects it.
    Operands of test_conv_c64_pixelshuffle (x uniform in +-1, w uniform in +-0.06, r = 1, 19 x 45): the same tap gains 0.015, a
    quarter of that test's weight amplitude.  Every output changes by 0.015 |x| <= 0.015, inside that test's bound
    1.5e-2 + 1e-2 |ref| everywhere: the tolerance comparison accepts the faulty conv."""
    co, ci, ky, kx = 37, 11, 0, 2
    H, W = 19, 45
    case = R.c64_case((2, H, W), 1, want=("plain",))
    o = case.operands
    ref = case.refs(torch.float64)["plain"]
    w_bad = o["w"].clone()
    w_bad[co, ci, ky, kx] += 1
    bad = R.conv_c64_ref(o["x"], w_bad, o["b"], 1)
    reach = torch.zeros_like(ref)                       # x at offset (ky - 1, kx - 1), zero padding outside
    xs = F.pad(o["x"][:, ci].double(), (1, 1, 1, 1))[:, ky:ky + H, kx:kx + W]
    reach[..., co] = xs
    assert torch.equal(bad - ref, reach)
    assert int((reach != 0).sum()) > 0 and float(reach[reach != 0].abs().min()) >= 1
    with pytest.raises(AssertionError, match="not bit-equal") as e:
        R.assert_bit_equal(bad.to(torch.bfloat16), ref.to(torch.bfloat16), what="one tap + 1")
    assert f"{int((reach != 0).sum())} of {ref.numel()} differ" in str(e.value)
    R.assert_bit_equal(ref.to(torch.bfloat16), ref.to(torch.bfloat16), what="unchanged")

    bf = lambda t: t.to(torch.bfloat16).float()
    x = bf(_old_rnd((2, 64, H, W), 4))
    w, b = bf(_old_rnd((64, 64, 3, 3), 5, 0.06)), _old_rnd((64,), 6, 0.2)
    old_ref = F.conv2d(x, w, b, padding=1)
    w_bad = w.clone()
    w_bad[co, ci, ky, kx] += 0.015
    err = (F.conv2d(x.double(), w_bad.double(), b.double(), padding=1) - old_ref.double()).abs()
    assert float(err.max()) > 0.01                                        # the fault is there ...
    assert bool((err <= 1.5e-2 + 1e-2 * old_ref.abs()).all())             # ... and the old bound holds it everywhere


def test_assert_bit_equal_places_the_mismatch():
    ref = torch.zeros(2, 16, 64, 4)
    got = ref.clone()
    got[1, 0, 5, 2] = 1
    with pytest.raises(AssertionError, match=r"1 of 8192 differ, all on the image border.*b 1, y 0, x 5, c 2.*tile \(0, 0\) at \(0, 5\)"):
        R.assert_bit_equal(got, ref, what="border")
    got = ref.clone()
    got[0, 8, 40, 0] = 1
    got[0, 7, 31, 1] = float("nan")
    with pytest.raises(AssertionError, match=r"2 of 8192 differ, all on a tile seam"):
        R.assert_bit_equal(got, ref, what="seam")
    got = ref.clone()
    got[0, 9, 21, 0] = 1                      # r = 2: LR pixel (4, 10), sub-pixel (1, 1)
    with pytest.raises(AssertionError, match=r"the rest inside tiles.*at \(4, 10\) sub-pixel \(1, 1\)"):
        R.assert_bit_equal(got, ref, r=2, what="inside")
    with pytest.raises(AssertionError, match="dtype"):
        R.assert_bit_equal(ref.to(torch.bfloat16), ref)
    ring = R.ring_mask(16, 64)
    got = ref.clone()
    got[0, 0, 0, 0] = 1
    R.assert_bit_equal(got, ref, region=~ring, what="interior only")
    with pytest.raises(AssertionError):
        R.assert_bit_equal(got, ref, region=ring, what="ring only")
