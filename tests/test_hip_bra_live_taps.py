"""Composed branch A at r = 2 on its live taps only (csrc/conv3x3_c64.hip: bra_rows_persistent_kernel skips the dead tap rows and
columns of every sub-pixel, conv5x5_border_fix_kernel walks the <= 8 live in-image taps of a ring pixel).

Shapes: one pixel (all ring); exactly one 8 x 28 tile; one extra row and column of tiles; seams in both directions with batch 2.
(a) against the fp64 application of the same bf16 composed weights, at test_branch_a_composed_training's tolerance;
(b) the same call with every dead tap of wp and wv overwritten by large finite values is bit-identical: the kernels do not read
    them, which is the contract of tup_conv5x5_c64_planar_fwd at r = 2;
(c) an image computed alone equals the same image computed in a batch, bit for bit."""
import pytest
import torch

import _bra_live_ref as L          # tests/ is on sys.path (rootdir-less test modules)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 8, 28), (1, 9, 29), (2, 19, 70)]
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else None


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from transformerupscaler_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def weights(dev):
    """(wp, bias, wv, bv) from packing.pack_branch_a and from ops.bra_compose, on the device; the CPU copies for the reference."""
    from transformerupscaler_amd import ops, packing
    g = torch.Generator().manual_seed(77)
    wu, bu, w3 = torch.randn((256, 64, 3, 3), generator=g) * 0.04, torch.randn((256,), generator=g) * 0.1, torch.randn((3, 64, 3, 3), generator=g) * 0.04
    host = packing.pack_branch_a(wu, bu, w3, 2)
    comp = ops.bra_compose(wu.to(dev), bu.to(dev), w3.to(dev))
    return {"pack_branch_a": tuple(t.to(dev) for t in host), "bra_compose": (comp["wp"], comp["bias"], comp["wv"], comp["bv"])}


def _feat(shape, dev):
    B, H, W = shape
    g = torch.Generator().manual_seed(31 + H)
    x = (torch.randn((B, H, W, 64), generator=g) * 0.7).to(torch.bfloat16)
    return x, x.to(dev)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_matches_fp64_of_bf16_weights(dev, weights, shape, relu):
    from transformerupscaler_amd import ops
    x_cpu, x = _feat(shape, dev)
    for name, (wp, bias, wv, bv) in weights.items():
        ref = L.apply_fp64(x_cpu, wp.cpu(), bias.cpu(), wv.cpu(), bv.cpu(), 2, relu)
        got = ops.branch_a_composed(x, wp, bias, wv, bv, 2, relu=relu).cpu().double()
        err = (got - ref).abs()
        bound = 3e-2 + 2e-2 * ref.abs()
        print(f"{name} {shape} relu={relu}: max abs err {err.max().item():.3e}")
        assert bool((err <= bound).all()), f"{name}: max err {err.max().item():.3e}, worst ratio {(err / bound).max().item():.2f}"


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_poisoned_dead_taps_are_not_read(dev, weights, shape):
    from transformerupscaler_amd import ops
    _, x = _feat(shape, dev)
    for name, (wp, bias, wv, bv) in weights.items():
        wp2, wv2 = L.poison_dead_taps(wp, wv)
        assert not torch.equal(wp2, wp) and not torch.equal(wv2, wv) and bool(torch.isfinite(wp2.float()).all())
        for relu in (True, False):
            clean = ops.branch_a_composed(x, wp, bias, wv, bv, 2, relu=relu)
            dirty = ops.branch_a_composed(x, wp2, bias, wv2, bv, 2, relu=relu)
            assert torch.equal(clean, dirty), f"{name} relu={relu}: {(clean != dirty).sum().item()} outputs changed"


def test_batch_equals_single(dev, weights):
    from transformerupscaler_amd import ops
    _, x = _feat((2, 19, 70), dev)
    wp, bias, wv, bv = weights["pack_branch_a"]
    both = ops.branch_a_composed(x, wp, bias, wv, bv, 2)
    for b in range(2):
        assert torch.equal(ops.branch_a_composed(x[b:b + 1].contiguous(), wp, bias, wv, bv, 2), both[b:b + 1])
