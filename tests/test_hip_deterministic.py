"""GPU checks of the deterministic weight-gradient convs (the *_det entries) and of the ordered slab reduce.

Every deterministic call runs on a fresh NaN-filled slab, so a slice a kernel failed to write would show.  Two calls must give
the same bits; the result must match an fp64 torch restatement of the same gradient (at the small shape), and the atomic form
to fp32-reordering noise.  ops.deterministic = True must route the wrappers to the same bits."""
import pytest
import torch
import torch.nn.functional as F

from transformerupscaler_amd import _lib, ops, packing

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(4, 720, 1280), (1, 36, 44)]          # config 3's maps and an odd B = 1 shape
# deterministic vs atomic form: the two differ only in the fp32 summation order of the per-workgroup partials.  Largest relative
# L2 distance measured over every case below on an MI355X: 1.16e-6 (the bias sums of the 4 x 720p thin case, 3.7 M pixels per
# output; every weight gradient <= 6.4e-7); the bound is about 9x that
REL_ATOMIC = 1e-5
# deterministic form vs an fp64 restatement of the same operands at 36 x 44: largest measured 1.34e-7 (planar r = 2 bias);
# the bound is about 15x that
REL_FP64 = 2e-6


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    ops.deterministic = False


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan_slab(kind, B, H, W, r=1):
    return torch.full((ops.conv_wgrad_slab_floats(kind, B, H, W, r),), float("nan"), dtype=torch.float32, device=DEV)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _check(det_call, atomic_out, name):
    """det_call() -> tuple of outputs (a fresh NaN slab per call): the two calls must be bit-identical and close to the atomic form."""
    first = det_call()
    second = det_call()
    for i, (a, b, ref) in enumerate(zip(first, second, atomic_out)):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)
        d = _rel(a, ref)
        print(f"{name}[{i}] det vs atomic rel L2 {d:.2e}")
        assert d <= REL_ATOMIC, (name, i, d)
    return first


def _fp64(name, got, ref):
    d = _rel(got, ref)
    print(f"{name} det vs fp64 rel L2 {d:.2e}")
    assert d <= REL_FP64, (name, d)


def _bf16(*shape, g):
    return torch.randn(shape, generator=g, device=DEV).to(torch.bfloat16)


def _nchw64(t):
    return t.permute(0, 3, 1, 2).double()


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("gr", [1, 2])
def test_c64_wgrad_det(B, H, W, gr):
    g = torch.Generator(device=DEV).manual_seed(1)
    x, gmap = _bf16(B, H, W, 64, g=g), _bf16(B, H * gr, W * gr, 64, g=g)
    ref = ops.conv_c64_wgrad(x, gmap, gr)

    def det():
        dwp = torch.zeros((gr * gr, 64, 9, 64), device=DEV)
        db = torch.zeros((gr * gr, 64), device=DEV)
        for sp in range(gr * gr):
            slab = _nan_slab(0, B, H, W)
            _lib.call("tup_conv3x3_c64_wgrad_det", x.data_ptr(), gmap.data_ptr(), dwp[sp].data_ptr(), db[sp].data_ptr(),
                      B, H, W, gr, sp, slab.data_ptr(), _stream())
        return dwp, db
    dwp, db = _check(det, ref, f"c64 gr={gr} {B}x{H}x{W}")
    if B * H * W <= 4096:
        # y = pixel_shuffle(conv2d(x, w, b, padding=1), gr): dW = conv2d_weight(x, pixel_unshuffle(gmap)), db = its pixel sums
        gpre = F.pixel_unshuffle(_nchw64(gmap), gr)
        dw64 = torch.nn.grad.conv2d_weight(_nchw64(x), (64 * gr * gr, 64, 3, 3), gpre, padding=1)
        dw, dbb = packing.unpack_conv_c64_wgrad(dwp, db, gr)
        _fp64(f"c64 gr={gr} dW", dw, dw64)
        _fp64(f"c64 gr={gr} db", dbb, gpre.sum((0, 2, 3)))
    ops.deterministic = True
    for a, b in zip(ops.conv_c64_wgrad(x, gmap, gr), (dwp, db)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_c64_wgrad_s2d_det(B, H, W):
    xr = 2
    H2, W2 = H // 2, W // 2
    g = torch.Generator(device=DEV).manual_seed(2)
    x, gmap = _bf16(B, H2 * xr, W2 * xr, 64, g=g), _bf16(B, H2, W2, 64, g=g)
    ref = ops.conv_c64_wgrad_s2d(x, gmap, xr)

    def det():
        dwp = torch.zeros((xr * xr, 64, 9, 64), device=DEV)
        db = torch.zeros((64,), device=DEV)
        for sp in range(xr * xr):
            slab = _nan_slab(0, B, H2, W2)
            _lib.call("tup_conv3x3_c64_wgrad_s2d_det", x.data_ptr(), gmap.data_ptr(), dwp[sp].data_ptr(),
                      db.data_ptr() if sp == 0 else None, B, H2, W2, xr, sp, slab.data_ptr(), _stream())
        return dwp, db
    dwp, db = _check(det, ref, f"c64 s2d {B}x{H}x{W}")
    if B * H * W <= 4096:
        dw64 = torch.nn.grad.conv2d_weight(_nchw64(x), (64, 64, 3, 3), _nchw64(gmap), stride=2, padding=1)
        _fp64("c64 s2d dW", packing.unpack_conv_c64_stride2_wgrad(dwp), dw64)
        _fp64("c64 s2d db", db, _nchw64(gmap).sum((0, 2, 3)))
    ops.deterministic = True
    for a, b in zip(ops.conv_c64_wgrad_s2d(x, gmap, xr), (dwp, db)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_thin_wgrad_det(B, H, W):
    g = torch.Generator(device=DEV).manual_seed(3)
    x = _bf16(B, H, W, 64, g=g)
    gpl = torch.randn((B, 3, H, W), generator=g, device=DEV)
    ref = ops.conv_thin_wgrad(x, gpl, True)

    def det():
        dwp = torch.zeros((3, 9, 64), device=DEV)
        db = torch.zeros((3,), device=DEV)
        slab = _nan_slab(1, B, H, W)
        _lib.call("tup_conv3x3_thin_wgrad_det", x.data_ptr(), gpl.data_ptr(), dwp.data_ptr(), db.data_ptr(), B, H, W,
                  slab.data_ptr(), _stream())
        return dwp, db
    dwp, db = _check(det, ref, f"thin {B}x{H}x{W}")
    if B * H * W <= 4096:
        # the kernel multiplies the bf16-rounded gradient (its MFMA operand); the bias sums the fp32 gradient
        dw64 = torch.nn.grad.conv2d_weight(_nchw64(x), (3, 64, 3, 3), gpl.to(torch.bfloat16).double(), padding=1)
        _fp64("thin dW", dwp.permute(0, 2, 1).reshape(3, 64, 3, 3), dw64)
        _fp64("thin db", db, gpl.double().sum((0, 2, 3)))
    ops.deterministic = True
    for a, b in zip(ops.conv_thin_wgrad(x, gpl, True), (dwp, db)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("r", [1, 2, 3])
def test_planar_wgrad_det(B, H, W, r):
    g = torch.Generator(device=DEV).manual_seed(4 + r)
    x = torch.randn((B, 3, H, W), generator=g, device=DEV)
    gpl = torch.randn((B, 3, H * r, W * r), generator=g, device=DEV)
    ref = ops.conv_planar_wgrad(x, gpl, r)

    def det():
        dw = torch.zeros((3 * r * r, 3, 3, 3), device=DEV)
        db = torch.zeros((3 * r * r,), device=DEV)
        slab = _nan_slab(2, B, H, W, r)
        _lib.call("tup_conv3x3_planar_wgrad_det", x.data_ptr(), gpl.data_ptr(), dw.data_ptr(), db.data_ptr(), B, H, W, r,
                  slab.data_ptr(), _stream())
        return dw, db
    dw, db = _check(det, ref, f"planar r={r} {B}x{H}x{W}")
    if B * H * W <= 4096:
        # dw[co][ci][ky][kx] = sum G_pre[co][p] X[ci][p + tap - 1], G_pre = pixel-unshuffled gpl (all fp32 operands)
        gpre = F.pixel_unshuffle(gpl.double(), r)
        _fp64(f"planar r={r} dW", dw, torch.nn.grad.conv2d_weight(x.double(), (3 * r * r, 3, 3, 3), gpre, padding=1))
        _fp64(f"planar r={r} db", db, gpre.sum((0, 2, 3)))
    ops.deterministic = True
    for a, b in zip(ops.conv_planar_wgrad(x, gpl, r), (dw, db)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("nslab,n", [(1, 4), (3, 8), (7, 12), (21, 100), (256, 36928), (33, 3)])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_slab_reduce_sums_in_its_documented_order(nslab, n, accumulate):
    """out = [out +] ((group 0 + group 2) + (group 1 + group 3)), group y = slab[y] + slab[y + 4] + ... left to right:
    restated with fp32 torch adds (each correctly rounded), the result must be bit-identical."""
    g = torch.Generator(device=DEV).manual_seed(9 + nslab)
    slab = torch.randn((nslab, n), generator=g, device=DEV)
    out0 = torch.randn((n,), generator=g, device=DEV)
    out = out0.clone()
    _lib.call("tup_slab_reduce", slab.data_ptr(), n, nslab, out.data_ptr(), n, accumulate, _stream())
    groups = []
    for y in range(4):
        acc = torch.zeros((n,), device=DEV)
        for s in range(y, nslab, 4):
            acc = acc + slab[s]
        groups.append(acc)
    want = (groups[0] + groups[2]) + (groups[1] + groups[3])
    if accumulate:
        want = out0 + want
    assert torch.equal(out, want)
