"""GPU checks of the second stage of the deterministic training mode: the *_det forms of the weight-gradient GEMMs, the column
sums and the LayerNorm backward, and the property they exist for -- a bit-reproducible training step.

Per entry: every deterministic call runs on a fresh NaN-filled slab (a slice a kernel failed to write would show); two calls give
the same bits; the wrapper under ops.deterministic = True gives the same bits again.  Accuracy has two bounds:
  * against the atomic twin on the same operands (relative L2).  Both add the same fp32 products in another order, so this is
    reordering noise.  Largest value measured over every case below on an MI355X: 4.92e-7 (the column sums of a 460,800 x 64 bf16
    map; every weight-gradient GEMM <= 2.3e-7, LayerNorm dgamma / dbeta <= 3.4e-7); the bound REL_ATOMIC = 5e-6 is about 10x that
    (the rule of test_hip_deterministic.py);
  * against an fp64 torch restatement at the small shapes: the deterministic form may be at most twice as far from it as the
    atomic twin is on the same inputs, with a floor of 1e-7 relative (fp32 epsilon) for cases where the twin is exact by luck
    (measured: deterministic 0-1.9e-7, twins 0-3.3e-7; the deterministic form was the closer one in every case with M > 100).
The step: two fresh modules, same seed / weights / data, three harness.train_step calls each under ops.deterministic_mode():
losses, parameters and Adam moments must be torch.equal.  The reference-fixture gradient tests are re-run under the mode."""
import importlib

import pytest
import torch

import test_hip_parity_r2 as T_r2
import test_hip_rt_train as T_rt
import test_hip_train as T_ft
import test_window_transformer as T_wt
from transformerupscaler_amd import _lib, autograd, harness, ops
from transformerupscaler_amd.weights import deterministic_state_dict, rt_deterministic_state_dict, wt_deterministic_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda"
REL_ATOMIC = 5e-6                  # about 10x the largest measured 4.92e-7 (header)
FP64_FLOOR = 1e-7
BF16, F32 = torch.bfloat16, torch.float32
M3, MRT, M1 = 61440, 7200, 64          # config 3 (4 x 720p), ResidualTransformer x6 720p batch 2, one window


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    ops.deterministic = False
    ops.release_det_slabs()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan_slab(kind, M, NI, NJ=0):
    return torch.full((ops.wgrad_slab_floats(kind, M, NI, NJ),), float("nan"), dtype=F32, device=DEV)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _check(det_call, atomic_out, name, fp64=None):
    """det_call() -> tuple of outputs (a fresh NaN slab per call).  Bit-identical repeats, finite, close to the atomic twin, and --
    where an fp64 restatement is given -- at most twice as far from it as the twin."""
    first = det_call()
    second = det_call()
    for i, (a, b, ref) in enumerate(zip(first, second, atomic_out)):
        assert torch.isfinite(a).all(), (name, i)
        assert torch.equal(a, b), (name, i)
        d = _rel(a, ref)
        print(f"{name}[{i}] det vs atomic rel L2 {d:.2e}")
        assert d <= REL_ATOMIC, (name, i, d)
        if fp64 is not None:
            dd, da = _rel(a, fp64[i]), _rel(ref, fp64[i])
            print(f"{name}[{i}] vs fp64: det {dd:.2e}, atomic {da:.2e}")
            assert dd <= max(2 * da, FP64_FLOOR), (name, i, dd, da)
    return first


def _operand(M, N, dtype, g):
    return torch.randn((M, N), generator=g, device=DEV).to(dtype)


# ---- Linear weight + bias gradients (tup_gemm_wgrad_bias_det; colsum_out = NULL is the plain form) ----
GEMM_CASES = ([(M3, ni, nj, pd) for ni, nj in ((576, 192), (192, 192), (768, 192), (192, 768)) for pd in (BF16, F32)]
              + [(MRT, ni, nj, pd) for ni, nj in ((384, 128), (128, 128), (512, 128), (128, 512)) for pd in (BF16, F32)]
              + [(M1, 192, 192, BF16), (M1, 576, 192, F32), (M1, 128, 512, BF16)])


@pytest.mark.parametrize("M,NI,NJ,pdtype", GEMM_CASES)
def test_gemm_wgrad_bias_det(M, NI, NJ, pdtype):
    g = torch.Generator(device=DEV).manual_seed(11)
    p, q = _operand(M, NI, pdtype, g), _operand(M, NJ, BF16, g)
    code = {BF16: 0, F32: 1}
    ref = ops.gemm_wgrad_bias(p, q)

    def det(bias=True):
        out = torch.zeros((NI, NJ), device=DEV)
        db = torch.zeros((NI,), device=DEV)
        slab = _nan_slab(0, M, NI, NJ)
        _lib.call("tup_gemm_wgrad_bias_det", p.data_ptr(), code[pdtype], NI, q.data_ptr(), 0, NJ, out.data_ptr(), NJ,
                  db.data_ptr() if bias else None, M, NI, NJ, slab.data_ptr(), _stream())
        return (out, db) if bias else (out,)
    fp64 = None
    if M <= MRT:          # the kernel multiplies bf16-rounded operands; the column sums add what it multiplied
        pd = p.to(BF16).double()
        fp64 = (pd.T @ q.double(), pd.sum(0))
    dw, db = _check(det, ref, f"gemm {M}x{NI}x{NJ} {pdtype}", fp64)
    assert torch.equal(det(bias=False)[0], dw)          # the plain form: the same weight bits without the bias
    # weight and bias output side by side (the zero pool's layout): one reduce launch, the same bits
    both = torch.zeros((NI * NJ + NI,), device=DEV)
    slab = _nan_slab(0, M, NI, NJ)
    _lib.call("tup_gemm_wgrad_bias_det", p.data_ptr(), code[pdtype], NI, q.data_ptr(), 0, NJ, both.data_ptr(), NJ,
              both[NI * NJ:].data_ptr(), M, NI, NJ, slab.data_ptr(), _stream())
    assert torch.equal(both[:NI * NJ].view(NI, NJ), dw) and torch.equal(both[NI * NJ:], db)
    with ops.deterministic_mode():
        a, b = ops.gemm_wgrad_bias(p, q)
        assert torch.equal(a, dw) and torch.equal(b, db)
        assert torch.equal(ops.gemm_wgrad(p, q), dw)


def test_gemm_wgrad_det_padded_output():
    """ldo > NJ (no caller in the package, but the twin's contract): row-by-row reduce, the same bits, the padding untouched."""
    M, NI, NJ, ldo = MRT, 128, 128, 192
    g = torch.Generator(device=DEV).manual_seed(12)
    p, q = _operand(M, NI, BF16, g), _operand(M, NJ, BF16, g)
    with ops.deterministic_mode():
        want = ops.gemm_wgrad(p, q)
    out = torch.full((NI, ldo), 7.0, device=DEV)
    out[:, :NJ] = 0
    _lib.call("tup_gemm_wgrad_bias_det", p.data_ptr(), 0, NI, q.data_ptr(), 0, NJ, out.data_ptr(), ldo, None, M, NI, NJ,
              _nan_slab(0, M, NI, NJ).data_ptr(), _stream())
    assert torch.equal(out[:, :NJ], want) and (out[:, NJ:] == 7.0).all()


# ---- column sums ----
@pytest.mark.parametrize("M,N,dtype,masked", [(M3, 192, F32, True), (4 * 720 * 1280, 64, BF16, False), (MRT, 128, F32, False),
                                             (2 * 360 * 640, 64, BF16, False), (M1, 192, F32, True), (M1, 64, BF16, False),
                                             (100, 128, F32, False)])
def test_colsum_det(M, N, dtype, masked):
    g = torch.Generator(device=DEV).manual_seed(13)
    x = _operand(M, N, dtype, g)
    mask = (torch.rand((M,), generator=g, device=DEV) < 0.9).to(torch.uint8) if masked else None
    ref = (ops.colsum(x, rowmask=mask),)

    def det():
        out = torch.zeros((N,), device=DEV)
        slab = _nan_slab(2, M, N)
        _lib.call("tup_colsum_det", x.data_ptr(), {BF16: 0, F32: 1}[dtype], N, out.data_ptr(), M, N,
                  None if mask is None else mask.data_ptr(), slab.data_ptr(), _stream())
        return (out,)
    fp64 = None
    if M <= MRT:
        xd = x.double() if mask is None else x.double() * mask.double().view(-1, 1)
        fp64 = (xd.sum(0),)
    out, = _check(det, ref, f"colsum {M}x{N} {dtype}", fp64)
    with ops.deterministic_mode():
        assert torch.equal(ops.colsum(x, rowmask=mask), out)


# ---- LayerNorm backward ----
@pytest.mark.parametrize("M,C,drop", [(M3, 192, False), (M3, 192, True), (MRT, 128, True), (MRT, 192, False), (M1, 192, True),
                                      (M1, 128, False), (M1 + 5, 128, False)])
def test_layernorm_bwd_det(M, C, drop):
    g = torch.Generator(device=DEV).manual_seed(14)
    x = torch.randn((M, C), generator=g, device=DEV) * 1.5 + 0.3
    gy = _operand(M, C, BF16, g)
    gres = torch.randn((M, C), generator=g, device=DEV)
    gamma = torch.rand((C,), generator=g, device=DEV) + 0.5
    mean = x.mean(1).contiguous()
    rstd = (x.var(1, unbiased=False) + 1e-5).rsqrt().contiguous()
    wrapper = ops.layernorm_bwd
    entry = "tup_layernorm_bwd_det" if C == 192 else "tup_layernorm128_bwd_det"
    dr = (0.1, 12345) if drop else None
    ref = wrapper(gy, x, mean, rstd, gamma, gres=gres, drop=dr)

    def det():
        dx = torch.empty((M, C), device=DEV)
        dg, db = torch.zeros((C,), device=DEV), torch.zeros((C,), device=DEV)
        gd = torch.empty((M, C), dtype=BF16, device=DEV) if drop else None
        slab = _nan_slab(3, M, C)
        _lib.call(entry, gy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), gres.data_ptr(),
                  dx.data_ptr(), dg.data_ptr(), db.data_ptr(), M, gd.data_ptr() if drop else None, 0.1 if drop else 0.0,
                  12345 if drop else 0, slab.data_ptr(), _stream())
        return dx, dg, db
    fp64 = None
    if M <= MRT:
        xh = (x.double() - mean.double().view(-1, 1)) * rstd.double().view(-1, 1)
        fp64 = (ref[0], (gy.double() * xh).sum(0), gy.double().sum(0))          # dx is not a reduction: the twin's own bits
    dx, dg, db = _check(det, ref[:3], f"layernorm_bwd {M}x{C}", fp64)
    assert torch.equal(dx, ref[0])          # the row-wise part is the same code
    with ops.deterministic_mode():
        got = wrapper(gy, x, mean, rstd, gamma, gres=gres, drop=dr)
    assert torch.equal(got[0], dx) and torch.equal(got[1], dg) and torch.equal(got[2], db)
    if drop:
        assert torch.equal(got[3], ref[3])


# ---- patch weights ----
def _patches_windows(fmap, reflect):
    """fp64 [M][4096] patch matrix of an NHWC map in window-layout token rows (H, W multiples of 64: no padding involved)."""
    B, H, W, C = fmap.shape
    assert H % 64 == 0 and W % 64 == 0
    t = fmap.double().view(B, H // 64, 8, 8, W // 64, 8, 8, C)          # b, wy, ty, i, wx, tx, j, c
    return t.permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(-1, 4096)


def _patches_linear(fmap):
    B, H, W, C = fmap.shape
    t = fmap.double().view(B, H // 8, 8, W // 8, 8, C)                   # b, ty, i, tx, j, c
    return t.permute(0, 1, 3, 2, 4, 5).reshape(-1, 4096)


@pytest.mark.parametrize("B,H,W,reflect", [(4, 720, 1280, False), (4, 720, 1280, True), (2, 68, 84, True), (1, 64, 64, False),
                                           (1, 64, 64, True)])
@pytest.mark.parametrize("wide", [True, False])
def test_patch_wgrad_det(B, H, W, reflect, wide):
    _, _, nwy, nwx = ops.window_geometry(H, W)
    M = B * nwy * nwx * 64
    g = torch.Generator(device=DEV).manual_seed(15)
    p = torch.randn((M, 192), generator=g, device=DEV)
    fmap = torch.randn((B, H, W, 64), generator=g, device=DEV).to(BF16)
    saved = ops.PATCH_WGRAD_WIDE
    ops.PATCH_WGRAD_WIDE = wide
    try:
        ref = (ops.patch_wgrad(p, fmap, reflect),)
        pb = p.to(BF16)

        def det():
            out = torch.zeros((192, 4096), device=DEV)
            if wide:
                slab = _nan_slab(1, M, 192, 4096)
                _lib.call("tup_patch_wgrad_bf16_det", pb.data_ptr(), fmap.data_ptr(), out.data_ptr(), B, H, W, int(reflect),
                          slab.data_ptr(), _stream())
            else:
                slab = _nan_slab(0, M, 192, 4096)
                _lib.call("tup_patch_wgrad_det", p.data_ptr(), fmap.data_ptr(), out.data_ptr(), B, H, W, int(reflect),
                          slab.data_ptr(), _stream())
            return (out,)
        fp64 = (pb.double().T @ _patches_windows(fmap, reflect),) if (H, W) == (64, 64) else None
        out, = _check(det, ref, f"patch_wgrad {'wide' if wide else '64x64'} {B}x{H}x{W} reflect={reflect}", fp64)
        with ops.deterministic_mode():
            assert torch.equal(ops.patch_wgrad(p, fmap, reflect), out)
    finally:
        ops.PATCH_WGRAD_WIDE = saved


@pytest.mark.parametrize("B,H,W", [(2, 360, 640), (1, 64, 64)])
def test_rt_patch_wgrad_det(B, H, W):
    M = B * (H // 8) * (W // 8)
    g = torch.Generator(device=DEV).manual_seed(16)
    p = torch.randn((M, 128), generator=g, device=DEV)
    fmap = torch.randn((B, H, W, 64), generator=g, device=DEV).to(BF16)
    ref = (ops.rt_patch_wgrad(p, fmap),)

    def det():
        out = torch.zeros((128, 4096), device=DEV)
        slab = _nan_slab(0, M, 128, 4096)
        _lib.call("tup_rt_patch_wgrad_det", p.data_ptr(), fmap.data_ptr(), out.data_ptr(), B, H, W, slab.data_ptr(), _stream())
        return (out,)
    out, = _check(det, ref, f"rt_patch_wgrad {B}x{H}x{W}", (p.to(BF16).double().T @ _patches_linear(fmap),))
    with ops.deterministic_mode():
        assert torch.equal(ops.rt_patch_wgrad(p, fmap), out)


@pytest.mark.parametrize("B,H,W", [(4, 360, 640), (2, 44, 60), (1, 64, 64)])
def test_wt_patch_wgrad_det(B, H, W):
    NI = 128
    M = B * ((H // 8 + 7) // 8) * ((W // 8 + 7) // 8) * 64
    g = torch.Generator(device=DEV).manual_seed(17)
    p = torch.randn((M, NI), generator=g, device=DEV)
    fmap = torch.randn((B, H, W, 64), generator=g, device=DEV).to(BF16)
    ref = (ops.wt_patch_wgrad(p, fmap),)

    def det():
        out = torch.zeros((NI, 4096), device=DEV)
        slab = _nan_slab(0, M, NI, 4096)
        _lib.call("tup_wt_patch_wgrad_det", p.data_ptr(), fmap.data_ptr(), out.data_ptr(), B, H, W, NI, slab.data_ptr(), _stream())
        return (out,)
    fp64 = (p.to(BF16).double().T @ _patches_windows(fmap, False),) if (H, W) == (64, 64) else None
    out, = _check(det, ref, f"wt_patch_wgrad {B}x{H}x{W}", fp64)
    with ops.deterministic_mode():
        assert torch.equal(ops.wt_patch_wgrad(p, fmap), out)


# ---- the training step ----
def _model(plugin, sd_fn, strict, **kw):
    m = importlib.import_module(f"models.{plugin}.model").TransformerModel(**kw)
    m.load_state_dict(sd_fn(0), strict=strict)
    return m


STEP_CASES = {
    "ft_x2_720p_b4": (lambda: _model("FastTransformer", deterministic_state_dict, False), (4, 3, 720, 1280), (1080, 1920)),
    "ft_x3_68x84_b2": (lambda: _model("FastTransformer", deterministic_state_dict, False), (2, 3, 68, 84), (204, 252)),
    "ft_x4_64x64_b1": (lambda: _model("FastTransformer", deterministic_state_dict, False), (1, 3, 64, 64), (256, 256)),
    "rt_x6_720p_b2": (lambda: _model("ResidualTransformer", rt_deterministic_state_dict, True), (2, 3, 720, 1280), (4320, 7680)),
    "wt_x2_88x120_drop": (lambda: _model("WindowTransformer", wt_deterministic_state_dict, False, dropout=0.1), (2, 3, 88, 120), (176, 240)),
}


def _three_steps(build, lr, hr):
    torch.manual_seed(0)
    m = build().to(DEV).train()          # dropout active
    assert m.dropout_p > 0
    opt = harness.make_optimizer(m, 1e-4)
    with ops.deterministic_mode():
        losses = [harness.train_step(m, opt, lr, hr).clone() for _ in range(3)]
    torch.cuda.synchronize()
    state = {"loss": torch.stack(losses).cpu()}
    for k, p in m.named_parameters():
        state["param." + k] = p.detach().cpu().clone()
        st = opt.state.get(p, {})
        for s in ("exp_avg", "exp_avg_sq"):
            if s in st:
                state[f"{s}.{k}"] = st[s].detach().cpu().clone()
    del m, opt
    torch.cuda.empty_cache()
    return state


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_training_step_is_bit_reproducible(case):
    build, lr_shape, hr_hw = STEP_CASES[case]
    g = torch.Generator().manual_seed(2024)          # CPU generator
    lr = torch.rand(lr_shape, generator=g).to(DEV)
    hr = torch.rand((lr_shape[0], 3) + hr_hw, generator=g).to(DEV)
    a = _three_steps(build, lr, hr)
    b = _three_steps(build, lr, hr)
    assert torch.isfinite(a["loss"]).all()
    assert any(k.startswith("exp_avg.") for k in a) and any(k.startswith("exp_avg_sq.") for k in a)
    assert a.keys() == b.keys()
    differing = [k for k in a if not torch.equal(a[k], b[k])]
    print(case, "losses", a["loss"].tolist(), "differing tensors", differing[:8])
    assert not differing, (case, len(differing), differing[:8])


# ---- deterministic mode still computes the right gradient: the reference-fixture tests, under the mode ----
def test_fixture_gradients_hold_in_deterministic_mode(det_sd, golden_dir):
    with ops.deterministic_mode():
        T_ft.test_train_step_grads_match_reference(det_sd, golden_dir)
        T_r2.test_train_720p_grads_match_reference(det_sd, golden_dir)
        T_rt.test_full_size_train_grads_match_reference_fixture(golden_dir)
        T_wt.test_hip_train_grads_match_reference_fixture(golden_dir)


# ---- the two route-arounds ----
def test_deterministic_mode_routes_around_the_sites_without_a_twin(monkeypatch):
    calls, svs = [], []
    real_call, real_fwd = _lib.call, autograd.forward_train

    def spy_call(name, *args):
        calls.append((name, args))
        return real_call(name, *args)

    def spy_fwd(*a, **kw):
        out, sv = real_fwd(*a, **kw)
        svs.append(sv)
        return out, sv
    monkeypatch.setattr(_lib, "call", spy_call)
    monkeypatch.setattr(autograd, "forward_train", spy_fwd)
    m = _model("FastTransformer", deterministic_state_dict, False).to(DEV).train()
    opt = harness.make_optimizer(m, 1e-4)
    g = torch.Generator().manual_seed(5)
    lr, hr = torch.rand((1, 3, 64, 64), generator=g).to(DEV), torch.rand((1, 3, 128, 128), generator=g).to(DEV)

    def names():
        return [n for n, _ in calls]

    def merge_colsum_pointers():
        return [a[6] for n, a in calls if n == "tup_patch_embed_bwd_merge"]
    # the default route of this shape takes both sites (otherwise the check below would show nothing)
    harness.train_step(m, opt, lr, hr)
    assert svs[-1]["bra"] is True and "tup_bra_backward" in names()
    assert merge_colsum_pointers() and all(ptr is not None for ptr in merge_colsum_pointers())
    del calls[:]
    with ops.deterministic_mode():
        harness.train_step(m, opt, lr, hr)
    assert svs[-1]["bra"] is False
    assert "tup_bra_backward" not in names()
    assert merge_colsum_pointers() and all(ptr is None for ptr in merge_colsum_pointers())
    atomic = {"tup_gemm_wgrad", "tup_gemm_wgrad_bias", "tup_patch_wgrad", "tup_patch_wgrad_bf16", "tup_colsum", "tup_layernorm_bwd",
              "tup_conv3x3_c64_wgrad", "tup_conv3x3_thin_wgrad", "tup_conv3x3_planar_wgrad"}
    assert not atomic & set(names()), atomic & set(names())
    # a backward follows the forward that produced its sv: forward under the mode, backward outside it
    del calls[:]
    opt.zero_grad(set_to_none=True)
    with ops.deterministic_mode():
        out = m(lr, res_out=(128, 128), require_ratio=False)
    out.sum().backward()
    assert svs[-1]["bra"] is False and "tup_bra_backward" not in names()
