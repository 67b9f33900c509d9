"""GPU checks of losses.quality_loss (csrc/quality_loss.hip) against the float64 torch restatement (tests/_quality_loss_ref.py).

Value: each term within the bound the existing tests apply to that quantity (test_hip_metrics.py: |dSSIM| <= 1e-6, relative dMSE
<= 1e-6; test_hip_train.py's L1 loss test: |dL1| <= 1e-6); a weighted sum within the weighted sum of those bounds.
Gradient: relative L2 distance to the float64 autograd gradient of the restatement (of the same fp32 inputs).  The yardstick is the
same loss composed of torch ops in plain fp32 on the GPU, differentiated by autograd -- independent of the code under test; the HIP
gradient may be at most twice as far from float64 as that, with a floor of 1e-6 (the rule of test_hip_deterministic_step.py).
Measured on an MI355X over every case and weight set below: see MEASURED.
Bits: two runs are torch.equal; image 0's gradient at B = 1, times 1/4, is its slice of the B = 4 gradient exactly (the batch size
enters only through the scalars w / N and w / (3 B Nwin), and 4 is a power of two; at another B one rounding of those scalars
intervenes); the SSIM-only loss at B = 1 is 1 - metrics.ssim to the bit (one definition, one kernel).
"""
import importlib

import pytest
import torch

import _quality_loss_ref as R          # tests/ is on sys.path (rootdir-less test modules)
import test_hip_metrics as TM
from transformerupscaler_amd import _lib, harness, losses, metrics, ops
from transformerupscaler_amd.autograd import l1_loss, resize_aa
from transformerupscaler_amd.weights import deterministic_state_dict, rt_deterministic_state_dict, wt_deterministic_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SSIM_TOL, MSE_RTOL, L1_TOL = TM.SSIM_TOL, TM.MSE_RTOL, 1e-6
GRAD_FLOOR = 1e-6
# MEASURED on an MI355X (relative L2 to float64; HIP / the fp32 composition of torch ops), SSIM-only weights: B = 2 37x53 1.6e-6 /
# 9.7e-6; 103x257 1.9e-6 / 2.4e-5; blurred 96x300 1.95e-6 (the worst HIP value) / 2.6e-5; B = 4 1080x1920 9.7e-7 / 6.9e-5; flat bright
# 40x40 7.7e-8 / 5.8e-4.  Mixed weights: HIP <= 1.8e-6.  L1-only and MSE-only: both <= 3.9e-8 (identical to the composition).
# out == target: max|grad| N = 4.1e-5 against 44.5 on the blurred pair (ratio 9e-7; bound 1e-3).
WEIGHTS = {"ssim": (0.0, 0.0, 1.0), "mse": (0.0, 1.0, 0.0), "l1": (1.0, 0.0, 0.0), "mixed": (0.5, 0.2, 0.3)}


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    ops.deterministic = False
    ops.release_det_slabs()


def _stack(pairs):
    return torch.stack([p[0] for p in pairs]).contiguous(), torch.stack([p[1] for p in pairs]).contiguous()


def _blur_pair():
    return _stack([TM._case("blur", 96, 300, seed=1)])          # the metrics kernel's worst case (test_f32_4k_and_batch_of_three)


def _inputs(case):
    if case == "b2_37x53":                                       # smaller than one strip
        return _stack([TM._case("noise", 37, 53, seed=1), TM._case("blur", 37, 53, seed=2)])
    if case == "103x257":                                        # crosses the column and the 96-row ownership seams
        return _stack([TM._case("blur", 103, 257, seed=3)])
    if case == "blur_96x300":
        return _blur_pair()
    if case == "b4_1080p":
        return _stack([TM._case(k, 1080, 1920, seed=20 + s) for s, k in enumerate(("noise", "smooth", "blur", "flat"))])
    if case == "flat_40x40":                                     # flat 0.9 + N(0, 1e-3): naive fp32 moments lose the variance
        return _stack([TM._case("flat", 40, 40, seed=4)])
    raise KeyError(case)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


def _hip(x, y, w, upstream=None):
    x = x.detach().clone().requires_grad_(True)
    loss = losses.quality_loss(x, y, l1=w[0], mse=w[1], ssim=w[2])
    assert loss.dtype == torch.float32 and loss.is_cuda and loss.dim() == 0
    (loss if upstream is None else loss * upstream).backward()
    assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    return loss.detach(), x.grad


def _float64_terms(x, y):
    """((L1, MSE, 1 - SSIM), their three gradients), float64 on the GPU."""
    xd, yd = x.double(), y.double()
    vals, grads = [], []
    for w in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)):
        v, g = R.autograd_grad(xd, yd, *w)
        vals.append(v.item())
        grads.append(g)
    return vals, grads


@pytest.mark.parametrize("case", ["b2_37x53", "103x257", "blur_96x300", "b4_1080p", "flat_40x40"])
def test_value_and_gradient(case):
    x, y = (t.to(DEV) for t in _inputs(case))
    (v_l1, v_mse, v_ssim), g64 = _float64_terms(x, y)
    for name, w in WEIGHTS.items():
        loss, grad = _hip(x, y, w)
        want = w[0] * v_l1 + w[1] * v_mse + w[2] * v_ssim
        bound = w[0] * L1_TOL + w[1] * MSE_RTOL * v_mse + w[2] * SSIM_TOL
        d_val = abs(loss.item() - want)
        ref = w[0] * g64[0] + w[1] * g64[1] + w[2] * g64[2]
        _, yard = R.autograd_grad(x, y, *w)                      # plain fp32 torch ops, on the GPU
        d_hip, d_yard = _rel(grad, ref), _rel(yard, ref)
        print(f"{case} {name}: loss {want:.8f} |d| {d_val:.2e} (bound {bound:.2e});  grad rel L2 HIP {d_hip:.2e}, fp32 torch ops {d_yard:.2e}")
        assert torch.isfinite(grad).all()
        assert d_val <= bound, (case, name, d_val, bound)
        assert d_hip <= max(2 * d_yard, GRAD_FLOOR), (case, name, d_hip, d_yard)


def test_upstream_scalar_is_read_from_device_memory():
    x, y = (t.to(DEV) for t in _inputs("b2_37x53"))
    for w in WEIGHTS.values():
        _, g1 = _hip(x, y, w)
        _, g3 = _hip(x, y, w, upstream=4.0)
        assert torch.equal(g3, g1 * 4.0)                         # a power of two scales every product exactly


def test_out_equal_to_target():
    xb, yb = (t.to(DEV) for t in _blur_pair())
    x = xb.clone()
    for name, w in WEIGHTS.items():
        loss, grad = _hip(x, x.clone(), w)
        _, gblur = _hip(xb, yb, w)
        scale, ref_scale = grad.abs().max().item() * x.numel(), gblur.abs().max().item() * xb.numel()
        print(f"out == target {name}: loss {loss.item():.3e}, max|grad| N {scale:.3e} (blurred pair: {ref_scale:.3e})")
        assert abs(loss.item()) <= w[2] * SSIM_TOL               # L1 and MSE are exactly 0
        assert scale <= 1e-3 * ref_scale, (name, scale, ref_scale)


def test_bits_repeatable_and_batch_independent():
    pairs = [TM._case(k, 300, 530, seed=10 + s) for s, k in enumerate(("noise", "smooth", "blur", "flat"))]
    x, y = (t.to(DEV) for t in _stack(pairs))
    for name, w in WEIGHTS.items():
        l4, g4 = _hip(x, y, w)
        l4b, g4b = _hip(x, y, w)
        assert torch.equal(l4, l4b) and torch.equal(g4, g4b), name
        for i in range(4):
            _, g1 = _hip(x[i:i + 1].contiguous(), y[i:i + 1].contiguous(), w)
            assert torch.equal(g1 * 0.25, g4[i:i + 1]), (name, i)
    for i in range(4):
        xi, yi = x[i:i + 1].contiguous(), y[i:i + 1].contiguous()
        l1, _ = _hip(xi, yi, WEIGHTS["ssim"])
        assert torch.equal(l1, (1.0 - metrics.ssim(xi, yi)[0]).float()), i


def test_errors():
    x = torch.rand(1, 3, 16, 16, device=DEV)
    with pytest.raises(ValueError):
        losses.quality_loss(torch.rand(1, 3, 6, 16, device=DEV), torch.rand(1, 3, 6, 16, device=DEV))
    with pytest.raises(ValueError):
        losses.quality_loss(x, torch.rand(1, 3, 16, 17, device=DEV))
    with pytest.raises(ValueError):
        losses.quality_loss(x, x.clone(), l1=0, mse=0, ssim=0)
    with pytest.raises(TypeError):
        losses.quality_loss(x, x.double())
    with pytest.raises(RuntimeError):
        losses.quality_loss(x.cpu(), x.cpu())
    with pytest.raises(ValueError):
        losses.quality_loss(x, torch.rand(1, 3, 16, 32, device=DEV)[..., ::2])          # non-contiguous
    x.requires_grad_(True)
    y = torch.rand(1, 3, 16, 16, device=DEV, requires_grad=True)
    losses.quality_loss(x, y, ssim=1.0).backward()               # the target gets no gradient
    assert x.grad is not None and y.grad is None


# ---- plumbing: the materialised gradient flows through the model nodes' plain-gradient paths ----
def _model(plugin, sd_fn, strict, **kw):
    m = importlib.import_module(f"models.{plugin}.model").TransformerModel(**kw)
    m.load_state_dict(sd_fn(0), strict=strict)
    return m.to(DEV).eval()          # eval: no dropout, the two runs see the same forward (parameters still require grad)


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def _check_plumbing(m, forward, hr, w):
    """quality_loss(forward(), hr).backward() leaves the .grad bits of forward().backward(gradient=G), G the loss's own gradient."""
    with ops.deterministic_mode():
        m.zero_grad(set_to_none=True)
        losses.quality_loss(forward(), hr, l1=w[0], mse=w[1], ssim=w[2]).backward()
        through_loss = _grads(m)
        m.zero_grad(set_to_none=True)
        out = forward()
        _, G = _hip(out.detach(), hr, w)
        out.backward(gradient=G)
        explicit = _grads(m)
    assert len(through_loss) > 10 and through_loss.keys() == explicit.keys()
    differing = [k for k in explicit if not torch.equal(through_loss[k], explicit[k])]
    assert not differing, differing[:8]
    assert all(torch.isfinite(v).all() for v in explicit.values())
    assert any(v.abs().max().item() > 0 for v in explicit.values())


@pytest.mark.parametrize("resize", [False, True])
def test_gradient_flows_into_fast_transformer(resize):
    m = _model("FastTransformer", deterministic_state_dict, False)
    g = torch.Generator().manual_seed(6)
    lr = torch.rand((2, 3, 68, 84), generator=g).to(DEV)
    hw = (102, 126) if resize else (136, 168)
    hr = torch.rand((2, 3) + hw, generator=g).to(DEV)

    def forward():
        out = m(lr, res_out=hw, require_ratio=False)
        if resize:
            assert tuple(out.shape[2:]) != hw          # the model leaves the Resize to the caller (harness.train_step)
            out = resize_aa(out, hw)
        assert tuple(out.shape[2:]) == hw
        return out
    _check_plumbing(m, forward, hr, WEIGHTS["mixed"])
    _check_plumbing(m, forward, hr, WEIGHTS["ssim"])


def test_gradient_flows_into_residual_transformer():
    m = _model("ResidualTransformer", rt_deterministic_state_dict, True)
    g = torch.Generator().manual_seed(7)
    lr = torch.rand((1, 3, 720, 1280), generator=g).to(DEV)          # the position embedding fixes the token grid
    hr = torch.rand((1, 3, 1440, 2560), generator=g).to(DEV)
    _check_plumbing(m, lambda: m(lr, upscale_factor=2), hr, WEIGHTS["mixed"])


def test_gradient_flows_into_window_transformer():
    m = _model("WindowTransformer", wt_deterministic_state_dict, False)
    g = torch.Generator().manual_seed(8)
    lr = torch.rand((2, 3, 88, 120), generator=g).to(DEV)
    hr = torch.rand((2, 3, 176, 240), generator=g).to(DEV)
    _check_plumbing(m, lambda: m(lr, upscale_factor=2), hr, WEIGHTS["mixed"])


# ---- the training step ----
def _three_steps(lr, hr, loss):
    torch.manual_seed(0)
    m = importlib.import_module("models.FastTransformer.model").TransformerModel()
    m.load_state_dict(deterministic_state_dict(0), strict=False)
    m = m.to(DEV).train()          # dropout active
    assert m.dropout_p > 0
    opt = harness.make_optimizer(m, 1e-4)
    with ops.deterministic_mode():
        out = [harness.train_step(m, opt, lr, hr, loss=loss).clone() for _ in range(3)]
    torch.cuda.synchronize()
    state = {"loss": torch.stack(out).cpu()}
    for k, p in m.named_parameters():
        state["param." + k] = p.detach().cpu().clone()
        st = opt.state.get(p, {})
        for s in ("exp_avg", "exp_avg_sq"):
            if s in st:
                state[f"{s}.{k}"] = st[s].detach().cpu().clone()
    return state


@pytest.mark.parametrize("lr_shape,hr_hw", [((2, 3, 68, 84), (136, 168)), ((2, 3, 68, 84), (102, 126))])
def test_quality_loss_training_step_is_bit_reproducible_and_descends(lr_shape, hr_hw):
    g = torch.Generator().manual_seed(2024)
    lr = torch.rand(lr_shape, generator=g).to(DEV)
    hr = torch.rand((lr_shape[0], 3) + hr_hw, generator=g).to(DEV)
    a = _three_steps(lr, hr, losses.QualityLoss(l1=0.5, ssim=0.5))
    b = _three_steps(lr, hr, losses.QualityLoss(l1=0.5, ssim=0.5))
    print("losses", a["loss"].tolist())
    assert torch.isfinite(a["loss"]).all()
    assert any(k.startswith("exp_avg.") for k in a) and any(k.startswith("exp_avg_sq.") for k in a)
    assert a.keys() == b.keys()
    differing = [k for k in a if not torch.equal(a[k], b[k])]
    assert not differing, (len(differing), differing[:8])
    assert a["loss"][2].item() < a["loss"][0].item()


# ---- the default path is the parent's ----
def _parent_train_step(model, optimizer, lr_batch, hr_batch):
    """harness.train_step as it was before it took `loss=`, line for line."""
    optimizer.zero_grad(set_to_none=True)
    out = model(lr_batch, res_out=tuple(hr_batch.shape[2:]), require_ratio=False)
    if tuple(out.shape[2:]) != tuple(hr_batch.shape[2:]):
        out = resize_aa(out, tuple(hr_batch.shape[2:]))
    loss = l1_loss(out, hr_batch, fuse_into_model_backward=True)
    loss.backward()
    optimizer.step()
    return loss.detach()


@pytest.mark.parametrize("hr_hw", [(128, 128), (96, 96)])
def test_default_step_launches_the_parents_call_sequence(monkeypatch, hr_hw):
    calls = []
    real_call = _lib.call

    def spy_call(name, *args):
        calls.append((name, tuple(a for a in args if isinstance(a, float) or (isinstance(a, int) and abs(a) < 1 << 24))))
        return real_call(name, *args)
    monkeypatch.setattr(_lib, "call", spy_call)
    g = torch.Generator().manual_seed(5)
    lr, hr = torch.rand((1, 3, 64, 64), generator=g).to(DEV), torch.rand((1, 3) + hr_hw, generator=g).to(DEV)
    runs = {}
    for which, step in (("parent", _parent_train_step), ("positional", harness.train_step),
                        ("loss=None", lambda *a: harness.train_step(*a, loss=None))):
        torch.manual_seed(0)
        m = importlib.import_module("models.FastTransformer.model").TransformerModel()
        m.load_state_dict(deterministic_state_dict(0), strict=False)
        m = m.to(DEV).train()
        opt = harness.make_optimizer(m, 1e-4)
        del calls[:]
        value = step(m, opt, lr, hr)
        torch.cuda.synchronize()
        runs[which] = (list(calls), value.clone())
    names = [n for n, _ in runs["parent"][0]]
    assert "tup_l1_loss_partial" in names and "tup_l1_loss_bwd" not in names          # the fused-L1 hand-off, as before
    assert not [n for n in names if n.startswith("tup_quality")]
    for which in ("positional", "loss=None"):
        assert runs[which][0] == runs["parent"][0], which
    # and a QualityLoss step takes the materialised-gradient route instead
    del calls[:]
    harness.train_step(m, opt, lr, hr, loss=losses.QualityLoss(l1=0.5, ssim=0.5))
    names = [n for n, _ in calls]
    assert names.count("tup_quality_loss_f32_bwd") == 1 and names.count("tup_quality_loss_reduce") == 1
    assert "tup_l1_loss_bwd" not in names
