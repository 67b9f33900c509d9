"""CPU checks of the quality-loss feature: the float64 restatement the GPU tests compare against (tests/_quality_loss_ref.py)
agrees with the scorer's restatement (tests/_metrics_ref.py) and with the closed-form gradient csrc/quality_loss.hip implements;
the new C-ABI entries are exported and bound; the public interface rejects what it cannot run."""
import inspect
import os
import re

import pytest
import torch

import _metrics_ref as M          # tests/ is on sys.path (rootdir-less test modules)
import _quality_loss_ref as R
from _abi import ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _pair(B, H, W, seed, noise=0.05):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, H, W, generator=g, dtype=F64)
    y = (x + noise * torch.randn(B, 3, H, W, generator=g, dtype=F64)).clamp(0, 1)
    return x, y


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("B,H,W", [(1, 7, 7), (2, 13, 29), (3, 40, 33)])
def test_restated_ssim_equals_the_scorers_restatement(B, H, W):
    x, y = _pair(B, H, W, seed=H)
    got = R.ssim(x, y, 1.0)
    for i in range(B):
        want = M.ssim(x[i].permute(1, 2, 0).numpy(), y[i].permute(1, 2, 0).numpy(), 1.0)
        assert abs(got[i].item() - want) <= 1e-12
    l1, mse, dssim = R.terms(x, y)
    assert abs(mse.item() - sum(M.mse(x[i].numpy(), y[i].numpy()) for i in range(B)) / B) <= 1e-15
    assert abs(l1.item() - (x - y).abs().mean().item()) <= 1e-15
    assert abs(dssim.item() - (1 - got.mean().item())) <= 1e-15
    assert R.quality_loss(x, y, 0.5, 0.2, 0.3).item() == pytest.approx(0.5 * l1.item() + 0.2 * mse.item() + 0.3 * dssim.item(), abs=1e-15)


@pytest.mark.parametrize("B,H,W,noise", [(1, 7, 7, 0.05), (2, 13, 29, 0.05), (2, 40, 33, 0.2), (1, 20, 31, 1e-3)])
def test_autograd_of_the_restatement_equals_the_closed_form(B, H, W, noise):
    x, y = _pair(B, H, W, seed=W, noise=noise)
    _, auto = R.autograd_grad(x, y, l1=0.0, mse=0.0, ssim=1.0)
    assert _rel(R.closed_form_ssim_grad(x, y), auto) <= 1e-12
    # the kernel's factoring around a shift is the same function, for any shift
    assert _rel(R.kernel_form_ssim_grad(x, y), auto) <= 1e-12
    assert _rel(R.kernel_form_ssim_grad(x, y, kx=torch.tensor(0.3, dtype=F64), ky=torch.tensor(0.7, dtype=F64)), auto) <= 1e-12


def test_flat_bright_pair_keeps_its_gradient_in_the_kernel_form_at_fp32():
    """What the shift is for: evaluated in fp32 on a flat bright pair, the kernel's form is closer to float64 (of the same fp32
    inputs) than the plain composition, whose E[x^2] - E[x]^2 of unshifted data cancels."""
    g = torch.Generator().manual_seed(4)
    y = torch.full((1, 3, 40, 40), 0.9)
    x = y + 1e-3 * torch.randn(1, 3, 40, 40, generator=g)
    _, auto = R.autograd_grad(x.double(), y.double(), l1=0.0, mse=0.0, ssim=1.0)
    shifted = _rel(R.kernel_form_ssim_grad(x, y).double(), auto)
    _, plain = R.autograd_grad(x, y, l1=0.0, mse=0.0, ssim=1.0)
    plain = _rel(plain.double(), auto)
    print(f"flat bright fp32: kernel form {shifted:.2e}, plain composition {plain:.2e}")
    assert shifted < plain


def test_pointwise_terms_of_the_restatement():
    x, y = _pair(2, 9, 11, seed=1)
    N = x.numel()
    _, g = R.autograd_grad(x, y, l1=0.5, mse=0.25, ssim=0.0)
    assert torch.allclose(g, 0.5 * torch.sign(x - y) / N + 0.25 * 2 * (x - y) / N, rtol=0, atol=1e-18)


def test_entries_in_header_signatures_and_library():
    from transformerupscaler_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tupscale_hip.h")).read()
    expected = {"tup_quality_loss_reduce": 12, "tup_quality_loss_f32_bwd": 12}
    lib = _lib.load()
    for name, nargs in expected.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert len(_lib.SIGNATURES[name]) == nargs, name
        assert hasattr(lib, name), name
    assert _lib.ABI_VERSION == ABI and lib.tup_abi_version() == ABI


def test_new_kernel_is_on_the_no_scratch_guard_list():
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_resources", os.path.join(ROOT, "transformerupscaler_amd", "csrc", "check_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert ("quality_loss.hip", ["quality_loss_bwd_kernel"]) in mod.GUARDED


def test_public_interface_rejects_what_it_cannot_run():
    from transformerupscaler_amd import harness, losses
    x = torch.rand(1, 3, 8, 8)
    with pytest.raises(RuntimeError):
        losses.quality_loss(x, x.clone())                                  # no CPU path
    with pytest.raises(RuntimeError):
        losses.QualityLoss(ssim=1.0, l1=0.0)(x, x.clone())
    with pytest.raises(ValueError):
        losses.quality_loss(x, x.clone(), l1=0.0, mse=0.0, ssim=0.0)
    with pytest.raises(ValueError):
        losses.QualityLoss(l1=0.0)
    with pytest.raises(ValueError):
        losses.quality_loss(torch.rand(1, 3, 6, 8), torch.rand(1, 3, 6, 8), ssim=1.0)
    with pytest.raises(ValueError):
        losses.quality_loss(x, torch.rand(1, 3, 8, 9))
    with pytest.raises(ValueError):
        losses.quality_loss(torch.rand(1, 1, 8, 8), torch.rand(1, 1, 8, 8))
    with pytest.raises(TypeError):
        losses.quality_loss(x.double(), x.double())
    sig = inspect.signature(losses.quality_loss)
    assert [(p, sig.parameters[p].default) for p in ("l1", "mse", "ssim", "data_range")] == [("l1", 1.0), ("mse", 0.0), ("ssim", 0.0), ("data_range", 1.0)]
    step = inspect.signature(harness.train_step)
    assert list(step.parameters)[-1] == "loss" and step.parameters["loss"].default is None
