"""Timing of losses.quality_loss (csrc/quality_loss.hip) at 4 x 3 x 1080 x 1920: five alternating runs, median [range].

  1. loss forward + backward: the HIP loss against the same loss composed of fp32 torch ops and differentiated by autograd (what a
     user could write without it), for the SSIM-only and the L1 + SSIM weights;
  2. the backward kernel alone and its achieved GB/s against the three-plane minimum (read x, read y, write grad = 0.30 GB);
  3. the FastTransformer x2 720p batch-4 training step: default L1 step against the QualityLoss(l1=0.5, ssim=0.5) step.

Needs a GPU; `--no-step` skips part 3."""
import os, sys; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import importlib, statistics, torch
import _quality_loss_ref as R
from transformerupscaler_amd import _lib, harness, losses, ops
from transformerupscaler_amd.weights import deterministic_state_dict

assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = "cuda"
g = torch.Generator(device=dev).manual_seed(0)
B, H, W = 4, 1080, 1920
y = torch.rand((B, 3, H, W), generator=g, device=dev)
x = (y + 0.05 * torch.randn((B, 3, H, W), generator=g, device=dev)).clamp(0, 1).requires_grad_(True)
MIN_GB = 3 * x.numel() * 4 / 1e9


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1000          # us per call


def alternate(arms, n, rounds=5):
    res = {k: [] for k in arms}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in arms.items():
            res[k].append(timed(fn, n))
    return res


def show(label, v, extra="", unit="us"):
    print(f"{label}: median {statistics.median(v):.1f} {unit} [{min(v):.1f}-{max(v):.1f}]{extra}")


def fwd_bwd(loss_fn):
    def run():
        x.grad = None
        loss_fn().backward()
    return run


for name, w in (("ssim only", (0.0, 0.0, 1.0)), ("l1 0.5 + ssim 0.5", (0.5, 0.0, 0.5))):
    res = alternate({"hip": fwd_bwd(lambda: losses.quality_loss(x, y, *w)), "torch": fwd_bwd(lambda: R.quality_loss(x, y, *w))}, n=10)
    show(f"loss forward + backward, {name}, HIP", res["hip"])
    show(f"loss forward + backward, {name}, fp32 torch ops", res["torch"])

one = torch.ones(1, device=dev)
grad = torch.empty_like(x)
xd = x.detach()


def bwd_only():
    _lib.call("tup_quality_loss_f32_bwd", xd.data_ptr(), y.data_ptr(), one.data_ptr(), grad.data_ptr(), B, H, W, 0.5, 0.0, 0.5, 1.0,
              torch.cuda.current_stream().cuda_stream)


def fwd_only():
    with torch.no_grad():
        losses.quality_loss(xd, y, 0.5, 0.0, 0.5)


res = alternate({"bwd": bwd_only, "fwd": fwd_only}, n=20)
med = statistics.median(res["bwd"])
show("backward kernel alone (l1 0.5 + ssim 0.5)", res["bwd"], f"  = {MIN_GB / (med * 1e-6):.0f} GB/s of the {MIN_GB:.2f} GB three-plane minimum")
show("forward alone (quality partials + l1 partials + reduce)", res["fwd"])

if "--no-step" not in sys.argv:
    g2 = torch.Generator().manual_seed(1)
    lr = torch.rand((4, 3, 720, 1280), generator=g2).to(dev)
    hr = torch.rand((4, 3, 1440, 2560), generator=g2).to(dev)
    arms = {}
    for label, loss in (("default L1 step", None), ("QualityLoss(l1=0.5, ssim=0.5) step", losses.QualityLoss(l1=0.5, ssim=0.5))):
        torch.manual_seed(0)
        m = importlib.import_module("models.FastTransformer.model").TransformerModel()
        m.load_state_dict(deterministic_state_dict(0), strict=False)
        m = m.to(dev).train()
        opt = harness.make_optimizer(m, 1e-4)
        arms[label] = lambda m=m, opt=opt, loss=loss: harness.train_step(m, opt, lr, hr, loss=loss)
    res = alternate(arms, n=5)
    for label, v in res.items():
        show(f"FastTransformer x2 720p batch 4, {label}", [t / 1000 for t in v], unit="ms")
