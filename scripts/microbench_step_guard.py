"""Timing of the guarded optimizer step: five alternating runs after warm-up, device-synchronised, median [range].

Three arms on the same parameters and gradients, an optimizer step alone (the gradients are given, nothing is reduced):
  1. `optim.Adam.step()` with every option off: ONE `tup_adam_step` launch (what existed);
  2. the guarded step, `optim.Adam(max_grad_norm=..., skip_nonfinite=True)`: norm, finish and guarded-step launches, the guard
     record's asynchronous read-back, and the next step's wait for it;
  3. stock torch: `clip_grad_norm_` + a finite check of the norm with `.item()` + `torch.optim.Adam.step()`
     (`harness.make_optimizer` under `harness.use_torch_adam`, the A/B arm).
On two gradient sets: the parameters a FastTransformer x2 step touches (97 segments, 4.49 M floats) and all parameters of the model
(every scale's upsampler: the full set).  `max_grad_norm` is half the gradient norm, so every step clips.

Needs a GPU."""
import os, sys; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import importlib, statistics, torch
from transformerupscaler_amd import harness
from transformerupscaler_amd.weights import active_param_names, deterministic_state_dict

assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = "cuda"


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1000          # us per call


def alternate(arms, n, rounds=5, warmup=2):
    res = {k: [] for k in arms}
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in arms.items():
            res[k].append(timed(fn, n))
    return res


def show(label, v, extra=""):
    print(f"{label}: median {statistics.median(v):.1f} us [{min(v):.1f}-{max(v):.1f}]{extra}", flush=True)


def arm(names, grads, torch_arm, **options):
    """A model of its own per arm (every arm moves its weights), the same gradients for all."""
    m = importlib.import_module("models.FastTransformer.model").TransformerModel()
    m.load_state_dict(deterministic_state_dict(0), strict=False)
    m = m.to(dev)
    harness.use_torch_adam = torch_arm
    try:
        opt = harness.make_optimizer(m, 1e-6, **options)
    finally:
        harness.use_torch_adam = False
    params = dict(m.named_parameters())
    own = {n: grads[n].clone() for n in names}          # the torch arm scales its gradients in place (the launches do not depend on the values)

    def step():
        for n in names:
            params[n].grad = own[n]
        opt.step()
    return step


probe = importlib.import_module("models.FastTransformer.model").TransformerModel()
shapes = {n: tuple(p.shape) for n, p in probe.named_parameters() if p.requires_grad}
sets = [("FastTransformer x2 gradient set", [n for n in active_param_names(2) if n in shapes]), ("all parameters", list(shapes))]
for title, names in sets:
    g = torch.Generator(device=dev).manual_seed(4)
    grads = {n: torch.randn(shapes[n], generator=g, device=dev) * 1e-3 for n in names}
    elements = sum(v.numel() for v in grads.values())
    norm = float(torch.sqrt(sum((v.double() ** 2).sum() for v in grads.values())))
    guard = dict(max_grad_norm=norm / 2, skip_nonfinite=True)
    arms = {
        "optimizer.step(), options off: one tup_adam_step": arm(names, grads, False),
        "guarded step: norm + finish + tup_adam_step_guarded": arm(names, grads, False, **guard),
        "torch: clip_grad_norm_ arithmetic + .item() finite check + torch.optim.Adam": arm(names, grads, True, **guard),
        "torch.optim.Adam alone (no guard)": arm(names, grads, True),
    }
    res = alternate(arms, n=50)
    print(f"-- {title}: {len(names)} segments, {elements / 1e6:.2f} M floats ({4 * elements / 1e6:.1f} MB of gradients)", flush=True)
    for label, v in res.items():
        show(label, v)
    keys = list(res)
    added = [b - a for a, b in zip(res[keys[0]], res[keys[1]])]
    show("the guard's added time per step (guarded - options off, per round)", added)
