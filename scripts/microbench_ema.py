"""Timing of the weight average inside the optimizer step: the protocol of scripts/microbench_step_guard.py -- five
alternating rounds of 50 steps after warm-up, device-synchronised, median [range] -- on its two gradient sets.

Three arms, each unguarded and guarded (`max_grad_norm` = half the gradient norm + `skip_nonfinite`), an optimizer step alone:
  1. the step without the average: `tup_adam_step` / norm + finish + `tup_adam_step_guarded`;
  2. the fused step, `ema_decay=0.999`: `tup_adam_step_ema` in the step launch's place (36 B per element against 28);
  3. the step without the average followed by `torch._foreach_lerp_(buffers, params, 1 - decay)` over the same buffers: what a user
     writes today (12 B per element more, in torch's multi-tensor launches; it cannot see a skipped step).
`--only NAME` runs one arm alone, 200 steps, for a kernel trace (`rocprofv3 --kernel-trace --stats -- python scripts/microbench_ema.py
--only fused`).

Needs a GPU."""
import os, sys; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse, importlib, statistics, torch
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


def show(label, v):
    print(f"{label}: median {statistics.median(v):.1f} us [{min(v):.1f}-{max(v):.1f}]", flush=True)


def arm(names, grads, kind, **options):
    """A model of its own per arm (every arm moves its weights), the same gradients for all.  kind: "off", "fused" or "lerp"."""
    m = importlib.import_module("models.FastTransformer.model").TransformerModel()
    m.load_state_dict(deterministic_state_dict(0), strict=False)
    m = m.to(dev)
    opt = harness.make_ema_optimizer(m, 0.999, lr=1e-6, **options) if kind == "fused" else harness.make_optimizer(m, 1e-6, **options)
    params = dict(m.named_parameters())
    stepped = [params[n] for n in names]
    buffers = [p.detach().clone() for p in stepped] if kind == "lerp" else None

    def step():
        for n in names:
            params[n].grad = grads[n]
        opt.step()
        if buffers is not None:
            torch._foreach_lerp_(buffers, [p.detach() for p in stepped], 1.0 - 0.999)
    return step


ap = argparse.ArgumentParser()
ap.add_argument("--only", choices=("off", "fused", "lerp"), default=None, help="run this arm alone (unguarded, all parameters, 200 steps)")
args = ap.parse_args()
probe = importlib.import_module("models.FastTransformer.model").TransformerModel()
shapes = {n: tuple(p.shape) for n, p in probe.named_parameters() if p.requires_grad}
sets = [("FastTransformer x2 gradient set", [n for n in active_param_names(2) if n in shapes]), ("all parameters", list(shapes))]
if args.only:
    sets = sets[1:]
for title, names in sets:
    g = torch.Generator(device=dev).manual_seed(4)
    grads = {n: torch.randn(shapes[n], generator=g, device=dev) * 1e-3 for n in names}
    elements = sum(v.numel() for v in grads.values())
    if args.only:
        fn = arm(names, grads, args.only)
        us = timed(fn, 200)
        print(f"{args.only}, {title}: {len(names)} segments, {elements / 1e6:.2f} M floats, {us:.1f} us per step over 200 steps", flush=True)
        break
    norm = float(torch.sqrt(sum((v.double() ** 2).sum() for v in grads.values())))
    guard = dict(max_grad_norm=norm / 2, skip_nonfinite=True)
    arms = {
        "step without the average: one tup_adam_step": arm(names, grads, "off"),
        "fused: one tup_adam_step_ema": arm(names, grads, "fused"),
        "step without the average + torch._foreach_lerp_": arm(names, grads, "lerp"),
        "guarded step without the average: norm + finish + tup_adam_step_guarded": arm(names, grads, "off", **guard),
        "guarded fused: norm + finish + tup_adam_step_ema": arm(names, grads, "fused", **guard),
        "guarded step without the average + torch._foreach_lerp_": arm(names, grads, "lerp", **guard),
    }
    res = alternate(arms, n=50)
    print(f"-- {title}: {len(names)} segments, {elements / 1e6:.2f} M floats ({4 * elements / 1e6:.1f} MB of gradients)", flush=True)
    for label, v in res.items():
        show(label, v)
    keys = list(res)
    for base, fused, lerp in ((0, 1, 2), (3, 4, 5)):
        show(f"added by the fused average ({'guarded' if base else 'unguarded'}, per round)", [b - a for a, b in zip(res[keys[base]], res[keys[fused]])])
        show(f"added by torch._foreach_lerp_ ({'guarded' if base else 'unguarded'}, per round)", [b - a for a, b in zip(res[keys[base]], res[keys[lerp]])])
