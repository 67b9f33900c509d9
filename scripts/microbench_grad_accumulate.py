"""Timing of the mixed-scale training step: five alternating runs after warm-up, device-synchronised, median [range].

  1. the per-sample loop that existed before (one backward per sample, torch accumulating into p.grad, then the optimizer step)
     against harness.train_step_samples with group=True and with group=False, FastTransformer, on two batches:
       (a) the dataset's first six scale pairs at their real sizes, 720p -> 1080p through 1440p -> 4K (`--no-large` skips it);
       (b) six 96 x 96 samples of pairs 6-9 (x2, x3, x4, x6, x2, x3);
  2. the accumulate call alone on a FastTransformer x2 gradient set (mode 1: 12 B per element; 54 MB, so the call is bound by its
     host path and launch, not by the kernel), against the same accumulation as one aten add_ per parameter;
  3. the kernel at a size where it is the whole time (4 segments of 16 M floats, mode 1, 805 MB), as GB/s, beside torch's add_.

Needs a GPU."""
import os, sys; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import importlib, statistics, torch
from transformerupscaler_amd import harness
from transformerupscaler_amd.accumulate import GradAccumulator
from transformerupscaler_amd.autograd import l1_loss, resize_aa
from transformerupscaler_amd.data import SCALE_PAIRS
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


def show(label, v, extra="", unit="us"):
    print(f"{label}: median {statistics.median(v):.1f} {unit} [{min(v):.1f}-{max(v):.1f}]{extra}", flush=True)


def model_and_optimizer():
    torch.manual_seed(0)
    m = importlib.import_module("models.FastTransformer.model").TransformerModel()
    m.load_state_dict(deterministic_state_dict(0), strict=False)
    m = m.to(dev).train()
    return m, harness.make_optimizer(m, 1e-4)


def per_sample_loop(m, opt, lrs, hrs):
    opt.zero_grad(set_to_none=True)
    for lr, hr in zip(lrs, hrs):
        hw = tuple(hr.shape[2:])
        out = resize_aa(m(lr, res_out=hw, require_ratio=False), hw)
        (l1_loss(out, hr, fuse_into_model_backward=True) * (1 / len(lrs))).backward()
    opt.step()


def samples(pairs, seed):
    g = torch.Generator().manual_seed(seed)
    lrs = [torch.rand((1, 3) + tuple(p["lr"]), generator=g).to(dev) for p in pairs]
    hrs = [torch.rand((1, 3) + tuple(p["hr"]), generator=g).to(dev) for p in pairs]
    return lrs, hrs


def step_arms(lrs, hrs):
    arms = {}
    m, opt = model_and_optimizer()
    arms["per-sample backward loop (torch accumulates)"] = lambda m=m, opt=opt: per_sample_loop(m, opt, lrs, hrs)
    for label, group in (("train_step_samples(group=True)", True), ("train_step_samples(group=False)", False)):
        m, opt = model_and_optimizer()
        arms[label] = lambda m=m, opt=opt, group=group: harness.train_step_samples(m, opt, lrs, hrs, group=group)
    return arms


batches = [("(b) six 96x96 samples of pairs 6-9", [SCALE_PAIRS[i] for i in (6, 7, 8, 9, 6, 7)], 10)]
if "--no-large" not in sys.argv:
    batches.append(("(a) pairs 0-5 at their real sizes", SCALE_PAIRS[:6], 1))
for title, pairs, n in batches:
    lrs, hrs = samples(pairs, 1)
    res = alternate(step_arms(lrs, hrs), n=n)
    for label, v in res.items():
        show(f"{title}, {label}", [t / 1000 for t in v], unit="ms")
    del lrs, hrs, res
    torch.cuda.empty_cache()

# ---- the accumulate launch alone ----
m, _ = model_and_optimizer()
acc = GradAccumulator(m)
names = [n for n in active_param_names(2) if n in acc.params]
g = torch.Generator(device=dev).manual_seed(2)
grads = {n: torch.randn(acc.params[n].shape, generator=g, device=dev) for n in names}
elements = sum(v.numel() for v in grads.values())
acc.begin()
acc.add(grads)                                       # first touch: mode 0
res = alternate({"add": lambda: acc.add(grads)}, n=50)          # later touches: mode 1
med = statistics.median(res["add"])
show(f"tup_grad_accumulate, mode 1, {len(names)} segments, {elements / 1e6:.2f} M floats (+ its pointer-table upload)", res["add"],
     f"  = {12 * elements / (med * 1e-6) / 1e9:.0f} GB/s at 12 B per element")
torch_arm = {n: torch.zeros_like(v) for n, v in grads.items()}


def torch_add():
    for n, v in grads.items():
        torch_arm[n].add_(v)


res = alternate({"torch": torch_add}, n=50)
show(f"the same accumulation as {len(names)} aten add_ launches", res["torch"])
acc.finish()

# ---- the kernel where it is the whole time ----
from transformerupscaler_amd.accumulate import SegmentLauncher
launcher = SegmentLauncher(torch.device(dev, torch.cuda.current_device()))
N = 16 << 20
dst = [torch.zeros((N,), device=dev) for _ in range(4)]
src = [torch.randn((N,), generator=g, device=dev) for _ in range(4)]
segs = [(d.data_ptr(), s.data_ptr(), N, 1.0, 1) for d, s in zip(dst, src)]


def aten_big():
    for d, s in zip(dst, src):
        d.add_(s)


res = alternate({"hip": lambda: launcher.launch(segs), "aten": aten_big}, n=20)
for k, label in (("hip", "tup_grad_accumulate, mode 1, 4 x 16 M floats"), ("aten", "the same as 4 aten add_ launches")):
    med = statistics.median(res[k])
    show(label, res[k], f"  = {12 * 4 * N / (med * 1e-6) / 1e12:.2f} TB/s at 12 B per element")
