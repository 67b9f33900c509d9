"""Training-step time with the weight-gradient convs in their atomic forms (ops.deterministic = False) and in their deterministic
forms (True): FastTransformer 2x 720p -> 1080p, batch 4 (config 3) and ResidualTransformer 6x 720p, batch 2 (config 5).
Five alternating runs of 10 steps per arm after warm-up; median [range] in ms per step."""
import importlib
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from transformerupscaler_amd import harness, ops  # noqa: E402
from transformerupscaler_amd.autograd import l1_loss  # noqa: E402
from transformerupscaler_amd.weights import deterministic_state_dict, rt_deterministic_state_dict  # noqa: E402

RUNS, STEPS = 5, 10


def ft_case():
    m = importlib.import_module("models.FastTransformer.model").TransformerModel()
    m.load_state_dict(deterministic_state_dict(0), strict=False)
    m = m.cuda().train()
    opt = harness.make_optimizer(m, 1e-4)
    g = torch.Generator().manual_seed(4321)
    lr = torch.rand((4, 3, 720, 1280), generator=g).cuda()
    hr = torch.rand((4, 3, 1080, 1920), generator=g).cuda()
    return lambda: harness.train_step(m, opt, lr, hr)


def rt_case():
    m = importlib.import_module("models.ResidualTransformer.model").TransformerModel()
    m.load_state_dict(rt_deterministic_state_dict(0))
    m = m.cuda().train()
    opt = harness.make_optimizer(m, 1e-4)
    g = torch.Generator().manual_seed(9876)
    lr = torch.rand((2, 3, 720, 1280), generator=g).cuda()
    hr = torch.rand((2, 3, 4320, 7680), generator=g).cuda()

    def step():
        opt.zero_grad(set_to_none=True)
        loss = l1_loss(m(lr, upscale_factor=6), hr, fuse_into_model_backward=True)
        loss.backward()
        opt.step()
    return step


def timed(step):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / STEPS * 1e3


for name, make in (("FastTransformer x2 B=4", ft_case), ("ResidualTransformer x6 B=2", rt_case)):
    step = make()
    res = {False: [], True: []}
    for arm in (False, True):
        ops.deterministic = arm
        for _ in range(2):
            step()
    for _ in range(RUNS):
        for arm in (False, True):
            ops.deterministic = arm
            res[arm].append(timed(step))
    ops.deterministic = False
    print(f"{name}: atomic {statistics.median(res[False]):.2f} ms [{min(res[False]):.2f}-{max(res[False]):.2f}], "
          f"deterministic convs {statistics.median(res[True]):.2f} ms [{min(res[True]):.2f}-{max(res[True]):.2f}]", flush=True)
    del step
    torch.cuda.empty_cache()
