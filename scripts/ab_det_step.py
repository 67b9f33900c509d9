"""Training-step time in the default mode (ops.deterministic = False: atomic forms), in the default mode with branch A on the
explicit stage convs (FastTransformer only: what that route-around of deterministic mode costs without the slab forms; the
second route-around, patch_unembed.bias from one more column-sum pass, is NOT in this arm, so the split it gives is incomplete) and in
deterministic mode (True): FastTransformer 2x 720p -> 1080p, batch 4 (config 3) and ResidualTransformer 6x 720p, batch 2
(config 5).  Five alternating runs of 10 steps per arm after warm-up; median [range] in ms per step.  Run the same
script from a checkout of an older commit for that commit's two arms (there True meant the convs only)."""
import importlib
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from transformerupscaler_amd import fast_transformer, harness, ops  # noqa: E402
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


ARMS = {"default": (False, True), "default, explicit branch A": (False, False), "deterministic": (True, True)}


def set_arm(arm):
    ops.deterministic, fast_transformer.compose_branch_a_in_training = ARMS[arm]


for name, make, arms in (("FastTransformer x2 B=4", ft_case, list(ARMS)), ("ResidualTransformer x6 B=2", rt_case, ["default", "deterministic"])):
    step = make()
    res = {arm: [] for arm in arms}
    for arm in arms:
        set_arm(arm)
        for _ in range(2):
            step()
    for _ in range(RUNS):
        for arm in arms:
            set_arm(arm)
            res[arm].append(timed(step))
    set_arm("default")
    print(f"{name}: " + ", ".join(f"{arm} {statistics.median(v):.2f} ms [{min(v):.2f}-{max(v):.2f}]" for arm, v in res.items()), flush=True)
    del step
    torch.cuda.empty_cache()
