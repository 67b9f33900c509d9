"""The mixed-scale training step on the MI355X: `harness.train_step_samples` + `accumulate.GradAccumulator` against the path that
existed before them (one `backward()` per sample, torch accumulating into ``p.grad``), against the real reference's gradients
(tests/golden/train_mixed_step.npz), under two data-parallel ranks, and through the `train.py` driver."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_hip_parity_r2 as T_r2
from transformerupscaler_amd import harness, ops
from transformerupscaler_amd.accumulate import GradAccumulator
from transformerupscaler_amd.autograd import l1_loss, resize_aa
from transformerupscaler_amd.weights import deterministic_state_dict, rt_deterministic_state_dict, wt_deterministic_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    ops.deterministic = False
    ops.release_det_slabs()


def fixture_samples(golden_dir):
    d = dict(np.load(os.path.join(golden_dir, "train_mixed_step.npz"), allow_pickle=False))
    n = len(d["scales"])
    lrs, hrs = ([torch.from_numpy(d[f"{k}_u8_{i}"]).float().div(255.0).unsqueeze(0).to(DEV) for i in range(n)] for k in ("lr", "hr"))
    return d, lrs, hrs


def ft_model():
    m = importlib.import_module("models.FastTransformer.model").TransformerModel()
    m.load_state_dict(deterministic_state_dict(0), strict=False)
    return m.to(DEV).eval()


def rt_small_model():
    """ResidualTransformer on a 4 x 6 token grid (64 x 96 input)."""
    sd = rt_deterministic_state_dict(0)
    sd["pos_embed"] = sd["pos_embed"][:, :24].clone()
    m = importlib.import_module("models.ResidualTransformer.model").TransformerModel()
    m.pos_embed = torch.nn.Parameter(torch.empty(1, 24, 128))
    m.num_tokens = 24
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def wt_model():
    m = importlib.import_module("models.WindowTransformer.model").TransformerModel()
    m.load_state_dict(wt_deterministic_state_dict(0), strict=False)
    return m.to(DEV).eval()


def parent_step(model, optimizer, lr_list, hr_list):
    """The step as it could be written before train_step_samples: per sample, in list order,
    ``(l1_loss(resize_aa(model(...)), hr) * (1 / B)).backward()`` with torch accumulating into p.grad, then optimizer.step()."""
    optimizer.zero_grad(set_to_none=True)
    B = len(lr_list)
    total = torch.zeros((), device=DEV)
    for lr, hr in zip(lr_list, hr_list):
        hw = tuple(hr.shape[2:])
        out = resize_aa(model(lr, res_out=hw, require_ratio=False), hw)
        value = l1_loss(out, hr, fuse_into_model_backward=True) * (1 / B)
        value.backward()
        total = total + value.detach()
    optimizer.step()
    return total


def snapshot(model, optimizer, loss):
    torch.cuda.synchronize()
    state = {"loss": loss.detach().cpu().clone()}
    for k, p in model.named_parameters():
        state["param." + k] = p.detach().cpu().clone()
        if p.grad is not None:
            state["grad." + k] = p.grad.detach().cpu().clone()
        for s in ("exp_avg", "exp_avg_sq"):
            if s in optimizer.state.get(p, {}):
                state[f"{s}.{k}"] = optimizer.state[p][s].detach().cpu().clone()
    return state


def rand_samples(pairs, seed):
    g = torch.Generator().manual_seed(seed)
    lrs = [torch.rand((1, 3) + lr, generator=g).to(DEV) for lr, _ in pairs]
    hrs = [torch.rand((1, 3) + hr, generator=g).to(DEV) for _, hr in pairs]
    return lrs, hrs


SMALL = {
    "rt": (rt_small_model, [((64, 96), (128, 192)), ((64, 96), (96, 144)), ((64, 96), (128, 192))]),
    "wt": (wt_model, [((88, 120), (176, 240)), ((32, 48), (96, 144)), ((88, 120), (176, 240))]),
}


# ---- 2. bit-equality with the pre-existing path ----
@pytest.mark.parametrize("case", ["ft", "rt", "wt"])
def test_ungrouped_step_is_bit_equal_to_the_per_sample_backward_loop(case, golden_dir):
    """Under ops.deterministic_mode(): two steps of train_step_samples(group=False) and two of `parent_step` on the same list --
    loss, gradients, updated parameters and Adam's moments torch.equal after each step."""
    if case == "ft":
        build = ft_model
        _, lrs, hrs = fixture_samples(golden_dir)
    else:
        build, pairs = SMALL[case]
        lrs, hrs = rand_samples(pairs, 31)
    states = {}
    for path in ("parent", "new"):
        torch.manual_seed(0)
        m = build()
        opt = harness.make_optimizer(m, 1e-4)
        snaps = []
        with ops.deterministic_mode():
            for _ in range(2):
                if path == "parent":
                    loss = parent_step(m, opt, lrs, hrs)
                else:
                    loss = harness.train_step_samples(m, opt, lrs, hrs, group=False)
                snaps.append(snapshot(m, opt, loss))
        states[path] = snaps
        del m, opt
    for step, (a, b) in enumerate(zip(states["parent"], states["new"])):
        assert torch.isfinite(a["loss"]).all()
        assert a.keys() == b.keys(), (step, sorted(set(a) ^ set(b))[:6])
        assert any(k.startswith("grad.") for k in a) and any(k.startswith("exp_avg_sq.") for k in a)
        differing = [k for k in a if not torch.equal(a[k], b[k])]
        assert not differing, (case, step, len(differing), differing[:8])


# ---- 3. grouped against ungrouped, and against the reference ----
def test_grouped_step_matches_ungrouped_and_the_reference(golden_dir):
    """The fixture's six samples (scales 2, 2, 3, 3, 6, 4; the two first equal-shaped; the fourth through the Resize).
      * grouped (5 backwards, one of B = 2) against ungrouped (6 backwards): per-parameter relative L2 <= 2e-2, the bound of
        test_hip_parity_r2.test_per_sample_loop_matches_reference_and_batched for batched-versus-loop;
      * both, and the pre-existing per-sample backward loop, against the real reference's fp32 step: loss within 2e-3, gradients
        within test_hip_parity_r2.GRAD_LIMITS.

    Measured on an MI355X (bf16 path against the fp32 reference; worst sampled error / norm error / full relative L2 per family;
    the pre-existing loop, the ungrouped and the grouped step gave the same figures to the digits shown):
        loss 0.207425 against 0.207431 (|diff| 5.6e-6)
        blocks          0.0452 / 0.0075 / 0.0294   (limits 0.08 / 0.02 / 0.08)
        cnn_bias+conv1  0.0313 / 0.0092 / 0.0252   (limits 0.11 / 0.03 / 0.11)
        cnn_weights     0.0170 / 0.0072 / 0.0045   (limits 0.08 / 0.02 / 0.08)
        relpos_table    0.0262 / 0.0139 / 0.0542   (limits 0.11 / 0.03 / 0.11)
    every figure x 1.3 is inside its limit (the headroom those limits were set with).  A first version of the fixture (uniform
    noise images, 20 x 28 inputs) put the pre-existing loop at 0.0786 sampled error in `blocks`, inside the limit but without that
    headroom, so the fixture's inputs were changed (smooth 8-bit scenes, 32 x 40 inputs), not the limits.
    Grouped against ungrouped: worst per-parameter relative L2 1.97e-7 (bound 2e-2)."""
    d, lrs, hrs = fixture_samples(golden_dir)
    grads = {}
    for name in ("parent", "ungrouped", "grouped"):
        m = ft_model()
        opt = harness.make_optimizer(m, 1e-4)
        if name == "parent":
            loss = parent_step(m, opt, lrs, hrs)
        else:
            loss = harness.train_step_samples(m, opt, lrs, hrs, group=(name == "grouped"))
        print(f"{name}: loss {loss.item():.6f} (reference {float(d['loss']):.6f}, |diff| {abs(loss.item() - float(d['loss'])):.2e})")
        assert abs(loss.item() - float(d["loss"])) <= 2e-3, (name, loss.item(), float(d["loss"]))
        T_r2._check_grads_vs_fixture(m, d)
        grads[name] = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
        assert len(grads[name]) == 113
    worst = (0.0, "")
    for k, ref in grads["ungrouped"].items():
        rel = (grads["grouped"][k] - ref).norm().item() / max(ref.norm().item(), 1e-12)
        worst = max(worst, (rel, k))
        assert rel <= 2e-2, (k, rel)
    print(f"grouped vs ungrouped: worst per-parameter relative L2 {worst[0]:.2e} ({worst[1]})")


# ---- 4. unused scales ----
def test_unused_scales_keep_no_gradient_and_no_adam_state(golden_dir):
    _, lrs, hrs = fixture_samples(golden_dir)
    m = ft_model()
    opt = harness.make_optimizer(m, 1e-4)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    for _ in range(2):
        harness.train_step_samples(m, opt, lrs[:2], hrs[:2])          # x2 samples only
    torch.cuda.synchronize()
    other = [k for k, _ in m.named_parameters() if ".upsamplers." in k and not k.split(".upsamplers.")[1].startswith("2.")]
    assert other and {k.split(".upsamplers.")[1].split(".")[0] for k in other} == {"3", "4", "6"}
    for k, p in m.named_parameters():
        if k in other:
            assert p.grad is None and len(opt.state.get(p, {})) == 0 and torch.equal(p, before[k]), k
        else:
            assert p.grad is not None and "exp_avg" in opt.state[p] and not torch.equal(p, before[k]), k
    # a later step at another scale brings that scale's upsamplers in
    harness.train_step_samples(m, opt, lrs[2:3], hrs[2:3])
    named = dict(m.named_parameters())
    assert all(named[k].grad is not None for k in other if ".upsamplers.3." in k)
    assert all(named[k].grad is None for k in other if ".upsamplers.4." in k or ".upsamplers.6." in k)
    assert all(named[k].grad is None for k in named if ".upsamplers.2." in k)


def test_accumulator_api_guards(golden_dir):
    m = ft_model()
    acc = GradAccumulator(m)
    assert acc.total_floats % 64 == 0 and all(o % 64 == 0 for o in acc.offset.values())
    assert list(acc.names) == [k for k, p in m.named_parameters() if p.requires_grad]
    g = torch.ones_like(m.conv1.bias)
    with pytest.raises(RuntimeError, match="begin"):
        acc.add({"conv1.bias": g})
    acc.begin()
    with pytest.raises(RuntimeError, match="layout"):
        acc.add({"no.such.parameter": g})
    with pytest.raises(ValueError):
        acc.add({"conv1.weight": g})
    with pytest.raises(TypeError):
        acc.add({"conv1.bias": g.double()})
    acc.add({"conv1.bias": g, "conv2.bias": None})
    acc.add({"conv1.bias": g}, alpha=0.5)
    assert acc.finish() == ["conv1.bias"]
    assert torch.equal(m.conv1.bias.grad, torch.full_like(g, 1.5)) and m.conv2.bias.grad is None
    # an error inside the step restores the suspended reducer and leaves the accumulator closed
    opt = harness.make_optimizer(m, 1e-4)
    _, lrs, hrs = fixture_samples(golden_dir)

    def boom(out, target):
        raise ZeroDivisionError("criterion failed")
    with pytest.raises(ZeroDivisionError):
        harness.train_step_samples(m, opt, lrs[:1], hrs[:1], loss=boom)
    assert m._grad_reducer is None and m._grad_accumulator._touched is None


# ---- 5. two ranks on one GPU ----
def test_two_ranks_reduce_once_per_step(golden_dir, tmp_path):
    """Rank 0: samples 0, 1 (x2) and 2 (x3); rank 1: sample 4 (x6); group=False.  The reduced gradients equal the single-process
    gradients of the four samples to <= 1e-3 relative L2 (same kernels, another summation order); a parameter touched on one rank
    only has a gradient on both; one round of bucket all-reduces per step."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_mixed_dp_worker.py")
    outfile = str(tmp_path / "mixed_dp")
    rdzv = outfile + ".rdzv"
    procs = [subprocess.Popen([sys.executable, worker, str(r), "2", "file://" + rdzv, outfile], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    try:
        outs = [p.communicate(timeout=420)[0] for p in procs]
    except subprocess.TimeoutExpired:
        for p in procs:
            p.kill()
        pytest.fail("DP workers stalled:\n" + "\n-----\n".join(p.communicate()[0] for p in procs))
    assert all(p.returncode == 0 for p in procs), outs
    ranks = [torch.load(f"{outfile}.{r}.pt") for r in range(2)]

    _, lrs, hrs = fixture_samples(golden_dir)
    pick = [0, 1, 2, 4]
    m = ft_model()
    opt = harness.make_optimizer(m, 1e-4)
    loss = harness.train_step_samples(m, opt, [lrs[i] for i in pick], [hrs[i] for i in pick], group=False)
    ref = {k: p.grad.detach().cpu().double() for k, p in m.named_parameters() if p.grad is not None}
    assert any(".upsamplers.6." in k for k in ref) and any(".upsamplers.3." in k for k in ref)
    assert not any(".upsamplers.4." in k for k in ref)
    worst = (0.0, "")
    for r, rec in enumerate(ranks):
        assert set(rec["grads"]) == set(ref), (r, sorted(set(rec["grads"]) ^ set(ref))[:6])      # touched on SOME rank <=> gradient
        for k, g in ref.items():
            rel = (rec["grads"][k].double() - g).norm().item() / max(g.norm().item(), 1e-12)
            worst = max(worst, (rel, k))
            assert rel <= 1e-3, (r, k, rel)
        assert rec["nbuckets"] > 1 and rec["launched_order"] == list(range(rec["nbuckets"])), rec["launched_order"]
        assert rec["episodes"] == 0          # the model's backward opened no reducer episode of its own
        assert rec["reducer_restored"]
    for k in ref:
        assert torch.equal(ranks[0]["grads"][k], ranks[1]["grads"][k]), k
    # the ranks' weighted losses sum to world x the step's mean loss
    assert abs((ranks[0]["loss"] + ranks[1]["loss"]) / 2 - loss.item()) <= 1e-5
    # second step: rank 1 holds no sample at all and still takes part
    for r, rec in enumerate(ranks):
        assert rec["step2_launched_order"] == list(range(rec["nbuckets"]))
        assert not any(".upsamplers.6." in k for k in rec["step2_grad_names"])
        assert any(".upsamplers.2." in k for k in rec["step2_grad_names"])
    assert ranks[0]["step2_grad_names"] == ranks[1]["step2_grad_names"]
    print(f"two ranks vs single process: worst per-parameter relative L2 {worst[0]:.2e} ({worst[1]})")


# ---- 6. the driver ----
def _write_images(d, n, hw=(64, 64)):
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    yy, xx = np.mgrid[0:hw[0], 0:hw[1]].astype(np.float64)
    for i in range(n):
        rng = np.random.RandomState(i)
        planes = [127 + 90 * np.sin(yy / (5 + c + i) + c) * np.cos(xx / (7 + 2 * c - i) + i) + rng.normal(0, 6, hw) for c in range(3)]
        Image.fromarray(np.clip(np.stack(planes, -1), 0, 255).astype(np.uint8)).save(os.path.join(d, f"img_{i}.png"))


def _train(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py")] + args, cwd=cwd, env=env, capture_output=True, text=True,
                       timeout=600)
    return r.returncode, r.stdout + r.stderr


def test_train_driver_checkpoints_resumes_and_is_reproducible(tmp_path):
    data = str(tmp_path / "images")
    _write_images(data, 3)
    common = ["--data_dir", data, "--pairs", "32x32:64x64,24x24:72x72", "--batch_size", "3", "--deterministic", "--seed", "7"]
    cks = [str(tmp_path / f"ck{i}") for i in range(2)]
    for ck in cks:          # two identical invocations
        code, out = _train(common + ["--epochs", "1", "--max_steps", "2", "--checkpoint_dir", ck], str(tmp_path))
        assert code == 0, out
        assert "Epoch [1/1] Step [1/2] Loss:" in out and "Epoch [1/1] Step [2/2] Loss:" in out and "Average Loss:" in out, out
        assert os.path.exists(os.path.join(ck, "model_epoch_1.pth")), out
    a, b = (torch.load(os.path.join(ck, "model_epoch_1.pth"), map_location="cpu") for ck in cks)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    fresh = importlib.import_module("models.FastTransformer.model").TransformerModel()
    init = {k: v.clone() for k, v in fresh.state_dict().items()}
    fresh.load_state_dict(a)                                             # strict
    assert any(not torch.equal(a[k], init[k]) for k in a if a[k].is_floating_point())
    # a second invocation resumes at epoch 1; one that asks for no more epochs is refused
    code, out = _train(common + ["--epochs", "2", "--max_steps", "1", "--checkpoint_dir", cks[0]], str(tmp_path))
    assert code == 0 and "Resuming from epoch 1" in out and "Epoch [2/2] Step [1/2]" in out, out
    assert os.path.exists(os.path.join(cks[0], "model_epoch_2.pth"))
    code, out = _train(common + ["--epochs", "1", "--checkpoint_dir", cks[1]], str(tmp_path))
    assert code != 0 and "not below --epochs 1" in out, out
    code, out = _train(["--model", "BicubicInterpolation", "--data_dir", data], str(tmp_path))
    assert code != 0 and "no trainable parameter" in out, out


def test_train_driver_overfits_one_image(tmp_path):
    data = str(tmp_path / "one")
    _write_images(data, 1)
    rec = str(tmp_path / "run.json")
    code, out = _train(["--data_dir", data, "--pairs", "32x32:64x64", "--batch_size", "1", "--epochs", "40", "--deterministic",
                        "--checkpoint_interval", "1000", "--checkpoint_dir", str(tmp_path / "ck"), "--json", rec, "--log_interval", "1"],
                       str(tmp_path))
    assert code == 0, out
    steps = json.load(open(rec))["steps"]
    assert len(steps) == 40
    first, last = steps[0]["loss"], steps[-1]["loss"]
    print(f"overfit one image, 40 steps: first loss {first:.5f}, last {last:.5f}")
    assert last < first, (first, last)
