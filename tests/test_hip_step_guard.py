"""The guarded optimizer step on the MI355X (csrc/step_guard.hip, optim.Adam / optim.AdamW, harness, train.py): the global
gradient norm, clipping, the skipping of steps with non-finite gradients and fused weight decay.  References are stock torch and
fp64 arithmetic written here, never the code under test.

Tolerances.  The norm: every lane accumulates exact fp64 squares in fp64, so whatever the summation order the relative error of the
sum is at most N * 2^-53 (N <= 6.5 M elements: 7.2e-10) and the square root halves it; the bound is 1e-9.  The trajectories: the
project's own bounds of tests/test_hip_train.py::test_fused_adam_equals_torch_adam (parameters rtol 2e-6 / atol 1e-7, exp_avg atol
1e-8, exp_avg_sq atol 1e-10, step counts equal).  Everything about skipping and reproducibility is `torch.equal`."""
import importlib
import json
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from transformerupscaler_amd import _lib, harness, ops
from transformerupscaler_amd.optim import Adam, AdamW
from transformerupscaler_amd.weights import deterministic_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
SIZES = [1, 63, 4095, 4096, 4097, 8197, 64 * 64 * 3 * 3]          # ..., a conv3x3 64 -> 64 weight
REC = struct.Struct("<ddfifiQQQQ")                                 # sumsq, norm, coef, apply, norm_f32, clipped, steps, applied, clipped, skipped
SHAPES = [(64, 3, 3, 3), (192,), (5000,), (768, 192), (1,)]        # the shapes of test_fused_adam_equals_torch_adam


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    ops.deterministic = False
    ops.release_det_slabs()


def ft_model():
    m = importlib.import_module("models.FastTransformer.model").TransformerModel()
    m.load_state_dict(deterministic_state_dict(0), strict=False)
    return m.to(DEV).eval()


# ---- 1. the norm kernels ----
class NormHarness:
    """Gradient segments inside one sentinel-guarded arena (segment i starts `shift` floats off a 64-float boundary), the partials and
    the guard record inside sentinel-guarded buffers of their own; `run()` issues tup_grad_sumsq_partial + tup_grad_guard_finish."""

    def __init__(self, sizes, shift, seed):
        gen = torch.Generator(device=DEV).manual_seed(seed)
        self.offs, cur = [], GUARD
        for n in sizes:
            cur = (cur + 63) // 64 * 64 + shift
            self.offs.append((cur, n))
            cur += n + GUARD
        self.arena = torch.randn((cur,), generator=gen, device=DEV)
        tab = []
        for si, (_, n) in enumerate(self.offs):
            tab += [(si, off) for off in range(0, n, 4096)]
        self.chunks = torch.tensor(tab, dtype=torch.int32, device=DEV)
        self.segs = torch.tensor([[self.arena.data_ptr() + 4 * o, n] for o, n in self.offs], dtype=torch.int64, device=DEV)
        self.partials = torch.full((8 + len(tab) + 8,), -7.0, dtype=torch.float64, device=DEV)
        self.rec = torch.full((4 + 8 + 4,), 0x5A5A5A5A, dtype=torch.int64, device=DEV)
        self.rec[4:12] = 0

    def segments(self):
        return [self.arena[o:o + n] for o, n in self.offs]

    def run(self, max_norm, skip_nonfinite):
        before = self.arena.clone()
        stream = torch.cuda.current_stream().cuda_stream
        n = self.chunks.shape[0]
        _lib.call("tup_grad_sumsq_partial", self.segs.data_ptr(), self.chunks.data_ptr(), n, self.partials.data_ptr() + 64, stream)
        _lib.call("tup_grad_guard_finish", self.partials.data_ptr() + 64, n, float(max_norm), int(skip_nonfinite),
                  self.rec.data_ptr() + 32, stream)
        torch.cuda.synchronize()
        # bitwise: NaN sentinels / planted values compare as their words
        assert torch.equal(self.arena.view(torch.int32), before.view(torch.int32)), "the gradients were written"
        assert (self.partials[:8] == -7.0).all() and (self.partials[-8:] == -7.0).all(), "floats around the partials were written"
        assert (self.rec[:4] == 0x5A5A5A5A).all() and (self.rec[-4:] == 0x5A5A5A5A).all(), "words around the guard record were written"
        raw = self.rec[4:12].cpu().numpy().tobytes()
        return REC.unpack(raw), raw


def fp64_norm(tensors):
    return math.sqrt(sum((t.double() ** 2).sum().item() for t in tensors))


@pytest.mark.parametrize("shift", [0, 1, 3])
def test_norm_kernel_against_fp64(shift):
    h = NormHarness(SIZES, shift, 11 + shift)
    if shift % 4:
        assert any(s.data_ptr() % 16 for s in h.segments())
    want = fp64_norm(h.segments())
    rec, raw = h.run(max_norm=want / 4, skip_nonfinite=True)
    rel = abs(rec[1] - want) / want
    print(f"shift {shift}: norm {rec[1]!r} fp64 reference {want!r} relative error {rel:.3e}")
    assert rel <= 1e-9
    assert abs(rec[0] - want * want) / (want * want) <= 2e-9
    coef = np.float32(min(1.0, (want / 4) / (want + 1e-6)))
    assert abs(rec[2] - float(coef)) <= 2.0 ** -23 * float(coef) and rec[2] < 1.0      # the reference's coef, at most one fp32 ulp off
    assert rec[2] == float(np.float32(min(1.0, (want / 4) / (rec[1] + 1e-6))))         # and exactly the rounding of its own norm
    assert rec[3] == 1 and rec[5] == 1 and rec[4] == float(np.float32(rec[1]))
    assert rec[6:] == (1, 1, 1, 0)
    # a second launch on the same gradients: the same bits (there is no atomic and no order that depends on timing)
    rec2, raw2 = h.run(max_norm=want / 4, skip_nonfinite=True)
    assert raw2[:32] == raw[:32] and rec2[6:] == (2, 2, 2, 0)
    # no max_norm: coef is exactly 1; a large one: not clipped
    assert h.run(max_norm=-1.0, skip_nonfinite=False)[0][2] == 1.0
    rec4, _ = h.run(max_norm=want * 2, skip_nonfinite=False)
    assert rec4[2] == 1.0 and rec4[5] == 0 and rec4[6:] == (4, 4, 2, 0)


def test_norm_of_zero_gradients():
    h = NormHarness(SIZES, 0, 3)
    for s in h.segments():
        s.zero_()
    rec, _ = h.run(max_norm=1.0, skip_nonfinite=True)
    assert rec[0] == 0.0 and rec[1] == 0.0 and rec[2] == 1.0 and rec[3] == 1 and rec[5] == 0


@pytest.mark.parametrize("value", [float("inf"), float("-inf"), float("nan")])
def test_one_nonfinite_element_clears_apply(value):
    for where in ("first", "last"):
        h = NormHarness(SIZES, 1, 5)
        seg = h.segments()[0 if where == "first" else -1]
        seg[0 if where == "first" else -1] = value
        rec, _ = h.run(max_norm=1.0, skip_nonfinite=True)
        assert rec[3] == 0 and rec[5] == 0 and rec[6:] == (1, 0, 0, 1), (value, where, rec)
        assert not math.isfinite(rec[0])
        rec, _ = h.run(max_norm=1.0, skip_nonfinite=False)          # without the option the step is applied, as torch would
        assert rec[3] == 1 and (rec[6], rec[7], rec[9]) == (2, 1, 1), (value, where, rec)
        assert not rec[2] > 0.0                                      # clip_grad_norm_'s coef of an infinite norm is 0, of a NaN norm NaN


# ---- 2. trajectory against torch ----
def _fp32_coef(grads, max_norm):
    norm64 = fp64_norm(grads)
    return float(np.float32(min(1.0, max_norm / (norm64 + 1e-6)))), norm64


@pytest.mark.parametrize("cls,ref_cls,wd", [(Adam, torch.optim.Adam, 0.0), (Adam, torch.optim.Adam, 1e-2), (AdamW, torch.optim.AdamW, 1e-2)])
def test_guarded_trajectory_equals_torch(cls, ref_cls, wd):
    g = torch.Generator(device=DEV).manual_seed(7)
    base = [torch.randn(s, device=DEV, generator=g) for s in SHAPES]
    pa = [torch.nn.Parameter(b.clone()) for b in base]
    pb = [torch.nn.Parameter(b.clone()) for b in base]
    groups = lambda ps: [{"params": ps[:3], "lr": 1e-3}, {"params": ps[3:], "lr": 3e-4}]      # noqa: E731
    oa = cls(groups(pa), weight_decay=wd, max_grad_norm=50.0, skip_nonfinite=True)
    ob = ref_cls(groups(pb), weight_decay=wd)
    scales = [5.0, 0.01, 5.0, 0.01, 1.0, 1.0]
    clipped = []
    for step, scale in enumerate(scales):
        grads = []
        for i, (x, y) in enumerate(zip(pa, pb)):
            if step == 1 and i == 2:
                x.grad = y.grad = None
                continue
            gr = torch.randn(x.shape, device=DEV, generator=g) * scale
            if step == 4 and i == 3:
                gr[5, 7] = float("inf")
            grads.append(gr)
            x.grad, y.grad = gr.clone(), gr.clone()
        kept = [x.grad.clone() if x.grad is not None else None for x in pa]
        before = [(x.detach().clone(), {k: v.clone() for k, v in oa.state[x].items()} if x in oa.state else None) for x in pa]
        oa.step()
        if step != 4:
            coef, norm64 = _fp32_coef(grads, 50.0)
            clipped.append(coef < 1.0)
            for y in pb:
                if y.grad is not None:
                    y.grad.mul_(coef)
            ob.step()
            assert abs(oa.grad_norm.item() - norm64) <= 1e-6 * norm64
        oa.guard_stats()                                           # settles: a skipped step's counts are taken back
        for x, k in zip(pa, kept):                                 # p.grad keeps the unclipped gradient
            assert (x.grad is None and k is None) or torch.equal(x.grad, k)
        for i, (x, y) in enumerate(zip(pa, pb)):
            if step == 4:
                assert torch.equal(x.detach(), before[i][0]), i
                for k, v in before[i][1].items():
                    assert torch.equal(oa.state[x][k], v), (i, k)
            assert torch.allclose(x, y, rtol=2e-6, atol=1e-7), (step, i, (x - y).abs().max().item())
            sa, sb = oa.state[x], ob.state[y]
            assert float(sa["step"]) == float(sb["step"]), (step, i)
            assert torch.allclose(sa["exp_avg"], sb["exp_avg"], rtol=2e-6, atol=1e-8), (step, i)
            assert torch.allclose(sa["exp_avg_sq"], sb["exp_avg_sq"], rtol=2e-6, atol=1e-10), (step, i)
    assert clipped == [True, False, True, False, True]
    assert oa.guard_stats() == {"steps": 6, "applied": 5, "clipped": 3, "skipped": 1}
    assert float(oa.state[pa[2]]["step"]) == 4.0 and float(oa.state[pa[0]]["step"]) == 5.0
    # the options are not in the state_dict: it loads into torch's class and torch's into this one
    ref_cls(groups(pb), weight_decay=wd).load_state_dict(oa.state_dict())
    cls(groups(pa), weight_decay=wd, max_grad_norm=50.0).load_state_dict(ob.state_dict())


# ---- 3. launches ----
class Launches:
    def __init__(self, monkeypatch):
        self.names, self.torch_steps = [], 0
        real_call, real_step = _lib.call, torch.optim.Adam.step

        def call(name, *a):
            self.names.append(name)
            return real_call(name, *a)

        def step(opt, *a, **k):
            self.torch_steps += 1
            return real_step(opt, *a, **k)
        monkeypatch.setattr(_lib, "call", call)
        monkeypatch.setattr(torch.optim.Adam, "step", step)


def _params_with_grads(seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, device=DEV, generator=g)) for s in SHAPES]
    for p in ps:
        p.grad = torch.randn(p.shape, device=DEV, generator=g)
    return ps


def test_options_off_issue_the_single_unguarded_launch(monkeypatch):
    for cls, kw in ((Adam, {}), (AdamW, {"weight_decay": 0.0})):
        opt = cls(_params_with_grads(), lr=1e-3, **kw)
        seen = Launches(monkeypatch)
        opt.step()
        opt.step()
        torch.cuda.synchronize()
        assert seen.names == ["tup_adam_step", "tup_adam_step"] and seen.torch_steps == 0, (cls, seen.names)
        assert opt.grad_norm is None and opt.guard_stats()["steps"] == 0
        monkeypatch.undo()


@pytest.mark.parametrize("cls,ref_cls", [(Adam, torch.optim.Adam), (AdamW, torch.optim.AdamW)])
def test_weight_decay_runs_in_the_fused_launch(monkeypatch, cls, ref_cls):
    pa, pb = _params_with_grads(), _params_with_grads()
    oa, ob = cls(pa, lr=1e-3, weight_decay=1e-2), ref_cls(pb, lr=1e-3, weight_decay=1e-2)
    ob.step()                                                      # the reference, before torch's step is instrumented
    seen = Launches(monkeypatch)
    oa.step()
    torch.cuda.synchronize()
    assert seen.names == ["tup_adam_step_guarded"] and seen.torch_steps == 0, seen.names
    for x, y, x0 in zip(pa, pb, _params_with_grads()):
        assert torch.allclose(x, y, rtol=2e-6, atol=1e-7)
        assert not torch.equal(x, x0)                              # and it did step


def test_guarded_step_is_three_launches(monkeypatch):
    opt = Adam(_params_with_grads(), lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0, skip_nonfinite=True)
    seen = Launches(monkeypatch)
    opt.step()
    torch.cuda.synchronize()
    assert seen.names == ["tup_grad_sumsq_partial", "tup_grad_guard_finish", "tup_adam_step_guarded"] and seen.torch_steps == 0
    assert opt.grad_norm.dtype == torch.float32 and opt.grad_norm.is_cuda and opt.grad_norm.dim() == 0


def test_guard_options_refuse_what_the_kernel_cannot_take():
    p = torch.nn.Parameter(torch.ones(8, device=DEV))
    with pytest.raises(ValueError):
        Adam([p], lr=1e-3, amsgrad=True, max_grad_norm=1.0)
    with pytest.raises(ValueError):
        Adam([torch.nn.Parameter(torch.ones(8, device=DEV, dtype=torch.float64))], lr=1e-3, skip_nonfinite=True)
    opt = Adam([p], lr=1e-3, skip_nonfinite=True)
    if hasattr(p, "grad_dtype"):
        p.grad_dtype = None                                       # newer torch pins a gradient's dtype to the parameter's unless told
    p.grad = torch.ones(8, device=DEV, dtype=torch.float64)       # a gradient the kernel cannot read
    with pytest.raises(ValueError):
        opt.step()


# ---- 4. the host runs ahead ----
def test_host_running_ahead_equals_synchronised_steps():
    g = torch.Generator(device=DEV).manual_seed(21)
    base = [torch.randn(s, device=DEV, generator=g) for s in SHAPES]
    steps = [[torch.randn(s, device=DEV, generator=g) * (3.0 if k % 2 else 0.05) for s in SHAPES] for k in range(12)]
    steps[6][2][17] = float("nan")

    def run(sync):
        ps = [torch.nn.Parameter(b.clone()) for b in base]
        opt = AdamW(ps, lr=1e-3, weight_decay=1e-2, max_grad_norm=40.0, skip_nonfinite=True)
        for grads in steps:
            for p, gr in zip(ps, grads):
                p.grad = gr
            opt.step()
            if sync:
                torch.cuda.synchronize()
        stats = opt.guard_stats()
        return ps, opt, stats

    pa, oa, sa = run(False)
    pb, ob, sb = run(True)
    assert sa == sb and sa["steps"] == 12 and sa["skipped"] == 1 and sa["applied"] == 11 and 0 < sa["clipped"] < 11
    for x, y in zip(pa, pb):
        assert torch.equal(x, y) and not torch.isnan(x).any()
        assert float(oa.state[x]["step"]) == float(ob.state[y]["step"]) == 11.0
        assert torch.equal(oa.state[x]["exp_avg"], ob.state[y]["exp_avg"])
        assert torch.equal(oa.state[x]["exp_avg_sq"], ob.state[y]["exp_avg_sq"])


# ---- 5. a poisoned batch on the model ----
def _batch(seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((1, 3, 64, 96), generator=g).to(DEV), torch.rand((1, 3, 96, 144), generator=g).to(DEV)


def _state(model, opt):
    torch.cuda.synchronize()
    out = {"p." + k: p.detach().clone() for k, p in model.named_parameters()}
    for k, p in model.named_parameters():
        for name, v in opt.state.get(p, {}).items():
            out[f"s.{k}.{name}"] = v.detach().clone()
    return out


def _poison_sequence(skip_nonfinite):
    m = ft_model()
    opt = harness.make_optimizer(m, 1e-4, skip_nonfinite=skip_nonfinite)
    lr, hr = _batch()
    bad = lr.clone()
    bad[0, 1, 30, 40] = float("nan")
    harness.train_step(m, opt, lr, hr)                               # a clean step first: the Adam state exists
    if skip_nonfinite:
        opt.guard_stats()
    before = _state(m, opt)
    harness.train_step(m, opt, bad, hr)
    if skip_nonfinite:
        stats = opt.guard_stats()
    else:
        stats = None
    after = _state(m, opt)
    loss = harness.train_step(m, opt, lr, hr)
    return m, opt, before, after, stats, loss.item()


def test_poisoned_batch_is_skipped_on_the_model():
    m, opt, before, after, stats, loss = _poison_sequence(True)
    assert stats == {"steps": 2, "applied": 1, "clipped": 0, "skipped": 1}
    assert before.keys() == after.keys() and any(k.startswith("s.") for k in before)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    final = _state(m, opt)
    assert math.isfinite(loss)
    assert any(not torch.equal(final[k], after[k]) for k in after if k.startswith("p."))          # the clean step moved the weights
    assert not any(torch.isnan(v).any() for v in final.values())
    assert opt.guard_stats() == {"steps": 3, "applied": 2, "clipped": 0, "skipped": 1}
    # the contrast (a numerical outcome, not a fault): without the option the same sequence poisons the parameters
    m2, opt2, _, after2, _, _ = _poison_sequence(False)
    assert any(torch.isnan(v).any() for k, v in after2.items() if k.startswith("p."))


# ---- 6. clipping on the model ----
def test_clipping_on_the_model_equals_torch_on_scaled_gradients():
    lr, hr = _batch(1)
    with ops.deterministic_mode(True):
        probe = ft_model()
        probe_opt = torch.optim.SGD(probe.parameters(), lr=0.0)      # train_step needs one; lr 0 and no momentum: nothing moves
        harness.train_step(probe, probe_opt, lr, hr)
        grads = {k: p.grad.detach().clone() for k, p in probe.named_parameters() if p.grad is not None}
        n = fp64_norm(grads.values())
        assert n > 0 and math.isfinite(n)
        m = ft_model()
        opt = harness.make_optimizer(m, 1e-4, max_grad_norm=n / 2)
        harness.train_step(m, opt, lr, hr)
    for k, p in m.named_parameters():                                 # the same deterministic step: the same gradients, unclipped
        assert (p.grad is None) == (k not in grads) and (p.grad is None or torch.equal(p.grad, grads[k])), k
    coef = float(np.float32(min(1.0, (n / 2) / (n + 1e-6))))
    assert 0.49 < coef < 0.5
    ref = ft_model()
    ref_opt = torch.optim.Adam(ref.parameters(), lr=1e-4)
    for k, p in ref.named_parameters():
        if k in grads:
            p.grad = grads[k] * coef
    ref_opt.step()
    rp = dict(ref.named_parameters())
    for k, p in m.named_parameters():
        assert torch.allclose(p, rp[k], rtol=2e-6, atol=1e-7), (k, (p - rp[k]).abs().max().item())
        if k in grads:
            assert torch.allclose(opt.state[p]["exp_avg"], ref_opt.state[rp[k]]["exp_avg"], rtol=2e-6, atol=1e-8), k
            assert torch.allclose(opt.state[p]["exp_avg_sq"], ref_opt.state[rp[k]]["exp_avg_sq"], rtol=2e-6, atol=1e-10), k
    assert opt.grad_norm.dtype == torch.float32 and opt.grad_norm.shape == ()
    got = opt.grad_norm.item()
    print(f"model gradient norm: fp64 {n!r}, optimizer.grad_norm {got!r}")
    assert abs(got - n) <= 1e-6 * n
    assert opt.guard_stats() == {"steps": 1, "applied": 1, "clipped": 1, "skipped": 0}


# ---- 7. reproducibility ----
def test_guarded_mixed_steps_are_bit_reproducible(golden_dir):
    d = dict(np.load(os.path.join(golden_dir, "train_mixed_step.npz"), allow_pickle=False))
    lrs, hrs = ([torch.from_numpy(d[f"{k}_u8_{i}"]).float().div(255.0).unsqueeze(0).to(DEV) for i in range(3)] for k in ("lr", "hr"))

    def run():
        m = ft_model()
        opt = harness.make_optimizer(m, 1e-4, weight_decay=1e-2, decoupled=True, max_grad_norm=1e-3, skip_nonfinite=True)
        with ops.deterministic_mode(True):
            losses = [harness.train_step_samples(m, opt, lrs, hrs).clone() for _ in range(3)]
        norm = opt.grad_norm.clone()
        st = _state(m, opt)
        st["loss"], st["norm"] = torch.stack(losses), norm
        return st, opt.guard_stats()

    a, sa = run()
    b, sb = run()
    assert sa == sb == {"steps": 3, "applied": 3, "clipped": 3, "skipped": 0}
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- 8. two ranks on one GPU ----
def test_two_ranks_take_the_same_decisions(tmp_path):
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_step_guard_dp_worker.py")
    outfile = str(tmp_path / "guard_dp")
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
    r0, r1 = (torch.load(f"{outfile}.{r}.pt") for r in range(2))
    assert len(r0["norm_bits"]) == 3 and r0["norm_bits"] == r1["norm_bits"], (r0["norm_bits"], r1["norm_bits"])
    assert math.isfinite(r0["norms"][0]) and r0["norms"][0] > 0 and not math.isfinite(r0["norms"][1]) and math.isfinite(r0["norms"][2])
    assert r0["stats"] == r1["stats"] == {"steps": 3, "applied": 2, "clipped": 2, "skipped": 1}
    assert r0["skipped_step_unchanged"] and r1["skipped_step_unchanged"]
    assert r0["params"].keys() == r1["params"].keys()
    for k in r0["params"]:
        assert torch.equal(r0["params"][k], r1["params"][k]), k
        assert not torch.isnan(r0["params"][k]).any(), k
    assert any(not torch.equal(r0["params"][k], r0["initial"][k]) for k in r0["params"])


# ---- 9. the driver ----
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


def test_train_driver_flags_and_record(tmp_path):
    import train
    data = str(tmp_path / "images")
    _write_images(data, 4)
    common = ["--data_dir", data, "--pairs", "32x32:64x64", "--batch_size", "1", "--epochs", "1", "--deterministic",
              "--checkpoint_interval", "1000"]
    rec = str(tmp_path / "guarded.json")
    code, out = _train(common + ["--clip_grad_norm", "0.05", "--skip_nonfinite", "--warmup_steps", "2", "--lr", "2e-4",
                                 "--checkpoint_dir", str(tmp_path / "ck0"), "--json", rec], str(tmp_path))
    assert code == 0, out
    r = json.load(open(rec))
    assert len(r["steps"]) == 4 and "LR:" in out and "GradNorm:" in out
    for k, e in enumerate(r["steps"]):
        assert set(e) == {"epoch", "step", "loss", "lr", "grad_norm"}
        assert e["lr"] == train.lr_at(k, 2e-4, 2, "constant", 4, 0.0), (k, e)
        assert math.isfinite(e["grad_norm"]) and e["grad_norm"] > 0
    assert [e["lr"] for e in r["steps"]] == [1e-4, 2e-4, 2e-4, 2e-4]
    assert set(r["guard"]) == {"applied", "clipped", "skipped"}
    assert r["guard"]["applied"] == 4 and r["guard"]["skipped"] == 0 and 0 <= r["guard"]["clipped"] <= 4
    # cosine + AdamW
    rec2 = str(tmp_path / "cosine.json")
    code, out = _train(common + ["--adamw", "--weight_decay", "0.01", "--lr_schedule", "cosine", "--lr_min", "1e-6", "--warmup_steps", "1",
                                 "--checkpoint_dir", str(tmp_path / "ck1"), "--json", rec2], str(tmp_path))
    assert code == 0, out
    r2 = json.load(open(rec2))
    assert [e["lr"] for e in r2["steps"]] == [train.lr_at(k, 1e-4, 1, "cosine", 4, 1e-6) for k in range(4)]
    assert r2["steps"][-1]["lr"] == 1e-6 and all(e["grad_norm"] is None for e in r2["steps"])
    assert r2["guard"] == {"applied": 4, "clipped": 0, "skipped": 0}
    # no new flag: exactly the record and the lines of before
    rec3 = str(tmp_path / "plain.json")
    code, out = _train(common + ["--checkpoint_dir", str(tmp_path / "ck2"), "--json", rec3], str(tmp_path))
    assert code == 0, out
    r3 = json.load(open(rec3))
    assert set(r3) == {"model", "world", "samples", "resumed_from_epoch", "steps", "epochs", "checkpoints"}
    assert all(set(e) == {"epoch", "step", "loss"} for e in r3["steps"]) and len(r3["steps"]) == 4
    assert "LR:" not in out and "GradNorm" not in out and "Optimizer steps applied" not in out
