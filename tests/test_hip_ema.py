"""The weight average inside the fused optimizer step on the MI355X (`tup_adam_step_ema`, csrc/step_guard.hip; optim.Adam /
optim.AdamW ``ema_decay=``; harness.ema_weights).  Everything here is bitwise (`torch.equal` / equal words): the kernel's p, m, v
against the entry it replaces (`tup_adam_step`, `tup_adam_step_guarded`) on cloned inputs, and its average against the three
rounded torch operations ``d = p - e; d = d * w; e = e + d`` on the new p, with ``w = fp32(1 - d_n)``."""
import importlib
import os
import struct
import subprocess
import sys

import pytest
import torch

from transformerupscaler_amd import _lib, harness, ops, optim
from transformerupscaler_amd.optim import Adam, AdamW
from transformerupscaler_amd.weights import deterministic_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
SIZES = [1, 63, 4095, 4096, 4097, 8197, 64 * 64 * 3 * 3]          # ..., a conv3x3 64 -> 64 weight
SHAPES = [(64, 3, 3, 3), (192,), (5000,), (768, 192), (1,)]
FIELDS = ("p", "g", "m", "v", "e")
I32 = torch.int32


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    ops.deterministic = False
    ops.release_det_slabs()


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def lerp3(e, p, w):
    d = p - e
    d = d * w
    return e + d


# ---- 1. the kernel through the C ABI ----
class Arena:
    """p, g, m, v, e of every segment inside one arena: each array starts `shift` floats off a 64-float boundary and has 64 floats
    of sentinel on either side.  `clone()` gives the same values at other addresses, for the entry the kernel is compared with."""

    def __init__(self, sizes, shift, seed=None, values=None):
        self.sizes, self.shift = sizes, shift
        self.off, cur = {}, GUARD
        for f in FIELDS:
            for si, n in enumerate(sizes):
                cur = (cur + 63) // 64 * 64 + shift
                self.off[f, si] = cur
                cur += n + GUARD
        if values is None:
            gen = torch.Generator(device=DEV).manual_seed(seed)
            values = torch.randn((cur,), generator=gen, device=DEV)
            for si, n in enumerate(sizes):                    # exp_avg_sq is a mean of squares
                o = self.off["v", si]
                values[o:o + n] = values[o:o + n].square() * 1e-2
        self.arena = values.clone()
        self.before = self.arena.clone()
        owned = torch.zeros(cur, dtype=torch.bool, device=DEV)
        for (f, si), o in self.off.items():
            owned[o:o + sizes[si]] = True
        self.outside = ~owned
        tab = []
        for si, n in enumerate(sizes):
            tab += [(si, o) for o in range(0, n, 4096)]
        self.chunks = torch.tensor(tab, dtype=I32, device=DEV)

    def clone(self):
        return Arena(self.sizes, self.shift, values=self.before)

    def view(self, f, si, which=None):
        o = self.off[f, si]
        return (self.arena if which is None else which)[o:o + self.sizes[si]]

    def ptr(self, f, si):
        return self.arena.data_ptr() + 4 * self.off[f, si]

    def unchanged(self, f, si):
        return torch.equal(self.view(f, si).view(I32), self.view(f, si, self.before).view(I32))

    def check_sentinels(self):
        assert torch.equal(self.arena[self.outside].view(I32), self.before[self.outside].view(I32)), "floats outside the segments were written"
        for si in range(len(self.sizes)):
            assert self.unchanged("g", si), "a gradient was written"


HYPER = dict(step_size=1e-3 / (1 - 0.9 ** 3), bc2=1 - 0.999 ** 3, beta2=0.999, omb1=1 - 0.9, omb2=1 - 0.999, eps=1e-8)


def _segs(a, form, wd_l2=0.0, decay=1.0, ema_w=None, no_grad=()):
    """The device table for arena `a`: the 64-byte records (form 'plain'), the 72-byte ones ('guarded') or the 88-byte EMA ones."""
    h = HYPER
    recs = []
    for si, n in enumerate(a.sizes):
        head = (a.ptr("p", si), 0 if si in no_grad else a.ptr("g", si), a.ptr("m", si), a.ptr("v", si), n, h["step_size"])
        tail = (h["beta2"], h["omb1"], h["omb2"], h["eps"])
        if ema_w is not None:
            bc2 = h["bc2"] ** 0.5 if form == "guarded" else 1.0 / h["bc2"] ** 0.5
            recs.append(optim._REC_EMA.pack(*head, bc2, *tail, wd_l2, decay, a.ptr("e", si), ema_w, 1 if form == "guarded" else 0))
        elif form == "guarded":
            recs.append(optim._REC_GUARDED.pack(*head, h["bc2"] ** 0.5, *tail, wd_l2, decay))
        else:
            recs.append(optim._REC.pack(*head, 1.0 / h["bc2"] ** 0.5, *tail))
    raw = b"".join(recs)
    return torch.frombuffer(bytearray(raw), dtype=torch.int64).to(DEV)


def _guard_record(coef, apply):
    raw = optim._REC_GUARD.pack(4.0, 2.0, coef, apply, 2.0, int(apply and coef < 1.0), 1, apply, 0, 1 - apply)
    return torch.frombuffer(bytearray(raw), dtype=torch.int64).to(DEV)


def _launch(name, a, segs, guard="absent"):
    stream = torch.cuda.current_stream().cuda_stream
    args = [segs.data_ptr(), a.chunks.data_ptr(), a.chunks.shape[0]]
    if guard != "absent":
        args.append(None if guard is None else guard.data_ptr())
    _lib.call(name, *args, stream)
    torch.cuda.synchronize()


W = f32(1.0 - 0.9)


@pytest.mark.parametrize("shift", [0, 1, 3])
def test_kernel_equals_the_entry_it_replaces(shift):
    cases = [("plain", 0.0, 1.0, "absent"),                   # tup_adam_step
             ("guarded", 0.0, 1.0, None), ("guarded", 1e-2, 1.0, None), ("guarded", 0.0, f32(1 - 1e-3 * 1e-2), None),      # no guard record
             ("guarded", 1e-2, 1.0, (1.0, 1)), ("guarded", 0.0, f32(1 - 1e-3 * 1e-2), (0.37, 1))]                           # applied; clipped
    for form, wd_l2, decay, guard in cases:
        a = Arena(SIZES, shift, seed=17 + shift)
        b = a.clone()
        if shift % 4:
            assert a.ptr("p", 0) % 16 and a.ptr("e", 0) % 16
        rec = _guard_record(*guard) if isinstance(guard, tuple) else None
        _launch("tup_adam_step_ema", a, _segs(a, form, wd_l2, decay, ema_w=W), rec)
        if form == "plain":
            _launch("tup_adam_step", b, _segs(b, "plain"))
        else:
            _launch("tup_adam_step_guarded", b, _segs(b, "guarded", wd_l2, decay), rec)
        a.check_sentinels()
        b.check_sentinels()
        for si in range(len(SIZES)):
            for f in ("p", "m", "v"):
                assert torch.equal(a.view(f, si).view(I32), b.view(f, si).view(I32)), (form, wd_l2, decay, guard, si, f)
                assert not a.unchanged(f, si), (form, si, f)
            assert b.unchanged("e", si)                       # the entry without the average never touched it
            want = lerp3(a.view("e", si, a.before), a.view("p", si), W)
            assert torch.equal(a.view("e", si).view(I32), want.view(I32)), (form, wd_l2, decay, guard, si)
            assert not a.unchanged("e", si)


@pytest.mark.parametrize("shift", [0, 3])
def test_kernel_skip_and_gradient_less_segments(shift):
    # a guard record with apply == 0: nothing is written
    a = Arena(SIZES, shift, seed=5)
    _launch("tup_adam_step_ema", a, _segs(a, "guarded", 1e-2, 1.0, ema_w=W), _guard_record(1.0, 0))
    a.check_sentinels()
    assert torch.equal(a.arena.view(I32), a.before.view(I32))
    # segments 1, 3 and 6 without a gradient (g = NULL): their average moves towards the unchanged p, m and v stay
    for form, rec in (("plain", None), ("guarded", _guard_record(0.5, 1))):
        a = Arena(SIZES, shift, seed=6)
        b = a.clone()
        idle = (1, 3, 6)
        _launch("tup_adam_step_ema", a, _segs(a, form, ema_w=W, no_grad=idle), rec)
        if form == "plain":
            _launch("tup_adam_step", b, _segs(b, "plain"))
        else:
            _launch("tup_adam_step_guarded", b, _segs(b, "guarded"), rec)
        a.check_sentinels()
        for si in range(len(SIZES)):
            if si in idle:
                assert a.unchanged("p", si) and a.unchanged("m", si) and a.unchanged("v", si), (form, si)
            else:
                for f in ("p", "m", "v"):
                    assert torch.equal(a.view(f, si).view(I32), b.view(f, si).view(I32)), (form, si, f)
            want = lerp3(a.view("e", si, a.before), a.view("p", si), W)
            assert torch.equal(a.view("e", si).view(I32), want.view(I32)) and not a.unchanged("e", si), (form, si)


# ---- 2. trajectories through the optimizer ----
@pytest.mark.parametrize("guarded", [False, True])
@pytest.mark.parametrize("cls,wd", [(Adam, 0.0), (Adam, 1e-2), (AdamW, 1e-2)])
def test_trajectory_raw_weights_and_average(cls, wd, guarded):
    g = torch.Generator(device=DEV).manual_seed(7)
    base = [torch.randn(s, device=DEV, generator=g) for s in SHAPES]
    pa = [torch.nn.Parameter(b.clone()) for b in base]
    pb = [torch.nn.Parameter(b.clone()) for b in base]
    groups = lambda ps: [{"params": ps[:3], "lr": 1e-3}, {"params": ps[3:], "lr": 3e-4}]      # noqa: E731
    kw = dict(max_grad_norm=50.0, skip_nonfinite=True) if guarded else {}
    oa = cls(groups(pa), weight_decay=wd, ema_decay=0.9, ema_warmup=True, **kw)
    ob = cls(groups(pb), weight_decay=wd, **kw)
    avg, n = [None] * len(SHAPES), 0
    for step, scale in enumerate([5.0, 0.01, 5.0, 0.01, 1.0, 1.0]):
        for i, (x, y) in enumerate(zip(pa, pb)):
            if (step == 0 and i == 4) or (step == 2 and i == 2):          # never stepped so far; stepped before: the average alone moves
                x.grad = y.grad = None
                continue
            gr = torch.randn(x.shape, device=DEV, generator=g) * scale
            if guarded and step == 4 and i == 3:
                gr[5, 7] = float("inf")
            x.grad, y.grad = gr.clone(), gr.clone()
        for i, y in enumerate(pb):
            if avg[i] is None and y.grad is not None:
                avg[i] = y.detach().clone()                   # created at the first step, from before the update
        oa.step()
        ob.step()
        skipped = guarded and step == 4
        if not skipped:
            w = f32(1.0 - optim.ema_decay_at(n, 0.9, True))
            avg = [None if e is None else lerp3(e, y.detach(), w) for e, y in zip(avg, pb)]
            n += 1
        assert oa.ema_updates == n, step
        if guarded:
            ob.guard_stats()
        for i, (x, y) in enumerate(zip(pa, pb)):
            assert torch.equal(x, y), (step, i)
            assert (x in oa.state) == (y in ob.state)
            if x in oa.state:
                assert float(oa.state[x]["step"]) == float(ob.state[y]["step"])
                assert torch.equal(oa.state[x]["exp_avg"], ob.state[y]["exp_avg"]), (step, i)
                assert torch.equal(oa.state[x]["exp_avg_sq"], ob.state[y]["exp_avg_sq"]), (step, i)
            if step == 0 and i == 4:
                assert x not in oa._ema
            else:
                assert torch.equal(oa._ema[x], avg[i]), (step, i)
    assert n == (5 if guarded else 6) and not torch.isnan(pa[3]).any()
    if guarded:
        assert oa.guard_stats() == ob.guard_stats() == {"steps": 6, "applied": 5, "clipped": 3, "skipped": 1}
    assert set(oa.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}


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


def test_launch_counts(monkeypatch):
    for kw, want in ((dict(), ["tup_adam_step_ema"]), (dict(weight_decay=1e-2), ["tup_adam_step_ema"]),
                     (dict(max_grad_norm=1.0, skip_nonfinite=True), ["tup_grad_sumsq_partial", "tup_grad_guard_finish", "tup_adam_step_ema"])):
        ps = _params_with_grads()
        opt = Adam(ps, lr=1e-3, ema_decay=0.99, **kw)
        seen = Launches(monkeypatch)
        opt.step()
        ps[1].grad = None                                     # a gradient-less parameter rides in the same launch
        opt.step()
        torch.cuda.synchronize()
        assert seen.names == want + want and seen.torch_steps == 0, (kw, seen.names)
        assert opt.ema_updates == 2
        monkeypatch.undo()
    opt = Adam(_params_with_grads(), lr=1e-3)                 # the option off: the launch of before
    seen = Launches(monkeypatch)
    opt.step()
    torch.cuda.synchronize()
    assert seen.names == ["tup_adam_step"] and seen.torch_steps == 0


# ---- 4. the host runs ahead ----
def test_host_running_ahead_equals_synchronised_steps():
    g = torch.Generator(device=DEV).manual_seed(21)
    base = [torch.randn(s, device=DEV, generator=g) for s in SHAPES]
    steps = [[torch.randn(s, device=DEV, generator=g) * (3.0 if k % 2 else 0.05) for s in SHAPES] for k in range(12)]
    steps[6][2][17] = float("nan")

    def run(sync):
        ps = [torch.nn.Parameter(b.clone()) for b in base]
        opt = AdamW(ps, lr=1e-3, weight_decay=1e-2, max_grad_norm=40.0, skip_nonfinite=True, ema_decay=0.9, ema_warmup=True)
        for k, grads in enumerate(steps):
            for i, (p, gr) in enumerate(zip(ps, grads)):
                p.grad = None if (k == 9 and i == 0) else gr
            opt.step()
            if sync:
                torch.cuda.synchronize()
        return ps, opt, opt.guard_stats()

    pa, oa, sa = run(False)
    pb, ob, sb = run(True)
    assert sa == sb and sa["steps"] == 12 and sa["skipped"] == 1
    assert oa.ema_updates == ob.ema_updates == 11
    for x, y in zip(pa, pb):
        assert torch.equal(x, y) and not torch.isnan(x).any()
        assert torch.equal(oa._ema[x], ob._ema[y]) and not torch.isnan(oa._ema[x]).any()
        assert not torch.equal(oa._ema[x], x.detach())


# ---- 5. FastTransformer, mixed scales ----
def ft_model():
    m = importlib.import_module("models.FastTransformer.model").TransformerModel()
    m.load_state_dict(deterministic_state_dict(0), strict=False)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def mixed_runs():
    """Three mixed-scale steps on LR 20 x 28 (scales 2 + 3, scale 2 alone, scales 2 + 3) with the average and without."""
    g = torch.Generator().manual_seed(4)
    lr = [torch.rand((1, 3, 20, 28), generator=g).to(DEV) for _ in range(2)]
    hr = [torch.rand((1, 3, 40, 56), generator=g).to(DEV), torch.rand((1, 3, 60, 84), generator=g).to(DEV)]
    out = {}
    for name in ("ema", "off"):
        m = ft_model()
        opt = harness.make_ema_optimizer(m, 0.9, lr=1e-4) if name == "ema" else harness.make_optimizer(m, 1e-4)
        snaps = []
        with ops.deterministic_mode(True):
            for lrs, hrs in ((lr, hr), (lr[:1], hr[:1]), (lr, hr)):
                harness.train_step_samples(m, opt, lrs, hrs)
                if name == "ema":
                    torch.cuda.synchronize()
                    snaps.append(({k: opt._ema[p].clone() for k, p in m.named_parameters() if p in opt._ema},
                                  {k: p.detach().clone() for k, p in m.named_parameters()}))
        out[name] = (m, opt, snaps)
    ops.deterministic = False
    ops.release_det_slabs()
    return out, lr, hr


def test_mixed_scale_steps_raw_weights_and_idle_average(mixed_runs):
    (runs, _, _) = mixed_runs
    (ma, oa, snaps), (mb, ob, _) = runs["ema"], runs["off"]
    pb = dict(mb.named_parameters())
    for k, p in ma.named_parameters():
        assert torch.equal(p, pb[k]), k
        assert (p in oa.state) == (pb[k] in ob.state), k
        if p in oa.state:
            assert float(oa.state[p]["step"]) == float(ob.state[pb[k]]["step"])
            assert torch.equal(oa.state[p]["exp_avg"], ob.state[pb[k]]["exp_avg"]), k
    assert oa.ema_updates == 3
    s3 = [k for k in snaps[0][0] if ".upsamplers.3." in k]
    assert s3 and not any(".upsamplers.4." in k or ".upsamplers.6." in k for k in snaps[0][0])          # never stepped: no buffer
    for k in s3:
        assert torch.equal(snaps[0][1][k], snaps[1][1][k]), k                 # no gradient in the scale-2 step: the weight stayed ...
        assert not torch.equal(snaps[0][0][k], snaps[1][0][k]), k             # ... and its average moved towards it
        assert torch.equal(snaps[1][0][k], lerp3(snaps[0][0][k], snaps[1][1][k], f32(1.0 - 0.9))), k
        assert float(oa.state[dict(ma.named_parameters())[k]]["step"]) == 2.0


def test_model_runs_on_the_average_without_invalidation(mixed_runs):
    runs, lr, hr = mixed_runs
    m, opt, _ = runs["ema"]
    x = lr[0]
    with torch.no_grad():
        before = m(x, res_out=(40, 56), require_ratio=False).clone()
        with harness.ema_weights(m, opt):
            inside = m(x, res_out=(40, 56), require_ratio=False).clone()
        after = m(x, res_out=(40, 56), require_ratio=False).clone()
        fresh = importlib.import_module("models.FastTransformer.model").TransformerModel().to(DEV).eval()
        fresh.load_state_dict(opt.ema_state_dict(m))
        want = fresh(x, res_out=(40, 56), require_ratio=False)
    assert torch.equal(inside, want)
    assert torch.equal(after, before) and not torch.equal(inside, before)


# ---- 6. two ranks on one GPU ----
def test_two_ranks_hold_the_same_average(tmp_path):
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_ema_dp_worker.py")
    outfile = str(tmp_path / "ema_dp")
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
    assert r0["updates"] == r1["updates"] == 2 and r0["stats"] == r1["stats"] and r0["stats"]["skipped"] == 1
    assert r0["ema"].keys() == r1["ema"].keys() == r0["params"].keys()
    for k in r0["ema"]:
        assert torch.equal(r0["ema"][k], r1["ema"][k]), k
        assert torch.equal(r0["params"][k], r1["params"][k]), k
        assert not torch.isnan(r0["ema"][k]).any(), k
    assert any(not torch.equal(r0["ema"][k], r0["params"][k]) for k in r0["ema"])
