"""CPU checks of the weight average of optim.Adam / optim.AdamW (``ema_decay``): the decay schedule as a pure function, the option's
refusals, a trajectory on CPU parameters (torch's step plus the three-op update) against an explicit loop, `state_dict()`
interchange with torch, `ema_state_dict`, `harness.ema_weights`, the `tup_adam_step_ema` entry through header / binding / library
with its record size, train.py's flag rules and the EMA checkpoint files.  Everything compared here is `torch.equal`: the update
``e = e + w * (p - e)`` is three rounded fp32 operations with ``w = fp32(1 - d_n)``, which the reference loops below spell out."""
import ctypes
import math
import os
import re
import struct

import pytest
import torch

from _abi import ABI          # tests/ is on sys.path (rootdir-less test modules)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def lerp3(e, p, w):
    """The kernel's three operations in torch, out of place."""
    d = p - e
    d = d * w
    return e + d


# ---- the schedule ----
def test_ema_decay_at():
    from transformerupscaler_amd.optim import ema_decay_at
    assert ema_decay_at(0, 0.999, True) == 0.1                                # (1 + 0) / (10 + 0)
    assert ema_decay_at(1, 0.999, True) == 2 / 11
    seq = [ema_decay_at(n, 0.9, True) for n in range(200)]
    assert all(a <= b for a, b in zip(seq, seq[1:])) and seq[0] == 0.1
    first = next(n for n, v in enumerate(seq) if v == 0.9)                    # (1 + n) / (10 + n) >= 0.9 from n = 80
    assert first == 80 and all(v == 0.9 for v in seq[first:])
    assert ema_decay_at(10 ** 9, 0.9999, True) == 0.9999
    assert all(ema_decay_at(n, 0.9, False) == 0.9 for n in (0, 1, 7, 10 ** 6))
    assert ema_decay_at(3, 0.0, True) == 0.0 and ema_decay_at(3, 0.0, False) == 0.0


@pytest.mark.parametrize("cls_name", ["Adam", "AdamW"])
def test_ema_decay_values_are_checked(cls_name):
    from transformerupscaler_amd import optim
    p = torch.nn.Parameter(torch.ones(5))
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            getattr(optim, cls_name)([p], lr=1e-3, ema_decay=bad)
    for ok in (0.0, 0.5, 0.9999):
        o = getattr(optim, cls_name)([p], lr=1e-3, ema_decay=ok)
        assert o.ema_decay == ok and o.ema_warmup is False and o.ema_updates == 0
    o = getattr(optim, cls_name)([p], lr=1e-3)
    assert o.ema_decay is None and o.ema_updates == 0


# ---- a trajectory on CPU parameters ----
@pytest.mark.parametrize("cls_name,wd,warmup", [("Adam", 0.0, False), ("Adam", 1e-2, True), ("AdamW", 1e-2, False)])
def test_cpu_trajectory_equals_the_three_op_loop(cls_name, wd, warmup):
    from transformerupscaler_amd import optim
    cls = getattr(optim, cls_name)
    g = torch.Generator().manual_seed(5)
    base = [torch.randn(s, generator=g) for s in ((7, 3), (33,), (4, 5, 2))]
    pa = [torch.nn.Parameter(b.clone()) for b in base]
    pb = [torch.nn.Parameter(b.clone()) for b in base]
    oa = cls(pa, lr=1e-2, weight_decay=wd, ema_decay=0.9, ema_warmup=warmup)
    ob = cls(pb, lr=1e-2, weight_decay=wd)
    avg = [None, None, None]                                                  # the reference: created at the first step, a copy from before
    for step in range(8):
        for i in range(3):
            if i == 2 and step in (0, 1, 2, 5):
                pa[i].grad = pb[i].grad = None
                continue
            gr = torch.randn(base[i].shape, generator=g)
            pa[i].grad, pb[i].grad = gr.clone(), gr.clone()
        for i in range(3):
            if avg[i] is None and pb[i].grad is not None:
                avg[i] = pb[i].detach().clone()
        oa.step()
        ob.step()
        w = f32(1.0 - optim.ema_decay_at(step, 0.9, warmup))                  # every step applies: update n is step n
        for i in range(3):
            if avg[i] is not None:                                            # with a gradient or without: the average moves
                avg[i] = lerp3(avg[i], pb[i].detach(), w)
        assert oa.ema_updates == step + 1
        for i in range(3):
            assert torch.equal(pa[i], pb[i]), (step, i)                       # the raw weights: the same optimizer without the option
            if avg[i] is None:
                assert pa[i] not in oa._ema
            else:
                assert torch.equal(oa._ema[pa[i]], avg[i]), (step, i)
    assert not torch.equal(oa._ema[pa[2]], pa[2].detach())
    # the average is not in the state: torch's keys, loadable in both directions
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa.keys() == sb.keys() and sa["state"].keys() == sb["state"].keys()
    for k in sa["state"]:
        assert set(sa["state"][k]) == {"step", "exp_avg", "exp_avg_sq"}
    assert [set(gr) for gr in sa["param_groups"]] == [set(gr) for gr in sb["param_groups"]]
    ref = getattr(torch.optim, cls_name)(pb, lr=1e-2, weight_decay=wd)
    ref.load_state_dict(sa)
    assert torch.equal(ref.state[pb[0]]["exp_avg"], oa.state[pa[0]]["exp_avg"])
    back = cls(pa, lr=1e-2, weight_decay=wd, ema_decay=0.9)
    back.load_state_dict(ref.state_dict())
    assert float(back.state[pa[0]]["step"]) == 8.0 and back.ema_updates == 0


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(3, 4)
        self.b = torch.nn.Linear(4, 2)
        self.frozen = torch.nn.Linear(2, 2)                                   # never stepped: no gradient reaches it
        self.register_buffer("index", torch.arange(6, dtype=torch.int64).reshape(2, 3))

    def forward(self, x):
        return self.b(self.a(x))


def _stepped_net(steps=3, **kw):
    from transformerupscaler_amd import optim
    torch.manual_seed(0)
    net = _Net()
    opt = optim.Adam(net.parameters(), lr=1e-2, ema_decay=0.9, **kw)
    g = torch.Generator().manual_seed(1)
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        net(torch.randn(5, 3, generator=g)).square().sum().backward()
        opt.step()
    return net, opt


def test_ema_state_dict_has_the_models_layout():
    net, opt = _stepped_net()
    sd, msd = opt.ema_state_dict(net), net.state_dict()
    assert list(sd) == list(msd)
    for k, p in net.named_parameters():
        if k.startswith("frozen."):
            assert p not in opt._ema and torch.equal(sd[k], p.detach())       # never stepped: its own value
        else:
            assert torch.equal(sd[k], opt._ema[p]) and not torch.equal(sd[k], p.detach())
        assert sd[k].data_ptr() != p.data_ptr() and sd[k].data_ptr() != opt._ema.get(p, p).data_ptr()          # copies
    assert sd["index"].dtype == torch.int64 and torch.equal(sd["index"], net.index) and sd["index"].data_ptr() != net.index.data_ptr()
    # ... and loads back: into a model, and into another optimizer's average
    other = _Net()
    other.load_state_dict(sd)
    net2, opt2 = _stepped_net(steps=1)
    opt2.load_ema_state_dict(net2, sd, updates=7)
    assert opt2.ema_updates == 7
    for k, p in net2.named_parameters():
        assert torch.equal(opt2._ema[p], sd[k])
    with pytest.raises(KeyError):
        opt2.load_ema_state_dict(net2, {k: v for k, v in sd.items() if k != "a.bias"})
    from transformerupscaler_amd import optim
    with pytest.raises(RuntimeError):
        optim.Adam(net.parameters(), lr=1e-2).ema_state_dict(net)


def test_ema_weights_exchanges_storage_and_restores():
    from transformerupscaler_amd import harness
    net, opt = _stepped_net()
    params = dict(net.named_parameters())
    raw_ptr = {k: p.data_ptr() for k, p in params.items()}
    raw_val = {k: p.detach().clone() for k, p in params.items()}
    ema_ptr = {k: opt._ema[p].data_ptr() for k, p in params.items() if p in opt._ema}
    ema_val = {k: opt._ema[p].clone() for k, p in params.items() if p in opt._ema}
    assert set(ema_ptr) == {"a.weight", "a.bias", "b.weight", "b.bias"}

    def check_raw():
        for k, p in params.items():
            assert p.data_ptr() == raw_ptr[k] and torch.equal(p.detach(), raw_val[k]), k
            if k in ema_ptr:
                assert opt._ema[p].data_ptr() == ema_ptr[k] and torch.equal(opt._ema[p], ema_val[k]), k

    x = torch.randn(2, 3, generator=torch.Generator().manual_seed(9))
    y_raw = net(x).detach().clone()
    with harness.ema_weights(net, opt) as m:
        assert m is net
        for k, p in params.items():
            if k in ema_ptr:
                assert p.data_ptr() == ema_ptr[k] and torch.equal(p.detach(), ema_val[k]), k          # the buffer itself: no copy
                assert isinstance(p, torch.nn.Parameter) and p.requires_grad
            else:
                assert p.data_ptr() == raw_ptr[k]
        y_ema = net(x).detach().clone()
        fresh = _Net()
        fresh.load_state_dict({k: ema_val.get(k, v) for k, v in net.state_dict().items()})
        assert torch.equal(y_ema, fresh(x)) and not torch.equal(y_ema, y_raw)
        with pytest.raises(RuntimeError, match="nest"):
            with harness.ema_weights(net, opt):
                pass
        for p in params.values():
            p.grad = torch.ones_like(p)
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.step()
    check_raw()
    assert torch.equal(net(x), y_raw)
    with pytest.raises(KeyError):                                              # an exception inside: restored all the same
        with harness.ema_weights(net, opt):
            raise KeyError("inside")
    check_raw()
    opt.step()                                                                 # and the optimizer steps again
    from transformerupscaler_amd import optim
    with pytest.raises(RuntimeError):
        with harness.ema_weights(net, optim.Adam(net.parameters(), lr=1e-2)):
            pass


def test_torch_arm_runs_the_same_average():
    """harness.use_torch_adam: torch's step plus the three-op update; on CPU parameters the fused class falls through to exactly that."""
    from transformerupscaler_amd import harness, optim
    runs = []
    for arm in (False, True):
        harness.use_torch_adam = arm
        try:
            torch.manual_seed(0)
            net = _Net()
            opt = harness.make_ema_optimizer(net, 0.9, True, lr=1e-2, weight_decay=1e-2, decoupled=True)
            assert isinstance(opt, torch.optim.AdamW) and isinstance(opt, optim.AdamW) != arm
        finally:
            harness.use_torch_adam = False
        g = torch.Generator().manual_seed(1)
        for _ in range(4):
            opt.zero_grad(set_to_none=True)
            net(torch.randn(5, 3, generator=g)).square().sum().backward()
            opt.step()
        assert opt.ema_updates == 4
        runs.append(opt.ema_state_dict(net))
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0])
    with pytest.raises(ValueError):
        harness.make_ema_optimizer(_Net(), None)
    with pytest.raises(TypeError):
        harness.make_ema_optimizer(_Net(), 0.9, momentum=0.5)


# ---- ABI ----
def test_ema_entry_is_declared_bound_and_exported():
    from transformerupscaler_amd import _lib, optim
    header = open(os.path.join(ROOT, "include", "tupscale_hip.h")).read()
    assert re.search(r"int tup_adam_step_ema\(const void\* segs, const int\* chunks, int nchunks, const void\* guard, void\* stream\);", header)
    P, I = _lib.P, _lib.I
    assert _lib.SIGNATURES["tup_adam_step_ema"] == [P, P, I, P, P]
    assert _lib.ABI_VERSION == ABI
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "tup_adam_step_ema") and lib.tup_abi_version() == ABI
    assert _lib.load() is not None
    src = open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", "step_guard.hip")).read()
    assert optim._REC_EMA.size == 88 and "sizeof(AdamEmaSeg) == 88" in src
    assert optim._REC.size == 64 and optim._REC_GUARDED.size == 72            # the two existing records stay
    # the fields where the kernel reads them: e at byte 72, ema_w at 80, form at 84; the first 72 bytes are AdamWSeg's
    packed = optim._REC_EMA.pack(1, 2, 3, 4, 5, 0.5, 0.25, 0.999, 0.1, 0.001, 1e-8, 0.01, 0.99, 0xABCDEF, 0.125, 1)
    assert packed[:72] == optim._REC_GUARDED.pack(1, 2, 3, 4, 5, 0.5, 0.25, 0.999, 0.1, 0.001, 1e-8, 0.01, 0.99)
    assert int.from_bytes(packed[72:80], "little") == 0xABCDEF
    assert struct.unpack("<f", packed[80:84])[0] == 0.125 and int.from_bytes(packed[84:88], "little") == 1
    guard = open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", "check_resources.py")).read()
    assert '("step_guard.hip", ["adam_ema_kernel"])' in guard


# ---- the driver's argument rules ----
def _refused(argv, monkeypatch):
    import train
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "")
    with pytest.raises(SystemExit) as e:
        train.main(argv)
    assert isinstance(e.value.code, str)                                      # a message, not a status: nothing ran
    return e.value.code


def test_train_py_ema_and_validation_argument_rules(tmp_path, monkeypatch):
    import train
    d = str(tmp_path)
    for extra in (["--val_interval", "2"], ["--val_pairs", "8x8:16x16"], ["--val_images", "3"], ["--val_both"], ["--keep_best", "psnr"],
                  ["--val_both", "--ema_decay", "0.9"]):
        assert "need --val_dir" in _refused(["--data_dir", d] + extra, monkeypatch), extra
    for extra in (["--val_both"], ["--ema_warmup"]):
        assert "need --ema_decay" in _refused(["--data_dir", d, "--val_dir", d] + extra, monkeypatch), extra
    assert "need --ema_decay" in _refused(["--data_dir", d, "--ema_warmup"], monkeypatch)
    for bad in ("1.0", "-0.5", "nan"):
        assert "--ema_decay" in _refused(["--data_dir", d, "--ema_decay", bad], monkeypatch)
    assert "--val_interval" in _refused(["--data_dir", d, "--val_dir", d, "--val_interval", "0"], monkeypatch)
    assert "--val_images" in _refused(["--data_dir", d, "--val_dir", d, "--val_images", "0"], monkeypatch)
    assert "--val_dir" in _refused(["--data_dir", d, "--val_dir", os.path.join(d, "missing")], monkeypatch)
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--keep_best", "loss"])
    a = train.build_parser().parse_args([])
    assert (a.ema_decay, a.ema_warmup, a.val_dir, a.val_interval, a.val_pairs, a.val_images, a.val_both, a.keep_best) \
        == (None, False, None, 1, None, None, False, None)
    assert train.val_options(a) is False                                      # without the flags: today's program
    b = train.build_parser().parse_args(["--val_dir", d, "--ema_decay", "0.99", "--ema_warmup", "--val_both", "--keep_best", "ssim"])
    assert train.val_options(b) is True


# ---- checkpoints ----
def test_ema_checkpoint_files_round_trip(tmp_path):
    from tools.utils import get_latest_checkpoint
    from transformerupscaler_amd import harness
    net, opt = _stepped_net(steps=3, ema_warmup=True)
    ck = str(tmp_path / "ck")
    path = harness.save_checkpoint(net, ck, 4, optimizer=opt, ema=opt)
    assert path == os.path.join(ck, "model_epoch_4.pth")
    assert sorted(os.listdir(ck)) == ["ema", "model_epoch_4.pth", "optim_epoch_4.pt"]
    assert sorted(os.listdir(os.path.join(ck, "ema"))) == ["ema_epoch_4.pt", "model_epoch_4.pth"]
    assert get_latest_checkpoint(ck) == (path, 4)                             # the raw file: the sub-directory is not looked into
    assert get_latest_checkpoint(os.path.join(ck, "ema")) == (os.path.join(ck, "ema", "model_epoch_4.pth"), 4)
    side = torch.load(os.path.join(ck, "ema", "ema_epoch_4.pt"))
    assert side == {"updates": 3, "decay": 0.9, "warmup": True}
    saved = torch.load(os.path.join(ck, "ema", "model_epoch_4.pth"))
    want = opt.ema_state_dict(net)
    assert list(saved) == list(net.state_dict()) and all(torch.equal(saved[k], want[k]) for k in want)
    _Net().load_state_dict(saved)                                             # the weight file's format: a strict load
    # resume: weights, Adam's state and the average
    net2, opt2 = _stepped_net(steps=0, ema_warmup=True)
    assert harness.load_latest_checkpoint(net2, ck, optimizer=opt2, map_location="cpu") == 4
    assert harness.load_ema_checkpoint(net2, ck, 4, opt2, map_location="cpu") == side
    assert opt2.ema_updates == 3
    got = opt2.ema_state_dict(net2)
    assert all(torch.equal(got[k], want[k]) for k in want)
    for n in (net, net2):                                                     # ... and both continue alike
        for p in n.parameters():
            p.grad = torch.full_like(p, 0.25)
    opt.step()
    opt2.step()
    a, b = opt.ema_state_dict(net), opt2.ema_state_dict(net2)
    assert all(torch.equal(a[k], b[k]) for k in a) and opt.ema_updates == opt2.ema_updates == 4
    assert harness.load_ema_checkpoint(net2, ck, 5, opt2) is None             # absent: nothing loaded
    harness.save_ema_checkpoint(net, ck, 6, opt, extra={"dropout_calls": 12})
    assert torch.load(os.path.join(ck, "ema", "ema_epoch_6.pt")) == {"updates": 4, "decay": 0.9, "warmup": True, "dropout_calls": 12}
    # without `ema` the directory is what it was before
    harness.save_checkpoint(net, str(tmp_path / "plain"), 1)
    assert os.listdir(str(tmp_path / "plain")) == ["model_epoch_1.pth"]
    assert math.isfinite(sum(v.double().sum().item() for v in saved.values()))
