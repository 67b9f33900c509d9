"""CPU checks of the guarded optimizer step: the three `csrc/step_guard.hip` entries through header / binding / library, the host
record formats against the kernel's `static_assert`ed struct sizes, train.py's learning-rate schedule as a pure function, the
parser's defaults, and the refusals of the guard options."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from _abi import ABI          # tests/ is on sys.path (rootdir-less test modules)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "tup_grad_sumsq_partial": r"int tup_grad_sumsq_partial\(const void\* segs, const int\* chunks, int nchunks, double\* partials, void\* stream\);",
    "tup_grad_guard_finish": r"int tup_grad_guard_finish\(const double\* partials, int npartials, double max_norm, int skip_nonfinite, "
                             r"void\* guard, void\* stream\);",
    "tup_adam_step_guarded": r"int tup_adam_step_guarded\(const void\* segs, const int\* chunks, int nchunks, const void\* guard, void\* stream\);",
}


# ---- ABI ----
def test_step_guard_entries_are_declared_bound_and_exported():
    from transformerupscaler_amd import _lib
    header = open(os.path.join(ROOT, "include", "tupscale_hip.h")).read()
    for name, decl in ENTRIES.items():
        assert re.search(decl, header), name
        assert name in _lib.SIGNATURES, name
    P, I = _lib.P, _lib.I
    assert _lib.SIGNATURES["tup_grad_sumsq_partial"] == [P, P, I, P, P]
    assert _lib.SIGNATURES["tup_grad_guard_finish"] == [P, I, ctypes.c_double, I, P, P]
    assert _lib.SIGNATURES["tup_adam_step_guarded"] == [P, P, I, P, P]
    assert _lib.SIGNATURES["tup_adam_step"] == [P, P, I, P]              # the unguarded entry is untouched
    assert _lib.ABI_VERSION == ABI
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
    assert lib.tup_abi_version() == ABI
    assert _lib.load() is not None                                       # every bound symbol resolves
    guard = open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", "check_resources.py")).read()
    assert '("step_guard.hip", ["grad_sumsq_kernel", "guard_finish_kernel", "adam_guarded_kernel"])' in guard


def test_host_records_match_the_kernel_structs():
    from transformerupscaler_amd import optim
    src = open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", "step_guard.hip")).read()
    assert optim._REC_NORM.size == 16 and "sizeof(NormSeg) == 16" in src
    assert optim._REC_GUARD.size == 64 and "sizeof(GuardRec) == 64" in src
    assert optim._REC_GUARDED.size == 72 and "sizeof(AdamWSeg) == 72" in src
    assert optim._CHUNK == 4096 and "GUARD_CHUNK = 4096" in src
    old = open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", "pack_plan.hip")).read()
    assert optim._REC.size == 64 and "sizeof(AdamSeg) == 64" in old      # tup_adam_step's record stays
    assert "atomic" not in src.split("#include")[1].lower()             # fixed-order sums only
    # the guard record's fields where the host reads them: apply is word 5 (bytes 20..24), the fp32 norm word 6
    packed = optim._REC_GUARD.pack(4.0, 2.0, 0.5, 1, 2.0, 1, 7, 6, 3, 1)
    assert int.from_bytes(packed[20:24], "little") == 1
    assert torch.frombuffer(bytearray(packed), dtype=torch.float32)[6].item() == 2.0


# ---- learning-rate schedule ----
def test_lr_at_warmup_cosine_and_resume():
    import train
    base, warm, total, lr_min = 2e-4, 5, 40, 1e-6
    assert train.lr_at(0, base, warm, "constant") == base / warm                     # first warm-up step
    assert train.lr_at(warm - 1, base, warm, "constant") == base                     # last warm-up step
    assert train.lr_at(warm, base, warm, "constant") == base and train.lr_at(10 ** 6, base, warm, "constant") == base
    assert train.lr_at(0, base) == base and train.lr_at(17, base) == base            # defaults: the constant rate of --lr
    seq = [train.lr_at(k, base, warm, "cosine", total, lr_min) for k in range(total)]
    assert seq[0] == base / warm and seq[warm - 1] == base and seq[warm] == base
    assert seq[-1] == lr_min                                                          # the cosine ends at lr_min
    assert all(a < b for a, b in zip(seq[:warm - 1], seq[1:warm]))                    # rising inside the warm-up
    assert all(a > b for a, b in zip(seq[warm:-1], seq[warm + 1:]))                   # falling inside the cosine
    assert all(lr_min <= v <= base for v in seq)
    mid = warm + (total - 1 - warm) / 2
    assert abs(train.lr_at(int(mid), base, warm, "cosine", total, lr_min) - (lr_min + 0.5 * (base - lr_min))) < 1e-12
    # a resumed run (epochs_trained * steps_per_epoch as offset) continues the sequence
    steps_per_epoch = 8
    resumed = [train.lr_at(2 * steps_per_epoch + s, base, warm, "cosine", total, lr_min) for s in range(steps_per_epoch)]
    assert resumed == seq[16:24]
    assert train.lr_at(total + 3, base, warm, "cosine", total, lr_min) == lr_min      # past the end: stays there
    assert train.lr_at(3, base, 0, "cosine", 1, lr_min) == lr_min                     # a run of one step
    with pytest.raises(ValueError):
        train.lr_at(9, base, warm, "cosine")                                          # no total
    with pytest.raises(ValueError):
        train.lr_at(9, base, warm, "linear", total)
    assert list(inspect.signature(train.lr_at).parameters) == ["k", "base", "warmup", "schedule", "total", "lr_min"]


def test_parser_defaults_leave_every_new_option_off():
    import train
    a = train.build_parser().parse_args([])
    assert a.weight_decay == 0.0 and a.adamw is False and a.clip_grad_norm is None and a.skip_nonfinite is False
    assert a.warmup_steps == 0 and a.lr_schedule == "constant" and a.lr_min == 0.0
    assert not train.guard_options(a)
    b = train.build_parser().parse_args(["--weight_decay", "0.01", "--adamw", "--clip_grad_norm", "1.5", "--skip_nonfinite",
                                         "--warmup_steps", "3", "--lr_schedule", "cosine", "--lr_min", "1e-6"])
    assert (b.weight_decay, b.adamw, b.clip_grad_norm, b.skip_nonfinite) == (0.01, True, 1.5, True)
    assert (b.warmup_steps, b.lr_schedule, b.lr_min) == (3, "cosine", 1e-6) and train.guard_options(b)
    for one in (["--clip_grad_norm", "1"], ["--skip_nonfinite"], ["--warmup_steps", "1"], ["--adamw"], ["--weight_decay", "0.1"]):
        assert train.guard_options(train.build_parser().parse_args(one)), one
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--lr_schedule", "step"])


# ---- refusals ----
@pytest.mark.parametrize("cls_name", ["Adam", "AdamW"])
@pytest.mark.parametrize("kw", [dict(max_grad_norm=1.0), dict(skip_nonfinite=True)])
def test_guard_options_on_cpu_parameters_raise(cls_name, kw):
    from transformerupscaler_amd import optim
    p = torch.nn.Parameter(torch.ones(5))
    with pytest.raises(ValueError):
        opt = getattr(optim, cls_name)([p], lr=1e-3, **kw)
        p.grad = torch.ones(5)
        opt.step()


def test_guard_option_values_and_surface():
    from transformerupscaler_amd import harness, optim
    p = torch.nn.Parameter(torch.ones(5))
    for cls in (optim.Adam, optim.AdamW):
        with pytest.raises(ValueError):
            cls([p], lr=1e-3, max_grad_norm=-1.0)
        with pytest.raises(ValueError):
            cls([p], lr=1e-3, max_grad_norm=float("nan"))
        with pytest.raises(ValueError):
            cls([torch.nn.Parameter(torch.ones(5, dtype=torch.float64))], lr=1e-3, skip_nonfinite=True)
    assert issubclass(optim.Adam, torch.optim.Adam) and issubclass(optim.AdamW, torch.optim.AdamW)
    # without the options the classes construct on anything torch's do, and the options are attributes, not group keys
    for cls, ref in ((optim.Adam, torch.optim.Adam), (optim.AdamW, torch.optim.AdamW)):
        o = cls([p], lr=1e-3, weight_decay=0.01)
        assert o.max_grad_norm is None and o.skip_nonfinite is False and o.grad_norm is None
        assert o.guard_stats() == {"steps": 0, "applied": 0, "clipped": 0, "skipped": 0}
        assert set(o.state_dict()["param_groups"][0]) == set(ref([p], lr=1e-3, weight_decay=0.01).state_dict()["param_groups"][0])
    names = list(inspect.signature(harness.make_optimizer).parameters)
    assert names == ["model", "lr", "weight_decay", "decoupled", "max_grad_norm", "skip_nonfinite"]
    sig = inspect.signature(harness.make_optimizer).parameters
    assert (sig["weight_decay"].default, sig["decoupled"].default, sig["max_grad_norm"].default, sig["skip_nonfinite"].default) \
        == (0.0, False, None, False)
    # a CPU step without the options still runs torch's own step (the documented per-group fall-through)
    q = torch.nn.Parameter(torch.ones(5))
    r = torch.nn.Parameter(torch.ones(5))
    q.grad, r.grad = torch.full((5,), 0.5), torch.full((5,), 0.5)
    optim.AdamW([q], lr=1e-2, weight_decay=0.1).step()
    torch.optim.AdamW([r], lr=1e-2, weight_decay=0.1).step()
    assert torch.equal(q, r) and not math.isnan(q.sum().item())
