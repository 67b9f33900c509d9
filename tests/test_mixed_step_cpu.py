"""CPU checks of the mixed-scale training step: the `tup_grad_accumulate` entry through header / binding / library, the grouping
plan of `harness.train_step_samples` as a pure function, `data.PairDataset`'s sample plan, train.py's parser, the fixture
tests/golden/train_mixed_step.npz against the CPU oracle's per-sample loop (fp32), and the absence of network code."""
import ast
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fast_transformer_oracle as O
from _abi import ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- ABI ----
def test_grad_accumulate_is_declared_bound_and_exported():
    from transformerupscaler_amd import _lib
    header = open(os.path.join(ROOT, "include", "tupscale_hip.h")).read()
    assert re.search(r"int tup_grad_accumulate\(const void\* segs, const int\* chunks, int nchunks, void\* stream\);", header)
    assert _lib.SIGNATURES["tup_grad_accumulate"] == [_lib.P, _lib.P, _lib.I, _lib.P]
    assert _lib.ABI_VERSION == ABI
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "tup_grad_accumulate")
    assert lib.tup_abi_version() == ABI
    assert _lib.load() is not None                      # every bound symbol resolves
    guard = open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", "check_resources.py")).read()
    assert '("grad_accumulate.hip", ["grad_accumulate_kernel"])' in guard


def test_segment_record_matches_the_kernel_struct():
    from transformerupscaler_amd import accumulate
    assert accumulate._REC.size == 32 and accumulate._CHUNK == 4096
    src = open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", "grad_accumulate.hip")).read()
    assert "sizeof(AccSeg) == 32" in src and "ACC_CHUNK = 4096" in src
    assert "atomic" not in src.split("#include")[1]     # every element has one writer


# ---- grouping ----
def test_plan_groups_order_and_weights():
    from transformerupscaler_amd.harness import plan_groups
    a, b, c = ("a",), ("b",), ("c",)
    plan = plan_groups([a, b, a, c, b, a])
    assert [idx for idx, _ in plan] == [[0, 2, 5], [1, 4], [3]]              # first occurrence, members in list order
    assert [w for _, w in plan] == [3 / 6, 2 / 6, 1 / 6]
    assert abs(sum(w for _, w in plan) - 1.0) < 1e-12
    plan = plan_groups([a, b, a, c], group=False)
    assert [idx for idx, _ in plan] == [[0], [1], [2], [3]]
    assert all(w == 1 * 1 / 4 for _, w in plan)                               # bit-equal to the parent loop's 1 / B
    # two ranks holding 3 + 1 samples of a global batch of 4: the reducer divides the sum over ranks by world
    p0 = plan_groups([a, a, b], world=2, b_global=4)
    p1 = plan_groups([c], world=2, b_global=4)
    assert [w for _, w in p0] == [2 * 2 / 4, 1 * 2 / 4] and [w for _, w in p1] == [1 * 2 / 4]
    assert abs((sum(w for _, w in p0) + sum(w for _, w in p1)) / 2 - 1.0) < 1e-12
    assert plan_groups([], world=2, b_global=3) == []                        # a rank without samples still takes part
    assert plan_groups([], group=False, world=2, b_global=3) == []
    assert plan_groups([a, a], world=2) == [([0, 1], 2 * 2 / 4)]             # default: every rank holds len(shapes)
    with pytest.raises(ValueError):
        plan_groups([a, a, a], world=1, b_global=2)
    with pytest.raises(ValueError):
        plan_groups([a], world=0)


def test_train_step_keeps_its_signature_and_samples_step_has_the_new_one():
    from transformerupscaler_amd import harness
    assert list(inspect.signature(harness.train_step).parameters) == ["model", "optimizer", "lr_batch", "hr_batch", "loss"]
    names = list(inspect.signature(harness.train_step_samples).parameters)
    assert names[:7] == ["model", "optimizer", "lr_list", "hr_list", "loss", "group", "accumulator"]
    sig = inspect.signature(harness.train_step_samples)
    assert sig.parameters["group"].default is True and sig.parameters["loss"].default is None
    assert sig.parameters["accumulator"].default is None


# ---- dataset ----
def _write_pngs(d, names, hw=(8, 8)):
    from PIL import Image
    for i, n in enumerate(names):
        Image.fromarray(np.full(hw + (3,), 10 * i, np.uint8)).save(os.path.join(d, n))


def test_pair_dataset_plan_and_length(tmp_path):
    import ab_test
    from transformerupscaler_amd import data
    assert ab_test.SCALE_PAIRS == data.SCALE_PAIRS and ab_test.MAX_SAMPLES == data.MAX_SAMPLES          # training and evaluation agree
    assert all(ab_test.sample_plan(n) == data.sample_plan(n) for n in (0, 1, 3, 20, 35))
    assert len(data.SCALE_PAIRS) == 10 and data.MAX_SAMPLES == 200
    _write_pngs(str(tmp_path), ["b.png", "a.PNG", "c.png"])
    (tmp_path / "notes.txt").write_text("x")
    (tmp_path / "d.jpg").write_text("x")
    ds = data.PairDataset(str(tmp_path), device="cpu")
    assert [os.path.basename(f) for f in ds.files] == ["a.PNG", "b.png", "c.png"]                  # sorted by name, .png only
    assert len(ds) == 30 and ds.plan[0] == (0, 0) and ds.plan[9] == (0, 9) and ds.plan[10] == (1, 0) and ds.plan[29] == (2, 9)
    assert ds.plan == data.sample_plan(3)
    assert len(data.sample_plan(20)) == 200 and len(data.sample_plan(35)) == 200                    # min(200, 10 * n_png)
    two = data.PairDataset(str(tmp_path), scale_pairs=data.parse_pairs("4x4:8x8, 2x3:6x9"), device="cpu")
    assert len(two) == 6 and two.plan[3] == (1, 1) and two.scale_pairs[1] == {"lr": (2, 3), "hr": (6, 9)}
    with pytest.raises(IndexError):
        two[6]
    # the LRU cache: bounded by bytes, one host decode per miss
    small = data.PairDataset(str(tmp_path), cache_bytes=2 * 8 * 8 * 3, device="cpu")
    for i in (0, 1, 0, 2, 0, 1):
        small.frame(i)
    assert small.decodes == 4 and list(small._cache) == [0, 1] and small._cached_bytes == 2 * 8 * 8 * 3


def test_pair_dataset_refuses_without_a_directory(tmp_path):
    from transformerupscaler_amd import data
    for bad in (None, ""):
        with pytest.raises(ValueError, match="data_dir"):
            data.PairDataset(bad)
    with pytest.raises(FileNotFoundError):
        data.PairDataset(str(tmp_path / "missing"))
    with pytest.raises(FileNotFoundError, match="no .png"):
        data.PairDataset(str(tmp_path))
    for bad in ("96x96", "96x96:192", "ax4:8x8", ""):
        with pytest.raises(ValueError):
            data.parse_pairs(bad)


# ---- driver surface ----
def test_train_parser_flags_and_defaults():
    import train
    a = train.build_parser().parse_args([])
    assert (a.data_dir, a.batch_size, a.epochs, a.lr, a.log_interval, a.checkpoint_interval) == (None, 6, 10, 1e-4, 1, 1)
    assert a.model == "FastTransformer" and a.checkpoint_dir is None and a.traceback is False
    assert (a.l1, a.mse, a.ssim) == (1.0, 0.0, 0.0) and train.pure_l1(a)
    assert a.deterministic is False and a.seed == 0 and a.max_steps is None and a.pairs is None and a.cache_gb == 2.0
    assert a.save_optimizer is False and a.no_group is False and a.json is None
    b = train.build_parser().parse_args(["--data_dir", "x", "--ssim", "0.5", "--no_group", "--deterministic", "--max_steps", "3",
                                         "--pairs", "8x8:16x16", "--traceback", "--save_optimizer", "--json", "r.json", "--seed", "4"])
    assert not train.pure_l1(b) and b.no_group and b.deterministic and b.max_steps == 3 and b.traceback and b.seed == 4


def test_train_refuses_without_data_dir():
    import train
    with pytest.raises(SystemExit) as e:
        train.run(train.build_parser().parse_args([]))
    assert "--data_dir is required" in str(e.value)


def test_epoch_batches_keep_the_partial_batch_and_follow_the_seed():
    import train
    g = torch.Generator().manual_seed(3)
    batches = train.epoch_batches(20, 6, g)
    assert [len(b) for b in batches] == [6, 6, 6, 2] and sorted(i for b in batches for i in b) == list(range(20))
    assert train.epoch_batches(20, 6, torch.Generator().manual_seed(3)) == batches
    assert train.epoch_batches(20, 6, g) != batches          # the next epoch of the same generator


def test_no_network_code_in_data_and_driver():
    banned = {"requests", "urllib", "urllib3", "socket", "http", "httpx", "aiohttp", "ftplib", "asyncio"}
    for rel in ("transformerupscaler_amd/data.py", "train.py"):
        tree = ast.parse(open(os.path.join(ROOT, rel)).read())
        for node in ast.walk(tree):
            mods = []
            if isinstance(node, ast.Import):
                mods = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                mods = [node.module or ""]
            for m in mods:
                assert m.split(".")[0] not in banned, (rel, m)
            if isinstance(node, ast.Attribute):
                assert node.attr not in ("urlopen", "urlretrieve", "create_connection"), (rel, node.attr)


# ---- the fixture against the oracle ----
def test_oracle_per_sample_loop_reproduces_the_fixture(golden_dir, det_sd):
    d = dict(np.load(os.path.join(golden_dir, "train_mixed_step.npz"), allow_pickle=False))
    n = len(d["scales"])
    assert n == 6 and sorted(set(d["scales"].tolist())) == [2, 3, 4, 6] and len(d["none_grads"]) == 0
    shapes = [(d[f"lr_u8_{i}"].shape, d[f"hr_u8_{i}"].shape) for i in range(n)]
    assert len(set(shapes)) < n                                               # two samples are equal-shaped
    leaf = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in det_sd.items()}
    losses, resized = [], 0
    for i in range(n):                                                        # train.py:119-133
        lr, hr = (torch.from_numpy(d[f"{k}_u8_{i}"]).float().div(255.0).unsqueeze(0) for k in ("lr", "hr"))      # ToTensor
        hw = tuple(hr.shape[2:])
        out = O.forward(leaf, lr, res_out=hw, require_ratio=False)
        assert out.shape[2] == lr.shape[2] * int(d["scales"][i])
        if tuple(out.shape[2:]) != hw:
            out = O.aa_resize(out, hw)
            resized += 1
        losses.append(F.l1_loss(out, hr))
    assert resized >= 1                                                       # one pair needs the Resize
    loss = sum(losses) / len(losses)
    loss.backward()
    assert abs(loss.item() - float(d["loss"])) < 1e-6
    assert np.abs(np.array([v.item() for v in losses]) - d["sample_losses"]).max() < 1e-6
    checked = 0
    for k, v in leaf.items():
        if not v.is_floating_point() or "gstat_" + k not in d:
            continue
        assert v.grad is not None, k
        st = d["gstat_" + k]
        gd = v.grad.double().flatten()
        assert abs(gd.norm().item() - st[1]) <= 1e-4 * max(1.0, st[1]), k
        assert np.abs(gd[torch.from_numpy(d["gidx_" + k])].float().numpy() - d["gval_" + k]).max() <= 1e-5 + 1e-4 * st[2], k
        checked += 1
    assert checked == 113
