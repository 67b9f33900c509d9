"""Validation on the MI355X: `harness.evaluate` against a manual B = 1 loop, and `train.py --val_dir / --ema_decay / --keep_best`
end to end.  Four synthetic 64 x 80 PNGs per directory under the pairs 32x40:64x80 (x2) and 16x20:64x80 (x4): eight samples.
Everything compared is equal floats / `torch.equal`: the driver runs are `--deterministic`, and `evaluate` is the same kernels on
the same inputs whichever way it is reached."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from transformerupscaler_amd import data, engine, harness, metrics, ops
from transformerupscaler_amd.autograd import l1_loss, resize_aa
from transformerupscaler_amd.weights import deterministic_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = "32x40:64x80,16x20:64x80"
SEED = 3
NAMES = ("l1", "mse", "psnr", "ssim")


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    ops.deterministic = False
    ops.release_det_slabs()


def _write_images(d, n, first=0, hw=(64, 80)):
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    yy, xx = np.mgrid[0:hw[0], 0:hw[1]].astype(np.float64)
    for i in range(first, first + n):
        rng = np.random.RandomState(i)
        planes = [127 + 90 * np.sin(yy / (5 + c + i) + c) * np.cos(xx / (7 + 2 * c - i) + i) + rng.normal(0, 6, hw) for c in range(3)]
        Image.fromarray(np.clip(np.stack(planes, -1), 0, 255).astype(np.uint8)).save(os.path.join(d, f"img_{i:02d}.png"))


def _model(sd=None):
    m = importlib.import_module("models.FastTransformer.model").TransformerModel()
    if sd is None:
        m.load_state_dict(deterministic_state_dict(0), strict=False)
    else:
        m.load_state_dict(sd)
    return m.to(DEV)


# ---- 1. evaluate against a manual loop ----
def test_evaluate_equals_a_manual_loop(tmp_path):
    _write_images(str(tmp_path), 4)
    ds = data.PairDataset(str(tmp_path), data.parse_pairs(PAIRS), device=DEV)
    assert len(ds) == 8
    # the precondition of group = True being bit-equal: a batch of four stays on the small-launch route of the transformer blocks
    assert 4 * (32 // 8) * (40 // 8) < engine.STREAM_MIN_WINDOWS
    model = _model().eval()
    want = {k: [] for k in NAMES}
    with torch.no_grad():
        for i in range(len(ds)):
            lr, hr = ds[i]
            lr, hr = lr.unsqueeze(0), hr.unsqueeze(0)
            out = model(lr, res_out=(64, 80), require_ratio=False)
            if tuple(out.shape[2:]) != (64, 80):
                out = resize_aa(out, (64, 80))
            q = metrics.quality(out, hr)
            want["l1"].append(l1_loss(out, hr).double().item())
            for k in NAMES[1:]:
                want[k].append(q[k].item())
    for mode, group in (("train", False), ("eval", True)):
        model.train(mode == "train")
        calls = model._dropout_calls
        got = harness.evaluate(model, ds, group=group)
        assert model.training == (mode == "train") and model._dropout_calls == calls          # restored; no dropout call
        assert set(got) == {"samples", "l1", "mse", "psnr", "ssim", "per_pair", "per_sample"} and got["samples"] == 8
        for k in NAMES:
            assert got["per_sample"][k] == want[k], (group, k)
            assert got[k] == sum(want[k][1:], want[k][0]) / 8, (group, k)                     # the mean in sample order
        assert list(got["per_pair"]) == ["32x40:64x80", "16x20:64x80"]
        for j, label in enumerate(got["per_pair"]):
            assert got["per_pair"][label]["samples"] == 4
            for k in NAMES:
                vals = want[k][j::2]
                assert got["per_pair"][label][k] == sum(vals[1:], vals[0]) / 4, (label, k)
    assert got["per_pair"]["32x40:64x80"]["psnr"] != got["per_pair"]["16x20:64x80"]["psnr"] and 0 < got["ssim"] < 1
    some = harness.evaluate(model, ds, indices=[5, 2, 7], batch_size=2)
    assert some["samples"] == 3 and all(some["per_sample"][k] == [want[k][i] for i in (5, 2, 7)] for k in NAMES)


# ---- 2. the driver ----
def _train(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py")] + args, cwd=cwd, env=env, capture_output=True, text=True,
                       timeout=600)
    return r.returncode, r.stdout + r.stderr


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Driver runs on the same four training images, shared by the tests below: `full` (two epochs with validation, the average,
    --val_both and --keep_best), `plain` (no new flag), `half` + `resumed` (one epoch, then the second from its checkpoint)."""
    tmp = tmp_path_factory.mktemp("validate")
    images, val = str(tmp / "train"), str(tmp / "val")
    _write_images(images, 4)
    _write_images(val, 4, first=10)
    common = ["--data_dir", images, "--pairs", PAIRS, "--batch_size", "4", "--deterministic", "--seed", str(SEED)]
    new = ["--val_dir", val, "--ema_decay", "0.9", "--save_optimizer"]
    out = {"val": val, "tmp": tmp, "common": common}
    for name, extra in (("full", new + ["--epochs", "2", "--val_both", "--keep_best", "psnr"]), ("plain", ["--epochs", "2"]),
                        ("half", new + ["--epochs", "1"]), ("resumed", new + ["--epochs", "2"])):
        ck = str(tmp / ("ck_resume" if name in ("half", "resumed") else f"ck_{name}"))
        rec = str(tmp / f"{name}.json")
        code, log = _train(common + extra + ["--checkpoint_dir", ck, "--json", rec], str(tmp))
        assert code == 0, log
        out[name] = {"record": json.load(open(rec)), "log": log, "ck": ck}
    return out


def _load(path):
    return torch.load(path, map_location="cpu")


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_record_equals_evaluate_on_the_saved_weights(runs):
    full = runs["full"]
    rec, ck = full["record"], full["ck"]
    assert [(e["epoch"], e["weights"]) for e in rec["val"]] == [(1, "ema"), (1, "raw"), (2, "ema"), (2, "raw")]
    assert full["log"].count("Validation (ema, 8 samples)") == 2 and full["log"].count("Validation (raw, 8 samples)") == 2
    ds = data.PairDataset(runs["val"], data.parse_pairs(PAIRS), device=DEV)
    with ops.deterministic_mode(True):
        for e in rec["val"]:
            assert set(e) == {"epoch", "weights", "l1", "mse", "psnr", "ssim", "per_pair", "seconds"} and e["seconds"] > 0
            sub = "ema" if e["weights"] == "ema" else ""
            got = harness.evaluate(_model(_load(os.path.join(ck, sub, f"model_epoch_{e['epoch']}.pth"))), ds)
            for k in NAMES:
                assert e[k] == got[k], (e["epoch"], e["weights"], k)
            assert e["per_pair"] == got["per_pair"]
    assert rec["val"][2]["psnr"] != rec["val"][3]["psnr"]                     # the average is not the raw weights
    assert rec["ema"] == {"decay": 0.9, "warmup": False, "updates": 4}
    assert not _same(_load(os.path.join(ck, "ema", "model_epoch_2.pth")), _load(os.path.join(ck, "model_epoch_2.pth")))


def test_raw_weights_do_not_depend_on_the_new_flags(runs):
    a = _load(os.path.join(runs["full"]["ck"], "model_epoch_2.pth"))
    b = _load(os.path.join(runs["plain"]["ck"], "model_epoch_2.pth"))
    assert _same(a, b)
    assert [s["loss"] for s in runs["full"]["record"]["steps"]] == [s["loss"] for s in runs["plain"]["record"]["steps"]]
    rec = runs["plain"]["record"]                                             # no new flag: the record and the lines of before
    assert set(rec) == {"model", "world", "samples", "resumed_from_epoch", "steps", "epochs", "checkpoints"}
    assert all(set(e) == {"epoch", "step", "loss"} for e in rec["steps"])
    assert "Validation" not in runs["plain"]["log"] and "EMA" not in runs["plain"]["log"]
    assert sorted(os.listdir(runs["plain"]["ck"])) == ["model_epoch_1.pth", "model_epoch_2.pth"]


def test_resumed_run_continues_the_average(runs):
    assert "Resuming from epoch 1" in runs["resumed"]["log"] and "restarts from the loaded weights" not in runs["resumed"]["log"]
    for sub in ("", "ema"):
        a = _load(os.path.join(runs["full"]["ck"], sub, "model_epoch_2.pth"))
        b = _load(os.path.join(runs["resumed"]["ck"], sub, "model_epoch_2.pth"))
        assert _same(a, b), sub
    assert runs["resumed"]["record"]["val"][0] | {"seconds": 0} == runs["full"]["record"]["val"][2] | {"seconds": 0}
    assert runs["resumed"]["record"]["ema"]["updates"] == 4
    assert _load(os.path.join(runs["resumed"]["ck"], "ema", "ema_epoch_2.pt"))["updates"] == 4


def test_keep_best_leaves_the_file_the_record_names(runs):
    rec, ck = runs["full"]["record"], runs["full"]["ck"]
    best = rec["best"]
    scored = {e["epoch"]: e["psnr"] for e in rec["val"] if e["weights"] == "ema"}
    want = max(scored, key=lambda ep: (scored[ep], -ep))                      # the first epoch that reached the maximum
    assert best["epoch"] == want and best["value"] == scored[want] and best["metric"] == "psnr" and best["weights"] == "ema"
    assert os.listdir(os.path.join(ck, "best")) == [f"model_epoch_{want}.pth"]
    assert _same(_load(os.path.join(ck, "best", f"model_epoch_{want}.pth")), _load(os.path.join(ck, "ema", f"model_epoch_{want}.pth")))


# ---- 3. two ranks on one GPU ----
def test_two_ranks_report_the_single_process_validation(runs, tmp_path):
    """--lr 0 keeps the weights at their seeded initial values on every rank, so that what is compared is the validation alone:
    sample k scored by rank k % 2, one all_reduce, against `harness.evaluate` in this process on the same initial weights."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_validate_dp_worker.py")
    rec = str(tmp_path / "dp.json")
    argv = runs["common"] + ["--val_dir", runs["val"], "--ema_decay", "0.9", "--epochs", "1", "--lr", "0", "--checkpoint_interval", "1000",
                             "--checkpoint_dir", str(tmp_path / "ck"), "--json", rec]
    rdzv = "file://" + str(tmp_path / "rdzv")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    procs = [subprocess.Popen([sys.executable, worker, str(r), "2", rdzv, "--"] + argv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True, env=env, cwd=str(tmp_path)) for r in range(2)]
    try:
        outs = [p.communicate(timeout=420)[0] for p in procs]
    except subprocess.TimeoutExpired:
        for p in procs:
            p.kill()
        pytest.fail("DP workers stalled:\n" + "\n-----\n".join(p.communicate()[0] for p in procs))
    assert all(p.returncode == 0 for p in procs), outs
    got = json.load(open(rec))
    assert got["world"] == 2 and len(got["val"]) == 1 and got["val"][0]["weights"] == "ema"
    torch.manual_seed(SEED)                                                   # the driver's initial weights
    model = importlib.import_module("models.FastTransformer.model").TransformerModel().to(DEV)
    ds = data.PairDataset(runs["val"], data.parse_pairs(PAIRS), device=DEV)
    with ops.deterministic_mode(True):
        want = harness.evaluate(model, ds)
    for k in NAMES:
        assert got["val"][0][k] == want[k], k
    assert got["val"][0]["per_pair"] == want["per_pair"]
