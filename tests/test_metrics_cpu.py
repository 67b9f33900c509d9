"""CPU checks of the quality-metric feature: the float64 SSIM / PSNR restatement the GPU tests compare against
(tests/_metrics_ref.py), the A/B driver's host logic (ab_test.py: sample plan, Resize(int) size rule, skip rule, CLI), and the
new C-ABI entries of csrc/metrics.hip."""
import os
import re

import numpy as np
import pytest

import ab_test
import _metrics_ref as R          # tests/ is on sys.path (rootdir-less test modules)
from _abi import ABI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_box_filter_equals_direct_7x7_loop():
    rng = np.random.default_rng(0)
    img = rng.random((13, 29))
    got = R.box7(img)
    ref = np.array([[img[i:i + 7, j:j + 7].mean() for j in range(29 - 6)] for i in range(13 - 6)])
    assert got.shape == (7, 23)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-14)


def test_identical_inputs_give_ssim_one_and_psnr_inf():
    img = np.random.default_rng(1).random((20, 31, 3))
    assert abs(R.ssim(img, img, 1.0) - 1.0) < 1e-12
    assert R.psnr(img, img, 1.0) == float("inf")
    assert R.mse(img, img) == 0.0


def test_ssim_is_symmetric_and_below_one_for_different_images():
    rng = np.random.default_rng(2)
    x = rng.random((16, 24, 3))
    y = np.clip(x + rng.normal(0, 0.05, x.shape), 0, 1)
    assert R.ssim(x, y, 1.0) == pytest.approx(R.ssim(y, x, 1.0), abs=1e-14)
    assert R.ssim(x, y, 1.0) < 0.999
    assert R.psnr(x, y, 1.0) == pytest.approx(10 * np.log10(1.0 / np.mean((x - y) ** 2)))


def test_restatement_rejects_images_smaller_than_the_window():
    with pytest.raises(ValueError):
        R.ssim_channel(np.zeros((6, 10)), np.zeros((6, 10)), 1.0)


def test_sample_plan_order_pairs_and_count(tmp_path):
    for name in ("b.png", "a.PNG", "c.jpg", "c.png"):
        (tmp_path / name).write_bytes(b"")
    files = ab_test.list_pngs(str(tmp_path))
    assert [os.path.basename(f) for f in files] == ["a.PNG", "b.png", "c.png"]           # sorted, .png only
    plan = ab_test.sample_plan(len(files))
    assert len(plan) == 30
    assert plan[:11] == [(0, p) for p in range(10)] + [(1, 0)]
    assert len(ab_test.sample_plan(25)) == 200 and ab_test.sample_plan(25)[-1] == (19, 9)     # min(200, 10 n)
    assert ab_test.sample_plan(0) == []
    assert [p["lr"] for p in ab_test.SCALE_PAIRS][:3] == [(720, 1280), (720, 1280), (1080, 1920)]
    assert [p["hr"] for p in ab_test.SCALE_PAIRS][-4:] == [(192, 192), (288, 288), (384, 384), (576, 576)]


def test_resize_int_size_rule():
    assert ab_test.resize_int_size(1080, 1920, 720) == (720, 1280)       # shorter side (height) -> 720
    assert ab_test.resize_int_size(1920, 1080, 720) == (1280, 720)       # portrait: width is shorter
    assert ab_test.resize_int_size(96, 96, 64) == (64, 64)
    assert ab_test.resize_int_size(1000, 1777, 720) == (720, int(720 * 1777 / 1000))


def test_skip_rule():
    assert ab_test.skip_sample((720, 1280), (720, 1280))
    assert ab_test.skip_sample((720, 1280), (1080, 1280))
    assert ab_test.skip_sample((720, 1280), (600, 1920))
    assert not ab_test.skip_sample((720, 1280), (1080, 1920))


def test_cli_keeps_the_reference_flags():
    args = ab_test.build_parser().parse_args(
        ["--data_dir", "d", "--model_a", "A", "--model_b", "B", "--checkpoint_dir_a", "ca", "--checkpoint_dir_b", "cb",
         "--batch_size", "2", "--log_interval", "5", "--res_in", "720", "--res_out", "1080", "--json", "o.json", "--no-checkpoint-b"])
    assert (args.data_dir, args.model_a, args.model_b, args.checkpoint_dir_a, args.checkpoint_dir_b) == ("d", "A", "B", "ca", "cb")
    assert (args.batch_size, args.log_interval, args.res_in, args.res_out, args.json) == (2, 5, 720, 1080, "o.json")
    assert args.no_checkpoint_b and not args.no_checkpoint_a
    d = ab_test.build_parser().parse_args(["--model_a", "A", "--model_b", "B"])
    assert (d.data_dir, d.batch_size, d.log_interval, d.res_in, d.res_out, d.json) == ("images/training_set", 1, 10, None, None, None)
    with pytest.raises(SystemExit):
        ab_test.build_parser().parse_args(["--model_a", "A"])


def test_quality_entries_in_header_and_signatures():
    from transformerupscaler_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tupscale_hip.h")).read()
    expected = {"tup_quality_f32_partial": 9, "tup_quality_u8hwc_partial": 9, "tup_quality_reduce": 8}
    for name, nargs in expected.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert len(_lib.SIGNATURES[name]) == nargs, name
    assert _lib.ABI_VERSION == ABI
    assert _lib.load().tup_abi_version() == ABI


def test_metrics_options_and_cpu_tensors_raise():
    import torch
    from transformerupscaler_amd import metrics
    x = torch.rand(1, 3, 8, 8)
    with pytest.raises(NotImplementedError):
        metrics.ssim(x, x, win_size=11)
    with pytest.raises(NotImplementedError):
        metrics.ssim(x, x, gaussian_weights=True)
    with pytest.raises(RuntimeError):
        metrics.quality(x, x)                                             # no CPU fallback
    with pytest.raises(ValueError):
        metrics.quality(torch.rand(1, 3, 6, 8), torch.rand(1, 3, 6, 8))
    with pytest.raises(TypeError):
        metrics.quality(x.double(), x.double())


def test_bicubic_plugin_surface():
    import importlib
    import inspect
    mod = importlib.import_module("models.BicubicInterpolation.model")
    m = mod.TransformerModel()
    assert sum(p.numel() for p in m.parameters()) == 0
    fsig = inspect.signature(mod.TransformerModel.forward)
    assert [p for p in fsig.parameters][1:] == ["x", "res_out"] and fsig.parameters["res_out"].default == (1080, 1920)
