"""GPU checks of the quality metrics (csrc/metrics.hip via transformerupscaler_amd.metrics) against the float64 restatement of
skimage's SSIM / PSNR (tests/_metrics_ref.py), of the BicubicInterpolation plugin against torch's bicubic interpolation, and of
the A/B driver (ab_test.py) end to end."""
import importlib
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _metrics_ref as R          # tests/ is on sys.path (rootdir-less test modules)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SSIM_TOL, PSNR_TOL, MSE_RTOL = 1e-6, 1e-4, 1e-6


def _smooth(h, w, g):
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h, dtype=torch.float64), torch.linspace(0, 1, w, dtype=torch.float64), indexing="ij")
    ph = torch.rand(3, 1, 1, generator=g, dtype=torch.float64) * 6
    return (0.5 + 0.4 * torch.sin(6 * xx + ph) * torch.cos(4 * yy - ph)).float()


def _blur(x):
    k = torch.ones(3, 1, 5, 5) / 25
    return F.conv2d(F.pad(x.unsqueeze(0), (2, 2, 2, 2), mode="replicate"), k, groups=3)[0]


def _case(kind, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "noise":
        a = torch.rand(3, h, w, generator=g)
        b = torch.rand(3, h, w, generator=g)
    elif kind == "smooth":
        a = _smooth(h, w, g)
        b = (a + 0.01 * torch.randn(3, h, w, generator=g)).clamp(0, 1)
    elif kind == "blur":
        a = (_smooth(h, w, g) + 0.05 * torch.randn(3, h, w, generator=g)).clamp(0, 1)
        b = _blur(a)
    else:                                                     # flat bright: catches naive fp32 window moments
        a = torch.full((3, h, w), 0.9)
        b = a + 1e-3 * torch.randn(3, h, w, generator=g)
    return a.contiguous(), b.contiguous()


def _ref(a, b, data_range=1.0):
    """float64 restatement of one planar [3][H][W] image pair (channel_axis=-1 after a transpose)."""
    x = a.double().permute(1, 2, 0).numpy()
    y = b.double().permute(1, 2, 0).numpy()
    return R.mse(x, y), R.psnr(x, y, data_range), R.ssim(x, y, data_range)


def _assert_close(q, i, ref, label):
    mse, psnr, ssim = ref
    got_mse, got_psnr, got_ssim = q["mse"][i].item(), q["psnr"][i].item(), q["ssim"][i].item()
    d_ssim, d_psnr = abs(got_ssim - ssim), abs(got_psnr - psnr)
    r_mse = abs(got_mse - mse) / mse
    print(f"{label}: |dSSIM| {d_ssim:.2e}  |dPSNR| {d_psnr:.2e} dB  rel dMSE {r_mse:.2e}  (SSIM {ssim:.6f}, PSNR {psnr:.3f})")
    assert d_ssim <= SSIM_TOL and d_psnr <= PSNR_TOL and r_mse <= MSE_RTOL, label


@pytest.mark.parametrize("kind", ["noise", "smooth", "blur", "flat"])
@pytest.mark.parametrize("hw", [(7, 7), (13, 29), (64, 64), (720, 1280)])
def test_f32_against_float64_restatement(kind, hw):
    a, b = _case(kind, *hw, seed=zlib.crc32(f"{kind}{hw}".encode()) % 1000)
    q = _quality(a.unsqueeze(0), b.unsqueeze(0))
    _assert_close(q, 0, _ref(a, b), f"f32 {kind} {hw}")
    chans = q["ssim_channels"][0].cpu()
    assert q["ssim_channels"].shape == (1, 3)
    assert abs(chans.mean().item() - q["ssim"][0].item()) < 1e-15


def _quality(a, b, **kw):
    from transformerupscaler_amd import metrics
    q = metrics.quality(a.to(DEV), b.to(DEV), **kw)
    assert all(v.dtype == torch.float64 and v.is_cuda for v in q.values())
    return q


def test_f32_4k_and_batch_of_three():
    a, b = _case("smooth", 2160, 3840, seed=5)
    _assert_close(_quality(a, b), 0, _ref(a, b), "f32 smooth 2160x3840 (3-D input)")
    pairs = [_case(k, 96, 300, seed=s) for s, k in enumerate(("noise", "blur", "flat"))]
    q = _quality(torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs]))
    assert q["ssim"].shape == (3,)
    for i, (a, b) in enumerate(pairs):
        _assert_close(q, i, _ref(a, b), f"f32 batch item {i}")


@pytest.mark.parametrize("hw", [(7, 7), (13, 29), (256, 520), (720, 1280)])
def test_u8_against_float64_restatement(hw):
    from transformerupscaler_amd import metrics, ops
    g = torch.Generator().manual_seed(hw[0])
    a = torch.randint(0, 256, (2, *hw, 3), dtype=torch.uint8, generator=g)
    noise = torch.randint(-20, 21, a.shape, generator=g)
    b = (a.int() + noise).clamp(0, 255).to(torch.uint8)
    q = _quality(a, b)
    for i in range(2):
        x = a[i].double().numpy() / 255
        y = b[i].double().numpy() / 255
        ref = (R.mse(a[i].numpy(), b[i].numpy()), R.psnr(x, y, 1.0), R.ssim(x, y, 1.0))
        _assert_close(q, i, ref, f"u8 {hw} item {i}")
    # the same quantity through ToTensor
    au, bu = a.to(DEV), b.to(DEV)
    s8 = metrics.ssim(au, bu)
    s32 = metrics.ssim(ops.frames_to_tensor(au), ops.frames_to_tensor(bu))
    assert (s8 - s32).abs().max().item() <= 1e-6


def test_identical_inputs():
    from transformerupscaler_amd import metrics
    a, _ = _case("smooth", 100, 300, seed=7)
    a = a.unsqueeze(0).to(DEV)
    q = metrics.quality(a, a.clone())
    assert q["mse"].item() == 0.0 and q["psnr"].item() == float("inf") and q["ssim"].item() >= 1 - 1e-6
    u = torch.randint(0, 256, (1, 50, 60, 3), dtype=torch.uint8, device=DEV)
    q = metrics.quality(u, u.clone())
    assert q["mse"].item() == 0.0 and q["psnr"].item() == float("inf") and q["ssim"].item() >= 1 - 1e-6


def test_bitwise_batch_independent_and_repeatable():
    from transformerupscaler_amd import metrics
    pairs = [_case(k, 300, 530, seed=10 + s) for s, k in enumerate(("noise", "smooth", "blur", "flat"))]
    A = torch.stack([p[0] for p in pairs]).to(DEV)
    Bt = torch.stack([p[1] for p in pairs]).to(DEV)
    q4 = metrics.quality(A, Bt)
    q4b = metrics.quality(A, Bt)
    u = (A * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    v = (Bt.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    u4 = metrics.quality(u, v)
    for key in ("mse", "psnr", "ssim", "ssim_channels"):
        assert torch.equal(q4[key], q4b[key]), key
    for i in range(4):
        q1 = metrics.quality(A[i:i + 1].contiguous(), Bt[i:i + 1].contiguous())
        u1 = metrics.quality(u[i:i + 1].contiguous(), v[i:i + 1].contiguous())
        for key in ("mse", "psnr", "ssim", "ssim_channels"):
            assert torch.equal(q1[key][0], q4[key][i]), (i, key)
            assert torch.equal(u1[key][0], u4[key][i]), (i, key)


def test_errors():
    from transformerupscaler_amd import metrics
    x = torch.rand(1, 3, 16, 16, device=DEV)
    with pytest.raises(ValueError):
        metrics.quality(torch.rand(1, 3, 6, 16, device=DEV), torch.rand(1, 3, 6, 16, device=DEV))
    with pytest.raises(ValueError):
        metrics.quality(torch.rand(1, 3, 16, 5, device=DEV), torch.rand(1, 3, 16, 5, device=DEV))
    with pytest.raises(ValueError):
        metrics.quality(x, torch.rand(1, 3, 16, 17, device=DEV))
    with pytest.raises(TypeError):
        metrics.quality(x, x.to(torch.float16))
    with pytest.raises(TypeError):
        metrics.quality(x.double(), x.double())
    with pytest.raises(ValueError):
        metrics.quality(x, torch.rand(1, 3, 16, 32, device=DEV)[..., ::2])          # non-contiguous
    with pytest.raises(RuntimeError):
        metrics.quality(x.cpu(), x.cpu())
    u = torch.zeros(1, 16, 16, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        metrics.quality(u, torch.zeros(1, 16, 16, 4, dtype=torch.uint8, device=DEV))
    with pytest.raises(NotImplementedError):
        metrics.ssim(x, x, win_size=11)


@pytest.mark.parametrize("hw_in,hw_out", [((24, 40), (48, 80)), ((37, 53), (100, 71)), ((96, 96), (576, 576)), ((50, 70), (75, 105))])
def test_bicubic_plugin_matches_torch(hw_in, hw_out):
    mod = importlib.import_module("models.BicubicInterpolation.model")
    x = torch.rand(2, 3, *hw_in, generator=torch.Generator().manual_seed(1)).to(DEV)
    y = mod.TransformerModel().to(DEV).eval()(x, res_out=hw_out)
    ref = F.interpolate(x, size=hw_out, mode="bicubic", align_corners=False)
    assert y.shape == ref.shape
    assert (y - ref).abs().max().item() <= 1e-5


def test_ab_test_end_to_end(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import ab_test
    from transformerupscaler_amd import harness, ops
    from transformerupscaler_amd.weights import deterministic_state_dict
    data = tmp_path / "data"
    data.mkdir()
    g = torch.Generator().manual_seed(3)
    for n in ("img_b.png", "img_a.png"):
        base = _smooth(270, 480, g).permute(1, 2, 0)
        arr = ((base + 0.05 * torch.rand(270, 480, 3, generator=g)).clamp(0, 1) * 255).to(torch.uint8).numpy()
        Image.fromarray(arr).save(data / n)
    ft = importlib.import_module("models.FastTransformer.model").TransformerModel()
    ft.load_state_dict(deterministic_state_dict(0), strict=False)
    harness.save_checkpoint(ft, str(tmp_path / "ckpt"), 1)
    out_json = tmp_path / "ab.json"
    record = ab_test.main(["--data_dir", str(data), "--model_a", "FastTransformer", "--model_b", "BicubicInterpolation",
                           "--checkpoint_dir_a", str(tmp_path / "ckpt"), "--no-checkpoint-b", "--json", str(out_json)])
    assert record["processed_samples"] == 20 and len(record["samples"]) == 20
    assert os.path.exists(out_json)
    model_a, _ = ab_test.load_model("FastTransformer", str(tmp_path / "ckpt"), True, DEV)
    model_b, _ = ab_test.load_model("BicubicInterpolation", None, False, DEV)
    files = ab_test.list_pngs(str(data))
    frames = {}
    with torch.no_grad():
        for s in record["samples"]:
            img, pair = divmod(s["index"], 10)
            assert (files[img].endswith(s["image"]), pair) == (True, s["pair"])
            if img not in frames:
                frames[img] = torch.from_numpy(np.asarray(Image.open(files[img]).convert("RGB")).copy()).to(DEV)
            p = ab_test.SCALE_PAIRS[pair]
            lr, hr = ab_test.make_pair(frames[img], p)
            assert torch.equal(lr, ops.resize_frames(frames[img], p["lr"], to_tensor=True))
            assert torch.equal(hr, ops.resize_frames(frames[img], p["hr"], to_tensor=True))
            for key, model in (("a", model_a), ("b", model_b)):
                ref = F.mse_loss(model(lr, res_out=tuple(hr.shape[2:])), hr).item()
                assert abs(s[key]["mse"] - ref) <= 1e-6 * ref, (s["index"], key, s[key]["mse"], ref)
    summ = record["summary"]
    assert summ["a"]["average_loss"] == pytest.approx(sum(s["a"]["mse"] for s in record["samples"]) / 20)
