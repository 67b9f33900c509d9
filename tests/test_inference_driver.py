"""The `inference.py` driver: its argument surface against the reference's (no GPU), and one run per model in a child process on a
small PNG written here (GPU): the three JPEG files, `bicubic.jpg` byte for byte against Pillow's own resize + save, and the recorded
scores against `metrics.py` applied to the decoded files."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (36, 52)


def test_the_parser_has_the_references_flags_and_defaults():
    import inference
    parser = inference.build_parser()
    args = parser.parse_args([])
    # reference inference.py:149-170: flag, default
    reference = {"image_path": "images/training_set/image_100.jpg", "model": "FastTransformer", "checkpoint_dir": None, "scale": 3,
                 "res_in": None, "inp": "input.jpg", "out": "model.jpg", "compile": False, "quantize": False}
    for flag, default in reference.items():
        assert getattr(args, flag) == default, flag
    added = {"no_checkpoint": False, "json": None, "quality": 75, "subsampling": "4:2:0"}
    assert {k: getattr(args, k) for k in added} == added and set(vars(args)) == set(reference) | set(added)
    args = parser.parse_args(["--image_path", "a.png", "--model", "BicubicInterpolation", "--checkpoint_dir", "ck", "--scale", "6", "--res_in", "720",
                              "--inp", "i.jpg", "--out", "o.jpg", "--compile", "--quantize", "--no-checkpoint", "--json", "r.json",
                              "--quality", "90", "--subsampling", "4:4:4"])
    assert (args.image_path, args.model, args.checkpoint_dir, args.scale, args.res_in, args.inp, args.out) == \
        ("a.png", "BicubicInterpolation", "ck", 6, "720", "i.jpg", "o.jpg")
    assert args.compile and args.quantize and args.no_checkpoint and (args.json, args.quality, args.subsampling) == ("r.json", 90, "4:4:4")
    for bad in (["--subsampling", "4:2:2"], ["--scale", "two"], ["--quality", "high"], ["--unknown"]):
        with pytest.raises(SystemExit):
            parser.parse_args(bad)
    text = parser.format_help()
    assert "skimage.transform.resize" in text and "GPU resize" in text and "no effect" in text
    assert inference.BICUBIC_PATH == "bicubic.jpg" and inference.SCALES == (2, 3, 4, 6)
    for argv, message in ((["--scale", "5"], "Resolution 5 not found in supported output resolutions."),
                          (["--res_in", "123"], "Resolution 123 not found in supported input resolutions.")):
        with pytest.raises(SystemExit) as e:                   # refused before an image is opened or the GPU is touched
            inference.main(["--image_path", "/nonexistent.png"] + argv)
        assert e.value.code == message


def _png(path):
    from PIL import Image
    yy, xx = np.mgrid[0:HW[0], 0:HW[1]].astype(np.float64)
    rng = np.random.RandomState(4)
    planes = [127 + 90 * np.sin(yy / (5 + c) + c) * np.cos(xx / (7 + 2 * c)) + rng.normal(0, 6, HW) for c in range(3)]
    a = np.clip(np.stack(planes, -1), 0, 255).astype(np.uint8)
    Image.fromarray(a).save(path)
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("model", ("FastTransformer", "BicubicInterpolation"))
def test_driver_writes_three_jpegs_and_scores_them(tmp_path, model):
    import torch
    from PIL import Image
    from transformerupscaler_amd import metrics, ops
    src = str(tmp_path / "in.png")
    a = _png(src)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference.py"), "--image_path", src, "--model", model, "--scale", "2",
                        "--no-checkpoint", "--json", "rec.json", "--inp", "lr.jpg", "--out", "sr.jpg", "--compile"],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = json.load(open(tmp_path / "rec.json"))
    files = {k: open(tmp_path / n, "rb").read() for k, n in (("inp", "lr.jpg"), ("bicubic", "bicubic.jpg"), ("out", "sr.jpg"))}
    decoded = {k: np.asarray(Image.open(io.BytesIO(v)).convert("RGB")) for k, v in files.items()}
    assert decoded["inp"].shape == HW + (3,) and decoded["bicubic"].shape == decoded["out"].shape == (2 * HW[0], 2 * HW[1], 3)
    for k, v in files.items():
        assert rec["files"][k]["bytes"] == len(v) and rec["files"][k]["size"] == list(decoded[k].shape[:2])

    def pil_jpeg(img):
        buf = io.BytesIO()
        img.save(buf, "JPEG", quality=75, restart_marker_rows=1)
        return buf.getvalue()
    assert files["inp"] == pil_jpeg(Image.fromarray(a))
    assert files["bicubic"] == pil_jpeg(Image.fromarray(a).resize((2 * HW[1], 2 * HW[0]), Image.BICUBIC))
    plain = io.BytesIO()                                        # ... and the pixels are those of Pillow's default save()
    Image.fromarray(a).save(plain, "JPEG")
    assert np.array_equal(decoded["inp"], np.asarray(Image.open(plain).convert("RGB")))

    # the recorded scores are metrics.py on the decoded files: original -> the output's size, low-res -> the original's, by the GPU resize
    dev = "cuda"
    original = ops.resize_frames(torch.from_numpy(a).to(dev), decoded["out"].shape[:2])
    lowres = ops.resize_frames(torch.from_numpy(decoded["inp"].copy()).to(dev), decoded["out"].shape[:2])
    for name, img in (("model", torch.from_numpy(decoded["out"].copy()).to(dev)[None]), ("bicubic", lowres)):
        q = metrics.quality(original, img.contiguous())
        assert rec["scores"][name] == {"ssim": float(q["ssim"][0]), "psnr": float(q["psnr"][0])}, name
        assert -1.0 <= rec["scores"][name]["ssim"] <= 1.0 and 0.0 < rec["scores"][name]["psnr"] < 100.0
    assert rec["scores"]["bicubic"]["ssim"] > 0.5 and rec["scores"]["bicubic"]["psnr"] > 15.0            # a smooth image, upscaled by 2
    out = r.stdout
    assert f"Bicubic Scores:\tSSIM: {rec['scores']['bicubic']['ssim']:.4f}, PSNR: {rec['scores']['bicubic']['psnr']:.2f} dB" in out
    assert f"Model Scores:\tSSIM: {rec['scores']['model']['ssim']:.4f}, PSNR: {rec['scores']['model']['psnr']:.2f} dB" in out
    assert f"Model has {rec['n_params']} trainable parameters" in out and "--compile has no effect" in out
    assert "Downscaled image saved to: lr.jpg" in out and "Bicubic image saved to: bicubic.jpg" in out and "Upscaled image saved to: sr.jpg" in out
    assert rec["n_params"] == (0 if model == "BicubicInterpolation" else rec["n_params"]) and (model != "FastTransformer" or rec["n_params"] > 10 ** 5)
    assert rec["checkpoint"] is None and rec["quality"] == 75 and rec["subsampling"] == "4:2:0" and rec["scale"] == 2
