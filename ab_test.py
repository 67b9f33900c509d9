#!/usr/bin/env python
"""A/B quality test of two model plugins (reference ab_test.py), with SSIM and PSNR next to the reference's MSE.

Both models run over the samples of ``--data_dir`` and each output is scored against its high-resolution target on the GPU
(``transformerupscaler_amd.metrics``: MSE, PSNR and SSIM from one kernel pass).  The reference's summary lines are printed
unchanged, followed by one ``PSNR: xx.xx dB | SSIM: 0.xxxx`` line per model (means over the samples).

    python ab_test.py --data_dir images/test_set --model_a FastTransformer --model_b BicubicInterpolation --no-checkpoint-b

Samples (the reference's ``highres_img_dataset``, data_handling/data_class.py:24-75):

* the ``.png`` files of ``--data_dir``, SORTED by name (the reference takes ``os.listdir`` order, which the file system decides);
* the ten scale pairs of data_class.py:34-45 in their order; sample ``i`` is image ``i // 10`` under pair ``i % 10``;
* ``min(200, 10 * n_png)`` samples.  The reference's dataset reports 200 whatever the directory holds and raises IndexError with
  fewer than 20 images; here a smaller directory gives fewer samples.

Each PNG is decoded once on the host (PIL) and uploaded as uint8; LR and HR are built on the GPU by ``ops.resize_frames``
(Pillow-exact BILINEAR Resize + ToTensor), instead of one decode and two host resizes per sample.  Then, per sample, as
ab_test.py:96-124: ``--res_in`` / ``--res_out`` resize LR / HR with ``Resize(int)`` (shorter side to the value, the longer
``int(value * long / short)``; torchvision's antialiased bilinear tensor resize = ``ops.resize_aa``) when their height differs;
the sample is skipped if HR is not larger than LR on both axes; then ``model(lr, res_out=hr_size)`` at batch 1.  Results stay on
the GPU until the end (one synchronisation).

Batch 1 is the reference's evaluation and is kept: at B = 1 FastTransformer's six blocks take the small-launch block kernel
(below ``engine.STREAM_MIN_WINDOWS`` windows), not the streamed kernel of large batches, and the numbers here are those of that
route (the two routes agree to fp32 rounding but are not bit-identical; ADVICE.md, batch invariance).  ``--batch_size`` only
groups the progress log, as in the reference.

Checkpoints: the latest ``*_<epoch>.pth`` of ``--checkpoint_dir_a`` / ``_b`` (default ``models/<name>/checkpoints``), loaded
strictly; ``--no-checkpoint-a`` / ``-b`` skip that for parameterless models such as BicubicInterpolation.  ``--json PATH``
writes a per-sample and summary record.
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# data_handling/data_class.py:34-45, in that order
SCALE_PAIRS = [
    {"lr": (720, 1280), "hr": (1080, 1920)},
    {"lr": (720, 1280), "hr": (1440, 2560)},
    {"lr": (1080, 1920), "hr": (1440, 2560)},
    {"lr": (720, 1280), "hr": (2160, 3840)},
    {"lr": (1080, 1920), "hr": (2160, 3840)},
    {"lr": (1440, 2560), "hr": (2160, 3840)},
    {"lr": (96, 96), "hr": (192, 192)},
    {"lr": (96, 96), "hr": (288, 288)},
    {"lr": (96, 96), "hr": (384, 384)},
    {"lr": (96, 96), "hr": (576, 576)},
]
MAX_SAMPLES = 200          # data_class.py:47-50: __len__ returns 200


def list_pngs(data_dir):
    """The ``.png`` files of data_dir (case-insensitive suffix, data_class.py:26-31), sorted by name."""
    return sorted(os.path.join(data_dir, f) for f in os.listdir(data_dir) if f.lower().endswith(".png"))


def sample_plan(n_png):
    """[(image index, scale-pair index)] of the samples: index i -> (i // 10, i % 10), min(200, 10 * n_png) of them."""
    n = min(MAX_SAMPLES, len(SCALE_PAIRS) * n_png)
    return [(i // len(SCALE_PAIRS), i % len(SCALE_PAIRS)) for i in range(n)]


def resize_int_size(h, w, size):
    """Output (h, w) of torchvision ``Resize(size)`` with an int: the shorter side becomes size, the longer int(size * long / short)."""
    size = int(size)
    if w <= h:
        return int(size * h / w), size
    return size, int(size * w / h)


def skip_sample(lr_hw, hr_hw):
    """ab_test.py:103-105: skip unless HR is larger than LR on both axes."""
    return hr_hw[0] / lr_hw[0] <= 1 or hr_hw[1] / lr_hw[1] <= 1


def build_parser():
    p = argparse.ArgumentParser(description="AB Test for Transformer Upscaler Models")
    p.add_argument("--data_dir", type=str, default="images/training_set", help="Directory containing images (.png)")
    p.add_argument("--batch_size", type=int, default=1, help="Samples per progress-log batch (evaluation itself is at batch 1)")
    p.add_argument("--log_interval", type=int, default=10, help="Log progress every N batches")
    p.add_argument("--model_a", type=str, required=True, help="Model A name (e.g. 'FastTransformer')")
    p.add_argument("--model_b", type=str, required=True, help="Model B name (e.g. 'BicubicInterpolation')")
    p.add_argument("--checkpoint_dir_a", type=str, default=None, help="Checkpoint directory for model A (default: models/{model_a}/checkpoints/)")
    p.add_argument("--checkpoint_dir_b", type=str, default=None, help="Checkpoint directory for model B (default: models/{model_b}/checkpoints/)")
    p.add_argument("--res_in", type=int, default=None, help="Resize LR images whose height differs to this (Resize(int))")
    p.add_argument("--res_out", type=int, default=None, help="Resize HR images whose height differs to this (Resize(int))")
    p.add_argument("--json", type=str, default=None, help="Write a per-sample and summary record to this path")
    p.add_argument("--no-checkpoint-a", dest="no_checkpoint_a", action="store_true", help="Model A has no parameters: load no checkpoint")
    p.add_argument("--no-checkpoint-b", dest="no_checkpoint_b", action="store_true", help="Model B has no parameters: load no checkpoint")
    return p


def load_model(name, checkpoint_dir, use_checkpoint, device):
    """(model on device in eval mode, checkpoint path or None)."""
    import torch
    from tools.utils import get_latest_checkpoint
    model = importlib.import_module(f"models.{name}.model").TransformerModel()
    ckpt = None
    if use_checkpoint:
        ckpt, _ = get_latest_checkpoint(checkpoint_dir or os.path.join("models", name, "checkpoints"))
        model.load_state_dict(torch.load(ckpt, map_location="cpu"))
    return model.to(device).eval(), ckpt


def decode_png(path, device):
    """uint8 [H][W][3] on the GPU (one host decode per image)."""
    import numpy as np
    import torch
    from PIL import Image
    with Image.open(path) as im:
        arr = np.asarray(im.convert("RGB"))
    return torch.from_numpy(arr.copy()).to(device)


def make_pair(frame_u8, pair, res_in=None, res_out=None):
    """(lr, hr) fp32 [1][3][h][w] of one decoded image under one scale pair, with the --res_in / --res_out rule applied."""
    from transformerupscaler_amd import ops
    lr = ops.resize_frames(frame_u8, pair["lr"], to_tensor=True)
    hr = ops.resize_frames(frame_u8, pair["hr"], to_tensor=True)
    if res_in is not None and lr.shape[2] != res_in:
        lr = ops.resize_aa(lr, resize_int_size(lr.shape[2], lr.shape[3], res_in))
    if res_out is not None and hr.shape[2] != res_out:
        hr = ops.resize_aa(hr, resize_int_size(hr.shape[2], hr.shape[3], res_out))
    return lr, hr


def run(args, device="cuda"):
    """The A/B pass; prints as the reference does and returns the record that --json writes."""
    import torch
    from transformerupscaler_amd import metrics

    print(f"Running AB test on device: {device}")
    files = list_pngs(args.data_dir)
    plan = sample_plan(len(files))
    model_a, ckpt_a = load_model(args.model_a, args.checkpoint_dir_a, not args.no_checkpoint_a, device)
    model_b, ckpt_b = load_model(args.model_b, args.checkpoint_dir_b, not args.no_checkpoint_b, device)
    print(f"Model A ({args.model_a}) checkpoint: {ckpt_a}")
    print(f"Model B ({args.model_b}) checkpoint: {ckpt_b}")

    samples, scores = [], []          # scores: per sample a [2][3] (model, {mse, psnr, ssim}) float64 GPU tensor
    frame, frame_idx = None, -1
    per_batch = max(1, args.batch_size)
    with torch.no_grad():
        for i, (img_idx, pair_idx) in enumerate(plan):
            if img_idx != frame_idx:
                frame, frame_idx = decode_png(files[img_idx], device), img_idx
            lr, hr = make_pair(frame, SCALE_PAIRS[pair_idx], args.res_in, args.res_out)
            lr_hw, hr_hw = tuple(lr.shape[2:]), tuple(hr.shape[2:])
            if not skip_sample(lr_hw, hr_hw):
                rows = []
                for model in (model_a, model_b):
                    q = metrics.quality(model(lr, res_out=hr_hw), hr)
                    rows.append(torch.stack([q["mse"][0], q["psnr"][0], q["ssim"][0]]))
                scores.append(torch.stack(rows))
                samples.append({"index": i, "image": os.path.basename(files[img_idx]), "pair": pair_idx,
                                "lr": list(lr_hw), "hr": list(hr_hw)})
            if (i // per_batch + 1) % args.log_interval == 0 and (i + 1) % per_batch == 0:
                print(f"Processed {len(samples)} samples so far...")

    record = {"model_a": args.model_a, "model_b": args.model_b, "checkpoint_a": ckpt_a, "checkpoint_b": ckpt_b,
              "samples": samples, "processed_samples": len(samples)}
    if not samples:
        print("No samples matched the specified resolution criteria.")
        return record
    vals = torch.stack(scores).cpu().tolist()          # the one synchronisation
    summary = {}
    for m, key in enumerate(("a", "b")):
        for s, v in zip(samples, vals):
            s[key] = {"mse": v[m][0], "psnr": v[m][1], "ssim": v[m][2]}
        losses = [v[m][0] for v in vals]
        psnrs = [v[m][1] for v in vals]
        total = sum(losses)
        summary[key] = {"total_loss": total, "average_loss": total / len(vals), "psnr": sum(psnrs) / len(psnrs),
                        "ssim": sum(v[m][2] for v in vals) / len(vals)}
    record["summary"] = summary
    a, b = summary["a"], summary["b"]
    print("========================================")
    print(f"Model A ({args.model_a}) Total Loss: {a['total_loss']:.6f} | Average Loss: {a['average_loss']:.6f}")
    print(f"Model B ({args.model_b}) Total Loss: {b['total_loss']:.6f} | Average Loss: {b['average_loss']:.6f}")
    print(f"Model A ({args.model_a}) PSNR: {a['psnr']:.2f} dB | SSIM: {a['ssim']:.4f}")
    print(f"Model B ({args.model_b}) PSNR: {b['psnr']:.2f} dB | SSIM: {b['ssim']:.4f}")
    print("========================================")
    return record


def main(argv=None):
    args = build_parser().parse_args(argv)
    record = run(args)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1, allow_nan=True)
    return record


if __name__ == "__main__":
    main()
