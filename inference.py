#!/usr/bin/env python
"""One image in, an upscaled image out, scored against the bicubic baseline (reference inference.py), with every image file written
by the GPU encoders: a PNG (lossless, ``ops.png_encode``) where the path ends in ``.png``, a JPEG (``ops.jpeg_encode``) otherwise.

    python inference.py --image_path images/training_set/image_0.png --model FastTransformer --res_in 720 --scale 3

What happens, in the reference's order (inference.py:64-146):

1. the input is decoded once: a baseline JPEG on the GPU (``ops.jpeg_decode``; a file without restart markers with ``index="sync"``,
   DESIGN 7l), anything else (PNG, progressive JPEG) on the host by Pillow and uploaded as uint8; ``--json`` names which
   (``input_decoder``);
2. ``Resize(res_in)`` + ``ToTensor`` run on the GPU (``ops.resize_frames``, Pillow-exact BILINEAR; ``ops.frames_to_tensor``);
3. ``--inp`` (the low-resolution input) and ``bicubic.jpg`` (``Image.resize(.., Image.BICUBIC)`` of it by ``--scale``, in the current
   directory as in the reference; ``ops.resize_frames(resample="bicubic")``, Pillow-exact) are encoded by ``ops.jpeg_encode``;
4. the model runs with ``upscale_factor=scale`` (plugins without that argument get ``res_out`` = the input size times scale);
5. ``--out`` is encoded by ``ops.jpeg_encode`` straight from the model's fp32 output: ``trunc(clamp(x * 255, 0, 255))`` happens inside
   the encoder's first kernel, so no uint8 frame is written in between.  (The reference's ``ToPILImage`` wraps values outside [0, 1]
   instead of clamping them; the models here clamp their output anyway.)

As in the reference, where ``Image.save(path)`` picks the format from the suffix, ``--inp x.png`` and ``--out y.png`` (any letter case)
are PNG files: 8-bit RGB, adaptive filtering, coded by ``ops.png_encode``.  ``--quality`` and ``--subsampling`` do not apply
to them, and nothing is decoded for their scores: a PNG holds exactly the uint8 frame that was encoded (``tensor_to_frames`` of the
output for ``--out``), so that frame is scored.  ``bicubic.jpg`` stays a JPEG.

``--png_bits 16`` makes ``--out``, when it is a ``.png``, a 16-bit file (IHDR depth 16, ``ops.png_encode(.., bits=16)``): the model's
fp32 output, the one source here with more than 8 bits, quantised by rounding to 0..65535 inside the encoder.  ``--inp`` and
``bicubic.jpg`` come from uint8 frames and stay as they are; the scores stay on the 8-bit frame (``tensor_to_frames`` of the output),
which is the reference's metric; the ``--json`` record names the depth of every file (``"bits"``).

The JPEG files are what Pillow's ``save()`` writes for the same pixels at ``--quality`` / ``--subsampling`` (defaults 75 and 4:2:0, Pillow's
own) with a restart marker after every MCU row; they decode to the same pixels as Pillow's files without restart markers.

Scores, as the reference computes them, on the DECODED files (``ops.jpeg_decode`` decodes the bytes just produced, to Pillow's
pixels): SSIM and PSNR of ``--out`` and of the upscaled ``--inp`` against the original, by ``transformerupscaler_amd.metrics`` (skimage's defaults: 7 x 7 uniform window,
``data_range`` = the full range).  The reference brings the original to the output's size, and the low-resolution input to the
original's, with ``skimage.transform.resize``; scikit-image is not a dependency here, so both resizes are the project's GPU resize
(``ops.resize_frames``, Pillow's BILINEAR, antialiased when shrinking).  The printed scores are therefore comparable with the
reference's, not equal to them digit for digit.

``--compile`` and ``--quantize`` are accepted and reported: there is nothing for torch.compile or dynamic quantisation to act on in
a forward made of HIP kernels.  ``--no-checkpoint`` runs the plugin as constructed (parameterless plugins such as
BicubicInterpolation, or a smoke run); ``--json PATH`` writes the record ``main`` returns.
"""
import argparse
import importlib
import inspect
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCALES = (2, 3, 4, 6)
BICUBIC_PATH = "bicubic.jpg"        # inference.py:84


def build_parser():
    p = argparse.ArgumentParser(
        description="Inference script for the Transformer upscaler: one image in, an upscaled image out, SSIM / PSNR against the bicubic "
                    "baseline.  All image files are written by the GPU encoders: a path that ends in .png gets a lossless PNG "
                    "(ops.png_encode), any other a JPEG (ops.jpeg_encode).  The scores are computed on the decoded JPEG files, or on the "
                    "frame a PNG was made from, with transformerupscaler_amd.metrics; where the reference resizes with skimage.transform.resize, "
                    "this driver uses the project's GPU resize (Pillow's BILINEAR), so the scores are comparable with the reference's, "
                    "not digit-for-digit equal.")
    p.add_argument("--image_path", type=str, default="images/training_set/image_100.jpg", help="Path to the input image file")
    p.add_argument("--model", type=str, default="FastTransformer", help="Model name to use (corresponds to models/{model}/model.py)")
    p.add_argument("--checkpoint_dir", type=str, default=None,
                   help="Directory containing model checkpoints (default: models/{model}/checkpoints/)")
    p.add_argument("--scale", type=int, default=3, help="Output resolution scale (2, 3, 4, 6)")
    p.add_argument("--res_in", type=str, default=None, help="Input resolution key (None for no downscaling)")
    p.add_argument("--inp", type=str, default="input.jpg", help="Output file path for the downscaled input image (.png: a lossless PNG; otherwise JPEG)")
    p.add_argument("--out", type=str, default="model.jpg", help="Output file path for the upscaled output image (.png: a lossless PNG; otherwise JPEG)")
    p.add_argument("--compile", action="store_true", help="Accepted for compatibility; no effect on the HIP path (reported)")
    p.add_argument("--quantize", action="store_true", help="Accepted for compatibility; no effect on the HIP path (reported)")
    p.add_argument("--no-checkpoint", dest="no_checkpoint", action="store_true", help="Load no checkpoint: run the model as constructed")
    p.add_argument("--json", type=str, default=None, help="Write the scores, sizes and file lengths to this path")
    p.add_argument("--quality", type=int, default=75, help="JPEG quality 1..100 (default 75, Pillow's); ignored for .png files")
    p.add_argument("--subsampling", type=str, default="4:2:0", choices=("4:2:0", "4:4:4"), help="JPEG chroma subsampling (default 4:2:0, Pillow's); ignored for .png files")
    return p


def parse_args(argv=None):
    """What the command line parses with: `build_parser()`, which stays the reference's flags plus the JPEG ones, and `--png_bits`."""
    p = build_parser()
    p.add_argument("--png_bits", type=int, default=8, choices=(8, 16),
                   help="Bit depth of --out when it is a .png: 8 (default), or 16 for the model's fp32 output rounded to 16 bits; --inp and "
                        "bicubic.jpg are made from 8-bit frames and stay 8-bit")
    p.epilog = "--png_decoder {host,gpu}: " + PNG_DECODER_HELP
    return p.parse_args(argv)


PNG_DECODERS = ("host", "gpu")
PNG_DECODER_HELP = "How a PNG --image_path is decoded: host (Pillow, default) or gpu (ops.png_decode: same pixels, slower for one file)"


def png_decoder_parser():
    """The parser of the one flag that is read ahead of `parse_args`, whose namespace stays the reference's flags plus the JPEG ones
    and --png_bits (tests pin it)."""
    p = argparse.ArgumentParser(add_help=False, allow_abbrev=False, prog="inference.py")
    p.add_argument("--png_decoder", choices=PNG_DECODERS, default="host",
                   help=PNG_DECODER_HELP)
    return p


def take_png_decoder(argv):
    """``--png_decoder {host,gpu}`` taken out of the command line -> (the decoder, the other arguments)."""
    known, rest = png_decoder_parser().parse_known_args(argv)
    return known.png_decoder, rest


def file_format(path):
    """'png' for a path that ends in .png in any letter case, else 'jpeg' (what this driver writes for every other name)"""
    return "png" if os.path.splitext(path)[1].lower() == ".png" else "jpeg"


def decode_image_named(path_or_bytes, device, gpu=True, png_decoder="host"):
    """(uint8 [H][W][3] RGB on the GPU, the decoder that made it).  With png_decoder="gpu" a PNG that ``ops.png_parse`` accepts is
    decoded by ``ops.png_decode`` ("gpu:png"; same pixels as Pillow's; a refused or damaged file goes to the host as before).  A baseline JPEG is decoded there by ``ops.jpeg_decode``, whose
    pixels are Pillow's: with restart markers (every file this driver writes) interval by interval ("gpu:restart-intervals"),
    without them through the self-synchronising index ("gpu:sync-index": ``index="sync"``, measured faster than the host for
    2160 x 3840 files).  Everything else (PNG, progressive JPEG, a damaged file), or everything with gpu=False, is one
    host decode by Pillow and an upload ("pillow")."""
    import numpy as np
    import torch
    from PIL import Image
    if gpu:
        from transformerupscaler_amd import ops
        data = path_or_bytes
        if not isinstance(data, (bytes, bytearray)):
            with open(data, "rb") as f:
                data = f.read()
        try:
            index = "serial" if ops.jpeg_parse(data)["restart_interval"] > 0 else "sync"
        except ValueError:
            index = None
        if index:
            with torch.cuda.device(device):
                frames, status = ops.jpeg_decode(data, index=index)
            if int(status[0]) == 0:
                return frames[0], "gpu:sync-index" if index == "sync" else "gpu:restart-intervals"
        elif png_decoder == "gpu":
            try:
                with torch.cuda.device(device):
                    frames, status = ops.png_decode(data)
                if int(status[0]) == 0:
                    return frames[0], "gpu:png"
            except ValueError as e:                         # what ops.png_parse or ops.png_decode refuses: the host decodes it
                import warnings
                warnings.warn(f"inference.py: the PNG is decoded on the host ({e})")
        path_or_bytes = data
    src = io.BytesIO(path_or_bytes) if isinstance(path_or_bytes, (bytes, bytearray)) else path_or_bytes
    with Image.open(src) as im:
        arr = np.asarray(im.convert("RGB"))
    return torch.from_numpy(arr.copy()).to(device), "pillow"


def decode_image(path_or_bytes, device, gpu=True, png_decoder="host"):
    """The frame of `decode_image_named`; the decoder's name rides on it as the attribute ``decoder``."""
    frame, name = decode_image_named(path_or_bytes, device, gpu, png_decoder)
    frame.decoder = name
    return frame


def forward(model, lr, scale):
    """model(lr, upscale_factor=scale), or res_out = scale times the input for a plugin that has no such argument."""
    if "upscale_factor" in inspect.signature(model.forward).parameters:
        return model(lr, upscale_factor=scale)
    return model(lr, res_out=(lr.shape[2] * scale, lr.shape[3] * scale))


def score(original_u8, pred_u8, lowres_u8):
    """inference.py:129-140 on decoded uint8 [H][W][3] frames: the original is brought to the output's size, the low-resolution
    input to the original's; returns {"model": {ssim, psnr}, "bicubic": {ssim, psnr}} as GPU scalars."""
    from transformerupscaler_amd import metrics, ops
    if tuple(original_u8.shape[:2]) != tuple(pred_u8.shape[:2]):
        original_u8 = ops.resize_frames(original_u8, tuple(pred_u8.shape[:2]))[0]
    lowres_u8 = ops.resize_frames(lowres_u8, tuple(original_u8.shape[:2]))[0]
    out = {}
    for name, img in (("model", pred_u8), ("bicubic", lowres_u8)):
        q = metrics.quality(original_u8.contiguous(), img.contiguous())
        out[name] = {"ssim": q["ssim"][0], "psnr": q["psnr"][0]}
    return out


def run(args, device="cuda"):
    import torch
    from tools.utils import get_latest_checkpoint, resolutions
    from transformerupscaler_amd import ops

    if args.scale not in SCALES:
        raise SystemExit(f"Resolution {args.scale} not found in supported output resolutions.")
    if args.res_in and args.res_in not in resolutions:
        raise SystemExit(f"Resolution {args.res_in} not found in supported input resolutions.")
    res_in = resolutions[args.res_in] if args.res_in else None
    print(f"Running inference on device: {device}")
    for flag in ("compile", "quantize"):
        if getattr(args, flag):
            print(f"--{flag} has no effect: the forward is made of HIP kernels")
    jpeg = dict(quality=args.quality, subsampling=args.subsampling)

    out_bits = 16 if getattr(args, "png_bits", 8) == 16 and file_format(args.out) == "png" else 8

    def save(frames, path, bits=8):
        if file_format(path) == "png":
            data = ops.png_files(*(ops.png_encode(frames, bits=16) if bits == 16 else ops.png_encode(frames)))[0]
        else:
            data = ops.jpeg_files(*ops.jpeg_encode(frames, **jpeg))[0]
        with open(path, "wb") as f:
            f.write(data)
        return data

    # the keyword only where it was asked for: callers and tests that stand in for decode_image take (path, device)
    original = decode_image(args.image_path, device, **({"png_decoder": "gpu"} if getattr(args, "png_decoder", "host") == "gpu" else {}))
    input_decoder = getattr(original, "decoder", None)
    lr_u8 = ops.resize_frames(original, res_in)[0] if res_in is not None else original
    files = {"inp": (args.inp, save(lr_u8, args.inp))}
    print(f"Downscaled image saved to: {args.inp}")
    h, w = int(lr_u8.shape[0]), int(lr_u8.shape[1])
    bicubic = ops.resize_frames(lr_u8, (h * args.scale, w * args.scale), resample="bicubic")
    files["bicubic"] = (BICUBIC_PATH, save(bicubic, BICUBIC_PATH))
    print(f"Bicubic image saved to: {BICUBIC_PATH}")

    model = importlib.import_module(f"models.{args.model}.model").TransformerModel()
    checkpoint = None
    if not args.no_checkpoint:
        checkpoint, _ = get_latest_checkpoint(args.checkpoint_dir or f"models/{args.model}/checkpoints")
        print(f"Loading checkpoint: {checkpoint}")
        model.load_state_dict(torch.load(checkpoint, map_location="cpu"))
    n_params = sum(p.numel() for p in model.parameters() if p.requires_grad)
    model = model.to(device).eval()
    with torch.no_grad():
        output = forward(model, ops.frames_to_tensor(lr_u8), args.scale)
    files["out"] = (args.out, save(output.contiguous(), args.out, out_bits))
    print(f"Upscaled image saved to: {args.out}")

    # a PNG is lossless: its pixels are the uint8 frame it was made from, so nothing is decoded for it (a 16-bit --out is scored on
    # the same 8-bit frame: the reference's metric is an 8-bit one)
    out_u8 = ops.tensor_to_frames(output.contiguous())[0] if file_format(args.out) == "png" else decode_image(files["out"][1], device)
    inp_u8 = lr_u8 if file_format(args.inp) == "png" else decode_image(files["inp"][1], device)
    scores = score(original, out_u8, inp_u8)
    scores = {k: {m: float(v) for m, v in d.items()} for k, d in scores.items()}
    print(f"Bicubic Scores:\tSSIM: {scores['bicubic']['ssim']:.4f}, PSNR: {scores['bicubic']['psnr']:.2f} dB")
    print(f"Model Scores:\tSSIM: {scores['model']['ssim']:.4f}, PSNR: {scores['model']['psnr']:.2f} dB")
    print(f"Model has {n_params} trainable parameters")
    sizes = {"inp": [h, w], "bicubic": [h * args.scale, w * args.scale], "out": [int(output.shape[2]), int(output.shape[3])]}
    return {"model": args.model, "checkpoint": checkpoint, "scale": args.scale, "res_in": args.res_in, "n_params": n_params,
            "quality": args.quality, "subsampling": args.subsampling, "scores": scores, "input_decoder": input_decoder,
            "files": {k: {"path": p, "format": file_format(p), "size": sizes[k], "bytes": len(d), "bits": out_bits if k == "out" else 8}
                      for k, (p, d) in files.items()}}


def main(argv=None):
    png_decoder, argv = take_png_decoder(argv)
    args = parse_args(argv)
    args.png_decoder = png_decoder
    record = run(args)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1, allow_nan=True)
    return record


if __name__ == "__main__":
    main()
