#!/usr/bin/env python
"""Per-frame latency of the frame path in any of its pixel formats: `speed_test.py`'s loop and flags, plus NV12 and P010 video surfaces.

    python frame_speed.py --pixfmt nv12 --graph                      # NV12 surface -> nv12_to_tensor -> model -> tensor_to_nv12
    python frame_speed.py --pixfmt nv12 --matrix bt601 --full_range
    python frame_speed.py --pixfmt p010 --matrix bt2020 --graph      # 10-bit surface -> p010_to_tensor -> model -> tensor_to_p010
    python frame_speed.py --graph                                    # rgb24: the frame speed_test.py times, for the same session

`speed_test.py` is one of the tools every change here is measured with and stays as it is; it speaks packed RGB / BGR bytes, which
is what a screen grab delivers.  A video decoder hands over NV12 (YUV 4:2:0: a Y plane and a plane of Cb/Cr pairs, DESIGN 3 "NV12 frames"), and this driver times that frame, eager
or as one hipGraph replay whose static input is the NV12 buffer.  Frames, model and weights are found as `speed_test.py` finds them
(its `load_frames` is used as it is); synthetic NV12 frames are random Y and UV bytes in one [3H/2][W] buffer, the RGB files of
`--data_dir` are converted once on the GPU with `ops.tensor_to_nv12`.  There is no Resize of NV12 surfaces and no byte order to
swap, so `--source_res` and `--bgr` are errors with `--pixfmt nv12`.  Prints one JSON line: `speed_test.py`'s fields plus "pixfmt"
and, for nv12 and p010, "matrix" and "range".

`--pixfmt p010` is the same frame in 10 bits (DESIGN 3 "P010 frames"): uint16 [3H/2][W] buffers with the code in the high ten bits of a
sample, `--matrix bt2020` in addition (an error with any other format), the same refusals of `--bgr` and `--source_res`.
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import speed_test  # noqa: E402
from speed_test import latency_summary, load_frames  # noqa: E402
from tools.utils import get_latest_checkpoint, resolutions  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser(description="Synced per-frame latency of the MI355X upscaler plugins on RGB24 or NV12 frames")
    ap.add_argument("--data_dir", type=str, default=None)
    ap.add_argument("--model", type=str, default="FastTransformer")
    ap.add_argument("--checkpoint_dir", type=str, default=None)
    ap.add_argument("--res_in", type=str, default="720", choices=list(resolutions))
    ap.add_argument("--res_out", type=int, nargs=2, default=(2160, 3840))
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--graph", action="store_true", help="capture one frame (pre-process, model, post-process) into a hipGraph and replay it")
    ap.add_argument("--bgr", action="store_true", help="rgb24 only: frames are BGR (screen grabs), output BGR")
    ap.add_argument("--source_res", type=str, default=None, choices=list(resolutions),
                    help="rgb24 only: frames arrive at this resolution and are resized to --res_in on the GPU (Pillow-exact)")
    ap.add_argument("--pixfmt", type=str, default="rgb24", choices=["rgb24", "nv12", "p010"],
                    help="pixel format of the frames in and out: packed RGB / BGR bytes, or NV12 (8-bit) / P010 (10-bit) video surfaces (YUV 4:2:0)")
    ap.add_argument("--matrix", type=str, default="bt709", choices=["bt601", "bt709", "bt2020"],
                    help="YCbCr matrix of --pixfmt nv12 / p010; bt2020 with p010 only")
    ap.add_argument("--full_range", action="store_true",
                    help="--pixfmt nv12 / p010: full-range Y and chroma (0..255 / 0..1023) instead of 16..235 / 16..240 (64..940 / 64..960)")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.pixfmt != "rgb24" and args.bgr:
        ap.error(f"--bgr is a byte order of --pixfmt rgb24; it does not apply to --pixfmt {args.pixfmt}")
    if args.pixfmt != "rgb24" and args.source_res:
        ap.error(f"--source_res needs --pixfmt rgb24: there is no Resize of {args.pixfmt.upper()} surfaces")
    if args.matrix == "bt2020" and args.pixfmt != "p010":
        ap.error("--matrix bt2020 needs --pixfmt p010")
    return args


def load_nv12_frames(args, device):
    """NV12 surfaces, one uint8 [3H/2][W] buffer per frame (Y rows on top, rows of Cb/Cr pairs below): the RGB files of --data_dir
    converted once on the GPU, or random Y and UV bytes."""
    from transformerupscaler_amd import ops
    h, w = resolutions[str(args.res_in)]
    if args.data_dir:
        rgb, source = load_frames(args, device)
        if source == "files":
            bufs = []
            for f in rgb:
                buf = torch.empty((h + h // 2, w), dtype=torch.uint8, device=device)
                ops.tensor_to_nv12(ops.frames_to_tensor(f), matrix=args.matrix, full_range=args.full_range, out=ops.nv12_planes(buf, h, w))
                bufs.append(buf)
            return bufs, "files"
    g = torch.Generator().manual_seed(1234)
    return [torch.randint(0, 256, (h + h // 2, w), dtype=torch.uint8, generator=g).to(device) for _ in range(min(args.frames, 8))], "synthetic"


def load_p010_frames(args, device):
    """P010 surfaces, one uint16 [3H/2][W] buffer per frame (Y rows on top, rows of Cb/Cr pairs below, the 10-bit code in the high
    bits of a sample): the RGB files of --data_dir converted once on the GPU, or random Y and UV codes."""
    from transformerupscaler_amd import ops
    h, w = resolutions[str(args.res_in)]
    if args.data_dir:
        rgb, source = load_frames(args, device)
        if source == "files":
            bufs = []
            for f in rgb:
                buf = torch.empty((h + h // 2, w), dtype=torch.uint16, device=device)
                ops.tensor_to_p010(ops.frames_to_tensor(f), matrix=args.matrix, full_range=args.full_range, out=ops.p010_planes(buf, h, w))
                bufs.append(buf)
            return bufs, "files"
    g = torch.Generator().manual_seed(1234)
    return [(torch.randint(0, 1024, (h + h // 2, w), dtype=torch.int32, generator=g) << 6).to(torch.uint16).to(device)
            for _ in range(min(args.frames, 8))], "synthetic"


def p010_frame_fn(model, res_out, args):
    """P010 surface [3H/2][W] on the GPU -> (y, uv) of the upscaled frame: the work of one frame."""
    from transformerupscaler_amd import ops
    h, w = resolutions[str(args.res_in)]

    def one_frame(buf):
        x = ops.p010_to_tensor(*ops.p010_planes(buf, h, w), matrix=args.matrix, full_range=args.full_range)
        return ops.tensor_to_p010(model(x, res_out=res_out), matrix=args.matrix, full_range=args.full_range)
    return one_frame


def nv12_frame_fn(model, res_out, args):
    """NV12 surface [3H/2][W] on the GPU -> (y, uv) of the upscaled frame: the work of one frame."""
    from transformerupscaler_amd import ops
    h, w = resolutions[str(args.res_in)]

    def one_frame(buf):
        x = ops.nv12_to_tensor(*ops.nv12_planes(buf, h, w), matrix=args.matrix, full_range=args.full_range)
        return ops.tensor_to_nv12(model(x, res_out=res_out), matrix=args.matrix, full_range=args.full_range)
    return one_frame


def frame_latency(one_frame, frames, n_frames, warmup, graph):
    """speed_test.frame_latency's loop around any `one_frame` (that function builds its RGB frame itself and takes no other; the
    rgb24 arm of this driver calls it as it is): one frame at a time, each timed to completion (`lat`) and to the
    return of the asynchronous call (`launch`); graph=True captures the frame once into a hipGraph and replays it, new frames being
    copied into the static input buffer.  Returns (last output, lat, launch, wall)."""
    g = static_in = static_out = None
    with torch.no_grad():
        for i in range(warmup):
            out = one_frame(frames[i % len(frames)])
        torch.cuda.synchronize()
        if graph:
            static_in = frames[0].clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                one_frame(static_in)
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                static_out = one_frame(static_in)
            torch.cuda.synchronize()

        def run(frame):
            if g is None:
                return one_frame(frame)
            static_in.copy_(frame)
            g.replay()
            return static_out

        lat, launch = [], []
        t_all = time.perf_counter()
        for i in range(n_frames):
            f = frames[i % len(frames)]
            t0 = time.perf_counter()
            out = run(f)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            launch.append(t1 - t0)
            lat.append(t2 - t0)
        wall = time.perf_counter() - t_all
    return out, lat, launch, wall


def load_model(args, device):
    model = importlib.import_module(f"models.{args.model}.model").TransformerModel().to(device)
    ckpt_dir = args.checkpoint_dir or f"models/{args.model}/checkpoints"
    if os.path.isdir(ckpt_dir) and any(f.endswith(".pth") for f in os.listdir(ckpt_dir)):
        path, epoch = get_latest_checkpoint(ckpt_dir)
        model.load_state_dict(torch.load(path, map_location=device))
        return model.eval(), f"{path} (epoch {epoch})"
    from transformerupscaler_amd import weights as W
    sd = {"ResidualTransformer": W.rt_deterministic_state_dict, "WindowTransformer": W.wt_deterministic_state_dict}.get(
        args.model, W.deterministic_state_dict)(0)
    model.load_state_dict(sd, strict=False)
    return model.eval(), "deterministic synthetic"


def main():
    args = parse_args()
    device = torch.device("cuda", 0)
    model, weights = load_model(args, device)
    planar = args.pixfmt != "rgb24"                                            # a 4:2:0 surface in two planes: nv12 or p010
    if args.pixfmt == "nv12":
        frames, source = load_nv12_frames(args, device)
        one_frame = nv12_frame_fn(model, tuple(args.res_out), args)
    elif args.pixfmt == "p010":
        frames, source = load_p010_frames(args, device)
        one_frame = p010_frame_fn(model, tuple(args.res_out), args)
    else:
        frames, source = load_frames(args, device)
    if planar:
        out, lat, launch, wall = frame_latency(one_frame, frames, args.frames, args.warmup, args.graph)
    else:
        out, lat, launch, wall = speed_test.frame_latency(model, frames, tuple(args.res_out), args.frames, args.warmup, args.graph, bgr=args.bgr,
                                                          lr_hw=resolutions[str(args.res_in)] if args.source_res else None)
    res = {"model": args.model, "weights": weights, "frames": args.frames, "source": source, "res_in": resolutions[str(args.res_in)],
           "res_out": list((out[0] if planar else out).shape[1:3]), "graph": bool(args.graph),
           "latency_ms": latency_summary(lat),
           "unsynced_launch_ms_mean": 1e3 * sum(launch) / len(launch), "images_per_sec": args.frames / wall,
           "pixfmt": args.pixfmt,
           "includes": (f"{args.pixfmt.upper()} surface -> RGB -> model -> {args.pixfmt.upper()} planes on the GPU (no PCIe)" if planar
                        else "uint8 HWC -> Resize (Pillow-exact) -> model -> uint8 HWC on the GPU (no PCIe)" if args.source_res
                        else "uint8 HWC -> model -> uint8 HWC on the GPU (no PCIe)")}
    if planar:
        res.update(matrix=args.matrix, range="full" if args.full_range else "limited")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
