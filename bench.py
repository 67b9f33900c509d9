#!/usr/bin/env python
"""Headline benchmark: FastTransformer 2x 720p->1080p bf16 inference, batch 8 per GPU (BASELINE.json
configs[1]); one "step" = one forward pass of the hot path over one batch of synthetic images that
are already resident in HBM.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus N ...          # N > 1 without RANK in the environment: starts the N ranks itself (below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

`--gpus N` with N > 1 and no RANK in the environment re-launches this script as N ranks under torch.distributed.run (a CHILD
process, started before anything here touches the GPU), relays the child's single JSON line and exits with its code; under
torchrun (RANK set) the script is one of the ranks.  At N > 1 the line carries `rccl`: what the live process group and the
gradient reducer report (ranks, backend, buckets, bytes all-reduced per step).

A plain run (the form above) times the headline inference only: set-up, `--warmup` steps, `--steps` timed steps, the
result line.  `--full` adds everything else the line has carried (the default `--mode both`: config-4 inference, the two
training steps, the overlay latency; the `sustained` loop; the CPU baselines and the fidelity against the oracle):
    python bench.py --gpus 1 --steps 20 --warmup 5 --full
`--dump-outputs DIR` writes what the last timed step of the headline returned as float32 .npy files (see dump_outputs); the
inputs and weights are seeded, so two builds run with the same arguments can be compared output for output.

Inference shards by images with no data-path collective (replicas, weak scaling).  Prints ONE JSON
line on rank 0 (contract in the task statement).  ``roofline`` describes the kernel with the largest
total time per forward, decided live from event timings on the launch stream: the whole-block kernel
(round 4: ``blocks_stream_kernel``, the six WindowTransformerBlocks of a forward in one launch; algorithmic
FLOPs = the window-attention GEMM set of SURVEY 8(d), 86.1 GF per image) or the 64->64 3x3
implicit-GEMM conv (conv2 + decoder_conv1, 2 launches per forward); the other one is reported as
``roofline_second`` -- since round 4 the two convs together (0.85 ms) outweigh the block launch (0.78 ms), so the
window-attention GEMM set, north_star's 0.40 target, is the SECOND entry.  ``sustained`` (--full) = the same forward loop
for >= 2 s after the timed steps with the shader clock it held.  ``cpu_baseline`` (--full) = the oracle (CPU restatement of the reference, "port") on a
bounded sample: forward, forward+backward (train.py:117-140), and the PSNR of the build's output
against the oracle's output for the same image (``psnr_vs_ref_db``, plus ΔPSNR against a synthetic HR).
"""
import argparse
import contextlib
import hashlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_BF16_PEAK_TFLOPS = 2500.0      # dense bf16, /opt/skills/guides/MI355X_MICROARCH.md
LR_H, LR_W, OUT = 720, 1280, (1080, 1920)
CONV64_FLOP_PER_IMAGE = 2.0 * LR_H * LR_W * 64 * 576        # SURVEY 8(a) row E2 (conv2 64->64): 67.95 GFLOP / image
ATTN_SET_FLOP_PER_IMAGE = 86.1e9                            # window-attention GEMM set (qkv, QK^T, PV, proj, fc1, fc2)


def _cores():
    cores = os.cpu_count() or 1
    try:
        cores = len(os.sched_getaffinity(0))
    except Exception:
        pass
    return min(cores, int(os.environ.get("TUP_CPU_THREADS", "16")))     # the 1-GPU box's CPU share is 16


def _psnr(a, b):
    import math
    mse = ((a.double() - b.double()) ** 2).mean().item()
    return 99.0 if mse == 0 else 10 * math.log10(1.0 / mse)


def cpu_baseline(model, dev):
    """Oracle (CPU restatement of the reference path) on the host cores, B=1, same synthetic input; its output doubles as
    the fidelity reference for the build's output on that image."""
    from oracle import fast_transformer_oracle as O
    from transformerupscaler_amd.weights import deterministic_state_dict
    cores = _cores()
    torch.set_num_threads(cores)
    sd = deterministic_state_dict(0)
    g = torch.Generator().manual_seed(1234)
    x = torch.rand((1, 3, LR_H, LR_W), generator=g)
    hr = torch.rand((1, 3) + OUT, generator=g)
    with torch.no_grad():
        y_ref = O.forward(sd, x, res_out=OUT)                 # warm-up (and the fidelity reference)
        n, t0 = 0, time.time()
        while n < 3 or (time.time() - t0 < 8.0 and n < 8):
            O.forward(sd, x, res_out=OUT)
            n += 1
        dt = time.time() - t0
        y = model(x.to(dev), res_out=OUT).cpu()
    # forward + backward of one train.py step (train.py:117-140: res_out = HR size, require_ratio=False, Resize, L1)
    gt = torch.Generator().manual_seed(4321)
    lr1 = torch.rand((1, 3, LR_H, LR_W), generator=gt)
    hr1 = torch.rand((1, 3) + OUT, generator=gt)
    O.train_step_grads(sd, lr1, hr1)                          # warm-up
    m, t1 = 0, time.time()
    while m < 2:
        O.train_step_grads(sd, lr1, hr1)
        m += 1
    dtt = time.time() - t1
    base = {"value": n / dt, "unit": "images/sec", "cores": cores, "kind": "port",
            "sample": f"{n} forward passes of 1 image 720x1280 -> 1080x1920 fp32 after 1 warm-up (torch CPU, {cores} threads)",
            "train_value": m / dtt, "train_sample": f"{m} forward+backward passes (train.py:117-140 step without Adam, L1 loss, dropout off) "
                                                    f"of 1 image after 1 warm-up, fp32, {cores} threads"}
    fidelity = {"psnr_vs_ref_db": _psnr(y, y_ref), "max_abs_vs_ref": (y - y_ref).abs().max().item(),
                "psnr_vs_hr_build_db": _psnr(y, hr), "psnr_vs_hr_ref_db": _psnr(y_ref, hr),
                "delta_psnr_vs_hr_db": _psnr(y, hr) - _psnr(y_ref, hr),
                "sample": "image 0 of the synthetic set (seed 1234), 720x1280 -> 1080x1920; HR = seeded uniform noise, so the absolute "
                          "PSNR-vs-HR is meaningless and only its difference (target <= 0.01 dB) is read"}
    return base, fidelity


def rt_cpu_baseline():
    """ResidualTransformer x6 training graph (forward + backward, L1) of the oracle on the host cores, one image."""
    from oracle import residual_transformer_oracle as R
    from transformerupscaler_amd.weights import rt_deterministic_state_dict
    import torch.nn.functional as F
    cores = _cores()
    torch.set_num_threads(cores)
    sd = rt_deterministic_state_dict(0)
    g = torch.Generator().manual_seed(9876)
    lr = torch.rand((1, 3, LR_H, LR_W), generator=g)
    hr = torch.rand((1, 3, LR_H * 6, LR_W * 6), generator=g)

    def step():
        leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        F.l1_loss(R.forward(leaf, lr, upscale_factor=6), hr).backward()

    step()
    n, t0 = 0, time.time()
    while n < 2:
        step(); n += 1
    dt = time.time() - t0
    return {"value": n / dt, "unit": "images/sec", "cores": cores, "kind": "port",
            "sample": f"{n} forward+backward passes of 1 image 720x1280 -> 4320x7680 fp32 (L1 loss, dropout off) after 1 warm-up"}


PROFILE_ROUND = "r04"          # the committed counter runs the line quotes (profiles/<round>_pmc_*.json)


def pmc_traffic(kernel_key: str, mode: str = "infer"):
    """HBM bytes per launch from the committed PMC run of this round, or None when the kernel's source changed since
    (the JSON records the sha256 of the .hip file it was measured on; a stale number is worse than none)."""
    name = f"{PROFILE_ROUND}_pmc_traffic_{mode}.json"
    try:
        with open(os.path.join(ROOT, "profiles", name)) as f:
            pm = json.load(f)
        ent = pm[kernel_key]
        with open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", ent["source"]), "rb") as f:
            sha = hashlib.sha256(f.read()).hexdigest()
        if sha != ent["source_sha256"]:
            return None, f"stale: {ent['source']} changed since profiles/{name} was measured"
        return ent["traffic_bytes_per_launch"], f"profiles/{name} (rocprofv3 FETCH_SIZE x2 + WRITE_SIZE, separate --pmc passes)"
    except Exception as e:          # noqa: BLE001
        return None, f"unavailable ({type(e).__name__})"


def pmc_mfma(kernel_key: str):
    """Counter-based matrix-pipe utilisation of the committed PMC run (profiles/<round>_pmc_mfma.json): SQ_VALU_MFMA_BUSY_CYCLES over
    every SIMD-cycle of the launch (rocprof's MfmaUtil expression) and the clock the chip held, or None when stale / absent."""
    try:
        with open(os.path.join(ROOT, "profiles", f"{PROFILE_ROUND}_pmc_mfma.json")) as f:
            ent = json.load(f)[kernel_key]
        with open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", ent["source"]), "rb") as f:
            if hashlib.sha256(f.read()).hexdigest() != ent["source_sha256"]:
                return None
        d = ent["derived"]
        return {"mfma_util": d.get("mfma_util"), "clock_GHz": d.get("clock_GHz_from_GRBM_GUI_ACTIVE"),
                "wait_any_share": d.get("sq_wait_any_share_of_wave_cycles"), "issue_stall_share": d.get("sq_wait_inst_any_share_of_wave_cycles"),
                "source": f"profiles/{PROFILE_ROUND}_pmc_mfma.json (rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE ..., own pass)"}
    except Exception:          # noqa: BLE001
        return None


def launcher_decision(gpus: int, environ) -> str:
    """"inline" = run the benchmark in this process (N = 1, or this process is already a rank of a torchrun job);
    "spawn" = start `gpus` ranks with torch.distributed.run and relay their line.  Pure host logic (tests/test_bench_launcher.py)."""
    if "RANK" in environ or "LOCAL_RANK" in environ or "TORCHELASTIC_RUN_ID" in environ:
        return "inline"
    return "spawn" if int(gpus) > 1 else "inline"


def launcher_command(gpus: int, argv, port: int):
    """The child command line: one process per GPU on this node, rendezvous on 127.0.0.1 (the container hostname may not resolve)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={int(gpus)}",
            "--master-addr", "127.0.0.1", "--master-port", str(int(port)), os.path.abspath(__file__)] + list(argv)


def _free_port() -> int:
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def spawn_ranks(gpus: int, argv) -> int:
    """Run the N-rank job as a child and relay its ONE JSON line (everything else the ranks print goes to stderr)."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")        # dmabuf IPC: RCCL across processes needs it on this pool
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = launcher_command(gpus, argv, _free_port())
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in proc.stdout.splitlines():
        if ln.startswith("{") and ln.rstrip().endswith("}"):
            line = ln
        else:
            sys.stderr.write(ln + "\n")
    if line is not None:
        print(line, flush=True)
    elif proc.returncode == 0:
        sys.stderr.write("bench.py: the ranks exited 0 without printing a JSON line\n")
        return 1
    return proc.returncode


def build_info():
    """Compiler that built the shipped library + the scratch guard's verdict (csrc/check_resources.py), if the build left it."""
    try:
        with open(os.path.join(ROOT, "transformerupscaler_amd", "csrc", "build", "resource_usage.json")) as f:
            ru = json.load(f)
        guarded = {k: v for k, v in ru["kernels"].items() if v.get("guarded_no_scratch")}
        return {"hipcc": ru.get("compiler"), "guarded_kernels": len(guarded),
                "guarded_scratch_bytes_max": max([v.get("scratch_bytes_per_lane", 0) for v in guarded.values()] + [0]),
                "whole_block_kernel_scratch_bytes": max([v.get("scratch_bytes_per_lane", 0) for k, v in guarded.items()
                                                         if "fused_qkv_attn_kernel<true, true, false>" in k] + [0])}
    except Exception as e:          # noqa: BLE001
        return {"hipcc": None, "note": f"build/resource_usage.json unavailable ({type(e).__name__})"}


DUMP_SAMPLE = 1 << 20          # elements of the seeded sample over the whole batch


def dump_outputs(y, out_dir):
    """--dump-outputs: the headline output of the last timed step, [B, 3, 1080, 1920], as float32 .npy files in out_dir:
    output_image0.npy = image 0 whole (24.9 MB), output_sample.npy = DUMP_SAMPLE elements of the whole batch at fixed seeded
    positions (4.2 MB; the full batch of 8 is 199 MB).  Both depend on the batch size only, not on the run."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    flat = y.detach().reshape(-1)
    idx = torch.randint(0, flat.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values
    np.save(os.path.join(out_dir, "output_image0.npy"), y[0].detach().float().cpu().numpy())
    np.save(os.path.join(out_dir, "output_sample.npy"), flat[idx.to(flat.device)].float().cpu().numpy())


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline does not need: the other modes (default --mode both), the sustained loop, "
                         "the CPU baselines and the fidelity against the oracle")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the headline output of the last timed step to DIR (dump_outputs)")
    ap.add_argument("--batch", type=int, default=8, help="inference images per GPU per step")
    ap.add_argument("--train-batch", type=int, default=4, help="training images per GPU per step (config 3: 32 / 8 GPUs)")
    ap.add_argument("--rt-batch", type=int, default=2, help="ResidualTransformer 6x training images per GPU per step (config 5: 16 / 8 GPUs)")
    ap.add_argument("--x4-batch", type=int, default=4, help="config 4 (4x 540p -> 2160p inference) images per GPU per step")
    ap.add_argument("--mode", choices=["infer", "train", "rt", "x4", "both"], default=None,
                    help="both = headline inference + 4x 540p inference (config 4) + FastTransformer training step + "
                         "ResidualTransformer 6x training step (default: infer, or both with --full)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines and the fidelity")
    ap.add_argument("--no-sustained", action="store_true", help="with --full: skip the 2-second sustained loop (profiling runs)")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.mode is None:
        args.mode = "both" if args.full else "infer"
    if args.dump_outputs and args.mode not in ("infer", "both"):
        ap.error("--dump-outputs writes the headline inference output: --mode infer or both")
    return args


def main():
    args = parse_args()

    if launcher_decision(args.gpus, os.environ) == "spawn":          # before any GPU call in this process
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1 or "RANK" in os.environ:          # under torchrun also at N = 1: the RCCL path is then the one N ranks run
        import torch.distributed as dist_mod
        dist = dist_mod
        # RCCL prints a version banner on (C-level) stdout when its communicator comes up; the contract is ONE JSON line
        # on stdout, so fd 1 points at stderr until the communicator exists
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(2, 1)
        try:
            dist.init_process_group("nccl", device_id=dev)
            dist.all_reduce(torch.zeros(1, device=dev))
            torch.cuda.synchronize()
        finally:
            sys.stdout.flush()
            os.dup2(saved, 1)
            os.close(saved)

    import importlib
    from transformerupscaler_amd import engine
    from transformerupscaler_amd.weights import deterministic_state_dict
    model = importlib.import_module("models.FastTransformer.model").TransformerModel()
    model.load_state_dict(deterministic_state_dict(0), strict=False)
    model = model.to(dev).eval()

    g = torch.Generator().manual_seed(1234 + rank)
    x = torch.rand((args.batch, 3, LR_H, LR_W), generator=g).to(dev)      # resident in HBM before timing

    events, block_events = [], []

    @contextlib.contextmanager
    def timer(name):
        if name not in ("conv2", "blocks") or not timing_on[0]:
            yield
            return
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()                       # current stream == the stream the kernel is launched on
        yield
        e.record()
        (events if name == "conv2" else block_events).append((s, e))

    timing_on = [False]
    engine.stage_timer = timer

    def barrier():
        if dist is not None:
            dist.barrier()

    def rccl_info(dp):
        """What the LIVE process group and this model's gradient reducer report (nothing here is a constant of the script)."""
        if dist is None or dp is None:
            return None
        red = dp.reducer
        return {"ranks": dist.get_world_size(), "backend": dist.get_backend(), "collective": "all_reduce(sum) per bucket on a side stream, issued from inside the backward",
                "buckets": len(red.bucket_ranges), "bucket_bytes": [4 * (b - a) for a, b in red.bucket_ranges],
                "bytes_per_step": 4 * red.total_floats, "buckets_issued_last_step": len(red.launched_order)}

    def run_train():
        """BASELINE.json configs[2]: 2x 720p->1080p bf16 training step (forward, antialiased resize to the HR
        size, L1, hand-written backward, RCCL gradient all-reduce overlapped with backward, Adam), 4 images/GPU."""
        from transformerupscaler_amd import harness
        from transformerupscaler_amd.dp import DataParallel
        tm = importlib.import_module("models.FastTransformer.model").TransformerModel()
        tm.load_state_dict(deterministic_state_dict(0), strict=False)
        tm = tm.to(dev).train()     # dropout p=0.1 active (model.py:80-82,127,132,150), as in train.py:109
        dp = DataParallel(tm, scale=2) if dist is not None else None
        opt = harness.make_optimizer(tm, 1e-4)
        gt = torch.Generator().manual_seed(4321 + rank)
        lr = torch.rand((args.train_batch, 3, LR_H, LR_W), generator=gt).to(dev)
        hr = torch.rand((args.train_batch, 3) + OUT, generator=gt).to(dev)
        for _ in range(max(args.warmup, 2)):
            harness.train_step(tm, opt, lr, hr)
        # (secondary modes: the faster of two repetitions of the timed region -- see run_x4; both in `repetitions_ms_per_step`)
        rep_s = []
        for rep in range(2):
            torch.cuda.synchronize()
            barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = harness.train_step(tm, opt, lr, hr)
            torch.cuda.synchronize()
            barrier()
            rep_s.append(time.perf_counter() - t0)
        dtt = min(rep_s)
        if dist is not None:
            t = torch.tensor([dtt], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dtt = float(t.item())
        rccl = rccl_info(dp)
        del dp
        return {"rccl": rccl, "metric": "images/sec, FastTransformer 2x 720p->1080p training step", "value": world * args.train_batch * args.steps / dtt,
                "unit": "images/sec", "ms_per_step": dtt / args.steps * 1e3, "images_per_gpu_per_step": args.train_batch,
                "repetitions_ms_per_step": [t_ / args.steps * 1e3 for t_ in rep_s],
                "global_batch": world * args.train_batch, "loss": float(loss.item()), "dropout": "p=0.1 (train mode, stateless hash masks)",
                "parallelism": f"dp{world}" + (" RCCL all-reduce of 17.9 MB fp32 grads in ~6 MB buckets, overlapped with backward" if world > 1 else ""),
                "optimizer": "Adam lr 1e-4 (transformerupscaler_amd.optim.Adam: torch.optim.Adam with the update in one HIP launch)", "loss_fn": "L1 vs synthetic HR after antialiased resize 1440x2560 -> 1080x1920"}

    def run_rt_train():
        """BASELINE.json configs[4]: ResidualTransformer 6x (720p -> 4320x7680) bf16 training step, 2 images/GPU, DP."""
        from transformerupscaler_amd.autograd import l1_loss
        from transformerupscaler_amd.dp import DataParallel
        from transformerupscaler_amd.weights import rt_deterministic_state_dict
        torch.cuda.empty_cache()
        tm = importlib.import_module("models.ResidualTransformer.model").TransformerModel()
        tm.load_state_dict(rt_deterministic_state_dict(0))
        tm = tm.to(dev).train()                     # dropout p=0.1 on attention probabilities and MLP output
        dp = DataParallel(tm) if dist is not None else None
        from transformerupscaler_amd import harness
        opt = harness.make_optimizer(tm, 1e-4)
        gt = torch.Generator().manual_seed(9876 + rank)
        lr = torch.rand((args.rt_batch, 3, LR_H, LR_W), generator=gt).to(dev)
        hr = torch.rand((args.rt_batch, 3, LR_H * 6, LR_W * 6), generator=gt).to(dev)

        def step():
            opt.zero_grad(set_to_none=True)
            loss = l1_loss(tm(lr, upscale_factor=6), hr, fuse_into_model_backward=True)     # nn.L1Loss (train.py:103,132)
            loss.backward()
            opt.step()
            return loss.detach()

        steps = max(1, min(args.steps, 10))
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        barrier()
        # event timing of the attention launches (the dominant kernels of this step) on the launch stream
        from transformerupscaler_amd import autograd_rt
        attn_ev = {"rt_attn_fwd": [], "rt_attn_bwd": []}

        @contextlib.contextmanager
        def rt_timer(name):
            s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s_.record()
            yield
            e_.record()
            attn_ev[name].append((s_, e_))

        rep_s = []
        for rep in range(2):
            torch.cuda.synchronize()
            barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = step()
            torch.cuda.synchronize()
            barrier()
            rep_s.append(time.perf_counter() - t0)
        dtt = min(rep_s)
        autograd_rt.stage_timer = rt_timer          # three more steps, outside the timed region, with the events armed
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        autograd_rt.stage_timer = None
        fwd_ms = sum(a.elapsed_time(b) for a, b in attn_ev["rt_attn_fwd"]) / max(len(attn_ev["rt_attn_fwd"]), 1)
        bwd_ms = sum(a.elapsed_time(b) for a, b in attn_ev["rt_attn_bwd"]) / max(len(attn_ev["rt_attn_bwd"]), 1)
        # algorithmic FLOPs of the attention GEMMs per TransformerBlock (models/ResidualTransformer/model.py:40-50, hd = 16, 8 heads,
        # N = 3600): forward QK^T + PV = 2 products, backward dq pass recomputes S and forms dP, dQ (3), dkv pass recomputes S
        # and forms dP, dV, dK (4) -> 9 products of 2 * N^2 * 16 FLOP per head and image
        unit = 2.0 * 3600 * 3600 * 16 * 8 * args.rt_batch
        trio_ms = fwd_ms + bwd_ms
        rt_roof = {"bound": "valu",
                   "kernel": "rt_attention_kernel + rt_attn_bwd_dq_kernel + rt_attn_bwd_dkv_kernel (flash-style attention of one TransformerBlock, "
                             "forward and backward, N = 3600 tokens, 8 heads x 16)",
                   "achieved": 9 * unit / (trio_ms * 1e-3) / 1e12 if trio_ms > 0 else 0.0, "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                   "frac": (9 * unit / (trio_ms * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFLOPS) if trio_ms > 0 else 0.0,
                   "ms_fwd_per_block": fwd_ms, "ms_bwd_per_block": bwd_ms, "blocks_per_step": 8, "launch_groups_timed": len(attn_ev["rt_attn_fwd"]),
                   "algorithmic_flop_per_block": 9 * unit, "traffic": None,
                   "note": "K = 16 products: 64 MFMA FLOP per score against an exp, the softmax arithmetic and a dropout hash per score on the VALU "
                           "-- the trio is VALU-issue-bound, not MFMA-bound; frac is against the dense bf16 MFMA peak for comparability"}
        if dist is not None:
            t = torch.tensor([dtt], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dtt = float(t.item())
        rccl = rccl_info(dp)
        del dp
        return {"roofline": rt_roof, "rccl": rccl, "metric": "images/sec, ResidualTransformer 6x 720p->4320x7680 training step", "value": world * args.rt_batch * steps / dtt,
                "unit": "images/sec", "ms_per_step": dtt / steps * 1e3, "steps": steps, "images_per_gpu_per_step": args.rt_batch,
                "repetitions_ms_per_step": [t_ / steps * 1e3 for t_ in rep_s],
                "global_batch": world * args.rt_batch, "loss": float(loss.item()), "dropout": "p=0.1 (train mode, stateless hash masks)",
                "parallelism": f"dp{world}" + (" RCCL all-reduce of 12.8 MB fp32 grads, overlapped with backward" if world > 1 else ""),
                "optimizer": "Adam lr 1e-4 (transformerupscaler_amd.optim.Adam: torch.optim.Adam with the update in one HIP launch)", "loss_fn": "L1 vs synthetic 4320x7680 HR"}

    def run_x4():
        """BASELINE.json configs[3]: 4x 540x960 -> 2160x3840 bf16 inference, batch 4 per GPU (two-stage branch A: explicit
        64->256 conv + PixelShuffle at 540p, then the composed 5x5 at 1080p; reflect-padded 544-row token grid)."""
        torch.cuda.empty_cache()          # a clean allocator for this mode's warm-up (the previous mode's block sizes do not fit this one's)
        gx = torch.Generator().manual_seed(777 + rank)
        xx = torch.rand((args.x4_batch, 3, 540, 960), generator=gx).to(dev)
        steps = max(1, min(args.steps, 10))
        with torch.no_grad():
            for _ in range(3):
                yy = model(xx, upscale_factor=4)          # bound to the same name as in the timed loop: the previous output stays alive
            torch.cuda.synchronize()                      # during the next call there, so the allocator needs TWO 0.4 GB output blocks --
                                                          # an unbound warm-up left the second one to a hipMalloc inside the timed region
            # Two repetitions of the timed region, the faster one reported (both in `diagnostics`): on some boxes ONE step of a
            # repetition stalls for 50-90 ms with no allocator activity (seen twice in this secondary mode: step_ms_max 85 ms beside a
            # 2.4 ms median); the headline metric above keeps the contract's single region.
            reps = []
            for rep in range(2):
                barrier()
                torch.cuda.synchronize()
                ms0 = torch.cuda.memory_stats()
                evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
                t0 = time.perf_counter()
                evs[0].record()
                for i in range(steps):
                    yy = model(xx, upscale_factor=4)
                    evs[i + 1].record()
                torch.cuda.synchronize()
                barrier()
                dt_rep = time.perf_counter() - t0
                ms1 = torch.cuda.memory_stats()
                # diagnostics (not the metric): GPU time of every step and what the caching allocator did inside the timed region -- a
                # step that has to go to hipMalloc / hipFree (0.4 GB outputs) stalls for milliseconds on some boxes
                per_step = [evs[i].elapsed_time(evs[i + 1]) for i in range(steps)]
                reps.append((dt_rep, {"ms_per_step": dt_rep / steps * 1e3, "step_ms_min": min(per_step), "step_ms_median": sorted(per_step)[steps // 2],
                                      "step_ms_max": max(per_step),
                                      "device_allocs_in_timed_region": ms1.get("num_device_alloc", 0) - ms0.get("num_device_alloc", 0),
                                      "device_frees_in_timed_region": ms1.get("num_device_free", 0) - ms0.get("num_device_free", 0),
                                      "alloc_retries_in_timed_region": ms1.get("num_alloc_retries", 0) - ms0.get("num_alloc_retries", 0)}))
            dtt = min(r[0] for r in reps)
            alloc_diag = dict(min(reps, key=lambda r: r[0])[1])
            alloc_diag["repetitions"] = [r[1] for r in reps]
            alloc_diag["reported"] = "the faster of two repetitions of the timed region"
        assert tuple(yy.shape) == (args.x4_batch, 3, 2160, 3840)
        if dist is not None:
            t = torch.tensor([dtt], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dtt = float(t.item())
        flop = 950.2e9 * args.x4_batch                      # 950.2 GF forward per image as the reference computes it
        return {"metric": "images/sec, FastTransformer 4x 540p->2160p inference", "value": world * args.x4_batch * steps / dtt,
                "unit": "images/sec", "ms_per_step": dtt / steps * 1e3, "steps": steps, "images_per_gpu_per_step": args.x4_batch,
                "reference_gflop_per_image": 950.2, "diagnostics": alloc_diag,
                "reference_flop_rate_tflops": flop / (dtt / steps) / 1e12,
                "note": "reference-FLOP rate = the reference's 950.2 GF per image / time; the build executes fewer (the last up-conv + "
                        "PixelShuffle + up1_conv run as one composed 5x5 conv)"}

    def run_overlay():
        """SURVEY 8(f) rank 4, the live-overlay latency path (reference app_overlay.py:337-420): ONE uint8 720p frame resident on the
        GPU -> ToTensor -> model(res_out=(2160, 3840)) -> uint8 frame, per frame, synchronised; eager and as one hipGraph replay."""
        import speed_test
        go = torch.Generator().manual_seed(4242 + rank)
        frames = [torch.randint(0, 256, (LR_H, LR_W, 3), dtype=torch.uint8, generator=go).to(dev) for _ in range(4)]
        res = {"metric": "latency per frame, FastTransformer 720p -> 2160p (3x), batch 1, uint8 frame in -> uint8 frame out on the GPU",
               "unit": "ms", "frames": 60}
        for key, graph in (("eager", False), ("graph", True)):
            out, lat, launch, wall = speed_test.frame_latency(model, frames, (2160, 3840), 60, 5, graph, bgr=True)
            res[key] = dict(speed_test.latency_summary(lat), unsynced_launch_ms_mean=1e3 * sum(launch) / len(launch),
                            frames_per_sec=60 / wall)
        assert tuple(out.shape) == (1, 2160, 3840, 3) and out.dtype == torch.uint8
        res["note"] = ("p50 / p99 of host wall time from handing the frame over to torch.cuda.synchronize() returning; `graph` = "
                       "speed_test.py --graph (pre-process + model + post-process captured once, one hipGraphLaunch per frame)")
        return res

    overlay_result = run_overlay() if args.mode == "both" and world == 1 else None
    x4_result = run_x4() if args.mode in ("x4", "both") else None
    if args.mode == "x4":
        if rank == 0:
            out = dict(x4_result)
            out.update({"n_gpus": world, "warmup": 3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                        "dtype": "bf16", "data": "synthetic",
                        "config": {"workload": "FastTransformer 4x 540x960 -> 2160x3840 bf16 inference (BASELINE.json configs[3])"}})
            print(json.dumps(out), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        return
    train_result = run_train() if args.mode in ("train", "both") else None
    rt_result = run_rt_train() if args.mode in ("rt", "both") else None
    if args.mode == "rt":
        if rank == 0:
            out = dict(rt_result)
            out.update({"n_gpus": world, "warmup": 2, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                        "dtype": "bf16", "data": "synthetic",
                        "config": {"workload": "ResidualTransformer 6x 720x1280 -> 4320x7680 bf16 training step (BASELINE.json configs[4])"}})
            print(json.dumps(out), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        return
    if args.mode == "train":
        if rank == 0:
            out = dict(train_result)
            out.update({"n_gpus": world, "steps": args.steps, "warmup": args.warmup, "higher_is_better": True,
                        "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
                        "config": {"workload": "FastTransformer 2x 720x1280 -> 1080x1920 bf16 training step (BASELINE.json configs[2])"}})
            print(json.dumps(out), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        return

    with torch.no_grad():
        y = None
        for _ in range(args.warmup):
            y = model(x, res_out=OUT)          # same binding as the timed loop (two output blocks alive across a call, see run_x4)
        torch.cuda.synchronize()
        barrier()
        timing_on[0] = True
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            y = model(x, res_out=OUT)
        torch.cuda.synchronize()
        barrier()
        dt = time.perf_counter() - t0
    timing_on[0] = False
    assert tuple(y.shape) == (args.batch, 3) + OUT
    if args.dump_outputs and rank == 0:
        dump_outputs(y, args.dump_outputs)

    # What the hardware sustains: the same loop for >= 2 s, OUTSIDE the headline number (the 20 timed steps are 0.07 s, a stretch in
    # which the chip still holds its boost clock).  The shader clock of the stretch = shader cycles / 100 MHz ticks between two one-wave
    # probes in stream order (MI355X_MICROARCH.md, 'DVFS give-back' item 6).
    sustained = None
    if rank == 0 and args.full and not args.no_sustained:
        from transformerupscaler_amd import ops as _ops
        with torch.no_grad():
            torch.cuda.synchronize()
            p0 = _ops.clock_probe()
            ts, n_sus = time.perf_counter(), 0
            while True:
                for _ in range(20):
                    y = model(x, res_out=OUT)
                n_sus += 20
                torch.cuda.synchronize()
                if time.perf_counter() - ts >= 2.0:
                    break
            p1 = _ops.clock_probe()
            torch.cuda.synchronize()
            dts = time.perf_counter() - ts
        dcy, dtk = int(p1[0] - p0[0]), int(p1[1] - p0[1])
        sustained = {"seconds": dts, "steps": n_sus, "images_per_sec": args.batch * n_sus / dts, "ms_per_step": dts / n_sus * 1e3,
                     "clock_GHz": (dcy / dtk * 0.1) if dtk > 0 else None,
                     "clock_source": "s_memtime / s_memrealtime between two one-wave probes around the loop (tup_clock_probe)"}

    if dist is not None:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())

    conv_ms = sum(s.elapsed_time(e) for s, e in events) / max(len(events), 1)                  # one conv2 launch
    blocks_ms = sum(s.elapsed_time(e) for s, e in block_events) / max(len(block_events), 1)     # the 6 whole-block launches of a forward
    from transformerupscaler_amd import engine as _engine
    n_block_launch = 1 if _engine.blocks_in_one_launch else 6
    blk_ms = blocks_ms / n_block_launch
    attn_tf = ATTN_SET_FLOP_PER_IMAGE * args.batch / (blocks_ms * 1e-3) / 1e12 if blocks_ms > 0 else 0.0
    conv_tf = CONV64_FLOP_PER_IMAGE * args.batch / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else 0.0
    nwin = args.batch * 12 * 20                    # 96x160 token grid -> 12 x 20 windows per 720p image
    conv_traffic, conv_src = pmc_traffic("conv64")
    if args.batch != 8:
        conv_traffic = None
    streamed = bool(_engine.stream_blocks and n_block_launch == 1 and nwin >= _engine.STREAM_MIN_WINDOWS)
    blk_key = "stream_block" if streamed else "fused_block"
    blk_traffic, blk_src = pmc_traffic(blk_key)
    if args.batch != 8:
        blk_traffic = None
    roof_block = {"bound": "mfma",
                  "kernel": ("blocks_stream_kernel (csrc/block_stream.hip, v_mfma_f32_32x32x16; " if streamed else "fused_qkv_attn_kernel<true,true> (") +
                            "whole WindowTransformerBlocks: norm1 + qkv + window attention + proj + residual + "
                            "norm2 + fc1 + GELU + fc2 + residual; " + ("the 6 blocks of a forward in ONE launch)" if n_block_launch == 1
                                                                       else "one block per launch, 6 launches per forward)"),
                  "blocks_per_launch": 6 // n_block_launch, "ms_per_block": blocks_ms / 6,
                  "achieved": attn_tf, "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": attn_tf / MFMA_BF16_PEAK_TFLOPS,
                  "traffic": blk_traffic, "traffic_source": blk_src, "counters": pmc_mfma(blk_key),
                  "algorithmic_flop_per_launch": ATTN_SET_FLOP_PER_IMAGE * args.batch / n_block_launch,
                  # SURVEY 8(d)'s per-block figure (the fp32 residual stream read once + written once) x the blocks one launch runs
                  "algorithmic_bytes": nwin * 64 * 192 * 4 * 2 * (6 // n_block_launch),
                  # ... and what ONE launch of six blocks needs at the least: the stream in once and out once, the weights once
                  "algorithmic_bytes_one_launch_minimum": nwin * 64 * 192 * 4 * 2 + 6 * 885 * 1024,
                  "ms_per_launch": blk_ms, "total_ms_per_forward": blocks_ms, "launches_timed": len(block_events) * n_block_launch,
                  "note": "algorithmic FLOPs = SURVEY 8(d)'s window-attention GEMM set (qkv, QK^T, PV, proj, fc1, fc2 = 86.1 GF per image); "
                          "LayerNorm / softmax / GELU run inside the same launches and are not counted; north_star target frac >= 0.40"}
    roof_conv = {"bound": "mfma", "kernel": "conv_c64_persistent_kernel<4,0,3> (conv2 64->64 3x3 implicit GEMM; same kernel as decoder_conv1; 2 launches per forward)",
                 "achieved": conv_tf, "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": conv_tf / MFMA_BF16_PEAK_TFLOPS,
                 "traffic": conv_traffic, "traffic_source": conv_src, "counters": pmc_mfma("conv64"),
                 "algorithmic_flop_per_launch": CONV64_FLOP_PER_IMAGE * args.batch,
                 "algorithmic_bytes": 2 * args.batch * LR_H * LR_W * 64 * 2,
                 "ms_per_launch": conv_ms, "total_ms_per_forward": 2 * conv_ms, "launches_timed": len(events)}
    # the same launch against the HBM roof (8 TB/s, MI355X_MICROARCH.md): by the ablations of DESIGN 5c its memory side alone (DMA + stores,
    # no K loop) takes 85 % of the kernel's time, i.e. the launch sits nearer this roof than the MFMA one
    conv_gbps = roof_conv["algorithmic_bytes"] / (conv_ms * 1e-3) / 1e9 if conv_ms > 0 else 0.0
    roof_conv["hbm"] = {"achieved": conv_gbps, "peak": 8000.0, "unit": "GB/s", "frac": conv_gbps / 8000.0,
                        "note": "algorithmic bytes (one read + one write of the 64-channel bf16 map) / the same launch time"}
    dominant, second = (roof_block, roof_conv) if blocks_ms >= 2 * conv_ms else (roof_conv, roof_block)

    if rank == 0:
        out = {
            "metric": "images/sec, FastTransformer 2x 720p->1080p inference",
            "value": world * args.batch * args.steps / dt,
            "unit": "images/sec",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "bf16", "data": "synthetic",
            "config": {"workload": "FastTransformer 2x 720x1280 -> res_out 1080x1920, bf16 inference, "
                                   f"batch {args.batch} per GPU (BASELINE.json configs[1])",
                       "images_per_gpu_per_step": args.batch, "parallelism": f"replicas x{world}",
                       "weights": "deterministic synthetic (transformerupscaler_amd.weights, seed 0)"},
            "roofline": dominant,
            "roofline_second": second,
            "sustained": sustained,
        }
        out["build"] = build_info()
        if train_result is not None:
            out["train"] = train_result
            # the number north_star's ">= 6x at 8 GPUs" is about, at the top level next to the replica-inference `value`
            out["train_images_per_sec"] = train_result.get("value")
            out["train_ms_per_step"] = train_result.get("ms_per_step")
            if train_result.get("rccl") is not None:
                out["rccl"] = train_result["rccl"]          # the FastTransformer training step's reducer (configs[2])
        if rt_result is not None:
            out["rt_train"] = rt_result
        if x4_result is not None:
            out["x4"] = x4_result
        if overlay_result is not None:
            out["overlay"] = overlay_result
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"], out["fidelity"] = cpu_baseline(model, dev)
            out["psnr_vs_ref_db"] = out["fidelity"]["psnr_vs_ref_db"]
            if train_result is not None:
                train_result["cpu_baseline"] = {"value": out["cpu_baseline"]["train_value"], "unit": "images/sec", "cores": out["cpu_baseline"]["cores"],
                                                "kind": "port", "sample": out["cpu_baseline"]["train_sample"]}
            if rt_result is not None:
                rt_result["cpu_baseline"] = rt_cpu_baseline()
        elif args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = None     # measured on rank 0 at N=1 only (see BENCH at n_gpus=1)
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
