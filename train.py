#!/usr/bin/env python
"""Training driver with the reference's train.py surface (train.py:41-194): the model plugin ``models/<model>/model.py`` is
trained on the samples of ``--data_dir`` with L1 loss and Adam, resumed from and checkpointed to
``models/<model>/checkpoints/model_epoch_<N>.pth``.

    python train.py --data_dir images/training_set --model FastTransformer --epochs 10
    torchrun --nproc_per_node 8 train.py --data_dir images/training_set            # data parallel, one process per GPU

A step is the reference's (train.py:110-146): a batch is a list of (lr, hr) samples of different sizes and scales
(``transformerupscaler_amd.data.PairDataset``: ten scale pairs per image resolving to x2, x3, x4 and x6), each sample counts
equally in the loss, and one optimizer step follows.  It runs as ``harness.train_step_samples``: equal-shaped samples of a batch
are batched (``--no_group`` runs them one by one as the reference does), each group's backward runs at once, and the gradients
are accumulated in one launch per backward.

What differs from the reference driver:

* ``--data_dir`` is required.  The reference's online dataset is not built; nothing here touches a network.
* ``--model`` defaults to ``FastTransformer`` (the reference's default names a model its own tree does not have).
* Images are decoded once on the host and resized on the GPU: no DataLoader worker processes.  The path computes in bf16 inside
  with fp32 parameters: no autocast, no GradScaler.
* The loss is read back only when a line is printed and at the end of an epoch.
* ``--l1 / --mse / --ssim`` weights train on ``losses.QualityLoss`` instead of pure L1; ``--deterministic`` makes the run
  bit-reproducible (``ops.deterministic_mode``); ``--seed`` seeds the shuffle and dropout; ``--max_steps`` ends the run early (a
  checkpoint of the unfinished epoch is still written); ``--pairs "96x96:192x192,..."`` replaces the scale-pair table;
  ``--cache_gb`` bounds the decoded-image cache; ``--save_optimizer`` writes Adam's state beside the weights and resumes from
  it; ``--json PATH`` writes a record of the run.
* ``--weight_decay W`` decays the weights inside the fused step (Adam's L2 form; ``--adamw``: AdamW's decoupled form).
  ``--clip_grad_norm C`` clips the step's global gradient norm to C and ``--skip_nonfinite`` skips a step whose gradients hold an
  inf or a NaN (what the reference's GradScaler does), both decided on the GPU without a host synchronisation; ``p.grad`` keeps
  the unclipped gradient.  ``--warmup_steps N`` / ``--lr_schedule cosine`` / ``--lr_min`` set the learning rate per optimizer
  step (`lr_at`).  With any of these a step line and its ``--json`` entry also carry ``lr`` and ``grad_norm``, and the record
  ``guard: {applied, clipped, skipped}``.
* ``--patch_size N`` trains on random patches instead of whole frames (``transformerupscaler_amd.data.PatchSampler``): every
  sample is an ``N x N`` LR patch and its ``N*s x N*s`` HR crop, s drawn from ``--patch_scales`` (default 2,3,4,6), with one of the
  8 flip / rotate variants (``--no_augment``: none); a step's samples are built in one launch per distinct scale.
  ``--patches_per_epoch`` sets the epoch length (default: the whole-frame dataset's).  Sample g of a run is a function of
  ``(--seed, g)`` alone, so resumed runs and ranks need no generator state.  ``--pairs`` does not apply; ResidualTransformer (fixed
  720x1280 input) cannot train on patches.  The ``--json`` record gains ``patch``.
* ``--degrade`` (with ``--patch_size``) passes every LR patch through blur, noise and a JPEG round trip after the clean downscale
  (``transformerupscaler_amd.data.DegradeSpec``, one ``ops.degrade`` launch per distinct scale; HR is untouched): with probability
  0.5 a Gaussian blur of sigma 0.2-1.5 pixels, with 0.5 noise of sigma 1-10 in 8-bit units (grey in 0.4 of those cases), with 0.7
  a 4:4:4 JPEG round trip at quality 30-95.  ``--degrade_blur LO,HI``, ``--degrade_noise LO,HI``, ``--degrade_jpeg LO,HI`` and
  ``--degrade_prob PB,PN,PJ`` set the ranges and the three probabilities, and each implies ``--degrade``.  ``--degrade_jpeg_420 P``
  (default 0; implies ``--degrade``) makes that share of the JPEG round trips 4:2:0, chroma subsampled as most JPEG files are:
  chroma averaged over 2 x 2 pixels, quantised in 16 x 16 pixel blocks and smeared back by the decoder's triangle filter.  The record
  of sample g is a function of ``(--seed, g)``, from a stream of its own.  The ``--json`` record gains ``degrade`` (the spec).
* ``--ema_decay D`` keeps an exponential moving average of the weights inside the fused optimizer step (``--ema_warmup``: timm's
  warm-up of the decay); a step skipped by ``--skip_nonfinite`` does not move it.  Every checkpoint then also writes
  ``<checkpoint_dir>/ema/model_epoch_<N>.pth`` (the weight file's format: ``ab_test.py --checkpoint_dir_a .../ema`` loads it) and a
  sidecar ``ema/ema_epoch_<N>.pt``; a resumed run loads both, or restarts the average from the loaded weights and says so.
  The sidecar also holds the model's dropout call count, so that with ``--save_optimizer`` a resumed single-process run continues
  bit for bit where the saved one stood.
* ``--val_dir DIR`` scores a held-out directory after every ``--val_interval`` epochs (``harness.evaluate``: the training step's
  forward on full images under the pairs of ``--val_pairs``, default ``--pairs`` or the dataset's ten; ``--val_images K``: the
  first K files): L1, MSE, PSNR, SSIM in one printed line and a ``val`` entry of the ``--json`` record.  With ``--ema_decay`` the
  averaged weights are scored (``--val_both``: the raw ones too).  ``--keep_best {psnr,ssim,l1}`` keeps
  ``<checkpoint_dir>/best/model_epoch_<N>.pth`` of the best validated weights so far (record ``best``).  The validation set takes
  half of the ``--cache_gb`` budget.
* ``--traceback`` is accepted; the reference's traceback window is not available here.
* With ``WORLD_SIZE > 1`` in the environment (torchrun) the run is data parallel: every rank shuffles with the same seed and
  trains ``batch[rank::world]``; the gradients of a step are all-reduced once.
"""
import argparse
import importlib
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    p = argparse.ArgumentParser(description="Train the TransformerModel for image upscaling")
    p.add_argument("--data_dir", type=str, default=None, help="Directory containing the training images (.png); required")
    p.add_argument("--batch_size", type=int, default=6, help="Samples per optimizer step")
    p.add_argument("--epochs", type=int, default=10, help="Number of training epochs")
    p.add_argument("--lr", type=float, default=1e-4, help="Learning rate of Adam")
    p.add_argument("--log_interval", type=int, default=1, help="Log the loss every N steps")
    p.add_argument("--checkpoint_interval", type=int, default=1, help="Save a checkpoint every N epochs")
    p.add_argument("--model", type=str, default="FastTransformer", help="Model name (models/{model}/model.py)")
    p.add_argument("--checkpoint_dir", type=str, default=None, help="Checkpoint directory (default: models/{model}/checkpoints/)")
    p.add_argument("--traceback", action="store_true", help="Accepted for compatibility; the traceback window is not available")
    p.add_argument("--l1", type=float, default=1.0, help="Weight of the L1 term of the loss")
    p.add_argument("--mse", type=float, default=0.0, help="Weight of the MSE term of the loss")
    p.add_argument("--ssim", type=float, default=0.0, help="Weight of the (1 - SSIM) term of the loss")
    p.add_argument("--deterministic", action="store_true", help="Bit-reproducible training (ops.deterministic_mode)")
    p.add_argument("--seed", type=int, default=0, help="Seed of the shuffle and of dropout")
    p.add_argument("--max_steps", type=int, default=None, help="Stop after this many optimizer steps of this invocation")
    p.add_argument("--pairs", type=str, default=None, help='Scale pairs "LRHxLRW:HRHxHRW,..." in place of the dataset\'s ten')
    p.add_argument("--cache_gb", type=float, default=2.0, help="Bound of the decoded-image cache on the GPU, in GiB")
    p.add_argument("--save_optimizer", action="store_true", help="Write / resume Adam's state beside the weights")
    p.add_argument("--no_group", action="store_true", help="Run every sample at batch 1, as the reference does")
    p.add_argument("--json", type=str, default=None, help="Write a record of the run to this path")
    p.add_argument("--weight_decay", type=float, default=0.0, help="Weight decay, inside the fused optimizer step")
    p.add_argument("--adamw", action="store_true", help="AdamW: decoupled weight decay (p *= 1 - lr * wd) instead of Adam's L2 form")
    p.add_argument("--clip_grad_norm", type=float, default=None, help="Clip the global gradient norm of a step to this value")
    p.add_argument("--skip_nonfinite", action="store_true", help="Skip an optimizer step whose gradients hold an inf or a NaN")
    p.add_argument("--warmup_steps", type=int, default=0, help="Linear learning-rate warm-up over this many optimizer steps")
    p.add_argument("--lr_schedule", choices=("constant", "cosine"), default="constant", help="Learning rate after the warm-up")
    p.add_argument("--lr_min", type=float, default=0.0, help="Final learning rate of the cosine schedule")
    p.add_argument("--patch_size", type=int, default=None, help="Train on random patches: the LR patch side (HR side = this x scale)")
    p.add_argument("--patch_scales", type=str, default="2,3,4,6", help="Scales the patches are drawn from (with --patch_size)")
    p.add_argument("--no_augment", action="store_true", help="No flip / rotate variants of the patches (with --patch_size)")
    p.add_argument("--patches_per_epoch", type=int, default=None, help="Samples per epoch with --patch_size (default: the dataset's)")
    p.add_argument("--degrade", action="store_true", help="Degrade the LR patches: blur, noise, JPEG round trip (with --patch_size)")
    p.add_argument("--degrade_blur", type=str, default=None, help="Blur sigma range LO,HI in pixels, at most 3 (default 0.2,1.5; implies --degrade)")
    p.add_argument("--degrade_noise", type=str, default=None, help="Noise sigma range LO,HI in 8-bit units (default 1,10; implies --degrade)")
    p.add_argument("--degrade_jpeg", type=str, default=None, help="JPEG quality range LO,HI in 1..100 (default 30,95; implies --degrade)")
    p.add_argument("--degrade_prob", type=str, default=None, help="Probabilities PB,PN,PJ of blur, noise, JPEG (default 0.5,0.5,0.7; implies --degrade)")
    p.add_argument("--degrade_jpeg_420", type=str, default=None, help="Share P of the JPEG round trips that are 4:2:0 instead of 4:4:4 (default 0; implies --degrade)")
    p.add_argument("--ema_decay", type=float, default=None, help="Keep an exponential moving average of the weights with this decay")
    p.add_argument("--ema_warmup", action="store_true", help="Warm the EMA decay up: min(decay, (1 + n) / (10 + n)) (with --ema_decay)")
    p.add_argument("--val_dir", type=str, default=None, help="Directory of held-out images (.png) scored after an epoch")
    p.add_argument("--val_interval", type=int, default=1, help="Validate every N epochs (with --val_dir)")
    p.add_argument("--val_pairs", type=str, default=None, help='Scale pairs of the validation set (default: --pairs, else the ten)')
    p.add_argument("--val_images", type=int, default=None, help="Validate on the first K files of --val_dir in sorted order")
    p.add_argument("--val_both", action="store_true", help="With --ema_decay: score the raw weights as well as the averaged ones")
    p.add_argument("--keep_best", choices=("psnr", "ssim", "l1"), default=None, help="Keep best/model_epoch_<N>.pth by this validation metric")
    p.add_argument("--png_decoder", choices=("host", "gpu"), default="host",
                   help="host: Pillow decodes an image when it is first used (default); gpu: the training set and --val_dir are decoded "
                        "into the cache before the first step, in batches, by ops.png_decode (same pixels)")
    return p


def lr_at(k, base, warmup=0, schedule="constant", total=None, lr_min=0.0):
    """The learning rate of global optimizer step k (0-based; a resumed run continues at epochs_trained * steps_per_epoch).
    k < warmup: linear warm-up ``base * (k + 1) / warmup`` (step warmup - 1 runs at `base`).  Afterwards "constant" stays at `base`
    and "cosine" runs from `base` (step `warmup`) to `lr_min` (step total - 1) over the remaining steps of the run."""
    if k < warmup:
        return base * (k + 1) / warmup
    if schedule == "constant":
        return base
    if schedule != "cosine":
        raise ValueError(f"unknown lr schedule {schedule!r}")
    if total is None:
        raise ValueError("the cosine schedule needs the run's total number of optimizer steps")
    span = total - 1 - warmup
    if span <= 0 or k >= total - 1:
        return lr_min
    return lr_min + 0.5 * (base - lr_min) * (1.0 + math.cos(math.pi * (k - warmup) / span))


def guard_options(args):
    """True if any optimizer option beyond the reference's plain Adam at a constant rate is set: the output gains lr / grad_norm."""
    return (args.weight_decay != 0.0 or args.adamw or args.clip_grad_norm is not None or args.skip_nonfinite
            or args.warmup_steps > 0 or args.lr_schedule != "constant")


def pure_l1(args):
    return args.l1 == 1.0 and args.mse == 0.0 and args.ssim == 0.0


def patch_options(args):
    """The patch-mode options, checked before anything touches the GPU: None without ``--patch_size``, else (patch, scales)."""
    if args.patch_size is None:
        if args.no_augment or args.patches_per_epoch is not None or args.patch_scales != "2,3,4,6":
            sys.exit("train.py: --patch_scales, --no_augment and --patches_per_epoch need --patch_size")
        if degrade_requested(args):
            sys.exit("train.py: --degrade, --degrade_blur, --degrade_noise, --degrade_jpeg, --degrade_prob and --degrade_jpeg_420 need --patch_size")
        return None
    degrade_options(args)
    if args.pairs:
        sys.exit("train.py: --pairs does not apply with --patch_size (patches are square: use --patch_scales)")
    if args.patch_size < 1:
        sys.exit("train.py: --patch_size must be >= 1")
    if args.patches_per_epoch is not None and args.patches_per_epoch < 1:
        sys.exit("train.py: --patches_per_epoch must be >= 1")
    try:
        scales = tuple(int(v) for v in args.patch_scales.split(","))
    except ValueError:
        sys.exit(f"train.py: --patch_scales {args.patch_scales!r}: expected integers separated by commas, e.g. 2,3,4,6")
    if args.model == "ResidualTransformer":
        sys.exit("train.py: --model ResidualTransformer takes only 720x1280 input (its position embedding fixes the token count); "
                 "it cannot train with --patch_size")
    if args.model == "WindowTransformer" and (args.patch_size + 1) // 2 < 8:
        sys.exit("train.py: --model WindowTransformer needs --patch_size >= 15 (one 8x8 patch after its stride-2 conv)")
    valid = (2, 3, 4, 6) if args.model == "FastTransformer" else tuple(range(1, 9))          # weights.VALID_SCALES; the sampler's range
    bad = [v for v in scales if v not in valid]
    if bad or not scales or len(set(scales)) != len(scales):
        sys.exit(f"train.py: --patch_scales {args.patch_scales!r}: --model {args.model} trains on distinct scales out of {list(valid)}")
    return args.patch_size, scales


def degrade_requested(args):
    return bool(args.degrade or args.degrade_blur or args.degrade_noise or args.degrade_jpeg or args.degrade_prob or args.degrade_jpeg_420)


def degrade_options(args):
    """The `data.DegradeSpec` keywords of the --degrade* options (an option that is not given keeps the spec's default), None
    without any of them.  Parsed and checked here, before anything touches the GPU; `patch_options` calls it."""
    if not degrade_requested(args):
        return None

    def numbers(flag, text, count, kind):
        try:
            values = tuple(kind(v) for v in text.split(","))
        except ValueError:
            values = ()
        if len(values) != count:
            if count == 1:
                sys.exit(f"train.py: {flag} {text!r}: expected one number")
            sys.exit(f"train.py: {flag} {text!r}: expected {count} {'integers' if kind is int else 'numbers'} separated by commas")
        return values
    kw = {}
    if args.degrade_blur:
        kw["blur_sigma"] = numbers("--degrade_blur", args.degrade_blur, 2, float)
    if args.degrade_noise:
        kw["noise_sigma"] = numbers("--degrade_noise", args.degrade_noise, 2, float)
    if args.degrade_jpeg:
        kw["jpeg_quality"] = numbers("--degrade_jpeg", args.degrade_jpeg, 2, int)
    if args.degrade_prob:
        kw["blur_prob"], kw["noise_prob"], kw["jpeg_prob"] = numbers("--degrade_prob", args.degrade_prob, 3, float)
    if args.degrade_jpeg_420:
        kw["jpeg_420_prob"], = numbers("--degrade_jpeg_420", args.degrade_jpeg_420, 1, float)
    from transformerupscaler_amd.data import DegradeSpec
    try:
        DegradeSpec(**kw)
    except ValueError as e:
        flag = {"blur_sigma": "--degrade_blur", "noise_sigma": "--degrade_noise", "jpeg_quality": "--degrade_jpeg", "jpeg_420_prob": "--degrade_jpeg_420"}
        name = next((f for k, f in flag.items() if k in str(e)), "--degrade_prob")
        sys.exit(f"train.py: {name}: {e}")
    return kw


def val_options(args):
    """The EMA and validation options, checked before anything touches the GPU; True if the run validates."""
    if args.val_dir is None:
        if (args.val_interval != 1 or args.val_pairs is not None or args.val_images is not None or args.val_both
                or args.keep_best is not None):
            sys.exit("train.py: --val_interval, --val_pairs, --val_images, --val_both and --keep_best need --val_dir")
    if args.ema_decay is None and (args.val_both or args.ema_warmup):
        sys.exit("train.py: --val_both and --ema_warmup need --ema_decay")
    if args.ema_decay is not None and not 0.0 <= args.ema_decay < 1.0:
        sys.exit(f"train.py: --ema_decay {args.ema_decay} must be in [0, 1)")
    if args.val_interval < 1:
        sys.exit("train.py: --val_interval must be >= 1")
    if args.val_images is not None and args.val_images < 1:
        sys.exit("train.py: --val_images must be >= 1")
    if args.val_dir is not None and not os.path.isdir(args.val_dir):
        sys.exit(f"train.py: --val_dir {args.val_dir!r} is not a directory")
    return args.val_dir is not None


def epoch_batches(n_samples, batch_size, generator):
    """The shuffled batches of one epoch (index lists); a last partial batch is kept (DataLoader's drop_last=False)."""
    import torch
    order = torch.randperm(n_samples, generator=generator).tolist()
    return [order[i:i + batch_size] for i in range(0, n_samples, batch_size)]


def run(args):
    if not args.data_dir:
        sys.exit("train.py: --data_dir is required (a directory of .png images); the reference's online dataset is not built")
    if args.batch_size < 1:
        sys.exit("train.py: --batch_size must be >= 1")
    patch = patch_options(args)
    degrade_kw = degrade_options(args) if patch is not None else None
    validating = val_options(args)
    ema = args.ema_decay is not None
    import torch

    from transformerupscaler_amd import harness, ops
    from transformerupscaler_amd.data import SCALE_PAIRS, DegradeSpec, PairDataset, PatchSampler, parse_pairs, sample_plan

    val_pairs = None
    if validating:
        try:
            val_pairs = parse_pairs(args.val_pairs) if args.val_pairs else (parse_pairs(args.pairs) if args.pairs else SCALE_PAIRS)
        except ValueError as e:
            sys.exit(f"train.py: {e}")
    if args.checkpoint_dir is None:
        args.checkpoint_dir = os.path.join("models", args.model, "checkpoints")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = 0
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        if not dist.is_initialized():                                     # a caller may have set a group up (two ranks on one GPU: gloo)
            dist.init_process_group("nccl")
        rank = dist.get_rank()
    device = torch.device("cuda", torch.cuda.current_device())
    say = print if rank == 0 else (lambda *a, **k: None)
    say(f"Training on device: {device}" + (f" ({world} ranks)" if world > 1 else ""))
    if args.traceback:
        say("--traceback: the traceback window is not available in this build; continuing without it")

    torch.manual_seed(args.seed)
    model = importlib.import_module(f"models.{args.model}.model").TransformerModel()
    if not any(p.requires_grad for p in model.parameters()):
        sys.exit(f"train.py: model {args.model} has no trainable parameter; there is nothing to train")
    model = model.to(device)
    options = dict(lr=args.lr, weight_decay=args.weight_decay, decoupled=args.adamw, max_grad_norm=args.clip_grad_norm,
                   skip_nonfinite=args.skip_nonfinite)
    optimizer = harness.make_ema_optimizer(model, args.ema_decay, args.ema_warmup, **options) if ema \
        else harness.make_optimizer(model, **options)
    epochs_trained = harness.load_latest_checkpoint(model, args.checkpoint_dir, optimizer if args.save_optimizer else None,
                                                    map_location=device)
    if epochs_trained:
        say(f"Resuming from epoch {epochs_trained} of {args.checkpoint_dir}")
        if ema:
            side = harness.load_ema_checkpoint(model, args.checkpoint_dir, epochs_trained, optimizer, map_location=device)
            if side is None:
                say(f"No averaged weights of epoch {epochs_trained} in {os.path.join(args.checkpoint_dir, 'ema')}: "
                    "the average restarts from the loaded weights")
            elif side.get("dropout_calls") is not None and hasattr(model, "_dropout_calls"):
                model._dropout_calls = side["dropout_calls"]              # the dropout masks continue where the saved run stood
        if epochs_trained >= args.epochs:
            sys.exit(f"train.py: the latest checkpoint in {args.checkpoint_dir} is of epoch {epochs_trained}, "
                     f"which is not below --epochs {args.epochs}")
    else:
        say(f"No checkpoint in {args.checkpoint_dir}: starting from the initial weights")

    dp = None
    if world > 1:
        from transformerupscaler_amd.dp import DataParallel
        from transformerupscaler_amd.weights import VALID_SCALES
        if args.model == "FastTransformer":
            dp = DataParallel(model, scales=tuple(VALID_SCALES))          # (2, 3, 4, 6): a step may use any of them
        else:
            dp = DataParallel(model)                                      # every parameter is active in every step

    cache_bytes = int(args.cache_gb * (1 << 30))
    val_set = None
    if validating:                                                        # full images, also in patch mode; half of the cache budget
        cache_bytes //= 2
        try:
            val_set = PairDataset(args.val_dir, val_pairs, cache_bytes=cache_bytes, device=device)
        except FileNotFoundError as e:
            sys.exit(f"train.py: {e}")
        if args.val_images is not None:                                   # the first K files in sorted order
            val_set.files = val_set.files[:args.val_images]
            val_set.plan = sample_plan(len(val_set.files), len(val_set.scale_pairs))
    if patch is not None:
        pairs = None
        try:
            dataset = PatchSampler(args.data_dir, patch=patch[0], scales=patch[1], augment=not args.no_augment, seed=args.seed,
                                   samples_per_epoch=args.patches_per_epoch, cache_bytes=cache_bytes, device=device,
                                   degrade=None if degrade_kw is None else DegradeSpec(**degrade_kw))
        except ValueError as e:
            sys.exit(f"train.py: {e}")
    else:
        pairs = parse_pairs(args.pairs) if args.pairs else SCALE_PAIRS
        dataset = PairDataset(args.data_dir, pairs, cache_bytes=cache_bytes, device=device)
    if args.png_decoder == "gpu":                                         # same frames as the host decode, so same samples and losses
        for cached in (dataset, val_set):
            if cached is not None:
                plan = getattr(cached, "plan", None)
                cached.preload(None if plan is None else sorted({i for i, _ in plan}), decoder="gpu")
                say(f"Preloaded {cached.gpu_decodes} images of {cached.image_dir} on the GPU ({cached.decodes} on the host)")
    criterion = None
    if not pure_l1(args):
        from transformerupscaler_amd.losses import QualityLoss
        criterion = QualityLoss(l1=args.l1, mse=args.mse, ssim=args.ssim)
    what = (f"{len(pairs)} scale pairs" if patch is None else
            f"{patch[0]}x{patch[0]} patches at scales {list(patch[1])}" + ("" if dataset.augment else ", no augmentation")
            + ("" if dataset.degrade is None else f", LR degraded by {dataset.degrade}"))
    say(f"{len(dataset)} samples from {len(dataset.files)} images, {what}; loss {'L1' if criterion is None else criterion}")
    if validating:
        say(f"Validation: {len(val_set)} samples from {len(val_set.files)} images of {args.val_dir}, {len(val_pairs)} scale pairs, "
            f"{'averaged' if ema else 'raw'} weights" + (" and raw weights" if args.val_both else ""))

    shuffle = torch.Generator().manual_seed(args.seed)
    for _ in range(epochs_trained):                                       # a resumed run continues the shuffle sequence
        torch.randperm(len(dataset), generator=shuffle)
    record = {"model": args.model, "world": world, "samples": len(dataset), "resumed_from_epoch": epochs_trained,
              "steps": [], "epochs": [], "checkpoints": []}
    if patch is not None:
        record["patch"] = {"size": patch[0], "scales": list(patch[1]), "augment": dataset.augment,
                           "samples_per_epoch": dataset.samples_per_epoch}
        if dataset.degrade is not None:
            record["degrade"] = dataset.degrade.as_dict()
    if validating:
        record["val"] = []
    if args.keep_best:
        record["best"] = None

    def validate(epoch, weights):
        """One scored pass over the validation set on the averaged or the raw weights: a printed line and a record entry."""
        t0 = time.perf_counter()
        if weights == "ema":
            with harness.ema_weights(model, optimizer):
                res = harness.evaluate(model, val_set, group=not args.no_group)
        else:
            res = harness.evaluate(model, val_set, group=not args.no_group)
        seconds = time.perf_counter() - t0                                # evaluate ends with its read-back: the GPU is done
        entry = {"epoch": epoch, "weights": weights, "l1": res["l1"], "mse": res["mse"], "psnr": res["psnr"], "ssim": res["ssim"],
                 "per_pair": res["per_pair"], "seconds": seconds}
        record["val"].append(entry)
        say(f"Epoch [{epoch}/{args.epochs}] Validation ({weights}, {res['samples']} samples): L1 {res['l1']:.6f} MSE {res['mse']:.6e} "
            f"PSNR {res['psnr']:.3f} dB SSIM {res['ssim']:.5f} ({seconds:.2f} s)")
        return entry

    def keep_best(entry):
        """Rank 0 keeps one file: the validated weights of the best epoch so far by --keep_best."""
        value, best = entry[args.keep_best], record["best"]
        better = best is None or (value < best["value"] if args.keep_best == "l1" else value > best["value"])
        if not better:
            return
        path = os.path.join(args.checkpoint_dir, "best", f"model_epoch_{entry['epoch']}.pth")
        if rank == 0:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            sd = optimizer.ema_state_dict(model) if entry["weights"] == "ema" else model.state_dict()
            torch.save({k: v.detach().cpu() for k, v in sd.items()}, path)
            if best is not None and best["path"] != path and os.path.exists(best["path"]):
                os.remove(best["path"])                                   # the single file is replaced
            say(f"Kept best checkpoint ({args.keep_best} {value:.6f}): {path}")
        record["best"] = {"epoch": entry["epoch"], "metric": args.keep_best, "value": value, "weights": entry["weights"], "path": path}

    timed = []                                                            # patch mode: (start, sampler done, step done) events
    steps_done = 0
    stop = False
    extras = guard_options(args)
    guarded = args.clip_grad_norm is not None or args.skip_nonfinite
    scheduled = args.warmup_steps > 0 or args.lr_schedule != "constant"
    steps_per_epoch = -(-len(dataset) // args.batch_size)
    model.train()
    with ops.deterministic_mode(args.deterministic):
        for epoch in range(epochs_trained, args.epochs):
            batches = epoch_batches(len(dataset), args.batch_size, shuffle)
            losses = []                                                   # device scalars: read back when printed / at epoch end
            for step, batch in enumerate(batches):
                mine = batch[rank::world]
                if patch is not None:                                     # global sample index: a function of (seed, g) alone
                    if len(timed) < 256:
                        marks = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                        marks[0].record()
                    lr_list, hr_list = dataset.batch([epoch * len(dataset) + i for i in mine])
                    if len(timed) < 256:
                        marks[1].record()
                else:
                    samples = [dataset[i] for i in mine]
                    lr_list, hr_list = [s[0] for s in samples], [s[1] for s in samples]
                lr_now = args.lr
                if scheduled:                                             # the kernel reads lr from the group at every step
                    lr_now = lr_at(epoch * steps_per_epoch + step, args.lr, args.warmup_steps, args.lr_schedule,
                                   args.epochs * steps_per_epoch, args.lr_min)
                    for group in optimizer.param_groups:
                        group["lr"] = lr_now
                loss = harness.train_step_samples(model, optimizer, lr_list, hr_list,
                                                  loss=criterion, group=not args.no_group, b_global=len(batch))
                if patch is not None and len(timed) < 256:
                    marks[2].record()
                    timed.append(marks)
                if world > 1:                                             # ranks hold their share / world of the step's mean loss
                    loss = loss.clone()
                    torch.distributed.all_reduce(loss)
                    loss = loss / world
                losses.append(loss)
                steps_done += 1
                if step % args.log_interval == 0:
                    value = loss.item()
                    entry = {"epoch": epoch + 1, "step": step + 1, "loss": value}
                    tail = ""
                    if extras:                                            # read back only here, where the loss already is
                        entry["lr"] = lr_now
                        entry["grad_norm"] = optimizer.grad_norm.item() if guarded and optimizer.grad_norm is not None else None
                        tail = f" LR: {lr_now:.3e}" + ("" if entry["grad_norm"] is None else f" GradNorm: {entry['grad_norm']:.4f}")
                    say(f"Epoch [{epoch + 1}/{args.epochs}] Step [{step + 1}/{len(batches)}] Loss: {value:.6f}{tail}")
                    record["steps"].append(entry)
                if args.max_steps is not None and steps_done >= args.max_steps:
                    stop = True
                    break
            avg = torch.stack(losses).mean().item()
            say(f"Epoch [{epoch + 1}/{args.epochs}] completed. Average Loss: {avg:.6f}")
            record["epochs"].append({"epoch": epoch + 1, "steps": len(losses), "average_loss": avg})
            if validating and (epoch + 1) % args.val_interval == 0:
                entry = validate(epoch + 1, "ema" if ema else "raw")
                if args.val_both:
                    validate(epoch + 1, "raw")
                if args.keep_best:
                    keep_best(entry)
            if (epoch + 1) % args.checkpoint_interval == 0 or stop:
                if rank == 0:
                    path = harness.save_checkpoint(model, args.checkpoint_dir, epoch + 1, optimizer if args.save_optimizer else None,
                                                   ema=optimizer if ema else None,
                                                   ema_extra={"dropout_calls": getattr(model, "_dropout_calls", None)})
                    say(f"Saved checkpoint: {path}")
                    record["checkpoints"].append(path)
            if stop:
                break
    if extras:
        stats = optimizer.guard_stats() if guarded else {"applied": steps_done, "clipped": 0, "skipped": 0}
        record["guard"] = {k: stats[k] for k in ("applied", "clipped", "skipped")}
        if guarded:
            say(f"Optimizer steps applied: {stats['applied']}, clipped: {stats['clipped']}, skipped: {stats['skipped']}")
    if ema:
        record["ema"] = {"decay": args.ema_decay, "warmup": args.ema_warmup, "updates": optimizer.ema_updates}
        say(f"EMA updates applied: {record['ema']['updates']}")
    if len(timed) > 1:                                                    # GPU time between stream events, first step (warm-up) left out
        torch.cuda.synchronize()
        sampler_ms = sum(m[0].elapsed_time(m[1]) for m in timed[1:]) / (len(timed) - 1)
        step_ms = sum(m[0].elapsed_time(m[2]) for m in timed[1:]) / (len(timed) - 1)
        record["patch"]["timing"] = {"steps": len(timed) - 1, "step_ms": step_ms, "sampler_ms": sampler_ms}
        say(f"Patch sampler: {sampler_ms:.3f} ms of {step_ms:.3f} ms per step ({len(timed) - 1} steps after the first)")
    say("Training complete!" if not stop else f"Stopped after {steps_done} steps (--max_steps).")
    if dp is not None:
        dp.detach()
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    return record


def main(argv=None):
    args = build_parser().parse_args(argv)
    record = run(args)
    if args.json and int(os.environ.get("RANK", "0")) == 0:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)
    return record


if __name__ == "__main__":
    main()
