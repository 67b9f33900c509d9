"""Training-step harness with the semantics of the reference loop (train.py:110-146): zero_grad,
forward with ``res_out = HR size, require_ratio=False``, antialiased Resize to the HR size when shapes
differ, L1 loss, backward, Adam step.  Equal-shaped samples are batched (the reference loops over
samples at B=1; mean of per-sample L1 means == batch L1 mean for equal shapes).
``train_step(..., loss=losses.QualityLoss(...))`` trains on another criterion (L1 / MSE / SSIM mix) in the L1 loss's place."""
from __future__ import annotations

import contextlib
import math
import os

import torch
import torch.nn.functional as F

from .autograd import l1_loss, resize_aa
from .optim import _EmaBook

use_torch_adam = False          # A/B attribute


class _TorchGuardedStep(_EmaBook):
    """The A/B arm of optim.Adam / optim.AdamW's guard options on stock torch: clip_grad_norm_'s arithmetic on the parameters with a
    gradient, a synchronised finite check (`.item()`), then torch's own step.  Unlike the fused step it scales ``p.grad`` in place.
    With `ema_decay` the weight average follows an applied step as three torch operations per parameter (optim._EmaBook)."""

    def __init__(self, params, *args, max_grad_norm=None, skip_nonfinite=False, ema_decay=None, ema_warmup=False, **kwargs):
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"max_grad_norm must be >= 0 or None, got {max_grad_norm}")
        super().__init__(params, *args, **kwargs)
        self._init_ema(ema_decay, ema_warmup)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.grad_norm = None
        self._counts = {"steps": 0, "applied": 0, "clipped": 0, "skipped": 0}

    def guard_stats(self) -> dict:
        return dict(self._counts)

    @torch.no_grad()
    def step(self, closure=None):
        self._ema_check_step()
        if self.ema_decay is None:
            return self._guarded_step(closure)[1]
        # buffers are created before the update (a copy of the parameter as it was); a parameter that has one moves in every step
        pairs = [(p, self._ema_buffer(p)) for g in self.param_groups for p in g["params"] if p.grad is not None or p in self._ema]
        applied, loss = self._guarded_step(closure)
        if applied and pairs:
            w = self._ema_weight()
            for p, e in pairs:
                self._ema_torch_update(p, e, w)
            self._ema_n += 1
        return loss

    def _guarded_step(self, closure):
        """(applied, loss): torch's step behind the clipping and the synchronised finite check."""
        if self.max_grad_norm is None and not self.skip_nonfinite:
            return True, super().step(closure)
        grads = [p.grad for g in self.param_groups for p in g["params"] if p.grad is not None]
        if not grads:
            return True, super().step(closure)
        norm = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(grads)).double())
        self.grad_norm = norm.float()
        self._counts["steps"] += 1
        value = norm.item()                                   # the host synchronisation the fused step does without
        if self.skip_nonfinite and not math.isfinite(value):
            self._counts["skipped"] += 1
            return False, None
        if self.max_grad_norm is not None:
            torch._foreach_mul_(grads, torch.clamp(self.max_grad_norm / (norm + 1e-6), max=1.0).float())
            self._counts["clipped"] += int(self.max_grad_norm / (value + 1e-6) < 1.0)
        self._counts["applied"] += 1
        return True, super().step(closure)


class _TorchAdam(_TorchGuardedStep, torch.optim.Adam):
    pass


class _TorchAdamW(_TorchGuardedStep, torch.optim.AdamW):
    pass


def make_optimizer(model, lr: float = 1e-4, weight_decay: float = 0.0, decoupled: bool = False, max_grad_norm=None,
                   skip_nonfinite: bool = False):
    """train.py:104 -- Adam, default betas/eps, no weight decay (parameters without grad are skipped).  `optim.Adam` is
    torch.optim.Adam with the whole update in one HIP launch; harness.use_torch_adam = True selects torch's own step (A/B).
    `weight_decay` with `decoupled` selects AdamW's form (``p *= 1 - lr * wd``) instead of Adam's (``g += wd * p``);
    `max_grad_norm` / `skip_nonfinite` are optim.Adam's guard options (global-norm clipping, GradScaler's skipping of a step whose
    gradients are not finite), which the torch arm runs as clip_grad_norm_'s arithmetic plus a synchronised finite check."""
    kw = dict(lr=lr, weight_decay=weight_decay)
    guard = dict(max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
    if use_torch_adam:
        if max_grad_norm is None and not skip_nonfinite:
            return (torch.optim.AdamW if decoupled else torch.optim.Adam)(model.parameters(), **kw)
        return (_TorchAdamW if decoupled else _TorchAdam)(model.parameters(), **kw, **guard)
    from .optim import Adam, AdamW
    return (AdamW if decoupled else Adam)(model.parameters(), **kw, **guard)


def make_ema_optimizer(model, ema_decay: float, ema_warmup: bool = False, **options):
    """`make_optimizer(model, **options)` with optim.Adam's weight average: ``ema_decay`` in [0, 1), ``ema_warmup`` for timm's
    warm-up of the decay.  (A factory of its own: `make_optimizer`'s parameter list is fixed.)  The fused step keeps the average
    inside its own launch; under `use_torch_adam` the same options run as torch's step plus three torch operations per parameter,
    a guarded skip honoured through that arm's `.item()` check."""
    if ema_decay is None:
        raise ValueError("make_ema_optimizer needs an ema_decay in [0, 1); use make_optimizer for a step without the average")
    names = ("lr", "weight_decay", "decoupled", "max_grad_norm", "skip_nonfinite")
    unknown = [k for k in options if k not in names]
    if unknown:
        raise TypeError(f"make_ema_optimizer: unexpected options {unknown}")
    decoupled = bool(options.pop("decoupled", False))
    kw = dict(lr=options.pop("lr", 1e-4), weight_decay=options.pop("weight_decay", 0.0), max_grad_norm=options.pop("max_grad_norm", None),
              skip_nonfinite=options.pop("skip_nonfinite", False), ema_decay=ema_decay, ema_warmup=ema_warmup)
    if use_torch_adam:
        return (_TorchAdamW if decoupled else _TorchAdam)(model.parameters(), **kw)
    from .optim import Adam, AdamW
    return (AdamW if decoupled else Adam)(model.parameters(), **kw)


@contextlib.contextmanager
def ema_weights(model, optimizer):
    """Run `model` on the optimizer's averaged weights: inside the context every parameter that has an EMA buffer holds the buffer's
    storage (``p.data`` is exchanged, nothing is copied) and the buffer slot holds the raw weights; they are exchanged back on exit,
    also after an exception.  ``data_ptr`` changes, so the models' packed-weight caches re-pack on their own.  The context does not
    nest, and `optimizer.step()` inside it raises."""
    if getattr(optimizer, "ema_decay", None) is None:
        raise RuntimeError("ema_weights(): the optimizer was built without ema_decay")
    if optimizer._ema_swapped:
        raise RuntimeError("ema_weights() does not nest: the parameters already hold the averaged weights")
    optimizer._ema_settle()
    params = [p for p in model.parameters() if p in optimizer._ema]

    def exchange():
        for p in params:
            other = optimizer._ema[p]
            optimizer._ema[p] = p.data
            p.data = other
            torch.autograd.graph.increment_version(p)          # caches keyed on (data_ptr, _version) see a new key at every exchange

    exchange()
    optimizer._ema_swapped = True
    try:
        yield model
    finally:
        exchange()
        optimizer._ema_swapped = False


def train_step(model, optimizer, lr_batch: torch.Tensor, hr_batch: torch.Tensor, loss=None) -> torch.Tensor:
    """`loss`: None = the reference's nn.L1Loss; or a callable ``loss(out, target) -> scalar`` (losses.QualityLoss) used in its place."""
    optimizer.zero_grad(set_to_none=True)                                    # train.py:113
    out = model(lr_batch, res_out=tuple(hr_batch.shape[2:]), require_ratio=False)      # train.py:124
    if tuple(out.shape[2:]) != tuple(hr_batch.shape[2:]):
        out = resize_aa(out, tuple(hr_batch.shape[2:]))                      # train.py:127-130
    if loss is None:
        loss = l1_loss(out, hr_batch, fuse_into_model_backward=True)         # train.py:103,132,136 (HIP forward + backward; `out` feeds nothing else)
    else:
        loss = loss(out, hr_batch)
    loss.backward()                                                          # train.py:138 (bf16 needs no loss scaling; GradScaler's step skipping is make_optimizer(skip_nonfinite=True))
    optimizer.step()                                                         # train.py:139
    return loss.detach()


def plan_groups(shapes, group: bool = True, world: int = 1, b_global: int = None):
    """How `train_step_samples` runs a list of samples: ``[(sample indices, loss weight)]`` in execution order.  shapes: one hashable
    key per sample (its LR and HR shapes).  group=True: samples with equal keys form one batched group, groups in order of first
    occurrence; group=False: every sample is its own group, in list order.  The weight of a group of n samples is
    ``n * world / b_global`` (b_global = the sum of the ranks' list lengths, default ``len(shapes) * world``): the group's batch-mean
    loss times its share of the step's mean over all samples, times `world` because the reducer divides the sum over ranks by it."""
    shapes = list(shapes)
    world = int(world)
    if world < 1:
        raise ValueError("world must be >= 1")
    if b_global is None:
        b_global = len(shapes) * world
    if shapes and b_global < len(shapes):
        raise ValueError(f"b_global = {b_global} is smaller than this rank's {len(shapes)} samples")
    if not shapes:
        return []          # a rank without samples (world > 1) still takes part in the step's reduction
    if group:
        members = {}
        for i, key in enumerate(shapes):
            members.setdefault(key, []).append(i)          # dicts keep insertion order: first occurrence
        groups = list(members.values())
    else:
        groups = [[i] for i in range(len(shapes))]
    return [(idx, len(idx) * world / b_global) for idx in groups]


def _accumulator_for(model):
    """The model's cached GradAccumulator, rebuilt when its reducer (DataParallel attached / detached) changed."""
    from .accumulate import GradAccumulator
    reducer = getattr(model, "_grad_reducer", None)
    acc = model.__dict__.get("_grad_accumulator")
    if acc is None or acc.reducer is not reducer:
        acc = GradAccumulator(model, reducer)
        model.__dict__["_grad_accumulator"] = acc
    return acc


def train_step_samples(model, optimizer, lr_list, hr_list, loss=None, group=True, accumulator=None, b_global=None) -> torch.Tensor:
    """One optimizer step on a list of (lr, hr) samples of different sizes and scales: the reference's step (train.py:113-140), which
    runs every sample at B = 1, averages the losses and steps once.  Samples are ``[3][h][w]`` or ``[1][3][h][w]`` GPU tensors.
    Equal-shaped samples are batched (`group`, see `plan_groups`); each group's backward runs at once, so its activations are freed
    before the next group's forward (the reference holds every graph until its single backward; the gradient is the same by
    linearity), and its gradients go to `accumulator` (accumulate.GradAccumulator, by default the model's own, built on first use)
    in one launch.  Under DataParallel the step's gradients are all-reduced once, in `accumulator.finish()`; ranks may hold different
    numbers of samples (also none) when `b_global`, the sum of the ranks' list lengths, is passed.  Returns this rank's weighted loss
    sum as a device scalar (no host synchronisation): the step's mean loss in a single process, and its sum over ranks / world
    otherwise."""
    if len(lr_list) != len(hr_list):
        raise ValueError(f"{len(lr_list)} LR samples but {len(hr_list)} HR samples")
    acc = accumulator if accumulator is not None else _accumulator_for(model)
    world = acc.reducer.world if acc.reducer is not None else 1
    lrs = [t.unsqueeze(0) if t.dim() == 3 else t for t in lr_list]
    hrs = [t.unsqueeze(0) if t.dim() == 3 else t for t in hr_list]
    plan = plan_groups([(tuple(a.shape), tuple(b.shape)) for a, b in zip(lrs, hrs)], group, world, b_global)
    names = list(acc.params)
    params = [acc.params[n] for n in names]
    optimizer.zero_grad(set_to_none=True)                                    # train.py:113
    total = torch.zeros((), dtype=torch.float32, device=acc.device)
    suspended = getattr(model, "_grad_reducer", None)                        # the accumulator reduces once per step: the model's
    model._grad_reducer = None                                               # backward opens no reducer episode of its own
    acc.begin()
    try:
        for idx, weight in plan:
            lr_b = lrs[idx[0]] if len(idx) == 1 else torch.cat([lrs[i] for i in idx])
            hr_b = hrs[idx[0]] if len(idx) == 1 else torch.cat([hrs[i] for i in idx])
            hw = tuple(hr_b.shape[2:])
            out = model(lr_b, res_out=hw, require_ratio=False)               # train.py:124
            if tuple(out.shape[2:]) != hw:
                out = resize_aa(out, hw)                                     # train.py:127-130
            if loss is None:
                value = l1_loss(out, hr_b, fuse_into_model_backward=True)    # train.py:103,132
            else:
                value = loss(out, hr_b)
            value = value * weight                                           # train.py:136, this group's share
            del out
            grads = torch.autograd.grad(value, params, allow_unused=True)    # train.py:138, for this group alone
            acc.add(dict(zip(names, grads)))
            total = total + value.detach()
            del grads, value
        acc.finish()
    except BaseException:
        acc._touched = None
        raise
    finally:
        model._grad_reducer = suspended
    optimizer.step()                                                         # train.py:139
    return total


def evaluate(model, dataset, indices=None, batch_size: int = 4, group: bool = True) -> dict:
    """Score `model` on the samples ``dataset[i]`` (``(lr, hr)`` fp32 ``[3][h][w]`` GPU tensors, data.PairDataset) for i in `indices`
    (default: all), with the training step's own forward -- ``model(lr, res_out=hr_hw, require_ratio=False)``, then `resize_aa`
    when the shape differs -- under ``model.eval()`` and ``torch.no_grad()``.  Equal-shaped samples are batched up to `batch_size`
    (`group`; at most ``batch_size - 1`` samples per distinct shape wait for their batch).  Per sample: L1 (`autograd.l1_loss`, the
    training loss's value) and MSE, PSNR, SSIM (`metrics.quality`), kept on the device in an fp64 vector indexed by sample and read
    back once at the end.  Returns ``{"samples", "l1", "mse", "psnr", "ssim", "per_pair", "per_sample"}``: means in sample order,
    ``per_pair["LRHxLRW:HRHxHRW"] = {"samples", "l1", "mse", "psnr", "ssim"}`` and the per-sample lists.  The previous train / eval
    mode is restored; nothing a training step depends on advances (no dropout call, no generator).  Under torch.distributed sample k
    is scored by rank ``k % world`` and one ``all_reduce(sum)`` of the vector, zero elsewhere, gives every rank the same numbers."""
    from . import metrics
    idx = list(range(len(dataset))) if indices is None else [int(i) for i in indices]
    n = len(idx)
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError("evaluate: batch_size must be >= 1")
    import torch.distributed as dist
    world, rank = (dist.get_world_size(), dist.get_rank()) if dist.is_available() and dist.is_initialized() else (1, 0)
    device = next(model.parameters()).device
    names = ("l1", "mse", "psnr", "ssim")
    scores = torch.zeros((len(names), n), dtype=torch.float64, device=device)
    labels = [None] * n

    def score(items):
        ks = [k for k, _, _ in items]
        lr_b = items[0][1].unsqueeze(0) if len(items) == 1 else torch.stack([lr for _, lr, _ in items])
        hr_b = items[0][2].unsqueeze(0) if len(items) == 1 else torch.stack([hr for _, _, hr in items])
        hw = tuple(hr_b.shape[2:])
        out = model(lr_b, res_out=hw, require_ratio=False)
        if tuple(out.shape[2:]) != hw:
            out = resize_aa(out, hw)
        out = out.contiguous()
        q = metrics.quality(out, hr_b)
        where = torch.tensor(ks, dtype=torch.int64).to(device, non_blocking=True)
        scores[0, where] = torch.stack([l1_loss(out[j:j + 1], hr_b[j:j + 1]) for j in range(len(ks))]).double()
        for row, name in enumerate(names[1:], start=1):
            scores[row, where] = q[name]

    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            waiting = {}
            for k in range(n):
                if k % world != rank:
                    continue
                lr, hr = dataset[idx[k]]
                if lr.dim() == 4:
                    lr, hr = lr[0], hr[0]
                key = (tuple(lr.shape), tuple(hr.shape))
                if not group or batch_size == 1:
                    score([(k, lr, hr)])
                    continue
                bucket = waiting.setdefault(key, [])
                bucket.append((k, lr, hr))
                if len(bucket) == batch_size:
                    score(bucket)
                    waiting[key] = []
            for bucket in waiting.values():
                if bucket:
                    score(bucket)
    finally:
        model.train(was_training)
    if world > 1:                                             # every slot has one non-zero contribution: the sum is exact
        if dist.get_backend() == "gloo":
            host = scores.cpu()
            dist.all_reduce(host)
        else:
            dist.all_reduce(scores)
            host = scores.cpu()
    else:
        host = scores.cpu()
    values = {name: host[row].tolist() for row, name in enumerate(names)}
    pair_of = getattr(dataset, "plan", None)
    pairs = getattr(dataset, "scale_pairs", None)
    for k in range(n):
        if pair_of is not None and pairs is not None:
            pr = pairs[pair_of[idx[k]][1]]
            labels[k] = f"{pr['lr'][0]}x{pr['lr'][1]}:{pr['hr'][0]}x{pr['hr'][1]}"
        else:
            labels[k] = "all"

    def mean(vals):
        total = 0.0
        for v in vals:                                        # in sample order
            total += v
        return total / len(vals) if vals else float("nan")

    result = {"samples": n}
    for name in names:
        result[name] = mean(values[name])
    per_pair = {}
    for label in dict.fromkeys(labels):
        members = [k for k in range(n) if labels[k] == label]
        per_pair[label] = {"samples": len(members), **{name: mean([values[name][k] for k in members]) for name in names}}
    result["per_pair"] = per_pair
    result["per_sample"] = values
    return result


def save_ema_checkpoint(model, checkpoint_dir: str, epoch: int, optimizer, extra=None) -> str:
    """The averaged weights as ``<checkpoint_dir>/ema/model_epoch_{n}.pth`` -- the weight file's format and keys, so every driver
    that loads a checkpoint directory loads ``.../ema`` unchanged; in a sub-directory because `get_latest_checkpoint` takes any
    ``*_N.pth`` -- and a sidecar ``ema/ema_epoch_{n}.pt`` = ``{"updates", "decay", "warmup"}`` for resuming the average (`extra`: further entries a driver wants back on resume)."""
    ema_dir = os.path.join(checkpoint_dir, "ema")
    os.makedirs(ema_dir, exist_ok=True)
    path = os.path.join(ema_dir, f"model_epoch_{epoch}.pth")
    torch.save({k: v.cpu() for k, v in optimizer.ema_state_dict(model).items()}, path)
    torch.save({"updates": optimizer.ema_updates, "decay": optimizer.ema_decay, "warmup": optimizer.ema_warmup, **(extra or {})},
               os.path.join(ema_dir, f"ema_epoch_{epoch}.pt"))
    return path


def load_ema_checkpoint(model, checkpoint_dir: str, epoch: int, optimizer, map_location=None):
    """Load what `save_ema_checkpoint` wrote for `epoch` into the optimizer's average and return the sidecar's dict; None (nothing
    loaded: the average restarts from the current weights at its first step) when the weight file or its sidecar is absent."""
    ema_dir = os.path.join(checkpoint_dir, "ema")
    path, side = os.path.join(ema_dir, f"model_epoch_{epoch}.pth"), os.path.join(ema_dir, f"ema_epoch_{epoch}.pt")
    if not (os.path.exists(path) and os.path.exists(side)):
        return None
    side = torch.load(side)
    optimizer.load_ema_state_dict(model, torch.load(path, map_location=map_location), updates=side["updates"])
    return side


def save_checkpoint(model, checkpoint_dir: str, epoch: int, optimizer=None, ema=None, ema_extra=None) -> str:
    """train.py:152-156: weights only, ``model_epoch_{n}.pth`` -- the file the reference's drivers load
    (``model.load_state_dict(torch.load(path))``, train.py:90, inference.py:97, speed_test.py:45), in both directions.
    The reference drops the optimizer state; with `optimizer` it goes to a sidecar ``optim_epoch_{n}.pt`` so a resumed
    run continues Adam's moments without changing the weight file's format.  `ema`: an optimizer built with ``ema_decay``; its
    averaged weights go to ``ema/model_epoch_{n}.pth`` as well (`save_ema_checkpoint`)."""
    os.makedirs(checkpoint_dir, exist_ok=True)
    path = os.path.join(checkpoint_dir, f"model_epoch_{epoch}.pth")
    torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, path)
    if optimizer is not None:
        torch.save(optimizer.state_dict(), os.path.join(checkpoint_dir, f"optim_epoch_{epoch}.pt"))
    if ema is not None:
        save_ema_checkpoint(model, checkpoint_dir, epoch, ema, ema_extra)
    return path


def load_latest_checkpoint(model, checkpoint_dir: str, optimizer=None, map_location=None) -> int:
    """Resume as train.py:86-92 does (latest ``*_<epoch>.pth``, strict load); returns the epoch (0 if none)."""
    from tools.utils import get_latest_checkpoint
    try:
        path, epoch = get_latest_checkpoint(checkpoint_dir)
    except (FileNotFoundError, OSError):
        return 0
    model.load_state_dict(torch.load(path, map_location=map_location))
    side = os.path.join(checkpoint_dir, f"optim_epoch_{epoch}.pt")
    if optimizer is not None and os.path.exists(side):
        optimizer.load_state_dict(torch.load(side, map_location=map_location))
    return epoch
