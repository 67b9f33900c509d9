#!/usr/bin/env python
"""Golden fixture of a MIXED-SCALE training step from the REAL reference module (runs only where the reference tree is present,
read-only; its source never enters this repository, only inputs / outputs):

  train_mixed_step.npz   FastTransformer, the loop of train.py:113-138 over six (lr, hr) samples of different sizes that resolve to
                         scales 2, 2, 3, 3, 6, 4 (eval-mode graph, dropout off, deterministic weights seed 0): the samples (8-bit
                         pixels, ``lr_u8_i`` / ``hr_u8_i``; the tensors are these / 255), the mean of the per-sample L1 losses, and every parameter's gradient in the grad_record format of make_golden_r2.py

The two first samples are equal-shaped (a grouped step batches them), the fourth needs train.py's external Resize
(24x40 -> scale 3 -> 72x120 -> 54x72), and every scale of the model appears, so every parameter receives a gradient.

    python tests/golden/make_golden_mixed.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import import_reference  # noqa: E402
from make_golden_r2 import grad_record  # noqa: E402

# (LR size, HR size, the scale the model resolves it to)
SAMPLES = [((32, 40), (64, 80), 2), ((32, 40), (64, 80), 2), ((32, 40), (96, 120), 3), ((24, 40), (54, 72), 3),
           ((24, 24), (144, 144), 6), ((24, 32), (96, 128), 4)]
SEED = 2718


def scene(rng):
    """A smooth random image as a function on the unit square (a few low-frequency waves per channel), so that LR and HR are
    the same picture at two resolutions, as the dataset's pairs are."""
    waves = [(rng.uniform(0.5, 4.0, 2), rng.uniform(0, 2 * np.pi), rng.uniform(0.03, 0.1)) for _ in range(3 * 4)]
    base = rng.uniform(0.35, 0.65, 3)

    def render(hw):
        v, u = np.meshgrid((np.arange(hw[0]) + 0.5) / hw[0], (np.arange(hw[1]) + 0.5) / hw[1], indexing="ij")
        planes = []
        for c in range(3):
            p = np.full(hw, base[c])
            for f, ph, a in waves[4 * c:4 * c + 4]:
                p = p + a * np.sin(2 * np.pi * (f[0] * v + f[1] * u) + ph)
            planes.append(p)
        img = np.stack(planes) + rng.normal(0, 0.01, (3,) + tuple(hw))
        return np.clip(np.round(img * 255), 0, 255).astype(np.uint8)          # what ToTensor sees: 8-bit pixels
    return render


def samples():
    """[(lr, hr)] fp32 [1][3][h][w] in [0, 1], k / 255 values."""
    rng = np.random.RandomState(SEED)
    out = []
    for lr, hr, _ in SAMPLES:
        render = scene(rng)
        out.append(tuple(torch.from_numpy(render(hw)).float().div(255.0).unsqueeze(0) for hw in (lr, hr)))
    return out


def main():
    from transformerupscaler_amd.weights import deterministic_state_dict
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref, Resize = import_reference()
    model = ref.TransformerModel().eval()
    model.load_state_dict(deterministic_state_dict(0), strict=False)
    model.zero_grad()
    losses = []
    data = samples()
    for (lr, hr), (_, _, scale) in zip(data, SAMPLES):
        hw = tuple(hr.shape[2:])
        o = model(lr, res_out=hw, require_ratio=False)                     # train.py:124
        assert o.shape[2] == lr.shape[2] * scale, (tuple(o.shape), scale)
        if tuple(o.shape[2:]) != hw:
            o = Resize(hw)(o)                                              # train.py:127-130
        losses.append(F.l1_loss(o, hr))
    loss = sum(losses) / len(losses)                                       # train.py:136
    loss.backward()
    out = grad_record(model, n_samples=256)
    assert len(out["none_grads"]) == 0, out["none_grads"]
    out["loss"] = np.float64(loss.item())
    out["sample_losses"] = np.array([v.item() for v in losses], np.float64)
    out["scales"] = np.array([s for _, _, s in SAMPLES])
    out["seed"] = np.array(SEED)
    for i, (lr, hr) in enumerate(data):
        out[f"lr_u8_{i}"] = lr[0].mul(255.0).round().to(torch.uint8).numpy()          # exact: the samples are k / 255
        out[f"hr_u8_{i}"] = hr[0].mul(255.0).round().to(torch.uint8).numpy()
    np.savez_compressed(os.path.join(HERE, "train_mixed_step.npz"), **out)
    print("train_mixed_step: loss", loss.item(), "per sample", out["sample_losses"].tolist())


if __name__ == "__main__":
    main()
