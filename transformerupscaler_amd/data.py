"""Training / evaluation samples from a directory of images: the reference's ``highres_img_dataset``
(data_handling/data_class.py:24-75) with the resizes on the GPU.

* the ``.png`` files of the directory, SORTED by name (the reference takes ``os.listdir`` order, which the file system decides);
* the ten scale pairs of data_class.py:34-45 in their order; sample ``i`` is image ``i // 10`` under pair ``i % 10``;
* ``min(200, 10 * n_png)`` samples (the reference reports 200 whatever the directory holds and raises IndexError with fewer than 20
  images; here a smaller directory gives fewer samples).

Each PNG is decoded once on the host (PIL) and kept as uint8 ``[H][W][3]`` on the GPU in an LRU cache bounded by `cache_bytes`; LR
and HR are built there by ``ops.resize_frames`` (Pillow-exact BILINEAR Resize + ToTensor), instead of one decode and two host
resizes per sample in DataLoader workers.  Only the local directory is read: the reference's online dataset is not built, and
nothing here opens a connection.  The table and the sample plan are the ones `ab_test.py` evaluates on (that driver keeps its own statement of them; a test checks that the two agree).

`PatchSampler` is the other way to train on the same directory: random square HR crops with the 8 flip / rotate variants and
their Pillow-exact LR counterparts, a whole batch per scale in one ``ops.patch_pairs`` launch (csrc/patch_pairs.hip).
"""
from __future__ import annotations

import os
import struct
from collections import OrderedDict

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
DEFAULT_CACHE_BYTES = 2 << 30


def list_pngs(data_dir):
    """The ``.png`` files of data_dir (case-insensitive suffix, data_class.py:26-31), sorted by name."""
    return sorted(os.path.join(data_dir, f) for f in os.listdir(data_dir) if f.lower().endswith(".png"))


def sample_plan(n_png, n_pairs=len(SCALE_PAIRS)):
    """[(image index, scale-pair index)] of the samples: index i -> (i // n_pairs, i % n_pairs), min(200, n_pairs * n_png) of them."""
    n = min(MAX_SAMPLES, n_pairs * n_png)
    return [(i // n_pairs, i % n_pairs) for i in range(n)]


def decode_png(path, device):
    """uint8 [H][W][3] on the GPU (one host decode per image)."""
    import numpy as np
    import torch
    from PIL import Image
    with Image.open(path) as im:
        arr = np.asarray(im.convert("RGB"))
    return torch.from_numpy(arr.copy()).to(device)


def parse_pairs(text):
    """``"HxW:HxW,HxW:HxW"`` -> a scale-pair table (LR size : HR size per entry), the form of SCALE_PAIRS."""
    pairs = []
    for item in text.split(","):
        try:
            lr, hr = item.strip().split(":")
            lr_hw = tuple(int(v) for v in lr.lower().split("x"))
            hr_hw = tuple(int(v) for v in hr.lower().split("x"))
            if len(lr_hw) != 2 or len(hr_hw) != 2 or min(lr_hw + hr_hw) < 1:
                raise ValueError
        except ValueError:
            raise ValueError(f"scale pair {item!r}: expected LRHxLRW:HRHxHRW, e.g. 96x96:192x192") from None
        pairs.append({"lr": lr_hw, "hr": hr_hw})
    if not pairs:
        raise ValueError("no scale pair given")
    return pairs


def png_size(path):
    """(H, W) of a PNG from its IHDR chunk: 24 bytes read, nothing decoded."""
    with open(path, "rb") as f:
        head = f.read(24)
    if len(head) < 24 or head[:8] != b"\x89PNG\r\n\x1a\n" or head[12:16] != b"IHDR":
        raise ValueError(f"{path!r} is not a PNG file")
    w, h = struct.unpack(">II", head[16:24])
    return h, w


class FrameCache:
    """The decoded images of `self.files` as uint8 [H][W][3] on `self.device`, one host decode each, in an LRU cache bounded by
    `cache_bytes` (an image larger than the bound is decoded per use and never kept)."""

    def _init_cache(self, cache_bytes, device):
        self.cache_bytes = int(cache_bytes)
        self.device = device
        self._cache: "OrderedDict[int, object]" = OrderedDict()
        self._cached_bytes = 0
        self.decodes = 0          # host decodes so far (a cache hit does none)

    def frame(self, img_idx):
        """The decoded image as uint8 [H][W][3] on the GPU, through the LRU cache."""
        f = self._cache.get(img_idx)
        if f is not None:
            self._cache.move_to_end(img_idx)
            return f
        f = decode_png(self.files[img_idx], self.device)
        self.decodes += 1
        size = f.numel()
        if size <= self.cache_bytes:
            while self._cache and self._cached_bytes + size > self.cache_bytes:
                _, old = self._cache.popitem(last=False)
                self._cached_bytes -= old.numel()
            self._cache[img_idx] = f
            self._cached_bytes += size
        return f


class PairDataset(FrameCache):
    """``PairDataset(image_dir)[i] -> (lr, hr)``: fp32 ``[3][h][w]`` GPU tensors in [0, 1] of image ``i // n_pairs`` under scale pair
    ``i % n_pairs`` (module docstring)."""

    def __init__(self, image_dir, scale_pairs=SCALE_PAIRS, cache_bytes=DEFAULT_CACHE_BYTES, device="cuda"):
        if not image_dir:
            raise ValueError("PairDataset needs a directory of .png images (data_dir); the reference's online dataset is not built")
        if not os.path.isdir(image_dir):
            raise FileNotFoundError(f"PairDataset: {image_dir!r} is not a directory")
        self.image_dir = image_dir
        self.scale_pairs = [{"lr": tuple(p["lr"]), "hr": tuple(p["hr"])} for p in scale_pairs]
        if not self.scale_pairs:
            raise ValueError("PairDataset: empty scale-pair table")
        self.files = list_pngs(image_dir)
        if not self.files:
            raise FileNotFoundError(f"PairDataset: no .png file in {image_dir!r}")
        self.plan = sample_plan(len(self.files), len(self.scale_pairs))
        self._init_cache(cache_bytes, device)

    def __len__(self):
        return len(self.plan)

    def __getitem__(self, i):
        from . import ops
        if not -len(self.plan) <= i < len(self.plan):
            raise IndexError(i)
        img_idx, pair_idx = self.plan[i]
        pair = self.scale_pairs[pair_idx]
        frame = self.frame(img_idx)
        lr = ops.resize_frames(frame, pair["lr"], to_tensor=True)[0]
        hr = ops.resize_frames(frame, pair["hr"], to_tensor=True)[0]
        return lr, hr


PATCH_SCALES = (2, 3, 4, 6)
MAX_PATCH_SCALE = 8          # the LDS window of csrc/patch_pairs.hip


class PatchSampler(FrameCache):
    """Random-crop training samples: ``draw(g)`` says what sample `g` is, ``batch(indices)`` builds a list of them on the GPU.

    Sample `g` (the global index ``epoch * samples_per_epoch + i``) is a pure host function of ``(seed, g)``: from
    ``numpy.random.default_rng([seed, g])`` come, in this order, the scale (uniform over `scales`), the image (uniform over the
    images with ``min(H, W) >= patch * scale``; sizes are read once from the PNG headers), the crop's corner ``y0``, ``x0`` (uniform
    over the positions that keep the ``patch * scale`` square inside the image) and `op` (uniform over the 8 flip / rotate variants;
    0 with ``augment=False``).  There is no generator state: a resumed run or another rank draws the same sample for the same `g`.

    The sample itself is ``ops.patch_pairs``'s: HR = ToTensor of the transformed crop, LR = ToTensor of its Pillow BILINEAR resize to
    ``patch x patch``.  `samples_per_epoch` defaults to `PairDataset`'s length for the same directory, ``min(200, 10 * n_png)``, so
    epochs, checkpoints and schedules count what they count on whole frames."""

    def __init__(self, image_dir, patch=96, scales=PATCH_SCALES, augment=True, seed=0, samples_per_epoch=None,
                 cache_bytes=DEFAULT_CACHE_BYTES, device="cuda"):
        if not image_dir:
            raise ValueError("PatchSampler needs a directory of .png images (data_dir); the reference's online dataset is not built")
        if not os.path.isdir(image_dir):
            raise FileNotFoundError(f"PatchSampler: {image_dir!r} is not a directory")
        self.image_dir = image_dir
        self.patch = int(patch)
        if self.patch < 1:
            raise ValueError(f"PatchSampler: patch = {patch} must be >= 1")
        try:
            self.scales = tuple(int(s) for s in scales)
            if any(a != b for a, b in zip(self.scales, scales)):
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError(f"PatchSampler: scales {scales!r} must be integers") from None
        if not self.scales or len(set(self.scales)) != len(self.scales) or not all(1 <= s <= MAX_PATCH_SCALE for s in self.scales):
            raise ValueError(f"PatchSampler: scales {scales!r} must be distinct integers in [1, {MAX_PATCH_SCALE}], at least one")
        self.files = list_pngs(image_dir)
        if not self.files:
            raise FileNotFoundError(f"PatchSampler: no .png file in {image_dir!r}")
        self.sizes = [png_size(f) for f in self.files]
        self.eligible = {}
        for s in self.scales:
            need = self.patch * s
            self.eligible[s] = [i for i, (h, w) in enumerate(self.sizes) if min(h, w) >= need]
            if not self.eligible[s]:
                raise ValueError(f"PatchSampler: no image in {image_dir!r} is large enough for scale {s}: it needs "
                                 f"{need} x {need} pixels (patch {self.patch} x scale {s})")
        self.augment = bool(augment)
        self.seed = int(seed)
        if samples_per_epoch is None:
            samples_per_epoch = len(sample_plan(len(self.files)))
        self.samples_per_epoch = int(samples_per_epoch)
        if self.samples_per_epoch < 1:
            raise ValueError(f"PatchSampler: samples_per_epoch = {samples_per_epoch} must be >= 1")
        self._init_cache(cache_bytes, device)

    def __len__(self):
        return self.samples_per_epoch

    def draw(self, g):
        """(image index, scale, y0, x0, op) of global sample g."""
        import numpy as np
        g = int(g)
        if g < 0:
            raise IndexError(g)
        rng = np.random.default_rng([self.seed, g])
        scale = self.scales[int(rng.integers(len(self.scales)))]
        images = self.eligible[scale]
        image = images[int(rng.integers(len(images)))]
        h, w = self.sizes[image]
        side = self.patch * scale
        y0 = int(rng.integers(h - side + 1))
        x0 = int(rng.integers(w - side + 1))
        op = int(rng.integers(8)) if self.augment else 0
        return image, scale, y0, x0, op

    def batch(self, indices):
        """(lr_list, hr_list) of the global samples `indices`, in that order: fp32 ``[3][patch][patch]`` and
        ``[3][patch * scale][patch * scale]`` views of one batched output per distinct scale (one launch each)."""
        from . import ops
        draws = [self.draw(g) for g in indices]
        by_scale = {}
        for pos, d in enumerate(draws):
            by_scale.setdefault(d[1], []).append(pos)
        lr_list, hr_list = [None] * len(draws), [None] * len(draws)
        for scale, members in by_scale.items():
            frames = [self.frame(draws[pos][0]) for pos in members]
            boxes = [draws[pos][2:5] for pos in members]
            lr, hr = ops.patch_pairs(frames, boxes, self.patch, scale)
            for j, pos in enumerate(members):
                lr_list[pos], hr_list[pos] = lr[j], hr[j]
        return lr_list, hr_list
