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
their Pillow-exact LR counterparts, a whole batch per scale in one ``ops.patch_pairs`` launch (csrc/patch_pairs.hip).  With a
`DegradeSpec` its LR patches also pass through blur, noise and a JPEG round trip (``ops.degrade``, csrc/degrade.hip).
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


PNG_DECODERS = ("host", "gpu")
PNG_GPU_BATCH = 64          # files per ops.png_decode call


def decode_pngs(paths, device, decoder="host"):
    """[uint8 [H][W][3] on the GPU] for a list of files: what `decode_png` returns for each.  decoder="host": that function, file by
    file.  decoder="gpu": the files are grouped by (H, W) and decoded by `ops.png_decode` in batches of at most PNG_GPU_BATCH, the
    status of a batch read back once; a file that `ops.png_parse` refuses (16-bit, interlaced, ...) or whose status is non-zero is
    decoded on the host instead, with one warning that names it."""
    return _decode_pngs(paths, device, decoder)[0]


def _decode_pngs(paths, device, decoder):
    """`decode_pngs` -> (frames, how many of them the host decoded)"""
    if decoder not in PNG_DECODERS:
        raise ValueError(f"decode_pngs: decoder must be one of {PNG_DECODERS}, got {decoder!r}")
    paths = list(paths)
    if decoder == "host":
        return [decode_png(p, device) for p in paths], len(paths)
    import warnings

    import torch

    from . import ops
    frames, groups, on_host = [None] * len(paths), OrderedDict(), 0
    for i, p in enumerate(paths):
        with open(p, "rb") as f:
            data = f.read()
        try:
            info = ops.png_parse(data)
            if info["H"] * (1 + 4 * info["W"]) >= 2 ** 31:
                raise ValueError(f"an image of {info['H']} x {info['W']}")
        except ValueError as e:
            warnings.warn(f"decode_pngs: {p!r} is decoded on the host ({e})")
            frames[i] = decode_png(p, device)
            on_host += 1
            continue
        groups.setdefault((info["H"], info["W"]), []).append((i, data))
    with torch.cuda.device(torch.device(device)):
        for members in groups.values():
            for at in range(0, len(members), PNG_GPU_BATCH):
                batch = members[at:at + PNG_GPU_BATCH]
                out, status = ops.png_decode([d for _, d in batch])
                for k, ((i, _), st) in enumerate(zip(batch, status.cpu().tolist())):
                    if st:
                        warnings.warn(f"decode_pngs: {paths[i]!r} is decoded on the host (status {st}: {ops.PNG_STATUS[st]})")
                        frames[i] = decode_png(paths[i], device)
                        on_host += 1
                    else:
                        frames[i] = out[k].clone() if len(batch) > 1 else out[k]      # a frame does not keep its batch alive
    return frames, on_host


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
        self.gpu_decodes = 0      # images `preload` decoded with ops.png_decode

    def preload(self, indices=None, decoder="gpu"):
        """Decode the given images (default: all) into the cache, in index order, until the next one would not fit in `cache_bytes`
        -> how many were loaded.  decoder="gpu": `decode_pngs`' batches (an image it had to hand to the host counts in `decodes`,
        the others in `gpu_decodes`); "host": `decode_png`, counted in `decodes`.  Images already cached are skipped."""
        todo, room = [], self.cache_bytes - self._cached_bytes
        for i in (range(len(self.files)) if indices is None else sorted(set(indices))):
            if i in self._cache:
                continue
            h, w = png_size(self.files[i])
            if 3 * h * w > room:
                break
            room -= 3 * h * w
            todo.append(i)
        for at in range(0, len(todo), PNG_GPU_BATCH):
            part = todo[at:at + PNG_GPU_BATCH]
            frames, on_host = _decode_pngs([self.files[i] for i in part], self.device, decoder)
            self.decodes += on_host
            self.gpu_decodes += len(part) - on_host
            for i, f in zip(part, frames):
                self._cache[i] = f
                self._cached_bytes += f.numel()
        return len(todo)

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


DEGRADE_STREAM = 0x44454752     # "DEGR": the third word of the seed of a sample's degradation stream


class DegradeSpec:
    """What `PatchSampler(degrade=...)` does to an LR patch after the clean downscale, BSRGAN / Real-ESRGAN style: with probability
    `blur_prob` a Gaussian blur of sigma uniform in `blur_sigma` (pixels, at most 3.0: the kernel's radius is 3), with `noise_prob`
    noise of standard deviation uniform in `noise_sigma` (8-bit units; with `grey_noise_prob` of those cases one value per pixel
    instead of one per channel), with `jpeg_prob` a JPEG round trip at a quality uniform over the integers of `jpeg_quality`: 4:2:0
    (chroma subsampled, what most JPEG files are) with `jpeg_420_prob` of those cases, else 4:4:4.
    The stages run in that order (``ops.degrade``).  Validated here; the defaults are the ones ``train.py --degrade`` uses."""

    FIELDS = ("blur_prob", "blur_sigma", "noise_prob", "noise_sigma", "grey_noise_prob", "jpeg_prob", "jpeg_quality")
    OPTIONAL = ("jpeg_420_prob",)          # shown by as_dict() and repr only when they are not zero: the default spec reads as it always did

    def __init__(self, blur_prob=0.5, blur_sigma=(0.2, 1.5), noise_prob=0.5, noise_sigma=(1.0, 10.0), grey_noise_prob=0.4,
                 jpeg_prob=0.7, jpeg_quality=(30, 95), jpeg_420_prob=0.0):
        from . import ops
        for name, v in (("blur_prob", blur_prob), ("noise_prob", noise_prob), ("grey_noise_prob", grey_noise_prob), ("jpeg_prob", jpeg_prob),
                        ("jpeg_420_prob", jpeg_420_prob)):
            try:
                ok = 0.0 <= float(v) <= 1.0
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"DegradeSpec: {name} = {v!r} must be a probability in [0, 1]")
            setattr(self, name, float(v))
        max_noise = ops.DEGRADE_MAX_NOISE_AMP * 147.80054 / 65536
        for name, v, top in (("blur_sigma", blur_sigma, ops.DEGRADE_MAX_BLUR_SIGMA), ("noise_sigma", noise_sigma, max_noise)):
            try:
                lo, hi = (float(t) for t in v)
                ok = 0.0 <= lo <= hi <= top
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"DegradeSpec: {name} = {v!r} must be (lo, hi) with 0 <= lo <= hi <= {top:g}")
            setattr(self, name, (lo, hi))
        try:
            lo, hi = (int(t) for t in jpeg_quality)
            ok = (lo, hi) == tuple(jpeg_quality) and 1 <= lo <= hi <= 100
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"DegradeSpec: jpeg_quality = {jpeg_quality!r} must be integers (lo, hi) with 1 <= lo <= hi <= 100")
        self.jpeg_quality = (lo, hi)

    def _shown(self):
        return self.FIELDS + tuple(k for k in self.OPTIONAL if getattr(self, k) != 0.0)

    def as_dict(self):
        return {k: (list(v) if isinstance(v, tuple) else v) for k, v in ((k, getattr(self, k)) for k in self._shown())}

    def __repr__(self):
        return "DegradeSpec(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self._shown()) + ")"

    def draw(self, rng):
        """One ``ops.degrade`` record from a numpy Generator.  Nine values are drawn whatever they decide (blur: coin, sigma; noise:
        coin, sigma, grey coin, seed; JPEG: coin, quality; last, the 4:2:0 coin), so one stage's setting never moves another's."""
        from . import ops
        blur_on, blur_sigma = rng.random() < self.blur_prob, float(rng.uniform(*self.blur_sigma))
        noise_on, noise_sigma = rng.random() < self.noise_prob, float(rng.uniform(*self.noise_sigma))
        grey, seed = rng.random() < self.grey_noise_prob, int(rng.integers(1 << 32))
        jpeg_on, quality = rng.random() < self.jpeg_prob, int(rng.integers(self.jpeg_quality[0], self.jpeg_quality[1] + 1))
        sub = rng.random() < self.jpeg_420_prob
        amp = ops.noise_amp(noise_sigma) if noise_on else 0
        return (ops.blur_taps(blur_sigma) if blur_on else ops.DEGRADE_TAPS_OFF, amp, seed if amp else 0,
                quality if jpeg_on else 0, (ops.DEGRADE_GREY_NOISE if amp and grey else 0) | (ops.DEGRADE_JPEG_420 if jpeg_on and sub else 0))


class PatchSampler(FrameCache):
    """Random-crop training samples: ``draw(g)`` says what sample `g` is, ``batch(indices)`` builds a list of them on the GPU.

    Sample `g` (the global index ``epoch * samples_per_epoch + i``) is a pure host function of ``(seed, g)``: from
    ``numpy.random.default_rng([seed, g])`` come, in this order, the scale (uniform over `scales`), the image (uniform over the
    images with ``min(H, W) >= patch * scale``; sizes are read once from the PNG headers), the crop's corner ``y0``, ``x0`` (uniform
    over the positions that keep the ``patch * scale`` square inside the image) and `op` (uniform over the 8 flip / rotate variants;
    0 with ``augment=False``).  There is no generator state: a resumed run or another rank draws the same sample for the same `g`.

    The sample itself is ``ops.patch_pairs``'s: HR = ToTensor of the transformed crop, LR = ToTensor of its Pillow BILINEAR resize to
    ``patch x patch``.  `samples_per_epoch` defaults to `PairDataset`'s length for the same directory, ``min(200, 10 * n_png)``, so
    epochs, checkpoints and schedules count what they count on whole frames.

    With ``degrade=DegradeSpec(...)`` the LR patch then passes through ``ops.degrade`` under the record ``draw_degrade(g)``, drawn
    from a stream of its own, ``default_rng([seed, g, DEGRADE_STREAM])``: ``draw(g)`` is what it is without it, and HR is untouched."""

    def __init__(self, image_dir, patch=96, scales=PATCH_SCALES, augment=True, seed=0, samples_per_epoch=None,
                 cache_bytes=DEFAULT_CACHE_BYTES, device="cuda", degrade=None):
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
        if degrade is not None and not isinstance(degrade, DegradeSpec):
            raise ValueError(f"PatchSampler: degrade = {degrade!r} must be a DegradeSpec or None")
        self.degrade = degrade
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

    def draw_degrade(self, g):
        """The ``ops.degrade`` record (taps, noise_amp, noise_seed, quality, flags) of global sample g; None without a spec."""
        import numpy as np
        g = int(g)
        if g < 0:
            raise IndexError(g)
        if self.degrade is None:
            return None
        return self.degrade.draw(np.random.default_rng([self.seed, g, DEGRADE_STREAM]))

    def batch(self, indices):
        """(lr_list, hr_list) of the global samples `indices`, in that order: fp32 ``[3][patch][patch]`` and
        ``[3][patch * scale][patch * scale]`` views of one batched output per distinct scale (one launch each, and one
        ``ops.degrade`` launch each with a `degrade` spec)."""
        from . import ops
        indices = list(indices)
        draws = [self.draw(g) for g in indices]
        by_scale = {}
        for pos, d in enumerate(draws):
            by_scale.setdefault(d[1], []).append(pos)
        lr_list, hr_list = [None] * len(draws), [None] * len(draws)
        for scale, members in by_scale.items():
            frames = [self.frame(draws[pos][0]) for pos in members]
            boxes = [draws[pos][2:5] for pos in members]
            lr, hr = ops.patch_pairs(frames, boxes, self.patch, scale)
            if self.degrade is not None:
                lr = ops.degrade(lr, [self.draw_degrade(indices[pos]) for pos in members])
            for j, pos in enumerate(members):
                lr_list[pos], hr_list[pos] = lr[j], hr[j]
        return lr_list, hr_list
