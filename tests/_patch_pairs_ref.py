"""TEST INFRASTRUCTURE ONLY -- the numpy statement of a patch training sample (`ops.patch_pairs`, csrc/patch_pairs.hip), built on
the Pillow-exact resize oracle.  Per sample: crop, flips, transpose (in that order), then ToTensor for HR and Pillow's two-pass 8-bit
BILINEAR resize + ToTensor for LR -- the resize runs on the TRANSFORMED crop (tests/test_patch_sampler_cpu.py pins this to Pillow
itself, and pins that the order matters)."""
import numpy as np

from oracle.image_io_oracle import pil_resize_bilinear_u8, to_tensor


def transform(frame: np.ndarray, y0: int, x0: int, op: int, P: int) -> np.ndarray:
    """uint8 [H][W][3] -> the transformed P x P crop, uint8 [P][P][3]."""
    t = frame[y0:y0 + P, x0:x0 + P]
    assert t.shape == (P, P, 3), "the crop leaves the frame"
    if op & 1:
        t = t[:, ::-1]
    if op & 2:
        t = t[::-1]
    if op & 4:
        t = t.transpose(1, 0, 2)
    return np.ascontiguousarray(t)


def patch_pair(frame: np.ndarray, y0: int, x0: int, op: int, p: int, scale: int):
    """(lr float32 [3][p][p], hr float32 [3][P][P]) of one sample."""
    t = transform(frame, y0, x0, op, p * scale)
    lr = pil_resize_bilinear_u8(t, (p, p))
    return to_tensor(lr[None])[0], to_tensor(t[None])[0]


def patch_pairs(frames, boxes, p: int, scale: int):
    """(lr float32 [B][3][p][p], hr float32 [B][3][P][P]) of a batch: frames a list of uint8 [H][W][3], boxes (y0, x0, op)."""
    pairs = [patch_pair(f, y0, x0, op, p, scale) for f, (y0, x0, op) in zip(frames, boxes)]
    return np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])


def resize_then_transpose(frame: np.ndarray, y0: int, x0: int, op: int, p: int, scale: int) -> np.ndarray:
    """The WRONG order for op & 4 (resize the flipped crop, transpose the result): float32 [3][p][p], 1 LSB off in places."""
    t = transform(frame, y0, x0, op & 3, p * scale)
    lr = pil_resize_bilinear_u8(t, (p, p))
    if op & 4:
        lr = np.ascontiguousarray(lr.transpose(1, 0, 2))
    return to_tensor(lr[None])[0]
