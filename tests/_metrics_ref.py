"""float64 restatement of skimage.metrics.structural_similarity / peak_signal_noise_ratio / mean_squared_error with the defaults
the reference uses (inference.py:128-145: ``data_range=1, channel_axis=-1``): 7x7 uniform window, use_sample_covariance=True,
K1 = 0.01, K2 = 0.03, mean over the interior [3:H-3, 3:W-3].  numpy only (scipy / skimage may be absent): the 7x7 box filter
is taken by cumulative sums, and only the window positions of the interior are formed, so border handling never enters."""
import numpy as np

WIN = 7


def box7(img):
    """Mean over every full 7x7 window of a 2-D array: [H-6][W-6] (the interior of skimage's uniform_filter)."""
    a = np.asarray(img, dtype=np.float64)
    c = np.zeros((a.shape[0] + 1, a.shape[1] + 1), dtype=np.float64)
    c[1:, 1:] = a.cumsum(0).cumsum(1)
    s = c[WIN:, WIN:] - c[:-WIN, WIN:] - c[WIN:, :-WIN] + c[:-WIN, :-WIN]
    return s / (WIN * WIN)


def ssim_channel(x, y, data_range):
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if x.shape[0] < WIN or x.shape[1] < WIN:
        raise ValueError("win_size exceeds image extent")
    n = WIN * WIN
    cov_norm = n / (n - 1.0)
    ux, uy = box7(x), box7(y)
    vx = cov_norm * (box7(x * x) - ux * ux)
    vy = cov_norm * (box7(y * y) - uy * uy)
    vxy = cov_norm * (box7(x * y) - ux * uy)
    c1 = (0.01 * data_range) ** 2
    c2 = (0.03 * data_range) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return float(s.mean(dtype=np.float64))


def ssim(x, y, data_range):
    """One image, channels LAST [H][W][C] (channel_axis=-1): mean of the per-channel SSIMs."""
    return float(np.mean([ssim_channel(x[..., c], y[..., c], data_range) for c in range(x.shape[-1])]))


def mse(x, y):
    d = np.asarray(x, dtype=np.float64) - np.asarray(y, dtype=np.float64)
    return float(np.mean(d * d))


def psnr(x, y, data_range):
    err = mse(x, y)
    return float("inf") if err == 0 else float(10 * np.log10(data_range ** 2 / err))
