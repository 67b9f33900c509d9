"""torch restatement of losses.quality_loss: l1 * mean|x - y| + mse * mean (x - y)^2 + ssim * (1 - mean_b SSIM(x[b], y[b])) with
skimage's default SSIM (7x7 uniform window as avg_pool2d(7, 1) on the moments, sample covariance 49/48, K1 = 0.01, K2 = 0.03,
interior mean, mean over the 3 channels).  In float64 it is what the GPU tests compare against (value, and gradient by autograd);
in float32 it is the composition of torch ops a user would write without the HIP loss.  `closed_form_ssim_grad` is the analytic
gradient the kernel implements, `kernel_form_ssim_grad` the same with the kernel's factoring around a shift."""
import torch
import torch.nn.functional as F

N, K = 49.0, 49.0 / 48.0


def _moments(x, y):
    ux, uy = F.avg_pool2d(x, 7, 1), F.avg_pool2d(y, 7, 1)
    vx = K * (F.avg_pool2d(x * x, 7, 1) - ux * ux)
    vy = K * (F.avg_pool2d(y * y, 7, 1) - uy * uy)
    vxy = K * (F.avg_pool2d(x * y, 7, 1) - ux * uy)
    return ux, uy, vx, vy, vxy


def ssim_map(x, y, data_range=1.0):
    """[B][3][H-6][W-6] map of S over the interior windows of planar [B][3][H][W] tensors."""
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    ux, uy, vx, vy, vxy = _moments(x, y)
    return ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))


def ssim(x, y, data_range=1.0):
    """[B]: per image, the mean of the three channels' interior means (metrics.ssim)."""
    return ssim_map(x, y, data_range).mean(dim=(2, 3)).mean(dim=1)


def terms(x, y, data_range=1.0):
    """(L1, MSE, 1 - mean_b SSIM) as scalars."""
    d = x - y
    return d.abs().mean(), (d * d).mean(), 1 - ssim(x, y, data_range).mean()


def quality_loss(x, y, l1=1.0, mse=0.0, ssim=0.0, data_range=1.0):
    t = terms(x, y, data_range)
    return sum(w * v for w, v in zip((l1, mse, ssim), t) if w != 0)


def autograd_grad(x, y, l1=1.0, mse=0.0, ssim=0.0, data_range=1.0):
    """(loss, d loss / d x) in the dtype of x."""
    x = x.detach().clone().requires_grad_(True)
    loss = quality_loss(x, y, l1, mse, ssim, data_range)
    loss.backward()
    return loss.detach(), x.grad


def _box_adjoint(m):
    """Sum over the windows that cover each pixel: [B][3][H-6][W-6] -> [B][3][H][W], zero outside the interior windows."""
    return F.avg_pool2d(F.pad(m, (6, 6, 6, 6)), 7, 1) * N


def closed_form_ssim_grad(x, y, data_range=1.0):
    """d (1 - mean_b SSIM) / d x by the closed form: window w gives a_w + b_w x_p + c_w y_p to every pixel p it covers."""
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    ux, uy, vx, vy, vxy = _moments(x, y)
    A1, A2, B1, B2 = 2 * ux * uy + c1, 2 * vxy + c2, ux * ux + uy * uy + c1, vx + vy + c2
    D = B1 * B2
    S = A1 * A2 / D
    b = -(2 / N) * K * S / B2
    c = (2 / N) * K * A1 / D
    a = (2 / N) * (uy * A2 / D - ux * S / B1 - K * uy * A1 / D + K * ux * S / B2)
    B, _, H, W = x.shape
    return -(_box_adjoint(a) + _box_adjoint(b) * x + _box_adjoint(c) * y) / (B * 3 * (H - 6) * (W - 6))


def kernel_form_ssim_grad(x, y, data_range=1.0, kx=None, ky=None):
    """The same gradient as csrc/quality_loss.hip forms it: moments of x - kx, y - ky, T_w factored, the affine form around the shift."""
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    kx = x[..., :1, :1] if kx is None else kx
    ky = y[..., :1, :1] if ky is None else ky
    xs, ys = x - kx, y - ky
    mx, my, vx, vy, vxy = _moments(xs, ys)
    ux, uy = mx + kx, my + ky
    A1, A2, B1, B2 = 2 * ux * uy + c1, 2 * vxy + c2, ux * ux + uy * uy + c1, vx + vy + c2
    D = B1 * B2
    tw = A2 * ((my - mx) + (ky - kx)) * (uy * (ux + uy) + c1) / (D * B1)
    c = (2 / 48.0) * A1 / D
    b = -(2 / 48.0) * (A1 * A2 / D) / B2
    a = (2 / N) * tw - (c * my + b * mx)
    B, _, H, W = x.shape
    return -(_box_adjoint(a) + _box_adjoint(b) * xs + _box_adjoint(c) * ys) / (B * 3 * (H - 6) * (W - 6))
