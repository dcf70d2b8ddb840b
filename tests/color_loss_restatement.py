"""Float64 numpy restatement of the photometric loss of a colour image: the masked L1 and the SSIM term of the
reference's compute_loss_color(use_ssim=True) (core/utils/loss_utils.py:188-209, core/utils/pytorch_ssim/ssim.py:4-35), with the gradient
with respect to the rendered image written out by hand, and the same formula as a torch composition for autograd to differentiate.

overlap = mask & gt_mask; l1 = mean |rgb - gt| over the overlap's 3 N entries. For SSIM both images are zeroed off the overlap; five
3 x 3 zero-padded box means, always divided by 9 (AvgPool2d(3, 1, padding=1)); C1 = 0.01^2, C2 = 0.03^2; ssim = n / (d + 1e-12); the loss
is the mean over 3 H W of clamp((1 - ssim) / 2, 0, 1). x is the ground truth (the first argument of loss_ssim), y the rendered image.
"""
import numpy as np

C1, C2, EPS = 0.01 ** 2, 0.03 ** 2, 1e-12


def box3(a):
    """3 x 3 zero-padded box mean of (..., H, W), always divided by 9. The operator is symmetric: it is its own adjoint."""
    a = np.asarray(a, np.float64)
    p = np.zeros(a.shape[:-2] + (a.shape[-2] + 2, a.shape[-1] + 2))
    p[..., 1:-1, 1:-1] = a
    H, W = a.shape[-2:]
    return sum(p[..., i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0


def ssim_map(x, y):
    """(ssim, the terms the gradient needs) of two (3, H, W) images"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    mx, my = box3(x), box3(y)
    sx, sy, sxy = box3(x * x) - mx * mx, box3(y * y) - my * my, box3(x * y) - mx * my
    A1, A2, B1, B2 = 2 * mx * my + C1, 2 * sxy + C2, mx * mx + my * my + C1, sx + sy + C2
    n, D = A1 * A2, B1 * B2 + EPS
    return n / D, (mx, my, A1, A2, B1, B2, n, D)


def _partials(x, y):
    """(ssim map, clamped-loss map t, the three box-averaged partials of the loss with respect to mu_y, E[y^2], E[xy])"""
    s, (mx, my, A1, A2, B1, B2, n, D) = ssim_map(x, y)
    t = (1.0 - s) / 2.0
    gs = np.where((t >= 0.0) & (t <= 1.0), -0.5, 0.0) / t.size            # torch.clamp passes the gradient on [min, max]
    dA1, dA2, dB1, dB2 = A2 / D, A1 / D, -n * B2 / D ** 2, -n * B1 / D ** 2
    g_mu = gs * (dA1 * 2 * mx - dA2 * 2 * mx + dB1 * 2 * my - dB2 * 2 * my)     # d ssim / d mu_y
    return s, t, box3(g_mu), box3(gs * dB2), box3(gs * dA2 * 2)                 # ..., d ssim / d E[y^2], d ssim / d E[xy]


def ssim_loss(x, y):
    """loss_ssim(x[None], y[None])[0] and its gradient with respect to y: (loss, g_y (3, H, W), ssim map)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    s, t, b_mu, b_eyy, b_exy = _partials(x, y)
    return np.clip(t, 0.0, 1.0).mean(), b_mu + 2 * y * b_eyy + x * b_exy, s


def ssim_grad_terms(x, y):
    """The size of what the gradient of ssim_loss is summed from, per entry: |box g_mu| + |2 y box g_eyy| + |x box g_exy|. Where the
    three cancel, an f32 evaluation is only as good as its relative error times THIS, not times the gradient."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    _, _, b_mu, b_eyy, b_exy = _partials(x, y)
    return np.abs(b_mu) + np.abs(2 * y * b_eyy) + np.abs(x * b_exy)


def color_loss(rgb, mask, gt, gt_mask, want_ssim=True):
    """One view: rgb, gt (H, W, 3), masks (H, W) -> dict(l1, ssim, overlap (count), g_l1, g_ssim: the gradients of the two values with
    respect to rgb (H, W, 3)). An empty overlap gives l1 = 0 and a zero L1 gradient (the reference yields NaN or raises there)."""
    rgb, gt = np.asarray(rgb, np.float64), np.asarray(gt, np.float64)
    ov = (np.asarray(mask) != 0) & (np.asarray(gt_mask) != 0)
    N = int(ov.sum())
    diff = (rgb - gt) * ov[..., None]
    out = dict(overlap=N, l1=(np.abs(diff).sum() / (3 * N)) if N else 0.0, g_l1=(np.sign(diff) / (3 * N)) if N else np.zeros_like(rgb), ssim=None, g_ssim=None)
    if want_ssim:
        x, y = (gt * ov[..., None]).transpose(2, 0, 1), (rgb * ov[..., None]).transpose(2, 0, 1)
        loss, g_y, _ = ssim_loss(x, y)
        out.update(ssim=loss, g_ssim=g_y.transpose(1, 2, 0) * ov[..., None])
    return out


def torch_color_loss(rgb, mask, gt, gt_mask):
    """The same formula as a torch composition (any dtype; autograd differentiates it): rgb, gt (H, W, 3) tensors, masks bool (H, W) ->
    (l1, ssim). An empty overlap gives NaN for l1, as torch's mean of nothing does."""
    import torch
    import torch.nn.functional as F
    ov = mask & gt_mask
    l1 = (rgb[ov] - gt[ov]).abs().mean()
    z = torch.zeros((), dtype=rgb.dtype)
    x = torch.where(ov[..., None], gt, z).permute(2, 0, 1)[None]
    y = torch.where(ov[..., None], rgb, z).permute(2, 0, 1)[None]
    pool = lambda a: F.avg_pool2d(a, 3, 1, padding=1)
    mx, my = pool(x), pool(y)
    sx, sy, sxy = pool(x * x) - mx * mx, pool(y * y) - my * my, pool(x * y) - mx * my
    s = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sx + sy + C2) + EPS)
    return l1, torch.clamp((1.0 - s) / 2.0, 0, 1).mean()
