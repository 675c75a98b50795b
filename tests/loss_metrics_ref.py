"""Float64 references of avr.losses.loss_fn and avr.metrics.image_metrics (torch and numpy only): the reference's
loss_fn (utils.py:364-377) with autograd, and what skimage.metrics' PSNR and SSIM compute with get_metrics'
arguments (utils.py:453-454), written out (skimage is not a dependency)."""
import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64


def loss_ref(img_coarse, img_fine, depth, gt, loss_params, near=0.5, far=2.0):
    """utils.py:364-377 in float64, term for term: the 0-dim loss, differentiable through torch autograd into any
    input that requires grad (inputs already float64 are used as they are). The `if loss.isnan()` host branch is
    the reference's own."""
    c = lambda t: None if t is None else t.to(F64)  # noqa: E731
    img_coarse, img_fine, depth, gt = c(img_coarse), c(img_fine), c(depth), c(gt)
    mse_loss = torch.nn.MSELoss()
    loss = 0
    if loss_params[0] != "fine":
        loss = loss + mse_loss(img_coarse, gt)
    if loss_params[0] != "coarse":
        loss = loss + mse_loss(img_fine, gt)
    if loss.isnan():
        loss = torch.tensor(1e-6, dtype=F64, device=gt.device)
    if loss_params[1]:
        penalty = torch.max(near - depth, torch.zeros_like(depth)) + torch.max(depth - far, torch.zeros_like(depth))
        loss = loss + torch.mean(penalty) * 10000
    return loss


def ssim_psnr_ref(img, gt, H, W):
    """(psnr (B,), ssim (B,)) float64 tensors for frames that flatten to (B, H * W, 3): PSNR = 10 log10(1 / mse)
    over all values; SSIM with a 7 x 7 uniform window per channel, sample covariance (49/48), C1 = 1e-4, C2 =
    9e-4, averaged over the window positions inside the frame and then over the channels. avg_pool2d(x, 7,
    stride=1) gives exactly those window means (the cropped interior of skimage's uniform_filter)."""
    x = img.detach().to(F64).reshape(-1, H, W, 3).permute(0, 3, 1, 2)
    y = gt.detach().to(F64).reshape(-1, H, W, 3).permute(0, 3, 1, 2)
    mse = ((x - y) ** 2).mean(dim=(1, 2, 3))
    psnr = 10.0 * torch.log10(1.0 / mse)
    pool = lambda t: F.avg_pool2d(t, 7, stride=1)  # noqa: E731
    ux, uy, uxx, uyy, uxy = pool(x), pool(y), pool(x * x), pool(y * y), pool(x * y)
    cov = 49.0 / 48.0
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return psnr, S.mean(dim=(2, 3)).mean(dim=1)


def ssim_psnr_scipy(img, gt, H, W):
    """The same through scipy.ndimage.uniform_filter and a 3-pixel crop, as skimage.metrics.structural_similarity
    is written (float64 numpy arrays, one frame at a time)."""
    from scipy.ndimage import uniform_filter
    x = np.asarray(img, dtype=np.float64).reshape(-1, H, W, 3)
    y = np.asarray(gt, dtype=np.float64).reshape(-1, H, W, 3)
    psnr, ssim = [], []
    for a, b in zip(x, y):
        with np.errstate(divide="ignore"):
            psnr.append(10.0 * np.log10(1.0 / np.mean((a - b) ** 2)))
        per_channel = []
        for ch in range(3):
            p, q = a[..., ch], b[..., ch]
            f = lambda t: uniform_filter(t, size=7)  # noqa: E731
            ux, uy, uxx, uyy, uxy = f(p), f(q), f(p * p), f(q * q), f(p * q)
            cov = 49.0 / 48.0
            vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
            C1, C2 = 0.01 ** 2, 0.03 ** 2
            S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
            per_channel.append(S[3:H - 3, 3:W - 3].mean())
        ssim.append(np.mean(per_channel))
    return np.array(psnr), np.array(ssim)


METRIC_SHAPES = [(1, 7, 7), (3, 8, 13), (2, 38, 33), (2, 45, 70), (2, 128, 128),
                 (2, 23, 39), (1, 17, 33)]   # the last two: the kernel's 16 x 32 tile of window positions, + 1


def metric_frames(B, H, W, kind, seed=0):
    """(img, gt) float32 CPU tensors (B, H * W, 3) in [0, 1]: 'noisy' = a smooth random gt and gt + 0.05 N(0, 1)
    clipped; 'white' = an all-white frame against that gt; 'constant' = two constant frames (0.25 and 0.75);
    'identical' = the gt against itself."""
    g = torch.Generator().manual_seed(1000 * seed + 97 * H + W + B)
    low = torch.rand(B, 3, max(H // 8, 2), max(W // 8, 2), generator=g)
    gt = F.interpolate(low, size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    gt = gt.reshape(B, H * W, 3).contiguous()
    if kind == "noisy":
        img = (gt + 0.05 * torch.randn(gt.shape, generator=g)).clamp(0.0, 1.0)
    elif kind == "white":
        img = torch.ones_like(gt)
    elif kind == "constant":
        img, gt = torch.full_like(gt, 0.25), torch.full_like(gt, 0.75)
    elif kind == "identical":
        img = gt.clone()
    else:
        raise ValueError(kind)
    return img, gt
