"""PSNR / SSIM of rendered frames on the device: `from avr.metrics import get_metrics` replaces
`from utils import get_metrics` (utils.py:431-461), which copies both frames to the host and calls
skimage.metrics. Here one HIP launch covers every frame (avr_image_metrics: 7 x 7 uniform-window SSIM with fp64
moments, PSNR from the same staged pixels) and only the two reported scalars cross to the host. No CPU path: host
tensors raise AVRError.
"""
import math

import torch

from ._lib import call, ptr, require_device, size_query, stream_of

F32 = torch.float32


def _f32c(t):
    return t if (t.dtype == F32 and t.is_contiguous()) else t.to(F32).contiguous()


def image_metrics(img, gt, H, W):
    """(psnr, ssim), two (B,) fp32 device tensors, of B frame pairs of H x W x 3 values in [0, 1]: img and gt of
    any leading shape that flattens to (B, H * W, 3). What skimage.metrics.peak_signal_noise_ratio(data_range=1)
    and structural_similarity(channel_axis=-1, data_range=1) return for each pair (identical frames: +inf and
    exactly 1). H, W >= 7 (the SSIM window)."""
    H, W = int(H), int(W)
    if img.numel() != gt.numel() or H < 1 or W < 1 or img.numel() % (H * W * 3) != 0:
        raise ValueError(f"image_metrics: img {tuple(img.shape)} and gt {tuple(gt.shape)} are not frames of "
                         f"{H} x {W} x 3")
    B = img.numel() // (H * W * 3)
    img, gt = _f32c(img.detach()), _f32c(gt.detach())
    require_device(img, gt)
    ws = torch.empty(size_query("avr_image_metrics_workspace_bytes", B, H, W), device=img.device, dtype=torch.uint8)
    out = torch.empty(2, B, device=img.device, dtype=F32)
    call("avr_image_metrics", ptr(img), ptr(gt), B, H, W, ptr(ws), ws.numel(), ptr(out[0]), ptr(out[1]),
         stream_of(img))
    return out[0], out[1]


def get_metrics(mlp_out, gts, fine=True):
    """get_metrics of utils.py:431-461: (psnr, ssim) as two Python floats for mlp_out = (rgbs_coarse, rgbs_fine,
    _, _) with rgbs (SB, sl^2, 3) or (SB, NV, sl^2, 3) square frames and gts of the same size.

    The reference's quirk, kept (DESIGN Q11): it averages per scene into lists it never returns, and returns
    np.mean of its loop variables -- the LAST frame's PSNR and SSIM, not the mean over the frames. Every frame is
    still measured (image_metrics returns them all); the only host transfer is the final pair."""
    rgbs = mlp_out[1] if fine else mlp_out[0]
    if rgbs.dim() not in (3, 4) or rgbs.shape[-1] != 3:
        raise ValueError(f"get_metrics: rgbs of shape {tuple(rgbs.shape)}: (SB, sl^2, 3) or (SB, NV, sl^2, 3)")
    sl2 = rgbs.shape[-2]
    sl = math.isqrt(sl2)
    if sl * sl != sl2:
        raise ValueError(f"get_metrics: {sl2} pixels per frame is not a square frame")
    psnr, ssim = image_metrics(rgbs.reshape(-1, sl2, 3), gts.reshape(-1, sl2, 3), sl, sl)
    last = torch.stack((psnr[-1], ssim[-1])).tolist()
    return last[0], last[1]


def evaluate(model, model_input, gt, loss_params):
    """The validation body of train.py:152-155 and test.py:47-57 (without LPIPS, whose VGG weights are a
    download): under no_grad, model(model_input), get_metrics on the fine image unless the loss mode is 'coarse',
    and loss_fn. -> dict(psnr, ssim: Python floats; loss: 0-dim device tensor, as loss_fn returns it)."""
    from .losses import loss_fn
    with torch.no_grad():
        out = model(model_input)
        psnr, ssim = get_metrics(out, gt, fine=loss_params[0] != "coarse")
        loss = loss_fn(out, gt, loss_params)
    return dict(psnr=psnr, ssim=ssim, loss=loss)


__all__ = ["image_metrics", "get_metrics", "evaluate"]
