"""train.py's loss (utils.py:364-377) on the device: `from avr.losses import loss_fn` replaces
`from utils import loss_fn`.

    loss = [mse(img_coarse, gt)] + [mse(img_fine, gt)] + [10000 * mean(max(near - depth, 0) + max(depth - far, 0))]

One HIP pass forward (avr_loss_fwd: fp64 sums combined in a fixed order, bit-identical from run to run) and one
launch backward (avr_loss_bwd), against about 15 launches of the torch expression. The reference's
`if loss.isnan(): loss = 1e-6` is a device-to-host sync on every step; here the decision is taken on the device
(DESIGN Q9), so loss_fn + backward can be recorded in a torch.cuda.graph (avr.graphs.GraphedTrainStep's step_fn).
No CPU path: host tensors raise AVRError.
"""
import functools

import torch

from ._lib import call, ptr, require_device, size_query, stream_of

F32 = torch.float32
COARSE, FINE, DEPTH = 1, 2, 4   # avr.h AVR_LOSS_*


def _f32c(t):
    return t if (t.dtype == F32 and t.is_contiguous()) else t.to(F32).contiguous()


@functools.lru_cache(maxsize=64)
def _workspace_bytes(n):
    return size_query("avr_loss_workspace_bytes", n)


def loss_terms(loss_params):
    """(mode, depth_regularization) -> the AVR_LOSS_* selection: the coarse MSE unless mode == 'fine', the fine
    MSE unless mode == 'coarse' (any other string: both, as the reference), the depth penalty if asked."""
    mode, reg = loss_params[0], loss_params[1]
    return (COARSE if mode != "fine" else 0) | (FINE if mode != "coarse" else 0) | (DEPTH if reg else 0)


def _forward(rgb_c, rgb_f, depth, gt, terms, near, far):
    """-> record (4,) = [loss, mse_coarse, mse_fine, penalty] (avr_loss_fwd)."""
    n = gt.numel() // 3
    record = torch.empty(4, device=gt.device, dtype=F32)
    ws = torch.empty(_workspace_bytes(n), device=gt.device, dtype=torch.uint8)
    call("avr_loss_fwd", n, terms, ptr(rgb_c), ptr(rgb_f), ptr(depth), ptr(gt), near, far, ptr(ws), ws.numel(),
         ptr(record), stream_of(gt))
    return record


class _Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb_c, rgb_f, depth, gt, terms, near, far):
        record = _forward(rgb_c, rgb_f, depth, gt, terms, near, far)
        ctx.save_for_backward(rgb_c, rgb_f, depth, gt, record)
        ctx.conf = (terms, near, far)
        return record[0]

    @staticmethod
    def backward(ctx, g):
        rgb_c, rgb_f, depth, gt, record = ctx.saved_tensors
        terms, near, far = ctx.conf
        g = _f32c(g)
        require_device(g)
        need = ctx.needs_input_grad
        g_c = torch.empty_like(rgb_c) if need[0] else None
        g_f = torch.empty_like(rgb_f) if need[1] else None
        g_d = torch.empty_like(depth) if need[2] else None
        call("avr_loss_bwd", gt.numel() // 3, terms, ptr(rgb_c), ptr(rgb_f), ptr(depth), ptr(gt), near, far,
             ptr(record), ptr(g), ptr(g_c), ptr(g_f), ptr(g_d), stream_of(gt))
        return g_c, g_f, g_d, None, None, None, None


def _inputs(mlp_out, gt, loss_params):
    img_coarse, img_fine, depth, _ = mlp_out
    terms = loss_terms(loss_params)
    rgb_c = img_coarse if terms & COARSE else None
    rgb_f = img_fine if terms & FINE else None
    depth = depth if terms & DEPTH else None
    if terms & COARSE and rgb_c is None:
        raise ValueError(f"loss mode {loss_params[0]!r} needs img_coarse")
    if terms & FINE and rgb_f is None:
        raise ValueError(f"loss mode {loss_params[0]!r} needs img_fine (a coarse-only renderer trains with "
                         "loss mode 'coarse')")
    if terms & DEPTH and depth is None:
        raise ValueError("depth regularization needs the depth output")
    if gt.numel() == 0 or gt.shape[-1] != 3:
        raise ValueError(f"gt of shape {tuple(gt.shape)}: (..., 3) with at least one ray")
    n = gt.numel() // 3
    for name, t, size in (("img_coarse", rgb_c, 3 * n), ("img_fine", rgb_f, 3 * n), ("depth", depth, n)):
        if t is not None and t.numel() != size:
            raise ValueError(f"{name} of shape {tuple(t.shape)} against gt of shape {tuple(gt.shape)}")
    tensors = [None if t is None else _f32c(t) for t in (rgb_c, rgb_f, depth)] + [_f32c(gt.detach())]
    require_device(*tensors)
    return tensors, terms


def loss_fn(mlp_out, gt, loss_params, near=0.5, far=2.0):
    """loss_fn of utils.py:364-377: mlp_out = (img_coarse, img_fine, depth, _) as the renderers return it
    (img_fine may be None with loss mode 'coarse'; depth (SB, R, 1) or (SB, R)), gt (SB, R, 3), loss_params =
    (mode, depth_regularization). Returns the loss as a 0-dim fp32 device tensor with autograd into the two
    images and the depth. No host sync and no data-dependent allocation.

    The reference's quirks, kept: the MSE part alone is guarded against NaN (it becomes 1e-6, and the images then
    get exactly zero gradient), the penalty is added after the guard and a non-finite depth reaches the loss;
    at depth == near / far exactly the penalty's gradient is half the slope (torch.max's backward at a tie; DESIGN Q9, Q10)."""
    (rgb_c, rgb_f, depth, gt), terms = _inputs(mlp_out, gt, loss_params)
    return _Loss.apply(rgb_c, rgb_f, depth, gt, terms, float(near), float(far))


def loss_parts(mlp_out, gt, loss_params, near=0.5, far=2.0):
    """The forward's record for logging, without autograd: a (4,) fp32 device tensor [loss, mse_coarse,
    mse_fine, penalty] (the MSEs as summed: NaN where the guard replaced the part; 0 for a term left out)."""
    (rgb_c, rgb_f, depth, gt), terms = _inputs(mlp_out, gt, loss_params)
    with torch.no_grad():
        return _forward(rgb_c, rgb_f, depth, gt, terms, float(near), float(far))


__all__ = ["loss_fn", "loss_parts", "loss_terms"]
