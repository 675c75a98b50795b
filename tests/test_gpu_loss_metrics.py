"""avr.losses.loss_fn and avr.metrics (ABI 17: csrc/loss.hip, csrc/metrics.hip) against the float64 references
of tests/loss_metrics_ref.py: the training loss of utils.py:364-377 (every mode, the depth penalty, its ties,
the NaN rule decided on the device, a HIP-graph capture of loss + backward) and skimage's PSNR / SSIM as
get_metrics (utils.py:431-461) calls them.

Bars. Loss: one fp32 ulp of the float64 value (the kernel sums in fp64 and rounds once). Gradients: rtol 2.5e-7,
atol 1e-12 of the float64 gradients (room for three fp32 roundings; the kernel makes one). SSIM: 1e-6 absolute
(fp64 moments leave the final fp32 rounding, 6e-8). PSNR: 1e-5 dB for finite values (the fp32 rounding of a
value below 128 dB is at most 4e-6)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loss_metrics_ref import METRIC_SHAPES, loss_ref, metric_frames, ssim_psnr_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None

# wave and workgroup boundaries, train.py's 4 x 512, the last single-workgroup size and the first with two
# (8 x 1024 colour values per workgroup), and one that needs many workgroups
RAYS = [1, 63, 64, 65, 257, 2048, 2730, 2731, 70001]
MODES = ["coarse", "fine", "both"]


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def _inputs(n, seed=0):
    """CPU fp32 (rgb_c, rgb_f, depth, gt) for n rays; depths in [0.2, 2.4]: both penalty arms and the dead zone.
    Shared by the tests and never modified (the tests clone)."""
    g = torch.Generator().manual_seed(17 * n + seed)
    rgb_c, rgb_f, gt = (torch.rand(1, n, 3, generator=g) for _ in range(3))
    depth = 0.2 + 2.2 * torch.rand(1, n, 1, generator=g)
    return rgb_c, rgb_f, depth, gt


@functools.lru_cache(maxsize=None)
def _reference(n, mode, reg, seed=0):
    """float64 loss and gradients (None for an input outside the loss) of _inputs(n)."""
    rgb_c, rgb_f, depth, gt = _inputs(n, seed)
    leaves = [t.double().requires_grad_(True) for t in (rgb_c, rgb_f, depth)]
    loss = loss_ref(*leaves, gt, (mode, reg))
    loss.backward()
    return loss.detach(), tuple(t.grad for t in leaves)


def _run(n, mode, reg, scale=None, flat_depth=False, seed=0, patch=None):
    """loss_fn + backward on the device -> (loss, [grad rgb_c, grad rgb_f, grad depth]) as CPU tensors."""
    from avr.losses import loss_fn
    rgb_c, rgb_f, depth, gt = (t.clone() for t in _inputs(n, seed))
    if patch is not None:
        patch(rgb_c, rgb_f, depth)
    if flat_depth:
        depth = depth.reshape(1, n)
    leaves = [t.to(DEV).requires_grad_(True) for t in (rgb_c, rgb_f, depth)]
    loss = loss_fn((*leaves, None), gt.to(DEV), (mode, reg))
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda
    (loss if scale is None else scale * loss).backward()
    return loss.detach().cpu(), [None if t.grad is None else t.grad.cpu() for t in leaves]


def _check_loss(got, ref):
    ref = float(ref)
    err = abs(float(got.double()) - ref)
    print(f"loss {float(got):.9g} vs float64 {ref:.12g}: error {err / abs(ref):.2e} relative")
    assert err <= 2.0 ** -23 * abs(ref)


def _check_grads(got, ref, scale=1.0):
    for name, a, b in zip(("rgb_c", "rgb_f", "depth"), got, ref):
        assert (a is None) == (b is None), name
        if a is None:
            continue
        b = scale * b.reshape(a.shape)
        err = (a.double() - b).abs()
        bound = 1e-12 + 2.5e-7 * b.abs()
        print(f"grad {name}: worst error {float((err / b.abs().clamp_min(1e-30)).max()):.2e} relative")
        assert bool((err <= bound).all()), f"{name}: {int((err > bound).sum())} of {a.numel()} values off"


@pytest.mark.parametrize("reg", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", RAYS)
def test_loss_and_gradients_match_float64(n, mode, reg):
    ref_loss, ref_grads = _reference(n, mode, reg)
    loss, grads = _run(n, mode, reg, flat_depth=bool(n % 2))
    _check_loss(loss, ref_loss)
    _check_grads(grads, ref_grads)
    # the upstream gradient is a device scalar the backward kernel reads
    loss3, grads3 = _run(n, mode, reg, scale=3.0)
    assert _bits_equal(loss3, loss)
    _check_grads(grads3, ref_grads, scale=3.0)


def test_penalty_ties_follow_torch_max():
    """depth == near / far exactly: -/+ 0.5 * 10000 / n, as torch.max(a, b)'s backward."""
    from avr.losses import loss_fn
    n = 8
    depth = torch.tensor([0.5, 2.0, 1.0, 0.25, 2.5, 0.5, 2.0, 1.9999999], device=DEV).reshape(1, n, 1)
    depth.requires_grad_(True)
    rgb = torch.rand(1, n, 3, device=DEV)
    loss_fn((rgb, rgb, depth, None), torch.rand(1, n, 3, device=DEV), ("both", True)).backward()
    want = torch.tensor([-0.5, 0.5, 0.0, -1.0, 1.0, -0.5, 0.5, 0.0]) * 10000 / n
    assert torch.equal(depth.grad.reshape(n).cpu(), want)
    near, far = 0.8, 1.8     # not fp32 values: the ties sit at the fp32 roundings, as in the reference's fp32 loss
    d2 = torch.tensor([near, far, 1.0], device=DEV).reshape(1, 3).requires_grad_(True)
    loss_fn((rgb[:, :3], None, d2, None), rgb[:, :3], ("coarse", True), near=near, far=far).backward()
    assert torch.equal(d2.grad.reshape(3).cpu(), torch.tensor([-0.5, 0.5, 0.0]) * 10000 / 3)


def test_nan_rule_on_device():
    """One NaN in rgb_fine, mode both, regularisation on: the MSE part becomes 1e-6, both images get exactly zero
    gradient, the penalty and the depth gradient are those of the clean run."""
    from avr.losses import loss_parts
    n = 257

    def poison(rgb_c, rgb_f, depth):
        rgb_f[0, 100, 1] = float("nan")

    clean_loss, clean_grads = _run(n, "both", True)
    loss, grads = _run(n, "both", True, patch=poison)
    rgb_c, rgb_f, depth, gt = _inputs(n)
    penalty = (torch.relu(0.5 - depth.double()) + torch.relu(depth.double() - 2.0)).mean() * 10000
    _check_loss(loss, float(np.float32(1e-6)) + penalty)
    assert torch.equal(grads[0], torch.zeros(1, n, 3)) and torch.equal(grads[1], torch.zeros(1, n, 3))
    assert _bits_equal(grads[2], clean_grads[2])
    assert float(clean_loss) > float(loss)
    # without the penalty the loss is the constant itself
    loss0, grads0 = _run(n, "both", False, patch=poison)
    assert float(loss0) == float(np.float32(1e-6)) and grads0[2] is None
    assert not grads0[0].any() and not grads0[1].any()
    # mode coarse does not read rgb_fine: the NaN there changes nothing
    loss_c, grads_c = _run(n, "coarse", True, patch=poison)
    _check_loss(loss_c, _reference(n, "coarse", True)[0])
    _check_grads(grads_c, _reference(n, "coarse", True)[1])
    # the record keeps the parts as summed
    bad_f = rgb_f.clone()
    poison(None, bad_f, None)
    rec = loss_parts((rgb_c.to(DEV), bad_f.to(DEV), depth.to(DEV), None), gt.to(DEV), ("both", True)).cpu()
    assert float(rec[0]) == float(loss) and torch.isnan(rec[2]) and torch.isfinite(rec[1])
    assert abs(float(rec[3]) - float(penalty)) <= 2.0 ** -23 * float(penalty)
    # a non-finite depth is not guarded (the reference guards the MSE part only)
    def bad_depth(rgb_c, rgb_f, depth):
        depth[0, 5, 0] = float("nan")
    assert torch.isnan(_run(n, "both", True, patch=bad_depth)[0])


def test_img_fine_none():
    from avr.losses import loss_fn
    rgb_c, _, depth, gt = (t.to(DEV) for t in _inputs(257))
    rgb_c.requires_grad_(True)
    loss = loss_fn((rgb_c, None, depth, None), gt, ("coarse", True))
    loss.backward()
    _check_loss(loss.detach().cpu(), _reference(257, "coarse", True)[0])
    _check_grads([rgb_c.grad.cpu(), None, None], [_reference(257, "coarse", True)[1][0], None, None])
    with pytest.raises(ValueError, match="img_fine"):
        loss_fn((rgb_c, None, depth, None), gt, ("both", True))


def test_loss_is_bit_deterministic():
    a_loss, a_grads = _run(70001, "both", True)
    b_loss, b_grads = _run(70001, "both", True)
    assert _bits_equal(a_loss, b_loss)
    assert all(_bits_equal(a, b) for a, b in zip(a_grads, b_grads))


def test_loss_and_backward_in_a_graph_capture():
    """loss_fn + backward recorded in a torch.cuda.graph on leaf tensors, replayed after in-place refills (one
    with a NaN): every replay equals the eager call bit for bit. The reference's `if loss.isnan()` is a host
    sync, which a capture refuses."""
    from avr.losses import loss_fn
    n = 257
    leaves = [t.to(DEV).requires_grad_(True) for t in _inputs(n)[:3]]
    gt = _inputs(n)[3].to(DEV)

    def step(ts, target):
        loss = loss_fn((*ts, None), target, ("both", True))
        return loss, torch.autograd.grad(loss, ts)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(leaves, gt)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_loss, g_grads = step(leaves, gt)
    for seed in (0, 1, 2):
        new = [t.clone() for t in _inputs(n, seed)]
        if seed == 2:
            new[0][0, 7, 2] = float("nan")
        with torch.no_grad():
            for dst, src in zip(leaves + [gt], new):
                dst.copy_(src)
        graph.replay()
        eager = [t.to(DEV).requires_grad_(True) for t in new[:3]]
        e_loss, e_grads = step(eager, new[3].to(DEV))
        assert _bits_equal(g_loss.detach(), e_loss.detach())
        assert all(_bits_equal(a, b) for a, b in zip(g_grads, e_grads))
        if seed == 2:
            assert not g_grads[0].any() and not g_grads[1].any() and g_grads[2].any()
            assert bool(torch.isfinite(g_loss))
    assert not _bits_equal(g_grads[2], torch.zeros_like(g_grads[2]))


def test_loss_through_the_renderer():
    """VolumeRenderer in training mode at 1 x 64 rays, mode both with the depth penalty (near / far of the loss
    set inside the rendered depths, so both arms and the dead zone act on the depth gradient): the net gradients
    of loss_fn against those of the torch expression of the same loss on the same outputs, each measured against
    the float64 expression pushed through the same fp32 backward -- the bar of tests/test_gpu_train.py (twice torch
    fp32's own error, or 3e-5 of a parameter's max |grad|)."""
    from test_gpu_train import _compare64, _net
    from avr.losses import loss_fn
    from avr.renderers import VolumeRenderer
    from avr.scene import INTRINSICS
    net = _net(64, 3, 64, (8, 8)).train()
    net.hip_backward = True
    R = 64
    g = torch.Generator(device="cpu").manual_seed(5)
    x_pix = torch.rand(1, R, 2, generator=g).to(DEV)
    c2w = torch.eye(4).reshape(1, 1, 4, 4).expand(1, R, 4, 4).clone()
    c2w[..., 2, 3] = -1.3
    c2w = c2w.to(DEV)
    K = torch.tensor([INTRINSICS], device=DEV)
    gt = torch.rand(1, R, 3, generator=g).to(DEV)
    rend = VolumeRenderer(0.8, 1.8, 32, 16, 4, 0.01, True)
    rend.seed = 11
    named = [(k, p) for k, p in net.named_parameters() if p.requires_grad]

    def render():
        """The same forward again (Philox draws keyed by seed and offset; the training paths are deterministic):
        the field's backward frees its saved state, so every loss gets a graph of its own."""
        rend._offset = 0
        return rend(c2w, K, x_pix, net)

    def grads(loss):
        gs = torch.autograd.grad(loss, [p for _, p in named], allow_unused=True)
        return {k: v for (k, _), v in zip(named, gs) if v is not None}

    first = render()
    assert first[2].requires_grad
    d = first[2].detach().flatten().sort().values
    near, far = float(d[R // 3]), float(d[2 * R // 3])   # a third of the rays below near, a third above far

    def expression(out, dtype):
        c, f, dd, t = out[0].to(dtype), out[1].to(dtype), out[2].to(dtype), gt.to(dtype)
        penalty = torch.max(near - dd, torch.zeros_like(dd)) + torch.max(dd - far, torch.zeros_like(dd))
        return ((c - t) ** 2).mean() + ((f - t) ** 2).mean() + torch.mean(penalty) * 10000

    hip_loss = loss_fn(first, gt, ("both", True), near=near, far=far)
    g_hip = grads(hip_loss)
    out = render()
    assert all(_bits_equal(a.detach(), b.detach()) for a, b in zip(out[:3], first[:3]))
    g_t32 = grads(expression(out, torch.float32))
    out = render()
    f64_loss = expression(out, torch.float64)
    g_64 = grads(f64_loss)
    _check_loss(hip_loss.detach().cpu(), f64_loss.detach().cpu())
    assert any(k.startswith("mlp_fine.") for k in g_hip) and any(k.startswith("mlp_coarse.") for k in g_hip)
    worst = _compare64(g_hip, g_t32, g_64)
    print(f"renderer step: worst loss_fn gradient error {worst:.2e} of max |grad|")
    # the depth penalty reaches the net: without it the fine MLP's gradient differs
    g_plain = grads(loss_fn(render(), gt, ("both", False)))
    assert any(not torch.equal(g_plain[k], g_hip[k]) for k in g_hip if k.startswith("mlp_fine."))


@functools.lru_cache(maxsize=None)
def _metric_case(B, H, W, kind):
    img, gt = metric_frames(B, H, W, kind)
    return img, gt, ssim_psnr_ref(img, gt, H, W)


@pytest.mark.parametrize("B,H,W", METRIC_SHAPES)
def test_image_metrics_match_float64(B, H, W):
    from avr.metrics import image_metrics
    for kind in ("noisy", "white", "constant", "identical"):
        img, gt, (ref_psnr, ref_ssim) = _metric_case(B, H, W, kind)
        a, b = img.to(DEV), gt.to(DEV)
        psnr, ssim = image_metrics(a, b, H, W)
        psnr2, ssim2 = image_metrics(a.reshape(B, H, W, 3), b.reshape(B, H, W, 3), H, W)
        assert psnr.shape == (B,) and ssim.shape == (B,) and psnr.dtype == torch.float32 and psnr.is_cuda
        assert _bits_equal(psnr, psnr2) and _bits_equal(ssim, ssim2)
        psnr, ssim = psnr.cpu().double(), ssim.cpu().double()
        print(f"{kind} {B}x{H}x{W}: ssim {ssim.tolist()} (error {float((ssim - ref_ssim).abs().max()):.2e}), "
              f"psnr {psnr.tolist()} (error {float((psnr - ref_psnr).abs().nan_to_num(0).max()):.2e} dB)")
        if kind == "identical":
            assert bool((ssim == 1.0).all()) and bool(torch.isposinf(psnr).all())
            continue
        assert bool(torch.isfinite(ref_psnr).all())
        assert bool(((ssim - ref_ssim).abs() <= 1e-6).all())
        assert bool(((psnr - ref_psnr).abs() <= 1e-5).all())


def test_get_metrics_returns_the_last_frame():
    """(SB, NV, sl^2, 3) with SB = 2, NV = 2, sl = 16: the reference returns np.mean of its loop variables, the
    last frame's pair (utils.py:461), not the mean over the frames."""
    from avr.metrics import get_metrics, image_metrics
    img, gt, (ref_psnr, ref_ssim) = _metric_case(4, 16, 16, "noisy")
    a, b = img.reshape(2, 2, 256, 3).to(DEV), gt.reshape(2, 2, 256, 3).to(DEV)
    psnr, ssim = get_metrics((None, a, None, None), b)
    assert isinstance(psnr, float) and isinstance(ssim, float)
    all_psnr, all_ssim = image_metrics(a, b, 16, 16)
    assert psnr == float(all_psnr[-1]) and ssim == float(all_ssim[-1])
    assert abs(psnr - float(ref_psnr[-1])) <= 1e-5 and abs(ssim - float(ref_ssim[-1])) <= 1e-6
    assert abs(ssim - float(ref_ssim.mean())) > 1e-4          # the frames differ: not the mean
    # the coarse image with fine=False, in the (SB, sl^2, 3) form
    p3, s3 = get_metrics((a[:, 1], None, None, None), b[:, 1], fine=False)
    assert (p3, s3) == (psnr, ssim)


def test_evaluate_is_its_pieces():
    """evaluate (test.py:47-57, train.py:152-155) on a 16 x 16 frame of the synthetic scene."""
    from avr.losses import loss_fn
    from avr.metrics import evaluate, get_metrics
    from avr.models import RadFieldAndRenderer
    from avr.renderers import VolumeRenderer
    from avr.scene import INTRINSICS, synthetic_scene
    net = synthetic_scene(DEV, 0, latent_hw=(16, 16))
    rend = VolumeRenderer(0.8, 1.8, 32, 16, 4, 0.01, True)
    rend.seed = 3
    model = RadFieldAndRenderer(net, rend)
    sl = 16
    ys, xs = torch.meshgrid(torch.arange(sl), torch.arange(sl), indexing="ij")
    x_pix = ((torch.stack([xs, ys], -1).reshape(1, sl * sl, 2).float() + 0.5) / sl).to(DEV)
    c2w = torch.eye(4).reshape(1, 1, 4, 4).repeat(1, sl * sl, 1, 1)
    c2w[..., 2, 3] = -1.3
    model_input = {"cam2world": c2w.to(DEV), "intrinsics": torch.tensor([INTRINSICS], device=DEV), "x_pix": x_pix}
    gt = torch.rand(1, sl * sl, 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    for params in (("both", True), ("coarse", False)):
        rend._offset = 0
        res = evaluate(model, model_input, gt, params)
        rend._offset = 0
        with torch.no_grad():
            out = model(model_input)
            psnr, ssim = get_metrics(out, gt, fine=params[0] != "coarse")
            loss = loss_fn(out, gt, params)
        assert set(res) == {"psnr", "ssim", "loss"}
        assert (res["psnr"], res["ssim"]) == (psnr, ssim) and _bits_equal(res["loss"], loss)
        assert np.isfinite(psnr) and -1.0 <= ssim < 1.0 and not res["loss"].requires_grad
