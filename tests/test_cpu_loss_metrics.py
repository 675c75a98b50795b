"""CPU-only checks of the loss / metrics feature (ABI 17): the argument checks of the five new C entries run
before any HIP call, the Python surface refuses host tensors, and the float64 references the GPU tests compare
against (tests/loss_metrics_ref.py) reproduce the reference's tie gradients and NaN rule and agree with a scipy
restatement of skimage's SSIM. No kernel is launched."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loss_metrics_ref import METRIC_SHAPES, loss_ref, metric_frames, ssim_psnr_ref, ssim_psnr_scipy  # noqa: E402

cf = ctypes.c_float


def test_loss_entry_points_argument_checks():
    """avr_loss_fwd / avr_loss_bwd / avr_loss_workspace_bytes: zero rays is a no-op; null pointers and an empty
    selection of terms return 1001 with a message."""
    from avr import _lib
    lib = _lib.load()
    n = ctypes.c_int64(-1)
    assert lib.avr_loss_workspace_bytes(0, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.avr_loss_workspace_bytes(2048, ctypes.byref(n)) == 0 and n.value > 0
    assert lib.avr_loss_workspace_bytes(2048, None) == 1001
    assert b"null" in lib.avr_last_error_string()
    assert lib.avr_loss_workspace_bytes(-1, ctypes.byref(n)) == 1001
    fwd, bwd = lib.avr_loss_fwd, lib.avr_loss_bwd
    for terms in (1, 2, 3, 5, 6, 7):
        assert fwd(0, terms, None, None, None, None, cf(0.5), cf(2.0), None, 0, None, None) == 0
        assert bwd(0, terms, None, None, None, None, cf(0.5), cf(2.0), None, None, None, None, None, None) == 0
        assert fwd(4, terms, None, None, None, None, cf(0.5), cf(2.0), None, 0, None, None) == 1001
        assert b"null" in lib.avr_last_error_string()
        assert bwd(4, terms, None, None, None, None, cf(0.5), cf(2.0), None, None, None, None, None, None) == 1001
        assert b"null" in lib.avr_last_error_string()
    for terms in (0, 4, 8, -1):   # no MSE term selected, or an unknown bit: refused even with zero rays
        assert fwd(0, terms, None, None, None, None, cf(0.5), cf(2.0), None, 0, None, None) == 1001
        assert b"selection of terms" in lib.avr_last_error_string()
        assert bwd(4, terms, None, None, None, None, cf(0.5), cf(2.0), None, None, None, None, None, None) == 1001
        assert b"selection of terms" in lib.avr_last_error_string()
    assert fwd(-1, 3, None, None, None, None, cf(0.5), cf(2.0), None, 0, None, None) == 1001


def test_image_metrics_entry_points_argument_checks():
    """avr_image_metrics / avr_image_metrics_workspace_bytes: zero frames is a no-op, height or width below the
    7 x 7 window and null pointers return 1001."""
    from avr import _lib
    lib = _lib.load()
    n = ctypes.c_int64(-1)
    assert lib.avr_image_metrics_workspace_bytes(0, 16, 16, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.avr_image_metrics_workspace_bytes(2, 7, 7, ctypes.byref(n)) == 0 and n.value == 2 * 16
    assert lib.avr_image_metrics_workspace_bytes(2, 128, 128, None) == 1001
    assert b"null" in lib.avr_last_error_string()
    m = lib.avr_image_metrics
    assert m(None, None, 0, 16, 16, None, 0, None, None, None) == 0
    for H, W in ((6, 16), (16, 6), (0, 0), (-3, 9)):
        assert lib.avr_image_metrics_workspace_bytes(1, H, W, ctypes.byref(n)) == 1001
        assert m(None, None, 1, H, W, None, 0, None, None, None) == 1001
        assert b">= 7" in lib.avr_last_error_string()
    assert m(None, None, 1, 16, 16, None, 0, None, None, None) == 1001
    assert b"null" in lib.avr_last_error_string()
    assert m(None, None, -1, 16, 16, None, 0, None, None, None) == 1001


def test_python_surface_refuses_host_tensors_and_bad_shapes():
    import avr
    from avr import _lib
    from avr.losses import loss_fn, loss_terms
    from avr.metrics import get_metrics, image_metrics
    assert avr.loss_fn is loss_fn and avr.get_metrics is get_metrics
    assert [loss_terms((m, r)) for m in ("coarse", "fine", "both", "anything") for r in (False, True)] == \
        [1, 5, 2, 6, 3, 7, 3, 7]
    rgb, gt, depth = torch.rand(2, 16, 3), torch.rand(2, 16, 3), torch.rand(2, 16, 1)
    with pytest.raises(_lib.AVRError):
        loss_fn((rgb, rgb, depth, None), gt, ("both", True))
    with pytest.raises(ValueError, match="img_fine"):
        loss_fn((rgb, None, depth, None), gt, ("both", False))
    with pytest.raises(ValueError, match="depth"):
        loss_fn((rgb, rgb, depth[:, :3], None), gt, ("both", True))
    with pytest.raises(_lib.AVRError):
        image_metrics(rgb, gt, 4, 4 * 2)
    with pytest.raises(_lib.AVRError):
        get_metrics((rgb, rgb, None, None), gt)
    with pytest.raises(ValueError, match="not a square"):
        get_metrics((torch.rand(2, 15, 3), torch.rand(2, 15, 3), None, None), torch.rand(2, 15, 3))
    with pytest.raises(ValueError, match="not a square"):
        get_metrics((None, torch.rand(1, 2, 63, 3), None, None), torch.rand(1, 2, 63, 3))
    with pytest.raises(ValueError):
        image_metrics(rgb, gt, 5, 5)


def test_loss_ref_ties_and_nan_rule():
    """The float64 reference: at depth == near / far exactly the penalty's gradient is -/+ 0.5 * 10000 / n
    (torch.max's backward at a tie); a NaN in an image makes the MSE part 1e-6 with no image gradient, and leaves
    the penalty and the depth gradient as they were."""
    n = 6
    g = torch.Generator().manual_seed(0)
    rgb_c, rgb_f, gt = (torch.rand(1, n, 3, generator=g, dtype=torch.float64) for _ in range(3))
    depth = torch.tensor([0.5, 2.0, 1.0, 0.25, 2.5, 0.5], dtype=torch.float64).reshape(1, n, 1).requires_grad_(True)
    loss_ref(rgb_c, rgb_f, depth, gt, ("both", True)).backward()
    want = torch.tensor([-0.5, 0.5, 0.0, -1.0, 1.0, -0.5], dtype=torch.float64) * 10000 / n
    assert torch.equal(depth.grad.reshape(n), want)

    clean = [t.clone().requires_grad_(True) for t in (rgb_c, rgb_f, depth.detach())]
    l_clean = loss_ref(*clean, gt, ("both", True))
    l_clean.backward()
    bad_f = rgb_f.clone()
    bad_f[0, 2, 1] = float("nan")
    bad = [t.clone().requires_grad_(True) for t in (rgb_c, bad_f, depth.detach())]
    l_bad = loss_ref(*bad, gt, ("both", True))
    l_bad.backward()
    penalty = 10000 * (0.25 + 0.5) / n
    assert float(l_bad.detach()) == pytest.approx(1e-6 + penalty, rel=1e-15)
    assert bad[0].grad is None and bad[1].grad is None     # the constant cut the images out of the graph
    assert torch.equal(bad[2].grad, clean[2].grad)
    mse = ((rgb_c - gt) ** 2).mean() + ((rgb_f - gt) ** 2).mean()
    assert float(l_clean.detach()) == pytest.approx(float(mse) + penalty, rel=1e-14)
    # modes
    assert float(loss_ref(rgb_c, None, None, gt, ("coarse", False))) == pytest.approx(float(((rgb_c - gt) ** 2).mean()))
    assert float(loss_ref(None, rgb_f, None, gt, ("fine", False))) == pytest.approx(float(((rgb_f - gt) ** 2).mean()))


@pytest.mark.parametrize("B,H,W", METRIC_SHAPES)
def test_ssim_psnr_ref_agrees_with_scipy_restatement(B, H, W):
    pytest.importorskip("scipy")
    for kind in ("noisy", "white", "constant", "identical"):
        img, gt = metric_frames(B, H, W, kind)
        psnr, ssim = ssim_psnr_ref(img, gt, H, W)
        psnr_s, ssim_s = ssim_psnr_scipy(img.numpy(), gt.numpy(), H, W)
        np.testing.assert_allclose(ssim.numpy(), ssim_s, rtol=0, atol=1e-14)
        if kind == "identical":
            assert np.isposinf(psnr.numpy()).all() and np.isposinf(psnr_s).all()
            assert (ssim.numpy() == 1.0).all()
        else:
            np.testing.assert_allclose(psnr.numpy(), psnr_s, rtol=0, atol=1e-12)
