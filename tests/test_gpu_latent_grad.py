"""d loss / d latent map on the HIP path (avr_latent_features_adjoint: the pixel-aligned lookup's adjoint onto the
maps, an inverted index and a per-texel sum with no float atomics): the op against torch's float64 grid_sample
input gradient, its chunked walk under skew, bit-reproducibility, the three training Functions' wiring
(FusedField.last_latent_grad), torch's deterministic mode, points and maps together, a real encoder behind the maps
and a captured training step. The yardstick is tests/test_gpu_train.py's: against float64, the HIP error relative
to max |grad| is at most twice PyTorch fp32 autograd's own error plus 3e-5."""
import math

import pytest
import torch

from test_gpu_train import _compare64, _fp64, _grads, _net, _points

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


# ------------------------------------------------------------------ the op alone
def _views(n_scenes, hw):
    """ViewDesc array of n_scenes source views of (H, W) maps (128 x 128 images): the synthetic scene's camera,
    each scene turned about y and shifted, so that the rotation, the translation and both map axes matter."""
    from avr._lib import ViewDesc
    H, W = hw
    views = (ViewDesc * n_scenes)()
    for s, v in enumerate(views):
        a = 0.15 * s
        R = [[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]]
        t = [0.05 * s, -0.03 * s, 1.3]
        v.poses[:] = [float(x) for i in range(3) for x in (R[i] + [t[i]])]
        v.focal[:] = [131.25, -131.25]
        v.c[:] = [64.0, 64.0]
        v.image_shape[:] = [128.0, 128.0]
        v.latent_scaling[:] = [W / (W - 1) * 2.0, H / (H - 1) * 2.0]     # encoder.py: (W, H) / (W - 1, H - 1) * 2
        v.latent_h, v.latent_w = H, W
    return views


def _op_points(views, n_points, seed, spread=1.6):
    """(n_scenes, n_points, 3) points of which about a third project outside the frame (spread), the first ones
    placed on texel centres of scene 0's view -- the last row and column among them (ix == W - 1, iy == H - 1)."""
    S = len(views)
    g = torch.Generator(device="cpu").manual_seed(seed)
    xyz = (torch.rand(S, n_points, 3, generator=g) - 0.5) * spread
    H, W = views[0].latent_h, views[0].latent_w
    centres = [(W - 1, H - 1), (0, 0), (W - 1, 0), (0, H - 1), (W // 2, H - 1), (W - 1, H // 2), (1, 1), (2, 3)]
    for i, (kx, ky) in enumerate(centres[:n_points]):
        # scene 0 has R = I, t = (0, 0, 1.3): z = -0.3 puts the point at camera depth 1; u = 128 kx / W is texel kx
        u, w = 128.0 * kx / W, 128.0 * ky / H
        xyz[:, i] = torch.tensor([(64.0 - u) / 131.25, (64.0 - w) / -131.25, -0.3])
    return xyz


def _grid_sample_grad(views, xyz, g_feat, hw, dtype):
    """torch's grid_sample input gradient (bilinear, border, align_corners=True) of the same views and points in
    `dtype` -> (n_scenes, C, H, W): NewPixelNeRFNet's projection (models.py:753-760) and SpatialEncoder.index."""
    H, W = hw
    S, N, _ = xyz.shape
    C = g_feat.shape[1]
    f32 = torch.float32
    out = []
    for s, v in enumerate(views):
        P = torch.tensor(list(v.poses), dtype=f32).reshape(3, 4).to(dtype)
        # the view's fp32 constants, as the library forms them (latent_scaling / image_shape in fp32)
        scale = (torch.tensor(list(v.latent_scaling), dtype=f32) / torch.tensor(list(v.image_shape), dtype=f32))
        x = xyz[s].cpu().to(dtype)
        xc = x @ P[:, :3].t() + P[:, 3]
        uv = -xc[:, :2] / xc[:, 2:] * torch.tensor(list(v.focal), dtype=f32).to(dtype)
        uv = uv + torch.tensor(list(v.c), dtype=f32).to(dtype)
        grid = uv * scale.to(dtype) - 1.0
        lat = torch.zeros(1, C, H, W, dtype=dtype, requires_grad=True)
        smp = torch.nn.functional.grid_sample(lat, grid.reshape(1, N, 1, 2), mode="bilinear", padding_mode="border",
                                              align_corners=True)
        smp.backward(g_feat[s * N:(s + 1) * N].cpu().to(dtype).t().reshape(1, C, N, 1))
        out.append(lat.grad[0])
    return torch.stack(out)


def _adjoint(views, xyz, g_feat, hw):
    """ops.latent_features_adjoint's (S, H*W, C) as (S, C, H, W) on the CPU."""
    from avr import ops
    H, W = hw
    S = xyz.shape[0]
    got = ops.latent_features_adjoint(views, xyz.to(DEV), g_feat.to(DEV), hw)
    assert got.shape == (S, H * W, g_feat.shape[1]) and got.dtype == torch.float32
    return got.reshape(S, H, W, -1).permute(0, 3, 1, 2).cpu()


@pytest.mark.parametrize("hw", [(8, 8), (5, 7)], ids=["8x8", "5x7"])
@pytest.mark.parametrize("n_scenes", [1, 3])
@pytest.mark.parametrize("C", [64, 512, 1024])
def test_adjoint_matches_float64_grid_sample(C, n_scenes, hw):
    """The op against the float64 grid_sample gradient: partial / two / four 256-channel lane groups, a square and
    a non-square map (a W / H swap shows), 1 and 3 scenes, ragged point counts and none, a third of the points
    out of frame, points on texel centres and on the last row and column."""
    views = _views(n_scenes, hw)
    for n_points in (0, 1, 63, 65, 700):
        xyz = _op_points(views, n_points, seed=C + n_points)
        g = torch.Generator(device="cpu").manual_seed(n_points + 1)
        g_feat = torch.randn(n_scenes * n_points, C, generator=g)
        got = _adjoint(views, xyz, g_feat, hw)
        if n_points == 0:
            assert bool((got == 0).all())
            continue
        ref = _grid_sample_grad(views, xyz, g_feat, hw, torch.float64)
        t32 = _grid_sample_grad(views, xyz, g_feat, hw, torch.float32)
        worst = _compare64({"latent": got}, {"latent": t32}, {"latent": ref})
        print(f"C {C} scenes {n_scenes} map {hw} points {n_points}: HIP error {worst:.2e} of max |grad|")
    if n_points:
        # the inputs do what the docstring says: about a third of the last case's points leave the frame
        H, W = hw
        assert float(ref[:, :, [0, H - 1], :].abs().max()) > 0 and float(ref[:, :, :, [0, W - 1]].abs().max()) > 0


def test_adjoint_strided_gradient_rows():
    """grad_features rows with a leading dimension past the channel count (ld_grad > channels)."""
    hw, C = (5, 7), 64
    views = _views(2, hw)
    xyz = _op_points(views, 130, seed=4)
    g = torch.Generator(device="cpu").manual_seed(8)
    wide = torch.randn(2 * 130, C + 8, generator=g).to(DEV)
    got = _adjoint(views, xyz, wide[:, :C], hw)
    ref = _grid_sample_grad(views, xyz, wide[:, :C], hw, torch.float64)
    t32 = _grid_sample_grad(views, xyz, wide[:, :C], hw, torch.float32)
    _compare64({"latent": got}, {"latent": t32}, {"latent": ref})
    # a column-offset view: rows off 16-B alignment are copied by the op, not refused by the library
    got = _adjoint(views, xyz, wide[:, 1:C + 1], hw)
    ref = _grid_sample_grad(views, xyz, wide[:, 1:C + 1], hw, torch.float64)
    t32 = _grid_sample_grad(views, xyz, wide[:, 1:C + 1], hw, torch.float32)
    _compare64({"latent": got}, {"latent": t32}, {"latent": ref})


@pytest.mark.parametrize("extra", ["chunk-1", "chunk", "chunk+1", "2chunk+1"])
def test_adjoint_skewed_lists_and_chunks(extra):
    """Every point of a scene projects past one corner of the frame (border padding), so one texel receives all of
    them: list lengths around the gather's chunk. Scene 0 lands on the last texel, scene 1 on texel 0 -- whose
    cell the walks of texels (0, 1), (1, 0) and (1, 1) also read, chunk by chunk, with zero weights. Same
    yardstick; every other texel is exactly 0.0."""
    from avr import _lib
    chunk = _lib.LATENT_ADJOINT_CHUNK
    n = {"chunk-1": chunk - 1, "chunk": chunk, "chunk+1": chunk + 1, "2chunk+1": 2 * chunk + 1}[extra]
    hw, C = (5, 7), 64
    H, W = hw
    views = _views(2, hw)
    g = torch.Generator(device="cpu").manual_seed(n)
    xyz = (torch.rand(2, n, 3, generator=g) - 0.5) * 0.2
    # scene s sees x - 3 (s = 0) / x + 3 (s = 1) of the camera axis: u = -xc_x / xc_z * f + c far past either edge,
    # and fy < 0 sends y the other way
    xyz[0, :, 0] -= 3.0
    xyz[0, :, 1] += 3.0
    xyz[1, :, 0] += 3.0
    xyz[1, :, 1] -= 3.0
    g_feat = torch.randn(2 * n, C, generator=g)
    got = _adjoint(views, xyz, g_feat, hw)
    ref = _grid_sample_grad(views, xyz, g_feat, hw, torch.float64)
    t32 = _grid_sample_grad(views, xyz, g_feat, hw, torch.float32)
    hit = torch.zeros(2, 1, H, W, dtype=torch.bool)
    hit[0, 0, H - 1, W - 1] = hit[1, 0, 0, 0] = True
    assert bool((ref[~hit.expand_as(ref)] == 0).all()) and float(ref[0, :, H - 1, W - 1].abs().min()) > 0
    assert float(ref[1, :, 0, 0].abs().min()) > 0, "the points must all land on the two corner texels"
    _compare64({"latent": got}, {"latent": t32}, {"latent": ref})
    assert bool((got[~hit.expand_as(got)] == 0.0).all())


def test_adjoint_is_bit_reproducible():
    """The same inputs three times, other kernels launched in between: torch.equal (no float atomics, no
    data-dependent order)."""
    from avr import ops
    hw, C, S, n = (8, 8), 512, 3, 700
    views = _views(S, hw)
    xyz = _op_points(views, n, seed=C + n).to(DEV)
    g_feat = torch.randn(S * n, C, generator=torch.Generator(device="cpu").manual_seed(n + 1)).to(DEV)
    runs = []
    for i in range(3):
        runs.append(ops.latent_features_adjoint(views, xyz, g_feat, hw).clone())
        junk = torch.randn(1 << (18 + i), device=DEV)         # other work between the runs
        (junk @ junk).item()
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert float(runs[0].abs().max()) > 0


# ------------------------------------------------------------------ wired into the training Functions
def test_field_train_latent_grad_is_bit_reproducible():
    """latent.grad of a whole _FieldTrain step (SB 2, fine MLP), three times: torch.equal."""
    net = _net(128, 3, 64, (8, 8), sb=2)
    xyz, vd, w = _points(2, 700, seed=3)
    runs = [_grads(net, xyz, vd, w, False, hip=True, latent_grad=True)[2] for _ in range(3)]
    assert net.fused().last_latent_grad == "hip"
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


def _fused_case(monkeypatch=None, via_autograd=False):
    net = _net(128, 3, 64, (8, 8), sb=2)
    xyz, vd, w = _points(2, 700, seed=3)
    if via_autograd:
        monkeypatch.setenv("AVR_LATENT_GRAD_VIA_AUTOGRAD", "1")
    _, g_h, l_h = _grads(net, xyz, vd, w, False, hip=True, latent_grad=True)
    path = net.fused().last_latent_grad
    _, g_t, l_t = _grads(net, xyz, vd, w, False, hip=False, latent_grad=True)
    _, g_d, l_d = _fp64(net, lambda: _grads(net, xyz.double(), vd.double(), w.double(), False, hip=False,
                                             latent_grad=True))
    worst = _compare64(dict(g_h, latent=l_h), dict(g_t, latent=l_t), dict(g_d, latent=l_d))
    return path, worst


def test_fused_path_takes_latent_grad_from_hip():
    """_FieldTrain: d_hidden 128, 3 blocks, SB 2, fine MLP, 700 points, the maps' gradient wanted."""
    path, worst = _fused_case()
    assert path == "hip"
    print(f"fused: worst HIP gradient error vs float64 {worst:.2e} of max |grad|")


def test_fused_path_autograd_switch(monkeypatch):
    """AVR_LATENT_GRAD_VIA_AUTOGRAD=1: the earlier path (torch's grid_sample adjoint), reported and still right."""
    path, _ = _fused_case(monkeypatch, via_autograd=True)
    assert path == "autograd"


def test_bn_path_takes_latent_grad_from_hip():
    """train.py --bn (avr.bn_train), d_hidden 64: the parameters under that path's own yardstick
    (tests/test_gpu_train_bn.py: fc_0's bias has an exactly zero gradient under batch statistics), the maps'
    gradient under this file's."""
    from test_gpu_train_bn import _bn_net, _compare64 as _compare64_bn, _grads_bn
    net = _bn_net(64, 3, sb=2)
    xyz, vd, w = _points(2, 700, seed=5)
    _, g_h, l_h = _grads_bn(net, xyz, vd, w, True, hip=True, latent_grad=True)
    assert net.fused().last_latent_grad == "hip"
    _, g_t, l_t = _grads_bn(net, xyz, vd, w, True, hip=False, latent_grad=True)
    _, g_d, l_d = _fp64(net, lambda: _grads_bn(net, xyz.double(), vd.double(), w.double(), True, hip=False,
                                                latent_grad=True))
    _compare64_bn(g_h, g_t, g_d)
    _compare64({"latent": l_h}, {"latent": l_t}, {"latent": l_d})


def test_layer_path_takes_latent_grad_from_hip(monkeypatch):
    """avr.layer_train with NS = 2 source views and use_spade, d_hidden 64: tests/test_gpu_layer_train.py's check
    of every gradient (the `latent` entry included, against float64 on the HIP forward's branch) with the maps'
    gradient seen to come from the HIP adjoint, per (object, view) map."""
    from avr import train_common
    from test_gpu_layer_train import _check_case
    seen = []
    orig = train_common.latent_grad_hip

    def spy(fused, latent, xyz, g_feat, ns=1):
        out = orig(fused, latent, xyz, g_feat, ns)
        seen.append((fused, ns, tuple(out.shape), tuple(latent.shape)))
        return out
    monkeypatch.setattr(train_common, "latent_grad_hip", spy)
    _check_case((64, 3, 64, 2, 2, 2, True, "average"))
    assert len(seen) == 2                                     # the coarse and the fine MLP's HIP runs
    for fused, ns, shape, lshape in seen:
        assert fused.last_latent_grad == "hip" and ns == 2 and shape == lshape == (4, 64, 8, 8)


def test_field_backward_under_deterministic_algorithms():
    """The fused case's backward under torch.use_deterministic_algorithms(True): torch's grid_sampler_2d_backward
    (float atomics) alerts there; with the maps' gradient on HIP no such op is left in the field's backward."""
    net = _net(128, 3, 64, (8, 8), sb=2)
    xyz, vd, w = _points(2, 700, seed=3)
    net.hip_backward = True
    net.zero_grad(set_to_none=True)
    lat = net.encoder.latent.detach().clone().requires_grad_(True)
    net.encoder.latent = lat
    out = net(xyz, coarse=False, viewdirs=vd)
    loss = (out * w).sum()
    torch.use_deterministic_algorithms(True)
    try:
        loss.backward()
    finally:
        torch.use_deterministic_algorithms(False)
    assert net.fused().last_latent_grad == "hip"
    assert lat.grad is not None and float(lat.grad.abs().max()) > 0


def test_points_and_latent_gradients_together():
    """The points and the maps both want a gradient (the adaptive renderer's band with a trainable encoder): one
    scene, d_hidden 128; both on HIP (no autograd re-forward), both within the yardstick."""
    from avr import train_common
    from test_gpu_layer_train import _grads as _grads_xyz
    net = _net(128, 3, 64, (8, 8))
    xyz, vd, w = _points(1, 700, seed=13)
    calls = []
    orig = train_common.input_grads_via_autograd
    train_common.input_grads_via_autograd = lambda *a: calls.append(1) or orig(*a)
    try:
        _, g_h = _grads_xyz(net, xyz, vd, w, True, hip=True, latent_grad=True)
    finally:
        train_common.input_grads_via_autograd = orig
    assert net.fused().last_latent_grad == "hip" and not calls
    _, g_t = _grads_xyz(net, xyz, vd, w, True, hip=False, latent_grad=True)
    _, g_d = _fp64(net, lambda: _grads_xyz(net, xyz.double(), vd.double(), w.double(), True, hip=False,
                                           latent_grad=True))
    assert {"xyz", "latent"} <= set(g_h)
    _compare64(g_h, g_t, g_d)


def test_latent_grad_flows_through_a_real_encoder(monkeypatch):
    """SpatialEncoder (num_layers = 1: C = 64, random init) encodes a (1, 1, 3, 16, 16) image; one VolumeRenderer
    training step with explicit noise. conv1's weight gradient with the maps' gradient from HIP (a channels-last
    strided tensor handed to cat / interpolate / conv backward) against the AVR_LATENT_GRAD_VIA_AUTOGRAD=1 step:
    the two differ in the maps' gradient's summation order alone, so the yardstick's floor (3e-5 of max |grad|)
    bounds the difference."""
    from avr.renderers import VolumeRenderer
    from avr.scene import INTRINSICS
    net = _net(128, 3, 64, (8, 8))
    R = 200
    g = torch.Generator(device="cpu").manual_seed(5)
    image = torch.rand(1, 1, 3, 16, 16, generator=g).to(DEV)
    src = torch.eye(4).reshape(1, 1, 4, 4).clone()
    src[..., 2, 3] = -1.3
    x_pix = torch.rand(1, R, 2, generator=g).to(DEV)
    c2w = torch.eye(4).reshape(1, 1, 4, 4).expand(1, R, 4, 4).clone()
    c2w[..., 2, 3] = -1.3
    c2w = c2w.to(DEV)
    K = torch.tensor([INTRINSICS], device=DEV)
    gt = torch.rand(1, R, 3, generator=g).to(DEV)
    rend = VolumeRenderer(0.8, 1.8, 32, 16, 4, 0.01, True)
    noise = {"coarse": torch.rand(1, R, 32, generator=g).to(DEV), "u": torch.rand(1, R, 12, generator=g).to(DEV),
             "u2": torch.rand(1, R, 12, generator=g).to(DEV), "depth": torch.randn(1, R, 4, generator=g).to(DEV)}
    conv1 = net.encoder.model.conv1.weight
    res = {}
    for mode in ("hip", "autograd"):
        if mode == "autograd":
            monkeypatch.setenv("AVR_LATENT_GRAD_VIA_AUTOGRAD", "1")
        net.zero_grad(set_to_none=True)
        net.encode(image, src.to(DEV), 16.4)
        assert net.encoder.latent.shape == (1, 64, 8, 8) and net.encoder.latent.requires_grad
        rgb_c, rgb_f, _, _ = rend(c2w, K, x_pix, net, noise=noise)
        (((rgb_c - gt) ** 2).mean() + ((rgb_f - gt) ** 2).mean()).backward()
        assert net.fused().last_latent_grad == mode
        res[mode] = conv1.grad.detach().clone()
    assert float(res["autograd"].abs().max()) > 0
    worst = _compare64({"conv1": res["hip"]}, {"conv1": res["autograd"]}, {"conv1": res["autograd"]})
    print(f"conv1.weight.grad: HIP vs autograd path {worst:.2e} of max |grad|")


def test_captured_adaptive_step_latent_grad_matches_eager():
    """tests/test_gpu_graphs.py's GraphedTrainStep of the adaptive step with the latent maps a leaf that requires
    grad (band points and maps both on HIP): each replay's latent.grad is bit-equal to the eager step's."""
    from test_gpu_poison import _setup
    from avr.graphs import GraphedTrainStep
    runs = []
    for graphed in (False, True):
        net, rend, named, (c2w, K, x_pix, gt), _ = _setup("adaptive", False)
        lat = net.encoder.latent.detach().clone().requires_grad_(True)
        net.encoder.latent = lat
        opt = torch.optim.Adam([p for _, p in named], lr=1e-4, capturable=True, fused=True)

        def step():
            rgb_c, rgb_f, _, _ = rend(c2w, K, x_pix, net)
            loss = ((rgb_c - gt) ** 2).mean() + ((rgb_f - gt) ** 2).mean()
            opt.zero_grad()
            lat.grad = None
            loss.backward()
            opt.step()
            return loss, lat.grad
        run = GraphedTrainStep(step, nets=[net], renderers=[rend], warmup=2) if graphed else step
        torch.manual_seed(123)
        grads = []
        for _ in range(4):
            loss, d_lat = run()
            grads.append((float(loss.detach()), d_lat.detach().clone()))
        assert rend.last_path == "hip_train" and net.fused().last_latent_grad == "hip"
        if graphed:
            assert run.captures == 1 and run.calls == 4
        runs.append(grads)
    for (le, ge), (lg, gg) in zip(*runs):
        assert le == lg and float(ge.abs().max()) > 0
        assert torch.equal(ge, gg)
