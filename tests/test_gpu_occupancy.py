"""Occupancy-grid empty-space skipping (avr.occupancy, csrc/occupancy.hip; not in the reference) on the device:
the four kernels against the numpy restatement of the contract (tests/occupancy_ref.py) bit for bit, gated_field
against forward_rays on the same samples, and VolumeRenderer with a grid against a chain built from the existing ops
with the reference's mask.

Shapes: R = 200 rays (not a multiple of 64, several workgroups of 4 rays), N in {40, 128, 192}
(a partial mask word, two words, three words), grids 32 x 32 x 32 and 64 x 32 x 16 over a box the camera's samples
partly leave. Field bar: atol 5e-5, rtol 1e-4 (tests/test_gpu_philox.py); the fp32 field kernel has no per-workgroup
run-time scale, so its rows do not depend on which samples share a workgroup: fp32 is held to bit equality."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occupancy_ref as ref  # noqa: E402
from helpers import build_net, to_np  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
LO, HI = (-0.45, -0.4, -0.35), (0.4, 0.45, 0.3)
CENTRE, RADIUS = (0.02, -0.03, 0.05), 0.3
GRIDS = {"cube": (32, 32, 32), "slab": (64, 32, 16)}
R_SMALL, SEED = 200, 99
_NETS = {}


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _net(golden, precision, scale=1.0):
    key = (precision, scale)
    if key not in _NETS:
        net = build_net(golden("g4_field_full.npz"), DEV, precision)
        if scale != 1.0:
            net.encoder.latent = net.encoder.latent * scale
        _NETS[key] = net
    return _NETS[key]


def _camera(R, seed=7, angle=0.7):
    from oracle import synth
    gen = torch.Generator(device="cpu").manual_seed(seed)
    x_pix = torch.rand(1, R, 2, generator=gen).to(DEV)
    c2w = T(synth.orbit_cam2world(angle)).reshape(1, 1, 4, 4).expand(1, R, 4, 4)
    K = T(synth.default_intrinsics())[None]
    return x_pix, c2w, K


def _rays(R, N, seed=SEED):
    from avr import ops
    x_pix, c2w, K = _camera(R)
    ro, rd, z, _, _ = ops.rays_sample_coarse(x_pix, K, c2w, 0.8, 1.8, N, seed=seed, offset=0)
    return ro[0].contiguous(), rd[0].contiguous(), z


def _occ(kind, res):
    rx, ry, rz = res
    if kind == "sphere":
        return ref.sphere_occ(res, LO, HI, CENTRE, RADIUS)
    return np.full((rz, ry, rx), kind == "all")


def _grid(occ, res):
    from avr.occupancy import OccupancyGrid
    return OccupancyGrid(LO, HI, res, T(ref.pack_bits(occ).view(np.int32)))


def _bits(grid):
    return grid.bits.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------ 1. build
@pytest.mark.parametrize("shape", sorted(GRIDS))
def test_build_matches_reference_bit_for_bit(shape):
    from avr.occupancy import OccupancyGrid
    res = GRIDS[shape]
    rng = np.random.default_rng(11)
    for K in (1, 3):
        sigma = (rng.standard_normal((K, res[2], res[1], res[0])) - 1.8).astype(np.float32)   # ~4 % above zero
        sigma[rng.random(sigma.shape) < 2e-3] = np.nan
        sigma[0, 0, 0, 0], sigma[-1, -1, -1, -1] = 1.0, np.nan                                 # the two far corners
        for thr in (0.0, 0.4):
            for dilate in (0, 1, 2):
                g = OccupancyGrid.from_sigma(T(sigma), LO, HI, thr, dilate)
                want = ref.build(sigma, thr, dilate)
                assert g.res == res and np.array_equal(_bits(g), ref.pack_bits(want)), (K, thr, dilate)
                assert g.live_fraction() == want.mean() and 0 < want.mean() < 1
    one = OccupancyGrid.from_sigma(T(sigma[0]), LO, HI, 0.0, 1)                                 # a (rz, ry, rx) plane
    assert np.array_equal(_bits(one), ref.pack_bits(ref.build(sigma[:1], 0.0, 1)))
    full = OccupancyGrid.all_occupied(LO, HI, res, DEV)
    assert np.array_equal(ref.unpack_bits(_bits(full), res), _occ("all", res)) and full.live_fraction() == 1.0


# ------------------------------------------------------------------ 2. classify / compact / expand
@pytest.mark.parametrize("kind,shape", [("sphere", "cube"), ("sphere", "slab"), ("all", "slab"), ("none", "cube")])
@pytest.mark.parametrize("N", [40, 128, 192])
def test_classify_compact_expand_match_reference(kind, shape, N):
    from avr import occupancy, ops
    res = GRIDS[shape]
    occ = _occ(kind, res)
    grid = _grid(occ, res)
    ro, rd, z = _rays(R_SMALL, N)
    z = z.clone()
    z[3, 5], z[17, N - 1], z[42, 0] = float("nan"), float("inf"), -float("inf")     # non-finite points are live
    z[5, 7] = 3e38                                                                   # finite, far outside: dead
    live, mask_r, counts_r = ref.classify(occ, LO, HI, to_np(ro), to_np(rd), to_np(z))
    assert live[3, 5] and live[17, N - 1] and live[42, 0] and not live[5, 7]
    assert not live[:, :].all() or kind == "all"     # the box does not hold every sample
    runs = []
    for _ in range(2):
        mask, counts = occupancy.classify(grid, ro, rd, z)
        incl = torch.cumsum(counts, 0, dtype=torch.int64)
        offsets = incl - counts
        M = int(incl[-1])
        xyz, vd = occupancy.compact(ro, rd, z, mask, offsets, M)
        gen = torch.Generator(device="cpu").manual_seed(5)
        fc = (torch.rand(M, 4, generator=gen) + 0.5).to(DEV)
        out = occupancy.expand(fc if M else None, mask, offsets, R_SMALL, N, M)
        torch.cuda.synchronize()
        runs.append([t.cpu().numpy() for t in (mask, counts, xyz, vd, out)] + [fc.cpu().numpy()])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))                    # two runs are bit-equal
    mask, counts, xyz, vd, out, fc = runs[0]
    assert np.array_equal(mask.view(np.uint64), mask_r) and np.array_equal(counts, counts_r)
    assert M == int(live.sum()) and (kind != "sphere" or 0 < M < live.size)
    xyz_r, vd_r = ref.compact(live, to_np(ro), to_np(rd), to_np(z))
    assert np.array_equal(xyz.view(np.uint32), xyz_r.view(np.uint32))                # NaN rows included
    assert np.array_equal(vd, vd_r)
    assert np.array_equal(out.view(np.uint32), ref.expand(live, fc).view(np.uint32))
    pts, _ = ops.points(ro, rd, z)
    assert np.array_equal(xyz.view(np.uint32), to_np(pts)[live.reshape(-1)].view(np.uint32))


# ------------------------------------------------------------------ 3. gated_field
@pytest.mark.parametrize("precision", ["fp32", "x3"])
@pytest.mark.parametrize("N,shape,coarse", [(40, "slab", True), (192, "cube", False)])
def test_gated_field_matches_forward_rays(golden, precision, N, shape, coarse):
    from avr.occupancy import gated_field
    net = _net(golden, precision)
    fused = net.fused()
    res = GRIDS[shape]
    occ = _occ("sphere", res)
    ro, rd, z = _rays(R_SMALL, N)
    with torch.no_grad():
        got, n_live = gated_field(fused, _grid(occ, res), ro, rd, z, coarse)
        full = fused.forward_rays(ro, rd, z, coarse)
    torch.cuda.synchronize()
    live = ref.classify(occ, LO, HI, to_np(ro), to_np(rd), to_np(z))[0].reshape(-1)
    got, full = to_np(got), to_np(full)
    assert got.shape == (R_SMALL * N, 4) and n_live == int(live.sum()) and 0 < n_live < live.size
    assert not got[~live].any() and not np.signbit(got[~live]).any()                 # dead rows: exactly +0.0
    err = float(np.abs(got[live] - full[live]).max())
    print(f"gated_field {precision} N={N}: live {n_live}/{live.size}, max |gated - forward_rays| on live rows {err:.3e}")
    if precision == "fp32":
        assert np.array_equal(got[live], full[live])                                 # no run-time scale: bit-equal
    np.testing.assert_allclose(got[live], full[live], atol=5e-5, rtol=1e-4)


def test_gated_field_empty_grid_launches_no_field(golden, monkeypatch):
    from avr import ops
    from avr.occupancy import gated_field
    net = _net(golden, "x3")
    fused = net.fused()
    res = GRIDS["cube"]
    N, NF = 128, 64
    ro, rd, z = _rays(R_SMALL, N)
    calls = []
    monkeypatch.setattr(fused, "forward_points_scene", lambda *a, **k: calls.append(a) or 1 / 0)
    with torch.no_grad():
        got, n_live = gated_field(fused, _grid(_occ("none", res), res), ro, rd, z, True)
        zeros = torch.zeros(R_SMALL, N, 4, device=DEV)
        a, b = ops.composite(z, got.reshape(R_SMALL, N, 4)), ops.composite(z, zeros)
        zs, _, _ = ops.sample_fine(a[2], z, 0.8, 1.8, NF, 0, 0.01, seed=SEED, offset=0)
    torch.cuda.synchronize()
    assert n_live == 0 and not calls and not to_np(got).any()
    for x, y in zip(a, b):
        assert np.array_equal(to_np(x), to_np(y))
    zs = to_np(zs)
    assert zs.shape == (R_SMALL, N + NF) and np.isfinite(zs).all() and (np.diff(zs, axis=-1) >= 0).all()


# ------------------------------------------------------------------ 4. / 5. end to end
def _masked_chain(net, x_pix, c2w, K, occ, NC=128, NF=64):
    """The renderer's chain from the existing ops under seed SEED, offset 0, with the rows the reference calls dead
    zeroed after a full forward_rays: rgb_c, rgb_f, depth, live counts (coarse, fine)."""
    from avr import ops
    R = x_pix.shape[1]
    fused = net.fused()

    def masked(z, coarse):
        f = fused.forward_rays(ro[0], rd[0], z, coarse)
        if occ is None:
            return f.reshape(R, -1, 4), z.numel()
        live = ref.classify(occ, LO, HI, to_np(ro[0]), to_np(rd[0]), to_np(z))[0]
        return (f * T(live.reshape(-1, 1).astype(np.float32))).reshape(R, -1, 4), int(live.sum())

    with torch.no_grad():
        ro, rd, zc, drow, _ = ops.rays_sample_coarse(x_pix, K, c2w, 0.8, 1.8, NC, seed=SEED, offset=0,
                                                     want_depth_row=True)
        fc, n_c = masked(zc, True)
        rgb_c, _, w_c = ops.composite(zc, fc)
        zs, _, _ = ops.sample_fine(w_c, zc, 0.8, 1.8, NF, 0, 0.01, seed=SEED, offset=0)
        ff, n_f = masked(zs, False)
        rgb_f, _, _, depth = ops.composite_depth(zs, ff, ro, rd, drow)
    torch.cuda.synchronize()
    return to_np(rgb_c), to_np(rgb_f), to_np(depth), (n_c, n_f)


def _render(net, x_pix, c2w, K, occupancy, offset=0):
    from avr.renderers import VolumeRenderer
    rend = VolumeRenderer(0.8, 1.8, 128, 64, 0, 0.01, True)
    rend.seed, rend._offset, rend.occupancy = SEED, offset, occupancy
    with torch.no_grad():
        rgb_c, rgb_f, depth, _ = rend(c2w, K, x_pix, net)
    torch.cuda.synchronize()
    assert rend.last_path == "fused"
    return to_np(rgb_c[0]), to_np(rgb_f[0]), to_np(depth[0]), rend


def _compare(precision, got, want, what):
    (g_c, g_f, g_d), (w_c, w_f, w_d) = got, want
    e_c = float(np.abs(g_c - w_c).max())
    ok = (np.abs(g_f - w_f).max(-1) <= 1e-4) & (np.abs(g_d - w_d) <= 1e-4)
    print(f"{what} {precision}: coarse max err {e_c:.2e}, fine rgb / depth within 1e-4 on {ok.mean():.5f} of rays")
    assert e_c <= 1e-4
    if precision == "fp32":
        assert ok.all(), ok.mean()        # the fp32 field is bit-equal under gating: every ray
    assert ok.mean() >= 0.997, ok.mean()  # x3: the project's share for inverse-CDF bin flips under weight noise


@pytest.mark.parametrize("precision", ["fp32", "x3"])
def test_renderer_with_sphere_grid_matches_masked_chain(golden, precision):
    net = _net(golden, precision)
    R, res = 4096, GRIDS["cube"]
    x_pix, c2w, K = _camera(R)
    occ = _occ("sphere", res)
    w_c, w_f, w_d, (n_c, n_f) = _masked_chain(net, x_pix, c2w, K, occ)
    g_c, g_f, g_d, rend = _render(net, x_pix, c2w, K, _grid(occ, res))
    _compare(precision, (g_c, g_f, g_d), (w_c, w_f, w_d), "sphere grid vs masked chain")
    print(f"live samples {rend.last_live_by_pass} of {(R * 128, R * 192)}")
    assert rend.last_live_samples == sum(rend.last_live_by_pass) < R * 192
    assert rend.last_live_by_pass[0] == n_c and 0 < n_c < R * 128
    assert rend.last_fine_samples == R * 192
    if precision == "fp32":
        assert rend.last_live_by_pass[1] == n_f


@pytest.mark.parametrize("precision", ["fp32", "x3"])
def test_all_occupied_grid_and_default(golden, precision):
    from avr.occupancy import OccupancyGrid
    net = _net(golden, precision)
    R, res = 4096, GRIDS["slab"]
    x_pix, c2w, K = _camera(R)
    u_c, u_f, u_d, fresh = _render(net, x_pix, c2w, K, None)
    assert fresh.last_live_samples == 0
    # a box that holds every sample, all cells set: the gated render is the ungated one up to field grouping
    big = OccupancyGrid.all_occupied((-2, -2, -2), (2, 2, 2), res, DEV)
    g_c, g_f, g_d, rend = _render(net, x_pix, c2w, K, big)
    assert rend.last_live_by_pass == (R * 128, R * 192)
    _compare(precision, (g_c, g_f, g_d), (u_c, u_f, u_d), "all-occupied grid vs ungated")
    # occupancy = None again: bit-equal to a renderer that never had a grid
    rend.occupancy, rend._offset = None, 0
    with torch.no_grad():
        n_c, n_f, n_d, _ = rend(c2w, K, x_pix, net)
    torch.cuda.synchronize()
    for a, b in ((n_c[0], u_c), (n_f[0], u_f), (n_d[0], u_d)):
        assert np.array_equal(to_np(a), b)


# ------------------------------------------------------------------ 6. from_field
def test_from_field_bits_and_staleness(golden):
    from avr.cache import bump_param_generation
    from avr.occupancy import AXIS_DIRS, OccupancyGrid
    net = build_net(golden("g4_field_full.npz"), DEV, "x3")      # its own net: a parameter is changed below
    res, chunk = (32, 32, 32), 8192                               # four chunks per plane
    grid = OccupancyGrid.from_field(net, LO, HI, res, sigma_thr=0.0, dilate=1, chunk=chunk)
    assert grid.key is not None and not grid.stale(net)
    # the test's own evaluation: float64 centres rounded once, both MLPs, the six axis directions, same chunks
    ax = [np.float64(np.float32(l)) + (np.arange(r) + 0.5) * ((np.float64(np.float32(h)) - np.float64(np.float32(l))) / r)
          for l, h, r in zip(LO, HI, res)]
    zz, yy, xx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    centres = T(np.stack([xx, yy, zz], -1).reshape(-1, 3).astype(np.float32))
    fused = net.fused()
    planes = []
    with torch.no_grad():
        for coarse in (True, False):
            for d in AXIS_DIRS:
                vd = torch.tensor([d], device=DEV)
                parts = [fused.forward_points(centres[c0:c0 + chunk][None],
                                              vd.expand(min(chunk, len(centres) - c0), 3)[None], coarse)[0, :, 3]
                         for c0 in range(0, len(centres), chunk)]
                planes.append(torch.cat(parts))
    planes = torch.stack(planes).reshape(12, res[2], res[1], res[0])
    own = OccupancyGrid.from_sigma(planes, LO, HI, 0.0, 1)
    assert np.array_equal(_bits(grid), _bits(own))
    sig = to_np(planes)
    occ = ref.unpack_bits(_bits(grid), res)
    assert np.array_equal(occ, ref.build(sig, 0.0, 1))
    assert (sig.max(0)[~occ] == 0).all()      # whatever the grid drops had sigma == 0 for every MLP and direction
    print(f"from_field on the fixture: live fraction {grid.live_fraction():.4f}")
    x_pix, c2w, K = _camera(R_SMALL)
    g = _render(net, x_pix, c2w, K, grid)
    assert g[3].last_live_samples <= R_SMALL * 320
    with torch.no_grad():
        net.mlp_fine.lin_out.bias[3] += 0.25                     # changed in place ...
    bump_param_generation()                                      # ... and announced
    assert grid.stale(net)
    with pytest.raises(ValueError, match="have changed"):
        _render(net, x_pix, c2w, K, grid)


# ------------------------------------------------------------------ 7. two scenes, two grids
def test_two_scenes_two_grids_equal_single_scene_renders(golden):
    res = GRIDS["cube"]
    R = 512
    one, other = _net(golden, "x3"), _net(golden, "x3", scale=0.9)
    both = build_net(golden("g4_field_full.npz"), DEV, "x3")
    both.encoder.latent = torch.cat([one.encoder.latent, other.encoder.latent], 0)
    both.poses = torch.cat([one.poses, one.poses], 0)
    grids = [_grid(_occ("sphere", res), res), _grid(ref.sphere_occ(res, LO, HI, (-0.1, 0.05, 0.0), 0.2), res)]
    cams = [_camera(R, seed=7, angle=0.7), _camera(R, seed=8, angle=2.1)]
    x_pix = torch.cat([c[0] for c in cams], 0)
    c2w = torch.cat([c[1] for c in cams], 0)
    K = torch.cat([c[2] for c in cams], 0)
    from avr.renderers import VolumeRenderer
    rend = VolumeRenderer(0.8, 1.8, 128, 64, 0, 0.01, True)
    rend.seed, rend.occupancy = SEED, grids
    with torch.no_grad():
        rgb_c, rgb_f, depth, _ = rend(c2w, K, x_pix, both)
    torch.cuda.synchronize()
    total = 0
    for b, net in enumerate((one, other)):
        s_c, s_f, s_d, single = _render(net, *cams[b], grids[b], offset=b * R)   # scene b's rays are ids b*R ...
        assert np.array_equal(to_np(rgb_c[b]), s_c) and np.array_equal(to_np(rgb_f[b]), s_f)
        assert np.array_equal(to_np(depth[b]), s_d)
        total += single.last_live_samples
    assert rend.last_live_samples == total
