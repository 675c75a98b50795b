"""Per-ray sampling bounds from the occupancy grid on the GPU (avr_occ_ray_bounds, avr_sample_coarse_bounds,
avr_sample_fine_bounds, VolumeRenderer.ray_bounds = "grid"; include/avr.h "occupancy grid: per-ray bounds").
References: tests/ray_bounds_ref.py (float64 brute force) for the kernel, the library's own avr_occ_classify for
safety, the scalar sampling entries under uniform bounds, the oracle's sample_coarse / sample_fine / sort and its
render chain under the kernel's bounds, and today's gated frame under an all-occupied grid.

Shapes. Kernel: the ray sets of ray_bounds_ref.cases() (1, 65 and 256 rays: one lane, a second wave with one lane, one
full workgroup) over 32^3 grids; the CPU test holds their in-between share to 10 %. Sampling: 67 rays (the fine
kernel's 4-ray workgroups end with three), n_coarse 32 and 33 (a power of two and not, a ragged last quad), n_fine 16,
n_fine_depth 0 and 4 (the two-list and the three-list merge). Renderer: 16 x 16 rays, 32 + 16 samples, a d_hidden 64
net."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_fp16_ref as ref16  # noqa: E402
import occupancy_ref as ref  # noqa: E402
import ray_bounds_ref as rb  # noqa: E402
from helpers import model_conf, oracle_field_from_net, to_np  # noqa: E402
from oracle import avr_oracle as O  # noqa: E402
from oracle import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
F = np.float32
CASES = ("sphere_fan_1", "sphere_fan_65", "sphere_fan_256", "empty", "full", "corner_cell", "axis_parallel",
         "inside_box", "far_cut", "non_finite")
NC, NF, SIDE = 32, 16, 16
NEAR, FAR = 0.8, 1.8
SEED = 99
_SCENE = {}


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def bits(t):
    return to_np(t).view(np.uint32)


def _grid(occ, lo=rb.LO, hi=rb.HI):
    from avr.occupancy import OccupancyGrid
    return OccupancyGrid(lo, hi, occ.shape[::-1], T(ref.pack_bits(occ).view(np.int32)))


# ------------------------------------------------------------------ 1. the kernel's contract
def _library_live(grid, ro, rd, z):
    """avr_occ_classify's live bits for z (R, N), N a multiple of 256 or below it, 256 depths per call."""
    from avr import occupancy
    R, N = z.shape
    live = np.zeros((R, N), bool)
    for c0 in range(0, N, 256):
        zc = T(z[:, c0:c0 + 256])
        mask, _ = occupancy.classify(grid, ro, rd, zc)
        m = mask.cpu().numpy().view(np.uint64)
        b = ((m[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(R, -1)
        live[:, c0:c0 + zc.shape[1]] = b[:, :zc.shape[1]]
    return live


def test_cases_are_the_reference_cases():
    assert CASES == tuple(rb.cases())


@pytest.mark.parametrize("name", CASES)
def test_kernel_contract(name):
    c = rb.cases()[name]
    grid = _grid(c["occ"])
    ro, rd = T(c["ro"]), T(c["rd"])
    n = ro.shape[0]
    outs = []
    for _ in range(2):
        buf = torch.full((2, n + 2), -7.0, device=DEV)                 # a guard element on either side
        tn, tf = grid.ray_bounds(ro, rd, c["near"], c["far"], out=(buf[0, 1:n + 1], buf[1, 1:n + 1]))
        torch.cuda.synchronize()
        assert (to_np(buf[:, 0]) == -7).all() and (to_np(buf[:, -1]) == -7).all()
        outs.append((to_np(tn), to_np(tf)))
    (tn, tf), again = outs
    assert np.array_equal(tn.view(np.uint32), again[0].view(np.uint32))
    assert np.array_equal(tf.view(np.uint32), again[1].view(np.uint32))   # two launches, the same bits
    clear_hit, clear_miss = rb.check(c, tn, tf)                        # range, (T), (M), the non-finite rule
    # (S) by the library's own live test: 16 x 256 depths over [near, far] and the floats next to each bound
    z = rb.dense_z(c["near"], c["far"], n, 16 * 256)
    edge = np.stack([np.nextafter(tn, F(-np.inf)), tn, tf, np.nextafter(tf, F(np.inf))], -1)
    edge = np.clip(edge, F(c["near"]), F(c["far"])).astype(F)
    z = np.concatenate([z, edge], -1)
    finite = np.isfinite(c["ro"]).all(-1) & np.isfinite(c["rd"]).all(-1)
    live = _library_live(grid, ro, rd, z)
    assert live[~finite].all()                                         # a non-finite ray: every depth is live
    outside = rb.live_outside(live, z, tn, tf)
    bounded = int(((tn > F(c["near"])) | (tf < F(c["far"]))).sum())
    print(f"{name}: {n} rays, clear hits {int(clear_hit.sum())}, clear misses {int(clear_miss.sum())}, bounded "
          f"{bounded}, live depths {int(live[finite].sum())}, outside the bounds {outside}")
    assert outside == 0
    assert live[clear_hit].any(1).all() and not live[clear_miss].any()
    if name == "full":
        assert bounded == 0                                            # the box holds every segment: (near, far)
    if name.startswith("sphere_fan") or name == "far_cut":
        assert (tn[clear_hit] > F(c["near"])).all()                    # the sphere starts behind near


def test_ray_bounds_shapes_and_empty():
    from avr.occupancy import OccupancyGrid
    grid = OccupancyGrid.all_occupied(rb.LO, rb.HI, rb.RES, DEV)
    ro, rd = rb.fan()
    tn, tf = grid.ray_bounds(T(ro).reshape(2, 128, 3), T(rd).reshape(2, 128, 3), NEAR, FAR)
    assert tn.shape == tf.shape == (2, 128) and tn.dtype == torch.float32
    tn, tf = grid.ray_bounds(torch.empty(0, 3, device=DEV), torch.empty(0, 3, device=DEV), NEAR, FAR)
    assert tn.shape == (0,)
    with pytest.raises(Exception, match="near"):
        grid.ray_bounds(T(ro), T(rd), FAR, NEAR)


# ------------------------------------------------------------------ 2. sampling
R_S = 67


def _draws(nc, nd, seed=5):
    rng = np.random.default_rng(seed)
    return {"coarse": rng.random((R_S, nc), dtype=F), "u": rng.random((R_S, NF), dtype=F),
            "u2": rng.random((R_S, NF), dtype=F), "depth": rng.standard_normal((R_S, nd)).astype(F),
            "w": (rng.random((R_S, nc), dtype=F) ** 4).astype(F)}


def _kernel_bounds():
    """65 + 2 rays with non-uniform bounds from the kernel (the sphere fan: hits with their own spans, misses with
    (near, far))."""
    c = rb.cases()["sphere_fan_65"]
    ro = np.concatenate([c["ro"], c["ro"][:2]])
    rd = np.concatenate([c["rd"], c["rd"][:2]])
    tn, tf = _grid(c["occ"]).ray_bounds(T(ro), T(rd), NEAR, FAR)
    assert len(np.unique(to_np(tn))) > 8
    return tn, tf


@pytest.mark.parametrize("nc", [32, 33])
@pytest.mark.parametrize("nd", [0, 4])
def test_uniform_bounds_equal_the_scalar_entries(nc, nd):
    from avr import ops
    d = _draws(nc, nd)
    near_r = torch.full((R_S,), NEAR, device=DEV)
    far_r = torch.full((R_S,), FAR, device=DEV)
    ids = T(np.random.default_rng(3).permutation(1000)[:R_S].astype(np.int64))
    for noise, kw in ((T(d["coarse"]), {}), (None, {"seed": SEED, "offset": 11}),
                      (None, {"seed": SEED, "offset": 11, "ray_ids": ids})):
        a = ops.sample_coarse(NEAR, FAR, R_S, nc, DEV, noise=noise, **kw)
        b = ops.sample_coarse_bounds(near_r, far_r, nc, noise=noise, **kw)
        assert np.array_equal(bits(a), bits(b)), kw
    zc = ops.sample_coarse(NEAR, FAR, R_S, nc, DEV, noise=T(d["coarse"]))
    w = T(d["w"])
    for kw in ({"u": T(d["u"]), "u2": T(d["u2"]), "noise_depth": T(d["depth"])}, {"seed": SEED, "offset": 11},
               {"seed": SEED, "offset": 11, "ray_ids": ids}):
        a = ops.sample_fine(w, zc, NEAR, FAR, NF, nd, 0.9, want_idx=True, want_fine=True, **kw)
        b = ops.sample_fine(w, zc, near_r, far_r, NF, nd, 0.9, want_idx=True, want_fine=True, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(bits(a[0]), bits(b[0])), kw
        assert np.array_equal(a[1].cpu().numpy(), b[1].cpu().numpy()), kw
        assert np.array_equal(bits(a[2]), bits(b[2])), kw


@pytest.mark.parametrize("nc", [32, 33])
@pytest.mark.parametrize("nd", [0, 4])
def test_kernel_bounds_against_the_oracle(nc, nd):
    """Non-uniform bounds from avr_occ_ray_bounds, explicit draws: the coarse z is the oracle's bit for bit, and so
    are the fine bins, the fine z and the sorted list given the weights the HIP call was given. depth_std 0.9 puts
    depth samples inside, below and above a ray's span, so that the per-ray clamp (quirk Q6) shows."""
    from avr import ops
    d = _draws(nc, nd)
    tn, tf = _kernel_bounds()
    tn_np, tf_np = to_np(tn), to_np(tf)
    zc = ops.sample_coarse_bounds(tn, tf, nc, noise=T(d["coarse"]))
    want_zc = O.sample_coarse(tn_np[None], tf_np[None], nc, d["coarse"][None])[0]
    assert np.array_equal(bits(zc), want_zc.view(np.uint32))
    zs, idx, zf = ops.sample_fine(T(d["w"]), zc, tn, tf, NF, nd, 0.9, u=T(d["u"]), u2=T(d["u2"]),
                                  noise_depth=T(d["depth"]), want_idx=True, want_fine=True)
    torch.cuda.synchronize()
    want_zf, want_idx = O.sample_fine(tn_np[None], tf_np[None], NF, d["w"][None, :, :, None], d["u"][None],
                                      d["u2"][None], return_idx=True)
    assert np.array_equal(idx.cpu().numpy(), want_idx[0])
    assert np.array_equal(bits(zf), want_zf[0].view(np.uint32))
    zd = np.minimum(np.maximum((d["depth"] * F(0.9)).astype(F), tn_np[:, None]), tf_np[:, None])
    if nd:
        assert (zd == tn_np[:, None]).any() and (zd == tf_np[:, None]).any()
    want_zs = np.sort(np.concatenate([want_zc, want_zf[0], zd], -1), -1)
    assert np.array_equal(bits(zs), want_zs.view(np.uint32))
    # the in-kernel draws under non-uniform bounds: a shard with ray_ids equals the whole call's rows
    pick = np.random.default_rng(4).permutation(R_S)[:23]
    ids = T(pick.astype(np.int64))
    whole = ops.sample_coarse_bounds(tn, tf, nc, seed=SEED, offset=5)
    part = ops.sample_coarse_bounds(tn[ids], tf[ids], nc, seed=SEED, offset=5, ray_ids=ids)
    assert np.array_equal(bits(whole)[pick], bits(part))
    w = T(d["w"])
    whole = ops.sample_fine(w, zc, tn, tf, NF, nd, 0.9, seed=SEED, offset=5, want_idx=True, want_fine=True)
    part = ops.sample_fine(w[ids], zc[ids], tn[ids], tf[ids], NF, nd, 0.9, seed=SEED, offset=5, ray_ids=ids,
                           want_idx=True, want_fine=True)
    for a, b in zip(whole, part):
        assert np.array_equal(a.cpu().numpy()[pick].view(np.uint32), b.cpu().numpy().view(np.uint32))


# ------------------------------------------------------------------ 3. the renderer
def _scene():
    """synthetic_scene(sigma_bias=30) at d_hidden 64 (three blocks, a 64-channel 16 x 16 latent) and a 16 x 16 ray
    frame with explicit draws, shared by the tests."""
    if not _SCENE:
        from avr.scene import synthetic_scene
        net = synthetic_scene(DEV, 0, model_conf(64, 3, 1000, 64), latent_hw=(16, 16), sigma_bias=30.0)
        R = SIDE * SIDE
        ij = (np.stack(np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="xy"), -1).reshape(1, R, 2) + 0.5) / SIDE
        rng = np.random.default_rng(7)
        noise = {"coarse": rng.random((1, R, NC), dtype=F), "u": rng.random((1, R, NF), dtype=F),
                 "u2": rng.random((1, R, NF), dtype=F), "depth": np.zeros((1, R, 0), F)}
        _SCENE.update(net=net, x_pix=ij.astype(F), c2w=synth.orbit_cam2world(0.4), K=synth.default_intrinsics()[None],
                      noise=noise, R=R, sphere=rb.sphere_grid())
    return _SCENE


def _renderer(seed=None, **attrs):
    from avr.renderers import VolumeRenderer
    rend = VolumeRenderer(NEAR, FAR, NC, NF, 0, 0.01, True)
    rend.seed, rend._offset = seed, 0
    for k, v in attrs.items():
        setattr(rend, k, v)
    return rend


def _frame(rend, precision="x3", explicit=False, rays=None, **kw):
    s = _scene()
    s["net"].field_precision = precision
    x_pix = T(s["x_pix"]) if rays is None else T(s["x_pix"][:, rays])
    c2w = T(s["c2w"]).reshape(1, 1, 4, 4).expand(1, x_pix.shape[1], 4, 4)
    noise = {k: T(v) for k, v in s["noise"].items()} if explicit else None
    with torch.no_grad():
        out = rend(c2w, T(s["K"]), x_pix, s["net"], noise=noise, **kw)
    torch.cuda.synchronize()
    assert rend.last_path == "fused"
    return out[:3]


def _sphere_grid():
    return _grid(_scene()["sphere"])


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("count", ["host", "device"])
def test_all_occupied_grid_equals_the_gated_frame_without_bounds(explicit, count):
    """A grid with every cell set whose box holds every ray's [near, far] segment: every ray's bounds are (near, far),
    and the bounded frame is the gated frame without bounds bit for bit."""
    from avr.occupancy import OccupancyGrid
    grid = OccupancyGrid.all_occupied((-4, -4, -4), (4, 4, 4), (32, 32, 32), DEV)
    seed = None if explicit else SEED
    want = _frame(_renderer(seed, occupancy=grid, occupancy_count=count), explicit=explicit)
    rend = _renderer(seed, occupancy=grid, occupancy_count=count, ray_bounds="grid")
    got = _frame(rend, explicit=explicit)
    tn, tf = rend.last_ray_bounds
    assert tn.shape == (1, _scene()["R"]) and (to_np(tn) == F(NEAR)).all() and (to_np(tf) == F(FAR)).all()
    for name, a, b in zip(("rgb_coarse", "rgb_fine", "depth"), got, want):
        assert np.array_equal(bits(a), bits(b)), name
    assert float(got[1].std()) > 0.01                                   # a picture, not a constant


def _oracle_chain(field, occ, tn, tf):
    """oracle.render's chain with per-ray bounds and gating: the field where occupancy_ref calls the sample live,
    exact zeros elsewhere. -> rgb_c, rgb_f, depth, aux."""
    s = _scene()
    n = s["noise"]
    c2w = np.broadcast_to(s["c2w"], (1, s["R"], 4, 4))
    ro, rd = O.get_world_rays(s["x_pix"], s["K"], c2w)

    def gated(z, coarse):
        pts = ro[..., None, :] + rd[..., None, :] * z[..., None]
        vd = np.broadcast_to(rd[..., None, :], pts.shape)
        f = np.asarray(field(pts.reshape(1, -1, 3), vd.reshape(1, -1, 3), coarse=coarse)).reshape(1, s["R"], -1, 4)
        live = ref.classify(occ, rb.LO, rb.HI, ro[0], rd[0], z[0])[0]
        return np.where(live[None, :, :, None], f, 0.0), live

    zc = O.sample_coarse(tn, tf, NC, n["coarse"])
    fc, live_c = gated(zc, True)
    rgb_c, dist_c, w_c = O.volume_integral(zc, fc[..., 3:4], fc[..., :3], True)
    zf, idx = O.sample_fine(tn, tf, NF, w_c, n["u"], n["u2"], return_idx=True)
    zs = np.sort(np.concatenate([zc, zf], -1), -1)
    ff, live_f = gated(zs, False)
    rgb_f, dist_f, _ = O.volume_integral(zs, ff[..., 3:4], ff[..., :3], True)
    depth = O.depth_from_world(ro + rd * dist_f, c2w)
    return rgb_c, rgb_f, depth, dict(zc=zc, idx=idx, zs=zs, live_c=live_c, live_f=live_f, ro=ro, rd=rd)


def _hip_stages(grid, tn, tf):
    """The bounded frame from the ops the renderer calls, explicit draws: -> rgb_c, rgb_f, depth and the stages."""
    from avr import ops
    from avr.occupancy import gated_field
    s = _scene()
    s["net"].field_precision = "x3"
    n = {k: T(v) for k, v in s["noise"].items()}
    R = s["R"]
    c2w = T(s["c2w"]).reshape(1, 1, 4, 4).expand(1, R, 4, 4)
    fused = s["net"].fused()
    with torch.no_grad():
        ro, rd, _, drow, _ = ops.rays_sample_coarse(T(s["x_pix"]), T(s["K"]), c2w, NEAR, FAR, NC, noise=n["coarse"],
                                                    want_depth_row=True)
        zc = ops.sample_coarse_bounds(tn, tf, NC, noise=n["coarse"])
        fc, _ = gated_field(fused, grid, ro[0], rd[0], zc, True)
        rgb_c, _, w_c = ops.composite(zc, fc.reshape(R, NC, 4))
        zs, idx, _ = ops.sample_fine(w_c, zc, tn, tf, NF, 0, 0.01, u=n["u"], u2=n["u2"], noise_depth=n["depth"],
                                     want_idx=True)
        ff, _ = gated_field(fused, grid, ro[0], rd[0], zs, False)
        rgb_f, _, _, depth = ops.composite_depth(zs, ff.reshape(R, NC + NF, 4), ro, rd, drow)
    torch.cuda.synchronize()
    return rgb_c, rgb_f, depth, dict(zc=zc, fc=fc.reshape(R, NC, 4), idx=idx, zs=zs, ff=ff.reshape(R, NC + NF, 4))


def test_sphere_grid_frame_against_the_oracle_chain():
    """The kernel's bounds fed to the oracle's chain on the same draws: the bins are equal, rgb and depth within 1e-4
    (the project's bar), dead samples contribute exact zeros, and the frame samples more densely than without
    bounds."""
    s = _scene()
    grid = _sphere_grid()
    rend = _renderer(occupancy=grid, ray_bounds="grid")
    got = _frame(rend, explicit=True)
    tn, tf = rend.last_ray_bounds
    live_bounded = rend.last_live_by_pass
    hc, hf, hd, st = _hip_stages(grid, tn.reshape(-1), tf.reshape(-1))
    for name, a, b in zip(("rgb_coarse", "rgb_fine", "depth"), got, (hc, hf, hd)):
        assert np.array_equal(bits(a).reshape(-1), bits(b).reshape(-1)), name     # the renderer is these stages
    o_c, o_f, o_d, aux = _oracle_chain(oracle_field_from_net(s["net"]), s["sphere"], to_np(tn), to_np(tf))
    assert np.array_equal(bits(st["zc"]), aux["zc"][0].view(np.uint32))
    assert np.array_equal(st["idx"].cpu().numpy(), aux["idx"][0])                 # bins
    assert np.array_equal(bits(st["zs"]), aux["zs"][0].view(np.uint32))
    assert not to_np(st["fc"])[~aux["live_c"]].any() and not to_np(st["ff"])[~aux["live_f"]].any()   # exact zeros
    e_c = float(np.abs(to_np(got[0]) - o_c).max())
    e_f = float(np.abs(to_np(got[1]) - o_f).max())
    e_d = float(np.abs(to_np(got[2]) - o_d).max())
    plain = _renderer(occupancy=grid)
    _frame(plain, explicit=True)
    bounded = int(((to_np(tn) > F(NEAR)) | (to_np(tf) < F(FAR))).sum())
    print(f"sphere grid: {bounded} of {s['R']} rays bounded; live samples (coarse, fine) {live_bounded} with bounds, "
          f"{plain.last_live_by_pass} without; max err vs the oracle chain: coarse {e_c:.2e}, fine {e_f:.2e}, depth "
          f"{e_d:.2e}")
    assert live_bounded == (int(aux["live_c"].sum()), int(aux["live_f"].sum()))
    assert e_c <= 1e-4 and e_f <= 1e-4 and e_d <= 1e-4
    assert 32 < bounded < s["R"]
    assert live_bounded[0] > plain.last_live_by_pass[0] and live_bounded[1] > plain.last_live_by_pass[1]


def test_two_shards_with_ray_ids_equal_the_frame():
    R = _scene()["R"]
    grid = _sphere_grid()
    whole = _frame(_renderer(SEED, occupancy=grid, ray_bounds="grid"))
    for rays in (np.arange(0, R // 2), np.arange(R // 2, R)):
        part = _frame(_renderer(SEED, occupancy=grid, ray_bounds="grid"), rays=rays, ray_ids=T(rays.astype(np.int64)),
                      n_rays_total=R)
        for a, b in zip(whole, part):
            assert np.array_equal(bits(a)[0][rays], bits(b)[0])


def test_two_scenes_two_grids_equal_two_single_scene_calls():
    from avr.scene import synthetic_scene
    s = _scene()
    R = s["R"]
    one = s["net"]
    one.field_precision = "x3"
    both = synthetic_scene(DEV, 0, model_conf(64, 3, 1000, 64), latent_hw=(16, 16), sigma_bias=30.0)
    other = synthetic_scene(DEV, 0, model_conf(64, 3, 1000, 64), latent_hw=(16, 16), sigma_bias=30.0)
    other.encoder.set_latent(one.encoder.latent * 0.9)
    both.encoder.set_latent(torch.cat([one.encoder.latent, other.encoder.latent], 0))
    both.poses = torch.cat([one.poses, one.poses], 0)
    grids = [_sphere_grid(), _grid(rb.sphere_grid(0.35))]
    cams = [synth.orbit_cam2world(0.4), synth.orbit_cam2world(2.1)]
    x_pix = T(np.concatenate([s["x_pix"], s["x_pix"][:, ::-1]], 0))
    c2w = torch.stack([T(c).reshape(1, 4, 4).expand(R, 4, 4) for c in cams])
    K = T(np.concatenate([s["K"], s["K"]], 0))
    rend = _renderer(SEED, occupancy=grids, ray_bounds="grid")
    with torch.no_grad():
        rgb_c, rgb_f, depth, _ = rend(c2w, K, x_pix, both)
        torch.cuda.synchronize()
        tn = to_np(rend.last_ray_bounds[0])
        assert not np.array_equal(tn[0], tn[1])
        for b, net in enumerate((one, other)):
            single = _renderer(SEED, occupancy=grids[b], ray_bounds="grid")
            single._offset = b * R                                      # scene b's rays are ids b * R ...
            s_c, s_f, s_d, _ = single(c2w[b:b + 1], K[b:b + 1], x_pix[b:b + 1], net)
            torch.cuda.synchronize()
            assert np.array_equal(bits(rgb_c[b]), bits(s_c[0])) and np.array_equal(bits(rgb_f[b]), bits(s_f[0]))
            assert np.array_equal(bits(depth[b]), bits(s_d[0]))
            assert np.array_equal(tn[b], to_np(single.last_ray_bounds[0])[0])


@pytest.mark.parametrize("t_stop", [None, 1e-3])
def test_graphed_renderer_replay_equals_the_eager_frame(t_stop):
    from avr.graphs import GraphedRenderer
    s = _scene()
    s["net"].field_precision = "x3"
    modes = dict(occupancy=_sphere_grid(), occupancy_count="device", ray_bounds="grid")
    if t_stop is not None:
        modes.update(t_stop=t_stop, t_stop_count="device")
    want = _frame(_renderer(SEED, **modes))
    c2w = T(s["c2w"]).reshape(1, 1, 4, 4).expand(1, s["R"], 4, 4)
    rend = _renderer(SEED, **modes)
    graphed = GraphedRenderer(rend, s["net"], c2w, T(s["K"]), T(s["x_pix"]))
    for _ in range(2):
        got = graphed()[:3]
        torch.cuda.synchronize()
        for name, a, b in zip(("rgb_coarse", "rgb_fine", "depth"), got, want):
            assert np.array_equal(bits(a), bits(b)), name
    assert graphed.captures == 1
    tn = to_np(rend.last_ray_bounds[0])
    assert (tn > F(NEAR)).any()
    counts = rend.last_live_counts.tolist()
    assert 0 < counts[0] < s["R"] * NC


def test_other_precisions_stay_within_their_bars_against_x3():
    """The bounded frame at "fp32" and "fp16" against the bounded x3 frame, same explicit draws, with the bars their
    own tests use for a frame: fp32 within 1e-4 (coarse everywhere; fine rgb and depth on 99.7 % of the rays, the
    project's share for inverse-CDF bin flips); fp16: rgb_coarse within twice what the oracle chain gives between the
    "e16" and "f64" reference fields under the same bounds, no 8-bit code of the fine frame more than one away."""
    s = _scene()
    grid = _sphere_grid()
    rend = _renderer(occupancy=grid, ray_bounds="grid")
    c3, f3, d3 = _frame(rend, "x3", explicit=True)
    tn, tf = (to_np(t) for t in rend.last_ray_bounds)
    c32, f32, d32 = _frame(_renderer(occupancy=grid, ray_bounds="grid"), "fp32", explicit=True)
    c16, f16, _ = _frame(_renderer(occupancy=grid, ray_bounds="grid"), "fp16", explicit=True)
    s["net"].field_precision = "x3"
    e32 = float((c32 - c3).abs().max())
    ok = ((f32 - f3).abs().amax(-1) <= 1e-4) & ((d32 - d3).abs() <= 1e-4)
    fo = oracle_field_from_net(s["net"])
    e_c = _oracle_chain(ref16.RefField(fo, "e16"), s["sphere"], tn, tf)[0]
    x_c = _oracle_chain(ref16.RefField(fo, "f64"), s["sphere"], tn, tf)[0]
    bound = float(np.abs(np.asarray(e_c, np.float64) - np.asarray(x_c, np.float64)).max())
    got = float((c16 - c3).abs().max())
    codes = lambda t: np.round(np.clip(to_np(t), 0.0, 1.0) * 255.0).astype(np.int32)   # noqa: E731
    dc = np.abs(codes(f16) - codes(f3))
    print(f"fp32 vs x3: coarse max {e32:.2e}, fine / depth within 1e-4 on {float(ok.float().mean()):.4f} of rays; "
          f"fp16 vs x3: coarse max {got:.3e}, emulation bound {bound:.3e}; fine codes differing by more than one: "
          f"{int((dc > 1).sum())} of {dc.size}")
    assert e32 <= 1e-4 and float(ok.float().mean()) >= 0.997
    assert 0.0 < got <= 2.0 * bound
    assert dc.max() <= 1


def test_refusals():
    """ValueError, never a quiet render without bounds: no grid, autograd, the module path, another value."""
    s = _scene()
    grid = _sphere_grid()
    with pytest.raises(ValueError, match="must be None or 'grid'"):
        _renderer(ray_bounds="cells")
    with pytest.raises(ValueError, match="needs occupancy"):
        _frame(_renderer(SEED, ray_bounds="grid"))
    rend = _renderer(SEED, occupancy=grid, ray_bounds="grid")
    c2w = T(s["c2w"]).reshape(1, 1, 4, 4).expand(1, s["R"], 4, 4)
    with pytest.raises(ValueError, match="inference only"):
        rend(c2w, T(s["K"]), T(s["x_pix"]), s["net"])                  # autograd on

    class Module(torch.nn.Module):                                      # honours rf(xyz, viewdirs=, coarse=)
        def forward(self, xyz, viewdirs=None, coarse=True):
            return torch.zeros(*xyz.shape[:-1], 4, device=xyz.device)
    with torch.no_grad(), pytest.raises(ValueError, match="fused path"):
        rend(c2w, T(s["K"]), T(s["x_pix"]), Module())
