"""Early termination of the fine pass with every count kept on the device (ops.march_fine_device,
VolumeRenderer.t_stop_count = "device", include/avr.h "fine pass, early termination on the device") on the GPU.
References: ops.march_fine (the host-read chain, pinned to float64 by tests/test_gpu_march_kernels.py), numpy
(tests/occupancy_ref.py) and the unchanged avr_field_fwd_points / avr_march_composite; nothing is compared with a
tolerance except the renderer's termination error, whose bounds are tests/test_gpu_march.py's.

Shapes. R in {1, 3, 65, 2049}: one wave, a partial 4-ray workgroup, several workgroups with a one-ray tail, and
AVR_OCC_SCAN_RAYS + 1 (avr_occ_scan's three-launch path). (N, chunk) from composite_ref.MARCH_CASES: a single partial
chunk, partial last chunks, chunk = 1 and chunk = 64. t_stop 0 stops nothing, 1.5 stops every ray after chunk 0,
MARCH_T_STOP stops some after the first chunk, some later and some never (march_amp)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import composite_ref as cref  # noqa: E402
import occupancy_ref as ref  # noqa: E402
from helpers import build_net, to_np  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
RES = (32, 32, 32)
WIDE_LO, WIDE_HI = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)             # holds every sample of march_rays
LO, HI = (-0.45, -0.4, -0.35), (0.4, 0.45, 0.3)                    # tests/test_gpu_occupancy_count.py's box and spheres
CENTRE, RADIUS = (0.02, -0.03, 0.05), 0.3
CENTRE_B, RADIUS_B = (-0.1, 0.05, 0.0), 0.2
SEED = 99
# The fixture field is a thin fog (no ray falls below T = 0.05 in 192 samples); with its sigma output biased up by 8
# some rays stop after the second chunk of 16, most later, and the frame's rays at every depth (30, as
# tests/test_gpu_march.py's dense scene, stops every ray after its first chunk).
SIGMA_BIAS = 8.0
_NETS = {}


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def bits(t):
    """The bit pattern of an fp32 tensor or array, for comparisons that NaN and -0.0 cannot fool."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _grid(occ, lo=LO, hi=HI):
    from avr.occupancy import OccupancyGrid
    return OccupancyGrid(lo, hi, RES, T(ref.pack_bits(occ).view(np.int32)))


def _full(value):
    return np.full((RES[2], RES[1], RES[0]), bool(value))


def _sphere(b=False):
    return ref.sphere_occ(RES, LO, HI, CENTRE_B if b else CENTRE, RADIUS_B if b else RADIUS)


def _rays(R, N):
    return tuple(t.to(DEV) for t in cref.march_rays(R, N, cref.MARCH_SEED))


def _points_fn(amp):
    """march_field at the compacted points: p + 0 * 0 is p, so this is march_field's own arithmetic on the points
    the chain formed. It touches every row of the buffers, the count is not needed."""
    def fn(xyz, vd, n_live):
        zero = torch.zeros_like(xyz)
        return cref.march_field(xyz, zero, zero[:, :1], amp)[:, 0, :].contiguous()
    return fn


def _rays_fn(amp, occ=None, lo=LO, hi=HI, seen=None):
    """ops.march_fine's field: march_field on the gathered chunk, times the reference mask of that chunk with a grid
    (seen: the masked samples of the rays alive in each chunk, counted in numpy)."""
    def fn(ro_c, rd_c, z_c):
        f = cref.march_field(ro_c, rd_c, z_c, amp)
        if occ is not None:
            live = ref.classify(occ, lo, hi, to_np(ro_c), to_np(rd_c), to_np(z_c))[0]
            seen.append(int(live.sum()))
            f = f * T(live.astype(np.float32))[..., None]
        return f.reshape(-1, 4)
    return fn


# ------------------------------------------------------------------ 1. the chain against ops.march_fine
@pytest.mark.parametrize("N,chunk", cref.MARCH_CASES)
@pytest.mark.parametrize("R", [1, 3, 65, 2049])
def test_chain_equals_march_fine_bit_for_bit(R, N, chunk):
    from avr import ops
    ro, rd, z = _rays(R, N)
    amp = cref.march_amp(N)
    stopped = []
    for t_stop in (0.0, cref.MARCH_T_STOP, 1.5):
        for white_back in (True, False):
            rgb_w, dist_w, n_w = ops.march_fine(ro, rd, z, _rays_fn(amp), t_stop, white_back, chunk=chunk)
            rgb, dist, total = ops.march_fine_device(ro, rd, z, _points_fn(amp), t_stop, white_back, chunk=chunk)
            torch.cuda.synchronize()
            assert total.dtype == torch.int64 and total.dim() == 0 and total.is_cuda
            assert rgb.shape == (R, 3) and dist.shape == (R,)
            assert np.array_equal(bits(rgb), bits(rgb_w)), (t_stop, white_back)      # every ray
            assert np.array_equal(bits(dist), bits(dist_w)), (t_stop, white_back)
            assert int(total.item()) == n_w, (t_stop, white_back)
            if t_stop == 0.0:
                assert n_w == R * N
            if t_stop == 1.5:
                assert n_w == R * min(chunk, N)
        stopped.append(n_w)
    if R == 2049 and chunk < N:
        assert stopped[2] < stopped[1] < stopped[0]      # MARCH_T_STOP stops some rays, not all after chunk 0


def test_zero_rays():
    from avr import ops
    ro, rd, z = _rays(4, 20)
    total = torch.full((), -7, device=DEV, dtype=torch.int64)
    rgb, dist, got = ops.march_fine_device(ro[:0], rd[:0], z[:0], _points_fn(1.0), 1e-3, total=total)
    torch.cuda.synchronize()
    assert got is total and int(total.item()) == 0 and rgb.shape == (0, 3) and dist.shape == (0,)


# ------------------------------------------------------------------ 2. with a grid
@pytest.mark.parametrize("N,chunk", [(100, 37), (208, 64)])
@pytest.mark.parametrize("R", [65, 2049])
def test_grid_all_occupied_all_clear_and_sphere(R, N, chunk):
    from avr import ops
    ro, rd, z = _rays(R, N)
    amp = cref.march_amp(N)
    t_stop = cref.MARCH_T_STOP
    for white_back in (True, False):
        want = ops.march_fine_device(ro, rd, z, _points_fn(amp), t_stop, white_back, chunk=chunk)
        got = ops.march_fine_device(ro, rd, z, _points_fn(amp), t_stop, white_back, chunk=chunk,
                                    grid=_grid(_full(True), WIDE_LO, WIDE_HI))
        torch.cuda.synchronize()
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
        assert int(got[2].item()) == int(want[2].item())

        rgb, dist, total = ops.march_fine_device(ro, rd, z, _points_fn(amp), t_stop, white_back, chunk=chunk,
                                                 grid=_grid(_full(False), WIDE_LO, WIDE_HI))
        torch.cuda.synchronize()
        assert np.array_equal(bits(rgb), bits(np.full((R, 3), 1.0 if white_back else 0.0, np.float32)))
        assert np.array_equal(bits(dist), bits(np.zeros(R, np.float32))) and int(total.item()) == 0

        occ, seen = _sphere(), []
        rgb_w, dist_w, _ = ops.march_fine(ro, rd, z, _rays_fn(amp, occ, seen=seen), t_stop, white_back, chunk=chunk)
        rgb, dist, total = ops.march_fine_device(ro, rd, z, _points_fn(amp), t_stop, white_back, chunk=chunk,
                                                 grid=_grid(occ))
        torch.cuda.synchronize()
        assert np.array_equal(bits(rgb), bits(rgb_w)) and np.array_equal(bits(dist), bits(dist_w))
        assert int(total.item()) == sum(seen)
        if R == 2049:
            assert 0 < sum(seen) < int(want[2].item())       # the grid removes samples that termination keeps


# ------------------------------------------------------------------ 3. sentinels
def _state(R, T_col):
    st = np.zeros((R, 6), np.float64)
    st[:, 0] = T_col
    return T(st)


@pytest.mark.parametrize("c0,C", [(0, 37), (37, 37), (74, 26), (5, 1), (36, 64)])
def test_classify_and_compact_write_what_they_own_and_nothing_else(c0, C):
    from avr import _lib
    from avr._lib import call, ptr
    import ctypes
    R, N, t_stop = 67, 100, 0.25
    ro, rd, z = _rays(R, N)
    rng = np.random.default_rng(5)
    T_col = rng.uniform(0.0, 0.5, R)
    T_col[::7] = np.float32(t_stop)              # exactly at the threshold: alive
    T_col[3] = np.nan                            # not >= t_stop: stopped
    state = _state(R, T_col)
    alive = np.full(R, True) if c0 == 0 else (T_col.astype(np.float32) >= np.float32(t_stop))
    assert c0 == 0 or 0 < alive.sum() < R
    occ = _sphere()
    s = _lib.stream_of(z)
    for grid in (None, _grid(occ)):
        win = (to_np(ro), to_np(rd), to_np(z)[:, c0:c0 + C])
        live = ref.classify(occ, LO, HI, *win)[0] if grid is not None else np.full((R, C), True)
        live = live & alive[:, None]
        mask = torch.full((R,), 0x5A5A5A5A5A5A5A5A, device=DEV, dtype=torch.int64)
        counts = torch.full((R,), -9, device=DEV, dtype=torch.int32)
        call("avr_march_classify", None if grid is None else ctypes.byref(grid.desc), ptr(ro), ptr(rd), ptr(z),
             ptr(state), R, N, c0, C, t_stop, ptr(mask), ptr(counts), s)
        torch.cuda.synchronize()
        want_mask = (live.astype(np.uint64) << np.arange(C, dtype=np.uint64)).sum(-1, dtype=np.uint64)
        assert np.array_equal(mask.cpu().numpy().view(np.uint64), want_mask)       # bits at or beyond C clear
        assert np.array_equal(counts.cpu().numpy(), live.sum(1).astype(np.int32))
        assert not mask.cpu().numpy()[~alive].any()

        offsets = T(np.cumsum(live.sum(1), dtype=np.int64) - live.sum(1))
        n_live = int(live.sum())
        total = torch.tensor(n_live, device=DEV, dtype=torch.int64)
        cap = R * C
        sentinel = np.uint32(0x7FC12345)                                           # a NaN: compare as integers
        xyz = torch.full((cap + 8, 3), 0, device=DEV, dtype=torch.int32)
        xyz.fill_(int(sentinel))
        xyz, vd = xyz.view(torch.float32), xyz.clone().view(torch.float32)
        call("avr_march_compact_counted", ptr(ro), ptr(rd), ptr(z), ptr(mask), ptr(offsets), R, N, c0, C, ptr(total),
             cap, ptr(xyz), ptr(vd), s)
        torch.cuda.synchronize()
        want_xyz, want_vd = ref.compact(live, *win)
        got_xyz, got_vd = bits(xyz), bits(vd)
        assert np.array_equal(got_xyz[:n_live], bits(want_xyz)) and np.array_equal(got_vd[:n_live], bits(want_vd))
        assert (got_xyz[n_live:] == sentinel).all() and (got_vd[n_live:] == sentinel).all()


def test_composite_masked_counter_writes_then_adds():
    """accumulate = 0 overwrites a poisoned counter, accumulate = 1 adds; a count beyond the capacity is held to it."""
    from avr._lib import call, ptr, stream_of
    R, N, C = 5, 16, 16
    ro, rd, z = _rays(R, N)
    state = _state(R, np.ones(R))
    mask = torch.zeros(R, device=DEV, dtype=torch.int64)
    offsets = torch.zeros(R, device=DEV, dtype=torch.int64)
    field = torch.zeros(R * C, 4, device=DEV)
    counter = torch.full((), -7, device=DEV, dtype=torch.int64)
    for n, acc, want in ((11, 0, 11), (30, 1, 41), (10 ** 12, 1, 41 + R * C), (-5, 1, 41 + R * C), (2, 0, 2)):
        n_live = torch.tensor(n, device=DEV, dtype=torch.int64)
        call("avr_march_composite_masked", ptr(z), ptr(field), ptr(mask), ptr(offsets), ptr(n_live), R * C, R, N, 0, C,
             1.8, 1e-3, ptr(state), ptr(counter), acc, stream_of(z))
        torch.cuda.synchronize()
        assert int(counter.item()) == want, (n, acc)
    st = state.cpu().numpy()
    assert (st[:, 0] == 1.0).all() and not st[:, 1:].any()        # all-clear masks: exact zeros leave the state alone


# ------------------------------------------------------------------ 4. the real field, both precisions
def _net(golden, precision, scale=1.0, sigma_bias=0.0):
    key = (precision, scale, sigma_bias)
    if key not in _NETS:
        net = build_net(golden("g4_field_full.npz"), DEV, precision)
        if scale != 1.0:
            net.encoder.latent = net.encoder.latent * scale
        if sigma_bias:
            with torch.no_grad():
                for mlp in (net.mlp_coarse, net.mlp_fine):
                    mlp.lin_out.bias[3] += sigma_bias
        _NETS[key] = net
    return _NETS[key]


def np_rays(R, N, seed=3):
    """tests/test_gpu_occupancy_count.py's rays: from a point outside the box towards points in and around it."""
    rng = np.random.default_rng(seed)
    ro = np.tile(np.array([[0.9, -0.7, 0.6]], np.float32), (R, 1)) + rng.normal(0, 0.01, (R, 3)).astype(np.float32)
    target = rng.uniform(-0.5, 0.5, (R, 3)).astype(np.float32)
    rd = target - ro
    rd = (rd / np.linalg.norm(rd, axis=-1, keepdims=True)).astype(np.float32)
    z = np.sort(rng.uniform(0.8, 1.8, (R, N)).astype(np.float32), -1)
    return ro, rd, z


def _restated_chain(fused, occ, ro, rd, z, t_stop, chunk, white_back=True, infinity=1.8):
    """The chain from entry points that were there before it, per chunk: alive set from the state, reference mask,
    numpy compaction, forward_points_scene, numpy expansion, avr_march_composite with the ascending active list."""
    from avr import _lib
    from avr._lib import call, ptr
    R, N = z.shape
    ro_t, rd_t, z_t = T(ro), T(rd), T(z)
    s = _lib.stream_of(z_t)
    state = torch.empty(_lib.size_query("avr_march_state_bytes", R), device=DEV, dtype=torch.uint8)
    scratch = torch.empty(R, device=DEV, dtype=torch.int32)
    n_next = torch.zeros(1, device=DEV, dtype=torch.int32)
    call("avr_march_init", R, ptr(state), ptr(scratch), s)
    evaluated, alive_counts = 0, []
    for c0 in range(0, N, chunk):
        C = min(chunk, N - c0)
        torch.cuda.synchronize()
        T_col = state.view(torch.float64).reshape(R, 6)[:, 0].cpu().numpy()
        alive = np.full(R, True) if c0 == 0 else (T_col.astype(np.float32) >= np.float32(t_stop))
        alive_counts.append(int(alive.sum()))
        if not alive.any():
            continue
        a_ro, a_rd, a_z = ro[alive], rd[alive], z[alive, c0:c0 + C]
        live = ref.classify(occ, LO, HI, a_ro, a_rd, a_z)[0] if occ is not None else np.full(a_z.shape, True)
        n = int(live.sum())
        evaluated += n
        xyz, vd = ref.compact(live, a_ro, a_rd, a_z)
        fc = to_np(fused.forward_points_scene(T(xyz), T(vd), False)) if n else np.zeros((0, 4), np.float32)
        field = T(ref.expand(live, fc))
        active = T(np.nonzero(alive)[0].astype(np.int32))
        n_next.zero_()
        call("avr_march_composite", ptr(z_t), ptr(field), ptr(active), int(alive.sum()), N, c0, C, infinity, t_stop,
             ptr(state), ptr(scratch), ptr(n_next), s)
    rgb = torch.empty(R, 3, device=DEV)
    dist = torch.empty(R, device=DEV)
    call("avr_march_finish", ptr(state), R, 1 if white_back else 0, ptr(rgb), ptr(dist), s)
    torch.cuda.synchronize()
    return rgb, dist, evaluated, alive_counts


@pytest.mark.parametrize("precision", ["fp32", "x3"])
@pytest.mark.parametrize("kind", ["none", "sphere"])
def test_real_field_equals_the_restated_chain(golden, precision, kind):
    from avr import ops
    fused = _net(golden, precision, sigma_bias=SIGMA_BIAS).fused()
    R, N, chunk, t_stop = 133, 72, 16, 0.05
    ro, rd, z = np_rays(R, N)
    occ = _sphere() if kind == "sphere" else None
    grid = _grid(occ) if occ is not None else None

    def fn(xyz, vd, n_live):
        return fused.forward_points_scene_counted(xyz, vd, n_live, False, 0)
    with torch.no_grad():
        rgb_w, dist_w, n_w, alive_counts = _restated_chain(fused, occ, ro, rd, z, t_stop, chunk)
        runs = [ops.march_fine_device(T(ro), T(rd), T(z), fn, t_stop, chunk=chunk, grid=grid) for _ in range(2)]
    torch.cuda.synchronize()
    print(f"{precision} {kind}: alive rays per chunk {alive_counts}, evaluated {n_w} of {R * N}")
    # termination bites, on some rays sooner than on others
    assert alive_counts[0] == R and alive_counts[1] > 0 and min(alive_counts) < R and len(set(alive_counts)) > 2
    for rgb, dist, total in runs:                                   # the second run: reproducible, also in x3
        assert np.array_equal(bits(rgb), bits(rgb_w)) and np.array_equal(bits(dist), bits(dist_w))
        assert int(total.item()) == n_w
    assert np.isfinite(to_np(rgb_w)).all()


# ------------------------------------------------------------------ 5. renderer
def _camera(R, seed=7, angle=0.7):
    from oracle import synth
    gen = torch.Generator(device="cpu").manual_seed(seed)
    x_pix = torch.rand(1, R, 2, generator=gen).to(DEV)
    c2w = T(synth.orbit_cam2world(angle)).reshape(1, 1, 4, 4).expand(1, R, 4, 4)
    K = T(synth.default_intrinsics())[None]
    return x_pix, c2w, K


def _renderer(t_stop, t_stop_count="device", occupancy=None, offset=0):
    from avr.renderers import VolumeRenderer
    rend = VolumeRenderer(0.8, 1.8, 128, 64, 0, 0.01, True)
    rend.seed, rend._offset, rend.t_stop, rend.t_stop_count = SEED, offset, t_stop, t_stop_count
    rend.occupancy, rend.occupancy_count = occupancy, "device"
    return rend


def _render(rend, net, x_pix, c2w, K):
    with torch.no_grad():
        out = rend(c2w, K, x_pix, net)
    torch.cuda.synchronize()
    assert rend.last_path == "fused"
    return [bits(o) for o in out]


def test_renderer_device_mode_equals_host_mode_in_fp32(golden):
    net = _net(golden, "fp32")
    x_pix, c2w, K = _camera(4096)
    host = _renderer(1e-3, "host")
    want = _render(host, net, x_pix, c2w, K)
    dev = _renderer(1e-3, "device")
    got = _render(dev, net, x_pix, c2w, K)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert dev.last_fine_samples is None
    counts = dev.last_fine_counts
    assert counts.dim() == 0 and counts.dtype == torch.int64 and counts.is_cuda
    # the host chain evaluates whole chunks of the rays alive; so does the device chain without a grid
    assert int(counts.item()) == host.last_fine_samples


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("t_stop", [1e-5, 1e-2, 0.3])
def test_renderer_grid_plus_termination_error_bound(golden, t_stop, dense):
    """Against the same grid without t_stop: tests/test_gpu_march.py::test_termination_error_bound's bounds (the
    skipped tail's weight is at most t_stop, its distance at most t_stop * max zz <= 1.8 t_stop, plus the fp32
    rounding of two different summation orders). On that test's dense scene (sigma about 30 inside the sphere grid,
    whose chords are at most 0.6 long) termination removes occupied samples where a ray falls below t_stop at a
    64-sample boundary with part of its chord still ahead: T = 1e-2 needs 0.15 of chord, 0.3 needs 0.04, so both
    must evaluate fewer samples than the grid alone; 1e-5 needs 0.38, which a ray may not have left at a boundary, so
    there only "no more than the grid alone" is asserted."""
    net = _net(golden, "x3", sigma_bias=30.0 if dense else 0.0)
    x_pix, c2w, K = _camera(4096)
    grid = _grid(_sphere())
    plain = _renderer(None, occupancy=grid)
    with torch.no_grad():
        rgb_c0, rgb_a, depth_a, _ = plain(c2w, K, x_pix, net)
    stop = _renderer(t_stop, occupancy=grid)
    with torch.no_grad():
        rgb_c1, rgb_b, depth_b, _ = stop(c2w, K, x_pix, net)
    torch.cuda.synchronize()
    assert np.array_equal(bits(rgb_c1), bits(rgb_c0))           # the coarse pass is untouched
    d_rgb = float((rgb_b - rgb_a).abs().max())
    d_depth = float((depth_b - depth_a).abs().max())
    fine_grid, fine_stop = int(plain.last_live_counts[1].item()), int(stop.last_fine_counts.item())
    print(f"t_stop {t_stop} dense {dense}: d_rgb {d_rgb:.3e} d_depth {d_depth:.3e}, fine samples {fine_stop} with "
          f"termination, {fine_grid} with the grid alone")
    assert d_rgb <= t_stop + 2e-6, d_rgb
    assert d_depth <= 2.0 * t_stop + 2e-5, d_depth
    assert stop.last_live_counts.tolist()[0] == plain.last_live_counts.tolist()[0]
    assert 0 < fine_stop <= fine_grid
    if dense and t_stop >= 1e-2:
        assert fine_stop < fine_grid


def test_two_scenes_two_grids_equal_single_scene_renders(golden):
    R = 512
    one, other = _net(golden, "x3"), _net(golden, "x3", scale=0.9)
    both = build_net(golden("g4_field_full.npz"), DEV, "x3")
    both.encoder.latent = torch.cat([one.encoder.latent, other.encoder.latent], 0)
    both.poses = torch.cat([one.poses, one.poses], 0)
    grids = [_grid(_sphere()), _grid(_sphere(b=True))]
    cams = [_camera(R, seed=7, angle=0.7), _camera(R, seed=8, angle=2.1)]
    x_pix = torch.cat([c[0] for c in cams], 0)
    c2w = torch.cat([c[1] for c in cams], 0)
    K = torch.cat([c[2] for c in cams], 0)
    rend = _renderer(0.3, occupancy=grids)
    with torch.no_grad():
        out = rend(c2w, K, x_pix, both)
    torch.cuda.synchronize()
    fine, live = 0, np.zeros(2, np.int64)
    for b, net in enumerate((one, other)):
        single = _renderer(0.3, occupancy=grids[b], offset=b * R)              # scene b's rays are ids b * R ...
        s_c, s_f, s_d, _ = _render(single, net, *cams[b])
        assert np.array_equal(bits(out[0][b]), s_c[0]) and np.array_equal(bits(out[1][b]), s_f[0])
        assert np.array_equal(bits(out[2][b]), s_d[0])
        fine += int(single.last_fine_counts.item())
        live += np.array(single.last_live_counts.tolist())
    assert int(rend.last_fine_counts.item()) == fine > 0
    assert rend.last_live_counts.tolist() == live.tolist() and live[1] == fine


# ------------------------------------------------------------------ 6. capture
@pytest.mark.parametrize("gated", [False, True])
def test_graphed_renderer_replays_the_device_chain(golden, gated):
    """The replay equals the eager call bit for bit, also after new poses; grid.copy_ between replays takes effect
    without a new capture; last_fine_counts is the replay's."""
    from avr.graphs import GraphedRenderer
    net = _net(golden, "x3", sigma_bias=SIGMA_BIAS)
    R, t_stop = 1024, 0.3
    x_pix, c2w, K = _camera(R)
    _, c2w_b, _ = _camera(R, angle=2.1)
    grid = _grid(_sphere()) if gated else None
    rend = _renderer(t_stop, occupancy=grid)
    graphed = GraphedRenderer(rend, net, c2w, K, x_pix)
    assert graphed.captures == 1
    seen = []
    steps = [(c2w, None), (c2w_b, None)] + ([(c2w_b, _sphere(b=True))] if gated else [])
    for pose, new_occ in steps:
        if new_occ is not None:
            grid.copy_(_grid(new_occ))
        out = graphed(cam2world=pose)
        torch.cuda.synchronize()
        got = [bits(o) for o in out]
        n_got = int(rend.last_fine_counts.item())
        eager = _renderer(t_stop, occupancy=grid)
        want = _render(eager, net, x_pix, pose, K)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        assert n_got == int(eager.last_fine_counts.item()) and 0 < n_got < R * 192
        if gated:
            assert rend.last_live_counts.tolist() == eager.last_live_counts.tolist()
        assert graphed.captures == 1
        seen.append((n_got, got[1].copy()))
    for a, b in zip(seen, seen[1:]):
        assert a[0] != b[0] and not np.array_equal(a[1], b[1])     # each step rendered something else


# ------------------------------------------------------------------ 7. CLI
def test_render_cli_device_mode_with_a_grid(capsys):
    """python -m avr.render with --t-stop-count device and --occupancy: the JSON line names the mode and reports the
    evaluated fine samples, below the grid's live fine samples' ceiling of every fine sample."""
    import json
    from avr import render
    render.main(["--frames", "2", "--res", "32", "--n-coarse", "64", "--n-fine", "32", "--t-stop", "1e-3",
                 "--t-stop-count", "device", "--occupancy", "32", "--occupancy-count", "device", "--sigma-bias", "30",
                 "--warmup", "0"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["t_stop_count"] == "device" and line["occupancy_count"] == "device" and line["t_stop"] == 1e-3
    assert 0 < line["fine_samples_evaluated"] < 2 * 32 * 32 * 96 and 0 < line["fine_samples_fraction"] < 1.0
    assert 0 < line["live_samples_fraction"] < 1.0
