"""Occupancy gating with the live count kept on the device (avr.occupancy count="device", include/avr.h "occupancy
grid, device-side count") on the GPU. References: numpy (tests/occupancy_ref.py, numpy.cumsum) and the unchanged
avr_field_fwd_points; the host-read gated_field is never one.

Shapes. avr_occ_scan: B = AVR_OCC_SCAN_RAYS rays per workgroup; R in {0, 1, B - 1, B, B + 1} (no launch of the
three-launch path, its single-workgroup path at both ends, two workgroups), 256 B + 1 (the one-workgroup middle
launch makes a second trip over the workgroup sums; there is no second scan level) and 2^23 + 1 rays of 256 (a total
above 2^31). Counted field: capacity 64 * 3 + 1 (workgroups own 64 rows in both precisions: three full ones and a
one-row tail), counts at both sides of a workgroup boundary. gated_field: 37 rays (ten 4-ray workgroups, the last
with one ray) of 40 samples (a partial mask word) and 192 (three words); the rays are made in numpy, so the live counts
of the sphere case were checked against occupancy_ref without a device: 0 < n_live < R N and n_live % 64 != 0 (the
last live field workgroup has a tail) are asserted below."""
import ctypes
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
CENTRE_B, RADIUS_B = (-0.1, 0.05, 0.0), 0.2
RES = (32, 32, 32)
SEED = 99
R_RAYS = 37
CAPACITY = 64 * 3 + 1
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


def np_rays(R, N, seed=3):
    """R rays from a point outside the box towards points in and around it, N sorted depths in [0.8, 1.8): numpy
    only, so the live counts of a case can be worked out without a device."""
    rng = np.random.default_rng(seed)
    ro = np.tile(np.array([[0.9, -0.7, 0.6]], np.float32), (R, 1)) + rng.normal(0, 0.01, (R, 3)).astype(np.float32)
    target = rng.uniform(-0.5, 0.5, (R, 3)).astype(np.float32)
    rd = target - ro
    rd = (rd / np.linalg.norm(rd, axis=-1, keepdims=True)).astype(np.float32)
    z = np.sort(rng.uniform(0.8, 1.8, (R, N)).astype(np.float32), -1)
    return ro, rd, z


def _occ(kind):
    rx, ry, rz = RES
    if kind == "sphere":
        return ref.sphere_occ(RES, LO, HI, CENTRE, RADIUS)
    if kind == "sphere_b":
        return ref.sphere_occ(RES, LO, HI, CENTRE_B, RADIUS_B)
    return np.full((rz, ry, rx), kind == "all")


def _grid(occ):
    from avr.occupancy import OccupancyGrid
    return OccupancyGrid(LO, HI, RES, T(ref.pack_bits(occ).view(np.int32)))


# ------------------------------------------------------------------ 1. avr_occ_scan
def _scan_case(counts_np):
    from avr import occupancy
    R = len(counts_np)
    counts = T(counts_np.astype(np.int32)) if R else torch.empty(0, device=DEV, dtype=torch.int32)
    total = torch.full((), -7, device=DEV, dtype=torch.int64)          # always written: no memset by the caller
    offsets, got_total = occupancy.scan(counts, total)
    torch.cuda.synchronize()
    assert got_total is total and offsets.dtype == torch.int64 and offsets.shape == (R,)
    incl = np.cumsum(counts_np.astype(np.int64), dtype=np.int64)
    want = incl - counts_np
    assert np.array_equal(offsets.cpu().numpy(), want), R
    assert int(total.item()) == (int(incl[-1]) if R else 0), R


def test_scan_matches_numpy_cumsum_exactly():
    from avr import _lib
    B = _lib.OCC_SCAN_RAYS
    rng = np.random.default_rng(17)
    for R in (0, 1, B - 1, B, B + 1, 256 * B + 1):
        for counts in (np.zeros(R, np.int64), np.full(R, 256, np.int64), rng.integers(0, 257, R)):
            _scan_case(counts)


def test_scan_total_above_2_to_31():
    R = 2 ** 23 + 1
    from avr import occupancy
    counts = torch.full((R,), 256, device=DEV, dtype=torch.int32)      # 32 MB of counts
    total = torch.full((), -7, device=DEV, dtype=torch.int64)
    offsets, _ = occupancy.scan(counts, total)
    torch.cuda.synchronize()
    assert int(total.item()) == 256 * R == 2 ** 31 + 256
    assert int(offsets[-1].item()) == 256 * (R - 1) == 2 ** 31
    assert np.array_equal(offsets.cpu().numpy(), np.arange(R, dtype=np.int64) * 256)


# ------------------------------------------------------------------ 2. avr_field_fwd_points_counted
def _points(n, seed=23):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-0.4, 0.4, (n, 3)).astype(np.float32)
    vd = rng.normal(0, 1, (n, 3))
    vd = (vd / np.linalg.norm(vd, axis=-1, keepdims=True)).astype(np.float32)
    return xyz, vd


@pytest.mark.parametrize("precision", ["fp32", "x3"])
@pytest.mark.parametrize("coarse", [True, False])
def test_counted_field_equals_field_of_the_count(golden, precision, coarse):
    net = _net(golden, precision)
    fused = net.fused()
    xyz_np, vd_np = _points(CAPACITY)
    sentinel = np.float32(-12345.5)
    for count in (0, 1, 63, 64, 65, CAPACITY):
        n = torch.tensor(count, device=DEV, dtype=torch.int64)
        with torch.no_grad():
            want = to_np(fused.forward_points_scene(T(xyz_np[:count]), T(vd_np[:count]), coarse))
            outs = []
            for tail in (np.nan, 0.0):        # what lies beyond the count is never read
                xyz, vd = xyz_np.copy(), vd_np.copy()
                xyz[count:], vd[count:] = tail, tail
                out = torch.full((CAPACITY, 4), float(sentinel), device=DEV)
                got = fused.forward_points_scene_counted(T(xyz), T(vd), n, coarse, out=out)
                assert got is out
                outs.append(to_np(out))
        torch.cuda.synchronize()
        a, b = outs
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), count
        assert np.array_equal(a[:count].view(np.uint32), want.view(np.uint32)), (precision, count)   # bit-equal
        assert (a[count:] == sentinel).all(), count                              # never written
        assert np.isfinite(a[:count]).all()


def test_counted_field_count_beyond_capacity_is_held_to_it(golden):
    """A device count above the capacity (inconsistent arguments) cannot reach past the buffers: it is held to
    capacity. The buffers here are longer than the capacity passed, so a write beyond it would show."""
    from avr import _lib
    from avr.field import PRECISIONS
    net = _net(golden, "x3")
    fused = net.fused()
    xyz_np, vd_np = _points(CAPACITY)
    cap = 100
    n = torch.tensor(10 ** 12, device=DEV, dtype=torch.int64)
    out = torch.full((CAPACITY, 4), 7.0, device=DEV)
    with torch.no_grad():
        want = to_np(fused.forward_points_scene(T(xyz_np[:cap]), T(vd_np[:cap]), True))
        entry = fused.packed(True)
        dims = entry.dims_as(PRECISIONS[fused.precision])
        xyz, vd = T(xyz_np), T(vd_np)
        _lib.call("avr_field_fwd_points_counted", ctypes.byref(dims), ctypes.byref(fused.view(0)),
                  _lib.ptr(entry.packed), _lib.ptr(fused.table(True, 0)), _lib.ptr(xyz), _lib.ptr(vd), cap,
                  _lib.ptr(n), _lib.ptr(out), _lib.stream_of(xyz))
    torch.cuda.synchronize()
    got = to_np(out)
    assert np.array_equal(got[:cap].view(np.uint32), want.view(np.uint32)) and (got[cap:] == 7.0).all()


# ------------------------------------------------------------------ 3. gated_field(count="device")
def _chain(fused, occ, ro, rd, z, coarse):
    """reference mask -> numpy compaction -> forward_points_scene -> numpy expansion."""
    live = ref.classify(occ, LO, HI, ro, rd, z)[0]
    xyz, vd = ref.compact(live, ro, rd, z)
    n = int(live.sum())
    fc = to_np(fused.forward_points_scene(T(xyz), T(vd), coarse)) if n else np.zeros((0, 4), np.float32)
    return ref.expand(live, fc), n


@pytest.mark.parametrize("precision", ["fp32", "x3"])
@pytest.mark.parametrize("N,coarse", [(40, True), (192, False)])
@pytest.mark.parametrize("kind", ["sphere", "all", "none"])
def test_gated_field_device_equals_the_reference_chain(golden, precision, N, coarse, kind):
    from avr.occupancy import gated_field
    fused = _net(golden, precision).fused()
    occ = _occ(kind)
    ro, rd, z = np_rays(R_RAYS, N)
    with torch.no_grad():
        want, n_live = _chain(fused, occ, ro, rd, z, coarse)
        got, total = gated_field(fused, _grid(occ), T(ro), T(rd), T(z), coarse, count="device")
    torch.cuda.synchronize()
    assert total.dtype == torch.int64 and total.dim() == 0 and total.is_cuda and int(total.item()) == n_live
    got = to_np(got)
    assert got.shape == (R_RAYS * N, 4)
    if kind == "sphere":
        assert 0 < n_live < R_RAYS * N and n_live % 64 != 0, n_live
    elif kind == "none":
        assert n_live == 0 and not got.any() and not np.signbit(got).any()       # every element 0.0f
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))            # bit-equal, dead rows +0.0


def test_gated_field_device_reads_nothing_back(golden, monkeypatch):
    """No .item(), no .cpu(), no torch arithmetic: the device-count chain runs with every host read of a tensor
    disabled, and under a stream capture."""
    from avr.occupancy import gated_field
    fused = _net(golden, "x3").fused()
    occ = _occ("sphere")
    ro, rd, z = (T(a) for a in np_rays(R_RAYS, 40))
    grid = _grid(occ)
    with torch.no_grad():
        gated_field(fused, grid, ro, rd, z, True, count="device")              # warm the caches
        torch.cuda.synchronize()

        def refuse(*a, **k):
            raise AssertionError("host read in the device-count chain")
        with monkeypatch.context() as m:
            for name in ("item", "cpu", "tolist", "numpy"):
                m.setattr(torch.Tensor, name, refuse)
            m.setattr(torch, "cumsum", refuse)
            got, total = gated_field(fused, grid, ro, rd, z, True, count="device")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            gated_field(fused, grid, ro, rd, z, True, count="device")
        torch.cuda.current_stream().wait_stream(side)
        with torch.cuda.graph(g):
            cap, cap_total = gated_field(fused, grid, ro, rd, z, True, count="device")
        g.replay()
        torch.cuda.synchronize()
    assert np.array_equal(to_np(cap).view(np.uint32), to_np(got).view(np.uint32))
    assert int(cap_total.item()) == int(total.item()) > 0


# ------------------------------------------------------------------ 4. renderer
def _camera(R, seed=7, angle=0.7):
    from oracle import synth
    gen = torch.Generator(device="cpu").manual_seed(seed)
    x_pix = torch.rand(1, R, 2, generator=gen).to(DEV)
    c2w = T(synth.orbit_cam2world(angle)).reshape(1, 1, 4, 4).expand(1, R, 4, 4)
    K = T(synth.default_intrinsics())[None]
    return x_pix, c2w, K


def _masked_chain(net, x_pix, c2w, K, occ, NC=128, NF=64):
    """The chain of tests/test_gpu_occupancy.py's test_renderer_with_sphere_grid_matches_masked_chain: the existing
    ops under seed SEED, offset 0, a full forward_rays, the rows the reference calls dead zeroed."""
    from avr import ops
    R = x_pix.shape[1]
    fused = net.fused()

    def masked(z, coarse):
        f = fused.forward_rays(ro[0], rd[0], z, coarse)
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


def _renderer(occupancy, offset=0):
    from avr.renderers import VolumeRenderer
    rend = VolumeRenderer(0.8, 1.8, 128, 64, 0, 0.01, True)
    rend.seed, rend._offset, rend.occupancy, rend.occupancy_count = SEED, offset, occupancy, "device"
    return rend


def _render(net, x_pix, c2w, K, occupancy, offset=0):
    rend = _renderer(occupancy, offset)
    with torch.no_grad():
        rgb_c, rgb_f, depth, _ = rend(c2w, K, x_pix, net)
    torch.cuda.synchronize()
    assert rend.last_path == "fused"
    return to_np(rgb_c[0]), to_np(rgb_f[0]), to_np(depth[0]), rend


def _compare(precision, got, want, what):
    """The bars of test_renderer_with_sphere_grid_matches_masked_chain."""
    (g_c, g_f, g_d), (w_c, w_f, w_d) = got, want
    e_c = float(np.abs(g_c - w_c).max())
    ok = (np.abs(g_f - w_f).max(-1) <= 1e-4) & (np.abs(g_d - w_d) <= 1e-4)
    print(f"{what} {precision}: coarse max err {e_c:.2e}, fine rgb / depth within 1e-4 on {ok.mean():.5f} of rays")
    assert e_c <= 1e-4
    if precision == "fp32":
        assert ok.all(), ok.mean()        # the fp32 field is bit-equal under gating: every ray
    assert ok.mean() >= 0.997, ok.mean()  # x3: the project's share for inverse-CDF bin flips under weight noise


@pytest.mark.parametrize("precision", ["fp32", "x3"])
def test_renderer_device_mode_matches_masked_chain(golden, precision):
    net = _net(golden, precision)
    R = 4096
    x_pix, c2w, K = _camera(R)
    occ = _occ("sphere")
    w_c, w_f, w_d, (n_c, n_f) = _masked_chain(net, x_pix, c2w, K, occ)
    g_c, g_f, g_d, rend = _render(net, x_pix, c2w, K, _grid(occ))
    _compare(precision, (g_c, g_f, g_d), (w_c, w_f, w_d), "device-count sphere grid vs masked chain")
    assert rend.last_live_samples is None and rend.last_live_by_pass is None
    counts = rend.last_live_counts
    assert counts.shape == (2,) and counts.dtype == torch.int64 and counts.is_cuda
    counts = counts.tolist()
    print(f"live samples {counts} of {(R * 128, R * 192)}")
    assert counts[0] == n_c and 0 < n_c < R * 128 and 0 < counts[1] < R * 192
    if precision == "fp32":
        assert counts[1] == n_f


def test_two_scenes_two_grids_equal_single_scene_device_renders(golden):
    R = 512
    one, other = _net(golden, "x3"), _net(golden, "x3", scale=0.9)
    both = build_net(golden("g4_field_full.npz"), DEV, "x3")
    both.encoder.latent = torch.cat([one.encoder.latent, other.encoder.latent], 0)
    both.poses = torch.cat([one.poses, one.poses], 0)
    grids = [_grid(_occ("sphere")), _grid(_occ("sphere_b"))]
    cams = [_camera(R, seed=7, angle=0.7), _camera(R, seed=8, angle=2.1)]
    x_pix = torch.cat([c[0] for c in cams], 0)
    c2w = torch.cat([c[1] for c in cams], 0)
    K = torch.cat([c[2] for c in cams], 0)
    rend = _renderer(grids)
    with torch.no_grad():
        rgb_c, rgb_f, depth, _ = rend(c2w, K, x_pix, both)
    torch.cuda.synchronize()
    total = np.zeros(2, np.int64)
    for b, net in enumerate((one, other)):
        s_c, s_f, s_d, single = _render(net, *cams[b], grids[b], offset=b * R)   # scene b's rays are ids b*R ...
        assert np.array_equal(to_np(rgb_c[b]), s_c) and np.array_equal(to_np(rgb_f[b]), s_f)
        assert np.array_equal(to_np(depth[b]), s_d)
        total += np.array(single.last_live_counts.tolist())
    assert rend.last_live_counts.tolist() == total.tolist() and (total > 0).all()


# ------------------------------------------------------------------ 5. graph
def test_graphed_renderer_reads_the_count_at_replay_time(golden):
    """A captured device-count frame with sphere grid A equals the chain masked by A; after grid.copy_(B) the next
    replay -- no new capture -- equals the chain masked by B, and last_live_counts holds B's counts. fp32: the
    gated field is bit-equal to the masked one, so the fine samples and with them the fine count are the chain's."""
    from avr.graphs import GraphedRenderer
    net = _net(golden, "fp32")
    R = 1024
    x_pix, c2w, K = _camera(R)
    occ_a, occ_b = _occ("sphere"), _occ("sphere_b")
    grid = _grid(occ_a)
    rend = _renderer(grid)
    graphed = GraphedRenderer(rend, net, c2w, K, x_pix)
    assert graphed.captures == 1 and any(t is grid.bits for t in graphed._held_occupancy)
    seen = []
    for occ in (occ_a, occ_b):
        if occ is occ_b:
            grid.copy_(_grid(occ_b))
        rgb_c, rgb_f, depth, _ = graphed()
        torch.cuda.synchronize()
        got = (to_np(rgb_c[0]), to_np(rgb_f[0]), to_np(depth[0]))
        counts = rend.last_live_counts.tolist()
        w_c, w_f, w_d, (n_c, n_f) = _masked_chain(net, x_pix, c2w, K, occ)
        _compare("fp32", got, (w_c, w_f, w_d), "graph replay vs masked chain")
        assert counts == [n_c, n_f] and 0 < n_c < R * 128, (counts, n_c, n_f)
        assert graphed.captures == 1
        seen.append(counts)
    assert seen[0] != seen[1]          # the two spheres differ: the second replay did not pass on the first's grid
