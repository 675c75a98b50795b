"""The field's "fp16" inference precision (AVR_FIELD_FP16: one fp16 product per term on the x3 blob) on the GPU.

Accuracy is judged against the reference's own goldens (g4_field_*), with the bar taken from the float64 emulation of
tests/field_fp16_ref.py computed here: the kernel's mean absolute error against the golden, rgb and sigma separately,
is at most 1.5x the emulation's, its max at most 2x (rounding flips cascade through the layers, so two correct
implementations differ on single points by up to the error itself; an fp32-accumulating emulation stayed within 1.03x /
1.05x, truncation instead of rounding to nearest is at 3x the mean). The kernel must really be on one product: mean
|fp16 - x3| on the same points is at least 0.25x the emulation's mean error. Then the shapes and entry points (ragged
sizes, rays, batches, the counted launch, determinism), the renderer routes that end in the field, and the plumbing
(shared blob and tables, training unchanged, the nets that stay on the module path). Every test here fails without
the precision ("fp16" is not one there)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_fp16_ref as ref  # noqa: E402
from helpers import build_net, oracle_field, oracle_field_from_net, to_np  # noqa: E402
from oracle import avr_oracle as O  # noqa: E402
from oracle import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
TAGS = ("small", "small_mv", "full", "mv512", "d256")
SENTINEL = np.float32(-12345.5)
_NETS, _REFS, _SCENE = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import avr
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    avr.load_library()


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def bits(t):
    return to_np(t).view(np.uint32)


def _net(golden, tag, precision="fp16"):
    """One net per tag; the precision is switched on it (x3 and fp16 share its blob and tables)."""
    if tag not in _NETS:
        _NETS[tag] = build_net(golden(f"g4_field_{tag}.npz"), DEV, precision)
    _NETS[tag].field_precision = precision
    return _NETS[tag]


def _refs(golden, tag):
    """tag -> (golden, {(mode, coarse): (384, 4) float64}): the emulation, computed once per tag."""
    if tag not in _REFS:
        g = golden(f"g4_field_{tag}.npz")
        f = oracle_field(g)
        _REFS[tag] = (g, {(mode, c): ref.RefField(f, mode)(g["xyz"], g["viewdirs"], coarse=c)[0]
                          for mode in ("f64", "e16") for c in (True, False)})
    return _REFS[tag]


def _gold(g, coarse):
    return g["out_coarse" if coarse else "out_fine"][0]


def _within_bars(what, out, emu, gold):
    """The bars of the module docstring on rows out / emu / gold (M, 4); returns the four ratios kernel / emulation."""
    k, e = ref.errors(out, gold), ref.errors(emu, gold)
    ratios = tuple(a / b if b > 0 else (0.0 if a == 0 else np.inf) for a, b in zip(k, e))
    print(f"{what}: kernel (rgb mean, rgb max, sigma mean, sigma max) {tuple(f'{v:.3e}' for v in k)} emulation "
          f"{tuple(f'{v:.3e}' for v in e)} ratios {tuple(f'{v:.2f}' for v in ratios)}")
    assert k[0] <= 1.5 * e[0] and k[2] <= 1.5 * e[2], (what, "mean", k, e)
    assert k[1] <= 2.0 * e[1] and k[3] <= 2.0 * e[3], (what, "max", k, e)
    return ratios


# ------------------------------------------------------------------ 1. parity against the goldens
@pytest.mark.parametrize("tag,waves", [(t, None) for t in TAGS] + [("full", "4"), ("mv512", "4")])
def test_field_parity_against_the_goldens(golden, tag, waves, monkeypatch):
    """waves "4": d_hidden 512 on the 4-wave layout (AVR_X3_WAVES=4); otherwise 8 waves at 512, 4 at 64 / 256."""
    if waves:
        monkeypatch.setenv("AVR_X3_WAVES", waves)
    g, emu = _refs(golden, tag)
    xyz, vd = T(g["xyz"]), T(g["viewdirs"])
    for coarse in (True, False):
        with torch.no_grad():
            net = _net(golden, tag, "fp16")
            assert net.can_fuse(xyz)
            out = to_np(net(xyz, coarse=coarse, viewdirs=vd))[0]
            x3 = to_np(_net(golden, tag, "x3")(xyz, coarse=coarse, viewdirs=vd))[0]
        _within_bars(f"{tag} waves {waves or 'default'} coarse {coarse}", out, emu[("e16", coarse)], _gold(g, coarse))
        e = ref.errors(emu[("e16", coarse)], _gold(g, coarse))
        d = ref.errors(out, x3)
        print(f"   mean |fp16 - x3| rgb {d[0]:.3e} sigma {d[2]:.3e} (emulation's mean error rgb {e[0]:.3e} sigma {e[2]:.3e})")
        assert d[0] >= 0.25 * e[0] and d[2] >= 0.25 * e[2], (tag, coarse, d, e)   # really one product


# ------------------------------------------------------------------ 2. shapes and entry points
@pytest.mark.parametrize("tag", ["full", "d256"])
@pytest.mark.parametrize("M", [1, 63, 65, 197])
def test_ragged_sizes_and_untouched_tail(golden, tag, M):
    g, emu = _refs(golden, tag)
    net = _net(golden, tag, "fp16")
    xyz, vd = T(g["xyz"][0, :M]), T(g["viewdirs"][0, :M])
    for coarse in (True, False):
        buf = torch.full((M + 70, 4), float(SENTINEL), device=DEV)
        with torch.no_grad():
            got = net.fused().forward_points_scene(xyz, vd, coarse, 0, out=buf[:M])
        torch.cuda.synchronize()
        assert got.data_ptr() == buf.data_ptr()
        assert (to_np(buf[M:]) == SENTINEL).all()
        _within_bars(f"{tag} M {M} coarse {coarse}", to_np(buf[:M]), emu[("e16", coarse)][:M], _gold(g, coarse)[:M])


@pytest.mark.parametrize("tag", ["full", "d256"])
def test_rays_entry_equals_points_entry(golden, tag):
    """What tests/test_gpu_parity.py::test_field_rays_mode_matches_points_mode holds x3 to: bit equality."""
    net = _net(golden, tag, "fp16")
    R, N = 300, 17
    gen = torch.Generator(device="cpu").manual_seed(11)
    ro = torch.tensor([[0.3, -1.1, 0.5]], device=DEV).expand(R, 3).contiguous()
    rd = torch.nn.functional.normalize(-ro + 0.2 * torch.randn(R, 3, generator=gen).to(DEV), dim=-1)
    z = torch.sort(0.8 + torch.rand(R, N, generator=gen).to(DEV), -1)[0]
    with torch.no_grad():
        a = net.fused().forward_rays(ro, rd, z, coarse=True)
        pts = ro[:, None, :] + rd[:, None, :] * z[..., None]
        b = net(pts.reshape(1, -1, 3), coarse=True, viewdirs=rd[:, None, :].expand(R, N, 3).reshape(1, -1, 3))
    assert np.array_equal(bits(a), bits(b[0]))


@pytest.mark.parametrize("tag", ["full", "d256"])
def test_three_scenes_in_one_launch_equal_three_launches(golden, tag):
    g = golden(f"g4_field_{tag}.npz")
    one = _net(golden, tag, "fp16")
    net = build_net(g, DEV, "fp16")
    net.encoder.latent = torch.cat([one.encoder.latent * s for s in (1.0, 0.9, 1.1)], 0)
    net.poses = torch.cat([one.poses] * 3, 0)
    B = 197
    rng = np.random.default_rng(5)
    xyz = T(rng.uniform(-0.4, 0.4, (3, B, 3)).astype(np.float32))
    vd = torch.nn.functional.normalize(T(rng.normal(0, 1, (3, B, 3)).astype(np.float32)), dim=-1)
    fused = net.fused()
    with torch.no_grad():
        both = net(xyz, coarse=False, viewdirs=vd)                                    # avr_field_fwd_points_batch
        singles = [fused.forward_points_scene(xyz[s], vd[s], False, s) for s in range(3)]
        R, N = 50, 7
        ro, rd = xyz[:, :R].contiguous(), vd[:, :R].contiguous()
        z = torch.sort(0.8 + T(rng.random((3 * R, N)).astype(np.float32)), -1)[0]
        rays = fused.forward_rays_batch(ro, rd, z, True)                              # avr_field_fwd_rays_batch
        rays_single = [fused.forward_rays(ro[s], rd[s], z[s * R:(s + 1) * R], True, sb=s) for s in range(3)]
    for s in range(3):
        assert np.array_equal(bits(both[s]), bits(singles[s])), s
        assert np.array_equal(bits(rays[s * R * N:(s + 1) * R * N]), bits(rays_single[s])), s
    assert not np.array_equal(bits(singles[0]), bits(singles[1]))


@pytest.mark.parametrize("tag", ["full", "d256"])
def test_counted_launch(golden, tag):
    """count = capacity equals the plain launch bit for bit; count 70 of capacity 197 writes rows below 70 only (the
    plain launch of those 70 rows); count 0 writes nothing."""
    g = golden(f"g4_field_{tag}.npz")
    fused = _net(golden, tag, "fp16").fused()
    cap = 197
    xyz, vd = T(g["xyz"][0, :cap]).contiguous(), T(g["viewdirs"][0, :cap]).contiguous()
    for count in (cap, 70, 0):
        n = torch.tensor(count, device=DEV, dtype=torch.int64)
        buf = torch.full((cap, 4), float(SENTINEL), device=DEV)
        with torch.no_grad():
            fused.forward_points_scene_counted(xyz, vd, n, False, 0, out=buf)
            plain = fused.forward_points_scene(xyz[:count], vd[:count], False, 0) if count else buf[:0]
        torch.cuda.synchronize()
        assert np.array_equal(bits(buf[:count]), bits(plain)), count
        assert (to_np(buf[count:]) == SENTINEL).all(), count


@pytest.mark.parametrize("tag", ["full", "d256"])
def test_two_launches_are_bit_identical(golden, tag):
    g = golden(f"g4_field_{tag}.npz")
    net = _net(golden, tag, "fp16")
    xyz, vd = T(g["xyz"]), T(g["viewdirs"])
    with torch.no_grad():
        a, b = (bits(net(xyz, coarse=False, viewdirs=vd)) for _ in range(2))
    assert np.array_equal(a, b)


# ------------------------------------------------------------------ 3. through the renderer
NC, NF, SIDE = 32, 16, 16
LO, HI, RES = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (32, 32, 32)


def _scene():
    """synthetic_scene(sigma_bias=30) and a 16 x 16 ray frame with explicit draws (fixed seed), shared by the tests."""
    if not _SCENE:
        from avr.scene import synthetic_scene
        net = synthetic_scene(DEV, sigma_bias=30.0)
        R = SIDE * SIDE
        ij = (np.stack(np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="xy"), -1).reshape(1, R, 2) + 0.5) / SIDE
        rng = np.random.default_rng(7)
        noise = {"coarse": rng.random((1, R, NC), dtype=np.float32), "u": rng.random((1, R, NF), dtype=np.float32),
                 "u2": rng.random((1, R, NF), dtype=np.float32), "depth": np.zeros((1, R, 0), np.float32)}
        _SCENE.update(net=net, x_pix=ij.astype(np.float32), c2w=synth.orbit_cam2world(0.4),
                      K=synth.default_intrinsics()[None], noise=noise, R=R)
    return _SCENE


def _renderer(seed=None, **attrs):
    from avr.renderers import VolumeRenderer
    rend = VolumeRenderer(0.8, 1.8, NC, NF, 0, 0.01, True)
    rend.seed, rend._offset = seed, 0
    for k, v in attrs.items():
        setattr(rend, k, v)
    return rend


def _frame(precision, rend=None, explicit=True):
    s = _scene()
    s["net"].field_precision = precision
    rend = rend or _renderer()
    c2w = T(s["c2w"]).reshape(1, 1, 4, 4).expand(1, s["R"], 4, 4)
    noise = {k: T(v) for k, v in s["noise"].items()} if explicit else None
    with torch.no_grad():
        out = rend(c2w, T(s["K"]), T(s["x_pix"]), s["net"], noise=noise)
    torch.cuda.synchronize()
    assert rend.last_path == "fused"
    return out[:3], rend


def test_fp16_frame_against_x3_frame():
    """rgb_coarse within 2x of what oracle.render gives between the "e16" and "f64" reference fields on the same
    draws; no 8-bit channel value of the fine frame more than one code away."""
    s = _scene()
    (c16, f16, _), _ = _frame("fp16")
    (c3, f3, _), _ = _frame("x3")
    fo = oracle_field_from_net(s["net"])
    n = s["noise"]
    args = (np.broadcast_to(s["c2w"], (1, s["R"], 4, 4)), s["K"], s["x_pix"])
    tail = (0.8, 1.8, NC, NF, 0, 0.01, True, n["coarse"], n["u"], n["u2"], n["depth"])
    e_c = O.render(*args, ref.RefField(fo, "e16"), *tail)[0]
    x_c = O.render(*args, ref.RefField(fo, "f64"), *tail)[0]
    bound = float(np.abs(np.asarray(e_c, np.float64) - np.asarray(x_c, np.float64)).max())
    got = float((c16 - c3).abs().max())
    codes = lambda t: np.round(np.clip(to_np(t), 0.0, 1.0) * 255.0).astype(np.int32)   # noqa: E731
    dc = np.abs(codes(f16) - codes(f3))
    print(f"rgb_coarse |fp16 - x3| max {got:.3e}, emulation |e16 - f64| max {bound:.3e} (ratio {got / bound:.2f}); "
          f"fine 8-bit codes differing: {(dc > 0).mean():.4f}, by more than one: {(dc > 1).sum()} of {dc.size}")
    assert got > 0.0 and got <= 2.0 * bound, (got, bound)
    assert dc.max() <= 1, int(dc.max())


def test_all_occupied_grid_and_idle_termination_equal_the_plain_frame():
    """occupancy_count = "device" under a grid with every cell set equals the ungated fp16 frame bit for bit (same
    samples in the same workgroups). t_stop_count = "device" at t_stop = 0, which terminates nothing: the coarse
    frame equals the plain one bit for bit and the fine pass evaluates every sample, but its chunked composite sums
    in another order than the single-launch one at any precision (tests/test_gpu_march.py::
    test_termination_off_equals_full_pass: rgb within 1e-6, depth within 1e-5; 1.2e-7, one ulp, measured here), so
    the fine frame is held bit for bit to the host-count chain of the same t_stop and to those bounds against the
    plain frame."""
    from avr.occupancy import OccupancyGrid
    want, _ = _frame("fp16", _renderer(seed=99), explicit=False)
    grid = OccupancyGrid.all_occupied(LO, HI, RES, DEV)
    gated, rend = _frame("fp16", _renderer(seed=99, occupancy=grid, occupancy_count="device"), explicit=False)
    for name, a, b in zip(("rgb_coarse", "rgb_fine", "depth"), gated, want):
        print(f"all-occupied {name}: max |gated - plain| {float((a - b).abs().max()):.3e}")
        assert np.array_equal(bits(a), bits(b)), name
    assert rend.last_live_counts.tolist() == [_scene()["R"] * NC, _scene()["R"] * (NC + NF)]
    stopped, rend = _frame("fp16", _renderer(seed=99, t_stop=0.0, t_stop_count="device"), explicit=False)
    host, _ = _frame("fp16", _renderer(seed=99, t_stop=0.0, t_stop_count="host"), explicit=False)
    for name, a, b, c in zip(("rgb_coarse", "rgb_fine", "depth"), stopped, want, host):
        print(f"t_stop 0 {name}: max |device - plain| {float((a - b).abs().max()):.3e}, |device - host| "
              f"{float((a - c).abs().max()):.3e}")
        assert np.array_equal(bits(a), bits(c)), name
    assert np.array_equal(bits(stopped[0]), bits(want[0]))
    assert float((stopped[1] - want[1]).abs().max()) <= 1e-6 and float((stopped[2] - want[2]).abs().max()) <= 1e-5
    assert int(rend.last_fine_counts.item()) == _scene()["R"] * (NC + NF)


def test_graphed_renderer_replays_and_recaptures_on_a_precision_switch():
    from avr.graphs import GraphedRenderer
    s = _scene()
    net = s["net"]
    c2w = T(s["c2w"]).reshape(1, 1, 4, 4).expand(1, s["R"], 4, 4)
    net.field_precision = "x3"
    graphed = GraphedRenderer(_renderer(seed=99), net, c2w, T(s["K"]), T(s["x_pix"]))
    x3 = [bits(o) for o in graphed()[:3]]
    assert graphed.captures == 1
    net.field_precision = "fp16"
    for _ in range(2):
        got = [bits(o) for o in graphed()[:3]]
        torch.cuda.synchronize()
        assert graphed.captures == 2                                  # the switch captured again, once
        want, _ = _frame("fp16", _renderer(seed=99), explicit=False)
        for a, b in zip(got, want):
            assert np.array_equal(a, bits(b))
    assert not np.array_equal(got[1], x3[1])
    want_x3, _ = _frame("x3", _renderer(seed=99), explicit=False)
    assert np.array_equal(x3[1], bits(want_x3[1]))


def test_grid_build_under_fp16_differs_from_x3_only_near_the_threshold():
    """OccupancyGrid.from_field on a 32^3 grid (dilate 0, so a cell's bit is its own sigma test; the threshold is the
    median sigma, so that both kinds of cell exist): the bits under fp16 equal those under x3 except in cells where
    some sigma the build looks at is within the emulation's sigma error of the threshold. That error is taken on
    this scene: twice (the max bar of the parity tests) the max |e16 - f64| sigma over 1024 of the cell centres.
    The count of such cells is printed, not capped."""
    from avr.occupancy import AXIS_DIRS, OccupancyGrid
    s = _scene()
    net = s["net"]
    net.field_precision = "x3"
    centres = OccupancyGrid.cell_centres(LO, HI, RES, DEV)
    sigmas = []
    with torch.no_grad():   # what the build evaluates: both MLPs, six directions, the centres in this order
        for coarse in (True, False):
            for d in AXIS_DIRS:
                vd = torch.tensor(d, device=DEV, dtype=torch.float32).expand_as(centres).contiguous()
                sigmas.append(net.fused().forward_points_scene(centres, vd, coarse)[:, 3])
    sigmas = torch.stack(sigmas)
    thr = float(sigmas.max(0)[0].median())
    rng = np.random.default_rng(13)
    pick = rng.choice(centres.shape[0], 1024, replace=False)
    pts = to_np(centres)[pick][None]
    vds = np.asarray(AXIS_DIRS, np.float32)[rng.integers(0, 6, 1024)][None]
    fo = oracle_field_from_net(net)
    tol = 2.0 * max(float(np.abs(ref.RefField(fo, "e16")(pts, vds, coarse=c)[..., 3]
                                 - ref.RefField(fo, "f64")(pts, vds, coarse=c)[..., 3]).max()) for c in (True, False))
    grids = {}
    for precision in ("x3", "fp16"):
        net.field_precision = precision
        grids[precision] = OccupancyGrid.from_field(net, LO, HI, RES, sigma_thr=thr, dilate=0)
    torch.cuda.synchronize()
    diff = (grids["x3"].bits ^ grids["fp16"].bits).cpu().numpy().view(np.uint32)
    cells = np.unpackbits(diff.view(np.uint8), bitorder="little").astype(bool)          # cell index, x fastest
    near = to_np(((sigmas - thr).abs() <= tol).any(0).float()).astype(bool)
    live = grids["x3"].live_fraction()
    print(f"grid build at threshold {thr:.4f}: {int(cells.sum())} of {cells.size} cells differ between fp16 and x3 "
          f"(live share {live:.3f}); {int(near.sum())} cells have a sigma within {tol:.2e} of the threshold")
    assert 0.0 < live < 1.0
    assert not (cells & ~near).any(), int((cells & ~near).sum())


def test_render_orbit_and_refine_under_fp16():
    from avr.occupancy import OccupancyGrid
    from avr.scene import INTRINSICS
    from avr.video import render_orbit
    net = _scene()["net"]
    net.field_precision = "fp16"
    frames, stats = render_orbit(_renderer(seed=3), net, torch.tensor(INTRINSICS, device=DEV), 2, 1.3, SIDE,
                                 occupancy=64, occupancy_sigma=1.0, occupancy_count="device", occupancy_refine=2)
    assert len(frames) == 2 and frames[0].shape == (SIDE, SIDE, 3) and frames[0].dtype == np.uint8
    coarse = OccupancyGrid.from_field(net, LO, HI, (32, 16, 16), sigma_thr=1.0)
    fine = OccupancyGrid.refine_from_field(net, coarse, 2, sigma_thr=1.0)
    assert tuple(fine.res) == (64, 32, 32) and 0.0 < fine.live_fraction() <= 1.0


# ------------------------------------------------------------------ 4. plumbing
def test_x3_and_fp16_share_one_blob_and_one_set_of_tables(golden):
    from avr import _lib
    from avr.field import PRECISIONS
    assert PRECISIONS["fp16"] == 2 == _lib.FIELD_FP16 and _lib.load().avr_version() == 18
    net = _net(golden, "small", "x3")
    fused = net.fused()
    seen = {}
    for precision in ("x3", "fp16", "x3", "fp16", "fp32"):
        net.field_precision = precision
        fused = net.fused()
        assert fused.precision == precision
        seen.setdefault(precision, []).append((fused.packed(True), fused.packed(False), fused.table(True),
                                               fused.table(False), fused.tables_batch(True, 1)))
    first = seen["x3"][0]
    for other in seen["x3"][1:] + seen["fp16"]:
        assert all(a is b for a, b in zip(first, other))              # nothing repacked, nothing rebuilt
    assert all(a is not b for a, b in zip(first, seen["fp32"][0]))     # fp32 keeps its own
    from avr.field import FusedField
    assert FusedField(net, "fp16").precision == "fp16"
    with pytest.raises(ValueError):
        FusedField(net, "fp8")


def test_training_step_is_bit_identical_to_x3(golden):
    g = golden("g4_field_small.npz")
    xyz, vd = T(g["xyz"]), T(g["viewdirs"])
    results = {}
    for precision in ("x3", "fp16"):
        net = build_net(g, DEV, precision)
        for p in net.parameters():
            p.requires_grad_(True)
        assert net.can_train_fused(xyz, vd) and not net.can_fuse(xyz)
        loss = ((net(xyz, coarse=True, viewdirs=vd) - 0.5) ** 2).mean() + net(xyz, coarse=False, viewdirs=vd).mean()
        loss.backward()
        torch.cuda.synchronize()
        grads = {k: bits(p.grad) for k, p in net.named_parameters() if p.grad is not None}
        results[precision] = (bits(loss.detach().reshape(1)), grads)
    (l3, g3), (l16, g16) = results["x3"], results["fp16"]
    assert np.array_equal(l3, l16) and g3.keys() == g16.keys() and len(g3) >= 2 * 22
    for k in g3:
        assert np.array_equal(g3[k], g16[k]), k


@pytest.mark.parametrize("tag", ["bn_small", "spade_small", "sp_small", "ns2_small"])
def test_unsupported_nets_stay_on_the_module_path(golden, tag):
    """BatchNorm, use_spade, Softplus and NS = 2 nets under fp16: the module path within the existing golden bar
    (tests/test_gpu_parity.py), the direct FusedField calls raise, and so does t_stop_count = "device"."""
    from avr import _lib
    from avr.renderers import VolumeRenderer
    from avr.scene import INTRINSICS
    g = golden(f"g4_field_{tag}.npz")
    net = build_net(g, DEV, "fp16")
    xyz, vd = T(g["xyz"]), T(g["viewdirs"])
    with torch.no_grad():
        assert not net.can_fuse(xyz) and not net.can_fuse_multiview(xyz)
        np.testing.assert_allclose(to_np(net(xyz, coarse=True, viewdirs=vd)), g["out_coarse"], atol=5e-5, rtol=1e-4)
        np.testing.assert_allclose(to_np(net(xyz, coarse=False, viewdirs=vd)), g["out_fine"], atol=5e-5, rtol=1e-4)
        with pytest.raises((_lib.AVRError, ValueError)):
            net.fused().forward_points(xyz[:1], vd[:1], True)
        if tag != "ns2_small":
            with pytest.raises((_lib.AVRError, ValueError)):
                net.fused().forward_points_scene(xyz[0], vd[0], True)
            with pytest.raises(ValueError):
                net.fused().forward_points_scene_counted(xyz[0].contiguous(), vd[0].contiguous(),
                                                         torch.tensor(5, device=DEV), True)
        R = 64
        x_pix = torch.rand(1, R, 2, generator=torch.Generator(device="cpu").manual_seed(2)).to(DEV)
        c2w = torch.eye(4, device=DEV).reshape(1, 1, 4, 4).expand(1, R, 4, 4).clone()
        c2w[..., 2, 3] = -1.3
        K = torch.tensor([INTRINSICS], device=DEV)
        rend = VolumeRenderer(0.8, 1.8, 16, 8, 0, 0.01, True)
        rend.seed = 5
        _, rgb_f, depth, _ = rend(c2w, K, x_pix, net)
        assert rend.last_path == "module" and torch.isfinite(rgb_f).all() and torch.isfinite(depth).all()
        rend.t_stop, rend.t_stop_count = 0.01, "device"
        with pytest.raises(ValueError):
            rend(c2w, K, x_pix, net)


def test_render_cli_writes_a_frame_under_fp16(tmp_path, capsys):
    import json
    from avr import render
    render.main(["--frames", "1", "--res", "16", "--n-coarse", "32", "--n-fine", "16", "--precision", "fp16",
                 "--sigma-bias", "30", "--warmup", "0", "--out", str(tmp_path)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["precision"] == "fp16" and line["rays_per_frame"] == 256
    data = open(os.path.join(str(tmp_path), "frame_000.ppm"), "rb").read()
    assert data.startswith(b"P6") and len(data) >= 16 * 16 * 3
