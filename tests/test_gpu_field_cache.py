"""FusedField's cache bookkeeping on the MI355X: no call leaves a cached blob's dims describing another precision
than the blob was packed for (every library call is given a _Packed.dims_as copy), and the training paths' shared
latent lookup (avr.train_common.lookup_features) gives the per-scene launch's rows bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
B = 64


def _net(sb):
    """d_hidden 64, 2 blocks, d_latent 64, an 8 x 8 latent map; sb scenes, each with its own map and pose."""
    from avr.conf import Conf, default_conf
    from avr.scene import synthetic_scene
    d = dict(default_conf()["model"])
    mlp = {"type": "resnet", "n_blocks": 2, "d_hidden": 64, "combine_layer": 1000, "beta": 0.0, "use_spade": False,
           "combine_type": "average"}
    d["mlp_coarse"], d["mlp_fine"] = dict(mlp), dict(mlp)
    d["encoder"] = {"backbone": "resnet34", "pretrained": False, "num_layers": 1}
    net = synthetic_scene(DEV, 0, Conf(d), latent_hw=(8, 8))
    g = torch.Generator(device="cpu").manual_seed(7)
    net.encoder.set_latent(torch.randn(sb, 64, 8, 8, generator=g).to(DEV))
    net.num_objs = sb
    poses = net.poses.repeat(sb, 1, 1)
    poses[:, 0, 3] += 0.1 * torch.arange(sb, device=DEV, dtype=torch.float32)
    net.poses = poses
    net.focal, net.c = net.focal.repeat(sb, 1), net.c.repeat(sb, 1)
    return net


def _points(sb, seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    xyz = (torch.rand(sb, B, 3, generator=g) - 0.5) * 0.8
    vd = torch.nn.functional.normalize(torch.randn(sb, B, 3, generator=g), dim=-1)
    return xyz.to(DEV), vd.to(DEV)


@pytest.mark.parametrize("precision", ["x3", "fp32"])
def test_cached_dims_are_never_left_mutated(precision):
    from avr.field import PRECISIONS, FusedField
    net = _net(2)
    fused = FusedField(net, precision)
    xyz, vd = _points(2)
    entry = fused.packed(True)
    snap = bytes(entry.dims)
    assert entry.dims.precision == PRECISIONS[precision]
    z = torch.linspace(0.8, 1.8, 8, device=DEV).repeat(B, 1)

    def train_step():
        x = xyz.clone().requires_grad_(True)
        fused.forward_train(x, vd, True).sum().backward()
        assert x.grad is not None and bool(torch.isfinite(x.grad).all())

    steps = [("forward_points SB=1", lambda: fused.forward_points(xyz[:1], vd[:1], True)),
             ("forward_points SB=2", lambda: fused.forward_points(xyz, vd, True)),
             ("forward_rays", lambda: fused.forward_rays(xyz[0], vd[0], z, True)),
             ("table", lambda: fused.table(True, 1)),
             ("tables_batch fast", lambda: fused.tables_batch(True, 2, fast=True))]
    if precision == "x3":
        steps.append(("forward_train + backward", train_step))
    for name, step in steps:
        step()
        again = fused.packed(True)
        assert again is entry, f"{name}: the blob was repacked"
        assert bytes(again.dims) == snap, f"{name}: left the cached dims changed"
    torch.cuda.synchronize()


@pytest.mark.parametrize("shared_map", [False, True], ids=["own-maps", "shared-map"])
def test_lookup_features_matches_the_per_scene_launch_bit_for_bit(shared_map, monkeypatch):
    """Three scenes with a map each: one avr_latent_features_batch launch; three scenes sharing one map: the
    per-scene path. Both against avr_latent_features scene by scene (avr.ops.latent_features)."""
    from avr import _lib, ops, train_common
    from avr.field import FusedField
    SB = 3
    net = _net(SB)
    if shared_map:
        net.encoder.set_latent(net.encoder.latent[:1].contiguous())
    fused = FusedField(net, "x3")
    lat = net.encoder.latent.detach()
    xyz, _ = _points(SB, seed=5)
    ref = torch.cat([ops.latent_features(fused.view(s), lat[min(s, lat.shape[0] - 1)], xyz[s]) for s in range(SB)])
    launches = []
    real = _lib.call
    monkeypatch.setattr(train_common, "call", lambda name, *a: launches.append(name) or real(name, *a))
    got = train_common.lookup_features(fused, lat, xyz.contiguous(), SB, B)
    assert got.shape == (SB * B, 64) and torch.equal(got, ref)
    assert launches == ([] if shared_map else ["avr_latent_features_batch"])   # (per scene: through avr.ops)


def test_a_value_cached_on_a_side_stream_inside_a_capture_is_ordered_before_its_reader():
    """The captured adaptive step's pattern (avr.renderers: the coarse backward fills FusedField._latent_cache on
    the graph's side stream, the band backward reads it on the capturing stream), in small: inside a capture
    scope the side stream runs a few milliseconds of GEMMs and then fills a record; the capturing stream's hit of
    that record must become a graph edge, so every replay copies this replay's value, not the one before."""
    from avr.cache import _cached, capture_scope
    n = 64 * 1024
    src, out = torch.zeros(n, device=DEV), torch.full((n,), -1.0, device=DEV)
    a = torch.full((2048, 2048), 1.0 / 2048, device=DEV)
    b, c = torch.ones(2048, 2048, device=DEV), torch.empty(2048, 2048, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    store, made = {}, []

    def make():
        made.append(1)
        return src * 2

    def delay():   # 24 x 17 GFLOP of fp32 GEMM: a few milliseconds, no allocation
        for _ in range(12):
            torch.mm(a, b, out=c)
            torch.mm(a, c, out=b)

    delay()        # (the GEMM library's first call, outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with capture_scope(), torch.cuda.graph(graph):
        main = torch.cuda.current_stream()
        fork = torch.cuda.Event()
        fork.record(main)
        side.wait_event(fork)
        with torch.cuda.stream(side):
            delay()
            value = _cached(store, "slot", "key", make)
        assert _cached(store, "slot", "key", make) is value and made == [1]   # a hit, on the capturing stream
        out.copy_(value)
        main.wait_stream(side)
    for fill in (1.0, 2.0, 3.0):
        src.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        assert bool((out == 2 * fill).all()), (fill, out[:4].tolist())
    assert made == [1] and bool((b == 1).all())
