"""AdaptiveVolumeRenderer / Raymarcher inference through avr_adaptive_front, renderer level: several scenes per
call against the golden run and against one-scene calls of the unseeded one-scene path, the Philox seed (explicit
draws, offsets, frame-wide ray ids), HIP-graph replay, and the render CLI's seeded and sharded branches."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from adaptive_scenes import (DEV, T, g6_inputs, make_avr, scene_inputs, scene_latents_poses,  # noqa: E402
                             set_scenes)
from helpers import build_net, to_np  # noqa: E402
from oracle import synth  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("rgb_coarse", "rgb", "depth_coarse", "depth")


def _one_scene_calls(avr, net, lat, poses, inputs, scenes):
    """Scene s rendered alone by the unseeded one-scene path (today's kernel chain) with its own noise."""
    c2w, K, x_pix, noise = inputs
    out = {}
    for s in scenes:
        set_scenes(net, lat[s:s + 1], poses[s:s + 1])
        one = avr(c2w[s:s + 1], K[s:s + 1], x_pix[s:s + 1], net, noise={k: v[s:s + 1] for k, v in noise.items()})
        assert avr.last_path == "fused"
        out[s] = one
    return out


def _compare(both, ones, label):
    """depth_coarse bit-equal (march, tables and depth involve no batched field launch); rgb_coarse, rgb, depth
    within 1e-4. Prints the largest difference per output."""
    worst = dict.fromkeys(NAMES, 0.0)
    for s, one in ones.items():
        for name, a, b in zip(NAMES, both, one):
            if a is None:
                assert b is None
                continue
            d = float((a[s:s + 1] - b).abs().max())
            worst[name] = max(worst[name], d)
            if name == "depth_coarse":
                assert torch.equal(a[s:s + 1], b), (label, s, d)
            else:
                assert d <= 1e-4, (label, s, name, d)
    print(label, "max |multi-scene - one-scene|:", worst)


@pytest.mark.parametrize("precision", ["x3", "fp32"])
def test_multi_scene_matches_golden_and_one_scene_calls(golden, precision):
    g = golden("g6_adaptive.npz")
    net = build_net(g, DEV, precision)
    avr = make_avr(g)
    n, R = 3, g["x_pix"].shape[1]
    lat, poses = scene_latents_poses(g, n)
    inputs = scene_inputs(g, n, R)
    with torch.no_grad():
        set_scenes(net, lat, poses)
        both = avr(*inputs[:3], net, noise=inputs[3])
        assert avr.last_path == "fused"
        for name, t in zip(NAMES, both):   # scene 0 is the golden run's scene and inputs
            np.testing.assert_allclose(to_np(t[0]), g[name][0], atol=1e-4, err_msg=name)
        assert all(bool(torch.isfinite(t).all()) for t in both)
        _compare(both, _one_scene_calls(avr, net, lat, poses, inputs, range(n)), f"SB=3 {precision}")


@pytest.mark.parametrize("precision", ["x3", "fp32"])
def test_seventeen_scenes_two_launch_groups(golden, precision):
    g = golden("g6_adaptive.npz")
    net = build_net(g, DEV, precision)
    avr = make_avr(g)
    n, R = 17, 3
    lat, poses = scene_latents_poses(g, n)
    inputs = scene_inputs(g, n, R)
    with torch.no_grad():
        set_scenes(net, lat, poses)
        both = avr(*inputs[:3], net, noise=inputs[3])
        assert avr.last_path == "fused" and both[0].shape == (n, R, 3) and both[3].shape == (n, R)
        assert all(bool(torch.isfinite(t).all()) for t in both)
        _compare(both, _one_scene_calls(avr, net, lat, poses, inputs, [0, 15, 16]), f"SB=17 {precision}")


def test_raymarcher_multi_scene(golden):
    g = golden("g6_adaptive.npz")
    net = build_net(g, DEV, "x3")
    rm = make_avr(g, "Raymarcher")
    n, R = 3, g["x_pix"].shape[1]
    lat, poses = scene_latents_poses(g, n)
    inputs = scene_inputs(g, n, R)
    with torch.no_grad():
        set_scenes(net, lat, poses)
        both = rm(*inputs[:3], net, noise=inputs[3])
        assert rm.last_path == "fused" and both[1] is None and both[2] is both[3]
        np.testing.assert_allclose(to_np(both[0][0]), g["rgb_coarse"][0], atol=1e-4)
        np.testing.assert_allclose(to_np(both[2][0]), g["depth_coarse"][0], atol=1e-4)
        ones = _one_scene_calls(rm, net, lat, poses, inputs, range(n))
        worst = 0.0
        for s, one in ones.items():
            assert one[1] is None
            assert torch.equal(both[2][s:s + 1], one[2]), s          # depth of the marched points
            worst = max(worst, float((both[0][s:s + 1] - one[0]).abs().max()))
        print("Raymarcher SB=3 max rgb |multi-scene - one-scene| =", worst)
        assert worst <= 1e-4


def test_seeded_call_equals_explicit_noise(golden):
    from avr import ops
    g = golden("g6_adaptive.npz")
    net = build_net(g, DEV, "x3")
    avr = make_avr(g)
    n, R, nb = 2, g["x_pix"].shape[1], int(g["n_coarse"])
    set_scenes(net, *scene_latents_poses(g, n))
    c2w, K, x_pix, _ = scene_inputs(g, n, R)
    avr.seed = 5
    with torch.no_grad():
        avr._offset = 640
        first = avr(c2w, K, x_pix, net)
        assert avr.last_path == "fused" and avr._offset == 640 + n * R
        second = avr(c2w, K, x_pix, net)
        assert avr._offset == 640 + 2 * n * R
        assert not torch.equal(first[1], second[1]) and not torch.equal(first[2], second[2])
        avr._offset = 640
        again = avr(c2w, K, x_pix, net)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
        # the draws of the first call, read through the kernel at the same offset, given back as explicit noise
        ro, rd, _ = ops.world_rays(x_pix, K, c2w)
        _, _, init, band = ops.adaptive_front(net.fused().views(range(n)), avr._gate_tables(net, n), avr.lstm,
                                              avr.out_layer, ro, rd, R, avr.steps, avr.epsilon, nb, seed=5,
                                              offset=640, want_draws=True)
        avr._offset = 640
        explicit = avr(c2w, K, x_pix, net, noise={"initial_distance": init.reshape(n, R, 1),
                                                  "band": band.reshape(n, R, nb)})
        assert avr.last_path == "fused"
        assert all(torch.equal(a, b) for a, b in zip(first, explicit))
        assert float((init - 0.8).abs().max()) < 6 * 0.05 and 0.0 <= float(band.min()) and float(band.max()) < 1.0


def test_sharded_frame_equals_full_frame(golden):
    """130 rays, one scene, seeded: the two ranks' shares (64-ray tiles, frame-wide ray ids) reassemble to the
    full frame bit for bit."""
    from avr.parallel import ray_tiles
    g = golden("g6_adaptive.npz")
    net = build_net(g, DEV, "x3")
    avr = make_avr(g)
    avr.seed = 8
    R = 130
    x_pix = T((synth.hashed_uniform((1, R, 2), 41) * g["x_pix"].max()).astype(np.float32))
    c2w = T(g["c2w_one"]).reshape(1, 1, 4, 4).expand(1, R, 4, 4)
    K = T(g["K"])
    with torch.no_grad():
        avr._offset = 77
        full = avr(c2w, K, x_pix, net)
        assert avr.last_path == "fused" and avr._offset == 77 + R
        parts = [torch.empty_like(t) for t in full]
        for rank in range(2):
            idx = ray_tiles(R, rank, 2, device=DEV)
            avr._offset = 77
            share = avr(c2w[:, idx], K, x_pix[:, idx].contiguous(), net, ray_ids=idx, n_rays_total=R)
            assert avr._offset == 77 + R                     # a share advances by the whole frame
            for p, t in zip(parts, share):
                p[:, idx] = t
    for name, a, b in zip(NAMES, full, parts):
        assert torch.equal(a, b), name


def _graph_scene(R, seed):
    from avr.renderers import AdaptiveVolumeRenderer
    from avr.scene import INTRINSICS, synthetic_scene
    net = synthetic_scene(DEV, 0, latent_hw=(16, 16))
    gen = torch.Generator(device="cpu").manual_seed(seed)
    x_pix = torch.rand(1, R, 2, generator=gen).to(DEV)
    c2w = torch.eye(4).reshape(1, 1, 4, 4).repeat(1, R, 1, 1)
    c2w[..., 2, 3] = -1.3 - 0.2 * torch.rand(1, R, generator=gen)
    K = torch.tensor([INTRINSICS], device=DEV)
    torch.manual_seed(2)
    rend = AdaptiveVolumeRenderer(net.d_latent, 10, 0.05, 20, True).to(DEV)
    return net, rend, c2w.to(DEV), K, x_pix


def test_graph_replay_equals_eager():
    from avr.graphs import GraphedRenderer
    net, rend, c2w, K, x_pix = _graph_scene(1000, 1)
    rend.seed = 77
    gr = GraphedRenderer(rend, net, c2w, K, x_pix)   # the capture succeeds: no host read, no host draw

    def check():
        for seed in (2, 3):
            _, _, c2w2, _, x2 = _graph_scene(1000, seed)
            got = [t.clone() for t in gr(c2w2, K, x2)]
            rend._offset = gr.offset
            with torch.no_grad():
                want = rend(c2w2, K, x2, net)
            assert rend.last_path == "fused"
            for a, b in zip(got, want):
                assert torch.equal(a, b)
        return got

    before = check()
    assert gr.captures == 1
    with torch.no_grad():
        rend.lstm.weight_ih.mul_(1.25)            # the gate table baked into the captured launches is stale now
    after = check()
    assert gr.captures == 2
    assert not torch.equal(before[1], after[1])
    # a warm eager seeded call reads no device memory on the host
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            out = rend(c2w, K, x_pix, net)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert all(bool(torch.isfinite(t).all()) for t in out)


def test_graph_refuses_the_host_draw():
    from avr.graphs import GraphedRenderer
    net, rend, c2w, K, x_pix = _graph_scene(64, 1)
    with pytest.raises(ValueError, match="seed"):
        GraphedRenderer(rend, net, c2w, K, x_pix)


def test_cli_philox_seed_is_reproducible(tmp_path, capsys):
    from avr import render
    frames = []
    for run in ("a", "b"):
        out = str(tmp_path / run)
        render.main(["--renderer", "adaptive", "--philox-seed", "3", "--res", "32", "--frames", "1", "--warmup", "0",
                     "--n-coarse", "20", "--out", out])
        frames.append(open(os.path.join(out, "frame_000.ppm"), "rb").read())
    capsys.readouterr()
    assert len(frames[0]) > 32 * 32 * 3 and frames[0] == frames[1]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture
def nccl_world1():
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
    try:
        yield dist
    finally:
        dist.destroy_process_group()


def test_cli_sharded_adaptor_through_render_sharded(golden, nccl_world1):
    """avr.render's adaptor for the sharded branch, through render_sharded on a one-rank RCCL group: full-frame
    outputs equal to the direct seeded call (the renderer's own third output, depth_coarse (SB, R, 1), does not
    fit render_sharded's packed depth column)."""
    from avr.parallel import render_sharded
    from avr.render import adaptive_shard_fn
    g = golden("g6_adaptive.npz")
    net = build_net(g, DEV, "x3")
    avr = make_avr(g)
    avr.seed = 3
    R = 130
    x_pix = T((synth.hashed_uniform((1, R, 2), 43) * g["x_pix"].max()).astype(np.float32))
    c2w = T(g["c2w_one"]).reshape(1, 1, 4, 4).expand(1, R, 4, 4)
    K = T(g["K"])
    with torch.no_grad():
        rgb_c, rgb, _, depth = avr(c2w, K, x_pix, net)
        avr._offset = 0
        got = render_sharded(adaptive_shard_fn(avr, net), c2w, K, x_pix)
    assert avr._offset == R
    assert torch.equal(got[0], rgb_c) and torch.equal(got[1], rgb)
    assert torch.equal(got[2], depth) and got[2].shape == (1, R) and got[3] is got[2]
