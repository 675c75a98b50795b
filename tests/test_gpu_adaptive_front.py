"""avr_adaptive_front (ops.adaptive_front), kernel level: its march against avr_raymarch, its band against
avr_band_fwd, its scene indexing against one-scene calls and its Philox draws against tests/adaptive_ref.py, all
bit for bit except the start distance's Box-Muller (held to tests/test_gpu_philox.py's bar)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_ref  # noqa: E402
from adaptive_scenes import DEV, T, make_avr, scene_inputs, scene_latents_poses, set_scenes  # noqa: E402
from helpers import build_net, to_np  # noqa: E402
from oracle import philox, synth  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 0.05


def _rays(g, R, seed=11):
    """R rays of g6's camera (its own pixels first), start distances and the net / renderer."""
    from avr import ops
    net = build_net(g, DEV, "fp32")
    avr = make_avr(g)
    x = np.concatenate([g["x_pix"][0], synth.hashed_uniform((80, 2), seed) * g["x_pix"].max()], 0)[:R]
    c2w = T(g["c2w_one"]).reshape(1, 1, 4, 4).expand(1, R, 4, 4)
    ro, rd, _ = ops.world_rays(T(x[None].astype(np.float32)), T(g["K"]), c2w)
    init = T((0.8 + synth.hashed_normalish((R,), seed + 1, 0.0625)).astype(np.float32))
    return net, avr, ro[0].contiguous(), rd[0].contiguous(), init


def _front(net, avr, ro, rd, R, steps, n_band, n_scenes=1, first=0, **kw):
    from avr import ops
    views = net.fused().views(range(first, first + n_scenes))
    tables = avr._gate_tables(net, net.encoder.latent.shape[0])[first:first + n_scenes]
    return ops.adaptive_front(views, tables, avr.lstm, avr.out_layer, ro, rd, R, steps, EPS, n_band, **kw)


@pytest.mark.parametrize("R", [1, 3, 48, 65])
def test_march_equals_raymarch(golden, R):
    """One scene, explicit start distances, no band: world is avr_raymarch's bit for bit, over partial 16-lane
    groups' neighbours (R = 1, 3), partial waves, whole and partial blocks (48, 65), and 0, 1, 10 steps."""
    from avr import ops
    g = golden("g6_adaptive.npz")
    net, avr, ro, rd, init = _rays(g, R)
    with torch.no_grad():
        for steps in (0, 1, 10):
            want, _ = ops.raymarch(net.fused().view(0), avr._gate_tables(net, 1)[0], avr.lstm, avr.out_layer, ro, rd,
                                   init, steps)
            world, z = _front(net, avr, ro, rd, R, steps, 0, init_dist=init)
            assert z is None and torch.equal(world, want), (R, steps)
            assert bool(torch.isfinite(world).all())


def _band_fwd(world, ro, rd, u, n):
    from avr import _lib
    R = world.shape[0]
    z = torch.empty(R, n, device=DEV)
    pts = torch.empty(R * n, 3, device=DEV)
    _lib.call("avr_band_fwd", R, n, _lib.ptr(world), _lib.ptr(ro), _lib.ptr(rd), _lib.ptr(u), EPS, _lib.ptr(z),
              _lib.ptr(pts), _lib.stream_of(world))
    return z


@pytest.mark.parametrize("n_band", [1, 7, 20, 64])
def test_band_equals_band_fwd(golden, n_band):
    """z_sorted against avr_band_fwd's z on the same world and noise, bit for bit; the noise sits at 0 and just
    below 1 on alternate samples of half the rays, where rounding swaps stratified neighbours."""
    g = golden("g6_adaptive.npz")
    R = 65
    net, avr, ro, rd, init = _rays(g, R)
    u = synth.hashed_uniform((R, n_band), 21)
    u[::2, 0::2] = 1.0 - 2.0 ** -24
    u[::2, 1::2] = 0.0
    u = T(u)
    with torch.no_grad():
        world, z = _front(net, avr, ro, rd, R, 10, n_band, init_dist=init, band_noise=u)
        want = _band_fwd(world, ro, rd, u, n_band)
    assert bool(torch.isfinite(z).all())
    assert torch.equal(z, want)
    assert bool((z[:, 1:] >= z[:, :-1]).all())


def test_band_keeps_the_nan_row_of_a_ray_without_x_direction(golden):
    """rd_x = 0 (quirk kept, renderers.py:490): that ray's z is NaN as today, its neighbours' are untouched."""
    g = golden("g6_adaptive.npz")
    R, n_band = 6, 20
    net, avr, ro, rd, init = _rays(g, R)
    u = T(synth.hashed_uniform((R, n_band), 22))
    rd2 = rd.clone()
    rd2[2, 0] = 0.0
    with torch.no_grad():
        _, z_ok = _front(net, avr, ro, rd, R, 10, n_band, init_dist=init, band_noise=u)
        world, z = _front(net, avr, ro, rd2, R, 10, n_band, init_dist=init, band_noise=u)
        want = _band_fwd(world, ro, rd2, u, n_band)
    assert bool(torch.isnan(z[2]).all()) and bool(torch.isnan(want[2]).all())
    keep = [0, 1, 3, 4, 5]
    assert torch.equal(z[keep], z_ok[keep]) and torch.equal(z[keep], want[keep])


def test_scene_indexing(golden):
    """Three distinct scenes of 5 rays (scene boundaries inside a wave): the three-scene call equals three
    one-scene calls on the slices bit for bit."""
    from avr import ops
    g = golden("g6_adaptive.npz")
    n, R, n_band = 3, 5, 20
    net = build_net(g, DEV, "fp32")
    avr = make_avr(g)
    set_scenes(net, *scene_latents_poses(g, n))
    c2w, K, x_pix, noise = scene_inputs(g, n, R)
    with torch.no_grad():
        ro, rd, _ = ops.world_rays(x_pix, K, c2w)
        init, band = noise["initial_distance"].reshape(n * R), noise["band"].reshape(n * R, n_band)
        world, z = _front(net, avr, ro, rd, R, 10, n_band, n_scenes=n, init_dist=init, band_noise=band)
        for s in range(n):
            sl = slice(s * R, (s + 1) * R)
            w1, z1 = _front(net, avr, ro[s], rd[s], R, 10, n_band, first=s, init_dist=init[sl], band_noise=band[sl])
            assert torch.equal(world[sl], w1) and torch.equal(z[sl], z1), s
        assert not torch.equal(world[:R], _front(net, avr, ro[0], rd[0], R, 10, n_band, first=1, init_dist=init[:R],
                                                 band_noise=band[:R])[0])   # the scenes do differ


def test_philox_draws(golden):
    """seed 99, offset 1000, ray ids a permutation with gaps, 7 band samples (no multiple of 4): the band noise
    is tests/adaptive_ref.py's bit for bit; the start distance is within 0.05 * 1e-5 (the Box-Muller bar of
    tests/test_gpu_philox.py, scaled by the standard deviation) + 2^-24 (the rounding of the sum near 0.8) of
    it; feeding the draws back as explicit arrays reproduces world and z bit for bit."""
    g = golden("g6_adaptive.npz")
    R, n_band, seed, offset = 13, 7, 99, 1000
    net, avr, ro, rd, _ = _rays(g, R)
    ids = np.array([40, 3, 17, 1000, 5, 0, 64, 63, 2 ** 33 + 1, 12, 11, 500, 7], np.int64)
    with torch.no_grad():
        world, z, init_out, noise_out = _front(net, avr, ro, rd, R, 10, n_band, seed=seed, offset=offset,
                                               ray_ids=T(ids), want_draws=True)
        keys = philox.ray_keys(R, offset, ids.astype(np.uint64))
        assert np.array_equal(to_np(noise_out), adaptive_ref.band_noise(seed, keys, n_band))
        err = float(np.abs(init_out.double().cpu().numpy() - adaptive_ref.init_distance(seed, keys)).max())
        print("start distance max |kernel - float64 reference| =", err)
        assert err <= 0.05 * 1e-5 + 2.0 ** -24
        w2, z2, i2, n2 = _front(net, avr, ro, rd, R, 10, n_band, init_dist=init_out, band_noise=noise_out,
                                want_draws=True)
        assert torch.equal(w2, world) and torch.equal(z2, z)
        assert torch.equal(i2, init_out) and torch.equal(n2, noise_out)   # given draws are handed back
        # without ray ids the key is offset + ray: ray 3 at offset 997 draws what id 1000 at offset 0 draws
        _, _, i3, n3 = _front(net, avr, ro, rd, R, 10, n_band, seed=seed, offset=offset + 997, want_draws=True)
        assert torch.equal(i3[3], init_out[3]) and torch.equal(n3[3], noise_out[3])
