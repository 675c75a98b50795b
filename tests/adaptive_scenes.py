"""Shared by the adaptive-inference GPU tests (test infrastructure only): the g6_adaptive.npz renderer and inputs
(as tests/test_gpu_adaptive.py builds them) and further scenes with the same weights -- scene s has the g6 latent
rolled by s texels along W and the world->camera pose of an orbit camera, scene 0 is g6's own."""
import numpy as np
import torch

from oracle import synth

DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def T(a):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a)), device=DEV)


def make_avr(g, cls="AdaptiveVolumeRenderer"):
    from avr import renderers
    if cls == "Raymarcher":
        m = renderers.Raymarcher(int(g["d_latent"]), int(g["steps"]))
    else:
        m = renderers.AdaptiveVolumeRenderer(int(g["d_latent"]), int(g["steps"]), float(g["epsilon"]),
                                             int(g["n_coarse"]), True)
    sd = {k[len("lstm_"):]: torch.from_numpy(g[k]) for k in g if k.startswith("lstm_")}
    m.lstm.load_state_dict(sd)
    m.out_layer.weight.data = torch.from_numpy(g["out_w"])
    m.out_layer.bias.data = torch.from_numpy(g["out_b"])
    return m.to(DEV)


def g6_inputs(g):
    R = g["x_pix"].shape[1]
    c2w = T(g["c2w_one"]).reshape(1, 1, 4, 4).expand(1, R, 4, 4)
    noise = {"initial_distance": T(g["init_dist"]), "band": T(g["band_noise"])}
    return c2w, T(g["K"]), T(g["x_pix"]), noise


def scene_latents_poses(g, n):
    """latent (n, C, H, W) and world->camera poses (n, 3, 4): scene 0 is the fixture's."""
    lat = np.concatenate([np.roll(g["latent"], s, axis=-1) for s in range(n)], 0)
    poses = [g["poses"][0]]
    for s in range(1, n):
        poses.append(np.linalg.inv(synth.orbit_cam2world(0.2 * s).astype(np.float64))[:3].astype(np.float32))
    return np.ascontiguousarray(lat), np.stack(poses)


def set_scenes(net, lat, poses):
    """Point `net` at these scenes (new tensors: the caches keyed by address and version rebuild)."""
    net.encoder.latent = T(lat)
    net.poses = T(poses)


def scene_inputs(g, n, R):
    """Cameras, pixels and explicit noise of n scenes of R rays: scene 0 takes g6's first R rays and draws."""
    n_band = int(g["n_coarse"])
    x = np.concatenate([g["x_pix"][:, :R]] + [synth.hashed_uniform((1, R, 2), 100 + s) * g["x_pix"].max()
                                              for s in range(1, n)], 0).astype(np.float32)
    c2w = np.stack([g["c2w_one"]] + [synth.orbit_cam2world(0.7 * s) for s in range(1, n)])
    init = np.concatenate([g["init_dist"][:, :R]] + [0.8 + synth.hashed_normalish((1, R, 1), 200 + s, 0.0625)
                                                     for s in range(1, n)], 0).astype(np.float32)
    band = np.concatenate([g["band_noise"][:, :R]] + [synth.hashed_uniform((1, R, n_band), 300 + s)
                                                      for s in range(1, n)], 0).astype(np.float32)
    c2w_t = T(c2w).reshape(n, 1, 4, 4).expand(n, R, 4, 4)
    K = T(g["K"]).expand(n, 3, 3)
    return c2w_t, K, T(x), {"initial_distance": T(init), "band": T(band)}
