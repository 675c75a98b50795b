"""Full-frame render CLI (the reference's generate_video
harness, utils.py:481-537, on the fused path; BASELINE configs 4 and 5).

    python -m avr.render --frames 4 --res 800 [--t-stop 1e-5] [--out DIR]
    torchrun --nproc-per-node N -m avr.render ...   # rays of every frame sharded over N GPUs
    python -m avr.render --renderer adaptive --n-coarse 20 --philox-seed 3   # in-kernel draws: reproducible frames
    python -m avr.render --occupancy 128 [--occupancy-sigma 0.0]   # skip empty space (avr.occupancy); prints the live share
    python -m avr.render --occupancy 128 --occupancy-refine 4      # the grid built hierarchically: the field only under a live 32^3 grid
    python -m avr.render --occupancy 128 --occupancy-count device  # the same with the live count kept on the device
    python -m avr.render --occupancy 128 --ray-bounds grid         # every ray samples the span of its own occupied cells
    python -m avr.render --t-stop 1e-3 --t-stop-count device [--occupancy 128]   # termination without host reads

Renders `--frames` views on the reference's camera ring (radius, height 0.4)
of the synthetic scene (avr.scene) or of a NewPixelNeRFNet state_dict
(`--weights`, loaded with weights_only=True) and a latent map (`--latent`,
.npy (1, 512, H, W)). Prints one JSON line with rays/s and the fine samples
evaluated; `--out` writes PPM frames. Multi-GPU: every rank renders its
64-ray tiles of each frame and one RCCL all_gather assembles the frame
(avr.parallel.render_sharded); the scene (weights, latent, source view) is
broadcast from rank 0 once before the first frame (avr.parallel.broadcast_scene)."""
import argparse
import json
import os
import time

import numpy as np
import torch


def build_net(args, device):
    from .scene import synthetic_scene
    net = synthetic_scene(device, args.seed, sigma_bias=args.sigma_bias)
    if args.weights:
        sd = torch.load(args.weights, map_location=device, weights_only=True)
        missing, unexpected = net.load_state_dict(sd, strict=False)
        bad = [k for k in missing if not k.startswith("encoder.")]
        if bad or unexpected:
            raise SystemExit(f"--weights: missing {bad[:5]} unexpected {list(unexpected)[:5]}")
    if args.latent:
        lat = torch.from_numpy(np.load(args.latent, allow_pickle=False)).float().to(device)
        net.encoder.set_latent(lat)
    net.field_precision = args.precision
    return net


def adaptive_shard_fn(rend, net):
    """The render_fn avr.parallel.render_sharded takes, for an AdaptiveVolumeRenderer: it passes the frame-wide
    ray ids on (a seeded renderer's draws then match the single-GPU frame) and hands back the fine depth map
    (SB, R) in both depth slots -- the renderer's third output is depth_coarse (SB, R, 1), which the packed
    all_gather has no column for."""
    def render_fn(cam2world, intrinsics, x_pix, ray_ids=None, n_rays_total=None):
        rgb_c, rgb, _, depth_map = rend(cam2world, intrinsics, x_pix, net, ray_ids=ray_ids,
                                        n_rays_total=n_rays_total)
        return rgb_c, rgb, depth_map, depth_map
    return render_fn


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--res", type=int, default=800, help="frame height = width (rays per frame = res^2)")
    ap.add_argument("--radius", type=float, default=1.3)
    ap.add_argument("--n-coarse", type=int, default=128)
    ap.add_argument("--n-fine", type=int, default=64)
    ap.add_argument("--near", type=float, default=0.8)
    ap.add_argument("--far", type=float, default=1.8)
    ap.add_argument("--t-stop", type=float, default=None, help="early ray termination of the fine pass")
    ap.add_argument("--precision", choices=["x3", "fp32", "fp16"], default="x3")
    ap.add_argument("--sigma-bias", type=float, default=0.0, help="synthetic scene: density bias (opacity)")
    ap.add_argument("--weights", default=None, help="NewPixelNeRFNet state_dict (torch.save)")
    ap.add_argument("--latent", default=None, help=".npy latent map (1, 512, H, W)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=1, help="untimed frames first")
    ap.add_argument("--renderer", choices=["volume", "adaptive"], default="volume",
                    help="VolumeRenderer (coarse/fine) or AdaptiveVolumeRenderer (LSTM march + band)")
    ap.add_argument("--raymarch-steps", type=int, default=10)
    ap.add_argument("--epsilon", type=float, default=0.05)
    ap.add_argument("--philox-seed", type=int, default=None,
                    help="adaptive renderer: in-kernel Philox draws with this seed (default: the reference's "
                         "torch draws); a sharded frame then does not depend on the number of ranks")
    ap.add_argument("--occupancy", type=int, default=None, metavar="RES",
                    help="volume renderer: skip empty space with a RES^3 occupancy grid built from the field once "
                         "before the frames (avr.occupancy; RES a multiple of 32, at most 256)")
    ap.add_argument("--occupancy-sigma", type=float, default=0.0, metavar="THR",
                    help="a cell is empty when sigma <= THR at its centre for both MLPs and six view directions "
                         "(default 0.0: exactly zero after the ReLU), before one cell of dilation")
    ap.add_argument("--occupancy-box", type=float, default=1.0, metavar="HALF",
                    help="the grid covers [-HALF, HALF]^3; samples outside it count as empty")
    ap.add_argument("--occupancy-refine", type=int, default=None, metavar="F",
                    help="with --occupancy: build the grid hierarchically (F = 2, 4 or 8): a (RES / F)^3 grid is built "
                         "densely and the field evaluated only at the fine cells under its live cells; what that "
                         "coarse grid calls empty is never looked at again")
    ap.add_argument("--occupancy-probe", type=int, default=None, metavar="P",
                    help="with --occupancy-refine: judge every coarse cell at P^3 interior points (P = 1, 2 or 4; "
                         "default 1: its centre alone) at P^3 times the coarse stage's cost")
    ap.add_argument("--ray-bounds", choices=("grid",), default=None,
                    help="with --occupancy: every ray spreads its samples over the span of its own occupied cells "
                         "instead of [near, far] (avr_occ_ray_bounds; a ray that misses them keeps [near, far])")
    ap.add_argument("--occupancy-count", choices=("host", "device"), default=None,
                    help="with --occupancy: where the live count of a gated pass is kept. host (default): read back "
                         "once per pass to size the launches; device: never read back, worst-case buffers (40 B per "
                         "sample), the live share is read once after the last frame")
    ap.add_argument("--t-stop-count", choices=("host", "device"), default=None,
                    help="with --t-stop: where early termination keeps its counts. host (default): the active-ray "
                         "count is read back after every 64-sample chunk; device: never read back, worst-case buffers "
                         "(40 B per ray and chunk sample), combinable with --occupancy, the evaluated fine samples are "
                         "read once after the last frame")
    ap.add_argument("--out", default=None, help="directory for frame_XXX.ppm")
    args = ap.parse_args(argv)
    from .renderers import check_skip_modes
    from .video import check_refine_modes
    try:   # the counts as given (None: flag not given), so that a count given without its feature is refused too
        flag = lambda n: "--" + n.replace("_", "-")  # noqa: E731
        check_skip_modes("", args.t_stop, args.t_stop_count, args.occupancy, args.occupancy_count, idle=None,
                         name=flag, ray_bounds=args.ray_bounds)
        check_refine_modes("", args.occupancy, args.occupancy_refine, args.occupancy_probe, idle=None, name=flag)
    except ValueError as e:
        ap.error(str(e))
    t_stop_count, occupancy_count = args.t_stop_count or "host", args.occupancy_count or "host"
    if args.renderer != "volume" and (t_stop_count == "device" or args.occupancy is not None):
        ap.error("--t-stop-count device and --occupancy need --renderer volume")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)

    from . import load_library
    from .parallel import render_sharded
    from .renderers import AdaptiveVolumeRenderer, VolumeRenderer
    from .scene import INTRINSICS
    from .video import FrameCounts, get_opencv_pixel_coordinates, orbit_cam2world, to_uint8, write_ppm
    load_library()
    net = build_net(args, device)
    if dist is not None:
        # every rank renders rank 0's scene: weights, latent map and source view from rank 0 (one collective per
        # dtype; the receivers' packed-weight / table caches are invalidated)
        from .parallel import broadcast_scene
        broadcast_scene(net, src=0)
    if args.renderer == "adaptive":
        torch.manual_seed(args.seed + 2)
        rend = AdaptiveVolumeRenderer(net.d_latent, args.raymarch_steps, args.epsilon, args.n_coarse, True).to(device)
        rend.seed = args.philox_seed
        samples_per_ray = args.n_coarse + 1 + args.raymarch_steps   # band + coarse point (+ LSTM lookups)
    else:
        rend = VolumeRenderer(args.near, args.far, args.n_coarse, args.n_fine, 0, 0.01, True)
        rend.seed = 1234
        rend.t_stop = args.t_stop
        rend.t_stop_count = t_stop_count
        samples_per_ray = args.n_coarse + args.n_fine
        if args.occupancy is not None:   # once per scene, before the frames (after the broadcast: every rank's own)
            from .occupancy import OccupancyGrid
            h = args.occupancy_box
            torch.cuda.synchronize()
            t_build = time.perf_counter()
            rend.occupancy = OccupancyGrid.from_field(net, (-h, -h, -h), (h, h, h), (args.occupancy,) * 3,
                                                      sigma_thr=args.occupancy_sigma, refine=args.occupancy_refine,
                                                      coarse_probe=args.occupancy_probe or 1)
            torch.cuda.synchronize()
            occupancy_build_ms = (time.perf_counter() - t_build) * 1e3
            rend.occupancy_count = occupancy_count
            rend.ray_bounds = args.ray_bounds
    K = torch.tensor([INTRINSICS], device=device)
    H = W = args.res
    x_pix = get_opencv_pixel_coordinates(H, W).reshape(1, -1, 2).to(device)
    n = x_pix.shape[1]
    poses = orbit_cam2world(args.frames, args.radius)

    def render(c2w):
        c2w = c2w.to(device).reshape(1, 1, 4, 4).expand(1, n, 4, 4)
        with torch.no_grad():
            if dist is None:
                return rend(c2w, K, x_pix, net)
            if isinstance(rend, VolumeRenderer):   # Philox keyed by frame-wide ray ids
                return render_sharded(lambda c, k, x, **ids: rend(c, k, x, net, **ids), c2w, K, x_pix,
                                      pass_ray_ids=True)
            return render_sharded(adaptive_shard_fn(rend, net), c2w, K, x_pix)

    for i in range(args.warmup):
        render(poses[i % len(poses)])
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    counts = FrameCounts(t_stop_count == "device", args.occupancy is not None and occupancy_count == "device")
    t0 = time.perf_counter()
    frames = []
    for c2w in poses:
        rend.last_fine_samples = 0
        _, rgb_f, _, _ = render(c2w)
        counts.add(rend)
        frames.append(rgb_f)
    torch.cuda.synchronize()
    fine_samples, live_samples = counts.read()   # the one read, after the last frame
    if dist is not None:
        dist.barrier()
    secs = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([secs, float(fine_samples), float(live_samples)], device=device, dtype=torch.float64)
        dist.all_reduce(t[:1], op=dist.ReduceOp.MAX)
        dist.all_reduce(t[1:], op=dist.ReduceOp.SUM)
        secs, fine_samples, live_samples = float(t[0]), int(t[1]), int(t[2])
    if rank == 0:
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            for i, f in enumerate(frames):
                write_ppm(os.path.join(args.out, f"frame_{i:03d}.ppm"), to_uint8(f[0].reshape(H, W, 3).cpu().numpy()))
        total_fine = args.frames * n * (args.n_coarse + args.n_fine)
        line = {"renderer": args.renderer, "samples_per_ray": samples_per_ray,
                "frames": args.frames, "res": args.res, "rays_per_frame": n, "n_gpus": world,
                "seconds": round(secs, 4), "rays_per_s": round(args.frames * n / secs, 1),
                "t_stop": args.t_stop, "t_stop_count": t_stop_count, "precision": args.precision,
                "sigma_bias": args.sigma_bias,
                "fine_samples_evaluated": fine_samples,
                "fine_samples_fraction": round(fine_samples / total_fine, 4)}
        if args.occupancy is not None:
            # the live share: field samples evaluated over both passes' n_coarse + (n_coarse + n_fine) per ray
            line.update({"occupancy": args.occupancy, "occupancy_sigma": args.occupancy_sigma,
                         "occupancy_count": occupancy_count, "occupancy_refine": args.occupancy_refine,
                         "ray_bounds": args.ray_bounds,
                         "occupancy_build_evals": rend.occupancy.build_evals,
                         "occupancy_build_ms": round(occupancy_build_ms, 3),
                         "occupancy_cells_set": round(rend.occupancy.live_fraction(), 4),
                         "live_samples_fraction": round(live_samples / (args.frames * n * (2 * args.n_coarse
                                                                                          + args.n_fine)), 4)})
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
