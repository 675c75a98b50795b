"""Per-ray sampling bounds from the occupancy grid (VolumeRenderer.ray_bounds = "grid", avr_occ_ray_bounds) against
the gated frame without them, in one process, legs alternating, so the run-to-run spread is measured with the
difference (the protocol of scripts/field_fp16_ab.py).

    python scripts/ray_bounds_ab.py [--rays 65536 4096] [--rounds 3] [--window 0.5] [--res 128] [--radius 0.35]
                                    [--sigma-bias 0]

Shape: a square frame of --rays rays on avr.scene.synthetic_scene, x3, under the sphere grid of scripts/occupancy_ab.py
(cells whose centre lies within --radius of the origin of [-1, 1]^3), occupancy_count = "device". Records per ray count:
  bounds   the avr_occ_ray_bounds launch alone against the gated frame at 128 + 64 without bounds, with the launch's
           share of that frame;
  frame    the gated frame at 128 + 64 without and with bounds: ms, the live samples per pass (last_live_counts) and
           the time per live sample;
  quality  an ungated frame at 256 + 128 as the yardstick (and a gated one without bounds at 170 + 86, the most the
           gated chain takes per ray, as a second one: the first also holds what the grid cuts away); then gated frames
           without and with bounds at 128 + 64, 64 + 32 and 32 + 16: ms and PSNR (avr.metrics) of the fine frame against
           each yardstick, same seed.
--sigma-bias B is synthetic_scene's: 0 is the thin fog of a random-init field, in which a ray still carries most of
its transmittance when it leaves the grid's cells; 30 makes rays saturate inside them, as on a scene with surfaces.
The difference matters to the picture: the composite gives a ray's last sample an unbounded extent (1e10), and with
bounds that sample lies inside the occupied span, where it is live, instead of at `far`, where the grid calls it dead.
Every timed window is HIP events around enough calls to last --window seconds, after warm-up calls of the same leg; a
leg's figure is ms per call: median, min and spread ((max - min) / median) over the rounds. One JSON line per record."""
import argparse
import json
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "adaptive-volume-rendering_amd"), REPO):
    sys.path.insert(0, p)

from avr import ops  # noqa: E402
from avr.metrics import image_metrics  # noqa: E402
from avr.occupancy import OccupancyGrid  # noqa: E402
from avr.renderers import VolumeRenderer  # noqa: E402
from avr.scene import INTRINSICS, synthetic_scene  # noqa: E402
from avr.video import get_opencv_pixel_coordinates, orbit_cam2world  # noqa: E402

DEV = torch.device("cuda:0")
NEAR, FAR = 0.8, 1.8
SETTINGS = ((128, 64), (64, 32), (32, 16))


def sphere_grid(res, radius):
    ax = torch.linspace(-1 + 1 / res, 1 - 1 / res, res, dtype=torch.float64)
    zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
    sigma = ((xx * xx + yy * yy + zz * zz) <= radius * radius).to(torch.float32).to(DEV)
    return OccupancyGrid.from_sigma(sigma, (-1, -1, -1), (1, 1, 1), 0.0, dilate=0)


def ms_per_call(fn, window):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(2):
        fn()
    b.record()
    torch.cuda.synchronize()
    n = max(2, int(window * 1e3 / max(a.elapsed_time(b) / 2, 1e-3)) + 1)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def summary(ts):
    s = sorted(ts)
    med = s[len(s) // 2]
    return {"ms": round(med, 4), "min_ms": round(s[0], 4), "spread": round((s[-1] - s[0]) / med, 4)}


def alternate(legs, rounds, window):
    for fn in legs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(ms_per_call(fn, window))
    return {k: summary(ts) for k, ts in times.items()}


def camera(side):
    x_pix = get_opencv_pixel_coordinates(side, side).reshape(1, -1, 2).to(DEV)
    R = x_pix.shape[1]
    c2w = orbit_cam2world(8, 1.3)[1].to(DEV).reshape(1, 1, 4, 4).expand(1, R, 4, 4).contiguous()
    return x_pix, c2w, torch.tensor([INTRINSICS], device=DEV)


def renderer(nc, nf, grid=None, bounds=None):
    rend = VolumeRenderer(NEAR, FAR, nc, nf, 0, 0.01, True)
    rend.seed = 1234
    if grid is not None:
        rend.occupancy, rend.occupancy_count, rend.ray_bounds = grid, "device", bounds
    return rend


def frame_of(rend, cam, net):
    x_pix, c2w, K = cam
    rend._offset = 0
    return rend(c2w, K, x_pix, net)[1]


def psnr(img, gt, side):
    v = float(image_metrics(img, gt, side, side)[0][0])
    return None if math.isinf(v) else round(v, 3)


def records(net, grid, side, args):
    cam = camera(side)
    x_pix, c2w, K = cam
    R = side * side
    base = {"rays": R, "grid": f"{args.res}^3 sphere, radius {args.radius}, occupancy_count device", "precision": "x3",
            "sigma_bias": args.sigma_bias, "rounds": args.rounds, "window_s": args.window}
    ro, rd, _ = ops.world_rays(x_pix, K, c2w)
    plain, bounded = renderer(128, 64, grid), renderer(128, 64, grid, "grid")
    # the bounds launch alone, beside the frame it would be added to
    out = alternate({"bounds_launch": lambda: grid.ray_bounds(ro[0], rd[0], NEAR, FAR),
                     "gated_frame": lambda: plain(c2w, K, x_pix, net)}, args.rounds, args.window)
    tn, tf = grid.ray_bounds(ro[0], rd[0], NEAR, FAR)
    cut = (tn > NEAR) | (tf < FAR)
    rec = dict(base, record="bounds", walk="single level", **out)
    rec["launch_share_of_frame"] = round(out["bounds_launch"]["ms"] / out["gated_frame"]["ms"], 5)
    rec["rays_bounded"] = round(float(cut.float().mean()), 4)
    rec["mean_span_of_bounded_rays"] = round(float(((tf - tn)[cut]).mean() / (FAR - NEAR)), 4) if bool(cut.any()) else None
    print(json.dumps(rec), flush=True)
    # frames at 128 + 64
    out = alternate({"gated": lambda: plain(c2w, K, x_pix, net), "gated_bounded": lambda: bounded(c2w, K, x_pix, net)},
                    args.rounds, args.window)
    rec = dict(base, record="frame", samples="128 + 64", **out)
    for k, r in (("gated", plain), ("gated_bounded", bounded)):
        live = [int(v) for v in r.last_live_counts.tolist()]
        rec[k].update(live_coarse=live[0], live_fine=live[1],
                      ns_per_live_sample=round(rec[k]["ms"] * 1e6 / max(sum(live), 1), 3))
    rec["bounded_over_gated_ms"] = round(out["gated_bounded"]["ms"] / out["gated"]["ms"], 4)
    rec["slower_beyond_spread"] = bool(
        out["gated_bounded"]["ms"] - out["gated"]["ms"]
        > out["gated"]["spread"] * out["gated"]["ms"] + out["gated_bounded"]["spread"] * out["gated_bounded"]["ms"])
    print(json.dumps(rec), flush=True)
    # equal quality: PSNR of the fine frame against the yardsticks, same seed
    yard = {"ungated_256+128": frame_of(renderer(256, 128), cam, net),
            "gated_170+86": frame_of(renderer(170, 86, grid), cam, net)}
    rends = {}
    for nc, nf in SETTINGS:
        rends[f"gated_{nc}+{nf}"] = renderer(nc, nf, grid)
        rends[f"bounded_{nc}+{nf}"] = renderer(nc, nf, grid, "grid")
    out = alternate({k: (lambda r=r: r(c2w, K, x_pix, net)) for k, r in rends.items()}, args.rounds, args.window)
    rec = dict(base, record="quality", **out)
    for k, r in rends.items():
        img = frame_of(r, cam, net)
        rec[k].update({f"psnr_vs_{y}": psnr(img, gt, side) for y, gt in yard.items()})
    ref_ms = out["gated_128+64"]["ms"]
    for y in yard:
        ref_psnr = rec["gated_128+64"][f"psnr_vs_{y}"]
        match = [k for k in rends if k.startswith("bounded") and (rec[k][f"psnr_vs_{y}"] or math.inf) >= ref_psnr]
        best = min(match, key=lambda k: out[k]["ms"]) if match else None
        rec[f"cheapest_bounded_matching_gated_128+64_vs_{y}"] = best
        rec[f"its_time_ratio_vs_{y}"] = round(out[best]["ms"] / ref_ms, 4) if best else None
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rays", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window (at least)")
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--radius", type=float, default=0.35)
    ap.add_argument("--sigma-bias", type=float, default=0.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    assert args.rounds >= 3 and args.window >= 0.5, "at least 3 rounds of windows of at least 0.5 s"
    net = synthetic_scene(DEV, 0, sigma_bias=args.sigma_bias)
    grid = sphere_grid(args.res, args.radius)
    with torch.no_grad():
        for R in args.rays:
            side = int(round(math.sqrt(R)))
            assert side * side == R, "a square frame"
            records(net, grid, side, args)


if __name__ == "__main__":
    main()
