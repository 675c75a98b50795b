"""Early termination with its counts on the device (renderer.t_stop_count = "device") against the host-read chain,
alone and on top of an occupancy grid, in one process, legs alternating, so the run-to-run spread is measured with
the difference (the protocol of scripts/occupancy_count_ab.py, whose helpers this script uses).

    python scripts/march_device_ab.py [--rays 65536 4096] [--t-stop 1e-3] [--sigma-bias 30] [--rounds 3] [--window 0.5]

Shape: --rays rays x (128 + 64) samples, x3, avr.scene.synthetic_scene with its density biased up by --sigma-bias (a
scene opaque enough that termination bites), the synthetic sphere grid of scripts/occupancy_ab.py. Legs per ray
count:
  stop_host               t_stop, t_stop_count = "host": ops.march_fine, the yardstick;
  stop_device             t_stop, t_stop_count = "device", eager;
  stop_device_graph       the same renderer replayed from avr.graphs.GraphedRenderer;
  grid_device             the sphere grid alone, occupancy_count = "device": the second yardstick;
  grid_stop_device        the grid and device-side t_stop, eager;
  grid_stop_device_graph  the same renderer replayed.
A leg's figure is ms per frame (HIP events around enough frames to last --window seconds, after warm-up frames of the
same leg); one JSON line per ray count with median, min and spread per leg, the fine samples each leg evaluated and
the share termination removed (of all fine samples without a grid, of the grid's live fine samples with one)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from occupancy_count_ab import DEV, NC, NF, alternate, sphere_grid  # noqa: E402  (puts the package on sys.path)

from avr.graphs import GraphedRenderer  # noqa: E402
from avr.renderers import VolumeRenderer  # noqa: E402
from avr.scene import INTRINSICS, synthetic_scene  # noqa: E402
from avr.video import orbit_cam2world  # noqa: E402


def frame_legs(net, grid, R, args):
    x_pix = torch.rand(1, R, 2, generator=torch.Generator().manual_seed(100)).to(DEV)
    c2w = orbit_cam2world(8, 1.3)[1].to(DEV).reshape(1, 1, 4, 4).expand(1, R, 4, 4).contiguous()
    K = torch.tensor([INTRINSICS], device=DEV)
    spec = {"stop_host": (None, args.t_stop, "host"), "stop_device": (None, args.t_stop, "device"),
            "stop_device_graph": (None, args.t_stop, "device"), "grid_device": (grid, None, "host"),
            "grid_stop_device": (grid, args.t_stop, "device"), "grid_stop_device_graph": (grid, args.t_stop, "device")}
    rends = {}
    for k, (g, t_stop, mode) in spec.items():
        r = rends[k] = VolumeRenderer(0.8, 1.8, NC, NF, 0, 0.01, True)
        r.seed, r.occupancy, r.occupancy_count, r.t_stop, r.t_stop_count = 1234, g, "device", t_stop, mode
    legs, graphs = {}, {}
    for k, r in rends.items():
        if k.endswith("_graph"):
            legs[k] = graphs[k] = GraphedRenderer(r, net, c2w, K, x_pix)
        else:
            legs[k] = lambda r=r: r(c2w, K, x_pix, net)
    out = {"shape": f"{R} rays x ({NC} + {NF}), x3, synthetic scene, sigma bias {args.sigma_bias}",
           "t_stop": args.t_stop, "rounds": args.rounds, "window_s": args.window,
           "grid": f"{args.res}^3 sphere, radius {args.radius}", "cells_set": round(grid.live_fraction(), 4)}
    out.update(alternate(legs, args.rounds, args.window))
    fine_all = R * (NC + NF)
    fine_grid = int(rends["grid_device"].last_live_counts[1].item())
    out["stop_host"]["fine_samples"] = rends["stop_host"].last_fine_samples
    out["grid_device"]["fine_samples"] = fine_grid
    for k in spec:
        if "stop_device" in k:
            out[k]["fine_samples"] = int(rends[k].last_fine_counts.item())
    for k in spec:
        if k != "grid_device":
            base = fine_grid if k.startswith("grid") else fine_all
            out[k]["removed_share"] = round(1.0 - out[k]["fine_samples"] / max(base, 1), 4)
    for k, g in graphs.items():
        out[k]["captures"] = g.captures
    out["chain_worst_case_MB"] = round(R * 64 * 40 / 1e6, 1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rays", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--t-stop", type=float, default=1e-3)
    ap.add_argument("--sigma-bias", type=float, default=30.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window (at least)")
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--radius", type=float, default=0.35)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    net = synthetic_scene(DEV, 0, sigma_bias=args.sigma_bias)
    net.field_precision = "x3"
    grid = sphere_grid(args.res, args.radius)
    with torch.no_grad():
        for R in args.rays:
            print(json.dumps(frame_legs(net, grid, R, args)), flush=True)


if __name__ == "__main__":
    main()
