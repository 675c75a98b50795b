"""Occupancy gating with the live count on the device (renderer.occupancy_count = "device") against the host-read
path, in one process, legs alternating, so the run-to-run spread is measured with the difference (the protocol of
scripts/occupancy_ab.py).

    python scripts/occupancy_count_ab.py [--rays 65536 4096] [--rounds 3] [--window 0.5] [--res 128]

Shape: --rays rays x (128 + 64) samples, x3, avr.scene.synthetic_scene, the synthetic sphere grid of
scripts/occupancy_ab.py (cells whose centre lies within --radius of the origin of [-1, 1]^3). Legs per ray count:
  ungated        renderer.occupancy = None;
  host           occupancy_count = "host": the host-read path, the yardstick;
  device         occupancy_count = "device", eager;
  device_graph   the same renderer replayed from avr.graphs.GraphedRenderer.
Every timed window is HIP events around enough frames to last --window seconds, after warm-up frames of the same
leg; a leg's figure is ms per frame; legs alternate within a round. One JSON line per ray count: median, min and
spread ((max - min) / median over the rounds) per leg. Then two records:
  scan           avr_occ_scan against the torch.cumsum and subtraction it replaces, at each ray count;
  empty_field    avr_field_fwd_points_counted at --empty-capacity rows with a count of 0: the cost of the workgroups
                 that exit at once, both passes' MLPs."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "adaptive-volume-rendering_amd"), REPO):
    sys.path.insert(0, p)

from avr import occupancy  # noqa: E402
from avr.graphs import GraphedRenderer  # noqa: E402
from avr.occupancy import OccupancyGrid  # noqa: E402
from avr.renderers import VolumeRenderer  # noqa: E402
from avr.scene import INTRINSICS, synthetic_scene  # noqa: E402
from avr.video import orbit_cam2world  # noqa: E402

DEV = torch.device("cuda:0")
NC, NF = 128, 64


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


def frame_legs(net, grid, R, args):
    x_pix = torch.rand(1, R, 2, generator=torch.Generator().manual_seed(100)).to(DEV)
    c2w = orbit_cam2world(8, 1.3)[1].to(DEV).reshape(1, 1, 4, 4).expand(1, R, 4, 4).contiguous()
    K = torch.tensor([INTRINSICS], device=DEV)
    rends = {}
    for k, (g, mode) in {"ungated": (None, "host"), "host": (grid, "host"), "device": (grid, "device"),
                         "device_graph": (grid, "device")}.items():
        rends[k] = VolumeRenderer(0.8, 1.8, NC, NF, 0, 0.01, True)
        rends[k].seed, rends[k].occupancy, rends[k].occupancy_count = 1234, g, mode
    legs = {k: (lambda r=r: r(c2w, K, x_pix, net)) for k, r in rends.items() if k != "device_graph"}
    graphed = GraphedRenderer(rends["device_graph"], net, c2w, K, x_pix)
    legs["device_graph"] = graphed
    out = {"shape": f"{R} rays x ({NC} + {NF}), x3, synthetic scene", "rounds": args.rounds, "window_s": args.window,
           "grid": f"{args.res}^3 sphere, radius {args.radius}", "cells_set": round(grid.live_fraction(), 4)}
    out.update(alternate(legs, args.rounds, args.window))
    per_frame = R * (2 * NC + NF)
    out["host"]["live_share"] = round(rends["host"].last_live_samples / per_frame, 4)
    for k in ("device", "device_graph"):
        out[k]["live_share"] = round(int(rends[k].last_live_counts.sum().item()) / per_frame, 4)
    out["device_graph"]["captures"] = graphed.captures
    out["device_graph"]["graph_pool_worst_case_MB"] = round(R * (NC + NF) * 40 / 1e6 + R * NC * 40 / 1e6, 1)
    return out


def scan_record(R, args):
    counts = torch.randint(0, 257, (R,), device=DEV, dtype=torch.int32)
    legs = {"torch_cumsum_sub": lambda: (lambda i: i - counts)(torch.cumsum(counts, 0, dtype=torch.int64)),
            "avr_occ_scan": lambda: occupancy.scan(counts)}
    rec = {"record": "scan", "rays": R}
    rec.update(alternate(legs, args.rounds, min(args.window, 0.2)))
    return rec


def empty_field_record(net, args):
    fused = net.fused()
    cap = args.empty_capacity
    xyz = torch.zeros(cap, 3, device=DEV)
    vd = torch.zeros(cap, 3, device=DEV)
    out = torch.empty(cap, 4, device=DEV)
    zero = torch.zeros((), device=DEV, dtype=torch.int64)
    legs = {("coarse" if c else "fine"): (lambda c=c: fused.forward_points_scene_counted(xyz, vd, zero, c, out=out))
            for c in (True, False)}
    rec = {"record": "empty_field", "capacity": cap, "count": 0, "workgroups": (cap + 63) // 64}
    rec.update(alternate(legs, args.rounds, min(args.window, 0.2)))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rays", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window (at least)")
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--radius", type=float, default=0.35)
    ap.add_argument("--empty-capacity", type=int, default=65536 * (NC + NF))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    net = synthetic_scene(DEV, 0)
    net.field_precision = "x3"
    grid = sphere_grid(args.res, args.radius)
    with torch.no_grad():
        for R in args.rays:
            print(json.dumps(frame_legs(net, grid, R, args)), flush=True)
        for R in args.rays:
            print(json.dumps(scan_record(R, args)), flush=True)
        print(json.dumps(empty_field_record(net, args)), flush=True)


if __name__ == "__main__":
    main()
