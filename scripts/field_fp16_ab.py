"""The field's "fp16" precision (one fp16 product per term, AVR_FIELD_FP16) against "x3", in one process, legs
alternating, so the run-to-run spread is measured with the difference (the protocol of scripts/occupancy_count_ab.py).

    python scripts/field_fp16_ab.py [--rays 65536 4096] [--rounds 3] [--window 0.5] [--res 128]

Shape: --rays rays x (128 + 64) samples on avr.scene.synthetic_scene; both precisions run on the one net (they share
its packed blob and lin_z tables), net.field_precision switched per call. Records per ray count:
  field   the fine field launch alone (FusedField.forward_rays, rays x 192 samples, the fine MLP);
  frame   the whole VolumeRenderer frame;
  gated   the frame under the sphere grid of scripts/occupancy_ab.py (cells whose centre lies within --radius of the
          origin of [-1, 1]^3), occupancy_count = "device".
Every timed window is HIP events around enough calls to last --window seconds, after warm-up calls of the same leg; a
leg's figure is ms per call; legs alternate within a round. One JSON line per record: median, min and spread
((max - min) / median over the rounds) per leg, the ratio x3 / fp16 of the medians, and whether the difference of the
medians exceeds the two legs' spreads added up (faster_beyond_spread). The frame and gated records also carry what
the precision costs in the picture: max and mean |rgb difference| of the coarse and the fine frame between the two
precisions on the same draws, and the share of the fine frame's 8-bit values that differ at all and by more than
one code."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "adaptive-volume-rendering_amd"), REPO):
    sys.path.insert(0, p)

from avr.occupancy import OccupancyGrid  # noqa: E402
from avr.renderers import VolumeRenderer  # noqa: E402
from avr.scene import INTRINSICS, synthetic_scene  # noqa: E402
from avr.video import orbit_cam2world  # noqa: E402

DEV = torch.device("cuda:0")
NC, NF = 128, 64
PRECISIONS = ("x3", "fp16")


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
    out = {k: summary(ts) for k, ts in times.items()}
    x3, fp16 = out["x3"], out["fp16"]
    out["x3_over_fp16"] = round(x3["ms"] / fp16["ms"], 4)
    out["faster_beyond_spread"] = bool(x3["ms"] - fp16["ms"] > x3["spread"] * x3["ms"] + fp16["spread"] * fp16["ms"])
    return out


def under(net, precision, fn):
    def call():
        net.field_precision = precision
        return fn()
    return call


def camera(R):
    x_pix = torch.rand(1, R, 2, generator=torch.Generator().manual_seed(100)).to(DEV)
    c2w = orbit_cam2world(8, 1.3)[1].to(DEV).reshape(1, 1, 4, 4).expand(1, R, 4, 4).contiguous()
    return x_pix, c2w, torch.tensor([INTRINSICS], device=DEV)


def field_record(net, R, args):
    from avr import ops
    x_pix, c2w, K = camera(R)     # the frame records' rays, sorted uniform depths in [near, far)
    ro, rd, _ = ops.world_rays(x_pix, K, c2w)
    ro, rd = ro[0].contiguous(), rd[0].contiguous()
    z = torch.sort(0.8 + torch.rand(R, NC + NF, generator=torch.Generator().manual_seed(101)), -1)[0].to(DEV)
    legs = {p: under(net, p, lambda: net.fused().forward_rays(ro, rd, z, False)) for p in PRECISIONS}
    rec = {"record": "field", "shape": f"{R} rays x {NC + NF} samples, fine MLP, synthetic scene",
           "rounds": args.rounds, "window_s": args.window}
    rec.update(alternate(legs, args.rounds, args.window))
    return rec


def picture(frames):
    (c3, f3), (c16, f16) = frames["x3"], frames["fp16"]
    codes = lambda t: torch.round(t.clamp(0.0, 1.0) * 255.0).to(torch.int32)   # noqa: E731
    dc = (codes(f3) - codes(f16)).abs()
    return {"rgb_coarse_max": float((c3 - c16).abs().max()), "rgb_coarse_mean": float((c3 - c16).abs().mean()),
            "rgb_fine_max": float((f3 - f16).abs().max()), "rgb_fine_mean": float((f3 - f16).abs().mean()),
            "codes_differing": round(float((dc > 0).float().mean()), 6),
            "codes_off_by_more_than_one": round(float((dc > 1).float().mean()), 6)}


def frame_record(net, grid, R, args):
    x_pix, c2w, K = camera(R)
    rend = VolumeRenderer(0.8, 1.8, NC, NF, 0, 0.01, True)
    rend.seed = 1234
    if grid is not None:
        rend.occupancy, rend.occupancy_count = grid, "device"
    frames = {}
    for p in PRECISIONS:   # the same draws for both precisions
        rend._offset = 0
        net.field_precision = p
        frames[p] = rend(c2w, K, x_pix, net)[:2]
    legs = {p: under(net, p, lambda: rend(c2w, K, x_pix, net)) for p in PRECISIONS}
    rec = {"record": "frame" if grid is None else "gated",
           "shape": f"{R} rays x ({NC} + {NF}), synthetic scene", "rounds": args.rounds, "window_s": args.window}
    if grid is not None:
        rec["grid"] = f"{args.res}^3 sphere, radius {args.radius}, occupancy_count device"
    rec.update(alternate(legs, args.rounds, args.window))
    if grid is not None:
        rec["live_share"] = round(int(rend.last_live_counts.sum().item()) / (R * (2 * NC + NF)), 4)
    rec["picture"] = picture(frames)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rays", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window (at least)")
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--radius", type=float, default=0.35)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    assert args.rounds >= 3 and args.window >= 0.5, "at least 3 rounds of windows of at least 0.5 s"
    net = synthetic_scene(DEV, 0)
    grid = sphere_grid(args.res, args.radius)
    with torch.no_grad():
        for R in args.rays:
            print(json.dumps(field_record(net, R, args)), flush=True)
            print(json.dumps(frame_record(net, None, R, args)), flush=True)
            print(json.dumps(frame_record(net, grid, R, args)), flush=True)


if __name__ == "__main__":
    main()
