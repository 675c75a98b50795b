"""AdaptiveVolumeRenderer inference: the one-launch front end (avr_adaptive_front: seeded, multi-scene,
graph-ready) against the code paths the renderer had before it, in one process, alternating, so the run-to-run
spread is measured with the difference.

    python scripts/adaptive_infer_time.py [--rounds 5] [--window 0.5] [--launches]

Scene: avr.scene.synthetic_scene with default_mv's adaptive settings (20 band samples, 10 steps, eps 0.05).
  (a) SB = 1, 16 384 rays (the reference's 128 x 128 validation frame): the unseeded chain (host draw + copy,
      avr_raymarch, torch arithmetic, avr_sample_coarse_rays, torch.sort; unchanged by the front end) against the
      seeded front-end path;
  (b) SB = 4 x 16 384 rays: the module path several scenes took before (the reference's Python loop: 10 x
      phi(return_features=True) + LSTMCell) against the front-end path. The old routing is restored for the
      "before" leg by switching the front end off on that renderer object (_front_path -> False): the code below
      that switch is the code the renderer ran before;
  (c) SB = 1, 640 000 rays, seeded: eager and as a GraphedRenderer.
Every timed window is HIP events around enough calls to last --window seconds (after warm-up calls of the same
shape); a leg's figure is ms per call; legs alternate within a round. One JSON line per shape: median, min and
spread ((max - min) / median over the rounds) per leg. --launches LEG: no timing; --calls calls of that leg, for
a separate `rocprofv3 --kernel-trace --stats` run: a kernel launched once per call shows --calls calls there
(set-up kernels, such as weight packing, show one)."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "adaptive-volume-rendering_amd"))

from avr.graphs import GraphedRenderer  # noqa: E402
from avr.renderers import AdaptiveVolumeRenderer  # noqa: E402
from avr.scene import INTRINSICS, synthetic_scene  # noqa: E402
from avr.video import orbit_cam2world  # noqa: E402

DEV = torch.device("cuda:0")


def scene(sb, rays):
    net = synthetic_scene(DEV, 0)
    if sb > 1:   # further scenes: the latent rolled along W, the same source view
        lat = net.encoder.latent
        net.encoder.latent = torch.cat([torch.roll(lat, 3 * s, -1) for s in range(sb)], 0).contiguous()
        net.poses = net.poses.expand(sb, 3, 4).contiguous()
    g = torch.Generator().manual_seed(1)
    x_pix = torch.rand(sb, rays, 2, generator=g).to(DEV)
    poses = orbit_cam2world(max(sb, 2), 1.3)
    c2w = torch.stack([poses[s] for s in range(sb)]).to(DEV).reshape(sb, 1, 4, 4).expand(sb, rays, 4, 4)
    K = torch.tensor([INTRINSICS], device=DEV).expand(sb, 3, 3).contiguous()
    return net, c2w, K, x_pix


def renderer(net, seed):
    torch.manual_seed(2)
    r = AdaptiveVolumeRenderer(net.d_latent, 10, 0.05, 20, True).to(DEV)
    r.seed = seed
    return r


def ms_per_call(fn, window):
    """HIP events around n calls, n sized from a short calibration so the window lasts `window` seconds."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(3):
        fn()
    b.record()
    torch.cuda.synchronize()
    n = max(3, int(window * 1e3 / max(a.elapsed_time(b) / 3, 1e-3)) + 1)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def compare(label, legs, rounds, window):
    for fn in legs.values():       # warm-up: every shape and path the windows use
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():   # alternating within the round
            times[k].append(ms_per_call(fn, window))
    out = {"shape": label, "rounds": rounds, "window_s": window}
    for k, ts in times.items():
        s = sorted(ts)
        med = s[len(s) // 2]
        out[k] = {"median_ms": round(med, 4), "min_ms": round(s[0], 4), "spread": round((s[-1] - s[0]) / med, 4)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window (at least)")
    ap.add_argument("--launches", default=None, metavar="LEG",
                    help="no timing: --calls calls of one leg (unseeded_chain, front_seeded, module_path, front, "
                         "front_seeded_eager, front_seeded_graph), for a kernel trace")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--big-rays", type=int, default=640000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"

    def legs_a():
        net, c2w, K, x = scene(1, 16384)
        before, after = renderer(net, None), renderer(net, 5)
        return {"unseeded_chain": lambda: before(c2w, K, x, net), "front_seeded": lambda: after(c2w, K, x, net)}

    def legs_b():
        net, c2w, K, x = scene(4, 16384)
        before, after = renderer(net, None), renderer(net, None)
        before._front_path = lambda *a, **k: False   # the routing before the front end: the module path
        legs = {"module_path": lambda: before(c2w, K, x, net), "front": lambda: after(c2w, K, x, net)}
        with torch.no_grad():
            legs["module_path"](), legs["front"]()
        assert before.last_path == "module" and after.last_path == "fused"
        return legs

    def legs_c():
        net, c2w, K, x = scene(1, args.big_rays)
        eager = renderer(net, 5)
        graphed = GraphedRenderer(renderer(net, 5), net, c2w, K, x)
        return {"front_seeded_eager": lambda: eager(c2w, K, x, net), "front_seeded_graph": lambda: graphed()}

    shapes = (("a: SB=1 x 16384 rays", legs_a, ("unseeded_chain", "front_seeded")),
              ("b: SB=4 x 16384 rays", legs_b, ("module_path", "front")),
              (f"c: SB=1 x {args.big_rays} rays", legs_c, ("front_seeded_eager", "front_seeded_graph")))
    for label, build, names in shapes:
        if args.launches and args.launches not in names:
            continue
        legs = build()
        with torch.no_grad():   # (a GraphedRenderer replay does not mind)
            if args.launches:
                for _ in range(args.calls):
                    legs[args.launches]()
                torch.cuda.synchronize()
                print(json.dumps({"leg": args.launches, "calls": args.calls}), flush=True)
            else:
                compare(label, legs, args.rounds, args.window)

if __name__ == "__main__":
    main()
