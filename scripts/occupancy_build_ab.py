"""The hierarchical occupancy-grid build (OccupancyGrid.from_field(refine=...), refine_from_field) against the dense
build, in one process, legs alternating, so the run-to-run spread is measured with the difference.

    python scripts/occupancy_build_ab.py [--res 128] [--refine 4] [--rounds 3] [--out profiles/occupancy_build_ab.txt]

Shape: --res^3 over [-1, 1]^3, x3, avr.scene.synthetic_scene, both MLPs, the six axis directions. Legs:
  a  dense        from_field as every earlier commit builds it: the figure to measure against;
  b  refine       from_field(refine=--refine) on that scene, whatever its coarse share turns out to be (recorded);
  c  sphere       the dense (--res / --refine)^3 stage (timed, its grid not used) plus refine_from_field under the
                  (--res / --refine)^3 sphere grid of scripts/occupancy_ab.py: a realistic share, and a timing that
                  does not depend on the field's values;
  d  break-even   for c: the build plus N gated 128 x 128 frames against N ungated frames, N = 1 and 10.
Every build is bracketed by synchronisations (host clock); a leg's figure is the median over the rounds, with min and
spread ((max - min) / median). Per leg: build_evals, ms, the ratios to leg a, and the peak of torch's allocated memory
during the build above what was allocated before it. One JSON line per record, written to --out and printed."""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "adaptive-volume-rendering_amd"), os.path.join(REPO, "tests"), REPO,
          os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)

from avr.occupancy import OccupancyGrid  # noqa: E402
from avr.renderers import VolumeRenderer  # noqa: E402
from avr.scene import INTRINSICS, synthetic_scene  # noqa: E402
from avr.video import get_opencv_pixel_coordinates, orbit_cam2world  # noqa: E402
from occupancy_ab import sphere_grid  # noqa: E402

DEV = torch.device("cuda:0")
NC, NF = 128, 64
BOX = ((-1, -1, -1), (1, 1, 1))


def build_timed(fn):
    """(grid, ms, peak MB above the allocation before the build) of one build, bracketed by synchronisations."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    grid = fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return grid, ms, (torch.cuda.max_memory_allocated() - base) / 1e6


def summary(ts):
    s = sorted(ts)
    med = s[len(s) // 2]
    return {"ms": round(med, 3), "min_ms": round(s[0], 3), "spread": round((s[-1] - s[0]) / med, 4)}


def frame_ms(rend, net, c2w, K, x_pix, rounds):
    ts = []
    for _ in range(rounds + 1):                    # the first one is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(4):
            rend(c2w, K, x_pix, net)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / 4)
    return summary(ts[1:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--refine", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--radius", type=float, default=0.35)
    ap.add_argument("--frame", type=int, default=128, help="leg d: frame height = width")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "occupancy_build_ab.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    res, f = (args.res,) * 3, args.refine
    rc = tuple(r // f for r in res)
    net = synthetic_scene(DEV, 0)
    net.field_precision = "x3"
    sphere = sphere_grid(rc[0], args.radius)

    stage_ms = {"coarse_dense_stage": [], "refine_stage": []}

    def leg_c():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        OccupancyGrid.from_field(net, *BOX, rc)                       # the dense coarse stage: paid, not used
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        grid = OccupancyGrid.refine_from_field(net, sphere, f)
        torch.cuda.synchronize()
        stage_ms["coarse_dense_stage"].append((t1 - t0) * 1e3)
        stage_ms["refine_stage"].append((time.perf_counter() - t1) * 1e3)
        return grid

    legs = {"a_dense": lambda: OccupancyGrid.from_field(net, *BOX, res),
            "b_refine": lambda: OccupancyGrid.from_field(net, *BOX, res, refine=f),
            "c_sphere": leg_c}
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    with torch.no_grad():
        for fn in legs.values():                                       # warm-up: caches, lin_z tables, code objects
            fn()
        times, peaks, grids = {k: [] for k in legs}, {k: 0.0 for k in legs}, {}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                grids[k], ms, peak = build_timed(fn)
                times[k].append(ms)
                peaks[k] = max(peaks[k], peak)
        coarse_evals = 12 * rc[0] * rc[1] * rc[2]
        rec = {"shape": f"{args.res}^3 over [-1, 1]^3, refine {f}, x3, synthetic scene, 12 planes",
               "rounds": args.rounds}
        a_ms = summary(times["a_dense"])["ms"]
        for k in legs:
            g = grids[k]
            evals = g.build_evals + (coarse_evals if k == "c_sphere" else 0)
            rec[k] = dict(summary(times[k]), build_evals=evals, peak_MB=round(peaks[k], 1),
                          cells_set=round(g.live_fraction(), 4),
                          evals_ratio_to_a=round(evals / grids["a_dense"].build_evals, 4),
                          ms_ratio_to_a=round(summary(times[k])["ms"] / a_ms, 4),
                          peak_ratio_to_a=round(peaks[k] / peaks["a_dense"], 4))
            if g.n_candidates is not None:
                rec[k]["n_candidates"] = g.n_candidates
                rec[k]["coarse_share"] = round(g.n_candidates / (res[0] * res[1] * res[2]), 4)
        # where leg c's time goes: its two stages (the last --rounds calls; each has 12 field launches), against
        # what leg a's rate per evaluated point would give them
        per_eval = a_ms / grids["a_dense"].build_evals
        rec["c_sphere"]["stages"] = {
            k: dict(summary(v[-args.rounds:]), at_dense_rate_ms=round(per_eval * n, 3))
            for (k, v), n in zip(stage_ms.items(), (coarse_evals, grids["c_sphere"].build_evals))}
        rec["b_refine"]["cells_missing_from_dense"] = grids["b_refine"].cells_missing_from(grids["a_dense"])
        emit(rec)

        # d: the break-even of leg c at a 128 x 128 frame
        H = W = args.frame
        x_pix = get_opencv_pixel_coordinates(H, W).reshape(1, -1, 2).to(DEV)
        n = x_pix.shape[1]
        c2w = orbit_cam2world(8, 1.3)[1].to(DEV).reshape(1, 1, 4, 4).expand(1, n, 4, 4)
        K = torch.tensor([INTRINSICS], device=DEV)
        frames = {}
        for k, g in (("ungated", None), ("gated", grids["c_sphere"])):
            rend = VolumeRenderer(0.8, 1.8, NC, NF, 0, 0.01, True)
            rend.seed, rend.occupancy = 1234, g
            frames[k] = frame_ms(rend, net, c2w, K, x_pix, args.rounds)
            if g is not None:
                frames[k]["live_share"] = round(rend.last_live_samples / (n * (2 * NC + NF)), 4)
        build = summary(times["c_sphere"])["ms"]
        d = {"record": f"d: break-even of leg c, {H} x {W} frames ({n} rays x ({NC} + {NF}))", "frames": frames,
             "build_ms": build, "dense_build_ms": a_ms}
        for N in (1, 10):
            d[f"N={N}"] = {"build_plus_gated_ms": round(build + N * frames["gated"]["ms"], 3),
                           "dense_build_plus_gated_ms": round(a_ms + N * frames["gated"]["ms"], 3),
                           "ungated_ms": round(N * frames["ungated"]["ms"], 3)}
        emit(d)
    with open(args.out, "w") as fh:
        fh.write("# python scripts/occupancy_build_ab.py   (MI355X, one process, legs alternating; synthetic scene "
                 "and synthetic sphere grid; no trained scene was available)\n")
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
