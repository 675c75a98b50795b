"""Timings of avr.losses.loss_fn and avr.metrics.image_metrics (DESIGN "Loss and metrics kernels"), HIP events,
warmed up, median of REPS; written to profiles/loss_metrics_timing.json (or OUT):
  1. loss forward + backward at 4 x 512 rays, mode both with the depth penalty, against the torch expression of the
     same loss on the same tensors: time and device launches (torch.profiler's kernel events);
  2. image_metrics at 2 x 128 x 128 and 1 x 800 x 800 against its algorithmic bytes (both frames read once) at the
     rate avr_stream_copy reaches on the same machine;
  3. the graphed adaptive default_mv training step (tests/test_gpu_poison._setup, avr.graphs.GraphedTrainStep)
     with loss_fn in step_fn against the hand-written MSE expression (SKIP_STEP=1 leaves it out).
"""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "adaptive-volume-rendering_amd"), REPO):
    sys.path.insert(0, p)
from avr import ops  # noqa: E402
from avr.losses import loss_fn  # noqa: E402
from avr.metrics import image_metrics  # noqa: E402

DEV = torch.device("cuda:0")
REPS = int(os.environ.get("REPS", "50"))
OUT = os.environ.get("OUT", os.path.join(REPO, "profiles", "loss_metrics_timing.json"))


def timed_us(fn, warmup=10, reps=REPS):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def launches(fn):
    """Device kernels (and memsets / copies) one call of fn enqueues, or None where the profiler has no device
    events."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if str(getattr(ev, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception as exc:   # the measurement is optional; the timing stands without it
        print(f"launch count unavailable: {exc}")
        return None


def graphed_us(fn, reps=REPS):
    """fn captured into one graph and replayed: the device time of its launches without the host between them."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return timed_us(graph.replay, reps=reps)


def loss_section():
    SB, R = 4, 512
    g = torch.Generator().manual_seed(0)
    rgb_c, rgb_f, gt = (torch.rand(SB, R, 3, generator=g).to(DEV) for _ in range(3))
    depth = (0.2 + 2.2 * torch.rand(SB, R, generator=g)).to(DEV)
    leaves = [t.requires_grad_(True) for t in (rgb_c, rgb_f, depth)]
    near, far = 0.5, 2.0

    def hip():
        return torch.autograd.grad(loss_fn((*leaves, None), gt, ("both", True)), leaves)

    def expr():
        penalty = torch.max(near - depth, torch.zeros_like(depth)) + torch.max(depth - far, torch.zeros_like(depth))
        loss = ((rgb_c - gt) ** 2).mean() + ((rgb_f - gt) ** 2).mean() + torch.mean(penalty) * 10000
        return torch.autograd.grad(loss, leaves)

    res = {"rays": SB * R, "mode": "both", "depth_regularization": True}
    for name, fn in (("loss_fn", hip), ("torch_expression", expr)):
        res[name] = {"eager_us": timed_us(fn), "graph_replay_us": graphed_us(fn), "launches": launches(fn)}
    return res


def metrics_section():
    n = 256 << 20
    src, dst = torch.empty(n, dtype=torch.uint8, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
    src.zero_()
    copy_us = timed_us(lambda: ops.stream_copy(src, dst))
    rate = 2.0 * n / (copy_us * 1e-6)       # bytes read + written per second
    res = {"stream_copy_GBps": rate / 1e9, "shapes": []}
    del src, dst
    for B, H, W in ((2, 128, 128), (1, 800, 800)):
        img, gt = torch.rand(B, H * W, 3, device=DEV), torch.rand(B, H * W, 3, device=DEV)
        us = timed_us(lambda: image_metrics(img, gt, H, W))
        nbytes = 2 * B * H * W * 3 * 4
        res["shapes"].append({"frames": B, "height": H, "width": W, "us": us, "algorithmic_bytes": nbytes,
                              "bytes_at_copy_rate_us": nbytes / rate * 1e6, "GBps": nbytes / (us * 1e-6) / 1e9})
    return res


def step_section():
    from test_gpu_poison import _setup
    from avr.graphs import GraphedTrainStep
    res = {}
    for name in ("hand_written_mse", "loss_fn"):
        torch.manual_seed(1234)
        net, rend, named, (c2w, K, x_pix, gt), _ = _setup("adaptive", False)
        opt = torch.optim.Adam([p for _, p in named], lr=1e-4, capturable=True, fused=True)

        def step():
            out = rend(c2w, K, x_pix, net)
            if name == "loss_fn":
                loss = loss_fn(out, gt, ("both", False))
            else:
                loss = ((out[0] - gt) ** 2).mean() + ((out[1] - gt) ** 2).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss

        run = GraphedTrainStep(step, nets=[net], renderers=[rend], warmup=3)
        first = float(run())
        for _ in range(5):
            loss = run()
        us = timed_us(run, warmup=3, reps=min(REPS, 30))
        assert run.captures == 1 and bool(torch.isfinite(run().detach()))
        # the first step's losses agree to an fp32 ulp; Adam then amplifies the last-bit gradient differences
        res[name] = {"step_us": us, "first_step_loss": first, "sixth_step_loss": float(loss.detach())}
        del run, opt, net, rend, named, loss
    return res


def main():
    out = {"device": torch.cuda.get_device_name(0), "reps": REPS, "loss": loss_section(),
           "image_metrics": metrics_section()}
    if not os.environ.get("SKIP_STEP"):
        out["graphed_adaptive_step"] = step_section()
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
