"""Time of one optimizer.step() over train.py's parameter set (DESIGN "Adam step"): the parameters of
bench.build_scene(conf="default_mv") plus the adaptive renderer's, gradients filled once, four forms in one process:
  torch.optim.Adam (default: foreach), torch.optim.Adam(fused=True), torch.optim.Adam(capturable=True, fused=True)
  and avr.optim.Adam.
HIP events around blocks of 25 eager step() calls, 6 blocks per form after a warm-up, the forms taking turns block
by block; per form the median block (microseconds per step) and the max - min spread of its 6 blocks. The eager
figure holds the host's share of a step (the launches are enqueued one step after the other, so a form whose
host side is slower than its kernels is bound by the host). The same step captured into a HIP graph and replayed
gives the device time alone, for the two forms a capture accepts. avr_stream_copy over the same number of bytes
(7 streams of 4 B per parameter: p, g, m, v read, p, m, v written) is the achievable-HBM yardstick.
Gate: avr.optim.Adam's median <= torch.optim.Adam(fused=True)'s median + that form's own spread.
Written to profiles/adam_step_default_mv.txt (or OUT)."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "adaptive-volume-rendering_amd"), REPO):
    sys.path.insert(0, p)
import bench  # noqa: E402
from avr import ops  # noqa: E402
from avr.conf import default_conf  # noqa: E402
from avr.optim import Adam  # noqa: E402
from avr.renderers import AdaptiveVolumeRenderer  # noqa: E402

DEV = torch.device("cuda:0")
BLOCKS, PER_BLOCK, WARMUP = 6, 25, 10
OUT = os.environ.get("OUT", os.path.join(REPO, "profiles", "adam_step_default_mv.txt"))


def block_us(fn, n=PER_BLOCK):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(n):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / n


def stats(ts):
    ts = sorted(ts)
    return 0.5 * (ts[len(ts) // 2 - 1] + ts[len(ts) // 2]), ts[-1] - ts[0]


def main():
    net = bench.build_scene(DEV, conf="default_mv")
    rend = AdaptiveVolumeRenderer.from_conf(default_conf()["adaptive_renderer"]).to(DEV)
    shapes = [p.shape for p in list(net.parameters()) + list(rend.parameters())]
    numel = sum(s.numel() for s in shapes)
    g = torch.Generator(device="cpu").manual_seed(0)
    values = [0.1 * torch.randn(s, generator=g) for s in shapes]
    grad_values = [torch.randn(s, generator=g) for s in shapes]

    def params():
        ps = [torch.nn.Parameter(v.to(DEV)) for v in values]
        for p, gv in zip(ps, grad_values):
            p.grad = gv.to(DEV)
        return ps

    forms = [("torch.optim.Adam()", lambda ps: torch.optim.Adam(ps, lr=1e-4)),
             ("torch.optim.Adam(fused=True)", lambda ps: torch.optim.Adam(ps, lr=1e-4, fused=True)),
             ("torch.optim.Adam(capturable=True, fused=True)",
              lambda ps: torch.optim.Adam(ps, lr=1e-4, capturable=True, fused=True)),
             ("avr.optim.Adam()", lambda ps: Adam(ps, lr=1e-4))]
    opts = [(name, make(params())) for name, make in forms]
    for _, opt in opts:
        for _ in range(WARMUP):
            opt.step()
    times = {name: [] for name, _ in opts}
    for _ in range(BLOCKS):
        for name, opt in opts:
            times[name].append(block_us(opt.step))

    replay = {}
    for name, opt in opts[2:]:
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph):
            opt.step()
        graph.replay()
        replay[name] = stats([block_us(graph.replay) for _ in range(BLOCKS)])

    half = (numel * 14 + 15) // 16 * 16                 # read + written = 28 B per parameter
    src, dst = torch.zeros(half, dtype=torch.uint8, device=DEV), torch.empty(half, dtype=torch.uint8, device=DEV)
    for _ in range(WARMUP):
        ops.stream_copy(src, dst)
    copy_us, copy_spread = stats([block_us(lambda: ops.stream_copy(src, dst)) for _ in range(BLOCKS)])

    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             f"parameter set: bench.build_scene(conf='default_mv') + AdaptiveVolumeRenderer: {len(shapes)} tensors, "
             f"{numel} parameters, {28 * numel / 1e6:.1f} MB moved per step (7 x 4 B per parameter)",
             f"eager step(): HIP events around {PER_BLOCK} calls, {BLOCKS} blocks per form, forms taking turns; "
             "us per step, median block [spread max - min]; blocks:"]
    med = {}
    for name, _ in opts:
        med[name], spread = stats(times[name])
        lines.append(f"  {name:48s} {med[name]:8.1f} [{spread:6.1f}]   " + " ".join(f"{t:.1f}" for t in times[name]))
    lines.append("the step captured into a HIP graph, replayed (device time without the host), us per step:")
    for name, (m, s) in replay.items():
        lines.append(f"  {name:48s} {m:8.1f} [{s:6.1f}]   {copy_us / m:.2f} of the yardstick")
    lines.append(f"avr_stream_copy of {half} B (as many bytes read + written as one step moves): {copy_us:.1f} us "
                 f"[{copy_spread:.1f}] = {2 * half / copy_us / 1e6:.2f} TB/s")
    fused = "torch.optim.Adam(fused=True)"
    limit = med[fused] + stats(times[fused])[1]
    ok = med["avr.optim.Adam()"] <= limit
    lines.append(f"gate: avr.optim.Adam() median {med['avr.optim.Adam()']:.1f} us <= {fused} median + spread "
                 f"{limit:.1f} us: {'PASS' if ok else 'FAIL'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
