"""Full-frame rendering on the fused path: the reference's video utilities
(utils.py:339-356 get_opencv_pixel_coordinates, :464-479 get_R, :481-537
generate_video) with the same signatures and pose conventions, plus
`render_orbit`, a frame loop that takes a ready radiance field (no encoder)
and can terminate the fine pass early (BASELINE config 4).

Frames come back as uint8 (H, W, 3) numpy arrays like the reference's;
`write_ppm` stores them without an image library."""
import contextlib
import math
import time

import numpy as np
import torch
import torch.nn.functional as F


def get_opencv_pixel_coordinates(y_resolution, x_resolution):
    """utils.py:339-356. (y_res, x_res, 2) pixel coordinates in [0, 1), origin
    top-left; quirk Q8 kept: both axes step by 1 / x_resolution."""
    i, j = torch.meshgrid(torch.linspace(0, 1 - 1 / x_resolution, steps=x_resolution),
                          torch.linspace(0, 1 - 1 / x_resolution, steps=y_resolution), indexing="ij")
    return torch.stack([i.float(), j.float()], dim=-1).permute(1, 0, 2)


def get_R(x, y, z):
    """Look-at rotation of a camera at (x, y, z) aimed at the origin, with the
    scene's (0, 0, -1) reference direction (utils.py:464-479): (1, 3, 3) whose
    columns are the camera's x, y and viewing axes. When the viewing axis is
    (anti)parallel to the reference direction, x is rebuilt from y and the
    viewing axis, as the reference does."""
    eye = torch.tensor([[float(x), float(y), float(z)]], dtype=torch.float32)
    ref_dir = torch.tensor([[0.0, 0.0, -1.0]])
    view = F.normalize(torch.zeros(1, 3) - eye, eps=1e-5)
    cam_x = F.normalize(torch.cross(ref_dir, view, dim=1), eps=1e-5)
    cam_y = F.normalize(torch.cross(view, cam_x, dim=1), eps=1e-5)
    degenerate = torch.isclose(cam_x, torch.tensor(0.0), atol=5e-3).all(dim=1, keepdim=True)
    if bool(degenerate.any()):
        cam_x = torch.where(degenerate, F.normalize(torch.cross(cam_y, view, dim=1), eps=1e-5), cam_x)
    return torch.stack([cam_x, cam_y, view], dim=2)


def orbit_cam2world(num_frames, radius, z_height=0.4):
    """The camera ring of generate_video (utils.py:499-515): num_frames poses
    at height z_height on a circle of the given radius around the origin,
    OpenCV convention (x diag(1, -1, -1, 1)). Returns a list of (4, 4)."""
    angles = torch.linspace(0, 2 * np.pi * (num_frames - 1) / num_frames, num_frames) + np.pi / num_frames
    rradius = math.sqrt(radius * radius - z_height * z_height)
    flip = torch.diag(torch.tensor([1, -1, -1, 1], dtype=torch.float32))
    out = []
    for i in range(num_frames):
        angle = float(angles[i])
        tx, ty, tz = rradius * math.sin(angle), rradius * math.cos(angle), z_height
        c2w = torch.zeros(4, 4)
        c2w[:3, :3] = get_R(tx, ty, tz)[0]
        c2w[0, 3], c2w[1, 3], c2w[2, 3], c2w[3, 3] = tx, ty, tz, 1.0
        out.append(c2w @ flip)
    return out


def to_uint8(img):
    """The reference's frame conversion (utils.py:528-531)."""
    return np.clip(img * 255, 0, 255).astype(np.uint8)


@contextlib.contextmanager
def renderer_modes(renderer, **modes):
    """renderer.NAME = value for every NAME=value while the block runs, the former values after it (a renderer without
    such an attribute is left with the attribute's default: None, or 'host' for a count)."""
    prev = {k: getattr(renderer, k, "host" if k.endswith("_count") else None) for k in modes}
    try:
        for k, v in modes.items():
            setattr(renderer, k, v)
        yield
    finally:
        for k, v in prev.items():
            setattr(renderer, k, v)


class FrameCounts:
    """The field samples a renderer evaluated over a run of frames, fine and live. A count the renderer keeps on the
    device (t_stop_count / occupancy_count = 'device') is summed there frame by frame; read() -> (fine, live) as ints
    reads those sums, once, after the last frame."""

    def __init__(self, fine_on_device, live_on_device):
        self._attrs = ("last_fine_counts" if fine_on_device else "last_fine_samples",
                       "last_live_counts" if live_on_device else "last_live_samples")
        self._sums = [0, 0]

    def add(self, renderer):   # (0 + a device tensor is a new tensor: a captured graph's buffer is not kept)
        self._sums = [s + getattr(renderer, a, 0) for s, a in zip(self._sums, self._attrs)]

    def read(self):
        return tuple(int(s.sum().item()) if torch.is_tensor(s) else s for s in self._sums)


def check_refine_modes(who, occupancy, refine, probe, idle=None, name=str):
    """The hierarchical grid build's two arguments, in check_skip_modes' style: refine (2, 4 or 8) and probe (1, 2 or
    4) need occupancy = RES, RES must be divisible by refine with RES / refine a multiple of 32, and probe needs
    refine; ValueError otherwise. `idle`: what probe holds when it was not given (render_orbit: 1, its default; the
    CLI: None). `name` spells the names in the caller's vocabulary."""
    from .occupancy import PROBE_FACTORS, REFINE_FACTORS
    if refine is None:
        if probe != idle:
            raise ValueError(f"{who}{name('occupancy_probe')} needs {name('occupancy_refine')}")
        return
    if occupancy is None:
        raise ValueError(f"{who}{name('occupancy_refine')} needs {name('occupancy')}")
    if refine not in REFINE_FACTORS:
        raise ValueError(f"{who}{name('occupancy_refine')} must be one of {REFINE_FACTORS}, got {refine!r}")
    if probe not in PROBE_FACTORS + (idle,):
        raise ValueError(f"{who}{name('occupancy_probe')} must be one of {PROBE_FACTORS}, got {probe!r}")
    if int(occupancy) % refine or (int(occupancy) // refine) % 32:
        raise ValueError(f"{who}{name('occupancy_refine')} {refine} needs {name('occupancy')} = a multiple of "
                         f"{32 * refine}, got {occupancy}")


def render_orbit(renderer, radiance_field, intrinsics, num_frames, radius, height, width=None, fine=True,
                 device=None, t_stop=None, on_frame=None, occupancy=None, occupancy_sigma=0.0, occupancy_box=1.0,
                 occupancy_count="host", t_stop_count="host", occupancy_refine=None, occupancy_probe=1,
                 ray_bounds=None):
    """Render num_frames full frames around the orbit with `renderer`
    (e.g. avr.renderers.VolumeRenderer) and a ready radiance field. One
    renderer call per frame (all H * W rays at once), no_grad. Returns
    (frames, stats): frames uint8 (H, W, 3); stats = seconds, rays/s and the
    fine samples evaluated (< H * W * (n_coarse + n_fine) once rays terminate).
    occupancy = RES (the CLI's --occupancy / --occupancy-sigma): a RES^3 grid over
    [-occupancy_box, occupancy_box]^3 is built from the field once before the frames
    (avr.occupancy.OccupancyGrid.from_field) and gates every frame; stats then carry
    the live share of the field samples, which is printed at the end.
    occupancy_count = "host" | "device" (renderer.occupancy_count for these frames): with "device" no frame reads
    its live count back; the counts are summed on the device and read once after the last frame.
    t_stop_count = "host" | "device" (renderer.t_stop_count for these frames; "device" needs t_stop): with "device"
    the fine pass is terminated, and with occupancy also gated, without a host read; the evaluated fine samples are
    summed on the device and read once after the last frame.
    occupancy_refine = F (2, 4 or 8), occupancy_probe = P (1, 2 or 4): the grid is built hierarchically
    (from_field(refine=F, coarse_probe=P): the field only under the live cells of a (RES / F)^3 grid); both need
    occupancy. stats then carry occupancy_build_evals and occupancy_build_ms.
    ray_bounds = None | "grid" (renderer.ray_bounds for these frames; "grid" needs occupancy): every ray samples the
    span of its own occupied cells; stats then carry ray_bounds."""
    from .renderers import check_skip_modes
    check_skip_modes("render_orbit: ", t_stop, t_stop_count, occupancy, occupancy_count, idle="host",
                     ray_bounds=ray_bounds)
    check_refine_modes("render_orbit: ", occupancy, occupancy_refine, occupancy_probe, idle=1)
    width = width or height
    device = device or intrinsics.device
    K = intrinsics.reshape(1, 3, 3).to(device)
    x_pix = get_opencv_pixel_coordinates(height, width).reshape(1, -1, 2).to(device)
    n = x_pix.shape[1]
    grid = None
    if occupancy is not None:
        from .occupancy import OccupancyGrid
        h = float(occupancy_box)
        on_gpu = torch.device(device).type == "cuda"      # (elsewhere from_field raises before any launch)
        if on_gpu:
            torch.cuda.synchronize(device)
        t_build = time.perf_counter()
        grid = OccupancyGrid.from_field(radiance_field, (-h, -h, -h), (h, h, h), (int(occupancy),) * 3,
                                        sigma_thr=occupancy_sigma, refine=occupancy_refine,
                                        coarse_probe=occupancy_probe)
        if on_gpu:
            torch.cuda.synchronize(device)
        build_ms = (time.perf_counter() - t_build) * 1e3
    modes = {"t_stop": t_stop}
    if t_stop is not None:
        modes["t_stop_count"] = t_stop_count
    if grid is not None:
        modes.update(occupancy=grid, occupancy_count=occupancy_count)
    if ray_bounds is not None:
        modes["ray_bounds"] = ray_bounds
    frames = []
    counts = FrameCounts(t_stop is not None and t_stop_count == "device",
                         grid is not None and occupancy_count == "device")
    with renderer_modes(renderer, **modes):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        with torch.no_grad():
            for c2w in orbit_cam2world(num_frames, radius):
                c2w = c2w.to(device).reshape(1, 1, 4, 4).expand(1, n, 4, 4)
                rgb_c, rgb_f, _, _ = renderer(c2w, K, x_pix, radiance_field)
                counts.add(renderer)
                img = (rgb_f if fine else rgb_c)[0].reshape(height, width, 3)
                frame = to_uint8(img.float().cpu().numpy())
                frames.append(frame)
                if on_frame is not None:
                    on_frame(len(frames) - 1, frame)
        torch.cuda.synchronize(device)
        secs = time.perf_counter() - t0
    fine_samples, live_samples = counts.read()
    stats = {"seconds": secs, "rays_per_s": num_frames * n / secs, "frames": num_frames,
             "rays_per_frame": n, "fine_samples": fine_samples}
    if grid is not None:
        per_ray = 2 * renderer.n_coarse + renderer.n_fine    # the coarse pass, then coarse + fine positions again
        stats["live_share"] = live_samples / max(num_frames * n * per_ray, 1)
        stats["occupancy_count"] = occupancy_count
        stats["ray_bounds"] = ray_bounds
        stats.update(occupancy_refine=occupancy_refine, occupancy_build_evals=grid.build_evals,
                     occupancy_build_ms=build_ms)
        print(f"occupancy {occupancy}^3: {stats['live_share']:.4f} of the field samples were live")
    return frames, stats


def generate_video(model_input, num_frames, radius, net, model, fine=True, occupancy=None, occupancy_count="host",
                   t_stop_count="host", occupancy_refine=None, occupancy_probe=1, ray_bounds=None):
    """utils.py:481-537 with the same arguments: encode the first source view
    of model_input into `net`, then render the orbit through `model`
    (a RadFieldAndRenderer). A net whose latent was set with encode_latent()
    keeps it (no `images` needed); otherwise the source view is encoded.
    occupancy = RES, occupancy_count = "host" | "device": render_orbit's empty-space skipping (not in the
    reference; off by default). t_stop_count = "host" | "device": where render_orbit keeps the counts of the
    renderer's early termination (model.renderer.t_stop; "device" needs it set). occupancy_refine = F,
    occupancy_probe = P: render_orbit's hierarchical grid build. ray_bounds = None | "grid": render_orbit's per-ray
    sampling bounds from the grid."""
    intrinsics = model_input["intrinsics"][0:1, 0, ...]
    if "images" in model_input and net.encoder.latent.shape[-1] <= 1:   # no latent yet
        gt = model_input["images"]
        _, _, sl2, _ = gt.shape
        sl = int(np.sqrt(sl2))
        src = gt[0:1, 0:1, ...].reshape(1, -1, sl, sl, 3).permute(0, 1, 4, 2, 3)
        net.encode(src, model_input["cam2world"][0:1, 0:1, ...], model_input["focal"][0, 0], model_input["c"][0, 0, :])
    sl = int(model_input.get("resolution", 0)) or int(np.sqrt(model_input["images"].shape[2]))
    # (render_orbit sets the renderer's t_stop for its frames: None as before, the renderer's own in device mode)
    t_stop = getattr(model.renderer, "t_stop", None) if t_stop_count == "device" else None
    frames, stats = render_orbit(model.renderer, net, intrinsics, num_frames, radius, sl, fine=fine,
                                 t_stop=t_stop, occupancy=occupancy,
                                 occupancy_count=occupancy_count, t_stop_count=t_stop_count,
                                 occupancy_refine=occupancy_refine, occupancy_probe=occupancy_probe,
                                 ray_bounds=ray_bounds)
    print(f"it takes {stats['seconds']} seconds to render a video")
    return frames


def write_ppm(path, frame):
    """Binary PPM (P6) of a uint8 (H, W, 3) frame."""
    h, w, _ = frame.shape
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(np.ascontiguousarray(frame, dtype=np.uint8).tobytes())
