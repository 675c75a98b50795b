"""Reference of alpha compositing (csrc/composite.hip: avr_composite_fwd / avr_composite_bwd) and of the fine pass with
early ray termination (csrc/march.hip, avr.ops.march_fine) in plain torch, in a dtype the caller passes: torch.float64
is the reference the kernels are held to, torch.float32 on the kernel's device the yardstick (the same expression in
the kernels' own number format, differentiated by autograd). Nothing here imports avr: volume_integral
(renderers.py:69-119) is restated, z (R, N) and field (R, N, 4) = (r, g, b, sigma):

    d_n = z_{n+1} - z_n, d_{N-1} = 1e10        alpha = 1 - exp(-sigma d)      t = 1 - alpha + 1e-10
    T_n = prod_{m<n} t_m                       w = alpha T                    zz_n = z_{n+1}, zz_{N-1} = infinity
    rgb = sum w c (+ 1 - sum w)                dist = sum w zz

`infinity` and `t_stop` reach the kernels as C floats, so they are rounded to fp32 before use; z and the field are the
fp32 inputs converted exactly.

The last column of d sigma is an array of its own. The last interval is 1e10 long, so d sigma[:, N-1] is 1e10 times
the gradient mass that reaches the last sample, and where sigma[N-1] = 0 it is not small. Measured on
tests/golden/g1_volume_integral.npz (N192_wb1, ray 3, last sample, sigma = 0): float64 autograd gives d sigma = -2.287,
the modelled project's fp32 autograd (the golden value) gives -1.769. The ray has an opaque sample (sigma = 1e4) whose
alpha rounds to exactly 1 in fp32, so the transmittance behind it is 1e-10 there and 1.3e-10 in float64, and the last
interval multiplies that difference by 1e10. That is what fp32 means, not a bug of either side. So d sigma is never
compared element by element in relative terms, and d sigma[:, N-1] is judged apart from d sigma[:, :N-1]."""
import numpy as np
import torch

EPS32 = float(torch.finfo(torch.float32).eps)


def _f32(x):
    return float(np.float32(x))


def _terms(z, field, infinity, dtype):
    z, field = z.to(dtype), field.to(dtype)
    d = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], -1)
    alpha = 1.0 - torch.exp(-field[..., 3] * d)
    t = 1.0 - alpha + 1e-10
    zz = torch.cat([z[:, 1:], torch.full_like(z[:, :1], _f32(infinity))], -1)
    return field[..., :3], alpha, t, zz


def volume_integral(z, field, white_back=True, infinity=1.8, dtype=torch.float64):
    """z (R, N), field (R, N, 4) -> rgb (R, 3), dist (R,), w (R, N), computed in dtype."""
    c, alpha, t, zz = _terms(z, field, infinity, dtype)
    T = torch.cumprod(torch.cat([torch.ones_like(t[:, :1]), t], -1), -1)[:, :-1]
    w = alpha * T
    rgb = (w[..., None] * c).sum(-2)
    if white_back:
        rgb = rgb + (1.0 - w.sum(-1, keepdim=True))
    dist = (w * zz).sum(-1)
    return rgb, dist, w


def grads(z, field, g_rgb, g_dist, g_w, white_back=True, infinity=1.8, dtype=torch.float64):
    """Autograd of volume_integral in dtype for the loss sum(rgb g_rgb) + sum(dist g_dist) + sum(w g_w); g_dist and
    g_w may each be None, which drops that term. -> (d field (R, N, 4), d z (R, N)) in dtype."""
    z = z.detach().to(dtype).requires_grad_(True)
    field = field.detach().to(dtype).requires_grad_(True)
    rgb, dist, w = volume_integral(z, field, white_back, infinity, dtype)
    loss = (rgb * g_rgb.to(dtype).reshape(rgb.shape)).sum()
    if g_dist is not None:
        loss = loss + (dist * g_dist.to(dtype).reshape(dist.shape)).sum()
    if g_w is not None:
        loss = loss + (w * g_w.to(dtype).reshape(w.shape)).sum()
    g_field, g_z = torch.autograd.grad(loss, (field, z))
    return g_field, g_z


def march(z, field, chunk, t_stop, white_back=True, infinity=1.8):
    """Early ray termination in float64: every ray consumes its samples front to back in chunks of `chunk`; after a
    chunk that ends at sample e < N it goes on iff float32(T_e) >= float32(t_stop). rgb and dist are the sums over the
    consumed prefix alone, the white background 1 - (sum of the consumed w).
    -> rgb (R, 3), dist (R,), consumed (R,) int64 samples per ray, margin (R,): the smallest |T_e / t_stop - 1| over
    the boundaries the ray reached (inf where it reached none or t_stop = 0), its distance from a flipped decision."""
    c, alpha, t, zz = _terms(z, field, infinity, torch.float64)
    R, N = alpha.shape
    Tincl = torch.cumprod(t, -1)                                   # Tincl[:, e - 1] = T_e
    w = alpha * torch.cat([torch.ones_like(t[:, :1]), Tincl[:, :-1]], -1)
    ts = _f32(t_stop)
    consumed = torch.full((R,), N, dtype=torch.int64, device=z.device)
    margin = torch.full((R,), float("inf"), dtype=torch.float64, device=z.device)
    alive = torch.ones(R, dtype=torch.bool, device=z.device)
    for e in range(chunk, N, chunk):
        Te = Tincl[:, e - 1]
        if ts > 0:
            margin = torch.where(alive, torch.minimum(margin, (Te / ts - 1.0).abs()), margin)
        stop = alive & (Te.to(torch.float32) < torch.tensor(ts, dtype=torch.float32, device=z.device))
        consumed = torch.where(stop, torch.full_like(consumed, e), consumed)
        alive = alive & ~stop
    keep = torch.arange(N, device=z.device)[None, :] < consumed[:, None]
    w = torch.where(keep, w, torch.zeros_like(w))
    rgb = (w[..., None] * c).sum(-2)
    if white_back:
        rgb = rgb + (1.0 - w.sum(-1, keepdim=True))
    dist = (w * zz).sum(-1)
    return rgb, dist, consumed, margin


# ---------------------------------------------------------------------------------------------------------- inputs
# Shared by tests/test_composite_ref_cpu.py (their conditions) and tests/test_gpu_composite.py (the kernels).

def ray_inputs(R, N, s, seed):
    """z sorted uniform in [0.8, 1.8], sigma = max(N(0, s), 0) with every 5th ray all zero and the last sample raised by
    0.5 (d sigma[:, N-1] is then exactly 0: the 1e10 column has cases of its own), rgb uniform, gradients standard
    normal. -> z (R, N), field (R, N, 4), g_rgb (R, 3), g_dist (R,), g_w (R, N), fp32 CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    z = torch.sort(0.8 + torch.rand(R, N, generator=g), -1)[0]
    sigma = (torch.randn(R, N, generator=g) * s).clamp_min(0.0)
    sigma[::5] = 0.0
    sigma[:, -1] += 0.5
    field = torch.cat([torch.rand(R, N, 3, generator=g), sigma[..., None]], -1)
    return z, field, torch.randn(R, 3, generator=g), torch.randn(R, generator=g), torch.randn(R, N, generator=g)


MARCH_K = ((7.0, 11.0, 13.0), (-9.0, 5.0, 17.0), (15.0, -8.0, 6.0))
MARCH_R, MARCH_SEED, MARCH_T_STOP, MARCH_MARGIN = 1001, 6, 1e-3, 1e-4
MARCH_CASES = [(20, 1), (100, 16), (100, 37), (100, 64), (208, 16), (208, 37), (208, 64)]     # (N, chunk)


def march_liveness(consumed, N, chunk):
    """How many rays stopped after the first chunk, after a later one, and never."""
    first = int((consumed == min(chunk, N)).sum()) if chunk < N else 0
    never = int((consumed == N).sum())
    return first, consumed.numel() - first - never, never


def march_rays(R, N, seed):
    """Rays with distinct origins and directions whose mid points (z = 1.3) lie in a cube of side 1 about the origin,
    and jittered sorted samples in [0.8, 1.8]. -> ro (R, 3), rd (R, 3), z (R, N), fp32 CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    rd = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    ro = (torch.rand(R, 3, generator=g) - 0.5) - 1.3 * rd
    z = 0.8 + (torch.arange(N, dtype=torch.float32)[None, :] + torch.rand(R, N, generator=g)) / N
    return ro, rd, z


def march_field(ro, rd, z, amp):
    """The march tests' field, from the rays themselves with elementwise torch ops (so a gathered chunk of rays gives,
    element for element, the values of the full grid): at p = ro + rd z, rgb_j = 0.5 + 0.5 sin(K_j . p) and sigma =
    amp exp(-|p|^2 / 0.2^2), a bump at the origin that rays meet at different depths or miss.
    ro, rd (n, 3), z (n, C) -> (n, C, 4)."""
    p = ro[:, None, :] + rd[:, None, :] * z[:, :, None]
    ch = []
    for k in MARCH_K:
        ch.append(0.5 + 0.5 * torch.sin(k[0] * p[..., 0] + k[1] * p[..., 1] + k[2] * p[..., 2]))
    r2 = p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1] + p[..., 2] * p[..., 2]
    ch.append(amp * torch.exp(-r2 / (0.2 * 0.2)))
    return torch.stack(ch, -1)


def march_amp(N):
    """sigma's peak such that the densest sample has an optical depth of about 10 (d is about 1 / N): a ray that
    starts in the bump's core falls below 1e-3 (optical depth 6.9) within its first sample, so some rays stop after
    the first chunk even where a chunk is one sample; rays that graze the bump stop after many, rays that miss it
    never."""
    return 10.0 * N


def random_poses(shape, seed):
    """Rigid cam2world matrices (*shape, 4, 4) fp32: a random rotation (QR of a normal matrix) and a translation."""
    g = torch.Generator().manual_seed(seed)
    q, r = torch.linalg.qr(torch.randn(*shape, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1))[..., None, :]
    c2w = torch.zeros(*shape, 4, 4, dtype=torch.float64)
    c2w[..., :3, :3] = q
    c2w[..., :3, 3] = torch.randn(*shape, 3, generator=g, dtype=torch.float64)
    c2w[..., 3, 3] = 1.0
    return c2w.to(torch.float32)


def depth_of_world(world, c2w):
    """depth_from_world (utils.py:358-361) in world's dtype: -(inv(c2w) [world, 1])_z. world (SB, R, 3),
    c2w (SB, R, 4, 4) (may be an expand)."""
    row = torch.linalg.inv(c2w.to(world.dtype))[..., 2, :]
    return -((row[..., :3] * world).sum(-1) + row[..., 3])
