"""csrc/composite.hip's backward, the early-termination march (csrc/march.hip) and the depth conversion's gradients
against tests/composite_ref.py in float64. Needs an MI355X: every test is marked gpu.

The accuracy bar is the project's ("2 x PyTorch fp32's error"): for each output array as a whole,
max|hip - f64| <= 2 max|torch_fp32 - f64| + eps32 max|f64|, torch_fp32 being the same expression differentiated by
autograd in fp32 on the GPU. d rgb, d sigma[:, :N-1], d sigma[:, N-1] (the 1e10 interval, see composite_ref) and d z
are arrays of their own. Every test prints its three numbers per array before it asserts."""
import numpy as np
import pytest
import torch

import composite_ref as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import avr
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a HIP device")
    avr.load_library()


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


class Bar:
    """Collects the arrays of one test: prints each, fails at the end with every array that missed."""

    def __init__(self, label):
        self.label, self.missed = label, []

    def add(self, kind, hip, f32, f64):
        if f64.numel() == 0:
            return
        f64 = f64.double()
        assert bool(torch.isfinite(hip).all()), f"{self.label} {kind}: not finite"
        eh, eb = float((hip.double() - f64).abs().max()), float((f32.double() - f64).abs().max())
        s = float(f64.abs().max())
        bound = 2.0 * eb + C.EPS32 * s
        ratio = eh / bound if bound > 0 else (0.0 if eh == 0 else float("inf"))
        print(f"bar {self.label} | {kind} | hip {eh:.3e} fp32 {eb:.3e} max {s:.3e} bound {bound:.3e} ratio {ratio:.3f}")
        if not eh <= bound:
            self.missed.append((kind, eh, eb, s))

    def add_grads(self, gf, gz, ref32, ref64):
        """d field (R, N, 4) and d z (R, N) of the kernel against (d field, d z) of the fp32 and float64 autograd."""
        for kind, sl in (("d rgb", (Ellipsis, slice(0, 3))), ("d sigma[:, :N-1]", (slice(None), slice(0, -1), 3)),
                         ("d sigma[:, N-1]", (slice(None), -1, 3))):
            if gf is not None:
                self.add(kind, gf[sl], ref32[0][sl], ref64[0][sl])
        if gz is not None:
            self.add("d z", gz, ref32[1], ref64[1])

    def check(self):
        assert not self.missed, f"{self.label}: {self.missed}"


def _hip_and_refs(z, field, g_rgb, g_dist, g_w, wb):
    from avr import ops
    z, field, g_rgb, g_dist, g_w = _dev(z, field, g_rgb, g_dist, g_w)
    gf, gz = ops.composite_bwd(z, field, g_rgb, g_dist, g_w, bool(wb), want_grad_z=True)
    assert gf.shape == z.shape + (4,) and gz.shape == z.shape
    ref32 = C.grads(z, field, g_rgb, g_dist, g_w, bool(wb), dtype=F32)
    ref64 = C.grads(z, field, g_rgb, g_dist, g_w, bool(wb), dtype=F64)
    return gf, gz, ref32, ref64


# ------------------------------------------------------------------------------- a. backward over rounds and edges
BWD_N = [1, 2, 63, 64, 65, 130, 208, 333, 1024]
BWD_CASES = [(N, wb, gd, True) for N in BWD_N for wb in (0, 1) for gd in (True, False)] \
    + [(N, wb, gd, False) for N in (65, 208) for wb in (0, 1) for gd in (True, False)]
BOUNDARY = (63, 64, 65, 127, 128, 129)


@pytest.mark.parametrize("N,wb,with_dist,with_w", BWD_CASES)
def test_composite_bwd_rounds(N, wb, with_dist, with_w):
    """composite_bwd_kernel with grad_z over one round, whole rounds and a ragged round after full ones (65, 130, 208 =
    the default fine pass, 333), the single sample, and N = 1024, whose 4 * 1024 * 16 bytes are the whole 64 KiB of
    dynamic LDS a launch may ask for without raising the kernel's attribute; grad_dist and grad_w each given or
    null; 37 rays, so the last workgroup holds one. sigma's scale is 3 and 30. Beyond the four arrays, d z at the
    samples either side of a round boundary meets the bar with both maxima taken over its ray: a wrong carry between
    rounds is an O(1) error there that a whole-array maximum taken elsewhere could hide."""
    R = 37
    bar = Bar(f"bwd N {N} wb {wb} g_dist {with_dist} g_w {with_w}")
    tight = []
    for s in (3.0, 30.0):
        z, field, g_rgb, g_dist, g_w = C.ray_inputs(R, N, s, 1000 * N + int(s))
        gf, gz, ref32, ref64 = _hip_and_refs(z, field, g_rgb, g_dist if with_dist else None,
                                             g_w if with_w else None, wb)
        bar.label = f"bwd N {N} wb {wb} g_dist {with_dist} g_w {with_w} s {s:g}"
        bar.add_grads(gf, gz, ref32, ref64)
        assert bool((gf[:, -1, 3] == 0).all())      # sigma[N-1] >= 0.5 over 1e10: the column is exactly 0 here
        if N > 64:
            idx = [n for n in BOUNDARY if n < N]
            eh = (gz.double() - ref64[1]).abs()[:, idx]
            bound = 2.0 * (ref32[1].double() - ref64[1]).abs().amax(-1) + C.EPS32 * ref64[1].abs().amax(-1)
            bound = bound[:, None].expand_as(eh)
            ratio = float(torch.where(eh == 0, torch.zeros_like(eh), eh / bound).max())
            print(f"bar {bar.label} | d z at round boundaries, per ray | ratio {ratio:.3f}")
            if not bool((eh <= bound).all()):
                tight.append((s, ratio))
    bar.check()
    assert not tight, f"d z at samples {BOUNDARY} misses its ray's bar: {tight}"


# ----------------------------------------------------------------------------------------- b. grad_z off equals on
@pytest.mark.parametrize("wb", [0, 1])
def test_composite_bwd_grad_z_off_is_bit_equal(wb):
    from avr import ops
    z, field, g_rgb, g_dist, g_w = _dev(*C.ray_inputs(37, 130, 30.0, 77))
    on, gz = ops.composite_bwd(z, field, g_rgb, g_dist, g_w, bool(wb), want_grad_z=True)
    off = ops.composite_bwd(z, field, g_rgb, g_dist, g_w, bool(wb), want_grad_z=False)
    assert gz is not None and torch.equal(on, off)


# ------------------------------------------------------------------------------------------------------- c. edges
def _edge_inputs(case, N):
    z, field, g_rgb, g_dist, g_w = C.ray_inputs(5, N, 3.0, 31)
    keep = [1, 2, 3]                                 # not the all-zero ray of ray_inputs
    z, field, g_rgb, g_dist, g_w = z[keep], field[keep].clone(), g_rgb[keep], g_dist[keep], g_w[keep]
    if case == "last_sigma_zero":                    # d sigma[N-1] = 1e10 x the gradient mass that arrives
        field[:, -1, 3] = 0.0
    elif case == "all_sigma_zero":
        field[..., 3] = 0.0
    elif case == "opaque_mid_sample":                # fp32 alpha = 1, t = 1e-10: S / t at its smallest divisor
        field[:, 40, 3] = 1e4
    elif case == "equal_z":                          # d = 0 inside a round and across the round boundary
        z = z.clone()
        z[:, 11] = z[:, 10]
        z[:, 64] = z[:, 63]
    return z, field, g_rgb, g_dist, g_w


@pytest.mark.parametrize("case", ["last_sigma_zero", "all_sigma_zero", "opaque_mid_sample", "equal_z"])
@pytest.mark.parametrize("wb", [0, 1])
def test_composite_bwd_edges(case, wb):
    """Three rays of N = 70 with the edge on each; all outputs finite, each array within the bar."""
    bar = Bar(f"edge {case} wb {wb}")
    gf, gz, ref32, ref64 = _hip_and_refs(*_edge_inputs(case, 70), wb)
    if case in ("last_sigma_zero", "all_sigma_zero"):
        assert float(gf[:, -1, 3].abs().min()) > 1.0          # the column is live
    bar.add_grads(gf, gz, ref32, ref64)
    bar.check()


@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("wb", [0, 1])
def test_composite_bwd_one_ray_and_one_full_workgroup(R, wb):
    bar = Bar(f"edge R {R} wb {wb}")
    inputs = [t[1:] for t in C.ray_inputs(R + 1, 65, 3.0, 32)]
    gf, gz, ref32, ref64 = _hip_and_refs(*inputs, wb)
    assert gf.shape == (R, 65, 4) and gz.shape == (R, 65)
    bar.add_grads(gf, gz, ref32, ref64)
    bar.check()


# --------------------------------------------------------------------------------------------- d. autograd surface
@pytest.mark.parametrize("case", ["rgb_sum", "w_only", "dist_only", "z_only", "field_only"])
def test_composite_autograd_surface(case):
    """ops.composite / _Composite at N = 70, R = 9: whatever torch hands backward() for the outputs the loss leaves
    out (None or zeros) and for rgb.sum() (an expanded stride-0 gradient), the gradients are the float64 reference's
    for that loss; an input that does not require grad gets None."""
    from avr import ops
    R, N = 9, 70
    wb = case != "dist_only"
    z0, f0, g_rgb, g_dist, g_w = _dev(*C.ray_inputs(R, N, 3.0, 41))
    z = z0.clone().requires_grad_(case != "field_only")
    field = f0.clone().requires_grad_(case != "z_only")
    rgb, dist, w = ops.composite(z, field, wb)
    if case == "rgb_sum":
        loss, ref_g = rgb.sum(), (torch.ones_like(g_rgb), None, None)
    elif case == "w_only":
        loss, ref_g = (w * g_w).sum(), (torch.zeros_like(g_rgb), None, g_w)
    elif case == "dist_only":
        loss, ref_g = (dist * g_dist).sum(), (torch.zeros_like(g_rgb), g_dist, None)
    else:
        loss, ref_g = (rgb * g_rgb).sum() + (dist * g_dist).sum() + (w * g_w).sum(), (g_rgb, g_dist, g_w)
    loss.backward()
    ref32 = C.grads(z0, f0, *ref_g, wb, dtype=F32)
    ref64 = C.grads(z0, f0, *ref_g, wb, dtype=F64)
    if case == "z_only":
        assert field.grad is None
    else:
        assert field.grad.shape == (R, N, 4)
    if case == "field_only":
        assert z.grad is None
    else:
        assert z.grad.shape == (R, N)
    bar = Bar(f"autograd {case}")
    bar.add_grads(field.grad, z.grad, ref32, ref64)
    bar.check()


# ------------------------------------------------------------------------------------ e. early-termination march
def _march_inputs(N):
    ro, rd, z = _dev(*C.march_rays(C.MARCH_R, N, C.MARCH_SEED))
    amp = C.march_amp(N)
    return ro, rd, z, C.march_field(ro, rd, z, amp), lambda a, b, c: C.march_field(a, b, c, amp).reshape(-1, 4)


@pytest.mark.parametrize("N,chunk", C.MARCH_CASES)
@pytest.mark.parametrize("wb", [False, True])
def test_march_without_stop_is_the_full_integral(N, chunk, wb):
    """t_stop = 0 stops nothing ((float)T >= 0 always): every sample of all 1001 rays is evaluated once, in chunks of
    1, 16, 37 and 64 with a short last chunk, and ray r's state receives ray r's samples: the field is computed
    from the gathered (ro, rd, z) themselves. rgb and dist within 2e-6, the forward tests' bound, of the float64
    integral and of composite_fwd on the same field."""
    from avr import ops
    ro, rd, z, field, fn = _march_inputs(N)
    rgb, dist, evaluated = ops.march_fine(ro, rd, z, fn, 0.0, wb, chunk=chunk)
    assert evaluated == C.MARCH_R * N
    r_rgb, r_dist, _ = C.volume_integral(z, field, wb)
    c_rgb, c_dist, _ = ops.composite_fwd(z, field, wb)
    e = [float((a.double() - b.double()).abs().max())
         for a, b in ((rgb, r_rgb), (dist, r_dist), (rgb, c_rgb), (dist, c_dist))]
    print(f"march N {N} chunk {chunk} wb {wb} t_stop 0: rgb {e[0]:.2e} dist {e[1]:.2e} vs float64, rgb {e[2]:.2e} "
          f"dist {e[3]:.2e} vs composite_fwd")
    assert max(e) <= 2e-6, e


@pytest.mark.parametrize("N,chunk", C.MARCH_CASES)
@pytest.mark.parametrize("wb", [False, True])
def test_march_stops_where_the_reference_stops(N, chunk, wb):
    """t_stop = 1e-3. A ray is decided if no boundary it reached has |T / t_stop - 1| <= 1e-4 in the reference: the
    kernel's T is a float64 product of fp32 factors rounded once, and a factor's absolute error of 2^-25 (alpha = 1 -
    exp rounded below 1) makes T's relative error at most 2^-25 sum 1 / t_m, which for T near 1e-3 stays below 4e-5.
    At most 1 % of the rays may be undecided (none are on the CPU, tests/test_composite_ref_cpu.py); decided rays
    carry the reference's prefix sums to 2e-6; the number of evaluated samples is the reference's, exactly when no ray
    is undecided, otherwise within N - chunk per undecided ray (it agrees with the reference up to its first
    boundary at least). The reference must have rays that stop after the first chunk, later, and never. A second
    run gives the same bits: the active list's order may differ between runs, no ray's arithmetic may."""
    from avr import ops
    ro, rd, z, field, fn = _march_inputs(N)
    r_rgb, r_dist, consumed, margin = C.march(z, field, chunk, C.MARCH_T_STOP, wb)
    first, middle, never = C.march_liveness(consumed, N, chunk)
    assert first > 0 and never > 0 and (middle > 0 or len(range(chunk, N, chunk)) < 2), (first, middle, never)
    decided = margin > C.MARCH_MARGIN
    undecided = C.MARCH_R - int(decided.sum())
    rgb, dist, evaluated = ops.march_fine(ro, rd, z, fn, C.MARCH_T_STOP, wb, chunk=chunk)
    e_rgb = float((rgb.double() - r_rgb)[decided].abs().max())
    e_dist = float((dist.double() - r_dist)[decided].abs().max())
    want = int(consumed.sum())
    print(f"march N {N} chunk {chunk} wb {wb} t_stop 1e-3: undecided {undecided}, stop first {first} middle {middle} "
          f"never {never}, evaluated {evaluated} reference {want} of {C.MARCH_R * N}, rgb {e_rgb:.2e} "
          f"dist {e_dist:.2e}")
    assert undecided <= C.MARCH_R // 100
    assert e_rgb <= 2e-6 and e_dist <= 2e-6
    assert abs(evaluated - want) <= undecided * (N - chunk)
    rgb2, dist2, evaluated2 = ops.march_fine(ro, rd, z, fn, C.MARCH_T_STOP, wb, chunk=chunk)
    assert evaluated2 == evaluated and torch.equal(rgb2, rgb) and torch.equal(dist2, dist)


# ----------------------------------------------------------------------------------- f. depth conversion gradient
@pytest.mark.parametrize("layout", ["per_ray", "per_batch", "single"])
def test_depth_conversion_gradients(layout):
    """ops.depth_from_world (depth of ro + rd dist and, through _Depth, d depth / d dist) and ops.depth_of_points
    (depth of explicit points and, through _DepthOfPoints, d depth / d world) against -(inv(c2w) [x, 1])_z in
    float64, with one pose per ray, one per batch (the stride-0 expand the callers pass) and one for all
    (sb_stride = ray_stride = 0)."""
    from avr import ops
    SB, R = 2, 300
    if layout == "per_ray":
        c2w = C.random_poses((SB, R), 51).to(DEV)
    elif layout == "per_batch":
        c2w = C.random_poses((SB, 1), 52).to(DEV).expand(SB, R, 4, 4)
    else:
        c2w = C.random_poses((1, 1), 53).to(DEV).expand(SB, R, 4, 4)
    info = ops._c2w_view(c2w)
    assert (info[1] == 0) == (layout == "single") and (info[2] == 0) == (layout != "per_ray")
    g = torch.Generator().manual_seed(54)
    ro = torch.randn(SB, R, 3, generator=g).to(DEV)
    rd = torch.nn.functional.normalize(torch.randn(SB, R, 3, generator=g), dim=-1).to(DEV)
    dist0 = (0.8 + torch.rand(SB, R, generator=g)).to(DEV)
    gd, gp = torch.randn(SB, R, generator=g).to(DEV), torch.randn(SB, R, generator=g).to(DEV)
    world0 = (ro + rd * dist0[..., None]).contiguous()

    def ref(dtype):
        d = dist0.to(dtype).requires_grad_(True)
        dep = C.depth_of_world(ro.to(dtype) + rd.to(dtype) * d[..., None], c2w)
        x = world0.to(dtype).requires_grad_(True)
        dep_p = C.depth_of_world(x, c2w)
        (g_d,) = torch.autograd.grad((dep * gd.to(dtype)).sum(), d)
        (g_x,) = torch.autograd.grad((dep_p * gp.to(dtype)).sum(), x)
        return dep.detach(), g_d, dep_p.detach(), g_x

    dist = dist0.clone().requires_grad_(True)
    dep = ops.depth_from_world(ro, rd, dist, info)
    (dep * gd).sum().backward()
    world = world0.clone().requires_grad_(True)
    dep_p = ops.depth_of_points(world, info)
    (dep_p * gp).sum().backward()
    assert torch.equal(ops.depth_from_world(ro, rd, dist0, info), dep.detach())
    assert torch.equal(ops.depth_of_points(world0, info), dep_p.detach())
    bar = Bar(f"depth {layout}")
    r32, r64 = ref(F32), ref(F64)
    for i, (kind, hip) in enumerate((("depth of ro + rd dist", dep.detach()), ("d depth / d dist", dist.grad),
                                     ("depth of points", dep_p.detach()), ("d depth / d world", world.grad))):
        assert hip.shape == r64[i].shape
        bar.add(kind, hip, r32[i], r64[i])
    bar.check()
