"""Reference of avr_occ_ray_bounds (csrc/occupancy_bounds.hip, include/avr.h "occupancy grid: per-ray bounds") in
numpy, float64, by brute force over the occupied cells. Nothing here imports avr: the contract is restated.

For ray r over [near, far], with "live" the test of occupancy_ref.classify (fp32 point, fp32 cell coordinates):
  range  near <= t_near[r] <= t_far[r] <= far;
  (S)    every fp32 z in [near, far] that is live has t_near[r] <= z <= t_far[r]; a ray with a non-finite component
         gets exactly (near, far);
  (T)    [a, b] = the hull of the ray's intersections with the occupied cells (closed boxes), clipped to [near, far];
         slack = sqrt(3) * max(cell edge) / |rd|; a clear hit -- a ray that crosses, within [near, far], some occupied
         cell shrunk by 1/8 of its edge on every side -- has t_near >= a - slack and t_far <= b + slack;
  (M)    a clear miss -- a ray that misses, within [near, far], every occupied cell grown by 1/8 of its edge on every
         side -- gets exactly (near, far);
  a ray that is neither (in between) may get either answer: the range and (S) hold for it.
The ray sets of the GPU tests are made here (cases()), so that the CPU test can assert that at most 10 % of each set
is in between: the rest is checked against (T) or (M)."""
import functools

import numpy as np

import occupancy_ref as ref

F = np.float32
MARGIN = 0.125          # of a cell edge: the shrink of a clear hit, the growth of a clear miss
PINHOLE = (0.0, 0.0, -1.3)
NEAR, FAR = 0.8, 1.8
LO, HI, RES = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (32, 32, 32)


def edges(lo, hi, res):
    lo, hi = np.asarray(lo, F).astype(np.float64), np.asarray(hi, F).astype(np.float64)
    return (hi - lo) / np.asarray(res, np.float64)


def slack(rd, lo, hi, res):
    """(R,) float64: sqrt(3) * max cell edge / |rd|."""
    n = np.linalg.norm(np.asarray(rd, np.float64), axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(3.0) * edges(lo, hi, res).max() / n


def hull(occ, lo, hi, ro, rd, near, far, grow=0.0):
    """-> hit (R,) bool, a, b (R,) float64: the hull over the occupied cells, each grown by `grow` cell edges on every
    side (negative: shrunk), of the ray's intersections with them, clipped to [near, far]; a, b = near, far where
    there is none. Slab test per cell in float64; a zero direction component is inside a slab or beside it for all
    t. Rays with a non-finite component: hit False."""
    rz, ry, rx = occ.shape
    near, far = float(F(near)), float(F(far))      # the entry's two floats
    e = edges(lo, hi, (rx, ry, rz))
    lo64 = np.asarray(lo, F).astype(np.float64)
    iz, iy, ix = np.nonzero(occ)
    idx = np.stack([ix, iy, iz], -1).astype(np.float64)                    # (M, 3)
    c_lo = lo64 + (idx - grow) * e
    c_hi = lo64 + (idx + 1.0 + grow) * e
    o, d = np.asarray(ro, F).astype(np.float64), np.asarray(rd, F).astype(np.float64)
    R = o.shape[0]
    finite = np.isfinite(o).all(-1) & np.isfinite(d).all(-1)
    o, d = np.where(finite[:, None], o, 0.0), np.where(finite[:, None], d, 0.0)
    t_in = np.full((R, len(idx)), near)
    t_out = np.full((R, len(idx)), far)
    for a in range(3):
        oa, da = o[:, a:a + 1], d[:, a:a + 1]
        zero = da == 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            t1, t2 = (c_lo[None, :, a] - oa) / da, (c_hi[None, :, a] - oa) / da
        inside = (oa >= c_lo[None, :, a]) & (oa <= c_hi[None, :, a])
        t_a = np.where(zero, np.where(inside, -np.inf, np.inf), np.minimum(t1, t2))
        t_b = np.where(zero, np.where(inside, np.inf, -np.inf), np.maximum(t1, t2))
        t_in, t_out = np.maximum(t_in, t_a), np.minimum(t_out, t_b)
    cross = (t_in <= t_out) & finite[:, None]
    hit = cross.any(1)
    a_r = np.where(hit, np.where(cross, t_in, np.inf).min(1, initial=np.inf), near)
    b_r = np.where(hit, np.where(cross, t_out, -np.inf).max(1, initial=-np.inf), far)
    return hit, a_r, b_r


def classes(occ, lo, hi, ro, rd, near, far):
    """-> clear_hit, clear_miss (R,) bool and the hull a, b (R,) of the cells as they are. A ray with a non-finite
    component is in neither class."""
    hit, a, b = hull(occ, lo, hi, ro, rd, near, far)
    clear_hit = hull(occ, lo, hi, ro, rd, near, far, -MARGIN)[0]
    finite = np.isfinite(np.asarray(ro, F)).all(-1) & np.isfinite(np.asarray(rd, F)).all(-1)
    clear_miss = ~hull(occ, lo, hi, ro, rd, near, far, MARGIN)[0] & finite
    assert not (clear_hit & ~hit).any() and not (clear_miss & hit).any()
    return clear_hit, clear_miss, a, b


def in_between_share(occ, lo, hi, ro, rd, near, far):
    """Share of the finite rays that are neither a clear hit nor a clear miss."""
    ch, cm, _, _ = classes(occ, lo, hi, ro, rd, near, far)
    finite = np.isfinite(np.asarray(ro, F)).all(-1) & np.isfinite(np.asarray(rd, F)).all(-1)
    return float((finite & ~ch & ~cm).sum()) / max(int(finite.sum()), 1)


def check(case, t_near, t_far):
    """The range, (T), (M) and the non-finite rule of the contract for bounds t_near, t_far (R,) float32 of `case`
    (a dict of cases()); (S) needs the live test and is checked by the caller (live_outside)."""
    near, far = F(case["near"]), F(case["far"])
    t_near, t_far = np.asarray(t_near), np.asarray(t_far)
    assert t_near.dtype == F and t_far.dtype == F
    assert ((near <= t_near) & (t_near <= t_far) & (t_far <= far)).all(), "range"
    ro, rd = case["ro"], case["rd"]
    ch, cm, a, b = classes(case["occ"], case["lo"], case["hi"], ro, rd, near, far)
    s = slack(rd, case["lo"], case["hi"], case["occ"].shape[::-1])
    assert (t_near[ch] >= a[ch] - s[ch]).all() and (t_far[ch] <= b[ch] + s[ch]).all(), "(T)"
    assert (t_near[cm] == near).all() and (t_far[cm] == far).all(), "(M)"
    bad = ~(np.isfinite(ro).all(-1) & np.isfinite(rd).all(-1))
    assert (t_near[bad] == near).all() and (t_far[bad] == far).all(), "non-finite ray"
    return ch, cm


def live_outside(live, z, t_near, t_far):
    """How many live samples (live, z: (R, N)) lie outside [t_near, t_far] (R,): (S) wants none."""
    return int((live & ((z < t_near[:, None]) | (z > t_far[:, None]))).sum())


def dense_z(near, far, n_rays, n):
    """(n_rays, n) float32: the same n depths over [near, far], both ends included, for every ray."""
    z = np.linspace(np.float64(F(near)), np.float64(F(far)), n).astype(F)
    z[0], z[-1] = F(near), F(far)
    return np.broadcast_to(z, (n_rays, n)).copy()


def sphere_grid(radius=0.5):
    return ref.sphere_occ(RES, LO, HI, (0.0, 0.0, 0.0), radius)


def fan(n_side=16, half=0.75, pinhole=PINHOLE):
    """n_side^2 rays from the pinhole through a regular grid over [-half, half]^2 in the plane z = 0; unit
    directions, float32."""
    g = np.linspace(-half, half, n_side)
    yy, xx = np.meshgrid(g, g, indexing="ij")
    target = np.stack([xx, yy, np.zeros_like(xx)], -1).reshape(-1, 3)
    o = np.asarray(pinhole, np.float64)
    d = target - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return np.broadcast_to(o, d.shape).astype(F).copy(), d.astype(F)


def fan_subset(n):
    """n rays of the 16 x 16 fan in a fixed shuffled order (spread over the fan); 256: the fan as it is."""
    ro, rd = fan()
    if n == 256:
        return ro, rd
    order = np.random.default_rng(5).permutation(256)[:n]
    return ro[order], rd[order]


def _case(occ, ro, rd, near=NEAR, far=FAR):
    return {"occ": occ, "lo": LO, "hi": HI, "ro": np.asarray(ro, F), "rd": np.asarray(rd, F), "near": near, "far": far}


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case: every ray set the GPU tests of the kernel run, over 32^3 grids on [-1, 1]^3."""
    rz, ry, rx = RES[2], RES[1], RES[0]
    sphere = sphere_grid()
    out = {f"sphere_fan_{n}": _case(sphere, *fan_subset(n)) for n in (1, 65, 256)}
    out["empty"] = _case(np.zeros((rz, ry, rx), bool), *fan())
    out["full"] = _case(np.ones((rz, ry, rx), bool), *fan())
    # one occupied corner cell, [-1, -0.9375]^3: 16 rays from a point outside the box towards it. Ten through points
    # inside the shrunk cell, five well beside it, and one that grazes it: parallel to its face x = -0.9375, 1/32 of
    # an edge outside (in between: either answer)
    corner = np.zeros((rz, ry, rx), bool)
    corner[0, 0, 0] = True
    e = 2.0 / 32
    o = np.array([-0.5, -0.3, -1.6])
    rng = np.random.default_rng(11)
    inside = -1.0 + e * rng.uniform(0.3, 0.7, (10, 3))
    beside = np.array([-1.0 + e * 0.5, -1.0 + e * 0.5, -1.0 + e * 0.5]) + e * np.array(
        [[2.0, 0, 0], [0, 2.5, 0], [0, 0, 3.0], [1.5, 1.5, 0], [-2.0, 0, 0.0]])
    d = np.concatenate([inside, beside]) - o
    graze_o = np.array([-0.9375 + e / 32, -1.0 + e * 0.5, -1.6])
    ro = np.concatenate([np.broadcast_to(o, d.shape), graze_o[None]])
    d = np.concatenate([d, np.array([[0.0, 0.0, 1.0]])])
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    out["corner_cell"] = _case(corner, ro, d, 0.3, 1.5)
    # rays parallel to the z axis (two zero components) and in a plane y = const (one), through the sphere grid and
    # beside it. x and y run through cell centres (a column of cells is crossed through its middle or not at all);
    # the z offsets of the second eight were chosen so that none grazes a cell either
    k = np.arange(8)
    cx = (np.array([6, 9, 12, 14, 16, 19, 22, 25]) + 0.5) / 16 - 1
    cy = (np.array([24, 21, 19, 17, 15, 12, 10, 7]) + 0.5) / 16 - 1
    ro_z = np.stack([cx, cy, np.full(8, -1.3)], -1)
    rd_z = np.tile(np.array([[0.0, 0.0, 1.0]]), (8, 1))
    ro_y = np.stack([np.full(8, -1.3), cy, -0.4 + 0.07 * k], -1)
    rd_y = np.stack([np.full(8, 0.96), np.zeros(8), 0.28 * np.where(k % 2, 1.0, -1.0)], -1)
    out["axis_parallel"] = _case(sphere, np.concatenate([ro_z, ro_y]), np.concatenate([rd_z, rd_y]))
    # rays that start inside the box, half of them inside the sphere (their hull starts at near)
    rng = np.random.default_rng(12)
    d = rng.normal(0, 1, (16, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    ro = np.where((np.arange(16) % 2 == 0)[:, None], np.array([[0.11, -0.07, 0.13]]), np.array([[0.7, 0.62, -0.66]]))
    out["inside_box"] = _case(sphere, ro, d, 0.05, 1.2)
    # far cuts the hull: the sphere's centre is 1.3 from the pinhole
    out["far_cut"] = _case(sphere, *fan(), NEAR, 1.3)
    ro, rd = fan_subset(16)
    ro, rd = ro.copy(), rd.copy()
    rd[3, 1] = np.nan
    ro[7, 0] = np.inf
    out["non_finite"] = _case(sphere, ro, rd)
    return out
