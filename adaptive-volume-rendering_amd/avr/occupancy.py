"""Occupancy-grid empty-space skipping for VolumeRenderer inference (not in the reference; DESIGN.md "Occupancy
grid", include/avr.h "occupancy grid").

    grid = OccupancyGrid.from_field(net, lo=(-1, -1, -1), hi=(1, 1, 1), res=(128, 128, 128))
    renderer.occupancy = grid                     # or a list with one grid per scene; None (default): ungated
    rgb_c, rgb_f, depth, _ = renderer(cam2world, intrinsics, x_pix, net)      # under torch.no_grad()

A grid is a bit per cell of an axis-aligned box. A sample whose point falls in a clear cell, or outside the box, is
not evaluated: the composite sees exactly 0.0 in all four channels for it (sigma = 0). The live samples are compacted
in ray-major sample order, evaluated by one avr_field_fwd_points launch and scattered back (gated_field): classify
-> cumsum -> one host read of the live count -> compact -> field -> expand. The host read makes that path eager only:
it cannot be recorded in a HIP-graph capture.

    renderer.occupancy_count = "device"           # "host" (default): the chain above

keeps the live count on the device instead (gated_field(count="device")): classify -> avr_occ_scan ->
avr_occ_compact_counted -> avr_field_fwd_points_counted -> avr_occ_expand_counted, no host read and no torch kernel,
so the gated frame can be captured (avr.graphs.GraphedRenderer) and OccupancyGrid.copy_ gives a captured graph a
new grid without a new capture. Its price is memory: the compacted buffers are sized for the worst case, R * N rows
(40 B per sample), where the host-read path allocates the live share only.

What the render loses is what the grid calls empty. from_field marks a cell from sigma at its centre alone, for a
handful of view directions, so a density feature thinner than a cell, or one that only other view directions see, can
be missed: `dilate` (cells of safety margin around every occupied cell) and `sigma_thr` trade that risk against the
live share. sigma_thr = 0.0 (the default) keeps every cell where any evaluated sigma is above exactly zero after the
ReLU; a positive threshold also drops faint fog, which changes the image by up to the weight that fog carried.

    grid = OccupancyGrid.from_field(net, lo, hi, res=(128, 128, 128), refine=4)      # hierarchical build

builds a coarse grid densely first (res / refine, here 32^3: 1/64 of the cells) and evaluates fine cells only under
its live cells (refine_from_field: children -> scan -> one host read of the candidate count M -> points -> field on
the point list per MLP and direction -> flag_sigma -> build_sparse); every buffer is sized by M, no (K, cells) plane
buffer is made. A fine cell under a clear coarse cell is never evaluated and counts as sigma = 0, so what the coarse
stage calls empty is lost whatever the fine field holds there. The coarse stage judges a coarse cell at its centre
alone -- one point per refine^3 fine cells -- so a feature narrower than a coarse cell that misses the centre of
every coarse cell it crosses is dropped, where the dense build would have met it at a fine centre. `coarse_dilate`
(default 1: a coarse cell stays live next to any live one, a margin of `refine` fine cells) and `coarse_probe` = p
(the coarse stage evaluated at res * p / refine and OR-ed down by p: p^3 interior points per coarse cell at p^3
times the coarse cost) trade that risk against the candidate share; neither is a guarantee.
cells_missing_from(dense) counts what a hierarchical grid dropped relative to a dense one.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import OccGrid, call, ptr, require_device, stream_of
from .cache import _version_key

F32 = torch.float32
AXIS_DIRS = ((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0))
REFINE_FACTORS = (2, 4, 8)   # fine cells per coarse cell and axis of a hierarchical build (avr_occ_children)
PROBE_FACTORS = (1, 2, 4)    # cells per coarse cell and axis of its dense probe (avr_occ_downsample)


def _check_res(res):
    res = tuple(int(r) for r in res)
    if len(res) != 3 or not all(1 <= r <= _lib.OCC_MAX_RES for r in res) or res[0] % 32:
        raise ValueError(f"occupancy grid resolution {res}: three values in 1..{_lib.OCC_MAX_RES}, the first a "
                         "multiple of 32")
    return res


def n_words(res):
    return (res[0] // 32) * res[1] * res[2]


def field_key(net):
    """The version key (avr.cache) of everything the field's values depend on: the parameters and buffers of both
    MLPs, the latent map, the source views. Returns (key, the tensors whose addresses are part of it)."""
    fused = net.fused()
    mlps = [net.mlp_coarse] + ([net.mlp_fine] if net.mlp_fine is not None else [])
    ts = []
    for mlp in mlps:
        _, ps, bs = fused._state(mlp)
        ts += ps + bs
    lat = net.encoder.latent
    srcs = fused._view_sources()
    return (_version_key(ts + [lat]), _version_key(srcs, gen=False), tuple(lat.shape)), ts + [lat] + srcs


class OccupancyGrid:
    """The descriptor and the device bits of one scene's grid: box [lo, hi), res = (rx, ry, rz) cells, bits an int32
    tensor of rx / 32 * ry * rz words (cell (ix, iy, iz) = bit ix % 32 of word (iz * ry + iy) * (rx / 32) + ix / 32).
    key: the field_key() of the net it was built from (from_field), or None for a grid that no net's state can
    make stale (from_sigma, all_occupied)."""

    def __init__(self, lo, hi, res, bits, key=None, keep=None):
        self.res = _check_res(res)
        self.lo = tuple(float(np.float32(v)) for v in lo)
        self.hi = tuple(float(np.float32(v)) for v in hi)
        if len(self.lo) != 3 or len(self.hi) != 3 or not all(h > l for l, h in zip(self.lo, self.hi)):
            raise ValueError(f"occupancy grid box lo {self.lo} hi {self.hi}: need hi > lo on three axes")
        if bits.dtype != torch.int32 or bits.numel() != n_words(self.res):
            raise ValueError(f"occupancy grid bits: {n_words(self.res)} int32 words for res {self.res}")
        self.bits = bits.reshape(-1).contiguous()
        self.key, self._keep = key, keep
        # from_field / refine_from_field: the candidates of a hierarchical build (None: built densely) and the field
        # points evaluated for this grid (None: not built from a field)
        self.n_candidates, self.build_evals = None, None
        self.inv =tuple(float(np.float32(r / (float(h) - float(l)))) for r, l, h in zip(self.res, self.lo, self.hi))
        self.desc = OccGrid((ctypes.c_float * 3)(*self.lo), (ctypes.c_float * 3)(*self.inv),
                            (ctypes.c_int * 3)(*self.res), self.bits.data_ptr())

    @property
    def device(self):
        return self.bits.device

    def copy_(self, other):
        """This grid's bits, key and kept tensors become `other`'s, in place (same box and resolution, else
        ValueError): the bits tensor keeps its address, so a captured graph that reads it (GraphedRenderer with
        occupancy_count = "device") renders with the new grid from its next replay on, without a new capture. The
        copy is ordered on the current stream."""
        if other.res != self.res or other.lo != self.lo or other.hi != self.hi:
            raise ValueError(f"OccupancyGrid.copy_: box {other.lo} .. {other.hi} res {other.res} into box {self.lo} "
                             f".. {self.hi} res {self.res}: the box and the resolution must match")
        self.bits.copy_(other.bits)
        self.key, self._keep = other.key, other._keep
        self.n_candidates, self.build_evals = other.n_candidates, other.build_evals
        return self

    def ray_bounds(self, ro, rd, near, far, out=None):
        """avr_occ_ray_bounds: ro, rd (..., 3) -> (t_near, t_far), each of ro's leading shape: where along [near, far]
        (two floats, near < far) every sample of a ray that this grid calls live lies. A ray that clearly misses the
        occupied cells, or has a non-finite component, gets exactly (near, far) (include/avr.h: safety, tightness,
        miss). out: two contiguous fp32 tensors of one element per ray to write into. Nothing is read back: the call
        may be captured in a graph."""
        shape = ro.shape[:-1]
        ro = ro.reshape(-1, 3).to(F32).contiguous()
        rd = rd.reshape(-1, 3).to(F32).contiguous()
        require_device(ro, rd, self.bits)
        if out is None:
            out = (torch.empty(ro.shape[0], device=ro.device, dtype=F32),
                   torch.empty(ro.shape[0], device=ro.device, dtype=F32))
        t_near, t_far = out
        require_device(t_near, t_far)
        if not all(t.dtype == F32 and t.numel() == ro.shape[0] for t in out):
            raise ValueError(f"OccupancyGrid.ray_bounds: out must be two float32 tensors of {ro.shape[0]} elements")
        call("avr_occ_ray_bounds", ctypes.byref(self.desc), ptr(ro), ptr(rd), ro.shape[0], float(near), float(far),
             ptr(t_near), ptr(t_far), stream_of(ro))
        return t_near.reshape(shape), t_far.reshape(shape)

    def live_fraction(self):
        """Share of the cells whose bit is set (a host read of the bits)."""
        words = self.bits.cpu().numpy().view(np.uint8)
        return float(np.unpackbits(words).sum()) / float(self.res[0] * self.res[1] * self.res[2])

    def stale(self, net):
        """True when the grid was built from a net's field (from_field) and `net`'s parameters, latent map or source
        views are no longer the ones it was built from."""
        return self.key is not None and self.key != field_key(net)[0]

    @classmethod
    def all_occupied(cls, lo, hi, res, device):
        res = _check_res(res)
        return cls(lo, hi, res, torch.full((n_words(res),), -1, dtype=torch.int32, device=device))

    @classmethod
    def from_sigma(cls, sigma_planes, lo, hi, thr, dilate=1, key=None, keep=None):
        """sigma_planes (K, rz, ry, rx) or (rz, ry, rx) fp32 on the device: a cell is set iff any plane at any cell
        within Chebyshev distance `dilate` (0, 1 or 2, clamped at the box faces) has not (sigma <= thr); NaN counts
        as occupied (avr_occ_build)."""
        s = sigma_planes if sigma_planes.dim() == 4 else sigma_planes[None]
        if s.dim() != 4 or s.shape[0] < 1:
            raise ValueError("from_sigma: sigma_planes must be (K, rz, ry, rx) or (rz, ry, rx)")
        if int(dilate) not in (0, 1, 2):
            raise ValueError("from_sigma: dilate must be 0, 1 or 2")
        res = _check_res((s.shape[3], s.shape[2], s.shape[1]))
        s = s.to(F32).contiguous()
        require_device(s)
        bits = torch.empty(n_words(res), dtype=torch.int32, device=s.device)
        call("avr_occ_build", ptr(s), s.shape[0], (ctypes.c_int * 3)(*res), float(thr), int(dilate), ptr(bits),
             stream_of(s))
        return cls(lo, hi, res, bits, key, keep)

    @staticmethod
    def cell_centres(lo, hi, res, device):
        """(rz * ry * rx, 3) fp32 cell centres, x fastest: lo + (i + 0.5) * cell in float64, then rounded."""
        ax = [np.float32(l).astype(np.float64) + (np.arange(r, dtype=np.float64) + 0.5)
              * ((np.float32(h).astype(np.float64) - np.float32(l).astype(np.float64)) / r)
              for l, h, r in zip(lo, hi, res)]
        zz, yy, xx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        return torch.from_numpy(np.stack([xx, yy, zz], -1).reshape(-1, 3).astype(np.float32)).to(device)

    @classmethod
    def from_field(cls, net, lo, hi, res=(128, 128, 128), sigma_thr=0.0, dilate=1, dirs=None, sb=0, chunk=1 << 20,
                   refine=None, coarse_dilate=1, coarse_probe=1):
        """The grid of scene `sb` of a fusable NewPixelNeRFNet: sigma (output channel 3) of both MLPs, coarse and
        fine if present, at every cell centre for every view direction in `dirs` (default: the six axis directions
        -- the MLP sees the view direction, so one is not enough), `chunk` points per field launch, then from_sigma
        over all those planes. The grid records the field_key() it was built under (stale()) and the field points it
        evaluated (build_evals).
        refine = f (2, 4 or 8; None, the default: the dense build above): the hierarchical build of the module
        docstring -- a dense probe at res * coarse_probe / f with dilate = coarse_dilate, probe.downsample(
        coarse_probe), then refine_from_field under that coarse grid; build_evals counts both stages."""
        if refine is not None:
            return cls._from_field_refined(net, lo, hi, res, sigma_thr, dilate, dirs, sb, chunk, refine,
                                           coarse_dilate, coarse_probe)
        from .field import fused_eligible
        if not fused_eligible(net):
            raise ValueError("OccupancyGrid.from_field: the net is not on the single-view fused path")
        res = _check_res(res)
        dev = net.encoder.latent.device
        fused = net.fused()
        dirs = AXIS_DIRS if dirs is None else dirs
        passes = [True] + ([False] if net.mlp_fine is not None else [])
        key, keep = field_key(net)
        with torch.no_grad():
            centres = cls.cell_centres(lo, hi, res, dev)
            n = centres.shape[0]
            planes = torch.empty(len(passes) * len(dirs), n, device=dev, dtype=F32)
            k = 0
            for coarse in passes:
                for d in dirs:
                    vd = torch.tensor([d], device=dev, dtype=F32)
                    for c0 in range(0, n, int(chunk)):
                        p = centres[c0:c0 + int(chunk)]
                        out = fused.forward_points_scene(p, vd.expand(p.shape[0], 3), coarse, sb)
                        planes[k, c0:c0 + p.shape[0]] = out[:, 3]
                    k += 1
            grid = cls.from_sigma(planes.reshape(-1, res[2], res[1], res[0]), lo, hi, sigma_thr, dilate, key, keep)
        grid.build_evals = planes.shape[0] * n
        return grid

    @classmethod
    def _from_field_refined(cls, net, lo, hi, res, sigma_thr, dilate, dirs, sb, chunk, refine, coarse_dilate,
                            coarse_probe):
        res = _check_res(res)
        f, p = int(refine), int(coarse_probe)
        if f not in REFINE_FACTORS or p not in PROBE_FACTORS:
            raise ValueError(f"OccupancyGrid.from_field: refine must be one of {REFINE_FACTORS} (got {refine!r}) and "
                             f"coarse_probe one of {PROBE_FACTORS} (got {coarse_probe!r})")
        if any(r % f for r in res) or (res[0] // f) % 32:
            raise ValueError(f"OccupancyGrid.from_field: res {res} with refine {f}: every value must be divisible by "
                             "it and the coarse res[0] a multiple of 32")
        _check_thr("OccupancyGrid.from_field", sigma_thr)
        probe = cls.from_field(net, lo, hi, tuple(r // f * p for r in res), sigma_thr, coarse_dilate, dirs, sb, chunk)
        coarse = probe.downsample(p)
        grid = cls.refine_from_field(net, coarse, f, sigma_thr, dilate, dirs, sb, chunk, lo=lo, hi=hi)
        grid.build_evals += probe.build_evals
        return grid

    @classmethod
    def refine_from_field(cls, net, coarse, factor, sigma_thr=0.0, dilate=1, dirs=None, sb=0, chunk=1 << 20, lo=None,
                          hi=None):
        """The fine grid of resolution coarse.res * factor (factor 2, 4 or 8) over coarse's box, with the field of
        scene `sb` evaluated only at the centres of the fine cells under coarse's live cells (the candidates, M =
        factor^3 * the live coarse cells, in linear fine-cell order): a fine cell is set iff a candidate within
        `dilate` cells of it has not (sigma <= sigma_thr) for some MLP and direction -- from_field's bits with sigma
        taken as 0 wherever coarse is clear. One host read (M) sizes every buffer; M == 0 launches no field. The
        result carries n_candidates = M and build_evals = M * MLPs * directions, and records field_key(net).
        ValueError: a net off the single-view fused path; a `coarse` that was built from a field and is stale for
        `net` (a grid without a key, such as all_occupied, is accepted); a factor, a fine resolution or a box (lo /
        hi, when given: compared with coarse's as float32) that does not fit; sigma_thr negative or NaN, which would
        call the unevaluated cells occupied."""
        from .field import fused_eligible
        who = "OccupancyGrid.refine_from_field"
        f = int(factor)
        if f not in REFINE_FACTORS:
            raise ValueError(f"{who}: factor must be one of {REFINE_FACTORS}, got {factor!r}")
        if max(coarse.res) * f > _lib.OCC_MAX_RES:
            raise ValueError(f"{who}: coarse res {coarse.res} times {f} exceeds {_lib.OCC_MAX_RES} cells per axis")
        for name, given, own in (("lo", lo, coarse.lo), ("hi", hi, coarse.hi)):
            if given is not None and tuple(float(np.float32(v)) for v in given) != own:
                raise ValueError(f"{who}: box {name} {tuple(given)} is not the coarse grid's {own}")
        if int(dilate) not in (0, 1, 2):
            raise ValueError(f"{who}: dilate must be 0, 1 or 2")
        thr = _check_thr(who, sigma_thr)
        if not fused_eligible(net):
            raise ValueError(f"{who}: the net is not on the single-view fused path")
        if coarse.stale(net):
            raise ValueError(f"{who}: the coarse grid was built from parameters, a latent map or source views that "
                             "have changed since; rebuild it")
        res = tuple(r * f for r in coarse.res)
        dev = net.encoder.latent.device
        fused = net.fused()
        dirs = AXIS_DIRS if dirs is None else dirs
        passes = [True] + ([False] if net.mlp_fine is not None else [])
        key, keep = field_key(net)
        chunk = int(chunk)
        with torch.no_grad():
            mask, counts = children(coarse, f, res)
            offsets, total = scan(counts)
            M = int(total.item())                        # the one host read: it sizes everything below
            flags = None
            if M:
                xyz, vd = child_points(mask, offsets, res, coarse.lo, coarse.hi, M, dirs[0])
                flags = torch.empty(M, dtype=torch.uint8, device=dev)
                k = 0
                for is_coarse in passes:
                    for d in dirs:
                        if k:
                            child_points(mask, offsets, res, coarse.lo, coarse.hi, M, d, xyz=False, viewdirs=vd)
                        for c0 in range(0, M, chunk):
                            out = fused.forward_points_scene(xyz[c0:c0 + chunk], vd[c0:c0 + chunk], is_coarse, sb)
                            flag_sigma(out, thr, k == 0, flags[c0:c0 + chunk])
                        k += 1
            bits = build_sparse(mask, offsets, flags, M, res, int(dilate))
        grid = cls(coarse.lo, coarse.hi, res, bits, key, keep)
        grid.n_candidates, grid.build_evals = M, M * len(passes) * len(dirs)
        return grid

    def downsample(self, p):
        """The grid of resolution res / p (p 1, 2 or 4; every res[a] divisible by it, res[0] / p a multiple of 32)
        over the same box whose cell is set iff any of its p^3 children is (avr_occ_downsample). It keeps this grid's
        key."""
        p = int(p)
        if p not in PROBE_FACTORS or any(r % p for r in self.res) or (self.res[0] // p) % 32:
            raise ValueError(f"OccupancyGrid.downsample: p = {p} with res {self.res}: p must be one of "
                             f"{PROBE_FACTORS}, divide every value and leave res[0] / p a multiple of 32")
        require_device(self.bits)
        res = tuple(r // p for r in self.res)
        bits = torch.empty(n_words(res), dtype=torch.int32, device=self.device)
        call("avr_occ_downsample", ptr(self.bits), (ctypes.c_int * 3)(*self.res), p, ptr(bits), stream_of(bits))
        grid = type(self)(self.lo, self.hi, res, bits, self.key, self._keep)
        grid.build_evals = self.build_evals
        return grid

    def cells_missing_from(self, other):
        """How many cells `other` (same box and resolution, else ValueError) sets that this grid leaves clear: what
        a hierarchical grid dropped relative to a dense one. A host read of both grids' bits."""
        if other.res != self.res or other.lo != self.lo or other.hi != self.hi:
            raise ValueError(f"OccupancyGrid.cells_missing_from: box {other.lo} .. {other.hi} res {other.res} against "
                             f"box {self.lo} .. {self.hi} res {self.res}: the box and the resolution must match")
        mine, theirs = (g.bits.cpu().numpy().view(np.uint8) for g in (self, other))
        return int(np.unpackbits(theirs & ~mine).sum())


def _check_thr(who, sigma_thr):
    thr = float(sigma_thr)
    if not thr >= 0.0:
        raise ValueError(f"{who}: sigma_thr {sigma_thr!r} must be >= 0 for a hierarchical build (a negative or NaN "
                         "threshold would call the cells that are never evaluated occupied)")
    return thr


def children(coarse, factor, res):
    """avr_occ_children: the fine cells of `res` under coarse's live cells -> mask (ry * rz, ceil(rx / 64)) int64
    (the uint64 words' bits), counts (ry * rz,) int32."""
    require_device(coarse.bits)
    rows = res[1] * res[2]
    mask = torch.empty(rows, (res[0] + 63) // 64, device=coarse.device, dtype=torch.int64)
    counts = torch.empty(rows, device=coarse.device, dtype=torch.int32)
    call("avr_occ_children", ctypes.byref(coarse.desc), int(factor), (ctypes.c_int * 3)(*res), ptr(mask), ptr(counts),
         stream_of(mask))
    return mask, counts


def refine_axes(lo, hi, res):
    """lo64[a] = double(float32 lo[a]) and step[a] = (hi64[a] - lo64[a]) / res[a], in double: cell_centres' terms."""
    lo64 = [float(np.float32(v)) for v in lo]
    return lo64, [(float(np.float32(h)) - l) / r for l, h, r in zip(lo64, hi, res)]


def child_points(mask, offsets, res, lo, hi, n_live, direction, xyz=None, viewdirs=None):
    """avr_occ_child_points -> xyz, viewdirs (n_live, 3): the candidates' centres (the rows of cell_centres at the
    candidates, bit for bit) and `direction` in every row. xyz / viewdirs: a tensor to write into, None to allocate
    one, False to leave that output out (not both)."""
    make = lambda t: torch.empty(n_live, 3, device=mask.device, dtype=F32) if t is None else t  # noqa: E731
    xyz, viewdirs = (None if t is False else make(t) for t in (xyz, viewdirs))
    lo64, step = refine_axes(lo, hi, res)
    call("avr_occ_child_points", ptr(mask), ptr(offsets), (ctypes.c_int * 3)(*res), (ctypes.c_double * 3)(*lo64),
         (ctypes.c_double * 3)(*step), (ctypes.c_float * 3)(*[float(v) for v in direction]), n_live, ptr(xyz),
         ptr(viewdirs), stream_of(mask))
    return xyz, viewdirs


def flag_sigma(field_c, thr, first, flags):
    """avr_occ_flag_sigma: flags[q] = (0 if first else flags[q]) | not (field_c[q, 3] <= thr), in place (uint8)."""
    require_device(field_c, flags)
    call("avr_occ_flag_sigma", ptr(field_c), float(thr), int(bool(first)), field_c.shape[0], ptr(flags),
         stream_of(field_c))
    return flags


def build_sparse(mask, offsets, flags, n_live, res, dilate):
    """avr_occ_build_sparse -> bits (n_words(res),) int32; flags may be None with n_live == 0."""
    bits = torch.empty(n_words(res), dtype=torch.int32, device=mask.device)
    call("avr_occ_build_sparse", ptr(mask), ptr(offsets), ptr(flags), n_live, (ctypes.c_int * 3)(*res), int(dilate),
         ptr(bits), stream_of(bits))
    return bits


def classify(grid, ro, rd, z):
    """avr_occ_classify: ro, rd (R, 3), z (R, N) -> mask (R, ceil(N / 64)) int64 (the uint64 words' bits), counts
    (R,) int32."""
    R, N = z.shape
    require_device(ro, rd, z, grid.bits)
    mask = torch.empty(R, (N + 63) // 64, device=z.device, dtype=torch.int64)
    counts = torch.empty(R, device=z.device, dtype=torch.int32)
    call("avr_occ_classify", ctypes.byref(grid.desc), ptr(ro), ptr(rd), ptr(z), R, N, ptr(mask), ptr(counts),
         stream_of(z))
    return mask, counts


def compact(ro, rd, z, mask, offsets, n_live):
    """avr_occ_compact -> xyz, viewdirs (n_live, 3) of the live samples, ray-major sample order."""
    R, N = z.shape
    xyz = torch.empty(n_live, 3, device=z.device, dtype=F32)
    vd = torch.empty_like(xyz)
    call("avr_occ_compact", ptr(ro), ptr(rd), ptr(z), ptr(mask), ptr(offsets), R, N, n_live, ptr(xyz), ptr(vd),
         stream_of(z))
    return xyz, vd


def expand(field_c, mask, offsets, R, N, n_live):
    """avr_occ_expand: field_c (n_live, 4) or None -> (R * N, 4), zeros for dead samples, every element written."""
    field = torch.empty(R * N, 4, device=mask.device, dtype=F32)
    call("avr_occ_expand", ptr(field_c), ptr(mask), ptr(offsets), R, N, n_live, ptr(field), stream_of(field))
    return field


def scan(counts, total=None):
    """avr_occ_scan: counts (R,) int32 -> offsets (R,) int64 (exclusive prefix sums), total 0-dim int64 on the
    device (written into `total` when given)."""
    R = counts.shape[0]
    require_device(counts)
    offsets = torch.empty(R, device=counts.device, dtype=torch.int64)
    if total is None:
        total = torch.empty((), device=counts.device, dtype=torch.int64)
    call("avr_occ_scan", ptr(counts), R, ptr(offsets), ptr(total), stream_of(counts))
    return offsets, total


def _gated_field_device(fused, grid, ro, rd, z, coarse, sb, total):
    """gated_field with the live count on the device: every buffer is sized for the worst case (capacity R * N), no
    host read, no torch kernel (torch.empty only), legal on a capturing stream."""
    R, N = z.shape
    cap = R * N
    mask, counts = classify(grid, ro, rd, z)
    offsets, total = scan(counts, total)
    xyz = torch.empty(cap, 3, device=z.device, dtype=F32)
    vd = torch.empty_like(xyz)
    call("avr_occ_compact_counted", ptr(ro), ptr(rd), ptr(z), ptr(mask), ptr(offsets), R, N, ptr(total), cap,
         ptr(xyz), ptr(vd), stream_of(z))
    field_c = fused.forward_points_scene_counted(xyz, vd, total, coarse, sb)
    field = torch.empty(cap, 4, device=z.device, dtype=F32)
    call("avr_occ_expand_counted", ptr(field_c), ptr(mask), ptr(offsets), R, N, ptr(total), cap, ptr(field),
         stream_of(z))
    return field, total


def gated_field(fused, grid, ro, rd, z, coarse, sb=0, count="host", total=None):
    """The field of scene `sb` at ro[r] + rd[r] * z[r, s] where `grid` is live, exactly zero elsewhere:
    (field (R * N, 4), n_live). count="host": one host read (the live count, an int); no field launch when nothing
    is live. count="device": the count stays on the device (a 0-dim int64 tensor, `total` when given), nothing is
    read back and the call may be captured."""
    if count not in ("host", "device"):
        raise ValueError(f"gated_field: count must be 'host' or 'device', got {count!r}")
    R, N = z.shape
    if count == "host" and z.is_cuda and torch.cuda.is_current_stream_capturing():
        raise ValueError("occupancy gating reads the live count back to the host: it cannot be captured in a graph")
    ro = ro.reshape(R, 3).to(F32).contiguous()
    rd = rd.reshape(R, 3).to(F32).contiguous()
    z = z.to(F32).contiguous()
    if count == "device":
        return _gated_field_device(fused, grid, ro, rd, z, coarse, sb, total)
    mask, counts = classify(grid, ro, rd, z)
    incl = torch.cumsum(counts, 0, dtype=torch.int64)
    offsets = incl - counts
    n_live = int(incl[-1].item()) if R else 0
    field_c = None
    if n_live:
        xyz, vd = compact(ro, rd, z, mask, offsets, n_live)
        field_c = fused.forward_points_scene(xyz, vd, coarse, sb)
    return expand(field_c, mask, offsets, R, N, n_live), n_live
