"""Reference of the hierarchical occupancy-grid build (csrc/occupancy_refine.hip, include/avr.h "occupancy grid:
hierarchical build") in numpy. Nothing here imports avr: the contract is restated.

Fine grid: box lo / hi, res = (rx, ry, rz); factor f in {2, 4, 8}, every res[a] % f == 0; the coarse grid C has res
rc = res / f with rc[0] % 32 == 0 over the same box. Fine cell (ix, iy, iz) is a candidate iff C's cell (ix / f,
iy / f, iz / f) is set. Candidates are ordered by the linear fine index (iz * ry + iy) * rx + ix; the mask is
(ry * rz, ceil(rx / 64)) uint64, row iz * ry + iy, bit ix % 64 of word ix / 64; counts int32 per row; offsets the
exclusive prefix sums; M = f^3 * popcount(C); a candidate's rank is offsets[row] + popcount of the lower mask bits of
its row. Points: the rows of the cell centres float32(lo64 + (i + 0.5) * step), lo64 = float64(float32(lo)), step =
(hi64 - lo64) / res, at the candidates. Flags: OR over the planes of not (sigma <= thr), NaN occupied. Bits: a fine
cell is set iff a candidate with a set flag lies within Chebyshev distance dilate (clamped at the faces) -- what the
dense build gives for planes that hold sigma at the candidates and 0 elsewhere (thr >= 0)."""
import numpy as np

F = np.float32


def check_shapes(res, f):
    res = tuple(int(r) for r in res)
    assert f in (2, 4, 8) and len(res) == 3 and all(1 <= r <= 256 and r % f == 0 for r in res), (res, f)
    rc = tuple(r // f for r in res)
    assert rc[0] % 32 == 0, rc
    return res, rc


def children(cocc, f):
    """cocc (rcz, rcy, rcx) bool -> cand (rz, ry, rx) bool: every fine cell under a live coarse cell."""
    return np.repeat(np.repeat(np.repeat(np.asarray(cocc, bool), f, 0), f, 1), f, 2)


def mask_counts_offsets(cand):
    """cand (rz, ry, rx) bool -> mask (ry * rz, ceil(rx / 64)) uint64, counts (rows,) int32, offsets (rows,) int64,
    total."""
    rz, ry, rx = cand.shape
    rows, W = rz * ry, (rx + 63) // 64
    padded = np.zeros((rows, W * 64), np.uint64)
    padded[:, :rx] = cand.reshape(rows, rx)
    mask = (padded.reshape(rows, W, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    counts = cand.reshape(rows, rx).sum(1).astype(np.int32)
    incl = np.cumsum(counts, dtype=np.int64)
    return mask, counts, incl - counts, int(incl[-1])


def ranks(cand):
    """(rz, ry, rx) int64: a candidate's rank = offsets[row] + the set mask bits of its row below it; -1 elsewhere.
    Worked out from the mask words, not from a flat cumsum, so that it restates the rule."""
    rz, ry, rx = cand.shape
    mask, _, offsets, _ = mask_counts_offsets(cand)
    out = np.full((rz * ry, rx), -1, np.int64)
    for row in range(rz * ry):
        for ix in np.nonzero(cand.reshape(rz * ry, rx)[row])[0].tolist():
            below = sum(bin(int(mask[row, w])).count("1") for w in range(ix // 64))
            below += bin(int(mask[row, ix // 64]) & ((1 << (ix % 64)) - 1)).count("1")
            out[row, ix] = offsets[row] + below
    return out.reshape(rz, ry, rx)


def axes(lo, hi, res):
    """lo64 (3,) and step (3,) in float64: lo64 = float64(float32(lo)), step = (hi64 - lo64) / res."""
    lo64 = np.asarray(lo, F).astype(np.float64)
    hi64 = np.asarray(hi, F).astype(np.float64)
    return lo64, (hi64 - lo64) / np.asarray(res, np.float64)


def centres(lo, hi, res):
    """(rz, ry, rx, 3) float32 cell centres: the product and the sum each rounded once in float64."""
    lo64, step = axes(lo, hi, res)
    ax = [(lo64[a] + (np.arange(res[a], dtype=np.float64) + 0.5) * step[a]).astype(F) for a in range(3)]
    zz, yy, xx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([xx, yy, zz], -1)


def child_points(cand, lo, hi, direction):
    """xyz, viewdirs (M, 3) float32 in candidate order (boolean indexing of a C-ordered array is that order)."""
    rz, ry, rx = cand.shape
    xyz = centres(lo, hi, (rx, ry, rz))[cand]
    return xyz, np.broadcast_to(np.asarray(direction, F), xyz.shape).copy()


def flag_sigma(sigma_planes, thr):
    """sigma_planes (K, M) float32 -> flags (M,) uint8: plane 0 overwrites, the later planes OR in."""
    flags = None
    with np.errstate(invalid="ignore"):
        for k, s in enumerate(np.asarray(sigma_planes, F)):
            occ = (~(s <= F(thr))).astype(np.uint8)
            flags = occ if k == 0 else flags | occ
    return flags


def build_sparse(cand, flags, dilate):
    """occ (rz, ry, rx) bool: set iff a candidate with a set flag lies within Chebyshev distance dilate."""
    assert dilate in (0, 1, 2)
    rz, ry, rx = cand.shape
    raw = np.zeros(cand.shape, bool)
    if cand.any():
        raw[cand] = np.asarray(flags).astype(bool)
    d = dilate
    pad = np.pad(raw, d, mode="constant", constant_values=False)
    occ = np.zeros_like(raw)
    for dz in range(2 * d + 1):
        for dy in range(2 * d + 1):
            for dx in range(2 * d + 1):
                occ |= pad[dz:dz + rz, dy:dy + ry, dx:dx + rx]
    return occ


def dense_planes(cand, sigma_planes):
    """(K, rz, ry, rx) float32: sigma at the candidates, 0 elsewhere -- the planes whose dense build equals
    build_sparse."""
    sigma_planes = np.asarray(sigma_planes, F)
    out = np.zeros((sigma_planes.shape[0],) + cand.shape, F)
    out[:, cand] = sigma_planes
    return out


def downsample(occ, p):
    """occ (rz, ry, rx) bool -> (rz / p, ry / p, rx / p): the OR of the p^3 children."""
    assert p in (1, 2, 4)
    rz, ry, rx = occ.shape
    assert rz % p == 0 and ry % p == 0 and rx % p == 0 and (rx // p) % 32 == 0
    return occ.reshape(rz // p, p, ry // p, p, rx // p, p).any((1, 3, 5))
