"""Reference of the occupancy-grid kernels (csrc/occupancy.hip, include/avr.h "occupancy grid") in numpy. Nothing
here imports avr: the contract is restated.

Grid: box lo / hi, res = (rx, ry, rz), rx % 32 == 0; cell (ix, iy, iz) is bit ix % 32 of uint32 word
(iz * ry + iy) * (rx / 32) + ix / 32; inv[a] = float32(res[a] / (float64(hi[a]) - float64(lo[a]))).
A sample: p = ro + rd * z with both operations rounded to float32 (no fused multiply-add), t = (p - lo) * inv
likewise, live iff every 0 <= t[a] < res[a] -- the test on i = floor(t) for finite t, and defined for an infinite
one -- and the cell's bit is set; a point with a non-finite coordinate is live, a point outside the box dead."""
import numpy as np

F = np.float32


def check_res(res):
    res = tuple(int(r) for r in res)
    assert len(res) == 3 and all(1 <= r <= 256 for r in res) and res[0] % 32 == 0, res
    return res


def inv_of(lo, hi, res):
    lo, hi = np.asarray(lo, F).astype(np.float64), np.asarray(hi, F).astype(np.float64)
    return (np.asarray(res, np.float64) / (hi - lo)).astype(F)


def pack_bits(occ):
    """occ (rz, ry, rx) bool -> uint32 words (rz * ry * rx / 32,), bit ix % 32 of word ... + ix / 32."""
    rz, ry, rx = occ.shape
    assert rx % 32 == 0
    b = occ.reshape(rz * ry * (rx // 32), 32).astype(np.uint64)
    return (b << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def unpack_bits(bits, res):
    rx, ry, rz = res
    w = np.asarray(bits).view(np.uint32).reshape(-1, 1)
    return ((w >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(rz, ry, rx)


def build(sigma, thr, dilate):
    """sigma (K, rz, ry, rx) float32 -> occ (rz, ry, rx) bool: any plane, any cell within Chebyshev distance dilate
    (clamped at the faces) with not (sigma <= thr); NaN is occupied."""
    assert dilate in (0, 1, 2)
    sigma = np.asarray(sigma, F)
    with np.errstate(invalid="ignore"):
        raw = (~(sigma <= F(thr))).any(0)
    rz, ry, rx = raw.shape
    occ = np.zeros_like(raw)
    d = dilate
    pad = np.pad(raw, d, mode="constant", constant_values=False)   # a clamped neighbour is a cell already counted
    for dz in range(2 * d + 1):
        for dy in range(2 * d + 1):
            for dx in range(2 * d + 1):
                occ |= pad[dz:dz + rz, dy:dy + ry, dx:dx + rx]
    return occ


def points(ro, rd, z):
    """(R, N, 3) float32: fadd(ro, fmul(rd, z)), each rounded once."""
    ro, rd, z = np.asarray(ro, F), np.asarray(rd, F), np.asarray(z, F)
    with np.errstate(all="ignore"):
        prod = (rd[:, None, :] * z[:, :, None]).astype(F)
        return (ro[:, None, :] + prod).astype(F)


def classify_points(occ, lo, hi, p):
    """p (..., 3) float32 -> live (...) bool."""
    rz, ry, rx = occ.shape
    res = np.array([rx, ry, rz])
    lo32, inv = np.asarray(lo, F), inv_of(lo, hi, res)
    with np.errstate(all="ignore"):
        t = ((p - lo32).astype(F) * inv).astype(F)
        inside = ((t >= 0) & (t < res.astype(F))).all(-1)
        i = np.where(inside[..., None], np.floor(t), 0).astype(np.int64)
    live = inside & occ[i[..., 2], i[..., 1], i[..., 0]]
    return live | ~np.isfinite(p).all(-1)


def classify(occ, lo, hi, ro, rd, z):
    """-> live (R, N) bool, mask (R, ceil(N / 64)) uint64 (bit s % 64 of word s / 64), counts (R,) int32."""
    live = classify_points(occ, lo, hi, points(ro, rd, z))
    R, N = live.shape
    W = (N + 63) // 64
    padded = np.zeros((R, W * 64), np.uint64)
    padded[:, :N] = live
    mask = (padded.reshape(R, W, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    return live, mask, live.sum(1).astype(np.int32)


def compact(live, ro, rd, z):
    """xyz, viewdirs (M, 3): the live samples in ray-major sample order."""
    p = points(ro, rd, z)
    vd = np.broadcast_to(np.asarray(rd, F)[:, None, :], p.shape)
    return p[live], vd[live]


def expand(live, field_c):
    """(R * N, 4): row k of field_c at the k-th live sample, exact zeros elsewhere."""
    out = np.zeros((live.size, 4), F)
    out[live.reshape(-1)] = field_c
    return out


def sphere_occ(res, lo, hi, centre, radius):
    """Cells whose centre lies within `radius` of `centre`: the synthetic grid of the tests and the A/B script."""
    rx, ry, rz = res
    ax = [np.float64(l) + (np.arange(r) + 0.5) * (np.float64(h) - np.float64(l)) / r for l, h, r in zip(lo, hi, res)]
    zz, yy, xx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    c = np.asarray(centre, np.float64)
    return (xx - c[0]) ** 2 + (yy - c[1]) ** 2 + (zz - c[2]) ** 2 <= radius ** 2
