// Per-ray sampling bounds from an occupancy grid (not in the reference; DESIGN.md "Occupancy grid: per-ray sampling
// bounds", include/avr.h "occupancy grid: per-ray bounds"): where along [near, far] the live cells of a ray begin and
// end, so that the renderer spreads its samples over that span alone.
//
//   avr_occ_ray_bounds  (grid, ro, rd, near, far) -> t_near, t_far   one ray per lane, no atomics, no LDS
//
// The walk runs in grid coordinates g(t) = o + d t (o = (ro - lo) inv, d = rd inv) in fp64, so its own rounding is
// far below the one thing it has to allow for: the live test rounds in fp32 (skip_common.h: sample_point, occ_live),
// so the cell it finds for a depth z can be a neighbour of the cell of g(z) when g(z) lies within delta[a] of a cell
// face (delta[a]: a bound on that fp32 error in cells, a few 1e-5 for a unit-sized scene). A slab clip against the
// grid's box grown by delta, then Amanatides-Woo segments between consecutive face crossings. Within the segment
// of cell c, the cells the live test can name at depth z are c + o, o in {-1, 0, 1}^3, where o[a] = -1 needs g[a](z)
// < c[a] + delta and o[a] = +1 needs g[a](z) >= c[a] + 1 - delta: g is monotone along the ray, so each condition
// holds on an interval at one end of the segment, and a neighbour is a candidate on the intersection of its three
// (usually empty but for the cell behind the entry face and the one ahead of the exit face, for about delta of
// depth). The earliest start of a set candidate's interval opens the ray's bounds; the same walk along the reversed
// ray closes them. Every depth the live test can call live lies in the interval of a set candidate, so safety holds
// by construction; a candidate is within delta of the ray, so the bounds are the exact hull widened by the depth
// the ray takes to cover delta, far inside the contract's slack.
#include "skip_common.h"

namespace avr {

constexpr int kBoundsThreads = 256;

struct BoundsRay {   // grid coordinates, fp64
  double o[3], d[3], delta[3];
};

__device__ __forceinline__ bool bounds_bit(const OccGrid& g, int ix, int iy, int iz) {
  return (g.bits[(iz * g.res[1] + iy) * (g.res[0] >> 5) + (ix >> 5)] >> (ix & 31)) & 1u;
}

// The earliest depth in the segment [ta, tb] of cell `cell` (ends at grid points ga, gb) at which a set cell is a
// candidate; false when none is.
__device__ __forceinline__ bool bounds_segment_first(const OccGrid& g, const BoundsRay& r, const double (&d)[3],
                                                     const double (&inv_d)[3], const int (&cell)[3], double ta,
                                                     double tb, const double (&ga)[3], const double (&gb)[3],
                                                     double& t_hit) {
  double s[3][3], e[3][3];   // [axis][offset + 1]: the depths where cell[a] + offset is the axis' candidate; s > e: none
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double below = (double)cell[a] + r.delta[a], above = (double)cell[a] + 1.0 - r.delta[a];
    const double t_below = (below - r.o[a]) * inv_d[a], t_above = (above - r.o[a]) * inv_d[a];
    const bool up = d[a] > 0.0, down = d[a] < 0.0;
    s[a][1] = ta;
    e[a][1] = tb;
    // g < below: from ta on going up, until tb going down, throughout for a zero component
    const bool near_lo = down ? gb[a] < below : ga[a] < below;
    s[a][0] = !near_lo ? INFINITY : (down ? fmax(ta, t_below) : ta);
    e[a][0] = !near_lo ? -INFINITY : (up ? fmin(tb, t_below) : tb);
    // g >= above: until tb going up, from ta on going down
    const bool near_hi = up ? gb[a] >= above : ga[a] >= above;
    s[a][2] = !near_hi ? INFINITY : (up ? fmax(ta, t_above) : ta);
    e[a][2] = !near_hi ? -INFINITY : (down ? fmin(tb, t_above) : tb);
  }
  double best = INFINITY;
#pragma unroll
  for (int ox = 0; ox < 3; ++ox) {
    const int ix = cell[0] + ox - 1;
    if (!(s[0][ox] <= e[0][ox]) || ix < 0 || ix >= g.res[0]) continue;
#pragma unroll
    for (int oy = 0; oy < 3; ++oy) {
      const int iy = cell[1] + oy - 1;
      const double sy = fmax(s[0][ox], s[1][oy]), ey = fmin(e[0][ox], e[1][oy]);
      if (!(sy <= ey) || iy < 0 || iy >= g.res[1]) continue;
#pragma unroll
      for (int oz = 0; oz < 3; ++oz) {
        const int iz = cell[2] + oz - 1;
        const double sz = fmax(sy, s[2][oz]), ez = fmin(ey, e[2][oz]);
        if (!(sz <= ez) || iz < 0 || iz >= g.res[2]) continue;   // (every read is inside the bits)
        if (bounds_bit(g, ix, iy, iz)) best = fmin(best, sz);
      }
    }
  }
  t_hit = best;
  return best < INFINITY;
}

// The earliest depth of o + d t, t in [t0, t1], at which a set cell is a candidate; false when there is none.
// `cap`: more segments than any ray has (one per face crossing); a walk that reaches it reports t0.
__device__ __forceinline__ bool bounds_first(const OccGrid& g, const BoundsRay& r, const double (&d)[3], double t0,
                                             double t1, int cap, double& t_first) {
  int cell[3], step[3];
  double inv_d[3], t_max[3], ga[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    ga[a] = r.o[a] + d[a] * t0;
    cell[a] = (int)floor(ga[a]);
    step[a] = d[a] > 0.0 ? 1 : -1;
    inv_d[a] = d[a] != 0.0 ? 1.0 / d[a] : 0.0;
    // the next face of axis a ahead of the ray: cell + 1 going up, cell going down; never for a zero component
    t_max[a] = d[a] != 0.0 ? ((double)(cell[a] + (d[a] > 0.0 ? 1 : 0)) - r.o[a]) * inv_d[a] : INFINITY;
  }
  double t = t0;
  for (int it = 0; it < cap; ++it) {
    const int a = t_max[0] <= t_max[1] ? (t_max[0] <= t_max[2] ? 0 : 2) : (t_max[1] <= t_max[2] ? 1 : 2);
    const double t_face = fmin(t_max[0], fmin(t_max[1], t_max[2]));
    const double t_next = fmin(fmax(t_face, t), t1);
    double gb[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) gb[b] = r.o[b] + d[b] * t_next;
    if (bounds_segment_first(g, r, d, inv_d, cell, t, t_next, ga, gb, t_first)) return true;
    if (t_next >= t1) return false;
    // cross the face: the cell counter moves by one, the next face comes from the counter (no accumulated sum)
#pragma unroll
    for (int b = 0; b < 3; ++b)
      if (b == a) {
        cell[b] += step[b];
        t_max[b] = ((double)(cell[b] + (d[b] > 0.0 ? 1 : 0)) - r.o[b]) * inv_d[b];
      }
    t = t_next;
#pragma unroll
    for (int b = 0; b < 3; ++b) ga[b] = gb[b];
  }
  t_first = t0;
  return true;
}

__global__ void __launch_bounds__(kBoundsThreads) occ_ray_bounds_kernel(OccGrid g, const float* __restrict__ ro,
                                                                         const float* __restrict__ rd, int64_t n_rays,
                                                                         float near_, float far_,
                                                                         float* __restrict__ t_near,
                                                                         float* __restrict__ t_far) {
  const int64_t i = (int64_t)blockIdx.x * kBoundsThreads + threadIdx.x;
  if (i >= n_rays) return;
  float tn = near_, tf = far_;   // a miss, a non-finite ray, an empty interval: the whole range
  const float o0 = ro[3 * i], o1 = ro[3 * i + 1], o2 = ro[3 * i + 2];
  const float d0 = rd[3 * i], d1 = rd[3 * i + 1], d2 = rd[3 * i + 2];
  if (isfinite(o0) && isfinite(o1) && isfinite(o2) && isfinite(d0) && isfinite(d1) && isfinite(d2)) {
    const float of[3] = {o0, o1, o2}, df[3] = {d0, d1, d2};
    const double z_max = fmax(fabs((double)near_), fabs((double)far_));
    BoundsRay r;
    double t0 = near_, t1 = far_;
    bool hit = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double inv = g.inv[a], res = g.res[a];
      r.o[a] = ((double)of[a] - (double)g.lo[a]) * inv;
      r.d[a] = (double)df[a] * inv;
      // the live test's fp32 error in cells: one rounding each of rd z, ro + rd z, p - lo and (p - lo) inv, each at
      // most 2^-24 of its result, summed with a factor 4 to spare, and 1e-6 cells for the walk's own fp64 rounding
      r.delta[a] = 0x1p-22 * (fabs(inv) * (fabs((double)of[a]) + 2.0 * fabs((double)df[a]) * z_max
                                           + fabs((double)g.lo[a])) + 2.0 * res) + 1e-6;
      // slab clip against the box grown by delta
      const double lo = -r.delta[a], hi = res + r.delta[a];
      if (r.d[a] != 0.0) {
        const double ta = (lo - r.o[a]) / r.d[a], tb = (hi - r.o[a]) / r.d[a];
        t0 = fmax(t0, fmin(ta, tb));
        t1 = fmin(t1, fmax(ta, tb));
      } else if (!(r.o[a] >= lo && r.o[a] <= hi)) {
        hit = false;
      }
    }
    // a delta of a cell or more (coordinates some 1e5 boxes away) leaves nothing to bound: the whole range, and the
    // cell counters below stay within res + 2
    hit = hit && r.delta[0] < 1.0 && r.delta[1] < 1.0 && r.delta[2] < 1.0;
    if (hit && t0 <= t1) {
      const int cap = g.res[0] + g.res[1] + g.res[2] + 8;
      const double back[3] = {-r.d[0], -r.d[1], -r.d[2]};
      double first, last;
      if (bounds_first(g, r, r.d, t0, t1, cap, first)) {
        // the reversed ray o + (-d) s over s in [-t1, -t0]; it can miss what the forward walk found only where no
        // point of the ray is near the set cell (the candidates are a box around a segment): the clip's end then
        last = bounds_first(g, r, back, -t1, -t0, cap, last) ? -last : t1;
        float a = (float)first, b = (float)last;   // rounded outwards
        if ((double)a > first) a = nextafterf(a, -INFINITY);
        if ((double)b < last) b = nextafterf(b, INFINITY);
        a = fmaxf(a, near_);
        b = fminf(b, far_);
        if (a < b) {
          tn = a;
          tf = b;
        }
      }
    }
  }
  t_near[i] = tn;
  t_far[i] = tf;
}

}  // namespace avr

using namespace avr;

extern "C" int avr_occ_ray_bounds(const avr_occ_grid* grid, const float* ro, const float* rd, int64_t n_rays,
                                  float near_, float far_, float* t_near, float* t_far, void* stream) {
  OccGrid g;
  const int rc = occ_grid_arg("avr_occ_ray_bounds", grid, false, &g);
  if (rc) return rc;
  AVR_REQUIRE(n_rays >= 0, "avr_occ_ray_bounds: negative n_rays");
  AVR_REQUIRE(near_ < far_, "avr_occ_ray_bounds: near %g must be below far %g", (double)near_, (double)far_);
  if (n_rays == 0) return AVR_OK;
  AVR_REQUIRE(ro && rd && t_near && t_far, "avr_occ_ray_bounds: null pointer");
  const int64_t blocks = (n_rays + kBoundsThreads - 1) / kBoundsThreads;
  AVR_REQUIRE(blocks < (1ll << 31), "avr_occ_ray_bounds: too many rays");
  occ_ray_bounds_kernel<<<(unsigned)blocks, kBoundsThreads, 0, as_stream(stream)>>>(g, ro, rd, n_rays, near_, far_,
                                                                                  t_near, t_far);
  return check_launch("occ_ray_bounds_kernel");
}
