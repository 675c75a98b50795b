// What the skip chain's three files share (occupancy.hip, march.hip, march_device.hip; DESIGN.md "Occupancy grid",
// "Early termination"), each piece once: the grid and its live test, the rank of a live sample, the device-side live
// count, the sample point, the per-ray compositing state, and the composite of one chunk of at most 64 samples.
#pragma once
#include "avr_common.h"

namespace avr {

struct OccGrid {   // bits == nullptr: no grid, every sample is live (avr_march_classify alone allows it)
  float lo[3], inv[3];
  int res[3];
  const uint32_t* bits;
};

// The live test of include/avr.h: the float comparisons 0 <= t < res are the integer test on floorf(t) for every
// finite t and stay defined for an infinite one (a finite point far outside the box: dead).
__device__ __forceinline__ bool occ_live(const OccGrid& g, float p0, float p1, float p2) {
  if (!(isfinite(p0) && isfinite(p1) && isfinite(p2))) return true;   // the field sees it, as in the ungated render
  const float t0 = fmul(fsub(p0, g.lo[0]), g.inv[0]);
  const float t1 = fmul(fsub(p1, g.lo[1]), g.inv[1]);
  const float t2 = fmul(fsub(p2, g.lo[2]), g.inv[2]);
  if (!(t0 >= 0.f && t0 < (float)g.res[0] && t1 >= 0.f && t1 < (float)g.res[1] && t2 >= 0.f && t2 < (float)g.res[2]))
    return false;
  const int ix = (int)floorf(t0), iy = (int)floorf(t1), iz = (int)floorf(t2);
  const int word = (iz * g.res[1] + iy) * (g.res[0] >> 5) + (ix >> 5);
  return (g.bits[word] >> (ix & 31)) & 1u;
}

// A live sample's rank among its ray's live samples of one mask word: the set bits below its own.
__device__ __forceinline__ int lane_rank(uint64_t m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

// The live count of the *_counted kernels: *n_live on the device, held to 0 .. capacity (what xyz, viewdirs and
// field_c were sized for), so q < *n_live and q < capacity are one test.
__device__ __forceinline__ int64_t counted_live(const int64_t* __restrict__ n_live, int64_t capacity) {
  const int64_t n = *n_live;
  return n < 0 ? 0 : (n < capacity ? n : capacity);
}

// Ray r's point at depth z, with the two roundings of field_common.h's sample_geom, so a compacted point is the
// point avr_field_fwd_rays would have formed, bit for bit.
struct Point3 {
  float x, y, z;
};
__device__ __forceinline__ Point3 sample_point(const float* __restrict__ ro, const float* __restrict__ rd, int64_t r,
                                               float z) {
  return {fadd(ro[3 * r], fmul(rd[3 * r], z)), fadd(ro[3 * r + 1], fmul(rd[3 * r + 1], z)),
          fadd(ro[3 * r + 2], fmul(rd[3 * r + 2], z))};
}

struct MarchState {  // per ray, fp64: transmittance and the sums of w * rgb, w * zz, w (include/avr.h: 48 bytes)
  double T, r, g, b, d, w;
};
static_assert(sizeof(MarchState) == 48, "avr_march_state_bytes: six doubles per ray");

// One sample's terms, with composite_fwd_kernel's rounding points (renderers.py:79-111).
struct SampleTerms {
  float d, e, alpha, t, zz;
};

__device__ __forceinline__ SampleTerms sample_terms(const float* __restrict__ zr, int n, int N, float sigma,
                                                    float infinity) {
  SampleTerms s;
  const float z0 = zr[n];
  const bool last = (n == N - 1);
  const float z1 = last ? 0.f : zr[n + 1];
  s.d = last ? 1e10f : fsub(z1, z0);
  s.zz = last ? infinity : z1;
  s.e = expf(-fmul(sigma, s.d));
  s.alpha = fsub(1.0f, s.e);
  s.t = fadd(fsub(1.0f, s.alpha), 1e-10f);
  return s;
}

// The composite of one chunk by one wave: this lane holds sample n of the ray whose depths are zr[0 .. N), with the
// field row f (ok: the lane holds a sample at all). fp64 product scan with the carried s.T, as composite_fwd_kernel
// carries it between its 64-sample rounds; s.T becomes the transmittance behind the chunk and the five sums grow by
// the chunk's share, in every lane alike.
__device__ __forceinline__ void chunk_composite(float4 f, bool ok, const float* __restrict__ zr, int n, int N,
                                                float infinity, int lane, MarchState& s) {
  const SampleTerms m = ok ? sample_terms(zr, n, N, f.w, infinity) : SampleTerms{0.f, 1.f, 0.f, 1.f, 0.f};
  const double incl = wave_incl_scan_mul((double)m.t, lane) * s.T;
  double excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = s.T;
  const float w = fmul(m.alpha, (float)excl);
  s.T = __shfl(incl, 63, 64);
  s.r += wave_sum_d(ok ? (double)w * f.x : 0.0);
  s.g += wave_sum_d(ok ? (double)w * f.y : 0.0);
  s.b += wave_sum_d(ok ? (double)w * f.z : 0.0);
  s.d += wave_sum_d(ok ? (double)w * m.zz : 0.0);
  s.w += wave_sum_d(ok ? (double)w : 0.0);
}

}  // namespace avr

// ---- host side: argument checks the entries share

static int occ_res(const char* who, const int* res) {
  AVR_REQUIRE(res, "%s: null res", who);
  for (int a = 0; a < 3; ++a)
    AVR_REQUIRE(res[a] >= 1 && res[a] <= AVR_OCC_MAX_RES, "%s: res[%d] = %d outside 1..%d", who, a, res[a],
                AVR_OCC_MAX_RES);
  AVR_REQUIRE(res[0] % 32 == 0, "%s: res[0] = %d is not a multiple of 32", who, res[0]);
  return AVR_OK;
}

// The grid of an entry, checked as include/avr.h states it, in the form the kernels take. null_ok: a null `grid`
// stands for no grid (bits stay nullptr).
static int occ_grid_arg(const char* who, const avr_occ_grid* grid, bool null_ok, avr::OccGrid* g) {
  *g = {};
  if (!grid && null_ok) return AVR_OK;
  AVR_REQUIRE(grid, "%s: null grid", who);
  const int rc = occ_res(who, grid->res);
  if (rc) return rc;
  AVR_REQUIRE(grid->bits, "%s: null grid bits", who);
  for (int a = 0; a < 3; ++a) { g->lo[a] = grid->lo[a]; g->inv[a] = grid->inv[a]; g->res[a] = grid->res[a]; }
  g->bits = grid->bits;
  return AVR_OK;
}

// A device-count entry's capacity: 0 .. n_rays * per_ray rows (`unit`: what per_ray is called in the message).
static int counted_capacity(const char* who, int64_t capacity, int64_t n_rays, int per_ray, const char* unit) {
  AVR_REQUIRE(capacity >= 0 && capacity <= n_rays * per_ray, "%s: capacity %lld outside 0..n_rays * %s", who,
              (long long)capacity, unit);
  return AVR_OK;
}
