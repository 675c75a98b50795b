// Early ray termination of the fine pass with every count kept on the device (not in the reference; DESIGN.md
// "Early termination: device-side chain"; include/avr.h "fine pass, early termination on the device"). march.hip's
// chain reads the active-ray count back after every chunk and appends survivors with an atomic; this one sizes
// nothing on the host, appends nothing and can be recorded in a HIP-graph capture. Per chunk [c0, c0 + C), C <= 64:
//
//   avr_march_classify          wave per ray, lane per chunk sample: ray alive (c0 == 0 or (float)T >= t_stop) and
//                               sample live against the grid (NULL grid: every sample) -> mask, counts
//   avr_occ_scan                counts -> offsets, *total                                         (occupancy.hip)
//   avr_march_compact_counted   the live samples' points and directions, ray-major -> rows [0, *total)
//   <field>                     avr_field_fwd_points_counted on those rows
//   avr_march_composite_masked  wave per ray: lane k takes row offsets[ray] + popcount(lower mask bits) or exact
//                               zeros, then march_composite_kernel's terms, fp64 scan with the carried T and sums
//
// A stopped ray needs no flag: its T is never updated again and T never rises, so the alive test on the state gives
// the same answer in every later chunk. No atomics, no workgroup waits on another, so every output is
// bit-reproducible. MarchState, the composite arithmetic, the live test and the rank are restated from march.hip
// and occupancy.hip (those files and their kernels' code stay as they are); tests/test_gpu_march_device.py holds
// the restatements to the originals bit for bit.
#include "avr_common.h"

namespace avr {

constexpr int kMarchDevWaves = 4;
constexpr int kMarchDevThreads = kWave * kMarchDevWaves;

struct MarchStateD {  // march.hip's MarchState
  double T, r, g, b, d, w;
};
static_assert(sizeof(MarchStateD) == 48, "MarchState of march.hip");

struct MarchGrid {   // occupancy.hip's OccGrid; bits == nullptr: no grid, every cell occupied
  float lo[3], inv[3];
  int res[3];
  const uint32_t* bits;
};

// occupancy.hip's occ_live
__device__ __forceinline__ bool march_occ_live(const MarchGrid& g, float p0, float p1, float p2) {
  if (!(isfinite(p0) && isfinite(p1) && isfinite(p2))) return true;
  const float t0 = fmul(fsub(p0, g.lo[0]), g.inv[0]);
  const float t1 = fmul(fsub(p1, g.lo[1]), g.inv[1]);
  const float t2 = fmul(fsub(p2, g.lo[2]), g.inv[2]);
  if (!(t0 >= 0.f && t0 < (float)g.res[0] && t1 >= 0.f && t1 < (float)g.res[1] && t2 >= 0.f && t2 < (float)g.res[2]))
    return false;
  const int ix = (int)floorf(t0), iy = (int)floorf(t1), iz = (int)floorf(t2);
  const int word = (iz * g.res[1] + iy) * (g.res[0] >> 5) + (ix >> 5);
  return (g.bits[word] >> (ix & 31)) & 1u;
}

__device__ __forceinline__ int march_lane_rank(uint64_t m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

__device__ __forceinline__ bool march_alive(const MarchStateD* __restrict__ st, int64_t ray, int c0, float t_stop) {
  return c0 == 0 || (float)st[ray].T >= t_stop;
}

__global__ void __launch_bounds__(kMarchDevThreads) march_classify_kernel(
    MarchGrid g, const float* __restrict__ ro, const float* __restrict__ rd, const float* __restrict__ z,
    const MarchStateD* __restrict__ st, int64_t n_rays, int N, int c0, int C, float t_stop,
    uint64_t* __restrict__ mask, int32_t* __restrict__ counts) {
  const int64_t r = (int64_t)blockIdx.x * kMarchDevWaves + (threadIdx.x >> 6);
  if (r >= n_rays) return;   // whole waves leave together
  const int lane = threadIdx.x & (kWave - 1);
  bool live = false;
  if (march_alive(st, r, c0, t_stop) && lane < C) {
    live = true;
    if (g.bits) {
      const float zz = z[r * N + c0 + lane];
      live = march_occ_live(g, fadd(ro[3 * r], fmul(rd[3 * r], zz)), fadd(ro[3 * r + 1], fmul(rd[3 * r + 1], zz)),
                            fadd(ro[3 * r + 2], fmul(rd[3 * r + 2], zz)));
    }
  }
  const uint64_t m = __ballot(live);
  if (lane == 0) {
    mask[r] = m;
    counts[r] = __popcll(m);
  }
}

__global__ void __launch_bounds__(kMarchDevThreads) march_compact_counted_kernel(
    const float* __restrict__ ro, const float* __restrict__ rd, const float* __restrict__ z,
    const uint64_t* __restrict__ mask, const int64_t* __restrict__ offsets, int64_t n_rays, int N, int c0, int C,
    const int64_t* __restrict__ n_live, int64_t capacity, float* __restrict__ xyz, float* __restrict__ vd) {
  const int64_t n = *n_live;
  const int64_t live = n < 0 ? 0 : (n < capacity ? n : capacity);
  const int64_t r = (int64_t)blockIdx.x * kMarchDevWaves + (threadIdx.x >> 6);
  if (live == 0 || r >= n_rays) return;
  const int lane = threadIdx.x & (kWave - 1);
  const uint64_t m = mask[r];
  const int64_t q = offsets[r] + march_lane_rank(m, lane);
  // lane < C and 0 <= q < *n_live hold for the mask and offsets of avr_march_classify and avr_occ_scan; checked so
  // that inconsistent arguments cannot read outside z or write outside xyz / viewdirs
  if (((m >> lane) & 1ull) && lane < C && q >= 0 && q < live) {
    const float zz = z[r * N + c0 + lane];
    const float d0 = rd[3 * r], d1 = rd[3 * r + 1], d2 = rd[3 * r + 2];
    xyz[3 * q] = fadd(ro[3 * r], fmul(d0, zz));
    xyz[3 * q + 1] = fadd(ro[3 * r + 1], fmul(d1, zz));
    xyz[3 * q + 2] = fadd(ro[3 * r + 2], fmul(d2, zz));
    vd[3 * q] = d0; vd[3 * q + 1] = d1; vd[3 * q + 2] = d2;
  }
}

// One wave per ray over all n_rays; lane k holds chunk sample c0 + k. From `alpha` on: march_composite_kernel.
__global__ void __launch_bounds__(kMarchDevThreads) march_composite_masked_kernel(
    const float* __restrict__ z, const float4* __restrict__ field, const uint64_t* __restrict__ mask,
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ n_live, int64_t capacity, int64_t n_rays, int N,
    int c0, int C, float infinity, float t_stop, MarchStateD* __restrict__ st, int64_t* __restrict__ evaluated,
    int accumulate) {
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * kMarchDevWaves + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x == 0) {   // launches on a stream are ordered: a plain load and store
    const int64_t n = *n_live;
    const int64_t live = n < 0 ? 0 : (n < capacity ? n : capacity);
    *evaluated = accumulate ? *evaluated + live : live;
  }
  if (ray >= n_rays) return;   // wave-uniform
  MarchStateD s = st[ray];
  if (!(c0 == 0 || (float)s.T >= t_stop)) return;   // a stopped ray, wave-uniform: before any store of its own
  const uint64_t m = mask[ray];
  const float* zr = z + ray * N;
  const int n = c0 + lane;
  const bool ok = lane < C;
  const int64_t q = offsets[ray] + march_lane_rank(m, lane);
  float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ok && ((m >> lane) & 1ull) && q >= 0 && q < capacity) f = field[q];
  float alpha = 0.f, t = 1.f, zz = 0.f;
  if (ok) {  // same terms and rounding points as composite_fwd_kernel (renderers.py:79-111)
    const bool last = n == N - 1;
    const float z0 = zr[n];
    const float z1 = last ? 0.f : zr[n + 1];
    const float d = last ? 1e10f : fsub(z1, z0);
    zz = last ? infinity : z1;
    alpha = fsub(1.0f, expf(-fmul(f.w, d)));
    t = fadd(fsub(1.0f, alpha), 1e-10f);
  }
  const double incl = wave_incl_scan_mul((double)t, lane) * s.T;
  double excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = s.T;
  const double Tn = __shfl(incl, 63, 64);
  const float w = fmul(alpha, (float)excl);
  const double r = wave_sum_d(ok ? (double)w * f.x : 0.0);
  const double g = wave_sum_d(ok ? (double)w * f.y : 0.0);
  const double b = wave_sum_d(ok ? (double)w * f.z : 0.0);
  const double dd = wave_sum_d(ok ? (double)w * zz : 0.0);
  const double ws = wave_sum_d(ok ? (double)w : 0.0);
  if (lane == 0) {
    s.T = Tn;
    s.r += r; s.g += g; s.b += b; s.d += dd; s.w += ws;
    st[ray] = s;
  }
}

}  // namespace avr

using namespace avr;

// The checks the three entries share; *blocks = the grid of a wave-per-ray launch.
static int march_dev_sizes(const char* who, int64_t n_rays, int n_samples, int c0, int chunk, int64_t* blocks) {
  AVR_REQUIRE(n_rays >= 0, "%s: negative n_rays", who);
  AVR_REQUIRE(chunk >= 1 && chunk <= 64, "%s: chunk %d outside 1..64", who, chunk);
  AVR_REQUIRE(n_samples >= 1 && c0 >= 0 && c0 <= n_samples - chunk,
              "%s: samples [c0 %d, c0 + chunk %d) outside 0..n_samples %d", who, c0, chunk, n_samples);
  *blocks = (n_rays + kMarchDevWaves - 1) / kMarchDevWaves;
  AVR_REQUIRE(*blocks < (1ll << 31), "%s: too many rays", who);
  return AVR_OK;
}

static int march_dev_capacity(const char* who, int64_t capacity, int64_t n_rays, int chunk) {
  AVR_REQUIRE(capacity >= 0 && capacity <= n_rays * chunk, "%s: capacity %lld outside 0..n_rays * chunk", who,
              (long long)capacity);
  return AVR_OK;
}

extern "C" int avr_march_classify(const avr_occ_grid* grid, const float* ro, const float* rd, const float* z,
                                  const void* state, int64_t n_rays, int n_samples, int c0, int chunk, float t_stop,
                                  uint64_t* mask, int32_t* counts, void* stream) {
  int64_t blocks;
  int rc = march_dev_sizes("avr_march_classify", n_rays, n_samples, c0, chunk, &blocks);
  if (rc) return rc;
  MarchGrid g = {};
  if (grid) {
    for (int a = 0; a < 3; ++a) {
      AVR_REQUIRE(grid->res[a] >= 1 && grid->res[a] <= AVR_OCC_MAX_RES,
                  "avr_march_classify: res[%d] = %d outside 1..%d", a, grid->res[a], AVR_OCC_MAX_RES);
      g.lo[a] = grid->lo[a]; g.inv[a] = grid->inv[a]; g.res[a] = grid->res[a];
    }
    AVR_REQUIRE(grid->res[0] % 32 == 0, "avr_march_classify: res[0] = %d is not a multiple of 32", grid->res[0]);
    AVR_REQUIRE(grid->bits, "avr_march_classify: null grid bits");
    g.bits = grid->bits;
  }
  if (n_rays == 0) return AVR_OK;
  AVR_REQUIRE(ro && rd && z && state && mask && counts, "avr_march_classify: null pointer");
  AVR_REQUIRE((((uintptr_t)mask | (uintptr_t)state) & 7) == 0 && ((uintptr_t)counts & 3) == 0,
              "avr_march_classify: mask and state must be 8-B aligned, counts 4-B");
  march_classify_kernel<<<(unsigned)blocks, kMarchDevThreads, 0, as_stream(stream)>>>(
      g, ro, rd, z, reinterpret_cast<const MarchStateD*>(state), n_rays, n_samples, c0, chunk, t_stop, mask, counts);
  return check_launch("march_classify_kernel");
}

extern "C" int avr_march_compact_counted(const float* ro, const float* rd, const float* z, const uint64_t* mask,
                                         const int64_t* offsets, int64_t n_rays, int n_samples, int c0, int chunk,
                                         const int64_t* n_live, int64_t capacity, float* xyz, float* viewdirs,
                                         void* stream) {
  int64_t blocks;
  int rc = march_dev_sizes("avr_march_compact_counted", n_rays, n_samples, c0, chunk, &blocks);
  if (rc || (rc = march_dev_capacity("avr_march_compact_counted", capacity, n_rays, chunk))) return rc;
  if (n_rays == 0 || capacity == 0) return AVR_OK;
  AVR_REQUIRE(ro && rd && z && mask && offsets && n_live && xyz && viewdirs, "avr_march_compact_counted: null pointer");
  AVR_REQUIRE((((uintptr_t)n_live | (uintptr_t)mask | (uintptr_t)offsets) & 7) == 0,
              "avr_march_compact_counted: n_live, mask and offsets must be 8-B aligned");
  march_compact_counted_kernel<<<(unsigned)blocks, kMarchDevThreads, 0, as_stream(stream)>>>(
      ro, rd, z, mask, offsets, n_rays, n_samples, c0, chunk, n_live, capacity, xyz, viewdirs);
  return check_launch("march_compact_counted_kernel");
}

extern "C" int avr_march_composite_masked(const float* z, const float* field_c, const uint64_t* mask,
                                          const int64_t* offsets, const int64_t* n_live, int64_t capacity,
                                          int64_t n_rays, int n_samples, int c0, int chunk, float infinity,
                                          float t_stop, void* state, int64_t* evaluated, int accumulate,
                                          void* stream) {
  int64_t blocks;
  int rc = march_dev_sizes("avr_march_composite_masked", n_rays, n_samples, c0, chunk, &blocks);
  if (rc || (rc = march_dev_capacity("avr_march_composite_masked", capacity, n_rays, chunk))) return rc;
  if (n_rays == 0) return AVR_OK;
  AVR_REQUIRE(z && field_c && mask && offsets && n_live && state && evaluated,
              "avr_march_composite_masked: null pointer");
  AVR_REQUIRE((((uintptr_t)n_live | (uintptr_t)evaluated | (uintptr_t)mask | (uintptr_t)offsets | (uintptr_t)state) &
               7) == 0,
              "avr_march_composite_masked: n_live, evaluated, mask, offsets and state must be 8-B aligned");
  AVR_REQUIRE(((uintptr_t)field_c & 15) == 0, "avr_march_composite_masked: field rows must be 16-B aligned");
  march_composite_masked_kernel<<<(unsigned)blocks, kMarchDevThreads, 0, as_stream(stream)>>>(
      z, reinterpret_cast<const float4*>(field_c), mask, offsets, n_live, capacity, n_rays, n_samples, c0, chunk,
      infinity, t_stop, reinterpret_cast<MarchStateD*>(state), evaluated, accumulate);
  return check_launch("march_composite_masked_kernel");
}
