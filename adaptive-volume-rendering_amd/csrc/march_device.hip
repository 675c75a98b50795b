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
//                               zeros, then the chunk composite march_composite_kernel runs (skip_common.h)
//
// A stopped ray needs no flag: its T is never updated again and T never rises, so the alive test on the state gives
// the same answer in every later chunk. No atomics, no workgroup waits on another, so every output is
// bit-reproducible. MarchState, the chunk composite, the grid, the live test, the rank, the sample point and the
// clamped device count are shared with march.hip and occupancy.hip through skip_common.h: this file holds the
// alive test, the mask and rank selection and the `evaluated` counter only. tests/test_gpu_march_device.py holds
// this chain to march.hip's and occupancy.hip's bit for bit, which pins that logic; the arithmetic is pinned by
// tests/composite_ref.py's float64 restatement and by the comparison with composite_fwd_kernel.
#include "skip_common.h"

namespace avr {

constexpr int kMarchDevWaves = 4;
constexpr int kMarchDevThreads = kWave * kMarchDevWaves;

// A ray is marched while its transmittance has not fallen below t_stop; before the first chunk every ray is.
__device__ __forceinline__ bool march_alive(const MarchState& s, int c0, float t_stop) {
  return c0 == 0 || (float)s.T >= t_stop;
}

__global__ void __launch_bounds__(kMarchDevThreads) march_classify_kernel(
    OccGrid g, const float* __restrict__ ro, const float* __restrict__ rd, const float* __restrict__ z,
    const MarchState* __restrict__ st, int64_t n_rays, int N, int c0, int C, float t_stop,
    uint64_t* __restrict__ mask, int32_t* __restrict__ counts) {
  const int64_t r = (int64_t)blockIdx.x * kMarchDevWaves + (threadIdx.x >> 6);
  if (r >= n_rays) return;   // whole waves leave together
  const int lane = threadIdx.x & (kWave - 1);
  bool live = false;
  if (march_alive(st[r], c0, t_stop) && lane < C) {
    live = true;
    if (g.bits) {
      const Point3 p = sample_point(ro, rd, r, z[r * N + c0 + lane]);
      live = occ_live(g, p.x, p.y, p.z);
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
  const int64_t live = counted_live(n_live, capacity);
  const int64_t r = (int64_t)blockIdx.x * kMarchDevWaves + (threadIdx.x >> 6);
  if (live == 0 || r >= n_rays) return;
  const int lane = threadIdx.x & (kWave - 1);
  const uint64_t m = mask[r];
  const int64_t q = offsets[r] + lane_rank(m, lane);
  // lane < C and 0 <= q < *n_live hold for the mask and offsets of avr_march_classify and avr_occ_scan; checked so
  // that inconsistent arguments cannot read outside z or write outside xyz / viewdirs
  if (((m >> lane) & 1ull) && lane < C && q >= 0 && q < live) {
    const Point3 p = sample_point(ro, rd, r, z[r * N + c0 + lane]);
    xyz[3 * q] = p.x; xyz[3 * q + 1] = p.y; xyz[3 * q + 2] = p.z;
    vd[3 * q] = rd[3 * r]; vd[3 * q + 1] = rd[3 * r + 1]; vd[3 * q + 2] = rd[3 * r + 2];
  }
}

// One wave per ray over all n_rays; lane k holds chunk sample c0 + k.
__global__ void __launch_bounds__(kMarchDevThreads) march_composite_masked_kernel(
    const float* __restrict__ z, const float4* __restrict__ field, const uint64_t* __restrict__ mask,
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ n_live, int64_t capacity, int64_t n_rays, int N,
    int c0, int C, float infinity, float t_stop, MarchState* __restrict__ st, int64_t* __restrict__ evaluated,
    int accumulate) {
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * kMarchDevWaves + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x == 0) {   // launches on a stream are ordered: a plain load and store
    const int64_t live = counted_live(n_live, capacity);
    *evaluated = accumulate ? *evaluated + live : live;
  }
  if (ray >= n_rays) return;   // wave-uniform
  MarchState s = st[ray];
  if (!march_alive(s, c0, t_stop)) return;   // a stopped ray, wave-uniform: before any store of its own
  const uint64_t m = mask[ray];
  const bool ok = lane < C;
  const int64_t q = offsets[ray] + lane_rank(m, lane);
  float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ok && ((m >> lane) & 1ull) && q >= 0 && q < capacity) f = field[q];
  chunk_composite(f, ok, z + ray * N, c0 + lane, N, infinity, lane, s);
  if (lane == 0) st[ray] = s;
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

extern "C" int avr_march_classify(const avr_occ_grid* grid, const float* ro, const float* rd, const float* z,
                                  const void* state, int64_t n_rays, int n_samples, int c0, int chunk, float t_stop,
                                  uint64_t* mask, int32_t* counts, void* stream) {
  int64_t blocks;
  OccGrid g;
  int rc = march_dev_sizes("avr_march_classify", n_rays, n_samples, c0, chunk, &blocks);
  if (rc || (rc = occ_grid_arg("avr_march_classify", grid, true, &g))) return rc;
  if (n_rays == 0) return AVR_OK;
  AVR_REQUIRE(ro && rd && z && state && mask && counts, "avr_march_classify: null pointer");
  AVR_REQUIRE((((uintptr_t)mask | (uintptr_t)state) & 7) == 0 && ((uintptr_t)counts & 3) == 0,
              "avr_march_classify: mask and state must be 8-B aligned, counts 4-B");
  march_classify_kernel<<<(unsigned)blocks, kMarchDevThreads, 0, as_stream(stream)>>>(
      g, ro, rd, z, reinterpret_cast<const MarchState*>(state), n_rays, n_samples, c0, chunk, t_stop, mask, counts);
  return check_launch("march_classify_kernel");
}

extern "C" int avr_march_compact_counted(const float* ro, const float* rd, const float* z, const uint64_t* mask,
                                         const int64_t* offsets, int64_t n_rays, int n_samples, int c0, int chunk,
                                         const int64_t* n_live, int64_t capacity, float* xyz, float* viewdirs,
                                         void* stream) {
  int64_t blocks;
  int rc = march_dev_sizes("avr_march_compact_counted", n_rays, n_samples, c0, chunk, &blocks);
  if (rc || (rc = counted_capacity("avr_march_compact_counted", capacity, n_rays, chunk, "chunk"))) return rc;
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
  if (rc || (rc = counted_capacity("avr_march_composite_masked", capacity, n_rays, chunk, "chunk"))) return rc;
  if (n_rays == 0) return AVR_OK;
  AVR_REQUIRE(z && field_c && mask && offsets && n_live && state && evaluated,
              "avr_march_composite_masked: null pointer");
  AVR_REQUIRE((((uintptr_t)n_live | (uintptr_t)evaluated | (uintptr_t)mask | (uintptr_t)offsets | (uintptr_t)state) &
               7) == 0,
              "avr_march_composite_masked: n_live, evaluated, mask, offsets and state must be 8-B aligned");
  AVR_REQUIRE(((uintptr_t)field_c & 15) == 0, "avr_march_composite_masked: field rows must be 16-B aligned");
  march_composite_masked_kernel<<<(unsigned)blocks, kMarchDevThreads, 0, as_stream(stream)>>>(
      z, reinterpret_cast<const float4*>(field_c), mask, offsets, n_live, capacity, n_rays, n_samples, c0, chunk,
      infinity, t_stop, reinterpret_cast<MarchState*>(state), evaluated, accumulate);
  return check_launch("march_composite_masked_kernel");
}
