// Occupancy-grid empty-space skipping for VolumeRenderer inference (not in the reference; DESIGN.md "Occupancy
// grid"): a per-scene bit grid over an axis-aligned box, a per-sample live test against it, and the compaction /
// expansion around one avr_field_fwd_points launch on the live samples.
//
//   avr_occ_build     sigma planes -> bits          one lane per cell, 64 cells = one ballot = two bit words
//   avr_occ_classify  (ro, rd, z)  -> mask, counts  one wave per ray, one lane per sample, one ballot per 64 samples
//   avr_occ_compact   mask, offsets -> xyz, viewdirs of the live samples, ray-major sample order
//   avr_occ_expand    field of the live samples -> the dense (R*N, 4) field, zeros for dead samples
// and, for the chain that keeps the live count on the device (capturable in a graph; DESIGN.md "Occupancy grid:
// device-side live count"):
//   avr_occ_scan             counts -> offsets (exclusive int64 prefix sums) and their total, reduce then scan
//   avr_occ_compact_counted  avr_occ_compact with n_live read from the device, buffers sized by a host capacity
//   avr_occ_expand_counted   avr_occ_expand likewise
//
// A live sample's rank in the compacted list is offsets[ray] + popcount of the lower mask bits of its ray: no slot
// array, no atomics, no data-dependent order, so every output is bit-reproducible. The point is formed with the
// operations of field_common.h's sample_geom (fadd(ro, fmul(rd, z))), so a compacted point is the point
// avr_field_fwd_rays would have formed, bit for bit. All four are bandwidth-trivial next to the field kernel; the
// grid (at most 2 Mbit) stays in L2. The grid, the live test, the rank, the point and the clamped device count are
// skip_common.h's, shared with march_device.hip.
#include "skip_common.h"

namespace avr {

constexpr int kOccThreads = 256;
constexpr int kOccRaysPerBlock = kOccThreads / kWave;

__global__ void __launch_bounds__(kOccThreads) occ_build_kernel(const float* __restrict__ sigma, int n_planes, int rx,
                                                                 int ry, int rz, float thr, int dilate,
                                                                 uint32_t* __restrict__ bits) {
  const int n_cells = rx * ry * rz;   // <= 2^24
  const int cell = blockIdx.x * kOccThreads + threadIdx.x;
  bool occ = false;
  if (cell < n_cells) {
    const int ix = cell % rx, iy = (cell / rx) % ry, iz = cell / (rx * ry);
    const int x0 = max(ix - dilate, 0), x1 = min(ix + dilate, rx - 1);
    const int y0 = max(iy - dilate, 0), y1 = min(iy + dilate, ry - 1);
    const int z0 = max(iz - dilate, 0), z1 = min(iz + dilate, rz - 1);
    for (int k = 0; k < n_planes && !occ; ++k) {
      const float* plane = sigma + (int64_t)k * n_cells;
      for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y)
          for (int x = x0; x <= x1; ++x) occ |= !(plane[(z * ry + y) * rx + x] <= thr);   // NaN: occupied
    }
  }
  const uint64_t m = __ballot(occ);   // cells 64 * wave .. + 63: words 2 * wave and 2 * wave + 1 (rx % 32 == 0)
  const int lane = threadIdx.x & (kWave - 1);
  if ((lane == 0 || lane == 32) && cell < n_cells) bits[cell >> 5] = (uint32_t)(m >> lane);
}

__global__ void __launch_bounds__(kOccThreads) occ_classify_kernel(OccGrid g, const float* __restrict__ ro,
                                                                    const float* __restrict__ rd,
                                                                    const float* __restrict__ z, int64_t n_rays,
                                                                    int n_samples, uint64_t* __restrict__ mask,
                                                                    int32_t* __restrict__ counts) {
  const int64_t r = (int64_t)blockIdx.x * kOccRaysPerBlock + (threadIdx.x >> 6);
  if (r >= n_rays) return;   // whole waves leave together
  const int lane = threadIdx.x & (kWave - 1);
  const int n_words = (n_samples + kWave - 1) / kWave;
  int count = 0;
  for (int w = 0; w < n_words; ++w) {
    const int s = w * kWave + lane;
    bool live = false;
    if (s < n_samples) {
      const Point3 p = sample_point(ro, rd, r, z[r * n_samples + s]);
      live = occ_live(g, p.x, p.y, p.z);
    }
    const uint64_t m = __ballot(live);
    if (lane == 0) mask[r * n_words + w] = m;
    count += __popcll(m);
  }
  if (lane == 0) counts[r] = count;
}

__device__ __forceinline__ void occ_compact_body(const float* __restrict__ ro, const float* __restrict__ rd,
                                                 const float* __restrict__ z, const uint64_t* __restrict__ mask,
                                                 const int64_t* __restrict__ offsets, int64_t n_rays, int n_samples,
                                                 int64_t n_live, float* __restrict__ xyz, float* __restrict__ vd) {
  const int64_t r = (int64_t)blockIdx.x * kOccRaysPerBlock + (threadIdx.x >> 6);
  if (r >= n_rays) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int n_words = (n_samples + kWave - 1) / kWave;
  const float d0 = rd[3 * r], d1 = rd[3 * r + 1], d2 = rd[3 * r + 2];
  int64_t base = offsets[r];
  for (int w = 0; w < n_words; ++w) {
    const uint64_t m = mask[r * n_words + w];
    const int s = w * kWave + lane;
    const int64_t q = base + lane_rank(m, lane);
    // s < n_samples and 0 <= q < n_live hold for the mask and offsets of avr_occ_classify; checked so that
    // inconsistent arguments cannot write outside xyz / viewdirs
    if (((m >> lane) & 1ull) && s < n_samples && q >= 0 && q < n_live) {
      const Point3 p = sample_point(ro, rd, r, z[r * n_samples + s]);
      xyz[3 * q] = p.x; xyz[3 * q + 1] = p.y; xyz[3 * q + 2] = p.z;
      vd[3 * q] = d0; vd[3 * q + 1] = d1; vd[3 * q + 2] = d2;
    }
    base += __popcll(m);
  }
}

__global__ void __launch_bounds__(kOccThreads) occ_compact_kernel(const float* __restrict__ ro,
                                                                   const float* __restrict__ rd,
                                                                   const float* __restrict__ z,
                                                                   const uint64_t* __restrict__ mask,
                                                                   const int64_t* __restrict__ offsets, int64_t n_rays,
                                                                   int n_samples, int64_t n_live,
                                                                   float* __restrict__ xyz, float* __restrict__ vd) {
  occ_compact_body(ro, rd, z, mask, offsets, n_rays, n_samples, n_live, xyz, vd);
}

__global__ void __launch_bounds__(kOccThreads) occ_compact_counted_kernel(
    const float* __restrict__ ro, const float* __restrict__ rd, const float* __restrict__ z,
    const uint64_t* __restrict__ mask, const int64_t* __restrict__ offsets, int64_t n_rays, int n_samples,
    const int64_t* __restrict__ n_live, int64_t capacity, float* __restrict__ xyz, float* __restrict__ vd) {
  const int64_t live = counted_live(n_live, capacity);
  if (live == 0) return;
  occ_compact_body(ro, rd, z, mask, offsets, n_rays, n_samples, live, xyz, vd);
}

__device__ __forceinline__ void occ_expand_body(const floatx4* __restrict__ field_c, const uint64_t* __restrict__ mask,
                                                const int64_t* __restrict__ offsets, int64_t n_rays, int n_samples,
                                                int64_t n_live, floatx4* __restrict__ field) {
  const int64_t r = (int64_t)blockIdx.x * kOccRaysPerBlock + (threadIdx.x >> 6);
  if (r >= n_rays) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int n_words = (n_samples + kWave - 1) / kWave;
  int64_t base = n_live > 0 ? offsets[r] : 0;
  for (int w = 0; w < n_words; ++w) {
    const uint64_t m = n_live > 0 ? mask[r * n_words + w] : 0ull;
    const int s = w * kWave + lane;
    const int64_t q = base + lane_rank(m, lane);
    floatx4 v = {0.f, 0.f, 0.f, 0.f};
    if (((m >> lane) & 1ull) && q >= 0 && q < n_live) v = field_c[q];   // (the range check: as in occ_compact_body)
    if (s < n_samples) field[r * n_samples + s] = v;
    base += __popcll(m);
  }
}

__global__ void __launch_bounds__(kOccThreads) occ_expand_kernel(const floatx4* __restrict__ field_c,
                                                                  const uint64_t* __restrict__ mask,
                                                                  const int64_t* __restrict__ offsets, int64_t n_rays,
                                                                  int n_samples, int64_t n_live,
                                                                  floatx4* __restrict__ field) {
  occ_expand_body(field_c, mask, offsets, n_rays, n_samples, n_live, field);
}

__global__ void __launch_bounds__(kOccThreads) occ_expand_counted_kernel(
    const floatx4* __restrict__ field_c, const uint64_t* __restrict__ mask, const int64_t* __restrict__ offsets,
    int64_t n_rays, int n_samples, const int64_t* __restrict__ n_live, int64_t capacity, floatx4* __restrict__ field) {
  occ_expand_body(field_c, mask, offsets, n_rays, n_samples, counted_live(n_live, capacity), field);
}

// ---- avr_occ_scan: exclusive int64 prefix sums of the per-ray counts and their total, on the device. Reduce, then
// scan, in separate launches: no workgroup waits on another. A workgroup owns kOccScanRays consecutive rays, a
// thread kOccScanItems consecutive ones of those. The workgroup sums need no scratch: workgroup b's sum lives in
// offsets[b * kOccScanRays], the first slot of its own range, between the launches:
//   occ_scan_reduce_kernel    sum of workgroup b's counts -> offsets[b * kOccScanRays]
//   occ_scan_partials_kernel  (one workgroup) those sums -> their exclusive prefix sums in place, *total
//   occ_scan_block_kernel     carry = offsets[b * kOccScanRays], read by every thread ahead of the barrier that
//                             precedes the first store; offsets of workgroup b's rays
// Up to kOccScanRays rays take the last kernel alone (carry 0, it writes *total). Integer adds only.
constexpr int kOccScanItems = 8;
constexpr int kOccScanRays = kOccThreads * kOccScanItems;
static_assert(kOccScanRays == AVR_OCC_SCAN_RAYS, "avr.h AVR_OCC_SCAN_RAYS");

__device__ __forceinline__ int64_t wave_incl_scan_i64(int64_t v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const long long o = __shfl_up((long long)v, d, kWave);
    if (lane >= d) v += o;
  }
  return v;
}

// Exclusive prefix of v over the workgroup's threads, and the workgroup's total (wsum: kOccRaysPerBlock LDS words;
// two barriers, every thread of the workgroup calls it).
__device__ __forceinline__ int64_t block_excl_scan_i64(int64_t v, int64_t* wsum, int64_t& total) {
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x >> 6;
  const int64_t incl = wave_incl_scan_i64(v, lane);
  if (lane == kWave - 1) wsum[wid] = incl;
  __syncthreads();
  int64_t pre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kOccRaysPerBlock; ++w) {
    const int64_t s = wsum[w];
    if (w < wid) pre += s;
    tot += s;
  }
  __syncthreads();
  total = tot;
  return pre + incl - v;
}

__device__ __forceinline__ int64_t scan_load(const int32_t* __restrict__ counts, int64_t n_rays, int64_t first,
                                             int32_t (&c)[kOccScanItems]) {
  int64_t sum = 0;
#pragma unroll
  for (int i = 0; i < kOccScanItems; ++i) {
    c[i] = first + i < n_rays ? counts[first + i] : 0;
    sum += c[i];
  }
  return sum;
}

__global__ void __launch_bounds__(kOccThreads) occ_scan_reduce_kernel(const int32_t* __restrict__ counts,
                                                                       int64_t n_rays, int64_t* __restrict__ offsets) {
  __shared__ int64_t wsum[kOccRaysPerBlock];
  int32_t c[kOccScanItems];
  const int64_t first = (int64_t)blockIdx.x * kOccScanRays + threadIdx.x * kOccScanItems;
  int64_t total;
  block_excl_scan_i64(scan_load(counts, n_rays, first, c), wsum, total);
  if (threadIdx.x == 0) offsets[(int64_t)blockIdx.x * kOccScanRays] = total;   // (block b's first ray is < n_rays)
}

__global__ void __launch_bounds__(kOccThreads) occ_scan_partials_kernel(int64_t* __restrict__ offsets,
                                                                         int64_t n_blocks,
                                                                         int64_t* __restrict__ total) {
  __shared__ int64_t wsum[kOccRaysPerBlock];
  int64_t carry = 0;
  for (int64_t p0 = 0; p0 < n_blocks; p0 += kOccThreads) {   // (uniform: every thread makes every trip)
    const int64_t p = p0 + threadIdx.x;
    const int64_t v = p < n_blocks ? offsets[p * kOccScanRays] : 0;
    int64_t tot;
    const int64_t pre = block_excl_scan_i64(v, wsum, tot);
    if (p < n_blocks) offsets[p * kOccScanRays] = carry + pre;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}

template <bool SINGLE>
__global__ void __launch_bounds__(kOccThreads) occ_scan_block_kernel(const int32_t* __restrict__ counts,
                                                                      int64_t n_rays, int64_t* offsets,
                                                                      int64_t* __restrict__ total) {
  __shared__ int64_t wsum[kOccRaysPerBlock];
  int32_t c[kOccScanItems];
  const int64_t carry = SINGLE ? 0 : offsets[(int64_t)blockIdx.x * kOccScanRays];
  const int64_t first = (int64_t)blockIdx.x * kOccScanRays + threadIdx.x * kOccScanItems;
  const int64_t sum = scan_load(counts, n_rays, first, c);
  int64_t tot;
  int64_t run = carry + block_excl_scan_i64(sum, wsum, tot);   // (its barriers: every carry is read by now)
#pragma unroll
  for (int i = 0; i < kOccScanItems; ++i) {
    if (first + i < n_rays) offsets[first + i] = run;
    run += c[i];
  }
  if (SINGLE && threadIdx.x == 0) *total = tot;
}

}  // namespace avr

using namespace avr;

static int occ_rays(const char* who, int64_t n_rays, int n_samples, int64_t* blocks) {
  AVR_REQUIRE(n_rays >= 0, "%s: negative n_rays", who);
  AVR_REQUIRE(n_samples >= 1 && n_samples <= AVR_OCC_MAX_SAMPLES, "%s: n_samples %d outside 1..%d", who, n_samples,
              AVR_OCC_MAX_SAMPLES);
  *blocks = (n_rays + kOccRaysPerBlock - 1) / kOccRaysPerBlock;
  AVR_REQUIRE(*blocks < (1ll << 31), "%s: too many rays", who);
  return AVR_OK;
}

extern "C" int avr_occ_build(const float* sigma, int n_planes, const int* res, float thr, int dilate, uint32_t* bits,
                             void* stream) {
  int rc = occ_res("avr_occ_build", res);
  if (rc) return rc;
  AVR_REQUIRE(n_planes >= 1, "avr_occ_build: n_planes %d below 1", n_planes);
  AVR_REQUIRE(dilate >= 0 && dilate <= 2, "avr_occ_build: dilate %d outside 0..2", dilate);
  AVR_REQUIRE(sigma && bits, "avr_occ_build: null pointer");
  const int n_cells = res[0] * res[1] * res[2];
  occ_build_kernel<<<(unsigned)((n_cells + kOccThreads - 1) / kOccThreads), kOccThreads, 0, as_stream(stream)>>>(
      sigma, n_planes, res[0], res[1], res[2], thr, dilate, bits);
  return check_launch("occ_build_kernel");
}

extern "C" int avr_occ_classify(const avr_occ_grid* grid, const float* ro, const float* rd, const float* z,
                                int64_t n_rays, int n_samples, uint64_t* mask, int32_t* counts, void* stream) {
  int64_t blocks;
  OccGrid g;
  int rc = occ_grid_arg("avr_occ_classify", grid, false, &g);
  if (rc || (rc = occ_rays("avr_occ_classify", n_rays, n_samples, &blocks))) return rc;
  if (n_rays == 0) return AVR_OK;
  AVR_REQUIRE(ro && rd && z && mask && counts, "avr_occ_classify: null pointer");
  occ_classify_kernel<<<(unsigned)blocks, kOccThreads, 0, as_stream(stream)>>>(g, ro, rd, z, n_rays, n_samples, mask,
                                                                              counts);
  return check_launch("occ_classify_kernel");
}

extern "C" int avr_occ_compact(const float* ro, const float* rd, const float* z, const uint64_t* mask,
                               const int64_t* offsets, int64_t n_rays, int n_samples, int64_t n_live, float* xyz,
                               float* viewdirs, void* stream) {
  int64_t blocks;
  int rc = occ_rays("avr_occ_compact", n_rays, n_samples, &blocks);
  if (rc) return rc;
  AVR_REQUIRE(n_live >= 0 && n_live <= n_rays * n_samples, "avr_occ_compact: n_live %lld outside 0..n_rays * n_samples",
              (long long)n_live);
  if (n_rays == 0 || n_live == 0) return AVR_OK;
  AVR_REQUIRE(ro && rd && z && mask && offsets && xyz && viewdirs, "avr_occ_compact: null pointer");
  occ_compact_kernel<<<(unsigned)blocks, kOccThreads, 0, as_stream(stream)>>>(ro, rd, z, mask, offsets, n_rays,
                                                                             n_samples, n_live, xyz, viewdirs);
  return check_launch("occ_compact_kernel");
}

extern "C" int avr_occ_expand(const float* field_c, const uint64_t* mask, const int64_t* offsets, int64_t n_rays,
                              int n_samples, int64_t n_live, float* field, void* stream) {
  int64_t blocks;
  int rc = occ_rays("avr_occ_expand", n_rays, n_samples, &blocks);
  if (rc) return rc;
  AVR_REQUIRE(n_live >= 0 && n_live <= n_rays * n_samples, "avr_occ_expand: n_live %lld outside 0..n_rays * n_samples",
              (long long)n_live);
  if (n_rays == 0) return AVR_OK;
  AVR_REQUIRE(field, "avr_occ_expand: null field");
  AVR_REQUIRE(n_live == 0 || (field_c && mask && offsets), "avr_occ_expand: null pointer with n_live > 0");
  AVR_REQUIRE((((uintptr_t)field | (uintptr_t)field_c) & 15) == 0, "avr_occ_expand: field rows must be 16-B aligned");
  occ_expand_kernel<<<(unsigned)blocks, kOccThreads, 0, as_stream(stream)>>>(
      reinterpret_cast<const floatx4*>(field_c), mask, offsets, n_rays, n_samples, n_live,
      reinterpret_cast<floatx4*>(field));
  return check_launch("occ_expand_kernel");
}

extern "C" int avr_occ_scan(const int32_t* counts, int64_t n_rays, int64_t* offsets, int64_t* total, void* stream) {
  AVR_REQUIRE(n_rays >= 0, "avr_occ_scan: negative n_rays");
  AVR_REQUIRE(total, "avr_occ_scan: null total");
  AVR_REQUIRE(n_rays == 0 || (counts && offsets), "avr_occ_scan: null pointer");
  AVR_REQUIRE((((uintptr_t)offsets | (uintptr_t)total) & 7) == 0 && ((uintptr_t)counts & 3) == 0,
              "avr_occ_scan: misaligned pointer");
  const int64_t blocks = (n_rays + kOccScanRays - 1) / kOccScanRays;
  AVR_REQUIRE(blocks < (1ll << 31), "avr_occ_scan: too many rays");
  hipStream_t s = as_stream(stream);
  if (blocks <= 1) {
    if (blocks == 0) {
      occ_scan_partials_kernel<<<1, kOccThreads, 0, s>>>(offsets, 0, total);   // *total = 0
      return check_launch("occ_scan_partials_kernel");
    }
    occ_scan_block_kernel<true><<<1, kOccThreads, 0, s>>>(counts, n_rays, offsets, total);
    return check_launch("occ_scan_block_kernel");
  }
  occ_scan_reduce_kernel<<<(unsigned)blocks, kOccThreads, 0, s>>>(counts, n_rays, offsets);
  int rc = check_launch("occ_scan_reduce_kernel");
  if (rc) return rc;
  occ_scan_partials_kernel<<<1, kOccThreads, 0, s>>>(offsets, blocks, total);
  if ((rc = check_launch("occ_scan_partials_kernel"))) return rc;
  occ_scan_block_kernel<false><<<(unsigned)blocks, kOccThreads, 0, s>>>(counts, n_rays, offsets, total);
  return check_launch("occ_scan_block_kernel");
}

extern "C" int avr_occ_compact_counted(const float* ro, const float* rd, const float* z, const uint64_t* mask,
                                       const int64_t* offsets, int64_t n_rays, int n_samples, const int64_t* n_live,
                                       int64_t capacity, float* xyz, float* viewdirs, void* stream) {
  int64_t blocks;
  int rc = occ_rays("avr_occ_compact_counted", n_rays, n_samples, &blocks);
  if (rc || (rc = counted_capacity("avr_occ_compact_counted", capacity, n_rays, n_samples, "n_samples"))) return rc;
  if (n_rays == 0 || capacity == 0) return AVR_OK;
  AVR_REQUIRE(ro && rd && z && mask && offsets && n_live && xyz && viewdirs, "avr_occ_compact_counted: null pointer");
  AVR_REQUIRE(((uintptr_t)n_live & 7) == 0, "avr_occ_compact_counted: n_live must be 8-B aligned");
  occ_compact_counted_kernel<<<(unsigned)blocks, kOccThreads, 0, as_stream(stream)>>>(
      ro, rd, z, mask, offsets, n_rays, n_samples, n_live, capacity, xyz, viewdirs);
  return check_launch("occ_compact_counted_kernel");
}

extern "C" int avr_occ_expand_counted(const float* field_c, const uint64_t* mask, const int64_t* offsets,
                                      int64_t n_rays, int n_samples, const int64_t* n_live, int64_t capacity,
                                      float* field, void* stream) {
  int64_t blocks;
  int rc = occ_rays("avr_occ_expand_counted", n_rays, n_samples, &blocks);
  if (rc || (rc = counted_capacity("avr_occ_expand_counted", capacity, n_rays, n_samples, "n_samples"))) return rc;
  if (n_rays == 0 || capacity == 0) return AVR_OK;
  AVR_REQUIRE(field_c && mask && offsets && n_live && field, "avr_occ_expand_counted: null pointer");
  AVR_REQUIRE(((uintptr_t)n_live & 7) == 0, "avr_occ_expand_counted: n_live must be 8-B aligned");
  AVR_REQUIRE((((uintptr_t)field | (uintptr_t)field_c) & 15) == 0,
              "avr_occ_expand_counted: field rows must be 16-B aligned");
  occ_expand_counted_kernel<<<(unsigned)blocks, kOccThreads, 0, as_stream(stream)>>>(
      reinterpret_cast<const floatx4*>(field_c), mask, offsets, n_rays, n_samples, n_live, capacity,
      reinterpret_cast<floatx4*>(field));
  return check_launch("occ_expand_counted_kernel");
}
