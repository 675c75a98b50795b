// Hierarchical occupancy-grid build (not in the reference; DESIGN.md "Occupancy grid: hierarchical build",
// include/avr.h "occupancy grid: hierarchical build"): the field is evaluated at the fine cells under live coarse
// cells only. The chain is the gating chain of occupancy.hip with a fine x-row for the ray and a cell of that row
// for the sample:
//
//   avr_occ_children      coarse bits, factor -> mask, counts   one wave per fine row, one ballot per 64 cells
//   avr_occ_scan          counts -> offsets, total              (occupancy.hip, as it is)
//   avr_occ_child_points  mask, offsets -> xyz, viewdirs        the candidates' centres, in linear fine-cell order
//   avr_occ_flag_sigma    field rows of the candidates -> one byte per candidate, OR-ed over the planes
//   avr_occ_build_sparse  mask, offsets, flags -> bits          one lane per fine cell, occ_build_kernel's ballot
//   avr_occ_downsample    bits -> the OR of every p^3 children
//
// A candidate's rank is offsets[row] + popcount of the lower mask bits of its row (skip_common.h's rule over the
// row's words): no slot array, no atomics, no memset, no data-dependent order. All five are bandwidth-trivial next
// to the field launches they size; the masks (at most 2 Mbit) and the coarse bits stay in L2.
#include "skip_common.h"

namespace avr {

constexpr int kRefThreads = 256;
constexpr int kRefRowsPerBlock = kRefThreads / kWave;

struct RefineAxes {   // lo64[a] and step[a] of the fine grid, from the host, in double
  double lo[3], step[3];
};

// Cell ix's rank among its row's candidates: the set bits of the row's mask words below it.
__device__ __forceinline__ int row_rank(const uint64_t* __restrict__ mrow, int ix) {
  int rank = 0;
  for (int w = 0; w < (ix >> 6); ++w) rank += __popcll(mrow[w]);
  return rank + lane_rank(mrow[ix >> 6], ix & 63);
}

// c = float(lo + (i + 0.5) * step): the product and the sum each rounded once in double, never fused.
__device__ __forceinline__ float cell_centre(double lo, double step, int i) {
  return (float)__dadd_rn(lo, __dmul_rn((double)i + 0.5, step));
}

__global__ void __launch_bounds__(kRefThreads) occ_children_kernel(const uint32_t* __restrict__ cbits, int cwords,
                                                                    int cry, int f, int rx, int ry, int rz,
                                                                    uint64_t* __restrict__ mask,
                                                                    int32_t* __restrict__ counts) {
  const int row = blockIdx.x * kRefRowsPerBlock + (threadIdx.x >> 6);
  if (row >= ry * rz) return;   // whole waves leave together
  const int lane = threadIdx.x & (kWave - 1);
  const int n_words = (rx + kWave - 1) / kWave;
  const int iy = row % ry, iz = row / ry;
  const uint32_t* crow = cbits + ((iz / f) * cry + iy / f) * cwords;
  int count = 0;
  for (int w = 0; w < n_words; ++w) {
    const int ix = w * kWave + lane;
    bool cand = false;
    if (ix < rx) {
      const int cx = ix / f;
      cand = (crow[cx >> 5] >> (cx & 31)) & 1u;
    }
    const uint64_t m = __ballot(cand);
    if (lane == 0) mask[(int64_t)row * n_words + w] = m;
    count += __popcll(m);
  }
  if (lane == 0) counts[row] = count;
}

__global__ void __launch_bounds__(kRefThreads) occ_child_points_kernel(const uint64_t* __restrict__ mask,
                                                                        const int64_t* __restrict__ offsets, int rx,
                                                                        int ry, int rz, RefineAxes ax, float d0,
                                                                        float d1, float d2, int64_t n_live,
                                                                        float* __restrict__ xyz,
                                                                        float* __restrict__ vd) {
  const int row = blockIdx.x * kRefRowsPerBlock + (threadIdx.x >> 6);
  if (row >= ry * rz) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int n_words = (rx + kWave - 1) / kWave;
  const float cy = cell_centre(ax.lo[1], ax.step[1], row % ry), cz = cell_centre(ax.lo[2], ax.step[2], row / ry);
  int64_t base = offsets[row];
  for (int w = 0; w < n_words; ++w) {
    const uint64_t m = mask[(int64_t)row * n_words + w];
    const int ix = w * kWave + lane;
    const int64_t q = base + lane_rank(m, lane);
    // ix < rx and 0 <= q < n_live hold for the mask and offsets of avr_occ_children; checked so that inconsistent
    // arguments cannot write outside xyz / viewdirs
    if (((m >> lane) & 1ull) && ix < rx && q >= 0 && q < n_live) {
      if (xyz) { xyz[3 * q] = cell_centre(ax.lo[0], ax.step[0], ix); xyz[3 * q + 1] = cy; xyz[3 * q + 2] = cz; }
      if (vd) { vd[3 * q] = d0; vd[3 * q + 1] = d1; vd[3 * q + 2] = d2; }
    }
    base += __popcll(m);
  }
}

__global__ void __launch_bounds__(kRefThreads) occ_flag_sigma_kernel(const floatx4* __restrict__ field_c, float thr,
                                                                      int first, int64_t n_live,
                                                                      uint8_t* __restrict__ flags) {
  const int64_t q = (int64_t)blockIdx.x * kRefThreads + threadIdx.x;
  if (q >= n_live) return;
  const uint8_t occ = !(field_c[q].w <= thr);   // NaN: occupied
  flags[q] = (uint8_t)((first ? 0 : flags[q]) | occ);
}

__global__ void __launch_bounds__(kRefThreads) occ_build_sparse_kernel(const uint64_t* __restrict__ mask,
                                                                        const int64_t* __restrict__ offsets,
                                                                        const uint8_t* __restrict__ flags,
                                                                        int64_t n_live, int rx, int ry, int rz,
                                                                        int dilate, uint32_t* __restrict__ bits) {
  const int n_cells = rx * ry * rz;   // <= 2^24
  const int cell = blockIdx.x * kRefThreads + threadIdx.x;
  const int n_words = (rx + kWave - 1) / kWave;
  bool occ = false;
  if (cell < n_cells && n_live > 0) {
    const int ix = cell % rx, iy = (cell / rx) % ry, iz = cell / (rx * ry);
    const int x0 = max(ix - dilate, 0), x1 = min(ix + dilate, rx - 1);
    const int y0 = max(iy - dilate, 0), y1 = min(iy + dilate, ry - 1);
    const int z0 = max(iz - dilate, 0), z1 = min(iz + dilate, rz - 1);
    for (int z = z0; z <= z1 && !occ; ++z)
      for (int y = y0; y <= y1 && !occ; ++y) {
        const int row = z * ry + y;
        const uint64_t* mrow = mask + (int64_t)row * n_words;
        for (int x = x0; x <= x1; ++x) {
          if (!((mrow[x >> 6] >> (x & 63)) & 1ull)) continue;   // not a candidate: its sigma counts as 0
          const int64_t q = offsets[row] + row_rank(mrow, x);
          if (q >= 0 && q < n_live) occ |= flags[q] != 0;       // (the range check: as in occ_child_points_kernel)
        }
      }
  }
  const uint64_t m = __ballot(occ);   // cells 64 * wave .. + 63: words 2 * wave and 2 * wave + 1 (rx % 32 == 0)
  const int lane = threadIdx.x & (kWave - 1);
  if ((lane == 0 || lane == 32) && cell < n_cells) bits[cell >> 5] = (uint32_t)(m >> lane);
}

__global__ void __launch_bounds__(kRefThreads) occ_downsample_kernel(const uint32_t* __restrict__ bits, int rx, int ry,
                                                                      int p, int cx, int cy, int cz,
                                                                      uint32_t* __restrict__ cbits) {
  const int n_cells = cx * cy * cz;
  const int cell = blockIdx.x * kRefThreads + threadIdx.x;
  bool occ = false;
  if (cell < n_cells) {
    const int ix = cell % cx, iy = (cell / cx) % cy, iz = cell / (cx * cy);
    for (int z = iz * p; z < (iz + 1) * p; ++z)
      for (int y = iy * p; y < (iy + 1) * p; ++y) {
        const uint32_t* frow = bits + (z * ry + y) * (rx >> 5);
        for (int x = ix * p; x < (ix + 1) * p; ++x) occ |= (frow[x >> 5] >> (x & 31)) & 1u;
      }
  }
  const uint64_t m = __ballot(occ);   // (cx % 32 == 0: the two-word store of occ_build_kernel)
  const int lane = threadIdx.x & (kWave - 1);
  if ((lane == 0 || lane == 32) && cell < n_cells) cbits[cell >> 5] = (uint32_t)(m >> lane);
}

}  // namespace avr

using namespace avr;

static int refine_factor(const char* who, const int* res, int factor) {
  AVR_REQUIRE(factor == 2 || factor == 4 || factor == 8, "%s: factor %d is not 2, 4 or 8", who, factor);
  for (int a = 0; a < 3; ++a)
    AVR_REQUIRE(res[a] % factor == 0, "%s: res[%d] = %d is not divisible by factor %d", who, a, res[a], factor);
  AVR_REQUIRE((res[0] / factor) % 32 == 0, "%s: coarse res[0] = %d is not a multiple of 32", who, res[0] / factor);
  return AVR_OK;
}

static int refine_live(const char* who, const int* res, int64_t n_live) {
  AVR_REQUIRE(n_live >= 0 && n_live <= (int64_t)res[0] * res[1] * res[2], "%s: n_live %lld outside 0..rx * ry * rz",
              who, (long long)n_live);
  return AVR_OK;
}

static unsigned refine_row_blocks(const int* res) {
  return (unsigned)((res[1] * res[2] + kRefRowsPerBlock - 1) / kRefRowsPerBlock);
}

extern "C" int avr_occ_children(const avr_occ_grid* coarse, int factor, const int* res, uint64_t* mask,
                                int32_t* counts, void* stream) {
  OccGrid c;
  int rc = occ_grid_arg("avr_occ_children", coarse, false, &c);
  if (rc || (rc = occ_res("avr_occ_children", res)) || (rc = refine_factor("avr_occ_children", res, factor)))
    return rc;
  for (int a = 0; a < 3; ++a)
    AVR_REQUIRE(c.res[a] * factor == res[a], "avr_occ_children: coarse res[%d] = %d is not res[%d] / factor = %d", a,
                c.res[a], a, res[a] / factor);
  AVR_REQUIRE(mask && counts, "avr_occ_children: null pointer");
  AVR_REQUIRE(((uintptr_t)mask & 7) == 0 && ((uintptr_t)counts & 3) == 0, "avr_occ_children: misaligned pointer");
  occ_children_kernel<<<refine_row_blocks(res), kRefThreads, 0, as_stream(stream)>>>(
      c.bits, c.res[0] >> 5, c.res[1], factor, res[0], res[1], res[2], mask, counts);
  return check_launch("occ_children_kernel");
}

extern "C" int avr_occ_child_points(const uint64_t* mask, const int64_t* offsets, const int* res, const double* lo64,
                                    const double* step, const float* dir, int64_t n_live, float* xyz, float* viewdirs,
                                    void* stream) {
  int rc = occ_res("avr_occ_child_points", res);
  if (rc || (rc = refine_live("avr_occ_child_points", res, n_live))) return rc;
  if (n_live == 0) return AVR_OK;
  AVR_REQUIRE(lo64 && step, "avr_occ_child_points: null lo64 or step");
  for (int a = 0; a < 3; ++a)
    AVR_REQUIRE(lo64[a] - lo64[a] == 0.0 && step[a] > 0.0 && step[a] - step[a] == 0.0,
                "avr_occ_child_points: lo64[%d] must be finite and step[%d] finite and positive", a, a);
  AVR_REQUIRE(xyz || viewdirs, "avr_occ_child_points: null xyz and viewdirs");
  AVR_REQUIRE(!viewdirs || dir, "avr_occ_child_points: null dir with viewdirs");
  AVR_REQUIRE(mask && offsets, "avr_occ_child_points: null pointer");
  AVR_REQUIRE((((uintptr_t)mask | (uintptr_t)offsets) & 7) == 0,
              "avr_occ_child_points: mask and offsets must be 8-B aligned");
  RefineAxes ax;
  for (int a = 0; a < 3; ++a) { ax.lo[a] = lo64[a]; ax.step[a] = step[a]; }
  const float d0 = viewdirs ? dir[0] : 0.f, d1 = viewdirs ? dir[1] : 0.f, d2 = viewdirs ? dir[2] : 0.f;
  occ_child_points_kernel<<<refine_row_blocks(res), kRefThreads, 0, as_stream(stream)>>>(
      mask, offsets, res[0], res[1], res[2], ax, d0, d1, d2, n_live, xyz, viewdirs);
  return check_launch("occ_child_points_kernel");
}

extern "C" int avr_occ_flag_sigma(const float* field_c, float thr, int first, int64_t n_live, uint8_t* flags,
                                  void* stream) {
  AVR_REQUIRE(thr >= 0.f, "avr_occ_flag_sigma: thr must be >= 0 (a negative or NaN thr calls unevaluated cells "
              "occupied)");
  AVR_REQUIRE(n_live >= 0, "avr_occ_flag_sigma: negative n_live");
  const int64_t blocks = (n_live + kRefThreads - 1) / kRefThreads;
  AVR_REQUIRE(blocks < (1ll << 31), "avr_occ_flag_sigma: n_live too large");
  if (n_live == 0) return AVR_OK;
  AVR_REQUIRE(field_c && flags, "avr_occ_flag_sigma: null pointer");
  AVR_REQUIRE(((uintptr_t)field_c & 15) == 0, "avr_occ_flag_sigma: field rows must be 16-B aligned");
  occ_flag_sigma_kernel<<<(unsigned)blocks, kRefThreads, 0, as_stream(stream)>>>(
      reinterpret_cast<const floatx4*>(field_c), thr, first, n_live, flags);
  return check_launch("occ_flag_sigma_kernel");
}

extern "C" int avr_occ_build_sparse(const uint64_t* mask, const int64_t* offsets, const uint8_t* flags,
                                    int64_t n_live, const int* res, int dilate, uint32_t* bits, void* stream) {
  int rc = occ_res("avr_occ_build_sparse", res);
  if (rc || (rc = refine_live("avr_occ_build_sparse", res, n_live))) return rc;
  AVR_REQUIRE(dilate >= 0 && dilate <= 2, "avr_occ_build_sparse: dilate %d outside 0..2", dilate);
  AVR_REQUIRE(bits, "avr_occ_build_sparse: null bits");
  AVR_REQUIRE(n_live == 0 || (mask && offsets && flags), "avr_occ_build_sparse: null pointer with n_live > 0");
  AVR_REQUIRE((((uintptr_t)mask | (uintptr_t)offsets) & 7) == 0,
              "avr_occ_build_sparse: mask and offsets must be 8-B aligned");
  const int n_cells = res[0] * res[1] * res[2];
  occ_build_sparse_kernel<<<(unsigned)((n_cells + kRefThreads - 1) / kRefThreads), kRefThreads, 0,
                            as_stream(stream)>>>(mask, offsets, flags, n_live, res[0], res[1], res[2], dilate, bits);
  return check_launch("occ_build_sparse_kernel");
}

extern "C" int avr_occ_downsample(const uint32_t* bits, const int* res, int p, uint32_t* coarse_bits, void* stream) {
  int rc = occ_res("avr_occ_downsample", res);
  if (rc) return rc;
  AVR_REQUIRE(p == 1 || p == 2 || p == 4, "avr_occ_downsample: p %d is not 1, 2 or 4", p);
  for (int a = 0; a < 3; ++a)
    AVR_REQUIRE(res[a] % p == 0, "avr_occ_downsample: res[%d] = %d is not divisible by p %d", a, res[a], p);
  AVR_REQUIRE((res[0] / p) % 32 == 0, "avr_occ_downsample: coarse res[0] = %d is not a multiple of 32", res[0] / p);
  AVR_REQUIRE(bits && coarse_bits, "avr_occ_downsample: null pointer");
  const int cx = res[0] / p, cy = res[1] / p, cz = res[2] / p;
  const int n_cells = cx * cy * cz;
  occ_downsample_kernel<<<(unsigned)((n_cells + kRefThreads - 1) / kRefThreads), kRefThreads, 0,
                          as_stream(stream)>>>(bits, res[0], res[1], p, cx, cy, cz, coarse_bits);
  return check_launch("occ_downsample_kernel");
}
