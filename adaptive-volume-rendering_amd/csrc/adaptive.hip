// Inference front end of AdaptiveVolumeRenderer / Raymarcher (renderers.py:313-343, :380-432, :490-496) in one
// launch, for several scenes: per ray
//   d0     = the given start distance, or 0.8 + 0.05 * N(0, 1) from Philox (normal_(mean=0.8, std=5e-2))
//   world  = the LSTM march from ro + rd * d0 (lstm_march.h: raymarch_kernel's instructions, nothing stored per
//            step)
//   z      = sample_coarse(d - eps, d + eps, n_band) sorted ascending, d = (world_x - ro_x) / rd_x (quirk kept:
//            rd_x = 0 gives a NaN row), with the given noise or Philox uniforms (band_fwd_kernel's operations
//            in its order)
// It replaces the host draw and its copy, avr_raymarch, four torch arithmetic kernels, avr_sample_coarse_rays
// and torch.sort of the one-scene chain.
//
// One ray per 16 lanes as in the march. Lane k of a ray holds band samples 4k .. 4k + 3 (one Philox block, one
// 16-B noise read), so nothing is indexed at run time and nothing lives in scratch. The sort runs the wave's 4
// rays one after another through wave_sort64 (wave_sort.h): lane l takes sample l of the ray from lane
// 16 q + l / 4 by four shuffles, lanes past n_band hold +inf, and lane l < n_band stores rank l: coalesced
// stores of whole rows.
#include <math.h>

#include "lstm_march.h"
#include "wave_sort.h"

namespace avr {

constexpr int kFrontBand = 64;   // band samples per ray at most: 4 per lane of the ray's 16

__global__ void __launch_bounds__(256) adaptive_front_kernel(
    MarchScenes sc, const float* __restrict__ tables, int64_t table_stride, const float* __restrict__ w_hh,
    const float* __restrict__ b_ih, const float* __restrict__ b_hh, const float* __restrict__ w_out,
    const float* __restrict__ b_out, const float* __restrict__ ro, const float* __restrict__ rd,
    const float* __restrict__ init_dist, const float* __restrict__ band_noise, uint64_t seed, uint64_t offset,
    const int64_t* __restrict__ ray_ids, int64_t n_per_scene, int64_t n_rays, int steps, float eps, int n_band,
    float* __restrict__ world, float* __restrict__ z_sorted, float* __restrict__ init_out,
    float* __restrict__ noise_out) {
  const int k = threadIdx.x & (kHid - 1);
  const int lane = threadIdx.x & 63;
  const int64_t ray_raw = (int64_t)blockIdx.x * (blockDim.x / kHid) + threadIdx.x / kHid;
  const bool live = ray_raw < n_rays;
  const int64_t ray = live ? ray_raw : n_rays - 1;   // keep the 16-lane group and the wave whole
  const int scene = (int)(ray / n_per_scene);
  const View& v = sc.v[scene];
  const float* table = tables + scene * table_stride;
  const MarchLane L = march_lane(w_hh, b_ih, b_hh, w_out, b_out, k);
  const float r0 = ro[3 * ray], r1 = ro[3 * ray + 1], r2 = ro[3 * ray + 2];
  const float e0 = rd[3 * ray], e1 = rd[3 * ray + 1], e2 = rd[3 * ray + 2];
  const uint64_t key = offset + (uint64_t)(ray_ids ? ray_ids[ray] : ray);   // Philox counter of this ray
  const float dist0 =
      init_dist ? init_dist[ray] : fadd(0.8f, fmul(0.05f, philox_normal(seed, key, 0, kStreamMarch)));
  if (init_out && live && k == 0) init_out[ray] = dist0;
  float x0 = fadd(r0, fmul(e0, dist0)), x1 = fadd(r1, fmul(e1, dist0)), x2 = fadd(r2, fmul(e2, dist0));
  float h = 0.f, c = 0.f;
  for (int s = 0; s < steps; ++s) {
    MarchGateValues gates;
    const float sd = march_step(v, table, L, x0, x1, x2, h, c, gates);
    x0 = fadd(x0, fmul(e0, sd));   // world_coords + rds * signed_distance (renderers.py:341, :432)
    x1 = fadd(x1, fmul(e1, sd));
    x2 = fadd(x2, fmul(e2, sd));
  }
  if (live && k < 3) world[3 * ray + k] = k == 0 ? x0 : (k == 1 ? x1 : x2);
  if (n_band <= 0) return;   // Raymarcher: no band (uniform: the whole grid leaves)

  // the band's z, samples 4k .. 4k + 3 of this ray (renderers.py:490-493, sample_coarse :10-14)
  const float d = fdiv(fsub(x0, r0), e0);
  const float near_ = fsub(d, eps), far_ = fadd(d, eps), span = fsub(far_, near_);
  const float fn = (float)n_band;
  float u[4];
  if (band_noise) {
    const float* nr = band_noise + ray * n_band + 4 * k;
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = 4 * k + j < n_band ? nr[j] : 0.f;
  } else {
    const float4 q = philox_uniform4(seed, key, (uint32_t)k, kStreamBand);
    u[0] = q.x; u[1] = q.y; u[2] = q.z; u[3] = q.w;
  }
  float zv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = 4 * k + j;
    zv[j] = fadd(fadd(near_, fmul(span, fdiv((float)i, fn))), fdiv(fmul(u[j], span), fn));
    if (noise_out && live && i < n_band) noise_out[ray * n_band + i] = u[j];
  }
  // sort: the wave's 4 rays in turn, one value per lane
  const int64_t wave_ray0 = (int64_t)blockIdx.x * (blockDim.x / kHid) + (threadIdx.x >> 6) * 4;
  const int part = lane & 3;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int src = 16 * q + (lane >> 2);
    const float t0 = __shfl(zv[0], src), t1 = __shfl(zv[1], src), t2 = __shfl(zv[2], src), t3 = __shfl(zv[3], src);
    const float mine = part == 0 ? t0 : (part == 1 ? t1 : (part == 2 ? t2 : t3));   // sample `lane` of ray q
    const bool in_band = lane < n_band;
    // d = +-inf or NaN (rd_x = 0) makes span, and so every z of the row, NaN: the row is stored as it is
    const bool nan_row = __any(in_band && mine != mine);
    const float sorted = wave_sort64(in_band ? mine : INFINITY, lane);
    const int64_t rq = wave_ray0 + q;
    if (in_band && rq < n_rays) z_sorted[rq * n_band + lane] = nan_row ? mine : sorted;
  }
}

}  // namespace avr

using namespace avr;

extern "C" int avr_adaptive_front(const avr_view_desc* views, int n_scenes, const float* gate_tables,
                                  const float* w_hh, const float* b_ih, const float* b_hh, const float* w_out,
                                  const float* b_out, const float* ro, const float* rd, const float* init_dist,
                                  const float* band_noise, uint64_t seed, uint64_t offset, const int64_t* ray_ids,
                                  int64_t n_per_scene, int steps, float eps, int n_band, float* world,
                                  float* z_sorted, float* init_out, float* noise_out, void* stream) {
  AVR_REQUIRE(n_scenes >= 1 && n_scenes <= AVR_MAX_SCENES, "avr_adaptive_front: n_scenes %d outside 1..%d", n_scenes,
              AVR_MAX_SCENES);
  AVR_REQUIRE(n_band >= 0 && n_band <= kFrontBand, "avr_adaptive_front: n_band %d outside 0..%d", n_band,
              kFrontBand);
  AVR_REQUIRE(steps >= 0, "avr_adaptive_front: negative steps");
  AVR_REQUIRE(n_per_scene >= 0, "avr_adaptive_front: negative n_per_scene");
  if (n_per_scene == 0) return AVR_OK;
  AVR_REQUIRE(views && gate_tables && w_hh && b_ih && b_hh && w_out && b_out && ro && rd && world,
              "avr_adaptive_front: null pointer");
  AVR_REQUIRE(n_band == 0 || z_sorted, "avr_adaptive_front: null z_sorted with n_band > 0");
  MarchScenes sc;
  int rc = march_scenes(views, n_scenes, &sc, "avr_adaptive_front");
  if (rc) return rc;
  const int64_t n = n_per_scene * n_scenes;
  const int64_t stride = (int64_t)views[0].latent_h * views[0].latent_w * kGates;
  const int per_block = 256 / kHid;
  const int64_t blocks = (n + per_block - 1) / per_block;
  AVR_REQUIRE(blocks < (1ll << 31), "avr_adaptive_front: too many rays");
  adaptive_front_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(
      sc, gate_tables, stride, w_hh, b_ih, b_hh, w_out, b_out, ro, rd, init_dist, band_noise, seed, offset, ray_ids,
      n_per_scene, n, steps, eps, n_band, world, z_sorted, init_out, noise_out);
  return check_launch("adaptive_front_kernel");
}
