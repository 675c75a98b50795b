// Pixel-aligned latent features at points: SpatialEncoder.index
// (models.py:245-274: project into the source view, uv * scale - 1, grid_sample
// bilinear / border / align_corners=True) as NewPixelNeRFNet.forward calls it
// (models.py:753-810) — the `latent` half of the MLP input, which the lin_z
// weight gradients contract against, and phi(..., return_features=True).
//
// The map is read channels-last, (H*W, C): one wave per point, each lane
// blends 8 channels of the 4 corner rows (2 x 16-B loads per corner, the rows
// of neighbouring points mostly L2 hits) and writes them with two 16-B stores,
// so a point costs one 2 KB row out (C = 512) and the output is row-major
// (n_points, C) with no transpose pass.
#include "field_common.h"

namespace avr {

// Scenes of a batch: blockIdx.y = scene s, its view, map lat_hwc + s * lat_stride, points xyz + 3 s n_points,
// rows out + s * n_points * C. The rows stream out non-temporally (they are read once, by the weight-gradient
// kernel, after every other kernel of the backward).
struct LatBatch {
  View v[AVR_MAX_SCENES];
};

__global__ void __launch_bounds__(256) latent_features_kernel(LatBatch vb, const float* __restrict__ lat_hwc,
                                                              int64_t lat_stride, int C, const float* __restrict__ xyz,
                                                              int64_t n_points, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= n_points) return;
  const int s = blockIdx.y;
  lat_hwc += s * lat_stride;
  xyz += 3 * s * n_points;
  out += s * n_points * C;
  const Bilinear bl = bilinear_at(vb.v[s], xyz[3 * m], xyz[3 * m + 1], xyz[3 * m + 2]);
  // two 256-channel groups per pass, both gathered before either is stored (a load behind a store waits for it)
  for (int c0 = 4 * lane; c0 < C; c0 += 512) {
    floatx4 acc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int c = c0 + 256 * u;
      if (c < C) {
        const floatx4 a = *reinterpret_cast<const floatx4*>(lat_hwc + (int64_t)bl.tex[0] * C + c);
        const floatx4 b = *reinterpret_cast<const floatx4*>(lat_hwc + (int64_t)bl.tex[1] * C + c);
        const floatx4 d = *reinterpret_cast<const floatx4*>(lat_hwc + (int64_t)bl.tex[2] * C + c);
        const floatx4 e = *reinterpret_cast<const floatx4*>(lat_hwc + (int64_t)bl.tex[3] * C + c);
        // grid_sample's order: nw, ne, sw, se
#pragma unroll
        for (int t = 0; t < 4; ++t)
          acc[u][t] = fadd(fadd(fadd(fmul(a[t], bl.w[0]), fmul(b[t], bl.w[1])), fmul(d[t], bl.w[2])), fmul(e[t], bl.w[3]));
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (c0 + 256 * u < C) __builtin_nontemporal_store(acc[u], reinterpret_cast<floatx4*>(out + m * C + c0 + 256 * u));
  }
}

}  // namespace avr

using namespace avr;

extern "C" int avr_latent_features(const avr_view_desc* view, const float* latent_hwc, int channels,
                                   const float* xyz, int64_t n_points, float* out, void* stream) {
  AVR_REQUIRE(n_points >= 0 && channels > 0 && channels % 4 == 0, "avr_latent_features: bad sizes");
  if (n_points == 0) return AVR_OK;
  AVR_REQUIRE(view && latent_hwc && xyz && out, "avr_latent_features: null pointer");
  AVR_REQUIRE(view->latent_h > 0 && view->latent_w > 0, "avr_latent_features: bad latent size");
  LatBatch vb;
  view_from_desc(view, &vb.v[0]);
  latent_features_kernel<<<dim3((unsigned)((n_points + 3) / 4), 1), 256, 0, as_stream(stream)>>>(
      vb, latent_hwc, 0, channels, xyz, n_points, out);
  return check_launch("latent_features_kernel");
}

extern "C" int avr_latent_features_batch(const avr_view_desc* views, int n_scenes, const float* latent_hwc,
                                         int channels, const float* xyz, int64_t n_points, float* out,
                                         void* stream) {
  AVR_REQUIRE(n_scenes >= 1 && n_scenes <= AVR_MAX_SCENES, "avr_latent_features_batch: 1..%d scenes per call",
              AVR_MAX_SCENES);
  AVR_REQUIRE(n_points >= 0 && channels > 0 && channels % 4 == 0, "avr_latent_features_batch: bad sizes");
  if (n_points == 0) return AVR_OK;
  AVR_REQUIRE(views && latent_hwc && xyz && out, "avr_latent_features_batch: null pointer");
  LatBatch vb;
  for (int s = 0; s < n_scenes; ++s) {
    AVR_REQUIRE(views[s].latent_h == views[0].latent_h && views[s].latent_w == views[0].latent_w &&
                    views[s].latent_h > 0 && views[s].latent_w > 0,
                "avr_latent_features_batch: scenes need latent maps of one (positive) size");
    view_from_desc(&views[s], &vb.v[s]);
  }
  const int64_t stride = (int64_t)views[0].latent_h * views[0].latent_w * channels;
  latent_features_kernel<<<dim3((unsigned)((n_points + 3) / 4), (unsigned)n_scenes), 256, 0, as_stream(stream)>>>(
      vb, latent_hwc, stride, channels, xyz, n_points, out);
  return check_launch("latent_features_kernel");
}

// ---- d loss / d xyz through the lookup (the adaptive renderer's band points carry a gradient): torch's
// grid_sample grid gradient (bilinear, border padding, align_corners=True: a clipped coordinate passes none)
// chained through grid = uv * scale - 1, uv = (-xc_xy / xc_z) * focal + c, xc = R x + t (models.py:753-810,
// :260-273). One wave per point: lane l sums channels 4l, 4l + 256, ... of
//   gix = sum_c g_c ((ne - nw) wy0 + (se - sw) wy1),  giy = sum_c g_c ((sw - nw) wx0 + (se - ne) wx1)
// over the corner rows of latent_hwc (H*W, C) and the feature gradient row g (C), then lane 0 applies the
// chain. The corners and weights are the forward's (bilinear_from_rot's operations); a corner past the edge
// only occurs with a zero weight or a clipped (zero-gradient) coordinate, so its clamped texel changes nothing.
namespace avr {

__device__ __forceinline__ float lane_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// The summed rows: term t contributes sum_c g_t[c] (corner differences of map_t)[c], map_t (H*W, C) of scene s at
// map[t] + s * map_scene_stride, g_t the point's row at g[t] + row * ldg[t]. One term (the looked-up latent and
// its feature gradient: avr_latent_features_grad_points) or one per linear layer fed by the lookup with that
// layer's per-texel table and output gradient (avr_latent_tables_grad_points).
struct GradTerms {
  const float* map[AVR_LOOKUP_GRAD_TERMS];
  const float* g[AVR_LOOKUP_GRAD_TERMS];
  int64_t ldg[AVR_LOOKUP_GRAD_TERMS];
  int64_t map_scene_stride;
  int n;
};

__global__ void __launch_bounds__(256) latent_features_grad_points_kernel(LatBatch vb, GradTerms T, int C,
                                                                          const float* __restrict__ xyz,
                                                                          int64_t n_points,
                                                                          float* __restrict__ gxyz) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= n_points) return;
  const int s = blockIdx.y;
  const View& v = vb.v[s];
  const int64_t row = s * n_points + m;
  const float x0 = xyz[3 * row], x1 = xyz[3 * row + 1], x2 = xyz[3 * row + 2];
  const float xr[3] = {dot3(v.R + 0, x0, x1, x2), dot3(v.R + 3, x0, x1, x2), dot3(v.R + 6, x0, x1, x2)};
  const Bilinear bl = bilinear_from_rot(v, xr);
  // the forward's coordinates again, for the weights and the clip masks
  const float xc0 = fadd(xr[0], v.t[0]), xc1 = fadd(xr[1], v.t[1]), xc2 = fadd(xr[2], v.t[2]);
  const float u = fadd(fmul(fdiv(-xc0, xc2), v.focal[0]), v.c[0]);
  const float w = fadd(fmul(fdiv(-xc1, xc2), v.focal[1]), v.c[1]);
  const float gx = fsub(fmul(u, v.scale[0]), 1.0f), gy = fsub(fmul(w, v.scale[1]), 1.0f);
  const float ixr = fmul(fdiv(fadd(gx, 1.0f), 2.0f), (float)(v.W - 1));
  const float iyr = fmul(fdiv(fadd(gy, 1.0f), 2.0f), (float)(v.H - 1));
  const float ix = fminf(fmaxf(ixr, 0.f), (float)(v.W - 1)), iy = fminf(fmaxf(iyr, 0.f), (float)(v.H - 1));
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const float wx1 = fsub(ix, fx0), wy1 = fsub(iy, fy0);
  const float wx0 = fsub(fadd(fx0, 1.0f), ix), wy0 = fsub(fadd(fy0, 1.0f), iy);
  float sx = 0.f, sy = 0.f;
  for (int t = 0; t < T.n; ++t) {
    const float* lat_hwc = T.map[t] + s * T.map_scene_stride;
    const float* g = T.g[t] + row * T.ldg[t];
    for (int c = 4 * lane; c < C; c += 256) {
      const floatx4 gv = *reinterpret_cast<const floatx4*>(g + c);
      const floatx4 nw = *reinterpret_cast<const floatx4*>(lat_hwc + (int64_t)bl.tex[0] * C + c);
      const floatx4 ne = *reinterpret_cast<const floatx4*>(lat_hwc + (int64_t)bl.tex[1] * C + c);
      const floatx4 sw = *reinterpret_cast<const floatx4*>(lat_hwc + (int64_t)bl.tex[2] * C + c);
      const floatx4 se = *reinterpret_cast<const floatx4*>(lat_hwc + (int64_t)bl.tex[3] * C + c);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        sx += gv[q] * ((ne[q] - nw[q]) * wy0 + (se[q] - sw[q]) * wy1);
        sy += gv[q] * ((sw[q] - nw[q]) * wx0 + (se[q] - ne[q]) * wx1);
      }
    }
  }
  sx = lane_sum(sx);
  sy = lane_sum(sy);
  if (lane == 0) {
    // d grid -> d uv (the clip passes no gradient at or past either edge) -> d xc -> d x = R^T d xc
    const float mxk = ixr > 0.f && ixr < (float)(v.W - 1) ? 1.f : 0.f;
    const float myk = iyr > 0.f && iyr < (float)(v.H - 1) ? 1.f : 0.f;
    const float gu = sx * (0.5f * (float)(v.W - 1)) * mxk * v.scale[0];
    const float gw = sy * (0.5f * (float)(v.H - 1)) * myk * v.scale[1];
    const float a0 = gu * v.focal[0], a1 = gw * v.focal[1];
    const float inv_z = 1.0f / xc2;
    // a clipped coordinate passes exactly zero: at a point on the source camera's plane (xc2 = 0: the lookup
    // is clipped, 1 / xc2 = inf) the chain would otherwise give 0 * inf = NaN (torch's autograd does: the
    // r04q adaptive train step hit a band point at world z = -1.3f, camera z 0, profiles/r05d_*)
    const float num = a0 * xc0 + a1 * xc1;
    const float d0 = a0 != 0.f ? -a0 * inv_z : 0.f, d1 = a1 != 0.f ? -a1 * inv_z : 0.f;
    const float d2 = num != 0.f ? num * inv_z * inv_z : 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) gxyz[3 * row + j] = v.R[j] * d0 + v.R[3 + j] * d1 + v.R[6 + j] * d2;
  }
}

// z_feature's position adjoint for the fused family (models.py:753-794 with PositionalEncoding :41-87): z = R x
// (normalize_z), zf = [z, sin(f_k z + 0), sin(f_k z + pi/2) for k < F (3 each), R d]; given g = d loss / d zf's
// first 3 + 6F columns, d z_c = g_c + sum_j f_j cos(phase_j + f_j z_c) g[3 + 3j + c] (j < 2F, f_j = f_(j/2) =
// freq_factor 2^(j/2)) and d x = R^T d z -- torch autograd's chain (sin', addcmul', bmm') in one thread per point.
__global__ void __launch_bounds__(256) zfeature_grad_points_kernel(LatBatch vb, const float* __restrict__ xyz,
                                                                   int64_t n_points, const float* __restrict__ g,
                                                                   int64_t ldg, int F, float freq_factor,
                                                                   int accumulate, float* __restrict__ gxyz) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= n_points) return;
  const int s = blockIdx.y;
  const View& v = vb.v[s];
  const int64_t row = s * n_points + m;
  const float x0 = xyz[3 * row], x1 = xyz[3 * row + 1], x2 = xyz[3 * row + 2];
  const float z[3] = {dot3(v.R + 0, x0, x1, x2), dot3(v.R + 3, x0, x1, x2), dot3(v.R + 6, x0, x1, x2)};
  const float* gr = g + row * ldg;
  float dz[3] = {gr[0], gr[1], gr[2]};
  constexpr float kHalfPi = 1.57079632679489662f;
  for (int j = 0; j < 2 * F; ++j) {
    const float f = ldexpf(freq_factor, j >> 1);   // freq_factor * 2^k exactly (models.py:45, fp32)
    const float ph = (j & 1) ? kHalfPi : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) dz[c] += gr[3 + 3 * j + c] * cosf(ph + z[c] * f) * f;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float d = v.R[k] * dz[0] + v.R[3 + k] * dz[1] + v.R[6 + k] * dz[2];
    gxyz[3 * row + k] = accumulate ? gxyz[3 * row + k] + d : d;
  }
}

}  // namespace avr

static int lookup_views(const avr_view_desc* views, int n_scenes, LatBatch* vb, const char* what) {
  AVR_REQUIRE(n_scenes >= 1 && n_scenes <= AVR_MAX_SCENES, "%s: 1..%d scenes per call", what, AVR_MAX_SCENES);
  for (int s = 0; s < n_scenes; ++s) {
    AVR_REQUIRE(views[s].latent_h == views[0].latent_h && views[s].latent_w == views[0].latent_w &&
                    views[s].latent_h > 0 && views[s].latent_w > 0,
                "%s: scenes need latent maps of one (positive) size", what);
    view_from_desc(&views[s], &vb->v[s]);
  }
  return AVR_OK;
}

extern "C" int avr_latent_features_grad_points(const avr_view_desc* views, int n_scenes, const float* latent_hwc,
                                               int channels, const float* xyz, int64_t n_points,
                                               const float* grad_features, float* grad_xyz, void* stream) {
  AVR_REQUIRE(n_scenes >= 1 && n_scenes <= AVR_MAX_SCENES,
              "avr_latent_features_grad_points: 1..%d scenes per call", AVR_MAX_SCENES);
  AVR_REQUIRE(n_points >= 0 && channels > 0 && channels % 4 == 0, "avr_latent_features_grad_points: bad sizes");
  if (n_points == 0) return AVR_OK;
  AVR_REQUIRE(views && latent_hwc && xyz && grad_features && grad_xyz, "avr_latent_features_grad_points: null pointer");
  LatBatch vb;
  int rc = lookup_views(views, n_scenes, &vb, "avr_latent_features_grad_points");
  if (rc) return rc;
  GradTerms T{};
  T.n = 1;
  T.map[0] = latent_hwc;
  T.g[0] = grad_features;
  T.ldg[0] = channels;
  T.map_scene_stride = (int64_t)views[0].latent_h * views[0].latent_w * channels;
  latent_features_grad_points_kernel<<<dim3((unsigned)((n_points + 3) / 4), (unsigned)n_scenes), 256, 0,
                                       as_stream(stream)>>>(vb, T, channels, xyz, n_points, grad_xyz);
  return check_launch("latent_features_grad_points_kernel");
}

extern "C" int avr_latent_tables_grad_points(const avr_view_desc* views, int n_scenes, const float* tables,
                                             int64_t table_scene_stride, int64_t table_stride, int n_tables,
                                             int channels, const float* xyz, int64_t n_points,
                                             const float* const* grads, int64_t ld_grad, float* grad_xyz,
                                             void* stream) {
  AVR_REQUIRE(n_points >= 0 && channels > 0 && channels % 4 == 0 && ld_grad >= channels && ld_grad % 4 == 0 &&
                  n_tables >= 1 && n_tables <= AVR_LOOKUP_GRAD_TERMS && table_stride >= 0 && table_scene_stride >= 0,
              "avr_latent_tables_grad_points: bad sizes");
  if (n_points == 0) return AVR_OK;
  AVR_REQUIRE(views && tables && xyz && grads && grad_xyz, "avr_latent_tables_grad_points: null pointer");
  LatBatch vb;
  int rc = lookup_views(views, n_scenes, &vb, "avr_latent_tables_grad_points");
  if (rc) return rc;
  const int64_t hw = (int64_t)views[0].latent_h * views[0].latent_w;
  AVR_REQUIRE((table_stride >= hw * channels || n_tables == 1) && (table_scene_stride >= n_tables * hw * channels ||
                                                                    n_scenes == 1),
              "avr_latent_tables_grad_points: overlapping tables");
  GradTerms T{};
  T.n = n_tables;
  T.map_scene_stride = table_scene_stride;
  for (int t = 0; t < n_tables; ++t) {
    AVR_REQUIRE(grads[t], "avr_latent_tables_grad_points: null gradient rows %d", t);
    T.map[t] = tables + t * table_stride;
    T.g[t] = grads[t];
    T.ldg[t] = ld_grad;
  }
  latent_features_grad_points_kernel<<<dim3((unsigned)((n_points + 3) / 4), (unsigned)n_scenes), 256, 0,
                                       as_stream(stream)>>>(vb, T, channels, xyz, n_points, grad_xyz);
  return check_launch("latent_features_grad_points_kernel");
}

extern "C" int avr_zfeature_grad_points(const avr_view_desc* views, int n_scenes, const float* xyz, int64_t n_points,
                                        const float* grad_zf, int64_t ld_grad, int num_freqs, float freq_factor,
                                        int accumulate, float* grad_xyz, void* stream) {
  AVR_REQUIRE(n_scenes >= 1 && n_scenes <= AVR_MAX_SCENES, "avr_zfeature_grad_points: 1..%d scenes per call",
              AVR_MAX_SCENES);
  AVR_REQUIRE(n_points >= 0 && num_freqs >= 0 && num_freqs <= 32 && ld_grad >= 3 + 6 * num_freqs,
              "avr_zfeature_grad_points: bad sizes");
  if (n_points == 0) return AVR_OK;
  AVR_REQUIRE(views && xyz && grad_zf && grad_xyz, "avr_zfeature_grad_points: null pointer");
  LatBatch vb;
  for (int s = 0; s < n_scenes; ++s) view_from_desc(&views[s], &vb.v[s]);   // only R is read
  avr::zfeature_grad_points_kernel<<<dim3((unsigned)((n_points + 255) / 256), (unsigned)n_scenes), 256, 0,
                                     as_stream(stream)>>>(vb, xyz, n_points, grad_zf, ld_grad, num_freqs, freq_factor,
                                                          accumulate ? 1 : 0, grad_xyz);
  return check_launch("zfeature_grad_points_kernel");
}

// ---- d loss / d latent map: the lookup's adjoint onto the maps (torch's grid_sample input gradient: bilinear,
// border padding, align_corners=True), channels-last, with no float atomics and a sum order that depends on the
// inputs alone. An inverted index and a per-destination sum:
//   1. rank     one wave per kAdjBlockPoints consecutive points of a scene, 64 at a time in point order: the
//               point's key is its nw texel (bilinear_at's tex[0]); lanes of one key take consecutive ranks from
//               the (scene, block, texel) counter. Only this wave touches that counter row, batch after batch, so
//               the integer atomicAdd (used for its coherent read-modify-write) leaves a rank that is the number
//               of earlier points of the block in the same texel.
//   2. columns  per (scene, texel): exclusive prefix of the counters over the blocks, and the texel's count.
//   3. offsets  one workgroup: exclusive scans over the texels of the counts (list starts), of every
//               destination's chunk count and of its partial-row count (destinations of more than one chunk).
//   4. place    order[start + block prefix + rank] = point: each texel's list in ascending point index.
//   5. gather   one wave per (destination texel, chunk of kAdjChunk rows): walks the lists of cells (y, x),
//               (y, x-1), (y-1, x), (y-1, x-1), recomputes each point's Bilinear and adds w_k * grad row for the
//               corners k whose texel is the destination; 4 channels per lane per 256-channel group, fp32. A
//               destination of one chunk writes its row of the map, the others a partial row in scratch.
//   6. reduce   adds a chunked destination's partial rows in chunk order.
namespace avr {

constexpr int kAdjChunk = AVR_LATENT_ADJOINT_CHUNK;
constexpr int kAdjBlockPoints = 1024;
constexpr int kAdjScanThreads = 1024;

__device__ __forceinline__ int adj_key(const View& v, const float* __restrict__ p) {
  const int t = bilinear_at(v, p[0], p[1], p[2]).tex[0];
  const int last = v.H * v.W - 1;
  return t < 0 ? 0 : (t > last ? last : t);   // the forward's texel always lies inside: this only guards the stores
}

__global__ void __launch_bounds__(64) latent_adjoint_rank_kernel(LatBatch vb, const float* __restrict__ xyz,
                                                                 int64_t n_points, int n_blocks,
                                                                 int* __restrict__ table, int* __restrict__ keys,
                                                                 int* __restrict__ ranks) {
  const int lane = threadIdx.x;
  const int s = blockIdx.y, b = blockIdx.x;
  const View& v = vb.v[s];
  const int hw = v.H * v.W;
  int* T = table + ((int64_t)s * n_blocks + b) * hw;
  const int64_t m0 = (int64_t)b * kAdjBlockPoints;
  const int64_t m1 = m0 + kAdjBlockPoints < n_points ? m0 + kAdjBlockPoints : n_points;
  for (int64_t base = m0; base < m1; base += 64) {
    const int64_t m = base + lane;
    const bool act = m < m1;
    const int64_t row = s * n_points + m;
    const int key = act ? adj_key(v, xyz + 3 * row) : -1;
    // the lanes of one key: their first lane (the leader), their number, each lane's place among them
    int leader = lane, members = 0, place = 0;
    uint64_t todo = __ballot(act);
    while (todo) {
      const int first = __ffsll((unsigned long long)todo) - 1;
      const int k = __shfl(key, first, 64);
      const uint64_t grp = __ballot(act && key == k);
      if (act && key == k) {
        leader = first;
        members = __popcll(grp);
        place = __popcll(grp & ((1ull << lane) - 1ull));
      }
      todo &= ~grp;
    }
    // one round trip per batch: every leader advances its key's counter (distinct addresses) and hands the old
    // value to its lanes
    int off = 0;
    if (act && lane == leader) off = atomicAdd(&T[key], members);
    off = __shfl(off, leader, 64);
    if (act) {
      keys[row] = key;
      ranks[row] = off + place;
    }
  }
}

__global__ void __launch_bounds__(256) latent_adjoint_columns_kernel(int n_texels, int hw, int n_blocks,
                                                                     int* __restrict__ table,
                                                                     int* __restrict__ count) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= n_texels) return;
  const int s = gid / hw, t = gid - s * hw;
  int* col = table + (int64_t)s * n_blocks * hw + t;
  int run = 0;
  for (int b = 0; b < n_blocks; ++b) {
    const int c = col[(int64_t)b * hw];
    col[(int64_t)b * hw] = run;
    run += c;
  }
  count[gid] = run;
}

// rows of destination gid's walk: the lists of its own cell and of the cells left, above and above-left of it
__device__ __forceinline__ int adj_walk_rows(const int* __restrict__ count, int gid, int hw, int W) {
  const int t = gid % hw, y = t / W, x = t - y * W;
  int n = count[gid];
  if (x > 0) n += count[gid - 1];
  if (y > 0) n += count[gid - W];
  if (x > 0 && y > 0) n += count[gid - W - 1];
  return n;
}

__device__ __forceinline__ int adj_chunks(int rows) { return rows <= kAdjChunk ? 1 : (rows + kAdjChunk - 1) / kAdjChunk; }

// start / chunk0 / pchunk0: n_texels + 1 entries each (the last one the total)
__global__ void __launch_bounds__(kAdjScanThreads) latent_adjoint_offsets_kernel(int n_texels, int hw, int W,
                                                                                 const int* __restrict__ count,
                                                                                 int* __restrict__ start,
                                                                                 int* __restrict__ chunk0,
                                                                                 int* __restrict__ pchunk0) {
  __shared__ int wave_sums[3][kAdjScanThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int carry[3] = {0, 0, 0};
  // 1024 texels per pass (coalesced reads): a shuffle scan per wave, the waves' totals through LDS, a running carry
  for (int tile = 0; tile < n_texels; tile += kAdjScanThreads) {
    const int g = tile + tid;
    int v[3] = {0, 0, 0};
    if (g < n_texels) {
      const int nc = adj_chunks(adj_walk_rows(count, g, hw, W));
      v[0] = count[g];
      v[1] = nc;
      v[2] = nc > 1 ? nc : 0;
    }
    int inc[3] = {v[0], v[1], v[2]};
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int o = __shfl_up(inc[k], d, 64);
        if (lane >= d) inc[k] += o;
      }
    }
    if (lane == 63) {
#pragma unroll
      for (int k = 0; k < 3; ++k) wave_sums[k][wid] = inc[k];
    }
    __syncthreads();
    int before[3] = {0, 0, 0}, total[3] = {0, 0, 0};
    for (int w = 0; w < kAdjScanThreads / 64; ++w) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int t = wave_sums[k][w];
        before[k] += w < wid ? t : 0;
        total[k] += t;
      }
    }
    if (g < n_texels) {
      start[g] = carry[0] + before[0] + inc[0] - v[0];
      chunk0[g] = carry[1] + before[1] + inc[1] - v[1];
      pchunk0[g] = carry[2] + before[2] + inc[2] - v[2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) carry[k] += total[k];
    __syncthreads();
  }
  if (tid == 0) { start[n_texels] = carry[0]; chunk0[n_texels] = carry[1]; pchunk0[n_texels] = carry[2]; }
}

__global__ void __launch_bounds__(256) latent_adjoint_place_kernel(int64_t n_rows, int64_t n_points, int hw,
                                                                   int n_blocks, const int* __restrict__ keys,
                                                                   const int* __restrict__ ranks,
                                                                   const int* __restrict__ table,
                                                                   const int* __restrict__ start,
                                                                   int* __restrict__ order) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n_rows) return;
  const int64_t s = row / n_points, m = row - s * n_points;
  const int key = keys[row];
  const int64_t b = m / kAdjBlockPoints;
  const int64_t pos = (int64_t)start[s * hw + key] + table[(s * n_blocks + b) * hw + key] + ranks[row];
  if (pos >= 0 && pos < n_rows) order[pos] = (int)m;
}

__global__ void __launch_bounds__(256) latent_adjoint_gather_kernel(LatBatch vb, const float* __restrict__ xyz,
                                                                    int64_t n_points, const float* __restrict__ grad,
                                                                    int64_t ldg, int C, int n_texels,
                                                                    const int* __restrict__ count,
                                                                    const int* __restrict__ start,
                                                                    const int* __restrict__ chunk0,
                                                                    const int* __restrict__ pchunk0,
                                                                    const int* __restrict__ order,
                                                                    int64_t max_partials, float* __restrict__ partial,
                                                                    float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (w >= chunk0[n_texels]) return;
  // the destination: the last texel whose first chunk is at or before w (every texel has at least one chunk)
  int lo = 0, hi = n_texels - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (chunk0[mid] <= w) lo = mid; else hi = mid - 1;
  }
  const int gid = __builtin_amdgcn_readfirstlane(lo);
  const int j = w - chunk0[gid], n_chunks = chunk0[gid + 1] - chunk0[gid];
  const int W = vb.v[0].W, hw = vb.v[0].H * W;
  const int s = gid / hw, t = gid - s * hw, y = t / W, x = t - y * W;
  const View& v = vb.v[s];
  float* dst;
  if (n_chunks == 1) {
    dst = out + (int64_t)gid * C;
  } else {
    const int64_t p = (int64_t)pchunk0[gid] + j;
    if (p >= max_partials) return;   // cannot happen (the bound is proved at the scratch layout): guards the store
    dst = partial + p * C;
  }
  const int r0 = j * kAdjChunk, r1 = r0 + kAdjChunk;   // this wave's rows of the destination's walk
  xyz += 3 * (int64_t)s * n_points;
  grad += (int64_t)s * n_points * ldg;
  // the walk: the lists of the four cells one after the other, cell q's rows at [vend[q], vend[q + 1]) of it
  int cstart[4], vend[5];
  vend[0] = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int dx = q & 1, dy = q >> 1;
    const bool there = x - dx >= 0 && y - dy >= 0;
    const int cell = there ? gid - dy * W - dx : gid;
    cstart[q] = __builtin_amdgcn_readfirstlane(start[cell]);
    vend[q + 1] = vend[q] + (there ? __builtin_amdgcn_readfirstlane(count[cell]) : 0);
  }
  const int e = r1 < vend[4] ? r1 : vend[4];
  for (int cb = 0; cb < C; cb += 1024) {
    floatx4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = floatx4{0.f, 0.f, 0.f, 0.f};
    for (int i = r0; i < e; i += 64) {
      const int nb = e - i < 64 ? e - i : 64;
      // lane l: row i + l of the walk -- its point and the weight it gives this texel (0 and point 0 past nb)
      int m = 0;
      float wt = 0.f;
      if (lane < nb) {
        const int vi = i + lane;
        const int pos = vi < vend[1] ? cstart[0] + vi
                                     : (vi < vend[2] ? cstart[1] + vi - vend[1]
                                                     : (vi < vend[3] ? cstart[2] + vi - vend[2] : cstart[3] + vi - vend[3]));
        m = order[pos];
        m = m < 0 ? 0 : (m < n_points ? m : (int)n_points - 1);   // a point index by construction: guards the reads
        const Bilinear bl = bilinear_at(v, xyz[3 * (int64_t)m], xyz[3 * (int64_t)m + 1], xyz[3 * (int64_t)m + 2]);
        // a corner clamped onto its neighbour carries an exact zero weight, so this sum is the one live weight
#pragma unroll
        for (int k = 0; k < 4; ++k) wt += bl.tex[k] == t ? bl.w[k] : 0.f;
      }
      // four rows' loads in flight before their sums (a row past nb reads point 0's row and is not added)
      for (int r = 0; r < nb; r += 4) {
        floatx4 gv[4][4];
        float wr[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int mr = __builtin_amdgcn_readlane(m, r + k);
          wr[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wt), r + k));
          const float* g = grad + (int64_t)mr * ldg + cb + 4 * lane;
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (cb + 4 * lane + 256 * u < C) gv[k][u] = *reinterpret_cast<const floatx4*>(g + 256 * u);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (r + k < nb) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              if (cb + 4 * lane + 256 * u < C) {
#pragma unroll
                for (int z = 0; z < 4; ++z) acc[u][z] = __builtin_fmaf(wr[k], gv[k][u][z], acc[u][z]);
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = cb + 4 * lane + 256 * u;
      if (c < C) *reinterpret_cast<floatx4*>(dst + c) = acc[u];
    }
  }
}

__global__ void __launch_bounds__(256) latent_adjoint_reduce_kernel(int C, int n_texels,
                                                                    const int* __restrict__ chunk0,
                                                                    const int* __restrict__ pchunk0,
                                                                    int64_t max_partials,
                                                                    const float* __restrict__ partial,
                                                                    float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int gid = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gid >= n_texels) return;
  const int n_chunks = chunk0[gid + 1] - chunk0[gid];
  if (n_chunks <= 1) return;
  const int64_t p0 = pchunk0[gid];
  if (p0 + n_chunks > max_partials) return;
  for (int c = 4 * lane; c < C; c += 256) {
    floatx4 acc = *reinterpret_cast<const floatx4*>(partial + p0 * C + c);
    for (int j = 1; j < n_chunks; ++j) acc += *reinterpret_cast<const floatx4*>(partial + (p0 + j) * C + c);
    *reinterpret_cast<floatx4*>(out + (int64_t)gid * C + c) = acc;
  }
}

__global__ void __launch_bounds__(256) latent_adjoint_zero_kernel(int64_t n4, floatx4* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n4) out[i] = floatx4{0.f, 0.f, 0.f, 0.f};
}

}  // namespace avr

// scratch regions of avr_latent_features_adjoint, 256-B aligned. A destination of more than one chunk walks
// rows > kAdjChunk rows in ceil(rows / kAdjChunk) < 2 rows / kAdjChunk chunks, and every point is walked by at
// most 4 destinations: at most 8 n_rows / kAdjChunk partial rows; at most 4 n_rows / kAdjChunk + n_texels chunks.
struct AdjScratch {
  int64_t keys, ranks, order, table, count, start, chunk0, pchunk0, partial, total;
  int64_t n_blocks, max_chunks, max_partials;
};

static AdjScratch adjoint_scratch(int n_scenes, int64_t n_points, int64_t hw, int channels) {
  const auto up = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
  const int64_t n_rows = (int64_t)n_scenes * n_points, n_texels = (int64_t)n_scenes * hw;
  AdjScratch m;
  m.n_blocks = (n_points + kAdjBlockPoints - 1) / kAdjBlockPoints;
  m.max_chunks = 4 * n_rows / kAdjChunk + n_texels;
  m.max_partials = 8 * n_rows / kAdjChunk;
  int64_t o = 0;
  m.keys = o;    o += up(n_rows * 4);
  m.ranks = o;   o += up(n_rows * 4);
  m.order = o;   o += up(n_rows * 4);
  m.table = o;   o += up(n_scenes * m.n_blocks * hw * 4);
  m.count = o;   o += up(n_texels * 4);
  m.start = o;   o += up((n_texels + 1) * 4);
  m.chunk0 = o;  o += up((n_texels + 1) * 4);
  m.pchunk0 = o; o += up((n_texels + 1) * 4);
  m.partial = o; o += up(m.max_partials * channels * 4);
  m.total = o;
  return m;
}

static int adjoint_sizes(const char* what, int n_scenes, int64_t n_points, int latent_h, int latent_w, int channels) {
  AVR_REQUIRE(n_scenes >= 1 && n_scenes <= AVR_MAX_SCENES, "%s: n_scenes %d not in 1..%d", what, n_scenes,
              AVR_MAX_SCENES);
  AVR_REQUIRE(latent_h > 0 && latent_w > 0 && (int64_t)latent_h * latent_w * n_scenes < (1ll << 31) / 2,
              "%s: bad latent size %d x %d", what, latent_h, latent_w);
  AVR_REQUIRE(channels > 0 && channels % 4 == 0, "%s: channels %d not a positive multiple of 4", what, channels);
  AVR_REQUIRE(n_points >= 0 && n_points * n_scenes < (1ll << 31) / 8, "%s: n_points %lld out of range", what,
              (long long)n_points);
  return AVR_OK;
}

extern "C" int avr_latent_features_adjoint_scratch_bytes(int n_scenes, int64_t n_points, int latent_h, int latent_w,
                                                         int channels, int64_t* n_bytes) {
  AVR_REQUIRE(n_bytes, "avr_latent_features_adjoint_scratch_bytes: null pointer");
  int rc = adjoint_sizes("avr_latent_features_adjoint_scratch_bytes", n_scenes, n_points, latent_h, latent_w, channels);
  if (rc) return rc;
  *n_bytes = adjoint_scratch(n_scenes, n_points, (int64_t)latent_h * latent_w, channels).total;
  return AVR_OK;
}

extern "C" int avr_latent_features_adjoint(const avr_view_desc* views, int n_scenes, const float* xyz,
                                           int64_t n_points, const float* grad_features, int64_t ld_grad,
                                           int channels, float* grad_latent_hwc, void* scratch,
                                           int64_t scratch_bytes, void* stream) {
  const char* what = "avr_latent_features_adjoint";
  AVR_REQUIRE(n_scenes >= 1 && n_scenes <= AVR_MAX_SCENES, "%s: n_scenes %d not in 1..%d", what, n_scenes,
              AVR_MAX_SCENES);
  AVR_REQUIRE(views && grad_latent_hwc && scratch && ((xyz && grad_features) || n_points == 0), "%s: null pointer",
              what);
  LatBatch vb;
  int rc = lookup_views(views, n_scenes, &vb, what);
  if (rc) return rc;
  rc = adjoint_sizes(what, n_scenes, n_points, views[0].latent_h, views[0].latent_w, channels);
  if (rc) return rc;
  AVR_REQUIRE(ld_grad >= channels, "%s: ld_grad %lld < channels %d", what, (long long)ld_grad, channels);
  AVR_REQUIRE(ld_grad % 4 == 0 && (uintptr_t)grad_features % 16 == 0 && (uintptr_t)grad_latent_hwc % 16 == 0 &&
                  (uintptr_t)scratch % 16 == 0,
              "%s: rows not 16-B aligned", what);
  const int hw = views[0].latent_h * views[0].latent_w;
  const AdjScratch m = adjoint_scratch(n_scenes, n_points, hw, channels);
  AVR_REQUIRE(scratch_bytes >= m.total, "%s: scratch of %lld bytes < %lld", what, (long long)scratch_bytes,
              (long long)m.total);
  hipStream_t st = as_stream(stream);
  const int n_texels = n_scenes * hw;
  const int64_t n_rows = (int64_t)n_scenes * n_points;
  if (n_points == 0) {
    const int64_t n4 = (int64_t)n_texels * channels / 4;
    latent_adjoint_zero_kernel<<<dim3((unsigned)((n4 + 255) / 256)), 256, 0, st>>>(
        n4, reinterpret_cast<floatx4*>(grad_latent_hwc));
    return check_launch("latent_adjoint_zero_kernel");
  }
  char* sb = static_cast<char*>(scratch);
  int* keys = reinterpret_cast<int*>(sb + m.keys);
  int* ranks = reinterpret_cast<int*>(sb + m.ranks);
  int* order = reinterpret_cast<int*>(sb + m.order);
  int* table = reinterpret_cast<int*>(sb + m.table);
  int* count = reinterpret_cast<int*>(sb + m.count);
  int* start = reinterpret_cast<int*>(sb + m.start);
  int* chunk0 = reinterpret_cast<int*>(sb + m.chunk0);
  int* pchunk0 = reinterpret_cast<int*>(sb + m.pchunk0);
  float* partial = reinterpret_cast<float*>(sb + m.partial);
  if (hipMemsetAsync(table, 0, (size_t)n_scenes * m.n_blocks * hw * 4, st) != hipSuccess)
    return check_launch("avr_latent_features_adjoint: clearing the counters");
  latent_adjoint_rank_kernel<<<dim3((unsigned)m.n_blocks, (unsigned)n_scenes), 64, 0, st>>>(
      vb, xyz, n_points, (int)m.n_blocks, table, keys, ranks);
  latent_adjoint_columns_kernel<<<dim3((unsigned)((n_texels + 255) / 256)), 256, 0, st>>>(n_texels, hw, (int)m.n_blocks,
                                                                                        table, count);
  latent_adjoint_offsets_kernel<<<1, kAdjScanThreads, 0, st>>>(n_texels, hw, views[0].latent_w, count, start, chunk0,
                                                               pchunk0);
  latent_adjoint_place_kernel<<<dim3((unsigned)((n_rows + 255) / 256)), 256, 0, st>>>(
      n_rows, n_points, hw, (int)m.n_blocks, keys, ranks, table, start, order);
  latent_adjoint_gather_kernel<<<dim3((unsigned)((m.max_chunks + 3) / 4)), 256, 0, st>>>(
      vb, xyz, n_points, grad_features, ld_grad, channels, n_texels, count, start, chunk0, pchunk0, order,
      m.max_partials, partial, grad_latent_hwc);
  latent_adjoint_reduce_kernel<<<dim3((unsigned)((n_texels + 3) / 4)), 256, 0, st>>>(
      channels, n_texels, chunk0, pchunk0, m.max_partials, partial, grad_latent_hwc);
  return check_launch("avr_latent_features_adjoint");
}
