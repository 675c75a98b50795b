// PSNR and SSIM of whole frames on the device: what get_metrics (utils.py:431-461) asks of skimage.metrics
// (peak_signal_noise_ratio(data_range=1), structural_similarity(channel_axis=-1, data_range=1)), for n_frames
// pairs of (height, width, 3) fp32 frames, pixel-major and channel-innermost as the renderers return them.
//   PSNR = 10 log10(1 / mse), mse over all height * width * 3 values (identical frames: +inf)
//   SSIM: per channel, the 7 x 7 uniform-window means ux, uy, uxx, uyy, uxy; sample covariances
//     v = 49/48 (u_ab - ua ub); S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), C1 = 1e-4,
//     C2 = 9e-4; the mean of S over the pixels whose window lies inside the frame (skimage crops the 3-pixel
//     border, so its filter's boundary mode never matters), then the mean of the three channels.
//
// metrics_tile_kernel, one launch for every frame, tile and channel: a workgroup owns kTileH x kTileW window
// positions of one frame. It stages their (kTileH + 6) x (kTileW + 6) pixels of both frames in LDS once (zeros
// past the frame), adding up the squared error of the staged pixels it owns on the way (every pixel has one
// owner: the tile whose first kTileH x kTileW staged pixels hold it, the last tile of a row / column also the
// rest). Then per channel the five window moments separably: a row pass (sums of 7 along x, to LDS) and a column
// pass (sums of 7 of those along y), S per window position. Products, sums and S in fp64: a product of two fp32
// values is exact in fp64, so uxx - ux^2 does not cancel as in skimage's own fp32 arithmetic. The workgroup's
// two fp64 sums go to partial[frame][tile]; metrics_finish_kernel (one wave per frame) adds a frame's tiles in
// index order. No floating-point atomics: bit-identical from run to run.
#include "avr_common.h"

namespace avr {

constexpr int kMetThreads = 256;
constexpr int kWin = 7;
constexpr int kTileH = 16, kTileW = 32;                         // window positions per workgroup
constexpr int kStageH = kTileH + kWin - 1, kStageW = kTileW + kWin - 1;
constexpr int kStageRow = 3 * kStageW;                          // floats per staged row (stride 3 per pixel: odd,
                                                                // so the lanes of a row read distinct banks)

struct MetricsTiles {
  int tiles_x, tiles_y;
};

static MetricsTiles metrics_tiles(int height, int width) {
  return {(width - (kWin - 1) + kTileW - 1) / kTileW, (height - (kWin - 1) + kTileH - 1) / kTileH};
}

__global__ void __launch_bounds__(kMetThreads) metrics_tile_kernel(const float* __restrict__ img,
                                                                   const float* __restrict__ gt, int height,
                                                                   int width, int tiles_x, int tiles_y,
                                                                   double* __restrict__ partial) {
  __shared__ float sx[kStageH * kStageRow], sy[kStageH * kStageRow];
  __shared__ double rowm[5][kStageH][kTileW];
  __shared__ double wsum[2][kMetThreads / kWave];

  const int tiles = tiles_x * tiles_y;
  const int64_t frame = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles, ty = tile / tiles_x, tx = tile % tiles_x;
  const int y0 = ty * kTileH, x0 = tx * kTileW;
  const bool last_y = ty == tiles_y - 1, last_x = tx == tiles_x - 1;
  const float* fi = img + frame * height * width * 3;
  const float* fg = gt + frame * height * width * 3;

  // stage both frames' pixels; the squared error of the ones this tile owns
  double se = 0.0;
  for (int i = threadIdx.x; i < kStageH * kStageRow; i += kMetThreads) {
    const int r = i / kStageRow, xc = i % kStageRow, px = xc / 3;
    const int y = y0 + r, x = x0 + px;
    float a = 0.f, b = 0.f;
    if (y < height && x < width) {
      const int64_t at = ((int64_t)y * width + x0) * 3 + xc;
      a = fi[at];
      b = fg[at];
      if ((r < kTileH || last_y) && (px < kTileW || last_x)) {
        const double d = (double)a - (double)b;
        se += d * d;
      }
    }
    sx[i] = a;
    sy[i] = b;
  }
  __syncthreads();

  const int out_h = height - (kWin - 1), out_w = width - (kWin - 1);   // window positions of the frame
  double ss = 0.0;
  for (int c = 0; c < 3; ++c) {
    // row pass: the five sums over x .. x + 6 of every staged row
    for (int i = threadIdx.x; i < kStageH * kTileW; i += kMetThreads) {
      const int r = i / kTileW, x = i % kTileW;
      const float* px = sx + r * kStageRow + 3 * x + c;
      const float* py = sy + r * kStageRow + 3 * x + c;
      double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k = 0; k < kWin; ++k) {
        const double a = (double)px[3 * k], b = (double)py[3 * k];
        m[0] += a;
        m[1] += b;
        m[2] += a * a;
        m[3] += b * b;
        m[4] += a * b;
      }
#pragma unroll
      for (int q = 0; q < 5; ++q) rowm[q][r][x] = m[q];
    }
    __syncthreads();
    // column pass and S
    for (int i = threadIdx.x; i < kTileH * kTileW; i += kMetThreads) {
      const int y = i / kTileW, x = i % kTileW;
      if (y0 + y >= out_h || x0 + x >= out_w) continue;
      double u[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < kWin; ++k) s += rowm[q][y + k][x];
        u[q] = s / (double)(kWin * kWin);
      }
      constexpr double kCov = (double)(kWin * kWin) / (double)(kWin * kWin - 1);
      constexpr double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
      const double vx = kCov * (u[2] - u[0] * u[0]), vy = kCov * (u[3] - u[1] * u[1]);
      const double vxy = kCov * (u[4] - u[0] * u[1]);
      const double num = (2.0 * (u[0] * u[1]) + C1) * (2.0 * vxy + C2);
      const double den = (u[0] * u[0] + u[1] * u[1] + C1) * (vx + vy + C2);
      ss += num / den;
    }
    __syncthreads();   // rowm is rewritten by the next channel
  }

  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  ss = wave_sum_d(ss);
  se = wave_sum_d(se);
  if (lane == 0) {
    wsum[0][wave] = ss;
    wsum[1][wave] = se;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < kMetThreads / kWave; ++w) {
      a += wsum[0][w];
      b += wsum[1][w];
    }
    partial[2 * (int64_t)blockIdx.x + 0] = a;
    partial[2 * (int64_t)blockIdx.x + 1] = b;
  }
}

// one wave per frame: lane l adds tiles l, l + 64, ... in order, then the lanes' sums (a fixed tree)
__global__ void __launch_bounds__(kWave) metrics_finish_kernel(int height, int width, int tiles,
                                                               const double* __restrict__ partial,
                                                               float* __restrict__ psnr, float* __restrict__ ssim) {
  const double* p = partial + 2 * (int64_t)blockIdx.x * tiles;
  double ss = 0.0, se = 0.0;
  for (int t = threadIdx.x; t < tiles; t += kWave) {
    ss += p[2 * t + 0];
    se += p[2 * t + 1];
  }
  ss = wave_sum_d(ss);
  se = wave_sum_d(se);
  if (threadIdx.x == 0) {
    const double mse = se / ((double)height * (double)width * 3.0);
    const double n_pos = (double)(height - (kWin - 1)) * (double)(width - (kWin - 1)) * 3.0;
    psnr[blockIdx.x] = (float)(10.0 * log10(1.0 / mse));
    ssim[blockIdx.x] = (float)(ss / n_pos);
  }
}

}  // namespace avr

using namespace avr;

static int metrics_check_sizes(const char* who, int64_t n_frames, int height, int width) {
  AVR_REQUIRE(n_frames >= 0, "%s: n_frames %lld", who, (long long)n_frames);
  AVR_REQUIRE(height >= kWin && width >= kWin && height <= (1 << 20) && width <= (1 << 20),
              "%s: frames of %d x %d (the 7 x 7 SSIM window needs height, width >= 7)", who, height, width);
  const MetricsTiles t = metrics_tiles(height, width);
  AVR_REQUIRE(n_frames * t.tiles_x * t.tiles_y < (1ll << 31) && n_frames < (1ll << 31), "%s: too many tiles (%lld frames)",
              who, (long long)n_frames);
  return AVR_OK;
}

extern "C" int avr_image_metrics_workspace_bytes(int64_t n_frames, int height, int width, int64_t* n_bytes) {
  AVR_REQUIRE(n_bytes, "avr_image_metrics_workspace_bytes: null pointer");
  if (const int rc = metrics_check_sizes("avr_image_metrics_workspace_bytes", n_frames, height, width)) return rc;
  const MetricsTiles t = metrics_tiles(height, width);
  *n_bytes = n_frames * t.tiles_x * t.tiles_y * 2 * (int64_t)sizeof(double);
  return AVR_OK;
}

extern "C" int avr_image_metrics(const float* img, const float* gt, int64_t n_frames, int height, int width,
                                 void* workspace, int64_t workspace_bytes, float* psnr, float* ssim, void* stream) {
  if (const int rc = metrics_check_sizes("avr_image_metrics", n_frames, height, width)) return rc;
  if (n_frames == 0) return AVR_OK;
  AVR_REQUIRE(img && gt && workspace && psnr && ssim, "avr_image_metrics: null pointer");
  const MetricsTiles t = metrics_tiles(height, width);
  const int64_t blocks = n_frames * t.tiles_x * t.tiles_y;
  AVR_REQUIRE(workspace_bytes >= blocks * 2 * (int64_t)sizeof(double) &&
                  (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
              "avr_image_metrics: the workspace needs avr_image_metrics_workspace_bytes() bytes, 8-B aligned (got %lld)",
              (long long)workspace_bytes);
  hipStream_t s = as_stream(stream);
  double* partial = reinterpret_cast<double*>(workspace);
  metrics_tile_kernel<<<(unsigned)blocks, kMetThreads, 0, s>>>(img, gt, height, width, t.tiles_x, t.tiles_y, partial);
  metrics_finish_kernel<<<(unsigned)n_frames, kWave, 0, s>>>(height, width, t.tiles_x * t.tiles_y, partial, psnr,
                                                            ssim);
  return check_launch("metrics_tile_kernel");
}
