// The training loss of train.py (utils.py:364-377), forward and backward, without a host sync:
//   loss = [mse(rgb_c, gt)] + [mse(rgb_f, gt)]  (NaN -> 1e-6)  + [10000 mean(max(near - d, 0) + max(d - far, 0))]
// over n rays: rgb_c, rgb_f, gt (n, 3) interleaved as the renderers return them, depth (n). The reference's
// `if loss.isnan(): loss = 1e-6` reads the loss on the host every step; here the decision is taken on the device
// and kept in the forward's record for the backward, so the loss can be recorded in a HIP-graph capture.
//
// Forward: one pass, loss_partial_kernel. A grid that depends on n alone walks the 3 n colour values and the n
// depths; differences, squares and sums in fp64; each workgroup reduces its three sums (wave shuffles, then its
// waves in order). One workgroup (n <= kLossSingle) writes the record itself; more write their partials to the
// workspace and loss_finish_kernel (one wave) adds them in index order. No floating-point atomics: the loss is
// bit-identical from run to run. record = {loss, mse_c, mse_f, penalty} (the MSEs as summed: NaN where the sum
// was; 0 for a term not selected).
// Backward: loss_bwd_kernel, one launch for the three gradients. It reads the upstream gradient from device
// memory and the NaN decision from the record (no second reduction):
//   d rgb = g 2 (rgb - gt) / (3 n), exactly 0 where the MSE part was NaN
//   d depth = g 10000 / n (c(d - far) - c(near - d)), c(t) = 1 for t > 0, 0.5 at t == 0, 0 for t < 0
// (torch.max(a, b)'s backward halves the gradient at a tie; a NaN passes it, as aten's masked_fill(a < b, 0)),
// each value computed in fp64 and rounded once.
#include "avr_common.h"

namespace avr {

constexpr int kLossThreads = 1024;
constexpr int kLossPerThread = 8;                               // colour values per thread per workgroup
constexpr int64_t kLossTile = (int64_t)kLossThreads * kLossPerThread;
constexpr int kLossMaxBlocks = 256;                             // one per CU
constexpr double kLossNanValue = 1e-6;                          // utils.py:373
constexpr double kLossPenaltyScale = 10000.0;                   // utils.py:376

static int loss_blocks(int64_t n) {
  const int64_t b = (3 * n + kLossTile - 1) / kLossTile;
  return (int)(b < kLossMaxBlocks ? b : kLossMaxBlocks);
}

// torch.max(t, 0) of the penalty arms: a NaN propagates (fmax would drop it)
__device__ __forceinline__ double relu_nan(double t) { return t < 0.0 ? 0.0 : t; }

__device__ __forceinline__ bool mse_part_is_nan(float mse_c, float mse_f) {
  // a term that was not selected is 0; the sums are of squares (never inf - inf), so the part is NaN exactly
  // where one of its terms is
  return mse_c != mse_c || mse_f != mse_f;
}

__device__ __forceinline__ void write_record(double sc, double sf, double sp, int64_t n, float* record) {
  const double mc = sc / (3.0 * (double)n), mf = sf / (3.0 * (double)n);
  const double pen = kLossPenaltyScale * (sp / (double)n);
  double mse = mc + mf;
  if (mse != mse) mse = kLossNanValue;
  record[0] = (float)(mse + pen);
  record[1] = (float)mc;
  record[2] = (float)mf;
  record[3] = (float)pen;
}

// the workgroup's sums of three per-thread values: every thread returns them (only thread 0 uses them)
__device__ __forceinline__ void block_sum3(double& a, double& b, double& c) {
  __shared__ double part[3][kLossThreads / kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  a = wave_sum_d(a);
  b = wave_sum_d(b);
  c = wave_sum_d(c);
  if (lane == 0) {
    part[0][wave] = a;
    part[1][wave] = b;
    part[2][wave] = c;
  }
  __syncthreads();
  a = b = c = 0.0;
  for (int w = 0; w < kLossThreads / kWave; ++w) {
    a += part[0][w];
    b += part[1][w];
    c += part[2][w];
  }
}

// rgb_c / rgb_f / depth NULL: the term is not selected
__global__ void __launch_bounds__(kLossThreads) loss_partial_kernel(int64_t n, const float* __restrict__ rgb_c,
                                                                    const float* __restrict__ rgb_f,
                                                                    const float* __restrict__ depth,
                                                                    const float* __restrict__ gt, float near_,
                                                                    float far_, double* __restrict__ partial,
                                                                    float* __restrict__ record) {
  const int64_t n3 = 3 * n, stride = (int64_t)gridDim.x * kLossThreads;
  const int64_t first = (int64_t)blockIdx.x * kLossThreads + threadIdx.x;
  double sc = 0.0, sf = 0.0, sp = 0.0;
  for (int64_t i = first; i < n3; i += stride) {
    const double t = (double)gt[i];
    if (rgb_c) {
      const double d = (double)rgb_c[i] - t;
      sc += d * d;
    }
    if (rgb_f) {
      const double d = (double)rgb_f[i] - t;
      sf += d * d;
    }
  }
  if (depth) {
    for (int64_t i = first; i < n; i += stride) {
      const double d = (double)depth[i];
      sp += relu_nan((double)near_ - d) + relu_nan(d - (double)far_);
    }
  }
  block_sum3(sc, sf, sp);
  if (threadIdx.x != 0) return;
  if (gridDim.x == 1) {
    write_record(sc, sf, sp, n, record);
  } else {
    partial[3 * blockIdx.x + 0] = sc;
    partial[3 * blockIdx.x + 1] = sf;
    partial[3 * blockIdx.x + 2] = sp;
  }
}

// one wave: lane l adds partials l, l + 64, ... in order, then the lanes' sums (a fixed tree)
__global__ void __launch_bounds__(kWave) loss_finish_kernel(int64_t n, int n_partials,
                                                            const double* __restrict__ partial,
                                                            float* __restrict__ record) {
  double sc = 0.0, sf = 0.0, sp = 0.0;
  for (int b = threadIdx.x; b < n_partials; b += kWave) {
    sc += partial[3 * b + 0];
    sf += partial[3 * b + 1];
    sp += partial[3 * b + 2];
  }
  sc = wave_sum_d(sc);
  sf = wave_sum_d(sf);
  sp = wave_sum_d(sp);
  if (threadIdx.x == 0) write_record(sc, sf, sp, n, record);
}

__device__ __forceinline__ double tie_slope(double t) { return t < 0.0 ? 0.0 : (t == 0.0 ? 0.5 : 1.0); }

// grad_* NULL: that gradient is not wanted (or its term not selected)
__global__ void __launch_bounds__(256) loss_bwd_kernel(int64_t n, const float* __restrict__ rgb_c,
                                                       const float* __restrict__ rgb_f,
                                                       const float* __restrict__ depth,
                                                       const float* __restrict__ gt, float near_, float far_,
                                                       const float* __restrict__ record,
                                                       const float* __restrict__ grad_loss,
                                                       float* __restrict__ grad_c, float* __restrict__ grad_f,
                                                       float* __restrict__ grad_d) {
  const int64_t n3 = 3 * n, stride = (int64_t)gridDim.x * 256;
  const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const double g = (double)grad_loss[0];
  const bool nan_rule = mse_part_is_nan(record[1], record[2]);
  const double s_rgb = g * (2.0 / (3.0 * (double)n)), s_d = g * (kLossPenaltyScale / (double)n);
  if (grad_c || grad_f) {
    for (int64_t i = first; i < n3; i += stride) {
      const double t = (double)gt[i];
      if (grad_c) grad_c[i] = nan_rule ? 0.f : (float)(s_rgb * ((double)rgb_c[i] - t));
      if (grad_f) grad_f[i] = nan_rule ? 0.f : (float)(s_rgb * ((double)rgb_f[i] - t));
    }
  }
  if (grad_d) {
    for (int64_t i = first; i < n; i += stride) {
      const double d = (double)depth[i];
      grad_d[i] = (float)(s_d * (tie_slope(d - (double)far_) - tie_slope((double)near_ - d)));
    }
  }
}

}  // namespace avr

using namespace avr;

static bool loss_terms_ok(int terms) { return terms > 0 && terms <= 7 && (terms & (AVR_LOSS_COARSE | AVR_LOSS_FINE)); }

extern "C" int avr_loss_workspace_bytes(int64_t n_rays, int64_t* n_bytes) {
  AVR_REQUIRE(n_bytes, "avr_loss_workspace_bytes: null pointer");
  AVR_REQUIRE(n_rays >= 0 && n_rays < (1ll << 60), "avr_loss_workspace_bytes: n_rays %lld", (long long)n_rays);
  *n_bytes = (int64_t)loss_blocks(n_rays) * 3 * (int64_t)sizeof(double);
  return AVR_OK;
}

extern "C" int avr_loss_fwd(int64_t n_rays, int terms, const float* rgb_c, const float* rgb_f, const float* depth,
                            const float* gt, float near_, float far_, void* workspace, int64_t workspace_bytes,
                            float* record, void* stream) {
  AVR_REQUIRE(n_rays >= 0 && n_rays < (1ll << 60), "avr_loss_fwd: n_rays %lld", (long long)n_rays);
  AVR_REQUIRE(loss_terms_ok(terms), "avr_loss_fwd: empty or unknown selection of terms (%d): AVR_LOSS_COARSE or "
              "AVR_LOSS_FINE, with or without AVR_LOSS_DEPTH", terms);
  if (n_rays == 0) return AVR_OK;
  AVR_REQUIRE(gt && record && (!(terms & AVR_LOSS_COARSE) || rgb_c) && (!(terms & AVR_LOSS_FINE) || rgb_f) &&
                  (!(terms & AVR_LOSS_DEPTH) || depth),
              "avr_loss_fwd: null pointer");
  const int blocks = loss_blocks(n_rays);
  AVR_REQUIRE(blocks == 1 || (workspace && workspace_bytes >= (int64_t)blocks * 3 * (int64_t)sizeof(double) &&
                              (reinterpret_cast<uintptr_t>(workspace) & 7) == 0),
              "avr_loss_fwd: the workspace needs avr_loss_workspace_bytes() bytes, 8-B aligned (got %lld)",
              (long long)workspace_bytes);
  hipStream_t s = as_stream(stream);
  double* partial = reinterpret_cast<double*>(workspace);
  loss_partial_kernel<<<blocks, kLossThreads, 0, s>>>(n_rays, (terms & AVR_LOSS_COARSE) ? rgb_c : nullptr,
                                                      (terms & AVR_LOSS_FINE) ? rgb_f : nullptr,
                                                      (terms & AVR_LOSS_DEPTH) ? depth : nullptr, gt, near_, far_,
                                                      partial, record);
  if (blocks > 1) loss_finish_kernel<<<1, kWave, 0, s>>>(n_rays, blocks, partial, record);
  return check_launch("loss_partial_kernel");
}

extern "C" int avr_loss_bwd(int64_t n_rays, int terms, const float* rgb_c, const float* rgb_f, const float* depth,
                            const float* gt, float near_, float far_, const float* record, const float* grad_loss,
                            float* grad_rgb_c, float* grad_rgb_f, float* grad_depth, void* stream) {
  AVR_REQUIRE(n_rays >= 0 && n_rays < (1ll << 60), "avr_loss_bwd: n_rays %lld", (long long)n_rays);
  AVR_REQUIRE(loss_terms_ok(terms), "avr_loss_bwd: empty or unknown selection of terms (%d)", terms);
  if (n_rays == 0) return AVR_OK;
  AVR_REQUIRE(!grad_rgb_c || (terms & AVR_LOSS_COARSE), "avr_loss_bwd: grad_rgb_c of a term that is not selected");
  AVR_REQUIRE(!grad_rgb_f || (terms & AVR_LOSS_FINE), "avr_loss_bwd: grad_rgb_f of a term that is not selected");
  AVR_REQUIRE(!grad_depth || (terms & AVR_LOSS_DEPTH), "avr_loss_bwd: grad_depth of a term that is not selected");
  AVR_REQUIRE(gt && record && grad_loss && (!grad_rgb_c || rgb_c) && (!grad_rgb_f || rgb_f) && (!grad_depth || depth),
              "avr_loss_bwd: null pointer");
  if (!grad_rgb_c && !grad_rgb_f && !grad_depth) return AVR_OK;
  const int64_t work = (grad_rgb_c || grad_rgb_f) ? 3 * n_rays : n_rays;
  const int64_t blocks = (work + 256 * 4 - 1) / (256 * 4);
  loss_bwd_kernel<<<(unsigned)(blocks < 2048 ? blocks : 2048), 256, 0, as_stream(stream)>>>(
      n_rays, rgb_c, rgb_f, depth, gt, near_, far_, record, grad_loss, grad_rgb_c, grad_rgb_f, grad_depth);
  return check_launch("loss_bwd_kernel");
}
