// avr_adam_step: torch.optim.Adam's update (train.py:112-114, :299) of a list of fp32 tensors in one launch
// per AVR_ADAM_MAX_TENSORS tensors, plus a one-wave launch that advances the step counter.
//
// Elementwise and HBM-bound: per element p, g, m, v are read and p, m, v written (28 B). The tensor list
// travels by value in the kernel arguments (as LinBatch / X3PackBatch in field.hip), so a captured graph holds
// the pointers in its node and nothing is read from the host or allocated at replay time. Work is cut into
// chunks of AVR_ADAM_CHUNK elements; a flat chunk index finds its tensor through the prefix table of the
// argument block (a binary search on wave-uniform values: scalar loads of the kernel-argument segment), the grid
// is capped and strides over the chunks. The step counter is one float in device memory that only the device
// reads: every workgroup of the update launches reads it, none writes it; the trailing launch adds 1.
#include "avr_common.h"

namespace avr {

constexpr int kAdamThreads = 256;
constexpr int kAdamMaxGrid = 2048;
constexpr int kAdamVec = AVR_ADAM_CHUNK / (4 * kAdamThreads);   // float4 per thread and chunk
static_assert(AVR_ADAM_CHUNK == kAdamVec * 4 * kAdamThreads && kAdamVec >= 1, "a chunk is whole float4 rows of the workgroup");

struct AdamBatch {
  float* p[AVR_ADAM_MAX_TENSORS];
  const float* g[AVR_ADAM_MAX_TENSORS];
  float* m[AVR_ADAM_MAX_TENSORS];
  float* v[AVR_ADAM_MAX_TENSORS];
  int64_t numel[AVR_ADAM_MAX_TENSORS];
  int first_chunk[AVR_ADAM_MAX_TENSORS + 1];   // prefix sums of the tensors' chunk counts; [count] = all chunks
  int count;
  double lr, beta1, beta2;                     // for the bias corrections (fp64 on the device)
  float w1, b2, w2, eps, wd;                   // 1 - beta1, beta2, 1 - beta2, eps, weight_decay: rounded once
  const float* step;
};
static_assert(sizeof(AdamBatch) <= 4096, "the tensor list must fit the 4 KB kernel-argument block");

struct AdamFactors {
  float w1, b2, w2, eps, wd;
  float neg_step_size;    // -(lr / (1 - beta1^t))
  float bc2_sqrt;         // sqrt(1 - beta2^t)
};

// torch's _single_tensor_adam, one rounding per operation (the build has -ffp-contract=off). NaN and inf in g
// propagate as the formula does.
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamFactors& f) {
  if (f.wd != 0.f) g = g + f.wd * p;
  m = m + (g - m) * f.w1;
  v = v * f.b2 + (f.w2 * g) * g;
  const float denom = sqrtf(v) / f.bc2_sqrt + f.eps;
  p = p + f.neg_step_size * (m / denom);
}

__device__ __forceinline__ void adam_elem4(floatx4& p, floatx4 g, floatx4& m, floatx4& v, const AdamFactors& f) {
  if (f.wd != 0.f) g = g + f.wd * p;
  m = m + (g - m) * f.w1;
  v = v * f.b2 + (f.w2 * g) * g;
  const floatx4 denom = floatx4{sqrtf(v.x), sqrtf(v.y), sqrtf(v.z), sqrtf(v.w)} / f.bc2_sqrt + f.eps;
  p = p + f.neg_step_size * (m / denom);
}

__device__ __forceinline__ floatx4 ld4(const float* a) { return *reinterpret_cast<const floatx4*>(a); }
__device__ __forceinline__ void st4(float* a, floatx4 x) { *reinterpret_cast<floatx4*>(a) = x; }

__global__ void __launch_bounds__(kAdamThreads) adam_kernel(AdamBatch bt) {
  __shared__ float s_bc[2];
  if (threadIdx.x == 0) {
    // t = step + 1 in fp32 as torch's counter; beta^t by squaring in fp64 (t an integer below 2^24 + 1)
    unsigned t = (unsigned)(*bt.step + 1.f);
    double p1 = 1.0, p2 = 1.0, a1 = bt.beta1, a2 = bt.beta2;
    for (; t; t >>= 1) {
      if (t & 1u) { p1 *= a1; p2 *= a2; }
      a1 *= a1;
      a2 *= a2;
    }
    s_bc[0] = (float)(-(bt.lr / (1.0 - p1)));
    s_bc[1] = (float)sqrt(1.0 - p2);
  }
  __syncthreads();
  const AdamFactors f{bt.w1, bt.b2, bt.w2, bt.eps, bt.wd, s_bc[0], s_bc[1]};
  const int total = bt.first_chunk[bt.count];
  for (int c = blockIdx.x; c < total; c += gridDim.x) {
    int lo = 0, hi = bt.count;   // the tensor k with first_chunk[k] <= c < first_chunk[k + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (bt.first_chunk[mid] <= c) lo = mid; else hi = mid;
    }
    const int64_t off = (int64_t)(c - bt.first_chunk[lo]) * AVR_ADAM_CHUNK;
    const int64_t left = bt.numel[lo] - off;
    const int n = left < AVR_ADAM_CHUNK ? (int)left : AVR_ADAM_CHUNK;
    float* p = bt.p[lo] + off;
    const float* g = bt.g[lo] + off;
    float* m = bt.m[lo] + off;
    float* v = bt.v[lo] + off;
    const bool aligned = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;   // off % 4 == 0
    const int n4 = aligned ? n >> 2 : 0;
    if (n4 == kAdamVec * kAdamThreads) {   // a whole chunk: every load of the thread in flight before the math
      floatx4 P[kAdamVec], G[kAdamVec], M[kAdamVec], V[kAdamVec];
#pragma unroll
      for (int k = 0; k < kAdamVec; ++k) {
        const int i = 4 * (k * kAdamThreads + threadIdx.x);
        P[k] = ld4(p + i); G[k] = ld4(g + i); M[k] = ld4(m + i); V[k] = ld4(v + i);
      }
#pragma unroll
      for (int k = 0; k < kAdamVec; ++k) {
        const int i = 4 * (k * kAdamThreads + threadIdx.x);
        adam_elem4(P[k], G[k], M[k], V[k], f);
        st4(p + i, P[k]); st4(m + i, M[k]); st4(v + i, V[k]);
      }
    } else {
      for (int q = threadIdx.x; q < n4; q += kAdamThreads) {
        const int i = 4 * q;
        floatx4 P = ld4(p + i), G = ld4(g + i), M = ld4(m + i), V = ld4(v + i);
        adam_elem4(P, G, M, V, f);
        st4(p + i, P); st4(m + i, M); st4(v + i, V);
      }
      for (int i = 4 * n4 + threadIdx.x; i < n; i += kAdamThreads) {   // the tail, or a tensor not 16-B aligned
        float P = p[i], M = m[i], V = v[i];
        adam_elem(P, g[i], M, V, f);
        p[i] = P; m[i] = M; v[i] = V;
      }
    }
  }
}

// after the update launches of a call (stream order): no launch both reads and writes the counter
__global__ void __launch_bounds__(kWave) adam_advance_kernel(float* step) {
  if (threadIdx.x == 0) *step = *step + 1.f;
}

}  // namespace avr

using namespace avr;

static int launch_adam(AdamBatch& bt, hipStream_t s) {
  if (bt.count == 0) return AVR_OK;
  const int total = bt.first_chunk[bt.count];
  adam_kernel<<<total < kAdamMaxGrid ? total : kAdamMaxGrid, kAdamThreads, 0, s>>>(bt);
  bt.count = 0;
  return check_launch("adam_kernel");
}

extern "C" int avr_adam_step(const avr_adam_tensor* tensors, int64_t n_tensors, double lr, double beta1, double beta2,
                             double eps, double weight_decay, float* step, void* stream) {
  AVR_REQUIRE(n_tensors >= 0, "avr_adam_step: negative n_tensors");
  if (n_tensors == 0) return AVR_OK;
  AVR_REQUIRE(tensors, "avr_adam_step: null tensor list");
  AVR_REQUIRE(step, "avr_adam_step: null step counter");
  AVR_REQUIRE(lr >= 0.0, "avr_adam_step: invalid lr %g (must be >= 0)", lr);
  AVR_REQUIRE(beta1 >= 0.0 && beta1 < 1.0, "avr_adam_step: invalid beta1 %g (must be in [0, 1))", beta1);
  AVR_REQUIRE(beta2 >= 0.0 && beta2 < 1.0, "avr_adam_step: invalid beta2 %g (must be in [0, 1))", beta2);
  AVR_REQUIRE(eps >= 0.0, "avr_adam_step: invalid eps %g (must be >= 0)", eps);
  AVR_REQUIRE(weight_decay >= 0.0, "avr_adam_step: invalid weight_decay %g (must be >= 0)", weight_decay);
  constexpr int64_t kMaxChunks = 1ll << 30;   // per launch: the prefix table is int
  for (int64_t k = 0; k < n_tensors; ++k) {
    const avr_adam_tensor& T = tensors[k];
    AVR_REQUIRE(T.numel >= 0, "avr_adam_step: tensor %lld has a negative numel", (long long)k);
    if (T.numel == 0) continue;
    AVR_REQUIRE(T.param && T.grad && T.exp_avg && T.exp_avg_sq, "avr_adam_step: tensor %lld has a null pointer",
                (long long)k);
    AVR_REQUIRE((T.numel + AVR_ADAM_CHUNK - 1) / AVR_ADAM_CHUNK <= kMaxChunks, "avr_adam_step: tensor %lld too large",
                (long long)k);
  }
  hipStream_t s = as_stream(stream);
  AdamBatch bt{};
  bt.lr = lr; bt.beta1 = beta1; bt.beta2 = beta2;
  bt.w1 = (float)(1.0 - beta1); bt.b2 = (float)beta2; bt.w2 = (float)(1.0 - beta2);
  bt.eps = (float)eps; bt.wd = (float)weight_decay;
  bt.step = step;
  int rc;
  for (int64_t k = 0; k < n_tensors; ++k) {
    const avr_adam_tensor& T = tensors[k];
    if (T.numel == 0) continue;
    const int64_t chunks = (T.numel + AVR_ADAM_CHUNK - 1) / AVR_ADAM_CHUNK;
    if (bt.count == AVR_ADAM_MAX_TENSORS || bt.first_chunk[bt.count] + chunks > kMaxChunks)
      if ((rc = launch_adam(bt, s))) return rc;
    const int c = bt.count++;
    bt.p[c] = T.param; bt.g[c] = T.grad; bt.m[c] = T.exp_avg; bt.v[c] = T.exp_avg_sq;
    bt.numel[c] = T.numel;
    bt.first_chunk[c + 1] = bt.first_chunk[c] + (int)chunks;
  }
  if ((rc = launch_adam(bt, s))) return rc;
  adam_advance_kernel<<<1, kWave, 0, s>>>(step);
  return check_launch("adam_advance_kernel");
}
