// One step of the LSTM ray march (renderers.py:320-343, :413-432), shared by raymarch_kernel,
// raymarch_train_kernel (raymarch.hip) and adaptive_front_kernel (adaptive.hip): the three run the same
// instructions on the same values, so their marched points agree bit for bit.
// One ray per 16 lanes; lane k owns hidden unit k (its 4 gate rows of W_hh stay in registers, h_j comes in by
// 16-lane shuffles).
#pragma once
#include "field_common.h"

namespace avr {

constexpr int kHid = 16;           // LSTMCell hidden size (renderers.py:301, :370)
constexpr int kGates = 4 * kHid;   // i, f, g, o

__device__ __forceinline__ float sigmoid_(float x) { return fdiv(1.0f, fadd(1.0f, expf(-x))); }

// Source views of a multi-scene launch (ray r in scene r / n_per_scene).
struct MarchScenes {
  View v[AVR_MAX_SCENES];
};

inline int march_scenes(const avr_view_desc* views, int n_scenes, MarchScenes* sc, const char* what) {
  AVR_REQUIRE(views && n_scenes >= 1 && n_scenes <= AVR_MAX_SCENES, "%s: 1..%d scenes", what, AVR_MAX_SCENES);
  for (int s = 0; s < n_scenes; ++s) {
    AVR_REQUIRE(views[s].latent_h == views[0].latent_h && views[s].latent_w == views[0].latent_w &&
                    views[s].latent_h > 0 && views[s].latent_w > 0,
                "%s: scenes need latent maps of one (positive) size", what);
    view_from_desc(&views[s], &sc->v[s]);
  }
  return AVR_OK;
}

// Lane k's share of the LSTMCell / out_layer parameters (torch layout: w_hh (64, 16), b_ih / b_hh (64),
// w_out (16), b_out (1)).
struct MarchLane {
  float wr[4][kHid], bias[4], wo, bo;
};

__device__ __forceinline__ MarchLane march_lane(const float* __restrict__ w_hh, const float* __restrict__ b_ih,
                                                const float* __restrict__ b_hh, const float* __restrict__ w_out,
                                                const float* __restrict__ b_out, int k) {
  MarchLane L;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int j = 0; j < kHid; ++j) L.wr[q][j] = w_hh[(q * kHid + k) * kHid + j];
    L.bias[q] = fadd(b_ih[q * kHid + k], b_hh[q * kHid + k]);
  }
  L.wo = w_out[k];
  L.bo = b_out[0];
  return L;
}

struct MarchGateValues {
  float ig, fg, gg, og;
};

// The step at point x: v = bilinear blend of the per-texel input projections (W_ih v, `table`), (h, c) =
// LSTMCell(v, (h, c)), returns sd = out_layer(h) (the same value on the ray's 16 lanes). `gates`: unit k's
// activations (the training forward stores them).
__device__ __forceinline__ float march_step(const View& v, const float* __restrict__ table, const MarchLane& L, float x0,
                                            float x1, float x2, float& h, float& c, MarchGateValues& gates) {
  const int k = threadIdx.x & (kHid - 1);
  const Bilinear bl = bilinear_at(v, x0, x1, x2);
  float g[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    // W_ih v + b_ih: bilinear blend of the per-texel projections
    const int row = q * kHid + k;
    const float p = ((table[(int64_t)bl.tex[0] * kGates + row] * bl.w[0] +
                      table[(int64_t)bl.tex[1] * kGates + row] * bl.w[1]) +
                     table[(int64_t)bl.tex[2] * kGates + row] * bl.w[2]) +
                    table[(int64_t)bl.tex[3] * kGates + row] * bl.w[3];
    g[q] = p + L.bias[q];
  }
#pragma unroll
  for (int j = 0; j < kHid; ++j) {
    const float hj = __shfl(h, j, kHid);
#pragma unroll
    for (int q = 0; q < 4; ++q) g[q] = fmaf(L.wr[q][j], hj, g[q]);
  }
  gates.ig = sigmoid_(g[0]);
  gates.fg = sigmoid_(g[1]);
  gates.gg = tanhf(g[2]);
  gates.og = sigmoid_(g[3]);
  c = fadd(fmul(gates.fg, c), fmul(gates.ig, gates.gg));
  h = fmul(gates.og, tanhf(c));
  float sd = fmul(L.wo, h);
#pragma unroll
  for (int d = kHid / 2; d > 0; d >>= 1) sd = fadd(sd, __shfl_xor(sd, d, kHid));
  return fadd(sd, L.bo);
}

}  // namespace avr
