// Ascending bitonic sort of one float per lane across a wave64 (sample_fine_kernel's fine / depth lists,
// adaptive_front_kernel's band): partners through DPP / swizzle / permlane swaps, no LDS round trips.
#pragma once
#include "avr_common.h"

namespace avr {

// lanes of a bitonic stage (k, j) that keep the minimum: ((l & k) == 0) == ((l & j) == 0)
__host__ __device__ constexpr uint64_t bitonic_min_lanes(int k, int j) {
  uint64_t m = 0;
  for (int l = 0; l < 64; ++l)
    if (((l & k) == 0) == ((l & j) == 0)) m |= 1ull << l;
  return m;
}

// partner value of lane l ^ J for the sort: quad-permute DPP (J = 1, 2; left
// to the compiler to fold into the min/max), a ds_swizzle xor within 32 lanes
// (J = 4, 8, 16: LDS crossbar, no memory traffic, one instruction instead of
// two DPP rows and a select), the permlane32 swap for J = 32
template <int J>
__device__ __forceinline__ float sort_partner(float v, int lane) {
  const int b = __float_as_int(v);
  if constexpr (J == 1) return __int_as_float(__builtin_amdgcn_mov_dpp(b, 0xB1, 0xf, 0xf, false));
  else if constexpr (J == 2) return __int_as_float(__builtin_amdgcn_mov_dpp(b, 0x4E, 0xf, 0xf, false));
  else if constexpr (J <= 16) return __int_as_float(__builtin_amdgcn_ds_swizzle(b, 0x1F | (J << 10)));
  else return lane_xor(v, J, lane);
}

template <int K, int J>
__device__ __forceinline__ float bitonic_stages(float v, int lane) {
  // keep v where (v < o) == (lane keeps the minimum), else o: one compare
  // (into a lane mask), a scalar xnor with the stage's constant, one select;
  // equal values are interchangeable (values-only sort, no NaN, no -0)
  const float o = sort_partner<J>(v, lane);
  const uint64_t keep_v = ~(__ballot(v < o) ^ bitonic_min_lanes(K, J));
  v = mask_select(keep_v, o, v);
  if constexpr (J > 1) return bitonic_stages<K, J / 2>(v, lane);
  else return v;
}

template <int K>
__device__ __forceinline__ float bitonic_from(float v, int lane) {
  v = bitonic_stages<K, K / 2>(v, lane);
  if constexpr (K < 64) return bitonic_from<2 * K>(v, lane);
  else return v;
}

// Ascending bitonic sort of one float per lane across the wave (64 values);
// partners through lane_xor (DPP / permlane swaps, no LDS round trips), the
// min/max choice by a constant lane mask.
__device__ __forceinline__ float wave_sort64(float v, int lane) { return bitonic_from<2>(v, lane); }

}  // namespace avr
