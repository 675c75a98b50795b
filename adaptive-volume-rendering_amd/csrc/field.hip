// Radiance field: NewPixelNeRFNet.forward (models.py:739-863) fused into one
// kernel on fp32 MFMA (v_mfma_f32_16x16x4_f32, exact f32 products).
//
// Transposed formulation: every layer computes Y^T = W . X^T with the hidden
// features on the MFMA rows and 16 samples on the MFMA columns, so a layer's
// 16x16 accumulator tile (lane l: sample l&15, features 4(l>>4)+0..3) is
// already in the lane order the next layer's B operand wants:
//   k-step (t, r) uses feature 16t + 4g + r from lane group g = l>>4.
// Weights are repacked once (avr_field_pack, field_pack.hip) into that fragment order,
// [t][ot][lane] float4 = W[16ot + (l&15)][16t + 4(l>>4) + 0..3], so each lane
// streams 16 B per 4 MFMAs with fully coalesced 1 KiB wave loads.
//
// One wave = 16 samples; a lane keeps the residual stream h and the block
// temporary t for its 16x(d_hidden) slice in registers (2 x d_hidden/4 VGPRs),
// and a 1 KiB-per-tile LDS slab (per wave, no cross-wave traffic, no barriers)
// turns an accumulator tile into the next layer's B operand with one
// ds_write_b128 / ds_read_b128 per tile.
//
// lin_z is applied to the latent map per texel (avr_field_latent_table) and
// bilinearly interpolated per sample; every bias (b_in + bz0, b1 + bz_{b+1},
// ...) is pre-summed at pack time.
//
// This file: the fp32 MFMA field kernel, the per-texel latent tables, and the C entry points of the field's
// forward and backward passes in both precisions (the x3 kernels are in field_x3.hip / field_bwd.hip, the
// blob layouts and the pack in field_pack.hip).
#include "field_common.h"

namespace avr {

// ----------------------------------------------------------------- fp32 MFMA tiles
// acc[ot] += sum_t sum_r A(ot,t,r) B(t,r); A from packed global [t][ot][lane]
// through a P-deep register ring that runs ahead across t iterations, B from
// the wave's LDS slab [t][lane].
// NTOT: output tiles per K tile in the packed layout (NT < NTOT: this call
// computes the NT tiles starting at W, a slice of them)
template <int NT, int P, int NTOT = NT>
__device__ __forceinline__ void gemm_tiles(floatx4 (&acc)[NT], const floatx4* __restrict__ W, int KT,
                                           const floatx4* slab, int lane) {
  static_assert(NT % P == 0 && P % 2 == 0, "ring must divide the tile count");
  const floatx4* wl = W + lane;
  floatx4 ring[P];
#pragma unroll
  for (int p = 0; p < P; ++p) ring[p] = wl[p * 64];
  for (int t = 0; t < KT; ++t) {
    const floatx4 bv = slab[t * 64 + lane];
    const floatx4* cur = wl + (int64_t)t * NTOT * 64;
    const floatx4* nxt = wl + (int64_t)(t + 1 < KT ? t + 1 : t) * NTOT * 64;
#pragma unroll
    for (int ot = 0; ot < NT; ot += 2) {
      const floatx4 a0 = ring[ot % P];
      const floatx4 a1 = ring[(ot + 1) % P];
      ring[ot % P] = (ot + P < NT) ? cur[(ot + P) * 64] : nxt[(ot + P - NT) * 64];
      ring[(ot + 1) % P] = (ot + 1 + P < NT) ? cur[(ot + 1 + P) * 64] : nxt[(ot + 1 + P - NT) * 64];
      acc[ot] = mfma4(a0.x, bv.x, acc[ot]);
      acc[ot + 1] = mfma4(a1.x, bv.x, acc[ot + 1]);
      acc[ot] = mfma4(a0.y, bv.y, acc[ot]);
      acc[ot + 1] = mfma4(a1.y, bv.y, acc[ot + 1]);
      acc[ot] = mfma4(a0.z, bv.z, acc[ot]);
      acc[ot + 1] = mfma4(a1.z, bv.z, acc[ot + 1]);
      acc[ot] = mfma4(a0.w, bv.w, acc[ot]);
      acc[ot + 1] = mfma4(a1.w, bv.w, acc[ot + 1]);
    }
  }
}

template <int NT>
__device__ __forceinline__ void load_bias(floatx4 (&acc)[NT], const float* __restrict__ bias, int g) {
#pragma unroll
  for (int ot = 0; ot < NT; ++ot) acc[ot] = *reinterpret_cast<const floatx4*>(bias + 16 * ot + 4 * g);
}

template <int NT>
__device__ __forceinline__ void add_bias(floatx4 (&acc)[NT], const float* __restrict__ bias, int g) {
#pragma unroll
  for (int ot = 0; ot < NT; ++ot) acc[ot] += *reinterpret_cast<const floatx4*>(bias + 16 * ot + 4 * g);
}

// acc += sum_c w_c * Z[texel_c][features of this lane]
template <int NT>
__device__ __forceinline__ void add_interp(floatx4 (&acc)[NT], const float* __restrict__ Z, const Bilinear& bl,
                                           int g) {
  constexpr int CH = NT < 8 ? NT : 8;
#pragma unroll
  for (int o0 = 0; o0 < NT; o0 += CH) {
    floatx4 v[CH][4];
#pragma unroll
    for (int k = 0; k < CH; ++k)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        v[k][c] = *reinterpret_cast<const floatx4*>(Z + (int64_t)bl.tex[c] * (NT * 16) + 16 * (o0 + k) + 4 * g);
#pragma unroll
    for (int k = 0; k < CH; ++k)
      acc[o0 + k] += ((bl.w[0] * v[k][0] + bl.w[1] * v[k][1]) + bl.w[2] * v[k][2]) + bl.w[3] * v[k][3];
  }
}

template <int NT>
__device__ __forceinline__ void store_relu(floatx4* slab, const floatx4 (&acc)[NT], int lane) {
#pragma unroll
  for (int ot = 0; ot < NT; ++ot) {
    floatx4 v = acc[ot];
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    slab[ot * 64 + lane] = v;
  }
}

// CNT (avr_field_fwd_points_counted): launched over a.M = capacity rows, the row count M read from a.count on the
// device by a wave-uniform load; a workgroup whose first row is at or beyond it leaves before anything else, the
// last live one clamps and guards its tail rows against it as the uncounted kernel does against a.M.
template <int NT, bool CNT = false>
__global__ void __launch_bounds__(256, 1) field_fwd_kernel(FieldArgs a) {
  int64_t M = a.M;
  if constexpr (CNT) {
    M = counted_rows(a);
    if ((int64_t)blockIdx.x * (kFieldWaves * kSPW) >= M) return;
  }
  extern __shared__ floatx4 lds[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  floatx4* slab = lds + (size_t)wid * (NT > kInTiles ? NT : kInTiles) * 64;
  const int64_t m = ((int64_t)blockIdx.x * kFieldWaves + wid) * kSPW + j;
  const bool valid = m < M;
  const int64_t mm = valid ? m : M - 1;

  // ---- sample geometry, z_feature (features 16t + 4g + r of this lane's sample -> slab[t][lane])
  const SampleGeom sg = sample_geom(a, mm);
#pragma unroll
  for (int t = 0; t < kInTiles; ++t) {
    float f[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) f[r] = z_feature(sg, 16 * t + 4 * g + r, a.num_freqs, a.freq_factor);
    slab[t * 64 + lane] = floatx4{f[0], f[1], f[2], f[3]};
  }
  const Bilinear& bl = sg.bl;

  const floatx4* P4 = reinterpret_cast<const floatx4*>(a.packed);
  floatx4 h[NT], tt[NT];
  constexpr int P = NT >= 16 ? 16 : NT;

  // ---- lin_in (+ lin_z[0] + both biases)
  load_bias<NT>(h, a.packed + a.L.b_in, g);
  if (a.n_lin_z > 0) add_interp<NT>(h, a.table, bl, g);
  gemm_tiles<NT, P>(h, P4 + a.L.w_in / 4, kInTiles, slab, lane);

  // ---- ResnetBlockFC x n_blocks
  for (int b = 0; b < a.n_blocks; ++b) {
    store_relu<NT>(slab, h, lane);
    load_bias<NT>(tt, a.packed + a.L.b_fc0[b], g);
    gemm_tiles<NT, P>(tt, P4 + a.L.fc0[b] / 4, NT, slab, lane);
    store_relu<NT>(slab, tt, lane);
    add_bias<NT>(h, a.packed + a.L.b_fc1[b], g);
    if (b + 1 < a.n_lin_z) add_interp<NT>(h, a.table + (b + 1) * a.table_stride, bl, g);
    gemm_tiles<NT, P>(h, P4 + a.L.fc1[b] / 4, NT, slab, lane);
  }

  // ---- lin_out(relu(h)) -> (sigmoid rgb, relu sigma)
  store_relu<NT>(slab, h, lane);
  floatx4 o0 = *reinterpret_cast<const floatx4*>(a.packed + a.L.b_out + 4 * g);
  floatx4 o1 = {0.f, 0.f, 0.f, 0.f};
  const floatx4* wo = P4 + a.L.w_out / 4 + lane;
#pragma unroll 4
  for (int t = 0; t < NT; t += 2) {
    const floatx4 A0 = wo[t * 64], A1 = wo[(t + 1) * 64];
    const floatx4 B0 = slab[t * 64 + lane], B1 = slab[(t + 1) * 64 + lane];
    o0 = mfma4(A0.x, B0.x, o0); o1 = mfma4(A1.x, B1.x, o1);
    o0 = mfma4(A0.y, B0.y, o0); o1 = mfma4(A1.y, B1.y, o1);
    o0 = mfma4(A0.z, B0.z, o0); o1 = mfma4(A1.z, B1.z, o1);
    o0 = mfma4(A0.w, B0.w, o0); o1 = mfma4(A1.w, B1.w, o1);
  }
  const floatx4 o = o0 + o1;
  if (g == 0 && valid) a.out[m] = make_float4(sigmoidf_(o.x), sigmoidf_(o.y), sigmoidf_(o.z), fmaxf(o.w, 0.f));
}

// Table t's weights: lin_z[t], then (use_spade) scale_z[t - n_lin_z].
__device__ __forceinline__ int64_t table_weights(const Layout& L, int t) {
  return t < L.n_lin_z ? L.lin_z[t] : L.scale_z[t - L.n_lin_z];
}

// table[b][texel][f] = sum_c Wz_b[f][c] latent[c][texel]  (16 texels per wave)
// (+ the table's bias with use_spade)
template <int NT>
__global__ void __launch_bounds__(256, 1) latent_table_kernel(const float* __restrict__ packed, Layout L,
                                                              const float* __restrict__ latent, int HW,
                                                              float* __restrict__ table) {
  extern __shared__ floatx4 lds[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int b = blockIdx.y;
  floatx4* slab = lds + (size_t)wid * L.KTl * 64;
  const int64_t texel = ((int64_t)blockIdx.x * kFieldWaves + wid) * kSPW + j;
  const bool valid = texel < HW;
  const int64_t tx = valid ? texel : HW - 1;
  for (int t = 0; t < L.KTl; ++t) {
    const int c0 = 16 * t + 4 * g;
    slab[t * 64 + lane] = floatx4{latent[(int64_t)c0 * HW + tx], latent[(int64_t)(c0 + 1) * HW + tx],
                                  latent[(int64_t)(c0 + 2) * HW + tx], latent[(int64_t)(c0 + 3) * HW + tx]};
  }
  floatx4 acc[NT];
#pragma unroll
  for (int ot = 0; ot < NT; ++ot) acc[ot] = floatx4{0.f, 0.f, 0.f, 0.f};
  constexpr int P = NT >= 16 ? 16 : NT;
  gemm_tiles<NT, P>(acc, reinterpret_cast<const floatx4*>(packed + table_weights(L, b)), L.KTl, slab, lane);
  if (L.spade) {
#pragma unroll
    for (int ot = 0; ot < NT; ++ot) acc[ot] += *reinterpret_cast<const floatx4*>(packed + L.b_tab[b] + 16 * ot + 4 * g);
  }
  if (valid) {
    float* dst = table + ((int64_t)b * HW + texel) * (NT * 16) + 4 * g;
#pragma unroll
    for (int ot = 0; ot < NT; ++ot) *reinterpret_cast<floatx4*>(dst + 16 * ot) = acc[ot];
  }
}

// The same table with the output tiles split over the workgroup's waves
// (NT >= 8): a workgroup owns 16 texels, their latent columns are staged in
// LDS once (32 KB at d_latent 512) and wave w computes output tiles
// [w NT/4, (w+1) NT/4). Four times the workgroups of latent_table_kernel at a
// quarter of the LDS each, so a 4096-texel table fills the chip.
template <int NT>
__global__ void __launch_bounds__(256) latent_table_split_kernel(const float* __restrict__ packed, Layout L,
                                                                 const float* __restrict__ latent, int HW,
                                                                 float* __restrict__ table) {
  constexpr int NWT = NT / kFieldWaves;          // output tiles per wave
  constexpr int P = NWT >= 16 ? 16 : NWT;
  extern __shared__ floatx4 lds[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int b = blockIdx.y;
  const int64_t texel = (int64_t)blockIdx.x * kSPW + j;
  const bool valid = texel < HW;
  const int64_t tx = valid ? texel : HW - 1;
  for (int t = wid; t < L.KTl; t += kFieldWaves) {
    const int c0 = 16 * t + 4 * g;
    lds[t * 64 + lane] = floatx4{latent[(int64_t)c0 * HW + tx], latent[(int64_t)(c0 + 1) * HW + tx],
                                 latent[(int64_t)(c0 + 2) * HW + tx], latent[(int64_t)(c0 + 3) * HW + tx]};
  }
  __syncthreads();
  floatx4 acc[NWT];
#pragma unroll
  for (int ot = 0; ot < NWT; ++ot) acc[ot] = floatx4{0.f, 0.f, 0.f, 0.f};
  gemm_tiles<NWT, P, NT>(acc, reinterpret_cast<const floatx4*>(packed + table_weights(L, b)) + NWT * wid * 64, L.KTl,
                         lds, lane);
  if (L.spade) {
#pragma unroll
    for (int ot = 0; ot < NWT; ++ot)
      acc[ot] += *reinterpret_cast<const floatx4*>(packed + L.b_tab[b] + 16 * (NWT * wid + ot) + 4 * g);
  }
  if (valid) {
    float* dst = table + ((int64_t)b * HW + texel) * (NT * 16) + 16 * NWT * wid + 4 * g;
#pragma unroll
    for (int ot = 0; ot < NWT; ++ot) *reinterpret_cast<floatx4*>(dst + 16 * ot) = acc[ot];
  }
}

// ----------------------------------------------------------------- host side
// d_hidden -> NT = d_hidden / 16 output tiles of the fp32 kernels: f(NT) is called with an integral constant
template <typename F>
static int fp32_width(int d_hidden, F f) {
  using std::integral_constant;
  switch (d_hidden) {
    case 64: return f(integral_constant<int, 4>{});
    case 128: return f(integral_constant<int, 8>{});
    case 256: return f(integral_constant<int, 16>{});
    case 512: return f(integral_constant<int, 32>{});
  }
  return fail(AVR_E_UNSUPPORTED, "field: d_hidden %d", d_hidden);
}

template <int NT, bool CNT = false>
static int launch_field(const FieldArgs& a, hipStream_t s) {
  const size_t shm = (size_t)kFieldWaves * (NT > kInTiles ? NT : kInTiles) * 64 * sizeof(floatx4);
  const int64_t per_block = kFieldWaves * kSPW;
  return launch_lds<field_fwd_kernel<NT, CNT>>("field_fwd_kernel", "field: too many points",
                                               (a.M + per_block - 1) / per_block, 1, 1, 64 * kFieldWaves, shm, shm, s,
                                               a);
}

// (the dynamic-LDS limit is set per call on purpose: it depends on d_latent, which can grow between calls)
template <int NT>
static int launch_table(const float* packed, const Layout& L, const float* latent, int HW, int n_lin_z,
                        float* table, hipStream_t s) {
  if constexpr (NT >= 8) {
    const size_t shm = (size_t)L.KTl * 64 * sizeof(floatx4);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&latent_table_split_kernel<NT>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess)
      return fail(AVR_E_HIP, "latent_table_split_kernel: cannot set dynamic LDS to %zu", shm);
    dim3 grid((HW + kSPW - 1) / kSPW, n_lin_z);
    latent_table_split_kernel<NT><<<grid, 64 * kFieldWaves, shm, s>>>(packed, L, latent, HW, table);
    return check_launch("latent_table_split_kernel");
  }
  const size_t shm = (size_t)kFieldWaves * L.KTl * 64 * sizeof(floatx4);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&latent_table_kernel<NT>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm) != hipSuccess)
    return fail(AVR_E_HIP, "latent_table_kernel: cannot set dynamic LDS to %zu", shm);
  const int per_block = kFieldWaves * kSPW;
  dim3 grid((HW + per_block - 1) / per_block, n_lin_z);
  latent_table_kernel<NT><<<grid, 64 * kFieldWaves, shm, s>>>(packed, L, latent, HW, table);
  return check_launch("latent_table_kernel");
}

static int field_common(const avr_field_dims* dims, const avr_view_desc* view, const float* packed,
                        const float* table, FieldArgs* a) {
  Layout L;
  int rc = field_layout(dims, &L);
  if (rc) return rc;
  AVR_REQUIRE(view && packed, "field: null view/packed");
  AVR_REQUIRE(dims->n_lin_z == 0 || table, "field: null latent table");
  AVR_REQUIRE(view->latent_h > 0 && view->latent_w > 0, "field: bad latent size");
  a->packed = packed;
  a->table = table;
  a->table_stride = (int64_t)view->latent_h * view->latent_w * dims->d_hidden;
  a->L = L;
  view_from_desc(view, &a->v);
  a->n_blocks = dims->n_blocks;
  a->n_lin_z = dims->n_lin_z;
  a->num_freqs = dims->num_freqs;
  a->freq_factor = dims->freq_factor;
  a->beta = dims->beta;
  a->b_begin = 0;
  a->b_end = dims->n_blocks;
  a->h_out = nullptr;
  a->h_in = nullptr;
  return AVR_OK;
}

// AVR_FIELD_FP16 reads the x3 fragments' hi halves: a blob packed for AVR_FIELD_X3 or AVR_FIELD_FP16 (the two
// pack the same bytes and are recorded alike), never an fp32 one of another layout.
static int fp16_blob_ok(const FieldArgs& a) {
  AVR_REQUIRE(packed_precision(a.packed) != AVR_FIELD_FP32,
              "field: the blob was packed for AVR_FIELD_FP32: pack it with AVR_FIELD_X3 or AVR_FIELD_FP16 to run "
              "the fp16 kernel");
  return AVR_OK;
}

static int dispatch_field(const avr_field_dims* dims, const FieldArgs& a, hipStream_t s) {
  const int d_hidden = dims->d_hidden;
  if (dims->precision == AVR_FIELD_X3) return dispatch_field_x3(d_hidden, a, s);
  if (dims->precision == AVR_FIELD_FP16) {
    if (int rc = fp16_blob_ok(a)) return rc;
    return dispatch_field_fp16(d_hidden, a, s);
  }
  AVR_REQUIRE(packed_precision(a.packed) != AVR_FIELD_X3,
              "field: the blob was packed for AVR_FIELD_X3 (no fp32 lin_in / fc_0 / fc_1 fragments): pack it with "
              "AVR_FIELD_FP32 to run the fp32 kernel");
  AVR_REQUIRE(!dims->bn, "field: BatchNorm nets run on the x3 path only");
  AVR_REQUIRE(!dims->spade && !(dims->beta > 0.f), "field: use_spade / Softplus nets run on the x3 path only");
  AVR_REQUIRE(dims->precision == AVR_FIELD_FP32, "field: unknown precision %d", dims->precision);
  return fp32_width(d_hidden, [&](auto nt) { return launch_field<decltype(nt)::value>(a, s); });
}

// The counted launch (avr_field_fwd_points_counted; a.count set): ReLU nets without BatchNorm / use_spade, either
// precision.
static int dispatch_field_counted(const avr_field_dims* dims, const FieldArgs& a, hipStream_t s) {
  if (dims->bn || dims->spade || dims->beta > 0.f)
    return fail(AVR_E_UNSUPPORTED, "avr_field_fwd_points_counted: BatchNorm, use_spade and Softplus nets have no "
                                   "counted kernel");
  if (dims->precision == AVR_FIELD_X3) return dispatch_field_x3_counted(dims->d_hidden, a, s);
  if (dims->precision == AVR_FIELD_FP16) {
    if (int rc = fp16_blob_ok(a)) return rc;
    return dispatch_field_fp16(dims->d_hidden, a, s);
  }
  AVR_REQUIRE(packed_precision(a.packed) != AVR_FIELD_X3,
              "field: the blob was packed for AVR_FIELD_X3 (no fp32 lin_in / fc_0 / fc_1 fragments): pack it with "
              "AVR_FIELD_FP32 to run the fp32 kernel");
  AVR_REQUIRE(dims->precision == AVR_FIELD_FP32, "field: unknown precision %d", dims->precision);
  return fp32_width(dims->d_hidden, [&](auto nt) { return launch_field<decltype(nt)::value, true>(a, s); });
}

}  // namespace avr

using namespace avr;

#ifdef AVR_STAMPS
static unsigned long long* g_stamps = nullptr;
extern "C" void avr_debug_set_stamps(void* p) { g_stamps = reinterpret_cast<unsigned long long*>(p); }
static int g_debug = 0;
extern "C" void avr_debug_set_flags(int f) { g_debug = f; }
#endif

// Several scenes in one launch (x3 path): scene s's samples are rows s * per_scene .. of the inputs, its lin_z
// tables at tables + s * max(n_tables, 1) * H*W * d_hidden (FusedField.tables_batch), its view views[s].
static int field_batch(const avr_field_dims* dims, const avr_view_desc* views, int n_scenes, const float* packed,
                       const float* tables, FieldArgs* a, int64_t per_scene, const char* what,
                       bool fp16_too = false) {
  AVR_REQUIRE(views && n_scenes >= 1 && n_scenes <= AVR_MAX_SCENES, "%s: 1..%d scenes per call", what,
              AVR_MAX_SCENES);
  AVR_REQUIRE(dims && (dims->precision == AVR_FIELD_X3 || (fp16_too && dims->precision == AVR_FIELD_FP16)),
              "%s: the multi-scene launch is %s", what, fp16_too ? "x3 or fp16" : "x3 only");
  int rc = field_common(dims, views, packed, tables, a);
  if (rc) return rc;
  for (int s = 0; s < n_scenes; ++s) {
    AVR_REQUIRE(views[s].latent_h == views[0].latent_h && views[s].latent_w == views[0].latent_w,
                "%s: scenes need latent maps of one size", what);
    view_from_desc(&views[s], &a->views[s]);
  }
  a->M = per_scene;
  a->n_scenes = n_scenes;
  a->blocks_per_scene = (per_scene + kX3Samples - 1) / kX3Samples;
  a->table_scene_stride = (int64_t)(a->L.n_tables > 0 ? a->L.n_tables : 1) * a->table_stride;
  return AVR_OK;
}

extern "C" int avr_field_fwd_points_train(const avr_field_dims* dims, const avr_view_desc* views, int n_scenes,
                                          const float* packed, const float* tables, const float* xyz,
                                          const float* viewdirs, int64_t n_points, float* out, float* act,
                                          int64_t act_rows, uint32_t* mask, uint32_t* act_max, float* z_feature,
                                          int ld_z, uint32_t* z_max, void* stream) {
  FieldArgs a{};
  int rc = field_batch(dims, views, n_scenes, packed, tables, &a, n_points, "avr_field_fwd_points_train");
  if (rc) return rc;
  AVR_REQUIRE(!dims->bn && !dims->spade,
              "avr_field_fwd_points_train: BatchNorm nets train on avr_bn_layer_run, use_spade nets on the module path");
  AVR_REQUIRE(n_points >= 0, "avr_field_fwd_points_train: bad size");
  AVR_REQUIRE(n_points == 0 || (xyz && viewdirs && out && act && mask), "avr_field_fwd_points_train: null pointer");
  AVR_REQUIRE(act_rows >= n_scenes * n_points, "avr_field_fwd_points_train: act_rows < n_scenes * n_points");
  a.xyz = xyz; a.vd = viewdirs; a.n_samples = 1;
  a.out = reinterpret_cast<float4*>(out);
  a.act = act;
  a.act_stride = act_rows * dims->d_hidden;
  a.mask = mask;
  a.act_max = act_max;
  AVR_REQUIRE(!z_feature || ld_z >= dims->d_in, "avr_field_fwd_points_train: ld_z %d < d_in %d", ld_z, dims->d_in);
  a.zf = z_feature;
  a.zf_ld = ld_z;
  a.zf_max = z_max;
  if (a.M == 0) return AVR_OK;
  return dispatch_field_x3(dims->d_hidden, a, as_stream(stream));
}

extern "C" int avr_field_bwd(const avr_field_dims* dims, const float* packed, const float* packed_bwd, int n_scenes,
                             int64_t n_points, const float* out, const float* grad_out, const uint32_t* mask,
                             const float* act, int64_t act_rows, float* grads, int64_t grads_rows,
                             uint32_t* grads_max, void* stream) {
  BwdArgs a{};
  int rc = field_layout(dims, &a.L);
  if (rc) return rc;
  AVR_REQUIRE(dims->precision == AVR_FIELD_X3, "avr_field_bwd: the training path is x3 only");
  AVR_REQUIRE(!dims->bn && !dims->spade,
              "avr_field_bwd: BatchNorm nets train on avr_bn_layer_run, use_spade nets on the module path");
  AVR_REQUIRE(!(dims->beta > 0.f) || (act && act_rows >= (int64_t)n_scenes * n_points),
              "avr_field_bwd: Softplus nets need the forward's act rows (act_rows >= n_scenes * n_points)");
  a.act = act;
  a.act_stride = act_rows * dims->d_hidden;
  a.beta = dims->beta;
  AVR_REQUIRE(n_points >= 0 && n_scenes >= 1, "avr_field_bwd: bad size");
  if (n_points == 0) return AVR_OK;
  AVR_REQUIRE(packed && packed_bwd && out && grad_out && mask && grads, "avr_field_bwd: null pointer");
  AVR_REQUIRE(grads_rows >= n_scenes * n_points, "avr_field_bwd: grads_rows < n_scenes * n_points");
  if ((rc = field_bwd_layout(dims, &a.LB))) return rc;
  a.packed = packed;
  a.packed_bwd = packed_bwd;
  a.n_blocks = dims->n_blocks;
  a.M = n_points;
  a.n_scenes = n_scenes;
  a.blocks_per_scene = (n_points + kX3Samples - 1) / kX3Samples;
  a.out = reinterpret_cast<const float4*>(out);
  a.grad_out = reinterpret_cast<const float4*>(grad_out);
  a.mask = mask;
  a.G = grads;
  a.g_stride = grads_rows * dims->d_hidden;
  a.g_max = grads_max;
  return dispatch_field_bwd_x3(dims->d_hidden, a, as_stream(stream));
}

extern "C" int avr_field_latent_table(const avr_field_dims* dims, const float* packed, const float* latent, int H,
                                      int W, float* table, void* stream) {
  Layout L;
  int rc = field_layout(dims, &L);
  if (rc) return rc;
  AVR_REQUIRE(packed && latent && table, "avr_field_latent_table: null pointer");
  AVR_REQUIRE(H > 0 && W > 0, "avr_field_latent_table: bad latent size");
  if (L.n_tables == 0) return AVR_OK;
  hipStream_t s = as_stream(stream);
  // AVR_FIELD_X3: tables on the split-fp16 GEMM (the training path, which recomputes them every step);
  // AVR_FIELD_FP32: exact fp32 products (inference: computed once per latent map)
  if (dims->precision == AVR_FIELD_X3 && L.x3_tables)
    return dispatch_table_x3(packed, L, latent, H * W, dims->d_latent, dims->d_hidden, table, 1, s);
  return fp32_width(dims->d_hidden, [&](auto nt) {
    return launch_table<decltype(nt)::value>(packed, L, latent, H * W, L.n_tables, table, s);
  });
}

extern "C" int avr_field_latent_table_batch(const avr_field_dims* dims, const float* packed, const float* latent,
                                            int n_scenes, int H, int W, float* table, void* stream) {
  Layout L;
  int rc = field_layout(dims, &L);
  if (rc) return rc;
  AVR_REQUIRE(n_scenes >= 1, "avr_field_latent_table_batch: n_scenes must be >= 1");
  AVR_REQUIRE(packed && latent && table, "avr_field_latent_table_batch: null pointer");
  AVR_REQUIRE(H > 0 && W > 0, "avr_field_latent_table_batch: bad latent size");
  if (L.n_tables == 0) return AVR_OK;
  if (dims->precision == AVR_FIELD_X3 && L.x3_tables)
    return dispatch_table_x3(packed, L, latent, H * W, dims->d_latent, dims->d_hidden, table, n_scenes,
                             as_stream(stream));
  const int64_t lat_stride = (int64_t)dims->d_latent * H * W, tab_stride = (int64_t)L.n_tables * H * W * dims->d_hidden;
  for (int sc = 0; sc < n_scenes; ++sc)
    if ((rc = avr_field_latent_table(dims, packed, latent + sc * lat_stride, H, W, table + sc * tab_stride, stream)))
      return rc;
  return AVR_OK;
}

extern "C" int avr_field_fwd_rays(const avr_field_dims* dims, const avr_view_desc* view, const float* packed,
                                  const float* table, const float* ro, const float* rd, const float* z,
                                  int64_t n_rays, int n_samples, float* out, void* stream) {
  FieldArgs a{};
  int rc = field_common(dims, view, packed, table, &a);
  if (rc) return rc;
  AVR_REQUIRE(n_rays >= 0 && n_samples > 0, "avr_field_fwd_rays: bad sizes");
  AVR_REQUIRE(n_rays == 0 || (ro && rd && z && out), "avr_field_fwd_rays: null pointer");
  a.ro = ro; a.rd = rd; a.z = z; a.n_samples = n_samples;
#ifdef AVR_STAMPS
  a.stamps = g_stamps;
  a.debug = g_debug;
#endif
  a.M = n_rays * n_samples;
  a.out = reinterpret_cast<float4*>(out);
  if (a.M == 0) return AVR_OK;
  return dispatch_field(dims, a, as_stream(stream));
}

extern "C" int avr_field_fwd_rays_batch(const avr_field_dims* dims, const avr_view_desc* views, int n_scenes,
                                        const float* packed, const float* tables, const float* ro, const float* rd,
                                        const float* z, int64_t n_rays, int n_samples, float* out, void* stream) {
  FieldArgs a{};
  AVR_REQUIRE(n_rays >= 0 && n_samples > 0, "avr_field_fwd_rays_batch: bad sizes");
  int rc = field_batch(dims, views, n_scenes, packed, tables, &a, n_rays * n_samples, "avr_field_fwd_rays_batch",
                       true);
  if (rc) return rc;
  AVR_REQUIRE(n_rays == 0 || (ro && rd && z && out), "avr_field_fwd_rays_batch: null pointer");
  a.ro = ro; a.rd = rd; a.z = z; a.n_samples = n_samples;
  a.out = reinterpret_cast<float4*>(out);
  if (a.M == 0) return AVR_OK;
  return dispatch_field(dims, a, as_stream(stream));
}

extern "C" int avr_field_fwd_points_batch(const avr_field_dims* dims, const avr_view_desc* views, int n_scenes,
                                          const float* packed, const float* tables, const float* xyz,
                                          const float* viewdirs, int64_t n_points, float* out, void* stream) {
  FieldArgs a{};
  AVR_REQUIRE(n_points >= 0, "avr_field_fwd_points_batch: bad size");
  int rc = field_batch(dims, views, n_scenes, packed, tables, &a, n_points, "avr_field_fwd_points_batch", true);
  if (rc) return rc;
  AVR_REQUIRE(n_points == 0 || (xyz && viewdirs && out), "avr_field_fwd_points_batch: null pointer");
  a.xyz = xyz; a.vd = viewdirs; a.n_samples = 1;
  a.out = reinterpret_cast<float4*>(out);
  if (a.M == 0) return AVR_OK;
  return dispatch_field(dims, a, as_stream(stream));
}

extern "C" int avr_field_fwd_points_split(const avr_field_dims* dims, const avr_view_desc* views, int n_scenes,
                                          const float* packed, const float* tables, const float* xyz,
                                          const float* viewdirs, int64_t n_points, int b_begin, int b_end,
                                          const float* h_in, float* h_out, float* out, void* stream) {
  FieldArgs a{};
  if (dims && dims->precision == AVR_FIELD_FP16)
    return fail(AVR_E_UNSUPPORTED, "avr_field_fwd_points_split: AVR_FIELD_FP16 has no split (NS > 1) launch");
  AVR_REQUIRE(n_points >= 0, "avr_field_fwd_points_split: bad size");
  int rc = field_batch(dims, views, n_scenes, packed, tables, &a, n_points, "avr_field_fwd_points_split");
  if (rc) return rc;
  const bool first = b_begin == 0;
  if (first) {
    AVR_REQUIRE(b_end > 0 && b_end < dims->n_blocks && b_end >= dims->n_lin_z,
                "avr_field_fwd_points_split: first launch needs n_lin_z <= b_end < n_blocks (got %d)", b_end);
    AVR_REQUIRE(n_points == 0 || (xyz && viewdirs && h_out), "avr_field_fwd_points_split: null pointer");
  } else {
    AVR_REQUIRE(b_begin >= dims->n_lin_z && b_begin < dims->n_blocks && b_end == dims->n_blocks,
                "avr_field_fwd_points_split: second launch needs n_lin_z <= b_begin < b_end == n_blocks");
    AVR_REQUIRE(n_points == 0 || (h_in && out), "avr_field_fwd_points_split: null pointer");
  }
  a.xyz = xyz; a.vd = viewdirs; a.n_samples = 1;
  a.b_begin = b_begin;
  a.b_end = b_end;
  a.h_in = first ? nullptr : h_in;
  a.h_out = first ? h_out : nullptr;
  a.out = reinterpret_cast<float4*>(out);
  if (a.M == 0) return AVR_OK;
  return dispatch_field_x3(dims->d_hidden, a, as_stream(stream));
}

extern "C" int avr_field_fwd_points(const avr_field_dims* dims, const avr_view_desc* view, const float* packed,
                                    const float* table, const float* xyz, const float* viewdirs, int64_t n_points,
                                    float* out, void* stream) {
  FieldArgs a{};
  int rc = field_common(dims, view, packed, table, &a);
  if (rc) return rc;
  AVR_REQUIRE(n_points >= 0, "avr_field_fwd_points: bad size");
  AVR_REQUIRE(n_points == 0 || (xyz && viewdirs && out), "avr_field_fwd_points: null pointer");
  a.xyz = xyz; a.vd = viewdirs; a.n_samples = 1;
  a.M = n_points;
  a.out = reinterpret_cast<float4*>(out);
  if (a.M == 0) return AVR_OK;
  return dispatch_field(dims, a, as_stream(stream));
}

// avr_field_fwd_points over `capacity` rows with the row count read from device memory (include/avr.h).
extern "C" int avr_field_fwd_points_counted(const avr_field_dims* dims, const avr_view_desc* view, const float* packed,
                                            const float* table, const float* xyz, const float* viewdirs,
                                            int64_t capacity, const int64_t* n_points, float* out, void* stream) {
  FieldArgs a{};
  int rc = field_common(dims, view, packed, table, &a);
  if (rc) return rc;
  AVR_REQUIRE(capacity >= 0, "avr_field_fwd_points_counted: negative capacity");
  AVR_REQUIRE(capacity == 0 || (xyz && viewdirs && out && n_points), "avr_field_fwd_points_counted: null pointer");
  AVR_REQUIRE((((uintptr_t)out) & 15) == 0 && (((uintptr_t)n_points) & 7) == 0,
              "avr_field_fwd_points_counted: out rows must be 16-B aligned, n_points 8-B aligned");
  a.xyz = xyz; a.vd = viewdirs; a.n_samples = 1;
  a.M = capacity;
  a.count = n_points;
  a.out = reinterpret_cast<float4*>(out);
  if (a.M == 0) return AVR_OK;
  return dispatch_field_counted(dims, a, as_stream(stream));
}
