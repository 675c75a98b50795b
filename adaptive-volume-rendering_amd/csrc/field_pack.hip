// The radiance field's packed blobs: their layouts (Layout: the forward blob of avr_field_pack, read by the fp32
// kernels of field.hip and the x3 kernels of field_x3.hip / bn_train.hip; BwdLayout: the transposed x3 fragments
// of avr_field_pack_bwd), the kernels that fill them, and the size queries.
#include <mutex>

#include "field_common.h"

namespace avr {

// ----------------------------------------------------------------- layout
int field_layout(const avr_field_dims* d, Layout* L) {
  AVR_REQUIRE(d, "field: null dims");
  AVR_REQUIRE(d->d_hidden == 64 || d->d_hidden == 128 || d->d_hidden == 256 || d->d_hidden == 512,
              "field: d_hidden must be 64/128/256/512 (got %d)", d->d_hidden);
  AVR_REQUIRE(d->d_latent > 0 && d->d_latent % 16 == 0 && d->d_latent <= 1024,
              "field: d_latent must be a positive multiple of 16 <= 1024 (got %d)", d->d_latent);
  AVR_REQUIRE(d->n_blocks >= 1 && d->n_blocks <= AVR_MAX_BLOCKS, "field: n_blocks must be in [1, %d]",
              AVR_MAX_BLOCKS);
  AVR_REQUIRE(d->n_lin_z >= 0 && d->n_lin_z <= d->n_blocks, "field: n_lin_z must be in [0, n_blocks]");
  AVR_REQUIRE(d->num_freqs >= 0 && 3 + 6 * d->num_freqs + 3 == d->d_in && d->d_in <= 16 * kInTiles,
              "field: d_in %d != 6*num_freqs+6 or > 48 (fused path supports PE(xyz)+raw viewdirs)", d->d_in);
  const int NT = d->d_hidden / 16, KC = d->d_hidden / 32;
  L->NT = NT;
  L->KTl = d->d_latent / 16;
  const int64_t tile = 64 * 4;  // floats per (t, ot) fp32 fragment block
  const int64_t tile16 = 64 * 8;  // floats per (c, ft) fp16 hi/lo fragment block (64 lanes x 32 B)
  int64_t o = 0;
  L->w_in = o; o += (int64_t)kInTiles * NT * tile;
  for (int b = 0; b < d->n_blocks; ++b) {
    L->fc0[b] = o; o += (int64_t)NT * NT * tile;
    L->fc1[b] = o; o += (int64_t)NT * NT * tile;
  }
  L->w_out = o; o += (int64_t)NT * tile;
  for (int b = 0; b < d->n_lin_z; ++b) { L->lin_z[b] = o; o += (int64_t)L->KTl * NT * tile; }
  L->b_in = o; o += d->d_hidden;
  for (int b = 0; b < d->n_blocks; ++b) {
    L->b_fc0[b] = o; o += d->d_hidden;
    L->b_fc1[b] = o; o += d->d_hidden;
  }
  L->b_out = o; o += 16;
  o = (o + 63) & ~(int64_t)63;
  L->x3_hdr = o; o += 64;
  L->x3_in = o; o += (int64_t)kX3InChunks * NT * tile16;
  for (int b = 0; b < d->n_blocks; ++b) {
    L->x3_fc0[b] = o; o += (int64_t)KC * NT * tile16;
    L->x3_fc1[b] = o; o += (int64_t)KC * NT * tile16;
  }
  L->x3_out = o; o += (int64_t)KC * tile16;
  AVR_REQUIRE(d->bn == 0 || d->bn == 1, "field: bn must be 0 or 1");
  L->bn = d->bn;
  for (int b = 0; b < d->n_blocks; ++b) {
    L->bn_a[b] = L->bn_c[b] = 0;
    if (d->bn) { L->bn_a[b] = o; o += d->d_hidden; L->bn_c[b] = o; o += d->d_hidden; }
  }
  AVR_REQUIRE(d->spade == 0 || d->spade == 1, "field: spade must be 0 or 1");
  AVR_REQUIRE(d->beta >= 0.f && d->beta < 1e30f, "field: beta must be >= 0 (0: ReLU)");
  AVR_REQUIRE(!(d->beta > 0.f && d->bn), "field: Softplus with BatchNorm runs on the module path");
  AVR_REQUIRE(!(d->spade && d->bn), "field: use_spade with BatchNorm runs on the module path");
  L->spade = d->spade;
  L->n_lin_z = d->n_lin_z;
  L->n_tables = d->n_lin_z * (d->spade ? 2 : 1);
  for (int b = 0; b < AVR_MAX_BLOCKS; ++b) L->scale_z[b] = 0;
  for (int t = 0; t < 2 * AVR_MAX_BLOCKS; ++t) L->b_tab[t] = 0;
  if (d->spade) {
    for (int b = 0; b < d->n_lin_z; ++b) { L->scale_z[b] = o; o += (int64_t)L->KTl * NT * tile; }
    for (int t = 0; t < L->n_tables; ++t) { L->b_tab[t] = o; o += d->d_hidden; }
  }
  L->x3_tables = d->d_latent % 64 == 0 && d->d_latent <= 512;
  for (int t = 0; t < 2 * AVR_MAX_BLOCKS; ++t) L->x3_tab[t] = 0;
  for (int t = 0; L->x3_tables && t < L->n_tables; ++t) {
    L->x3_tab[t] = o;
    o += (int64_t)(d->d_latent / 32) * NT * tile16;
  }
  L->total = o;
  return AVR_OK;
}

int field_bwd_layout(const avr_field_dims* d, BwdLayout* LB) {
  Layout L;
  const int rc = field_layout(d, &L);   // the dims' checks
  if (rc) return rc;
  const int64_t S = (int64_t)(d->d_hidden / 32) * (d->d_hidden / 16) * 64 * 8;   // floats per x3 hidden layer
  int64_t o = 64;
  for (int b = 0; b < d->n_blocks; ++b) {
    LB->fc0t[b] = o; o += S;
    LB->fc1t[b] = o; o += S;
  }
  // lin_z[b]^T (d_latent x d_hidden after the transpose: a hidden layer's shape when d_latent == d_hidden) for
  // avr_bn_layer_run's transposed products (the point gradient's sum_b Gz[b] . W_z[b])
  for (int b = 0; b < AVR_MAX_BLOCKS; ++b) {
    LB->lzt[b] = -1;
    if (b < d->n_lin_z && d->d_latent == d->d_hidden && !d->spade) { LB->lzt[b] = o; o += S; }
  }
  LB->total = o;
  return AVR_OK;
}

// ----------------------------------------------------------------- packing
// fp32 fragments: dst[(t*NTo + ot)*64 + l][r] = W[16ot + (l&15)][16t + 4(l>>4) + r] (zero padded);
// bias vectors: dst[i] = a[i] + b[i] (b may be null), zero beyond n.
// The fp32 fragments and bias vectors of a pack in two launches (blockIdx.y = job), not one launch each:
// the pack runs in every training step (the weights change).
struct LinJob {
  const float* W;
  float* dst;
  int out_dim, in_dim, NTo, KTi;
};
struct LinBatch {
  LinJob j[2 + 4 * AVR_MAX_BLOCKS];
  int count;
};
struct BiasJob {
  const float* a;
  const float* b;
  float* dst;
  int n, n_pad;
};
struct BiasBatch {
  BiasJob j[2 + 8 * AVR_MAX_BLOCKS];
  int count;
};

__global__ void pack_linear_batch_kernel(LinBatch bt) {
  const LinJob& J = bt.j[blockIdx.y];
  const int64_t n = (int64_t)J.KTi * J.NTo * 256;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i & 3);
    const int l = (int)((i >> 2) & 63);
    const int64_t blk = i >> 8;
    const int ot = (int)(blk % J.NTo), t = (int)(blk / J.NTo);
    const int row = 16 * ot + (l & 15), col = 16 * t + 4 * (l >> 4) + r;
    J.dst[i] = (row < J.out_dim && col < J.in_dim) ? J.W[(int64_t)row * J.in_dim + col] : 0.f;
  }
}

__global__ void pack_bias_batch_kernel(BiasBatch bt) {
  const BiasJob& J = bt.j[blockIdx.y];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < J.n_pad; i += gridDim.x * blockDim.x)
    J.dst[i] = (i < J.n) ? (J.b ? fadd(J.a[i], J.b[i]) : J.a[i]) : 0.f;
}


// x3 fragments: dst[((c*FTt + ft)*2 + {0, 1})*512 + 8l + e] = (hi, lo) of
// (a tile's 64 hi lanes, then its 64 lo lanes: each 16-B-per-lane load of one
// half reads 1 KiB contiguous, whole 128-B lines)
// W[16ft + (l&15)][32c + (e<4 ? 4g+e : 16+4g+e-4)] * s_w, g = l>>4, with
// s_w = 2^(14 - ceil-exponent of max|W|) from the layer's header word.
// (rs, cs) = element strides of W's rows / columns: (in_dim, 1) for W, (1, ld) for W^T.
__device__ __forceinline__ void pack_x3_elem(const float* __restrict__ W, int out_dim, int in_dim, int64_t rs,
                                             int64_t cs, int FTt, const unsigned* __restrict__ maxbits,
                                             _Float16* __restrict__ dst, int64_t i) {
  const int e = (int)(i & 7);
  const int l = (int)((i >> 3) & 63);
  const int64_t blk = i >> 9;
  const int ft = (int)(blk % FTt), c = (int)(blk / FTt);
  const int g = l >> 4;
  const int row = 16 * ft + (l & 15);
  const int col = 32 * c + (e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4));
  const float sw = pow2_scale_for(__uint_as_float(*maxbits));
  const float v = (row < out_dim && col < in_dim) ? W[(int64_t)row * rs + (int64_t)col * cs] * sw : 0.f;
  const _Float16 hi = (_Float16)v;
  const _Float16 lo = (_Float16)(v - (float)hi);
  const int64_t base = ((int64_t)c * FTt + ft) * 2 * 64 * 8 + l * 8;
  dst[base + e] = hi;
  dst[base + 64 * 8 + e] = lo;
}

// Every layer of a pack in two launches (max |W| of each layer, then its
// fragments; blockIdx.y = layer) instead of two per layer: the weight pack
// runs in every training step.
struct X3PackJob {
  const float* W;
  unsigned* maxbits;
  _Float16* dst;
  int64_t rs, cs, nw, n;
  int out_dim, in_dim, FTt;
};
struct X3PackBatch {
  X3PackJob j[kX3PackJobs];
  int count;
};

// max|W| of each layer as float bits (atomicMax on non-negative floats = on their bits)
// (one atomic per workgroup: a few dozen per layer, not one per wave)
__global__ void absmax_batch_kernel(X3PackBatch b) {
  __shared__ float wm[4];
  const X3PackJob& J = b.j[blockIdx.y];
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < J.nw; i += (int64_t)gridDim.x * blockDim.x)
    m = fmaxf(m, fabsf(J.W[i]));
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicMax(J.maxbits, __float_as_uint(fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]))));
}

__global__ void pack_x3_batch_kernel(X3PackBatch b) {
  const X3PackJob& J = b.j[blockIdx.y];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < J.n; i += (int64_t)gridDim.x * blockDim.x)
    pack_x3_elem(J.W, J.out_dim, J.in_dim, J.rs, J.cs, J.FTt, J.maxbits, J.dst, i);
}

// ----------------------------------------------------------------- pack batches
// job (reading tensor src) -> the batch's next slot
template <typename Batch, typename Job>
static int append_job(Batch& bt, const float* src, const Job& job) {
  AVR_REQUIRE(src, "avr_field_pack: null weight / bias tensor");
  AVR_REQUIRE(bt.count < (int)(sizeof(bt.j) / sizeof(bt.j[0])), "avr_field_pack: too many layers");
  bt.j[bt.count++] = job;
  return AVR_OK;
}

static int pack_linear(const float* W, int out_dim, int in_dim, int NTo, int KTi, float* dst, LinBatch& bt) {
  return append_job(bt, W, LinJob{W, dst, out_dim, in_dim, NTo, KTi});
}

// one layer into a batch (W is (out_dim, in_dim) row-major; transpose: (in_dim,
// out_dim), and the fragments hold W^T)
static int add_x3(X3PackBatch& bt, const float* W, int out_dim, int in_dim, int KC, int FTt, unsigned* maxbits,
                  float* dst, bool transpose = false) {
  X3PackJob J;
  J.W = W;
  J.maxbits = maxbits;
  J.dst = reinterpret_cast<_Float16*>(dst);
  J.rs = transpose ? 1 : in_dim;
  J.cs = transpose ? out_dim : 1;
  J.nw = (int64_t)out_dim * in_dim;
  J.n = (int64_t)KC * FTt * 64 * 8;
  J.out_dim = out_dim;
  J.in_dim = in_dim;
  J.FTt = FTt;
  return append_job(bt, W, J);
}

static int run_x3(const X3PackBatch& bt, hipStream_t s) {
  if (bt.count == 0) return AVR_OK;
  int64_t nw = 0, n = 0;
  for (int k = 0; k < bt.count; ++k) {
    nw = bt.j[k].nw > nw ? bt.j[k].nw : nw;
    n = bt.j[k].n > n ? bt.j[k].n : n;
  }
  const unsigned ga = (unsigned)((nw + 4095) / 4096 < 64 ? (nw + 4095) / 4096 : 64);   // >= 16 values per thread
  absmax_batch_kernel<<<dim3(ga, bt.count), 256, 0, s>>>(bt);
  int rc = check_launch("absmax_batch_kernel");
  if (rc) return rc;
  const unsigned gp = (unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
  pack_x3_batch_kernel<<<dim3(gp, bt.count), 256, 0, s>>>(bt);
  return check_launch("pack_x3_batch_kernel");
}

static int pack_bias(const float* a, const float* b, int n, int n_pad, float* dst, BiasBatch& bt) {
  return append_job(bt, a, BiasJob{a, b, dst, n, n_pad});
}

static int run_fp32_packs(const LinBatch& lb, const BiasBatch& bb, hipStream_t s) {
  int64_t n = 0;
  for (int k = 0; k < lb.count; ++k) {
    const int64_t nk = (int64_t)lb.j[k].KTi * lb.j[k].NTo * 256;
    n = nk > n ? nk : n;
  }
  if (lb.count) {
    pack_linear_batch_kernel<<<dim3((unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024), lb.count), 256, 0,
                               s>>>(lb);
    const int rc = check_launch("pack_linear_batch_kernel");
    if (rc) return rc;
  }
  int nb = 0;
  for (int k = 0; k < bb.count; ++k) nb = bb.j[k].n_pad > nb ? bb.j[k].n_pad : nb;
  if (bb.count == 0) return AVR_OK;
  pack_bias_batch_kernel<<<dim3((unsigned)((nb + 255) / 256), bb.count), 256, 0, s>>>(bb);
  return check_launch("pack_bias_batch_kernel");
}

// The precision each blob was packed for (avr_field_pack): an AVR_FIELD_X3 blob holds no fp32 fragments of
// lin_in / fc_0 / fc_1, so the fp32 kernel must not run on it. A small host-side table keyed by the blob's
// address (the last kPackTags packs; the device header is not read back: that would synchronise the stream).
namespace {
constexpr int kPackTags = 128;
struct PackTag {
  const float* p;
  int precision;
};
std::mutex g_pack_mu;
PackTag g_pack_tags[kPackTags] = {};
int g_pack_next = 0;

void record_pack(const float* p, int precision) {
  std::lock_guard<std::mutex> lock(g_pack_mu);
  for (PackTag& t : g_pack_tags)
    if (t.p == p) {
      t.precision = precision;
      return;
    }
  g_pack_tags[g_pack_next] = PackTag{p, precision};
  g_pack_next = (g_pack_next + 1) % kPackTags;
}

}  // namespace

int packed_precision(const float* p) {
  std::lock_guard<std::mutex> lock(g_pack_mu);
  for (const PackTag& t : g_pack_tags)
    if (t.p == p) return t.precision;
  return -1;
}


}  // namespace avr

using namespace avr;

extern "C" int avr_field_packed_floats(const avr_field_dims* dims, int64_t* n_floats) {
  Layout L;
  const int rc = field_layout(dims, &L);
  if (rc) return rc;
  AVR_REQUIRE(n_floats, "avr_field_packed_floats: null output");
  *n_floats = L.total;
  return AVR_OK;
}

extern "C" int avr_field_pack(const avr_field_dims* dims, const avr_resnetfc_weights* w, float* packed,
                              void* stream) {
  Layout L;
  int rc = field_layout(dims, &L);
  if (rc) return rc;
  AVR_REQUIRE(w && packed, "avr_field_pack: null pointer");
  hipStream_t s = as_stream(stream);
  const int H = dims->d_hidden, NT = L.NT;
  // the fp32 fragments the x3 kernels never read (lin_in, fc_0, fc_1) are packed only for an fp32 blob; the
  // lin_z / scale_z ones always (the exact-fp32 tables)
  const bool fp32 = dims->precision != AVR_FIELD_X3 && dims->precision != AVR_FIELD_FP16;
  LinBatch lb{};
  BiasBatch bb{};
  if (fp32 && (rc = pack_linear(w->lin_in_w, H, dims->d_in, NT, kInTiles, packed + L.w_in, lb))) return rc;
  if ((rc = pack_linear(w->lin_out_w, 4, H, 1, NT, packed + L.w_out, lb))) return rc;   // also the backward's
  for (int b = 0; b < dims->n_blocks; ++b) {
    if (fp32 && (rc = pack_linear(w->fc0_w[b], H, H, NT, NT, packed + L.fc0[b], lb))) return rc;
    if (fp32 && (rc = pack_linear(w->fc1_w[b], H, H, NT, NT, packed + L.fc1[b], lb))) return rc;
    if ((rc = pack_bias(w->fc0_b[b], nullptr, H, H, packed + L.b_fc0[b], bb))) return rc;
    const float* bz = (b + 1 < dims->n_lin_z && !dims->spade) ? w->lin_z_b[b + 1] : nullptr;
    if ((rc = pack_bias(w->fc1_b[b], bz, H, H, packed + L.b_fc1[b], bb))) return rc;
  }
  for (int b = 0; b < dims->n_lin_z; ++b)
    if ((rc = pack_linear(w->lin_z_w[b], H, dims->d_latent, NT, L.KTl, packed + L.lin_z[b], lb))) return rc;
  if ((rc = pack_bias(w->lin_in_b, dims->n_lin_z > 0 && !dims->spade ? w->lin_z_b[0] : nullptr, H, H,
                      packed + L.b_in, bb)))
    return rc;
  for (int b = 0; dims->spade && b < dims->n_lin_z; ++b) {
    AVR_REQUIRE(w->scale_z_w[b] && w->scale_z_b[b] && w->lin_z_b[b],
                "avr_field_pack: use_spade needs scale_z weight / bias and lin_z bias of every lin_z block");
    if ((rc = pack_linear(w->scale_z_w[b], H, dims->d_latent, NT, L.KTl, packed + L.scale_z[b], lb)))
      return rc;
    if ((rc = pack_bias(w->lin_z_b[b], nullptr, H, H, packed + L.b_tab[b], bb))) return rc;
    if ((rc = pack_bias(w->scale_z_b[b], nullptr, H, H, packed + L.b_tab[dims->n_lin_z + b], bb))) return rc;
  }
  if ((rc = pack_bias(w->lin_out_b, nullptr, 4, 16, packed + L.b_out, bb))) return rc;
  for (int b = 0; dims->bn && b < dims->n_blocks; ++b) {
    AVR_REQUIRE(w->bn_scale[b] && w->bn_shift[b], "avr_field_pack: bn needs bn_scale / bn_shift of every block");
    if ((rc = pack_bias(w->bn_scale[b], nullptr, H, H, packed + L.bn_a[b], bb))) return rc;
    if ((rc = pack_bias(w->bn_shift[b], nullptr, H, H, packed + L.bn_c[b], bb))) return rc;
  }
  if ((rc = run_fp32_packs(lb, bb, s))) return rc;
  // split-fp16 fragments (header word per layer: 0 lin_in, 1 lin_out, 2+2b fc0[b], 3+2b fc1[b])
  unsigned* hdr = reinterpret_cast<unsigned*>(packed + L.x3_hdr);
  if (hipMemsetAsync(hdr, 0, 64 * sizeof(float), s) != hipSuccess) return fail(AVR_E_HIP, "avr_field_pack: memset");
  const int KC = H / 32;
  X3PackBatch bt{};
  if ((rc = add_x3(bt, w->lin_in_w, H, dims->d_in, kX3InChunks, NT, hdr + 0, packed + L.x3_in))) return rc;
  if ((rc = add_x3(bt, w->lin_out_w, 4, H, KC, 1, hdr + 1, packed + L.x3_out))) return rc;
  for (int b = 0; b < dims->n_blocks; ++b) {
    if ((rc = add_x3(bt, w->fc0_w[b], H, H, KC, NT, hdr + 2 + 2 * b, packed + L.x3_fc0[b]))) return rc;
    if ((rc = add_x3(bt, w->fc1_w[b], H, H, KC, NT, hdr + 3 + 2 * b, packed + L.x3_fc1[b]))) return rc;
  }
  // the table weights for the x3 table kernel (lin_z[t], then scale_z with use_spade)
  for (int t = 0; L.x3_tables && t < L.n_tables; ++t) {
    const float* Wt = t < dims->n_lin_z ? w->lin_z_w[t] : w->scale_z_w[t - dims->n_lin_z];
    if ((rc = add_x3(bt, Wt, H, dims->d_latent, dims->d_latent / 32, NT, hdr + kX3TabHdr + t, packed + L.x3_tab[t])))
      return rc;
  }
  if ((rc = run_x3(bt, s))) return rc;
  // (AVR_FIELD_FP16 packs what AVR_FIELD_X3 packs: recorded as that)
  record_pack(packed, dims->precision == AVR_FIELD_FP16 ? AVR_FIELD_X3 : dims->precision);
  return AVR_OK;
}

extern "C" int avr_field_bwd_packed_floats(const avr_field_dims* dims, int64_t* n_floats) {
  BwdLayout LB;
  const int rc = field_bwd_layout(dims, &LB);
  if (rc) return rc;
  AVR_REQUIRE(n_floats, "avr_field_bwd_packed_floats: null output");
  *n_floats = LB.total;
  return AVR_OK;
}

extern "C" int avr_field_pack_bwd(const avr_field_dims* dims, const avr_resnetfc_weights* w, float* packed_bwd,
                                  void* stream) {
  BwdLayout LB;
  int rc = field_bwd_layout(dims, &LB);
  if (rc) return rc;
  AVR_REQUIRE(w && packed_bwd, "avr_field_pack_bwd: null pointer");
  hipStream_t s = as_stream(stream);
  unsigned* hdr = reinterpret_cast<unsigned*>(packed_bwd);
  if (hipMemsetAsync(hdr, 0, 64 * sizeof(float), s) != hipSuccess) return fail(AVR_E_HIP, "avr_field_pack_bwd: memset");
  const int H = dims->d_hidden, KC = H / 32, NT = H / 16;
  X3PackBatch bt{};
  for (int b = 0; b < dims->n_blocks; ++b) {
    if ((rc = add_x3(bt, w->fc0_w[b], H, H, KC, NT, hdr + 2 + 2 * b, packed_bwd + LB.fc0t[b], true))) return rc;
    if ((rc = add_x3(bt, w->fc1_w[b], H, H, KC, NT, hdr + 3 + 2 * b, packed_bwd + LB.fc1t[b], true))) return rc;
  }
  for (int b = 0; b < AVR_MAX_BLOCKS; ++b)
    if (LB.lzt[b] >= 0 &&
        (rc = add_x3(bt, w->lin_z_w[b], H, H, KC, NT, hdr + kBwdLinZHdr + b, packed_bwd + LB.lzt[b], true)))
      return rc;
  return run_x3(bt, s);
}

extern "C" int avr_field_train_sizes(const avr_field_dims* dims, int n_scenes, int64_t n_points, int64_t* act_floats,
                                     int64_t* mask_words_out) {
  Layout L;
  const int rc = field_layout(dims, &L);
  if (rc) return rc;
  AVR_REQUIRE(n_scenes >= 1 && n_points >= 0 && act_floats && mask_words_out, "avr_field_train_sizes: bad argument");
  const int64_t layers = 2 * dims->n_blocks + 1;
  const int64_t blocks = n_scenes * ((n_points + kX3Samples - 1) / kX3Samples);
  *act_floats = layers * n_scenes * n_points * dims->d_hidden;
  *mask_words_out = layers * blocks * 4 * mask_words(dims->d_hidden / 64) * 64;
  return AVR_OK;
}
