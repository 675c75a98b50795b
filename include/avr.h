/*
 * avr.h — C ABI of libavr_hip.so, the MI355X (gfx950) kernels for the
 * coarse/fine volume-rendering hot path of yankeesong/adaptive-volume-rendering.
 *
 * Every entry point:
 *   - takes DEVICE pointers owned by the caller (fp32, contiguous, ray-major,
 *     sample-minor, channel-innermost unless stated) and an explicit HIP stream
 *     (hipStream_t passed as void*; NULL = legacy default stream);
 *   - allocates nothing, is stateless and re-entrant, and only enqueues work;
 *   - returns 0 (AVR_OK) or an error code; avr_last_error_string() describes
 *     the last failure on the calling thread.
 *
 * The reference is pure Python/PyTorch, so there is no foreign binding to
 * replace; each function below replaces one stage of the reference's Python
 * call chain (file:line in /root/reference) and is bound from Python by
 * ctypes (adaptive-volume-rendering_amd/avr/_lib.py).
 */
#ifndef AVR_H_
#define AVR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVR_ABI_VERSION 18
#define AVR_MAX_BLOCKS 8
#define AVR_LOOKUP_GRAD_TERMS 8   /* tables per avr_latent_tables_grad_points call */
#define AVR_MAX_SCENES 16   /* scenes per training-forward launch */
#define AVR_ADAM_CHUNK 4096        /* elements per work chunk of avr_adam_step; exported so tests can place sizes around it */
#define AVR_ADAM_MAX_TENSORS 88    /* tensors per avr_adam_step launch (what the 4 KB kernel-argument block holds) */

enum {
  AVR_OK = 0,
  AVR_E_INVALID = 1001,     /* bad argument (null pointer, size out of range) */
  AVR_E_UNSUPPORTED = 1002, /* configuration the kernels do not implement     */
  AVR_E_HIP = 1003          /* a HIP runtime call failed                       */
};

int avr_version(void);
const char* avr_last_error_string(void);
/* Number of HIP devices visible (0 when no GPU); never fails. */
int avr_device_count(void);

/* ---------------------------------------------------------------- geometry
 * get_world_rays — utils.py:315-336 (unproject :246-267, normalisation
 * :309-312, transform_rigid :297-307).
 *   x_pix  (n_sb, n_rays, 2)      pixel coordinates
 *   K      (n_sb, 3, 3)           intrinsics
 *   c2w    element (sb, r) at c2w + sb*c2w_sb_stride + r*c2w_ray_stride
 *          (strides in floats; ray stride 0 = one pose per batch, the
 *          stride-0 `expand` the reference's callers pass)
 *   ro, rd (n_sb, n_rays, 3)      outputs                                      */
int avr_world_rays(const float* x_pix, const float* K, const float* c2w, int64_t c2w_sb_stride,
                   int64_t c2w_ray_stride, int64_t n_sb, int64_t n_rays, float* ro, float* rd, void* stream);

/* depth_from_world(ro + rd*dist, c2w) — renderers.py:274-275, utils.py:358-361
 * (transform_world2cam :270-281, a general 4x4 inverse per ray).
 *   dist (n_sb, n_rays) -> depth (n_sb, n_rays)
 *   ddepth_ddist (n_sb, n_rays) or NULL: d depth / d dist, for autograd.
 *   rd = NULL: ro holds world points (dist unused) — depth_from_world of the
 *   raymarcher's final coordinates (renderers.py:346, :459).                   */
int avr_depth_from_world(const float* ro, const float* rd, const float* dist, const float* c2w,
                         int64_t c2w_sb_stride, int64_t c2w_ray_stride, int64_t n_sb, int64_t n_rays,
                         float* depth, float* ddepth_ddist, void* stream);

/* ---------------------------------------------------------------- sampling
 * sample_coarse — renderers.py:4-24 (infinity == -1 branch).
 *   z (n_rays, n_samples) = near + (far-near)*i/N + U*(far-near)/N
 *   noise (n_rays, n_samples) U[0,1) draws, or NULL: counter-based Philox
 *   keyed on (seed, offset + id(ray), sample).
 *   ray_ids (n_rays) int64 or NULL: id(ray) = ray_ids[ray] instead of ray --
 *   a rank's share of a sharded frame keyed by each ray's index in the whole
 *   frame, so the draws do not depend on how the frame was dealt out.          */
int avr_sample_coarse(float near_, float far_, int64_t n_rays, int n_samples, const float* noise,
                      uint64_t seed, uint64_t offset, const int64_t* ray_ids, float* z, void* stream);

/* get_world_rays + sample_coarse in one launch (utils.py:315-336,
 * renderers.py:4-24; the renderer's stage order): the inputs of
 * avr_world_rays, then near / far / n_samples / noise / seed / offset /
 * ray_ids of avr_sample_coarse -> ro, rd (n_sb, n_rays, 3), z (n_sb * n_rays,
 * n_samples), and, if depth_row is not NULL, row 2 of inverse(cam2world) per
 * ray in fp64 (n_sb * n_rays, 4 doubles) for avr_composite_fwd_depth.
 * Outputs equal avr_world_rays + avr_sample_coarse bit for bit.               */
int avr_rays_sample_coarse(const float* x_pix, const float* K, const float* c2w, int64_t c2w_sb_stride,
                           int64_t c2w_ray_stride, int64_t n_sb, int64_t n_rays, float near_, float far_, int n_samples,
                           const float* noise, uint64_t seed, uint64_t offset, const int64_t* ray_ids, float* ro,
                           float* rd, double* depth_row, float* z, void* stream);

/* sample_coarse with per-ray near/far (n_rays) — AdaptiveVolumeRenderer's band
 * around the raymarched distance (renderers.py:492-493).                        */
int avr_sample_coarse_rays(const float* near_, const float* far_, int64_t n_rays, int n_samples,
                           const float* noise, uint64_t seed, uint64_t offset, float* z, void* stream);
/* ABI 16: AdaptiveVolumeRenderer's band for training (renderers.py:490-508): per ray d = (world_x - ro_x) / rd_x,
 * z = sample_coarse(d - eps, d + eps, n_samples) with the given noise (renderers.py:10-14's fp32 operations in
 * torch's order), sorted ascending per ray (torch.sort), and the band points pts = ro + rd * z. world / ro / rd
 * (n_rays, 3), noise / z (n_rays, n_samples), pts (n_rays * n_samples, 3); n_samples <= 64. avr_band_bwd: its
 * adjoint, grad_world (n_rays, 3) = ((sum_i grad_z_i + grad_pts_i . rd) / rd_x, 0, 0); grad_z or grad_pts may be
 * NULL (no gradient).                                                                                            */
int avr_band_fwd(int64_t n_rays, int n_samples, const float* world, const float* ro, const float* rd,
                 const float* noise, float eps, float* z, float* pts, void* stream);
int avr_band_bwd(int64_t n_rays, int n_samples, const float* rd, const float* grad_z, const float* grad_pts,
                 float* grad_world, void* stream);

/* sample_fine + sample_depth + clamp + sort(cat(...)) — renderers.py:27-54,
 * :56-66, :252-258.
 *   weights  (n_rays, n_coarse)  coarse weights (detached)
 *   z_coarse (n_rays, n_coarse)
 *   u, u2    (n_rays, n_importance) the rand / rand_like draws,
 *   noise_depth (n_rays, n_depth)   the randn_like draw;
 *            all three NULL together => in-kernel Philox (seed, offset + id(ray)),
 *            ray_ids as for avr_sample_coarse.
 *   z_sorted (n_rays, n_coarse + n_importance + n_depth) ascending
 *   idx      (n_rays, n_importance) int32 inverse-CDF bin (may be NULL)
 *   z_fine   (n_rays, n_importance) unsorted importance z (may be NULL)
 * n_coarse <= 256, total samples <= 512.                                       */
int avr_sample_fine(const float* weights, const float* z_coarse, float near_, float far_, int64_t n_rays,
                    int n_coarse, int n_importance, int n_depth, float depth_std, const float* u, const float* u2,
                    const float* noise_depth, uint64_t seed, uint64_t offset, const int64_t* ray_ids,
                    float* z_sorted, int32_t* idx, float* z_fine, void* stream);

/* --------------------------------------------------------------- composite
 * volume_integral — renderers.py:69-119.
 *   z (n_rays, N), field (n_rays, N, 4) = (r, g, b, sigma) per sample
 *   rgb (n_rays, 3), dist (n_rays), weights (n_rays, N) or NULL.
 * N <= 1024.                                                                   */
int avr_composite_fwd(const float* z, const float* field, int64_t n_rays, int n_samples, int white_back,
                      float infinity, float* rgb, float* dist, float* weights, void* stream);

/* avr_composite_fwd + depth_from_world(ro + rd * dist, cam2world) in the
 * epilogue (renderers.py:274-275, utils.py:358-361) from the depth rows of
 * avr_rays_sample_coarse: depth (n_rays), equal to avr_depth_from_world bit
 * for bit. ro, rd (n_rays, 3).                                                 */
int avr_composite_fwd_depth(const float* z, const float* field, int64_t n_rays, int n_samples, int white_back,
                            float infinity, const float* ro, const float* rd, const double* depth_row, float* rgb,
                            float* dist, float* weights, float* depth, void* stream);

/* Gradient of volume_integral (autograd of renderers.py:78-112).
 *   grad_rgb (n_rays,3), grad_dist (n_rays) or NULL, grad_weights (n_rays,N)
 *   or NULL -> grad_field (n_rays, N, 4) = d/d(r, g, b, sigma), and grad_z
 *   (n_rays, N) or NULL = d/dz (VolumeRenderer's z carries no gradient;
 *   AdaptiveVolumeRenderer's band does, renderers.py:492-508).               */
int avr_composite_bwd(const float* z, const float* field, int64_t n_rays, int n_samples, int white_back,
                      float infinity, const float* grad_rgb, const float* grad_dist, const float* grad_weights,
                      float* grad_field, float* grad_z, void* stream);

/* ----------------------------------------------- fine pass, early termination
 * BASELINE config 4 (not in the reference; SURVEY §8d "C4 early termination":
 * stop when T < T_stop, fine pass only). The fine samples z (n_rays, N) are
 * consumed front to back in chunks [c0, c0 + C) (C <= 64): gather the active
 * rays' (ro, rd, z chunk), evaluate the field on them, composite the chunk
 * into the per-ray state (fp64 T and sums, the same terms and T carry as
 * avr_composite_fwd) and append the rays with T >= t_stop to active_next
 * (*n_next counts them; zero it first). finish writes rgb (+ 1 - sum w on a
 * white background) and dist. The skipped tail changes rgb by <= t_stop.
 * state: opaque, avr_march_state_bytes(n_rays) bytes of device memory.        */
int avr_march_state_bytes(int64_t n_rays, int64_t* n_bytes);
int avr_march_init(int64_t n_rays, void* state, int32_t* active, void* stream);
int avr_march_gather(const float* ro, const float* rd, const float* z, const int32_t* active, int64_t n_act,
                     int n_samples, int c0, int chunk, float* ro_c, float* rd_c, float* z_c, void* stream);
int avr_march_composite(const float* z, const float* field_c, const int32_t* active, int64_t n_act,
                        int n_samples, int c0, int chunk, float infinity, float t_stop, void* state,
                        int32_t* active_next, int32_t* n_next, void* stream);
int avr_march_finish(const void* state, int64_t n_rays, int white_back, float* rgb, float* dist, void* stream);

/* ------------------------------------------------------------------- field
 * NewPixelNeRFNet.forward — models.py:739-863 with PositionalEncoding :41-87,
 * SpatialEncoder.index :245-274 (bilinear, border, align_corners=True),
 * ResnetFC :541-592, ResnetBlockFC :454-470 — for the default.conf family:
 * use_encoder, use_xyz, normalize_z, PE on xyz only (include_input), raw
 * viewdirs, ReLU, NS = 1, and (x3 inference) eval-mode BatchNorm (dims->bn)
 * and use_spade (dims->spade).
 *
 * The lin_z projections are applied to the latent map once per texel
 * (avr_field_latent_table) and bilinearly interpolated per sample: the
 * interpolation and lin_z are both linear, so this is the same function with
 * one third fewer per-sample FLOPs.                                            */
typedef struct {
  int d_in;        /* MLP input width without latent: 3 + 6*num_freqs + 3 */
  int d_latent;    /* latent channels (multiple of 16, <= 1024)           */
  int d_hidden;    /* 64, 128, 256 or 512                                 */
  int n_blocks;    /* ResnetBlockFC count (<= AVR_MAX_BLOCKS)             */
  int n_lin_z;     /* min(combine_layer, n_blocks)                        */
  int num_freqs;   /* positional-encoding frequencies                     */
  float freq_factor;
  int precision;   /* AVR_FIELD_FP32: v_mfma_f32_16x16x4_f32;
                      AVR_FIELD_X3: split-fp16 v_mfma_f32_16x16x32_f16 (3 products, fp32 accumulate);
                      AVR_FIELD_FP16: the same MFMA, one product (inference only, see below)         */
  int bn;          /* 1: eval-mode BatchNorm in every block (train.py --bn, models.py:430-432, 456-461):
                      ResnetBlockFC applies bn_0 in front of BOTH relus (the reference's bn_0-twice quirk).
                      The caller folds the second one into fc_0 (fc0_w := diag(a) W0, fc0_b := a*b0 + c) and
                      passes the per-feature affine y = a*x + c of bn_0 as bn_scale / bn_shift; the kernel
                      applies it to the residual stream in front of fc_0's relu. x3 inference only.       */
  int spade;       /* 1: ResnetFC(use_spade=True) (models.py:528-534, 585-587): before block b < n_lin_z the
                      residual stream becomes scale_z[b](z) * x + lin_z[b](z). Both projections are per-texel
                      tables with their biases included (avr_field_latent_table writes 2 * n_lin_z tables:
                      lin_z then scale_z), so the lin_z biases are NOT folded into lin_in / fc_1 here.
                      x3 inference only, not with bn.                                                      */
  float beta;      /* > 0: ResnetFC(beta=beta) — every ReLU of the MLP is Softplus(beta) (models.py:442-445,
                      536-537; torch: x where beta*x > 20, else log1p(exp(beta*x)) / beta). 0: ReLU.
                      x3 inference only, not with bn.                                                      */
} avr_field_dims;

#define AVR_FIELD_FP32 0
#define AVR_FIELD_X3 1
/* AVR_FIELD_FP16 (an addition within ABI 18): single-product fp16 MFMA for inference rendering. Every linear
 * layer of the ResnetFC -- lin_in, fc_0 and fc_1 of every block, and lin_out -- keeps the one product Wh.xh of
 * the three AVR_FIELD_X3 computes: operands rounded to fp16 (to nearest even) under the same power-of-two scales
 * (s_w per layer from the blob header, s_x per layer and workgroup from the block's max), fp32 accumulation. The
 * lin_z tables and their blend stay fp32. Not fp32-equivalent: about 1e-4 mean, 2e-3 max absolute error on rgb
 * against the fp32 field at d_hidden 512, meant for 8-bit frames, never for training or parity.
 *   - reads the AVR_FIELD_X3 blob byte for byte: avr_field_pack with AVR_FIELD_FP16 packs what AVR_FIELD_X3
 *     packs, and the fp16 entries accept a blob packed for either;
 *   - accepted by avr_field_fwd_rays, avr_field_fwd_points, their _batch forms and
 *     avr_field_fwd_points_counted;
 *   - AVR_E_UNSUPPORTED (never another path): a BatchNorm, use_spade or Softplus net, and
 *     avr_field_fwd_points_split (NS > 1);
 *   - the training, backward and table entries accept what they accepted before it existed. */
#define AVR_FIELD_FP16 2

/* One ResnetFC's nn.Linear tensors, PyTorch layout (out, in) row-major. */
typedef struct {
  const float* lin_in_w;  const float* lin_in_b;
  const float* lin_out_w; const float* lin_out_b;
  const float* fc0_w[AVR_MAX_BLOCKS]; const float* fc0_b[AVR_MAX_BLOCKS];
  const float* fc1_w[AVR_MAX_BLOCKS]; const float* fc1_b[AVR_MAX_BLOCKS];
  const float* lin_z_w[AVR_MAX_BLOCKS]; const float* lin_z_b[AVR_MAX_BLOCKS];
  /* dims->bn only: eval BatchNorm1d bn_0 of block b as a per-feature affine (d_hidden floats each):
     a = weight / sqrt(running_var + eps), c = bias - running_mean * a                                 */
  const float* bn_scale[AVR_MAX_BLOCKS]; const float* bn_shift[AVR_MAX_BLOCKS];
  /* dims->spade only: ResnetFC.scale_z[b] (d_hidden, d_latent) and its bias, b < n_lin_z             */
  const float* scale_z_w[AVR_MAX_BLOCKS]; const float* scale_z_b[AVR_MAX_BLOCKS];
} avr_resnetfc_weights;

/* Source-view buffers set by NewPixelNeRFNet.encode (models.py:705-734) and
 * SpatialEncoder.forward (models.py:326-328). Host struct, passed by pointer. */
typedef struct {
  float poses[12];        /* world->cam rows [R | t], 3x4 row-major */
  float focal[2];         /* (fx, -fy) as stored by encode           */
  float c[2];
  float image_shape[2];   /* (W, H)                                  */
  float latent_scaling[2];
  int latent_h, latent_w;
} avr_view_desc;

/* Floats needed for one packed ResnetFC (fragment-ordered weights + biases). */
int avr_field_packed_floats(const avr_field_dims* dims, int64_t* n_floats);
/* Repack one ResnetFC into MFMA fragment order (device -> device). dims->precision selects what is packed:
 * AVR_FIELD_FP32 both the fp32 and the split-fp16 fragments, AVR_FIELD_X3 only what the x3 kernels and the
 * tables read (ABI 9) -- run the field kernels with the precision the blob was packed for: the fp32 field
 * entry points reject a blob this library packed for AVR_FIELD_X3 (AVR_E_INVALID; host-side record of the
 * last 128 packs, round 4). */
int avr_field_pack(const avr_field_dims* dims, const avr_resnetfc_weights* w, float* packed, void* stream);
/* table (n_lin_z, H*W, d_hidden) = lin_z[b].weight @ latent[:, texel] (no bias;
 * the bias is folded into the packed biases). latent (d_latent, H, W).
 * dims->spade: (2 * n_lin_z, H*W, d_hidden) — lin_z[b] tables, then scale_z[b]
 * tables, each with its bias added. dims->precision: AVR_FIELD_FP32 exact fp32
 * products, AVR_FIELD_X3 the split-fp16 GEMM (d_latent a multiple of 64 up to
 * 512; ABI 9 -- the training path, which recomputes the tables every step).    */
int avr_field_latent_table(const avr_field_dims* dims, const float* packed, const float* latent, int H, int W,
                           float* table, void* stream);
/* The same for n_scenes maps in one launch (ABI 9): latent (n_scenes, d_latent, H, W), table (n_scenes,
 * max(n_tables, 1), H*W, d_hidden) -- the layout avr_field_fwd_*_batch / _train read.                   */
int avr_field_latent_table_batch(const avr_field_dims* dims, const float* packed, const float* latent, int n_scenes,
                                 int H, int W, float* table, void* stream);
/* Field at xyz = ro[r] + rd[r] * z[r, s], viewdir = rd[r]; out (n_rays*n_samples, 4)
 * = (sigmoid rgb, relu sigma).                                                 */
int avr_field_fwd_rays(const avr_field_dims* dims, const avr_view_desc* view, const float* packed,
                       const float* table, const float* ro, const float* rd, const float* z, int64_t n_rays,
                       int n_samples, float* out, void* stream);
/* Field at explicit points: xyz, viewdirs (n_points, 3) -> out (n_points, 4). */
int avr_field_fwd_points(const avr_field_dims* dims, const avr_view_desc* view, const float* packed,
                         const float* table, const float* xyz, const float* viewdirs, int64_t n_points,
                         float* out, void* stream);

/* Several scenes (<= AVR_MAX_SCENES) in one launch, x3 path only: scene s has
 * its own view views[s] (host array) and lin_z tables (tables + s *
 * max(n_lin_z, 1) * H*W * d_hidden: the per-scene tables back to back), and
 * its samples at rows s * n_rays * n_samples (rays: ro / rd rows s * n_rays)
 * or s * n_points (points) of the inputs and of out. The same results as one
 * avr_field_fwd_rays / _points call per scene (the VolumeRenderer's SB > 1
 * batches, renderers.py:171-174 over models.py:739-863 per object).           */
/* NS > 1 source views per object (NewPixelNeRFNet.num_views_per_obj, models.py:749-853; the MLP combines
 * the views at combine_layer, ResnetFC.forward :566-579 with combine_interleaved, utils.py:71-81): x3
 * inference as two launches around the caller's combine.
 *   b_begin == 0 < b_end < n_blocks (b_end >= n_lin_z): lin_in and blocks [0, b_end) of n_scenes
 *     (object, source view) pairs laid out as avr_field_fwd_points_batch's scenes (view s's pose, focal,
 *     principal point and lin_z tables); h_out (n_scenes * n_points, d_hidden) receives the residual
 *     stream entering block b_end instead of an output.
 *   n_lin_z <= b_begin < b_end == n_blocks: blocks [b_begin, n_blocks) and lin_out of n_scenes objects
 *     from h_in rows (the combined stream); out (n_scenes * n_points, 4). views / tables are checked as
 *     in the batch call but not read; xyz / viewdirs may be NULL.                                      */
int avr_field_fwd_points_split(const avr_field_dims* dims, const avr_view_desc* views, int n_scenes,
                               const float* packed, const float* tables, const float* xyz, const float* viewdirs,
                               int64_t n_points, int b_begin, int b_end, const float* h_in, float* h_out, float* out,
                               void* stream);

int avr_field_fwd_rays_batch(const avr_field_dims* dims, const avr_view_desc* views, int n_scenes,
                             const float* packed, const float* tables, const float* ro, const float* rd,
                             const float* z, int64_t n_rays, int n_samples, float* out, void* stream);
int avr_field_fwd_points_batch(const avr_field_dims* dims, const avr_view_desc* views, int n_scenes,
                               const float* packed, const float* tables, const float* xyz, const float* viewdirs,
                               int64_t n_points, float* out, void* stream);

/* ---------------------------------------------------------- field training
 * Autograd of NewPixelNeRFNet.forward for train.py:108-114 (loss.backward()
 * through the ResnetFC: models.py:541-592, :454-470, :856-862), on the x3
 * path (dims->precision must be AVR_FIELD_X3).
 *
 * Both take a batch of n_scenes (<= AVR_MAX_SCENES) scenes of n_points points
 * each in one launch: views[n_scenes] (host array), tables = the scenes'
 * avr_field_latent_table outputs back to back, xyz / viewdirs (n_scenes,
 * n_points, 3), out (n_scenes * n_points, 4); rows r = scene * n_points + m.
 * Forward: avr_field_fwd_points_train = avr_field_fwd_points that also writes
 *   act  (2 n_blocks + 1) layers of (rows, d_hidden) fp32, layer l at
 *        act + l * act_rows * d_hidden (act_rows >= n_scenes * n_points, so
 *        calls for more scenes can fill one buffer): the relu'd input of every
 *        hidden GEMM, act[2b] = relu(x) into fc_0 of block b, act[2b+1] =
 *        relu(fc_0 out) into fc_1, act[2 n_blocks] = relu(x) into lin_out;
 *   mask (mask_words) their relu masks (opaque, read by avr_field_bwd);
 *   act_max (2 n_blocks + 1) or NULL: atomicMax of max |act[l]| (float bits;
 *        zero it first), the split scales of avr_weight_grads;
 *   z_feature (rows, ld_z >= d_in) or NULL (ABI 9): lin_in's input rows as the
 *        kernel computed them (xyz_rot, PE, viewdir_rot, models.py:763-789),
 *        columns d_in .. ld_z-1 zero; z_max (1 word) or NULL: their max |.|.
 * Backward: avr_field_bwd, given the forward's out and d loss / d out
 * (n_points, 4), writes grads (layer l at grads + l * grads_rows * d_hidden,
 * grads_max as act_max):
 *   grads[2b]   = d loss / d fc_0[b] output (pre-relu),
 *   grads[2b+1] = d loss / d fc_1[b] output,
 *   grads[2 n_blocks] = d loss / d lin_in output.
 * so that dW = grads[l]^T act[l] and db = column sums of grads[l] (fc layers;
 * lin_in with the MLP input, lin_z[b] with the interpolated latent and
 * grads[2b-1] (b >= 1) or grads[2 n_blocks] (b = 0), the gradient at block
 * b's input). packed_bwd: avr_field_bwd_packed_floats floats, filled by
 * avr_field_pack_bwd (fc_0 / fc_1 transposed, x3 fragments).                    */
int avr_field_train_sizes(const avr_field_dims* dims, int n_scenes, int64_t n_points, int64_t* act_floats,
                          int64_t* mask_words);
int avr_field_bwd_packed_floats(const avr_field_dims* dims, int64_t* n_floats);
int avr_field_pack_bwd(const avr_field_dims* dims, const avr_resnetfc_weights* w, float* packed_bwd, void* stream);
int avr_field_fwd_points_train(const avr_field_dims* dims, const avr_view_desc* views, int n_scenes,
                               const float* packed, const float* tables, const float* xyz, const float* viewdirs,
                               int64_t n_points, float* out, float* act, int64_t act_rows, uint32_t* mask,
                               uint32_t* act_max, float* z_feature, int ld_z, uint32_t* z_max, void* stream);
/* ABI 11: act / act_rows = the forward's act buffer and its rows per layer (as passed to
 * avr_field_fwd_points_train): read for Softplus(beta) nets (dims->beta > 0), whose activation derivative
 * comes from the saved activations instead of the relu masks; may be NULL for ReLU nets. */
int avr_field_bwd(const avr_field_dims* dims, const float* packed, const float* packed_bwd, int n_scenes,
                  int64_t n_points, const float* out, const float* grad_out, const uint32_t* mask, const float* act,
                  int64_t act_rows, float* grads, int64_t grads_rows, uint32_t* grads_max, void* stream);

/* Weight gradients of linear layers, dW = G^T X and db = sum_rows G (the
 * parameter half of nn.Linear's autograd, models.py:541-592), for up to
 * AVR_WGRAD_MAX_LAYERS layers in one launch: split-K over the rows (n_split
 * ranges), split-fp16 MFMA (3 products, fp32 accumulate) under power-of-two
 * scales from grad_max / input_max (max |.| as float bits, device; the
 * training kernels above accumulate them with atomicMax). The caller sums
 * the partials over the split: dW = sum_k partial[k], db = sum_k bias_partial[k]. */
#define AVR_WGRAD_MAX_LAYERS 16
typedef struct {
  const float* grad;        /* (n_rows, ld_grad): d loss / d layer output, columns [0, out_dim) */
  int64_t ld_grad;
  const float* input;       /* (n_rows, ld_input): the layer input, columns [0, in_dim) */
  int64_t ld_input;
  int out_dim, in_dim;      /* multiples of 4 */
  const uint32_t* grad_max;
  const uint32_t* input_max;
  float* partial;           /* (n_split, out_dim, in_dim) */
  float* bias_partial;      /* (n_split, out_dim) or NULL */
  /* ABI 12: NULL, or the layer input is relu((input - in_mu) * in_scale + in_shift) per column (in_dim each,
   * 16-B aligned) -- a training-mode BatchNorm's operand rebuilt from its pre-BN rows (avr_bn_layer's
   * AVR_BN_RELU, bit for bit); input_max is then the max of the rebuilt values. */
  const float* in_mu; const float* in_scale; const float* in_shift;
  /* ABI 14: nonzero (in_mu / in_scale / in_shift NULL): the layer input is relu(input) (the layer-by-layer path's
   * identity statistics without their column parameters); input_max is then the max of relu(input). */
  int input_relu;
} avr_wgrad_layer;
int avr_weight_grads(const avr_wgrad_layer* layers, int n_layers, int64_t n_rows, int n_split, void* stream);
/* The caller's sum above, for the whole layer list in one launch (ABI 9): dw[l] (out_dim, in_dim) =
 * sum_k layers[l].partial[k], and db[l] (out_dim) = sum_k layers[l].bias_partial[k] where bias_partial is
 * not NULL, the splits added in order k = 0 .. n_split - 1 in fp32 (replaces torch's partial.sum(0) per
 * layer; train.py's loss.backward() fills .grad from these). 16-B aligned buffers. */
int avr_weight_grads_reduce(const avr_wgrad_layer* layers, int n_layers, int n_split, float* const* dw,
                            float* const* db, void* stream);

/* ------------------------------------------------ training-mode BatchNorm (ABI 11, 12)
 * train.py --bn (train.py:210, :265) builds ResnetBlockFC(bn=True): relu(bn_0(x)) -> fc_0 -> relu(bn_0(net))
 * -> fc_1 (+ x), bn_0 twice per block with batch statistics over every row of the field call
 * (models.py:430-432, 454-461; bn_1 is unused). The statistics are a reduction over all rows between two
 * GEMMs, so this path runs the MLP layer by layer over row-major fp32 rows (n_rows, in_dim / out_dim):
 *
 * avr_bn_layer: one x3 GEMM of a layer over all rows (split-fp16 MFMA, fp32 accumulate, as the fused kernels).
 *   mode AVR_BN_FWD: out = W . op + bias (+ add1) (+ add2) with W = the forward blob's layer `layer` (header
 *     numbering: 0 lin_in, 2 + 2b fc_0[b], 3 + 2b fc_1[b]; pack with dims->bn = 0: no eval-BN folding; ABI 13:
 *     a use_spade blob as well -- avr.layer_train runs use_spade / NS > 1 nets on these layers with identity
 *     statistics, in_mu = out_mu = shift = 0, scale = invstd = 1: op = relu(src), mask = [pre_rows > 0]);
 *     partial (n_wg, 2, out_dim) = per 64-row workgroup (mean, sum of squared deviations) of out's columns.
 *   mode AVR_BN_BWD: gp = (W^T . op) * [(pre_rows - out_mu) * out_scale + out_shift > 0] with W^T from the
 *     backward blob (avr_field_pack_bwd): the relu mask of the forward's AVR_BN_RELU operand, recomputed from
 *     the pre-BN rows (ABI 12; the relu'd operands need not be stored); out = gp (+ add1: ABI 14, a residual
 *     gradient, ld d_hidden; add2 / lin_z_table must be NULL); partial = per workgroup (sum gp, sum gp * xhat),
 *     xhat = (pre_rows - out_mu) * out_invstd. ABI 14: layer AVR_BN_LAYER_LIN_Z_T + b (b < n_lin_z, d_latent ==
 *     d_hidden, no use_spade) is lin_z[b]^T with no mask (pre_rows and the out_* vectors NULL): out = W_z[b]^T .
 *     op (+ add1), the point gradient's sum_b Gz[b] . W_z[b] one layer at a time; the partial is zeros.
 *   The operand op (n_rows, in_dim), read from src (columns >= in_valid are 0):
 *     AVR_BN_PLAIN op = src;
 *     AVR_BN_RELU  op = relu((src - in_mu) * in_scale + in_shift)                 (forward: relu(bn_0(x)));
 *     AVR_BN_GRAD  op = src_res + in_scale * (src - in_m1 - (src_pre - in_mu) * in_invstd * in_m2)
 *                  (src = d loss / d bn output, torch's batch_norm backward; src_res may be NULL).
 *   operand_out (ld in_dim) / operand_max (float bits, atomicMax): the operand as the GEMM used it, or NULL.
 * avr_bn_stats: the forward partials -> batch mean / invstd (folded in fp64: sum n mean, sum M2 + n mean^2),
 *   scale = gamma * invstd, and
 *   the running statistics updated as torch does (momentum; unbiased variance).
 * avr_bn_grad_stats: the backward partials -> m1 = mean gp, m2 = mean gp * xhat, coef = gamma * invstd, and
 *   dgamma += sum gp * xhat, dbeta += sum gp.
 * avr_bn_grad_rows: out = res + coef * (g - m1 - (pre - mu) * invstd * m2) (the last BN backward, no GEMM after
 *   it), out_max as operand_max; out must not overlap g, pre or res.                                                                               */
#define AVR_BN_FWD 0
#define AVR_BN_BWD 1
#define AVR_BN_LAYER_LIN_Z_T 34   /* + b: lin_z[b]^T from the backward blob (AVR_BN_BWD, ABI 14; see below) */
#define AVR_BN_PLAIN 0
#define AVR_BN_RELU 1
#define AVR_BN_GRAD 2
typedef struct {
  int64_t n_rows;
  int mode, prologue;
  int in_dim, in_valid;     /* in_dim: 32 * chunks (64 for lin_in, d_hidden otherwise); in_valid <= in_dim  */
  const float* src; int64_t ld_src;
  const float* src_pre;     /* AVR_BN_GRAD: pre-BN rows (ld ld_src) */
  const float* src_res;     /* AVR_BN_GRAD: rows added (ld ld_src) or NULL */
  const float* in_mu; const float* in_scale; const float* in_shift;
  const float* in_m1; const float* in_m2; const float* in_invstd;
  float* operand_out; uint32_t* operand_max;
  const float* blob; int layer;
  const float* bias; const float* add1; const float* add2;   /* AVR_BN_FWD; add1 also BWD (rows ld d_hidden) */
  float* out;                                                 /* (n_rows, d_hidden) */
  const float* pre_rows;                                      /* AVR_BN_BWD (ld d_hidden) */
  const float* out_mu; const float* out_invstd; const float* out_scale; const float* out_shift;
  float* partial;           /* (ceil(n_rows / 64), 2, d_hidden), within avr_bn_partial_floats floats */
  /* AVR_BN_FWD (ABI 12): NULL, or lin_z rows added last, gathered in the epilogue: row m of scene
   * s = m / rows_per_scene (n_views scenes, n_rows = n_views * rows_per_scene) adds the bilinear blend of the table
   * lin_z_table + s * lin_z_scene_stride ((latent_h * latent_w, d_hidden), e.g. avr_field_latent_table's) at the
   * world point xyz[m] (n_rows, 3) in views[s] -- avr_latent_features' lookup and blend, bit for bit. */
  const float* lin_z_table; int64_t lin_z_scene_stride;
  const float* xyz; const avr_view_desc* views; int n_views; int64_t rows_per_scene;
  /* AVR_BN_BWD (ABI 14): NULL, or max |out| over the stored rows as float bits, max with what is there (the next
   * weight gradient's scale without a reduction pass over the rows) */
  uint32_t* out_max;
} avr_bn_layer;
int avr_bn_layer_run(const avr_field_dims* dims, const avr_bn_layer* l, void* stream);
/* Floats of an avr_bn_layer partial buffer for n_rows rows of n_cols columns: the per-workgroup partials
 * followed by the fp64 scratch avr_bn_stats / avr_bn_grad_stats fold them through (no allocation inside). */
int avr_bn_partial_floats(int64_t n_rows, int n_cols, int64_t* n_floats);
int avr_bn_stats(const float* partial, int64_t n_rows, int n_cols, const float* gamma, float eps, float momentum,
                 float* running_mean, float* running_var, float* mu, float* invstd, float* scale, void* stream);
int avr_bn_grad_stats(const float* partial, int64_t n_rows, int n_cols, const float* gamma, const float* invstd,
                      float* coef, float* m1, float* m2, float* dgamma, float* dbeta, void* stream);
int avr_bn_grad_rows(int64_t n_rows, int n_cols, const float* g, const float* pre, const float* res,
                     const float* coef, const float* m1, const float* m2, const float* mu, const float* invstd,
                     float* out, uint32_t* out_max, void* stream);
/* lin_out over row-major rows (ABI 14), the layer-by-layer paths' output layer (avr.bn_train, avr.layer_train;
 * replaces their torch relu / addmm / sigmoid / threshold_backward, models.py:592, 856-862), d_hidden 64 .. 512
 * (a multiple of 64), every pointer 16-B aligned, weight (4, d_hidden) and bias (4) as nn.Linear holds them:
 * avr_lin_out_fwd_rows: out (n_rows, 4) = [sigmoid(raw[0:3]), relu(raw[3])], raw = relu(x) . weight^T + bias,
 *   x (n_rows, ld_x); x_max (or NULL): max relu(x) as float bits, max with what is there.
 * avr_lin_out_bwd_rows: d_raw (n_rows, 4) = [(grad_out (1 - y)) y rgb, sigma: grad_out where y > 0 else 0] with
 *   y = out (aten's sigmoid_backward and ReluBackward's threshold_backward, bit for bit), g (n_rows, d_hidden) = d_raw . weight where pre > 0, else 0 (aten
 *   threshold_backward; pre (n_rows, ld_pre) = lin_out's input before its relu); d_raw_max (or NULL): max |d_raw|
 *   as float bits, max with what is there. */
/* The spade product rule's backward (ABI 14; avr.layer_train, models.py:585-587: X' = S * X + T): over n values
 * (a multiple of 4, 16-B aligned arrays) gs = g * x and g_out = s * g, each one fp32 product as torch's mul (bit
 * for bit); gs_max (or NULL): max |gs| as float bits, max with what is there. */
int avr_spade_bwd_rows(int64_t n, const float* g, const float* x, const float* s, float* gs, float* g_out,
                       uint32_t* gs_max, void* stream);
int avr_lin_out_fwd_rows(int64_t n_rows, int d_hidden, const float* x, int64_t ld_x, const float* weight,
                         const float* bias, float* out, uint32_t* x_max, void* stream);
int avr_lin_out_bwd_rows(int64_t n_rows, int d_hidden, const float* grad_out, const float* out, const float* weight,
                         const float* pre, int64_t ld_pre, float* d_raw, float* g, uint32_t* d_raw_max, void* stream);
/* ABI 16: the activations' backward alone, d_raw (n_rows, 4) and d_raw_max as avr_lin_out_bwd_rows computes them
 * (no lin_out^T: the fused training path's chain kernel applies it); 16-B aligned (n_rows, 4) rows. */
int avr_lin_out_act_bwd_rows(int64_t n_rows, const float* grad_out, const float* out, float* d_raw,
                             uint32_t* d_raw_max, void* stream);

/* Latent features at points — SpatialEncoder.index (models.py:245-274) as
 * NewPixelNeRFNet.forward uses it (models.py:753-810): bilinear / border /
 * align_corners=True lookup of latent_hwc (H*W, channels), the source view's
 * map channels-last, at world points xyz (n_points, 3) -> out (n_points,
 * channels). channels multiple of 4.                                           */
int avr_latent_features(const avr_view_desc* view, const float* latent_hwc, int channels, const float* xyz,
                        int64_t n_points, float* out, void* stream);
/* n_scenes (<= AVR_MAX_SCENES) views in one launch (ABI 9): latent_hwc (n_scenes, H*W, channels), xyz
 * (n_scenes, n_points, 3), out (n_scenes * n_points, channels).                                         */
int avr_latent_features_batch(const avr_view_desc* views, int n_scenes, const float* latent_hwc, int channels,
                              const float* xyz, int64_t n_points, float* out, void* stream);
/* ABI 12: the adjoint of that lookup with respect to the points -- grad_xyz (n_scenes * n_points, 3) = d loss /
 * d xyz given grad_features (n_scenes * n_points, channels) = d loss / d features: grid_sample's grid gradient
 * (bilinear, border padding -- a clipped coordinate passes no gradient --, align_corners=True) through the
 * projection uv = (-xc_xy / xc_z) * focal + c, xc = R xyz + t (models.py:753-810, :260-273). Replaces the torch
 * autograd of SpatialEncoder.index for the adaptive renderer's band points (renderers.py:492-508).           */
int avr_latent_features_grad_points(const avr_view_desc* views, int n_scenes, const float* latent_hwc, int channels,
                                    const float* xyz, int64_t n_points, const float* grad_features, float* grad_xyz,
                                    void* stream);
/* ABI 15: the same position gradient where the looked-up features feed only linear maps whose per-texel images are
 * at hand -- the lin_z tables (avr_field_latent_table: table_b = lin_z[b].weight @ latent, no bias): sum_b
 * grad_b . lin_z[b](interp(latent, p)) = sum_b grad_b . interp(table_b, p) (both linear), so the gradient through
 * the lookup needs no d loss / d features = sum_b grad_b W_z[b] (a d_hidden x d_latent product per point per
 * table) -- the corner differences of each table dotted with its row of grad_b. tables: scene s, table b at
 * tables + s * table_scene_stride + b * table_stride, (H*W, channels) each; grads[b] (n_scenes * n_points, ld_grad)
 * the gradient at lin_z[b]'s output (d loss / d block-b input); grad_xyz (n_scenes * n_points, 3) written.
 * 1 <= n_tables <= AVR_LOOKUP_GRAD_TERMS. Replaces the torch autograd of SpatialEncoder.index for points whose
 * latent map needs no gradient (the adaptive renderer's band, renderers.py:492-508). */
int avr_latent_tables_grad_points(const avr_view_desc* views, int n_scenes, const float* tables,
                                  int64_t table_scene_stride, int64_t table_stride, int n_tables, int channels,
                                  const float* xyz, int64_t n_points, const float* const* grads, int64_t ld_grad,
                                  float* grad_xyz, void* stream);
/* ABI 16: the position gradient through z_feature for the fused family (use_xyz, normalize_z, PositionalEncoding
 * with include_input on z = R xyz, raw view directions after it; models.py:753-794, :41-87): grad_zf (n_scenes *
 * n_points rows of ld_grad >= 3 + 6 num_freqs) = d loss / d z_feature's first 3 + 6 num_freqs columns; grad_xyz
 * (n_scenes * n_points, 3) = R_s^T d loss / d z, written (accumulate = 0) or added to (accumulate = 1: after the
 * lookup's gradient). Replaces the torch autograd of z_feature for the adaptive renderer's band points.        */
int avr_zfeature_grad_points(const avr_view_desc* views, int n_scenes, const float* xyz, int64_t n_points,
                             const float* grad_zf, int64_t ld_grad, int num_freqs, float freq_factor, int accumulate,
                             float* grad_xyz, void* stream);
/* An addition within ABI 18: the adjoint of the batched lookup with respect to the maps -- grid_sample's input
 * gradient (bilinear, border padding, align_corners=True), channels-last like latent_hwc:
 *   grad_latent_hwc[s, t, :] = sum over points m of scene s and corners k with tex_k(m) == t of
 *                              w_k(m) * grad_features[s * n_points + m, :]
 * with (tex, w) the forward's corners and weights (a clamped corner keeps its zero weight). views / xyz as
 * avr_latent_features_batch; grad_features rows s * n_points + m of ld_grad >= channels floats; grad_latent_hwc
 * (n_scenes, H*W, channels), every row written (zeros where no point lands: no memset needed; n_points = 0 writes
 * a zero map). No float atomics and no data-dependent sum order, so a call is bit-reproducible: the points are
 * ordered stably by (scene, nw texel) -- integer counting, equal texels in ascending point index -- and one wave
 * per destination texel sums the rows of its four neighbouring cells in that order, in chunks of
 * AVR_LATENT_ADJOINT_CHUNK rows whose partial rows (chunk order) a short pass adds. Nothing is read back to the
 * host: grids and scratch are sized by bounds. `scratch` holds avr_latent_features_adjoint_scratch_bytes(...)
 * bytes (monotone in n_points), 16-B aligned like grad_features, its rows (ld_grad a multiple of 4) and
 * grad_latent_hwc; channels a multiple of 4; n_scenes * n_points < 2^28. xyz and grad_features may be NULL when
 * n_points = 0. A bad argument returns AVR_E_INVALID before any launch.                                           */
#define AVR_LATENT_ADJOINT_CHUNK 512
int avr_latent_features_adjoint_scratch_bytes(int n_scenes, int64_t n_points, int latent_h, int latent_w,
                                              int channels, int64_t* n_bytes);
int avr_latent_features_adjoint(const avr_view_desc* views, int n_scenes, const float* xyz, int64_t n_points,
                                const float* grad_features, int64_t ld_grad, int channels,
                                float* grad_latent_hwc, void* scratch, int64_t scratch_bytes, void* stream);

/* --------------------------------------------------------- LSTM ray marcher
 * Raymarcher / AdaptiveVolumeRenderer march (renderers.py:313-351, :380-432):
 * x = ro + rd * init_dist, then `steps` x { v = latent features at x
 * (bilinear, models.py:753-823), (h, c) = LSTMCell(v, (h, c)) with hidden 16,
 * sd = out_layer(h), x += rd * sd }; world (n_rays, 3) = final x, final_dist
 * (n_rays) or NULL = (x - ro)_x / rd_x (renderers.py:490, quirk kept), trace
 * ((steps + 1), n_rays, 3) or NULL = every x. gate_table (H*W, 64) =
 * latent (C, H*W)^T . weight_ih^T (C = feature channels), the input projection
 * per texel; w_hh (64, 16), b_ih / b_hh (64), w_out (16), b_out (1) are the
 * LSTMCell / Linear parameters in torch layout.                               */
int avr_raymarch(const avr_view_desc* view, const float* gate_table, const float* w_hh, const float* b_ih,
                 const float* b_hh, const float* w_out, const float* b_out, const float* ro, const float* rd,
                 const float* init_dist, int64_t n_rays, int steps, float* world, float* final_dist, float* trace,
                 void* stream);

/* Training (ABI 11): the march with autograd for train.py's AdaptiveVolumeRenderer / Raymarcher step
 * (renderers.py:413-432, :320-343). n_scenes (<= AVR_MAX_SCENES) scenes of n_per_scene rays each (ray r in
 * scene r / n_per_scene, its view and gate table; gate_tables (n_scenes, H*W, 64)). Forward: world (n, 3),
 * trace ((steps + 1), n, 3) = every point, state (steps, n, 96) = h, c, i, f, g, o per step (the backward's
 * input). Backward, given grad_world (n, 3): d_tables (n_scenes, H*W, 64), fp32, = d loss / d gate table
 * (written whole; W_ih's gradient is then sum_s d_tables[s]^T latent_s^T, the latent's W_ih^T d_tables[s]),
 * d_grads (64*16 + 64 + 16 + 1) = d W_hh, d (b_ih = b_hh), d w_out, d b_out, with the reference's clamp(-10, 10)
 * of every h gradient (state[0].register_hook) and grid_sample's border / align_corners=True position gradient.
 * ABI 15: bit-deterministic by construction, no floating-point atomics -- the table gradient summed as int64
 * fixed-point values under one power-of-two scale per call (chosen from max |dg| so no sum can overflow; integer
 * sums do not depend on the order), then rounded once to fp32 (an entry a NaN / inf gate gradient reached is
 * NaN); the parameter gradients summed in a fixed order.
 * Accuracy of d_tables: absolute, relative to the largest gate gradient of the call. With e the frexp exponent of
 * max |dg| over the call's finite gate gradients and cbits = ceil(log2(4 * steps * n)), every contribution
 * w_corner * dg (the exact product of the two fp32 values) is rounded once onto a grid of 2^(cbits + e - 62), so an
 * entry that n_i lookups reach differs from the exact sum of its contributions by at most n_i * 2^(cbits + e - 63)
 * <= n_i * 2^(cbits - 62) * max |dg|, plus the one rounding of the sum to fp32 (tests/test_gpu_march_kernels.py,
 * test_fixed_point_*). For callers: entries below about 2^-22 of the call's largest are not accurate to fp32
 * relative precision (a contribution below 2^(cbits - 62) of max |dg| is lost altogether); the table gradient is
 * meant to be consumed at the scale of its largest entries, as W_ih's and the latent's gradients do. A ray whose
 * gate gradients are NaN / inf (a NaN in its grad_world, say) makes the entries its lookups touch NaN and the
 * parameter gradients non-finite, and changes no other table entry; steps = 0 (or n_per_scene = 0) writes d_tables and d_grads as exact zeros.
 * `scratch` holds avr_raymarch_bwd_scratch_bytes(n, steps,
 * n_scenes * H*W * 64) bytes (n = n_scenes * n_per_scene; the accumulators, the stored gate gradients and
 * lookups, the workgroups' partials), scratch_bytes its size; lookup_grad 1 =
 * the lookup's position gradient flows into the points (models.py:753-823 with stop_encoder_grad False), 0 = it
 * does not (stop_encoder_grad True detaches the looked-up latent, models.py:810-811: W_ih, the LSTM and
 * out_layer still get theirs, the points only through x += rd * sd).                                          */
int avr_raymarch_train(const avr_view_desc* views, int n_scenes, const float* gate_tables, const float* w_hh,
                       const float* b_ih, const float* b_hh, const float* w_out, const float* b_out, const float* ro,
                       const float* rd, const float* init_dist, int64_t n_per_scene, int steps, float* world,
                       float* trace, float* state, void* stream);
int avr_raymarch_bwd_scratch_bytes(int64_t n_rays, int steps, int64_t table_entries, int64_t* n_bytes);
int avr_raymarch_bwd(const avr_view_desc* views, int n_scenes, const float* gate_tables, const float* w_hh,
                     const float* w_out, const float* rd, const float* trace, const float* state,
                     const float* grad_world, int64_t n_per_scene, int steps, int lookup_grad, float* d_tables,
                     float* d_grads, void* scratch, int64_t scratch_bytes, void* stream);

/* AdaptiveVolumeRenderer / Raymarcher inference front end (renderers.py:313-343, :380-432, :490-496), n_scenes
 * (<= AVR_MAX_SCENES) scenes of n_per_scene rays (ray r in scene r / n_per_scene: its view and gate table), in
 * one launch. Added within ABI 18 (no version change). Per ray:
 *   start distance  init_dist[r], or with init_dist NULL 0.8 + 0.05 * N(0, 1) (the reference's
 *                   normal_(mean=0.8, std=5e-2)) from Philox;
 *   world (n, 3)    the march of avr_raymarch from ro + rd * start (the same instructions: for one scene and a
 *                   given init_dist, bit-equal to avr_raymarch's world);
 *   z_sorted (n, n_band), n_band > 0: d = (world_x - ro_x) / rd_x (quirk kept; rd_x = 0 gives a NaN row),
 *                   z_i = ((d - eps) + span * (i / n_band)) + (u_i * span) / n_band, span = (d + eps) - (d - eps),
 *                   sorted ascending: avr_band_fwd's z bit for bit for the same world and noise. u = band_noise
 *                   (n, n_band), or with band_noise NULL Philox uniforms. n_band = 0 (Raymarcher): no band,
 *                   z_sorted may be NULL.
 * Philox draws use key = offset + (ray_ids ? ray_ids[r] : r), as avr_sample_coarse keys its draws. Streams
 * (counter word 3) of the library: 0x1001 coarse noise, 0x2002 fine (u, u2), 0x4004 depth normals
 * (avr_sample_coarse / avr_sample_fine); 0x8008 the march's start distance (Box-Muller on words 0, 1 of block
 * 0); 0x10010 the band noise (sample i = word i & 3 of block i >> 2).
 * init_out (n) / noise_out (n, n_band), when not NULL, receive the start distances / band noise used (drawn or
 * given). n_per_scene = 0 returns AVR_OK without a launch. */
int avr_adaptive_front(const avr_view_desc* views, int n_scenes, const float* gate_tables, const float* w_hh,
                       const float* b_ih, const float* b_hh, const float* w_out, const float* b_out,
                       const float* ro, const float* rd, const float* init_dist, const float* band_noise,
                       uint64_t seed, uint64_t offset, const int64_t* ray_ids, int64_t n_per_scene, int steps,
                       float eps, int n_band, float* world, float* z_sorted, float* init_out, float* noise_out,
                       void* stream);

/* ------------------------------------------------- training loss and metrics
 * ABI 17: loss_fn (utils.py:364-377) over n_rays rays without a host sync, so it can be recorded in a HIP-graph
 * capture. terms = AVR_LOSS_COARSE | AVR_LOSS_FINE | AVR_LOSS_DEPTH selects
 *   loss = [mean((rgb_c - gt)^2)] + [mean((rgb_f - gt)^2)] + [10000 mean(max(near - d, 0) + max(d - far, 0))]
 * (--loss_mode coarse | fine | both, --depth_regularization); rgb_c, rgb_f, gt (n_rays, 3) and depth (n_rays) as
 * the renderers return them; the pointer of a term that is not selected is not read. If the MSE part (the sum of
 * the selected MSEs) is NaN it becomes 1e-6 and every rgb gradient exactly 0 (the reference's `if loss.isnan()`,
 * decided on the device); the penalty is added and differentiated as usual, and a non-finite depth propagates.
 * Forward: one pass, every difference, square and sum in fp64, the workgroups' partials added in a fixed order
 * (no floating-point atomics: bit-identical from run to run) -> record[4] = {loss, mse_c, mse_f, penalty} (the
 * MSEs as summed, NaN included; 0 for a term not selected). `workspace` holds avr_loss_workspace_bytes(n_rays)
 * bytes (the partials; may be NULL where one workgroup covers n_rays). One launch, two above 2730 rays.
 * Backward, one launch: grad_rgb_c / grad_rgb_f (n_rays, 3) = g 2 (rgb - gt) / (3 n_rays), or 0 under the NaN rule
 * read from the forward's record; grad_depth (n_rays) = g 10000 / n_rays (c(d - far) - c(near - d)) with c(t) = 1
 * for t > 0, 0.5 at t == 0 (torch.max's backward at a tie) and 0 below; g = grad_loss[0], a DEVICE scalar. A NULL
 * gradient pointer is skipped. n_rays == 0 is a no-op; null pointers of selected terms and a selection without
 * AVR_LOSS_COARSE or AVR_LOSS_FINE are refused before any HIP call.                                              */
#define AVR_LOSS_COARSE 1
#define AVR_LOSS_FINE 2
#define AVR_LOSS_DEPTH 4
int avr_loss_workspace_bytes(int64_t n_rays, int64_t* n_bytes);
int avr_loss_fwd(int64_t n_rays, int terms, const float* rgb_c, const float* rgb_f, const float* depth,
                 const float* gt, float near_, float far_, void* workspace, int64_t workspace_bytes, float* record,
                 void* stream);
int avr_loss_bwd(int64_t n_rays, int terms, const float* rgb_c, const float* rgb_f, const float* depth,
                 const float* gt, float near_, float far_, const float* record, const float* grad_loss,
                 float* grad_rgb_c, float* grad_rgb_f, float* grad_depth, void* stream);

/* ABI 17: PSNR and SSIM of n_frames pairs of (height, width, 3) frames, pixel-major and channel-innermost -- what
 * get_metrics (utils.py:431-461) asks of skimage.metrics with data_range = 1: psnr[f] = 10 log10(1 / mse) over all
 * height * width * 3 values (+inf for identical frames); ssim[f] = structural_similarity(channel_axis=-1): per
 * channel the 7 x 7 uniform-window means, sample covariances (49/48), C1 = 1e-4, C2 = 9e-4, S averaged over the
 * window positions inside the frame (the 3-pixel border cropped), then over the channels. Moments and S in fp64
 * (products of fp32 values are exact there); the tiles' fp64 partials of S and of the squared error are added in
 * a fixed order (bit-identical from run to run). `workspace` holds avr_image_metrics_workspace_bytes() bytes.
 * Two launches (every tile of every frame, then one wave per frame). height, width >= 7; n_frames == 0 is a
 * no-op; sizes and null pointers are checked before any HIP call.                                              */
int avr_image_metrics_workspace_bytes(int64_t n_frames, int height, int width, int64_t* n_bytes);
int avr_image_metrics(const float* img, const float* gt, int64_t n_frames, int height, int width, void* workspace,
                      int64_t workspace_bytes, float* psnr, float* ssim, void* stream);

/* ---------------------------------------------------------------- optimizer
 * ABI 18: optimizer.step() of train.py:112-114 with the torch.optim.Adam of train.py:299, for a list of fp32
 * tensors. Per element, in the order of torch's _single_tensor_adam, every operation rounded once to fp32:
 *   g = grad (+ weight_decay * p   if weight_decay != 0)
 *   m = m + (g - m) * (1 - beta1)
 *   v = v * beta2 + ((1 - beta2) * g) * g
 *   t = step + 1
 *   p = p + -(lr / (1 - beta1^t)) * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps))
 * `tensors` is a HOST array of n_tensors entries; param, grad, exp_avg, exp_avg_sq are device pointers to numel
 * contiguous floats each (the same element order in all four). The list is copied into the kernel arguments
 * (AVR_ADAM_MAX_TENSORS entries per launch; a longer list takes several launches), so the array may be freed on
 * return and a captured launch reads no host memory. A tensor whose four pointers are all 16-B aligned is
 * read and written 16 B per lane; any other, and a tail of fewer than 4 elements, 4 B per lane. `step` is the
 * step counter, one float in DEVICE memory that the host never reads: the update launches read it and compute the
 * two bias-correction factors from it in fp64 (beta^t by squaring), rounded once to fp32; a trailing one-wave
 * launch then advances it by 1, once per call, so no launch reads the counter while another workgroup writes it.
 * ceil(non-empty tensors / AVR_ADAM_MAX_TENSORS) + 1 launches per call; nothing is allocated, nothing
 * synchronises: the call can be recorded in a HIP-graph capture, which bakes in the hyper-parameters.
 * NaN and inf in a gradient propagate as the formula does (no guard, no skipped step).
 * Checked before any HIP call: n_tensors == 0 is a no-op that leaves `step` untouched; n_tensors < 0, a null
 * `tensors` or `step`, numel < 0, a null pointer in an entry with numel > 0, lr < 0, a beta outside [0, 1),
 * eps < 0 and weight_decay < 0 return AVR_E_INVALID. An entry with numel == 0 is skipped.                       */
typedef struct {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
} avr_adam_tensor;
int avr_adam_step(const avr_adam_tensor* tensors, int64_t n_tensors, double lr, double beta1, double beta2, double eps,
                  double weight_decay, float* step, void* stream);

/* ---------------------------------------------------------- occupancy grid
 * Additions within ABI 18 (no version change): empty-space skipping for VolumeRenderer inference (not in the
 * reference; DESIGN.md "Occupancy grid"). A grid is a bit per cell of an axis-aligned box [lo, hi) with res =
 * (rx, ry, rz) cells, each in 1 .. AVR_OCC_MAX_RES, rx a multiple of 32, packed along x into uint32 words: cell
 * (ix, iy, iz) is bit ix % 32 of word (iz * ry + iy) * (rx / 32) + ix / 32. inv[a] = (float)(res[a] / ((double)hi[a]
 * - (double)lo[a])) is computed by the caller.
 * A sample (ray r, z[r, s]) is the point p = fadd(ro, fmul(rd, z)) of avr_field_fwd_rays (the same two roundings,
 * uncontracted); with t[a] = fmul(fsub(p[a], lo[a]), inv[a]) and i[a] = (int)floorf(t[a]) it is LIVE iff every
 * 0 <= i[a] < res[a] (tested as 0 <= t[a] < res[a], the same for finite t and defined for an infinite one) and the
 * cell's bit is set. A point outside the box is dead; a point with a non-finite coordinate is live (the field sees
 * it, as in the ungated render).
 *   avr_occ_build: sigma (n_planes, rz, ry, rx) fp32 -> bits (rx / 32 * ry * rz words, every word written): a cell
 *     is set iff any plane at any cell within Chebyshev distance dilate (0, 1 or 2; neighbours clamped at the box
 *     faces) has !(sigma <= thr) -- NaN counts as occupied.
 *   avr_occ_classify: ro, rd (n_rays, 3), z (n_rays, n_samples), n_samples in 1 .. AVR_OCC_MAX_SAMPLES -> mask
 *     (n_rays, ceil(n_samples / 64)) uint64, bit s % 64 of word s / 64 = sample s is live (bits past n_samples
 *     clear), and counts (n_rays) int32 = live samples of the ray.
 *   avr_occ_compact: mask and offsets (n_rays) int64 = the exclusive prefix sum of counts -> xyz, viewdirs
 *     (n_live, 3): the live samples' points and ray directions in ray-major sample order (rank of a live sample =
 *     offsets[r] + popcount of the lower mask bits of its ray), n_live = the sum of counts.
 *   avr_occ_expand: field_c (n_live, 4) = the field at the compacted points -> field (n_rays * n_samples, 4): a
 *     live sample's row of field_c, exactly 0.0f in all four channels for a dead one; every element is written (no
 *     memset). field and field_c 16-B aligned.
 * No atomics, so every output is bit-reproducible. Checked before any HIP call (AVR_E_INVALID): null pointers, res
 * and n_samples out of range, rx % 32 != 0, dilate outside 0 .. 2, n_planes < 1, negative n_rays, n_live outside
 * 0 .. n_rays * n_samples. n_rays == 0 launches nothing and succeeds, as does compact with n_live == 0; expand with
 * n_live == 0 writes zeros and reads neither field_c, mask nor offsets (they may be NULL).                        */
#define AVR_OCC_MAX_RES 256
#define AVR_OCC_MAX_SAMPLES 256
typedef struct {
  float lo[3];
  float inv[3];
  int res[3];             /* rx, ry, rz */
  const uint32_t* bits;   /* device */
} avr_occ_grid;
int avr_occ_build(const float* sigma, int n_planes, const int* res, float thr, int dilate, uint32_t* bits,
                  void* stream);
int avr_occ_classify(const avr_occ_grid* grid, const float* ro, const float* rd, const float* z, int64_t n_rays,
                     int n_samples, uint64_t* mask, int32_t* counts, void* stream);
int avr_occ_compact(const float* ro, const float* rd, const float* z, const uint64_t* mask, const int64_t* offsets,
                    int64_t n_rays, int n_samples, int64_t n_live, float* xyz, float* viewdirs, void* stream);
int avr_occ_expand(const float* field_c, const uint64_t* mask, const int64_t* offsets, int64_t n_rays, int n_samples,
                   int64_t n_live, float* field, void* stream);

/* ------------------------------------------- occupancy grid, device-side count
 * Additions within ABI 18 (no version change; DESIGN.md "Occupancy grid: device-side live count"): the same gated
 * chain with the live count kept on the device from avr_occ_classify to avr_occ_expand, so that no host read sizes a
 * launch and the chain can be recorded in a HIP-graph capture:
 *   classify -> avr_occ_scan -> avr_occ_compact_counted -> avr_field_fwd_points_counted -> avr_occ_expand_counted
 * The compacted buffers (xyz, viewdirs (capacity, 3); field_c (capacity, 4)) are sized by a host `capacity`, 0 <=
 * *n_live <= capacity <= n_rays * n_samples; a device count outside 0 .. capacity is held to that range by every
 * kernel that reads it, so no row at or beyond capacity is touched.
 *   avr_occ_scan: counts (n_rays) int32 -> offsets (n_rays) int64 = the exclusive prefix sums, *total (device int64)
 *     = the sum. total is always written (0 for n_rays == 0: one tiny launch), no memset by the caller. Every n_rays
 *     avr_occ_classify accepts. Reduce, then scan: at most three launches (one up to AVR_OCC_SCAN_RAYS rays), each
 *     workgroup owning AVR_OCC_SCAN_RAYS consecutive rays; no kernel waits on another workgroup; integer adds only,
 *     so the result is exact and reproducible for every sum that fits int64. Between its launches offsets holds the
 *     workgroup sums (no scratch buffer). offsets and total 8-B aligned.
 *   avr_occ_compact_counted / avr_occ_expand_counted: avr_occ_compact / avr_occ_expand with n_live read from the
 *     device (8-B aligned). Compact writes rows [0, *n_live) of xyz and viewdirs and nothing beyond; expand writes
 *     every element of field and never reads a field_c row at or beyond *n_live (with *n_live == 0 it reads neither
 *     mask nor offsets). capacity == 0 launches nothing (expand then leaves field unwritten: there is no compacted
 *     buffer to expand; avr_occ_expand with n_live = 0 zero-fills).
 *   avr_field_fwd_points_counted: avr_field_fwd_points launched over `capacity` rows, with every use of the row
 *     count taken from *n_points (device int64, 8-B aligned). Rows [*n_points, capacity) of out, xyz and viewdirs are
 *     neither read nor written; rows below the count are bit-equal to avr_field_fwd_points with n_points = the count
 *     (same workgroup membership). A workgroup whose first row is at or beyond the count returns at once. Both
 *     precisions, ReLU nets without BatchNorm or use_spade at every d_hidden of the fused path; a BatchNorm,
 *     use_spade or Softplus net is AVR_E_UNSUPPORTED (no counted kernel, never another path).
 * Checked before any launch (AVR_E_INVALID): null pointers, negative n_rays / capacity, n_samples out of range,
 * capacity above n_rays * n_samples, misaligned field rows or counts. capacity == 0 or n_rays == 0 returns AVR_OK
 * with no launch, except that avr_occ_scan writes *total.                                                          */
#define AVR_OCC_SCAN_RAYS 2048
int avr_occ_scan(const int32_t* counts, int64_t n_rays, int64_t* offsets, int64_t* total, void* stream);
int avr_occ_compact_counted(const float* ro, const float* rd, const float* z, const uint64_t* mask,
                            const int64_t* offsets, int64_t n_rays, int n_samples, const int64_t* n_live,
                            int64_t capacity, float* xyz, float* viewdirs, void* stream);
int avr_occ_expand_counted(const float* field_c, const uint64_t* mask, const int64_t* offsets, int64_t n_rays,
                           int n_samples, const int64_t* n_live, int64_t capacity, float* field, void* stream);
int avr_field_fwd_points_counted(const avr_field_dims* dims, const avr_view_desc* view, const float* packed,
                                 const float* table, const float* xyz, const float* viewdirs, int64_t capacity,
                                 const int64_t* n_points, float* out, void* stream);

/* ------------------------------------ occupancy grid: hierarchical build
 * Additions within ABI 18 (no version change; DESIGN.md "Occupancy grid: hierarchical build"): the field is evaluated
 * at the fine cells under live coarse cells only, by the gating chain with a fine x-row for the ray and a cell of the
 * row for the sample:
 *   avr_occ_children -> avr_occ_scan -> (one host read of the total) -> avr_occ_child_points
 *     -> per plane: the field on the point list, avr_occ_flag_sigma -> avr_occ_build_sparse
 * Shapes: the fine grid has res = (rx, ry, rz) within the limits above; factor f in {2, 4, 8}; every res[a] % f == 0;
 * the coarse grid C has res rc = res / f, rc[0] % 32 == 0, over the same box.
 * Candidates: fine cell (ix, iy, iz) is a candidate iff bit (ix / f, iy / f, iz / f) of C is set. They are ordered by
 * the linear fine index (iz * ry + iy) * rx + ix, ascending; the order does not depend on the data. mask is
 * (ry * rz, ceil(rx / 64)) uint64: row iz * ry + iy, bit ix % 64 of word ix / 64 (bits at or past rx clear); counts
 * int32 per row; offsets and total are avr_occ_scan's over the ry * rz rows; M = total = f^3 * popcount(C). A
 * candidate's rank is offsets[row] + popcount of the lower mask bits of its row. No atomics, no slot array, no
 * memset: every output is bit-reproducible.
 *   avr_occ_children: coarse descriptor (its box is not read), f, fine res -> mask, counts; every element written.
 *   avr_occ_child_points: xyz[rank] = (c_x, c_y, c_z), c_a = (float)(lo64[a] + (i_a + 0.5) * step[a]) with lo64[a] =
 *     (double)(float)lo[a] and step[a] = (hi64[a] - lo64[a]) / res[a] computed once by the caller in double (host
 *     arrays of three); the product and the sum are each rounded once in double, never fused. viewdirs[rank] = dir
 *     (host array of three floats). xyz or viewdirs may be NULL (not both): one xyz serves several directions.
 *   avr_occ_flag_sigma: field_c (n_live, 4; 16-B aligned), sigma = channel 3 -> flags (n_live) bytes:
 *     flags[q] = (first ? 0 : flags[q]) | !(sigma[q] <= thr); NaN counts as occupied. thr must be >= 0.
 *   avr_occ_build_sparse: fine cell c is set iff some cell within Chebyshev distance dilate (0, 1 or 2, clamped at
 *     the faces) of c is a candidate whose flag is set; every word of bits is written; n_live == 0 writes zeros and
 *     reads neither mask, offsets nor flags (they may be NULL). These are the bits avr_occ_build gives for planes
 *     that hold the evaluated sigma at the candidates and 0 elsewhere, which is why thr < 0 (and NaN) is refused: it
 *     would call unevaluated cells occupied.
 *   avr_occ_downsample: p in {1, 2, 4}, res[a] % p == 0, (res[0] / p) % 32 == 0 -> coarse_bits of res / p: the OR of
 *     the p^3 children; every word written.
 * Checked before any launch (AVR_E_INVALID): null pointers, res out of range, factor, p, divisibility, a coarse res
 * that is not res / factor, dilate outside 0 .. 2, thr negative or NaN, n_live outside 0 .. rx * ry * rz, mask or
 * offsets not 8-B aligned, field rows not 16-B aligned. avr_occ_child_points and avr_occ_flag_sigma with n_live == 0
 * return AVR_OK with no launch.                                                                                    */
int avr_occ_children(const avr_occ_grid* coarse, int factor, const int* res, uint64_t* mask, int32_t* counts,
                     void* stream);
int avr_occ_child_points(const uint64_t* mask, const int64_t* offsets, const int* res, const double* lo64,
                         const double* step, const float* dir, int64_t n_live, float* xyz, float* viewdirs,
                         void* stream);
int avr_occ_flag_sigma(const float* field_c, float thr, int first, int64_t n_live, uint8_t* flags, void* stream);
int avr_occ_build_sparse(const uint64_t* mask, const int64_t* offsets, const uint8_t* flags, int64_t n_live,
                         const int* res, int dilate, uint32_t* bits, void* stream);
int avr_occ_downsample(const uint32_t* bits, const int* res, int p, uint32_t* coarse_bits, void* stream);

/* ------------------------------- fine pass, early termination on the device
 * Additions within ABI 18 (no version change; DESIGN.md "Early termination: device-side chain"): the early
 * termination of avr_march_* with every count kept on the device, combinable with an occupancy grid. No host read
 * sizes a launch, nothing is appended with an atomic, so the chain can be recorded in a HIP-graph capture and every
 * output is bit-reproducible. state is avr_march_init's (its active list is not used). Per chunk [c0, c0 + chunk)
 * of z (n_rays, n_samples), chunk in 1 .. 64, the number of chunks fixed on the host:
 *   avr_march_classify -> avr_occ_scan -> avr_march_compact_counted -> avr_field_fwd_points_counted
 *     -> avr_march_composite_masked
 * and avr_march_finish after the last chunk.
 *   avr_march_classify: ray r is ALIVE iff c0 == 0 or (float)state[r].T >= t_stop (avr_march_composite's survivor
 *     rule: a stopped ray's T is never updated again, so the test needs no flag). A sample of an alive ray is live
 *     iff it passes avr_occ_classify's test against `grid` (the same point, the same float tests, a non-finite
 *     coordinate is live); grid == NULL: every sample of an alive ray. -> mask (n_rays) uint64, bit k = sample
 *     c0 + k is live, bits at or beyond chunk clear, and counts (n_rays) int32. A stopped ray writes mask 0 and
 *     count 0; every element is written (no memset).
 *   avr_march_compact_counted: avr_occ_compact_counted for the column window: with offsets and *n_live from
 *     avr_occ_scan(counts) it writes rows [0, *n_live) of xyz and viewdirs (capacity, 3), ray-major, and nothing
 *     beyond. capacity <= n_rays * chunk; a device count outside 0 .. capacity is held to that range.
 *   avr_march_composite_masked: one wave per ray over all n_rays. A stopped ray is left as it is. Otherwise sample
 *     c0 + k takes row offsets[r] + popcount(mask[r] & ((1 << k) - 1)) of field_c (capacity, 4; 16-B aligned) where
 *     bit k is set and exactly 0.0f in all four channels where it is clear; from there on the terms, rounding
 *     points, fp64 scan with the carried T and sums of avr_march_composite, so state is bit-equal to that entry's
 *     over the same field values. *evaluated (device int64) = *n_live (accumulate == 0) or *evaluated + *n_live
 *     (accumulate != 0), by a plain load and store of one lane: launches on a stream are ordered.
 * Checked before any HIP call (AVR_E_INVALID): null pointers, negative n_rays, chunk outside 1 .. 64, c0 < 0 or
 * c0 + chunk > n_samples, capacity outside 0 .. n_rays * chunk, a grid avr_occ_classify refuses, counts, masks,
 * offsets or state not 8-B aligned, field rows not 16-B aligned. n_rays == 0 returns AVR_OK with no launch, as does
 * avr_march_compact_counted with capacity == 0.                                                                  */
int avr_march_classify(const avr_occ_grid* grid, const float* ro, const float* rd, const float* z, const void* state,
                       int64_t n_rays, int n_samples, int c0, int chunk, float t_stop, uint64_t* mask,
                       int32_t* counts, void* stream);
int avr_march_compact_counted(const float* ro, const float* rd, const float* z, const uint64_t* mask,
                              const int64_t* offsets, int64_t n_rays, int n_samples, int c0, int chunk,
                              const int64_t* n_live, int64_t capacity, float* xyz, float* viewdirs, void* stream);
int avr_march_composite_masked(const float* z, const float* field_c, const uint64_t* mask, const int64_t* offsets,
                               const int64_t* n_live, int64_t capacity, int64_t n_rays, int n_samples, int c0,
                               int chunk, float infinity, float t_stop, void* state, int64_t* evaluated,
                               int accumulate, void* stream);

/* ------------------------------------------ occupancy grid: per-ray bounds
 * Additions within ABI 18 (no version change; DESIGN.md "Occupancy grid: per-ray sampling bounds"): where along
 * [near_, far_] a ray's occupied cells begin and end, and the two sampling entries with per-ray bounds that place the
 * renderer's samples there. "Live" below is avr_occ_classify's test: the fp32 point fadd(ro, fmul(rd, z)), the fp32
 * cell coordinates, a non-finite coordinate live, a point outside the box dead.
 *   avr_occ_ray_bounds: ro, rd (n_rays, 3) -> t_near, t_far (n_rays), near_ <= t_near[r] <= t_far[r] <= far_.
 *     (S) Safety: every fp32 z in [near_, far_] that is live for ray r has t_near[r] <= z <= t_far[r]: no sample that
 *       gating would have evaluated falls outside the bounds. A ray with a non-finite ro or rd component gets exactly
 *       (near_, far_).
 *     (T) Tightness: with [a, b] the hull, in exact arithmetic, of the ray's intersections with the occupied cells
 *       clipped to [near_, far_], and slack = sqrt(3) * max_a(cell edge_a) / |rd|: a ray that crosses some occupied
 *       cell shrunk by 1/8 of a cell edge on every side (a clear hit) has t_near >= a - slack, t_far <= b + slack.
 *     (M) Miss: a ray that misses every occupied cell grown by 1/8 of a cell edge on every side (a clear miss) gets
 *       exactly (near_, far_): gating evaluates none of its samples wherever they lie, and its sampling -- its
 *       background pixel -- stays as it is without bounds, bit for bit.
 *     A ray that is neither may get either answer; (S) and the range hold for it. An interval that is empty or
 *     inverted after the clamp to [near_, far_] is reported as a miss. One ray per lane, no atomics: two launches give
 *     the same bits.
 *   avr_sample_coarse_bounds: avr_sample_coarse with near_r, far_r (n_rays) in place of the two scalars; noise,
 *     seed, offset and ray_ids as there (the same Philox keying).
 *   avr_sample_fine_bounds: avr_sample_fine with near_r, far_r (n_rays) in place of the two scalars: ray r's
 *     importance samples are scaled to, and its depth samples clamped to (quirk Q6), its own [near_r[r], far_r[r]].
 *   Where every element of near_r / far_r equals the scalars, both give their scalar counterpart's outputs bit for bit.
 * Checked before any launch (AVR_E_INVALID): null pointers, a grid avr_occ_classify refuses, negative n_rays,
 * !(near_ < far_), and what avr_sample_coarse / avr_sample_fine check. n_rays == 0 returns AVR_OK with no launch.  */
int avr_occ_ray_bounds(const avr_occ_grid* grid, const float* ro, const float* rd, int64_t n_rays, float near_,
                       float far_, float* t_near, float* t_far, void* stream);
int avr_sample_coarse_bounds(const float* near_r, const float* far_r, int64_t n_rays, int n_samples,
                             const float* noise, uint64_t seed, uint64_t offset, const int64_t* ray_ids, float* z,
                             void* stream);
int avr_sample_fine_bounds(const float* weights, const float* z_coarse, const float* near_r, const float* far_r,
                           int64_t n_rays, int n_coarse, int n_importance, int n_depth, float depth_std,
                           const float* u, const float* u2, const float* noise_depth, uint64_t seed, uint64_t offset,
                           const int64_t* ray_ids, float* z_sorted, int32_t* idx, float* z_fine, void* stream);

/* ------------------------------------------------------------ measurement
 * Streaming device copy dst[0, n_bytes) = src[0, n_bytes) (16-B aligned,
 * n_bytes a multiple of 16): the achievable-HBM yardstick bench.py reports
 * every renderer kernel against. Not on the rendering path.      */
int avr_stream_copy(const void* src, void* dst, int64_t n_bytes, void* stream);

/* Streaming device fill: every 32-bit word of dst[0, n_bytes) = word (16-B
 * aligned, n_bytes a multiple of 16): the write-only yardstick (the ceiling
 * of store-dominated kernels such as the stratified sampler). Not on the
 * rendering path (ABI 10).                                                    */
int avr_stream_fill(void* dst, int64_t n_bytes, uint32_t word, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AVR_H_ */
