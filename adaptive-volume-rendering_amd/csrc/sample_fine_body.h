// The body of sample_fine_kernel and sample_fine_bounds_kernel (sampling.hip), included inside each after the kernel
// has set: lds (the dynamic LDS), lane, wid, ray (this wave's ray, a scalar < n_rays) and near_, far_ -- the launch's
// two scalars, or the ray's own bounds, which then also scale its importance samples, clamp its depth samples and
// seed its merge's first guess. Kept as text, not as a function: the scalar kernel compiles to the instructions it
// had before the per-ray kernel existed (an inlined function did not).
  const int Nc = NC ? NC : Nc_, Nf = NC ? NF : Nf_, Nd = NC ? ND : Nd_;
  const int Ntot = Nc + Nf + Nd;
  float* cdf = lds + (size_t)wid * fine_wave_floats(Nc, sort_n, Ntot);   // [0 .. Nc]
  float* scratch = cdf + Nc + 1;
  float* sbuf = scratch + 64;   // lists: coarse [0, Nc) | fine [Nc, Nc+Nf) | depth [Nc+Nf, Ntot)
  float* obuf = sbuf + sort_n;
  const float span = fsub(far_, near_);
  const uint64_t key = offset + (uint64_t)(ray_ids ? ray_ids[ray] : ray);   // Philox counter of this ray
  const float inv_nc = 1.0f / (float)Nc;

  // 1) + 2)
  const float* w = weights + ray * Nc;
  const float* zc = z_coarse + ray * Nc;
  bool coarse_sorted = true;
  float wv[kMaxK], zv[kMaxK];
#pragma unroll
  for (int m = 0; m < kMaxK; ++m) {
    const int k = lane + 64 * m;
    wv[m] = k < Nc ? w[k] : 0.f;
    zv[m] = k < Nc ? zc[k] : 0.f;
  }
  // the in-kernel (u, u2) draw of this lane's fine sample does not depend on
  // the weights: it runs while their loads are in flight (one sample per lane)
  float4 draw = {0.f, 0.f, 0.f, 0.f};
  if (!u_in && Nf <= 64 && lane < Nf) draw = philox_uniform4(seed, key, (uint32_t)lane, kStreamFine);
  float xr[kMaxK];
#pragma unroll
  for (int m = 0; m < kMaxK; ++m) {
    const int k = lane + 64 * m;
    xr[m] = 0.f;
    if (k < Nc) {
      xr[m] = fadd(wv[m], 1e-5f);
      cdf[1 + k] = xr[m];
      sbuf[k] = zv[m];
    }
  }
  float s;
  if ((Nc & 63) == 0) {
    s = cascade_sum_regs(xr, Nc >> 6, lane);
    wave_sync();
  } else {
    wave_sync();
    s = cascade_sum_wave(cdf + 1, Nc, lane, scratch);
  }
  for (int k = lane; k + 1 < Nc; k += 64) coarse_sorted &= sbuf[k] <= sbuf[k + 1];
  coarse_sorted = __all(coarse_sorted);
  {
    const int K = (Nc + 63) >> 6, k0 = K * lane;
    float pv[kMaxK];
    double part = 0.0;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      pv[k] = (k < K && k0 + k < Nc) ? fdiv(cdf[1 + k0 + k], s) : 0.f;
      part += (double)pv[k];
    }
    double run = wave_excl_sum_dpp(part);
    wave_sync();   // every pdf read before any cdf write
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
      if (k < K && k0 + k < Nc) {
        run += (double)pv[k];
        cdf[1 + k0 + k] = (float)run;
      }
    if (lane == 0) cdf[0] = 0.f;
  }
  wave_sync();

  // 3) importance samples
  float zf_mine = FLT_MAX;
  for (int f = lane; f < Nf; f += 64) {
    float u, u2;
    if (u_in) {
      u = u_in[ray * Nf + f];
      u2 = u2_in[ray * Nf + f];
    } else {
      const float4 v = Nf <= 64 ? draw : philox_uniform4(seed, key, (uint32_t)f, kStreamFine);
      u = v.x;
      u2 = v.y;
    }
    const int cnt = count_below<false>(cdf, Nc + 1, u);   // #{cdf <= u}
    const int idx = cnt > 0 ? cnt - 1 : 0;
    const float steps = div_count<POW2>(fadd((float)idx, u2), (float)Nc, inv_nc);
    const float zf = fadd(near_, fmul(span, steps));
    if (idx_out) idx_out[ray * Nf + f] = idx;
    if (z_fine_out) z_fine_out[ray * Nf + f] = zf;
    sbuf[Nc + f] = zf;
    zf_mine = zf;
  }
  // 4) depth samples: clamp(randn * std, near, far)  (quirk Q6)
  float zd_mine = FLT_MAX;
  for (int d = lane; d < Nd; d += 64) {
    const float n = nd_in ? nd_in[ray * Nd + d] : philox_normal(seed, key, d, kStreamDepth);
    zd_mine = fminf(fmaxf(fmul(n, depth_std), near_), far_);
    sbuf[Nc + Nf + d] = zd_mine;
  }
  wave_sync();

  // 5) sort
  float* out = z_sorted + ray * Ntot;
  if (coarse_sorted && Nf <= 64 && Nd == 0) {
    // two lists: the fine values take slots lane + #{A <= bf} (increasing in
    // lane); the coarse values fill the other slots in order. A slot's list
    // index = the number of fine slots before it (ballot + mbcnt) or the rest.
    const float* A = sbuf;
    float* B = sbuf + Nc;
    int* marks = reinterpret_cast<int*>(obuf);
    for (int k = lane; k < Ntot; k += 64) marks[k] = 0;
    const float bf = wave_sort64(zf_mine, lane);
    wave_sync();   // the unsorted fine list is read by nobody past this point
    if (lane < Nf) {
      B[lane] = bf;
      const float t = (bf - near_) * ((float)Nc * __builtin_amdgcn_rcpf(span));   // a guess: verified below
      const int g = t > 0.f ? (t < (float)Nc ? (int)t : Nc) : 0;
      marks[lane + count_below_near<false>(A, Nc, bf, g)] = 1;
    }
    wave_sync();
    int base = 0;
    for (int s0 = 0; s0 < Ntot; s0 += 64) {
      const int k = s0 + lane;
      const bool fine = k < Ntot && marks[k] != 0;
      const uint64_t mask = __ballot(fine);
      const int before = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                                               __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
      if (k < Ntot) out[k] = sbuf[fine ? Nc + before : k - before];   // B[before] or A[k - before]: one read
      base += __popcll(mask);
    }
    return;
  }
  if (coarse_sorted && Nf <= 64 && Nd <= 64) {
    const float* A = sbuf;
    float* B = sbuf + Nc;
    float* D = sbuf + Nc + Nf;
    const float bf = wave_sort64(zf_mine, lane);
    const float bd = Nd > 0 ? wave_sort64(zd_mine, lane) : FLT_MAX;
    wave_sync();   // the unsorted lists are read by nobody past this point
    if (lane < Nf) B[lane] = bf;
    if (lane < Nd) D[lane] = bd;
    wave_sync();
    for (int k = lane; k < Nc; k += 64) {
      const float x = A[k];
      obuf[k + count_below<true>(B, Nf, x) + count_below<true>(D, Nd, x)] = x;
    }
    if (lane < Nf) {
      // stratified coarse lists put #{A <= bf} within a step of bf's bin
      const float t = (bf - near_) * ((float)Nc * __builtin_amdgcn_rcpf(span));   // a guess: verified below
      const int g = t > 0.f ? (t < (float)Nc ? (int)t : Nc) : 0;
      obuf[lane + count_below_near<false>(A, Nc, bf, g) + count_below<true>(D, Nd, bf)] = bf;
    }
    if (lane < Nd) obuf[lane + count_below<false>(A, Nc, bd) + count_below<false>(B, Nf, bd)] = bd;
    wave_sync();
    for (int k = lane; k < Ntot; k += 64) out[k] = obuf[k];
    return;
  }
  for (int k = Ntot + lane; k < sort_n; k += 64) sbuf[k] = FLT_MAX;
  wave_sync();
  for (int size = 2; size <= sort_n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = lane; t < (sort_n >> 1); t += 64) {
        const int i = 2 * t - (t & (stride - 1));
        const int j = i + stride;
        const float a = sbuf[i], b = sbuf[j];
        const bool up = ((i & size) == 0);
        if ((a > b) == up) { sbuf[i] = b; sbuf[j] = a; }
      }
      wave_sync();
    }
  }
  for (int k = lane; k < Ntot; k += 64) out[k] = sbuf[k];
