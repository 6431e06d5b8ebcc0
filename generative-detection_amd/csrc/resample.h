// The conv-less resamplers (ddconfig.resamp_with_conv = False): Downsample = F.avg_pool2d(x, 2, 2), Upsample = F.interpolate(scale 2,
// nearest) ([UPSTREAM] ldm .../model.py Downsample / Upsample), NHWC, shared by the f32 kernels (elementwise.hip) and the bf16 ones
// (bf16_ops.hip).  Include inside the file's anonymous namespace, after the vector policy V:
//   V::elem_t                       element type in HBM (float, or bf16 bits)
//   V::W                            elements per 16-byte vector (4 / 8)
//   V::load(const elem_t*, float (&)[W])     streaming 16-byte load, widened to f32
//   V::store(elem_t*, float (&)[W])          one rounding + streaming 16-byte store; leaves the values AS STORED in the array
// Every byte is touched once (non-temporal accesses, as the GroupNorm apply passes), all index arithmetic is 64-bit, no atomics.
//
// A ResnetBlock's norm1 reads a resampler's result next, so the forward kernels can leave its GroupNorm statistics the way the
// convs' epilogues do: partial [N][chunks][G][2] = (sum, sum of squares) of the stored values.  The pixels of the SMALL grid (the
// pooled output / the upsampler's input) of one sample are cut into `chunks` runs of pix_per_chunk; block (chunk, n) walks one run --
// thread = (channel vector q, pixel lane psub), as gn_stats_kernel -- and reduces its per-thread f32 sums the way that kernel does
// (LDS, per-channel totals, per-group partials).  A run past the end writes zeros: every slot of `partial` is written.
// The consumer fixes `chunks` (the conv kernels' tile counts: 2 per image at 32 x 32), so where chunks x N blocks would leave most of the chip
// idle a block takes only a SLICE of the channels -- whole groups, at least 128 bytes per pixel -- and blockIdx.z counts the slices: the
// statistics are per group, so every slot still has exactly one writer.
#pragma once

struct RsShape {
  int N, C, cslice, vecs, pix_per_pass;      // cslice: channels per block (blockIdx.z = slice), vecs = cslice / V::W, pix_per_pass = 256 / vecs
  int Hs, Ws;                        // the small grid
  int Hb, Wb;                        // the big one (avg-pool input, which may have an odd last row / column; upsampler output = 2 Hs x 2 Ws)
  int G, cpg, chunks;                // statistics: groups, channels per group; chunks per sample (also the grid's x extent)
  int64_t pix_per_chunk;
};

// per-thread sums -> partial[n][chunk][G][2] * scale.  red: [2][256 * W] floats.  All 256 threads call it.
template <int W>
__device__ __forceinline__ void rs_reduce_stats(const RsShape& s, const float (&sm)[W], const float (&sq)[W], float scale,
                                                float (*red)[256 * W], float* __restrict__ partial) {
  const int tid = threadIdx.x, q = tid % s.vecs, psub = tid / s.vecs;
  if (psub < s.pix_per_pass) {
#pragma unroll
    for (int j = 0; j < W; ++j) { red[0][psub * s.cslice + W * q + j] = sm[j]; red[1][psub * s.cslice + W * q + j] = sq[j]; }
  }
  __syncthreads();
  for (int c = tid; c < s.cslice; c += 256) {
    float a = 0.f, b = 0.f;
    for (int ps = 0; ps < s.pix_per_pass; ++ps) { a += red[0][ps * s.cslice + c]; b += red[1][ps * s.cslice + c]; }
    red[0][c] = a; red[1][c] = b;   // row 0 only read by its own writer in this loop
  }
  __syncthreads();
  if (tid < s.cslice / s.cpg) {     // the groups of this block's channel slice
    float a = 0.f, b = 0.f;
    for (int j = 0; j < s.cpg; ++j) { a += red[0][tid * s.cpg + j]; b += red[1][tid * s.cpg + j]; }
    float* o = partial + (((int64_t)blockIdx.y * s.chunks + blockIdx.x) * s.G + blockIdx.z * (s.cslice / s.cpg) + tid) * 2;
    o[0] = a * scale; o[1] = b * scale;
  }
}

// y[n][i][j] = 0.25 * ((x[2i][2j] + x[2i][2j+1]) + (x[2i+1][2j] + x[2i+1][2j+1])), f32 arithmetic, one rounding on the way out
template <typename V, bool STATS>
__global__ __launch_bounds__(256) void rs_avgpool_kernel(const typename V::elem_t* __restrict__ x, typename V::elem_t* __restrict__ y,
                                                         RsShape s, float* __restrict__ partial) {
  constexpr int W = V::W;
  __shared__ float red[STATS ? 2 : 1][STATS ? 256 * W : 1];
  const int tid = threadIdx.x, q = tid % s.vecs, psub = tid / s.vecs;
  const int64_t n = blockIdx.y, npix = (int64_t)s.Hs * s.Ws;
  const int c0 = blockIdx.z * s.cslice;
  const int64_t p_beg = (int64_t)blockIdx.x * s.pix_per_chunk;
  const int64_t p_end = p_beg + s.pix_per_chunk < npix ? p_beg + s.pix_per_chunk : npix;
  const int64_t row = (int64_t)s.Wb * s.C;
  float sm[W], sq[W];
#pragma unroll
  for (int j = 0; j < W; ++j) sm[j] = sq[j] = 0.f;
  if (psub < s.pix_per_pass)
    for (int64_t p = p_beg + psub; p < p_end; p += s.pix_per_pass) {
      const int64_t i = p / s.Ws, j0 = p % s.Ws;
      const typename V::elem_t* src = x + ((n * s.Hb + 2 * i) * s.Wb + 2 * j0) * s.C + c0 + W * q;
      float a[W], b[W], c[W], d[W];
      V::load(src, a); V::load(src + s.C, b); V::load(src + row, c); V::load(src + row + s.C, d);
#pragma unroll
      for (int j = 0; j < W; ++j) a[j] = 0.25f * ((a[j] + b[j]) + (c[j] + d[j]));
      V::store(y + (n * npix + p) * s.C + c0 + W * q, a);
      if constexpr (STATS) {
#pragma unroll
        for (int j = 0; j < W; ++j) { sm[j] += a[j]; sq[j] += a[j] * a[j]; }
      }
    }
  if constexpr (STATS) rs_reduce_stats<W>(s, sm, sq, 1.f, red, partial);
}

// u[n][2i+a][2j+b] = x[n][i][j]: one load, four stores.  The statistics of u are 4 x those of x (exact in f32): x is summed once.
template <typename V, bool STATS>
__global__ __launch_bounds__(256) void rs_upsample_kernel(const typename V::elem_t* __restrict__ x, typename V::elem_t* __restrict__ u,
                                                          RsShape s, float* __restrict__ partial) {
  constexpr int W = V::W;
  __shared__ float red[STATS ? 2 : 1][STATS ? 256 * W : 1];
  const int tid = threadIdx.x, q = tid % s.vecs, psub = tid / s.vecs;
  const int64_t n = blockIdx.y, npix = (int64_t)s.Hs * s.Ws;
  const int c0 = blockIdx.z * s.cslice;
  const int64_t p_beg = (int64_t)blockIdx.x * s.pix_per_chunk;
  const int64_t p_end = p_beg + s.pix_per_chunk < npix ? p_beg + s.pix_per_chunk : npix;
  const int64_t row = (int64_t)s.Wb * s.C;
  float sm[W], sq[W];
#pragma unroll
  for (int j = 0; j < W; ++j) sm[j] = sq[j] = 0.f;
  auto put = [&](int64_t p, float (&v)[W]) {
    const int64_t i = p / s.Ws, j0 = p % s.Ws;
    typename V::elem_t* dst = u + ((n * s.Hb + 2 * i) * s.Wb + 2 * j0) * s.C + c0 + W * q;
    V::store(dst, v); V::store(dst + s.C, v); V::store(dst + row, v); V::store(dst + row + s.C, v);
    if constexpr (STATS) {
#pragma unroll
      for (int j = 0; j < W; ++j) { sm[j] += v[j]; sq[j] += v[j] * v[j]; }
    }
  };
  if (psub < s.pix_per_pass) {
    const typename V::elem_t* xn = x + n * npix * s.C + c0 + W * q;
    const int64_t step = s.pix_per_pass;
    int64_t p = p_beg + psub;
    for (; p + 3 * step < p_end; p += 4 * step) {      // four loads in flight
      float v0[W], v1[W], v2[W], v3[W];
      V::load(xn + p * s.C, v0); V::load(xn + (p + step) * s.C, v1); V::load(xn + (p + 2 * step) * s.C, v2); V::load(xn + (p + 3 * step) * s.C, v3);
      put(p, v0); put(p + step, v1); put(p + 2 * step, v2); put(p + 3 * step, v3);
    }
    for (; p < p_end; p += step) {
      float v[W];
      V::load(xn + p * s.C, v);
      put(p, v);
    }
  }
  if constexpr (STATS) rs_reduce_stats<W>(s, sm, sq, 4.f, red, partial);
}

// dx[n][2i+a][2j+b] = 0.25 * dy[n][i][j]; dx comes uninitialised, so the thread of the last pooled column / row also writes the ZEROS of
// an odd input's dropped column / row (and the corner).  One thread per dy vector, grid-stride.
template <typename V>
__global__ __launch_bounds__(256) void rs_avgpool_bwd_kernel(const typename V::elem_t* __restrict__ dy, typename V::elem_t* __restrict__ dx, RsShape s) {
  constexpr int W = V::W;
  const int64_t total = (int64_t)s.N * s.Hs * s.Ws * s.vecs;
  const int64_t row = (int64_t)s.Wb * s.C;
  const bool odd_w = s.Wb > 2 * s.Ws, odd_h = s.Hb > 2 * s.Hs;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int q = (int)(idx % s.vecs);
    int64_t r = idx / s.vecs;
    const int64_t j0 = r % s.Ws; r /= s.Ws;
    const int64_t i = r % s.Hs, n = r / s.Hs;
    float v[W], z[W];
    V::load(dy + idx * W, v);
#pragma unroll
    for (int j = 0; j < W; ++j) { v[j] *= 0.25f; z[j] = 0.f; }
    typename V::elem_t* dst = dx + ((n * s.Hb + 2 * i) * s.Wb + 2 * j0) * s.C + W * q;
    V::store(dst, v); V::store(dst + s.C, v); V::store(dst + row, v); V::store(dst + row + s.C, v);
    const bool last_w = odd_w && j0 == s.Ws - 1, last_h = odd_h && i == s.Hs - 1;
    if (last_w) { V::store(dst + 2 * s.C, z); V::store(dst + row + 2 * s.C, z); }
    if (last_h) { V::store(dst + 2 * row, z); V::store(dst + 2 * row + s.C, z); }
    if (last_w && last_h) V::store(dst + 2 * row + 2 * s.C, z);
  }
}

// ---- host side ----
// shape of a launch over the small grid Hs x Ws; chunks = 0: no statistics, the launcher cuts the runs itself
static inline RsShape rs_shape(int N, int Hs, int Ws, int Hb, int Wb, int C, int W, int G, int chunks) {
  RsShape s;
  s.N = N; s.C = C; s.cslice = C;
  s.Hs = Hs; s.Ws = Ws; s.Hb = Hb; s.Wb = Wb;
  s.G = G > 0 ? G : 1; s.cpg = C / s.G;
  const int64_t npix = (int64_t)Hs * Ws;
  if (chunks > 0) {
    s.chunks = chunks;
    s.pix_per_chunk = ceil_div64(npix, chunks);
    // too few (chunk, n) blocks for the chip: halve the channel slice while it stays whole groups, whole vectors and >= 128 bytes per pixel
    const int min_slice = 128 * W / 16;
    while ((int64_t)N * chunks * (C / s.cslice) < 2048 && s.cslice % 2 == 0 && (s.cslice / 2) % s.cpg == 0 && (s.cslice / 2) % W == 0 &&
           s.cslice / 2 >= min_slice)
      s.cslice /= 2;
  } else {      // >= 4 pixels per thread, <= 16384 runs per sample
    s.pix_per_chunk = std::max<int64_t>(4 * (256 / (C / W)), ceil_div64(npix, 16384));
    s.chunks = (int)ceil_div64(npix, s.pix_per_chunk);
  }
  s.vecs = s.cslice / W; s.pix_per_pass = 256 / s.vecs;
  return s;
}

#define RS_CHECK_SHAPE(name, x, y, N, H, W, C, VW)                                                                                      \
  ODVAE_CHECK_ARG((x) && (y) && (N) > 0 && (N) <= 65535 && (H) > 0 && (W) > 0 && (C) > 0 && (C) % (VW) == 0 && (C) / (VW) <= 256,      \
                  name ": need C %% %d == 0, C <= %d, N <= 65535 (N=%d H=%d W=%d C=%d)", VW, 256 * (VW), N, H, W, C);                \
  ODVAE_CHECK_ARG((((uintptr_t)(x) | (uintptr_t)(y)) & 15) == 0, name ": operands must be 16-byte aligned")
#define RS_CHECK_STATS(name, gn_partial, gn_groups, chunks, C)                                                                          \
  ODVAE_CHECK_ARG(!(gn_partial) || ((gn_groups) > 0 && (gn_groups) <= 256 && (C) % (gn_groups) == 0 && (chunks) > 0),                  \
                  name ": statistics need 0 < gn_groups <= 256 dividing C and chunks > 0 (gn_groups=%d chunks=%d C=%d)", gn_groups, chunks, C)

template <typename V>
static int rs_avgpool(const void* x, void* y, int N, int H, int W, int C, float* gn_partial, int gn_groups, int chunks, void* stream) {
  RS_CHECK_SHAPE("avgpool2x2", x, y, N, H, W, C, V::W);
  ODVAE_CHECK_ARG(H >= 2 && W >= 2, "avgpool2x2: H, W >= 2 needed (H=%d W=%d)", H, W);
  RS_CHECK_STATS("avgpool2x2", gn_partial, gn_groups, chunks, C);
  const RsShape s = rs_shape(N, H / 2, W / 2, H, W, C, V::W, gn_partial ? gn_groups : 0, gn_partial ? chunks : 0);
  const dim3 grid(s.chunks, N, s.C / s.cslice), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto* xi = static_cast<const typename V::elem_t*>(x);
  auto* yo = static_cast<typename V::elem_t*>(y);
  if (gn_partial) hipLaunchKernelGGL((rs_avgpool_kernel<V, true>), grid, block, 0, st, xi, yo, s, gn_partial);
  else            hipLaunchKernelGGL((rs_avgpool_kernel<V, false>), grid, block, 0, st, xi, yo, s, gn_partial);
  ODVAE_LAUNCH_CHECK("avgpool2x2");
  return ODVAE_OK;
}

template <typename V>
static int rs_avgpool_bwd(const void* dy, void* dx, int N, int H, int W, int C, void* stream) {
  RS_CHECK_SHAPE("avgpool2x2_bwd", dy, dx, N, H, W, C, V::W);
  ODVAE_CHECK_ARG(H >= 2 && W >= 2, "avgpool2x2_bwd: H, W >= 2 needed (H=%d W=%d)", H, W);
  const RsShape s = rs_shape(N, H / 2, W / 2, H, W, C, V::W, 0, 0);
  const int64_t work = (int64_t)N * s.Hs * s.Ws * s.vecs;
  hipLaunchKernelGGL((rs_avgpool_bwd_kernel<V>), dim3((unsigned)std::min<int64_t>(ceil_div64(work, 256), 16384)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const typename V::elem_t*>(dy), static_cast<typename V::elem_t*>(dx), s);
  ODVAE_LAUNCH_CHECK("avgpool2x2_bwd");
  return ODVAE_OK;
}

template <typename V>
static int rs_upsample(const void* x, void* u, int N, int H, int W, int C, float* gn_partial, int gn_groups, int chunks, void* stream) {
  RS_CHECK_SHAPE("upsample2x", x, u, N, H, W, C, V::W);
  ODVAE_CHECK_ARG(H <= 0x3fffffff && W <= 0x3fffffff, "upsample2x: H, W too large (H=%d W=%d)", H, W);
  RS_CHECK_STATS("upsample2x", gn_partial, gn_groups, chunks, C);
  const RsShape s = rs_shape(N, H, W, 2 * H, 2 * W, C, V::W, gn_partial ? gn_groups : 0, gn_partial ? chunks : 0);
  const dim3 grid(s.chunks, N, s.C / s.cslice), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto* xi = static_cast<const typename V::elem_t*>(x);
  auto* uo = static_cast<typename V::elem_t*>(u);
  if (gn_partial) hipLaunchKernelGGL((rs_upsample_kernel<V, true>), grid, block, 0, st, xi, uo, s, gn_partial);
  else            hipLaunchKernelGGL((rs_upsample_kernel<V, false>), grid, block, 0, st, xi, uo, s, gn_partial);
  ODVAE_LAUNCH_CHECK("upsample2x");
  return ODVAE_OK;
}
