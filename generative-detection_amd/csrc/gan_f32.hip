// PatchGAN discriminator support kernels, NHWC f32, gfx950.  All HBM-bound.
//
// [UPSTREAM] taming/modules/discriminator/model.py NLayerDiscriminator (reference call sites
// src/modules/losses/contperceptual.py:285,355-356): Conv2d(4x4, stride 2|1, pad 1) -> BatchNorm2d -> LeakyReLU(0.2).
// The 4x4 convolutions run as im2col + the f32 MFMA GEMM (gemm_f32.hip) -- BASELINE.json's north_star allows the matrix
// cores for "im2col dense contractions"; 288 GB of HBM makes the column matrices (<= 1 GB at B = 32) a non-issue.
//   fwd   cols = im2col(x)           y    = cols . W'^T     (W' = weight reordered to [Cout][kh][kw][Cin])
//   dgrad dcols = dy . W'            dx   = col2im(dcols)   (gather form: no atomics, deterministic)
//   wgrad dW'  = dy^T . cols
// BatchNorm2d uses batch statistics in training (biased variance for normalisation, unbiased for the running
// estimate, momentum 0.1) and is fused with the LeakyReLU that follows it.
#include "common.h"

namespace {

// cols[(n,oy,ox)][(kh*4+kw)*C + c] = x[n][oy*S-1+kh][ox*S-1+kw][c]  (zero outside)
__global__ __launch_bounds__(256) void im2col4x4_kernel(const float* __restrict__ x, float* __restrict__ cols,
                                                         int N, int Hi, int Wi, int C, int Ho, int Wo, int S) {
  const int64_t total = (int64_t)N * Ho * Wo * 16 * C;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    int64_t r = idx / C;
    const int tap = (int)(r % 16); r /= 16;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho); const int n = (int)(r / Ho);
    const int iy = oy * S - 1 + (tap >> 2), ix = ox * S - 1 + (tap & 3);
    float v = 0.f;
    if (iy >= 0 && iy < Hi && ix >= 0 && ix < Wi) v = x[(((int64_t)n * Hi + iy) * Wi + ix) * C + c];
    cols[idx] = v;
  }
}

// dx[n][iy][ix][c] = sum over taps (kh,kw) with (iy+1-kh) % S == 0 of dcols[(n,(iy+1-kh)/S,(ix+1-kw)/S)][(kh*4+kw)*C+c]
__global__ __launch_bounds__(256) void col2im4x4_kernel(const float* __restrict__ dcols, float* __restrict__ dx,
                                                         int N, int Hi, int Wi, int C, int Ho, int Wo, int S) {
  const int64_t total = (int64_t)N * Hi * Wi * C;
  const int K = 16 * C;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    int64_t r = idx / C;
    const int ix = (int)(r % Wi); r /= Wi;
    const int iy = (int)(r % Hi); const int n = (int)(r / Hi);
    float s = 0.f;
#pragma unroll
    for (int kh = 0; kh < 4; ++kh) {
      const int ty = iy + 1 - kh;
      if (ty < 0 || ty % S != 0) continue;
      const int oy = ty / S;
      if (oy >= Ho) continue;
#pragma unroll
      for (int kw = 0; kw < 4; ++kw) {
        const int tx = ix + 1 - kw;
        if (tx < 0 || tx % S != 0) continue;
        const int ox = tx / S;
        if (ox >= Wo) continue;
        s += dcols[(((int64_t)n * Ho + oy) * Wo + ox) * K + (kh * 4 + kw) * C + c];
      }
    }
    dx[idx] = s;
  }
}

// OIHW [Cout][Cin][4][4] <-> GEMM layout [Cout][(kh*4+kw)*Cin + ci]
__global__ void weight4x4_reorder_kernel(const float* __restrict__ src, float* __restrict__ dst, int Cout, int Cin, int to_gemm) {
  const int64_t total = (int64_t)Cout * Cin * 16;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    // idx enumerates the OIHW side
    const int tap = (int)(idx % 16);
    const int ci = (int)((idx / 16) % Cin);
    const int co = (int)(idx / (16 * (int64_t)Cin));
    const int64_t g = ((int64_t)co * 16 + tap) * Cin + ci;
    if (to_gemm) dst[g] = src[idx]; else dst[idx] = src[g];
  }
}

// ---- per-channel statistics over rows of an [M][C] matrix (shared by BN forward and backward) ---------------
// part[blk][2][C]: sums of f1 and f2 per channel, where (f1,f2) = (d, d^2), d = x - x[0][c], for MODE 0 and
// (g, g*xhat) for MODE 1 with g = dy * lrelu'(u), u = xhat*gamma+beta.
// MODE 0 sums about a pivot, the channel's value in row 0: the PatchGAN convolutions have no bias and read LeakyReLU outputs, so a
// channel's mean can lie many standard deviations from zero, and var = E[x^2] - E[x]^2 from f32 sums of x and x^2 loses ~ 2^-24 r^2 of
// the variance, r = |mean| / std (from r = 64 on rstd was outside the tests' rule at every shape; at r >= 256 no variance was left).
// d is of the size of the spread whatever the mean is, and x - pivot is exact for neighbouring values.  The pivot is one sample: if it
// lies k standard deviations from the channel's mean the sums lose ~ 2^-24 k^2 again, so this holds for channels whose row 0 is no far
// outlier (k of a few, as for any light-tailed activation), not for a value planted hundreds of deviations out
// (tests/test_batchnorm_offset_gpu.py, profiles/bn_offset.md).
template <int MODE>
__global__ __launch_bounds__(256) void bn_colstats_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float slope, int64_t rows, int C, int rows_per_block,
                                                          float* __restrict__ part) {
  __shared__ float sh[2][256];
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = std::min<int64_t>(rows, r0 + rows_per_block);
  for (int cbase = 0; cbase < C; cbase += 256) {
    const int cw = min(256, C - cbase);
    const int lanes = 256 / cw;
    const int c = cbase + threadIdx.x % cw, rl = threadIdx.x / cw;
    float a = 0.f, b = 0.f;
    if (rl < lanes) {
      float mu = 0.f, rs = 0.f, ga = 0.f, be = 0.f, pivot = 0.f;
      if (MODE == 1) { mu = mean[c]; rs = rstd[c]; ga = gamma[c]; be = beta[c]; }
      else pivot = x[c];
      for (int64_t r = r0 + rl; r < r1; r += lanes) {
        const float v = x[r * C + c];
        if (MODE == 0) { const float d = v - pivot; a += d; b += d * d; }
        else {
          const float xh = (v - mu) * rs;
          const float u = xh * ga + be;
          const float g = dy[r * C + c] * (u > 0.f ? 1.f : slope);
          a += g; b += g * xh;
        }
      }
    }
    sh[0][threadIdx.x] = a; sh[1][threadIdx.x] = b;
    __syncthreads();
    if (threadIdx.x < cw) {
      float ta = 0.f, tb = 0.f;
      for (int k = 0; k < lanes; ++k) { ta += sh[0][k * cw + threadIdx.x]; tb += sh[1][k * cw + threadIdx.x]; }
      part[((int64_t)blockIdx.x * 2 + 0) * C + cbase + threadIdx.x] = ta;
      part[((int64_t)blockIdx.x * 2 + 1) * C + cbase + threadIdx.x] = tb;
    }
    __syncthreads();
  }
}

// training-mode forward statistics: mean, rstd and the running estimates (momentum update, unbiased variance) from the sums about
// the pivot x[0][c]: mean = pivot + E[d], var = E[d^2] - E[d]^2
__global__ void bn_finalize_kernel(const float* __restrict__ part, const float* __restrict__ x, int nblk, int C, int64_t rows, float eps, float momentum,
                                   float* __restrict__ mean, float* __restrict__ rstd,
                                   float* __restrict__ running_mean, float* __restrict__ running_var) {
  // one wavefront per channel: the partials are summed lane-strided in f64, then by a fixed butterfly (deterministic).  One thread per
  // channel walking all nblk partials was a chain of ~1 000 dependent loads: 125 us per launch for 4 KB of output.
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (int k = lane; k < nblk; k += 64) { a += (double)part[((int64_t)k * 2 + 0) * C + c]; b += (double)part[((int64_t)k * 2 + 1) * C + c]; }
  a = wave_sum_f64(a); b = wave_sum_f64(b);
  if (lane != 0) return;
  const double m = (double)rows;
  const double dm = a / m;
  const double mu = (double)x[c] + dm;
  double var = b / m - dm * dm;
  if (var < 0.0) var = 0.0;
  mean[c] = (float)mu;
  rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) {
    const double unbiased = rows > 1 ? var * m / (m - 1.0) : var;
    running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mu);
    running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unbiased);
  }
}

// sums[2][C] = column totals of the partials (backward: sum g, sum g*xhat)
__global__ void bn_sum_partials_kernel(const float* __restrict__ part, int nblk, int C, float* __restrict__ sums) {
  const int lane = threadIdx.x & 63;      // one wavefront per (which, channel), as bn_finalize_kernel
  const int idx = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (idx >= 2 * C) return;
  const int which = idx / C, c = idx % C;
  double a = 0.0;
  for (int k = lane; k < nblk; k += 64) a += (double)part[((int64_t)k * 2 + which) * C + c];
  a = wave_sum_f64(a);
  if (lane == 0) sums[idx] = (float)a;
}

// ---- synchronised BatchNorm: the statistics and the backward sums of one rank as f64 records, merged over ranks in index order -------
// record[c] = {rows, mean_c, M2_c}, M2 = sum (x - mean_c)^2, from the partials of bn_colstats_kernel<0> about the pivot x[0][c]:
// mean = pivot + a / m, M2 = b - a^2 / m.  One wavefront per channel, f64, the order of bn_finalize_kernel.
__global__ void bn_record_kernel(const float* __restrict__ part, const float* __restrict__ x, int nblk, int C, int64_t rows,
                                 double* __restrict__ record) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (int k = lane; k < nblk; k += 64) { a += (double)part[((int64_t)k * 2 + 0) * C + c]; b += (double)part[((int64_t)k * 2 + 1) * C + c]; }
  a = wave_sum_f64(a); b = wave_sum_f64(b);
  if (lane != 0) return;
  const double m = (double)rows;
  const double dm = a / m;
  double m2 = b - a * dm;
  if (m2 < 0.0) m2 = 0.0;
  record[(int64_t)c * 3 + 0] = m;
  record[(int64_t)c * 3 + 1] = (double)x[c] + dm;
  record[(int64_t)c * 3 + 2] = m2;
}

// records[world][C][3] -> mean, rstd and the running estimates of the union of the ranks' rows.  The records are merged pairwise in
// index order by Chan's update (delta = mean_b - mean_a, M2 = M2_a + M2_b + delta^2 n_a n_b / n), one thread per channel, all in f64:
// every rank that holds the same records gets the same bits.  The running variance is the unbiased one over the TOTAL count.
__global__ void bn_merge_records_kernel(const double* __restrict__ records, int world, int C, float eps, float momentum,
                                        float* __restrict__ mean, float* __restrict__ rstd,
                                        float* __restrict__ running_mean, float* __restrict__ running_var,
                                        double* __restrict__ total_rows) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double n = records[(int64_t)c * 3 + 0], mu = records[(int64_t)c * 3 + 1], m2 = records[(int64_t)c * 3 + 2];
  for (int w = 1; w < world; ++w) {
    const double* r = records + ((int64_t)w * C + c) * 3;
    const double nb = r[0], nt = n + nb;
    const double delta = r[1] - mu;
    mu += delta * (nb / nt);
    m2 += r[2] + delta * delta * (n * nb / nt);
    n = nt;
  }
  if (c == 0 && total_rows) *total_rows = n;      // the count is the same in every channel
  double var = m2 / n;
  if (var < 0.0) var = 0.0;
  mean[c] = (float)mu;
  rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) {
    const double unbiased = n > 1.0 ? var * n / (n - 1.0) : var;
    running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mu);
    running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unbiased);
  }
}

// bn_sum_partials_kernel that keeps the f64 totals: sums64[2][C] = (sum g, sum g*xhat) for the exchange; dbeta, dgamma are their f32
// roundings, the values the unsynchronised backward returns
__global__ void bn_sum_partials_f64_kernel(const float* __restrict__ part, int nblk, int C, double* __restrict__ sums64,
                                           float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int lane = threadIdx.x & 63;
  const int idx = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (idx >= 2 * C) return;
  const int which = idx / C, c = idx % C;
  double a = 0.0;
  for (int k = lane; k < nblk; k += 64) a += (double)part[((int64_t)k * 2 + which) * C + c];
  a = wave_sum_f64(a);
  if (lane != 0) return;
  sums64[idx] = a;
  if (which == 0) dbeta[c] = (float)a; else dgamma[c] = (float)a;
}

// sums[2][C] (f32, what bn_lrelu_bwd_apply_kernel reads) = the ranks' sums64[world][2][C] added in index order in f64
__global__ void bn_merge_sums_kernel(const double* __restrict__ sums64, int world, int C, float* __restrict__ sums) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * C) return;
  double a = sums64[idx];
  for (int w = 1; w < world; ++w) a += sums64[(int64_t)w * 2 * C + idx];
  sums[idx] = (float)a;
}

// y = lrelu((x-mean)*rstd*gamma+beta)
__global__ __launch_bounds__(256) void bn_lrelu_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float slope, int64_t total, int C,
                                                             float* __restrict__ y) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    const float u = (x[idx] - mean[c]) * rstd[c] * gamma[c] + beta[c];
    y[idx] = u > 0.f ? u : slope * u;
  }
}

// training: dx = gamma*rstd/M * (M*g - sum_g - xhat*sum_gxhat); eval (train=0): dx = gamma*rstd*g.  M = m: the rows the sums were
// taken over -- `rows`, or *m_total (device), all ranks' rows, when the sums are the merged ones (synchronised BatchNorm)
__global__ __launch_bounds__(256) void bn_lrelu_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                 const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 const float* __restrict__ sums, float slope, int64_t rows, const double* __restrict__ m_total,
                                                                 int C, int train, float* __restrict__ dx) {
  const int64_t total = rows * C;
  const float inv_m = 1.f / (m_total ? (float)*m_total : (float)rows);
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    const float xh = (x[idx] - mean[c]) * rstd[c];
    const float u = xh * gamma[c] + beta[c];
    const float g = dy[idx] * (u > 0.f ? 1.f : slope);
    float v = g;
    if (train) v = g - (sums[c] + xh * sums[C + c]) * inv_m;
    dx[idx] = gamma[c] * rstd[c] * v;
  }
}

__global__ __launch_bounds__(256) void lrelu_kernel(const float* __restrict__ x, float* __restrict__ y, float slope, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = x[i];
    y[i] = v > 0.f ? v : slope * v;
  }
}
// dx = dy * (x > 0 ? 1 : slope); with slope = 0 this is the ReLU backward given the pre- or post-activation
__global__ __launch_bounds__(256) void lrelu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                        float* __restrict__ dx, float slope, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dx[i] = dy[i] * (x[i] > 0.f ? 1.f : slope);
}

// ---- ActNorm + LeakyReLU ([UPSTREAM] taming/modules/util.py ActNorm, NLayerDiscriminator(use_actnorm=True)) -----------------------
// h = scale[c] * (x + loc[c]), y = lrelu(h).  loc and scale are parameters: nothing is reduced in the forward, and in the backward dx
// does not depend on the parameter sums, so the activations are read once (BatchNorm in training mode: 3 tensor passes forward, 5
// backward; here 2 and 3).  V = 4: 16-byte accesses (C % 4 == 0 and 16-byte aligned pointers, every real layer); V = 1: scalar.
template <int V> struct an_vec;
template <> struct an_vec<1> { typedef float type; };
template <> struct an_vec<4> { typedef f32x4 type; };
template <int V> __device__ __forceinline__ void an_load(const float* p, float (&v)[V]) {
  const typename an_vec<V>::type t = *reinterpret_cast<const typename an_vec<V>::type*>(p);
  if constexpr (V == 1) v[0] = t; else { v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
}
template <int V> __device__ __forceinline__ void an_store(float* p, const float (&v)[V]) {
  typename an_vec<V>::type t;
  if constexpr (V == 1) t = v[0]; else { t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3]; }
  *reinterpret_cast<typename an_vec<V>::type*>(p) = t;
}

// BWD = 0: y = lrelu(scale * (x + loc)).  BWD = 1 (neither parameter needs a gradient): dx = scale * dy * lrelu'(scale * (x + loc)).
// Both evaluate h by the same two f32 operations, so the backward sees the sign the forward saw.
template <int V, int BWD>
__global__ __launch_bounds__(256) void an_lrelu_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                       const float* __restrict__ loc, const float* __restrict__ scale, float slope,
                                                       int64_t total_v, int CV, float* __restrict__ out) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total_v; idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % CV) * V;
    float xv[V], lo[V], sc[V], dv[V], o[V];
    an_load<V>(x + idx * V, xv); an_load<V>(loc + c, lo); an_load<V>(scale + c, sc);
    if (BWD) an_load<V>(dy + idx * V, dv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float h = sc[j] * (xv[j] + lo[j]);
      o[j] = BWD ? sc[j] * (dv[j] * (h > 0.f ? 1.f : slope)) : (h > 0.f ? h : slope * h);
    }
    an_store<V>(out + idx * V, o);
  }
}

// One pass over x and dy: dx = scale * g, g = dy * lrelu'(h), and part[blk][2][C] = the block's sums of g and of g * (x + loc).
// A thread keeps one channel (V = 4: four adjacent ones) and walks every `lanes`-th row of the block's row range, as bn_colstats_kernel.
template <int V>
__global__ __launch_bounds__(256) void an_lrelu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                           const float* __restrict__ loc, const float* __restrict__ scale, float slope,
                                                           int64_t rows, int C, int rows_per_block, float* __restrict__ dx,
                                                           float* __restrict__ part) {
  __shared__ float sh[2][V][256];
  const int CV = C / V;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = std::min<int64_t>(rows, r0 + rows_per_block);
  for (int cbase = 0; cbase < CV; cbase += 256) {
    const int cw = min(256, CV - cbase);
    const int lanes = 256 / cw;
    const int c = (cbase + threadIdx.x % cw) * V, rl = threadIdx.x / cw;
    float a[V], b[V];
#pragma unroll
    for (int j = 0; j < V; ++j) a[j] = b[j] = 0.f;
    if (rl < lanes) {
      float lo[V], sc[V];
      an_load<V>(loc + c, lo); an_load<V>(scale + c, sc);
      for (int64_t r = r0 + rl; r < r1; r += lanes) {
        float xv[V], dv[V], o[V];
        an_load<V>(x + r * C + c, xv); an_load<V>(dy + r * C + c, dv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float t = xv[j] + lo[j];
          const float h = sc[j] * t;
          const float g = dv[j] * (h > 0.f ? 1.f : slope);
          a[j] += g; b[j] += g * t;
          o[j] = sc[j] * g;
        }
        an_store<V>(dx + r * C + c, o);
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) { sh[0][j][threadIdx.x] = a[j]; sh[1][j][threadIdx.x] = b[j]; }
    __syncthreads();
    if (threadIdx.x < cw) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float ta = 0.f, tb = 0.f;
        for (int k = 0; k < lanes; ++k) { ta += sh[0][j][k * cw + threadIdx.x]; tb += sh[1][j][k * cw + threadIdx.x]; }
        part[((int64_t)blockIdx.x * 2 + 0) * C + (cbase + threadIdx.x) * V + j] = ta;
        part[((int64_t)blockIdx.x * 2 + 1) * C + (cbase + threadIdx.x) * V + j] = tb;
      }
    }
    __syncthreads();
  }
}

// dloc = scale * sum g, dscale = sum g (x + loc): one wavefront per (which, channel), f64, fixed butterfly (as bn_sum_partials_kernel)
__global__ void an_sum_partials_kernel(const float* __restrict__ part, const float* __restrict__ scale, int nblk, int C,
                                       float* __restrict__ dloc, float* __restrict__ dscale) {
  const int lane = threadIdx.x & 63;
  const int idx = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (idx >= 2 * C) return;
  const int which = idx / C, c = idx % C;
  double a = 0.0;
  for (int k = lane; k < nblk; k += 64) a += (double)part[((int64_t)k * 2 + which) * C + c];
  a = wave_sum_f64(a);
  if (lane != 0) return;
  if (which == 0) dloc[c] = (float)((double)scale[c] * a); else dscale[c] = (float)a;
}

// data-dependent initialisation from the partials of bn_colstats_kernel<0> (sums of d and d^2 about the pivot x[0][c]):
// loc = -mean, scale = 1 / (std + eps) with the unbiased (rows - 1) std, written into the parameters' own storage.
// One wavefront per channel, f64, as bn_finalize_kernel.
__global__ void an_init_finalize_kernel(const float* __restrict__ part, const float* __restrict__ x, int nblk, int C, int64_t rows, float eps,
                                        float* __restrict__ loc, float* __restrict__ scale) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (int k = lane; k < nblk; k += 64) { a += (double)part[((int64_t)k * 2 + 0) * C + c]; b += (double)part[((int64_t)k * 2 + 1) * C + c]; }
  a = wave_sum_f64(a); b = wave_sum_f64(b);
  if (lane != 0) return;
  const double m = (double)rows;
  const double dm = a / m;
  double var = (b - a * dm) / (m - 1.0);
  if (var < 0.0) var = 0.0;
  loc[c] = (float)(-((double)x[c] + dm));
  scale[c] = (float)(1.0 / (sqrt(var) + (double)eps));
}

// blocks of the one-pass backward: ~16 rows per thread, at most 1024 blocks (the partials stay a few per cent of the tensor)
int an_bwd_blocks(int64_t rows, int C, int V) {
  const int lanes = 256 / std::min(C / V, 256);
  return (int)std::min<int64_t>(std::max<int64_t>(rows / (16 * (int64_t)lanes), 1), 1024);
}
bool an_vec4(int C, const void* a, const void* b, const void* c, const void* d, const void* e) {
  return C % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & 15) == 0;
}

// ---- the scalar terms of the GAN losses over the discriminator's logits ([UPSTREAM] ldm contperceptual.py LPIPSWithDiscriminator.forward,
// taming vqperceptual.py hinge_d_loss / vanilla_d_loss) ------------------------------------------------------------------------------------
// out6 = [mean real, mean fake, mean relu(1 - real), mean relu(1 + fake), mean softplus(-real), mean softplus(fake)].
// The logits are a few thousand values (N x 30 x 30 at 256 x 256), so every term is taken in f64 from the f32 logit: sums of logits that
// are multiples of 2^-k are exact, and the softplus / sigmoid terms reach the result rounded once.  Three stages, all in a fixed order (no
// atomics): wave shuffles, LDS across the four waves of a block, partial[block][6] in the workspace, one final block.
constexpr int kLogitBlocks = 1024;      // grid cap of the partial stage: past 1024 * 256 logits a thread loops
int logit_blocks(int64_t n_real, int64_t n_fake) { return grid_1d(std::max(n_real, n_fake), kLogitBlocks); }

// comparisons, not fmax: a NaN logit stays a NaN in each of its terms
__device__ __forceinline__ double relu_f64(double t) { return t < 0.0 ? 0.0 : t; }
// max(x, 0) + log1p(exp(-|x|)): no overflow at +100, no cancellation at -100 (torch's thresholded form to rounding)
__device__ __forceinline__ double softplus_f64(double x) { return relu_f64(x) + log1p(exp(-fabs(x))); }
__device__ __forceinline__ double sigmoid_f64(double x) {
  if (x >= 0.0) return 1.0 / (1.0 + exp(-x));
  const double e = exp(x);      // (a NaN comes this way and stays one)
  return e / (1.0 + e);
}

__global__ __launch_bounds__(256) void logit_terms_partial_kernel(const float* __restrict__ real, int64_t n_real, const float* __restrict__ fake,
                                                                  int64_t n_fake, double* __restrict__ part) {
  __shared__ double sh[4][6];
  double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = i0; i < n_real; i += step) {
    const double x = (double)real[i];
    a[0] += x; a[2] += relu_f64(1.0 - x); a[4] += softplus_f64(-x);
  }
  for (int64_t i = i0; i < n_fake; i += step) {
    const double x = (double)fake[i];
    a[1] += x; a[3] += relu_f64(1.0 + x); a[5] += softplus_f64(x);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    a[k] = wave_sum_f64(a[k]);
    if (lane == 0) sh[wave][k] = a[k];
  }
  __syncthreads();
  if (threadIdx.x < 6) part[(int64_t)blockIdx.x * 6 + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}
// one block of six waves, wave k sums term k over the blocks; the division by n in f64, then the one rounding to f32
__global__ __launch_bounds__(384) void logit_terms_final_kernel(const double* __restrict__ part, int nblk, int64_t n_real, int64_t n_fake,
                                                                float* __restrict__ out6) {
  const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
  double s = 0.0;
  for (int i = lane; i < nblk; i += 64) s += part[(int64_t)i * 6 + k];
  s = wave_sum_f64(s);
  if (lane != 0) return;
  const int64_t n = (k & 1) ? n_fake : n_real;
  out6[k] = n > 0 ? (float)(s / (double)n) : 0.f;
}
// d mean / d x = 1 / n; relu'(0) = 0 (strict inequalities, as torch); softplus' = sigmoid.  dout6 is read on the device.
__global__ __launch_bounds__(256) void logit_terms_bwd_kernel(const float* __restrict__ real, int64_t n_real, const float* __restrict__ fake,
                                                              int64_t n_fake, const float* __restrict__ dout6, float* __restrict__ dreal,
                                                              float* __restrict__ dfake) {
  const double d0 = (double)dout6[0], d1 = (double)dout6[1], d2 = (double)dout6[2], d3 = (double)dout6[3], d4 = (double)dout6[4], d5 = (double)dout6[5];
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
  if (dreal) {
    for (int64_t i = i0; i < n_real; i += step) {
      const double x = (double)real[i];
      dreal[i] = (float)((d0 - (x < 1.0 ? d2 : 0.0) - d4 * sigmoid_f64(-x)) / (double)n_real);
    }
  }
  if (dfake) {
    for (int64_t i = i0; i < n_fake; i += step) {
      const double x = (double)fake[i];
      dfake[i] = (float)((d1 + (x > -1.0 ? d3 : 0.0) + d5 * sigmoid_f64(x)) / (double)n_fake);
    }
  }
}

}  // namespace

extern "C" {

int odvae_im2col4x4_f32(const float* x, float* cols, int N, int Hi, int Wi, int C, int Ho, int Wo, int stride, void* stream) {
  ODVAE_CHECK_ARG(x && cols && N > 0 && C > 0 && (stride == 1 || stride == 2), "im2col4x4: bad arguments");
  // Hi, Wi >= 2: the padded image holds the 4x4 window (and (Hi - 2) / stride is no truncation of a negative number)
  ODVAE_CHECK_ARG(Hi >= 2 && Wi >= 2 && Ho == (Hi - 2) / stride + 1 && Wo == (Wi - 2) / stride + 1, "im2col4x4: Ho/Wo do not match k=4, pad=1, stride=%d", stride);
  hipLaunchKernelGGL(im2col4x4_kernel, dim3(grid_1d((int64_t)N * Ho * Wo * 16 * C, 16384)), dim3(256), 0, static_cast<hipStream_t>(stream), x, cols, N, Hi, Wi, C, Ho, Wo, stride);
  ODVAE_LAUNCH_CHECK("im2col4x4");
  return ODVAE_OK;
}

int odvae_col2im4x4_f32(const float* dcols, float* dx, int N, int Hi, int Wi, int C, int Ho, int Wo, int stride, void* stream) {
  ODVAE_CHECK_ARG(dcols && dx && N > 0 && C > 0 && Hi > 0 && Wi > 0 && (stride == 1 || stride == 2), "col2im4x4: bad arguments");
  ODVAE_CHECK_ARG(Hi >= 2 && Wi >= 2 && Ho == (Hi - 2) / stride + 1 && Wo == (Wi - 2) / stride + 1, "col2im4x4: Ho/Wo do not match k=4, pad=1, stride=%d", stride);
  hipLaunchKernelGGL(col2im4x4_kernel, dim3(grid_1d((int64_t)N * Hi * Wi * C, 16384)), dim3(256), 0, static_cast<hipStream_t>(stream), dcols, dx, N, Hi, Wi, C, Ho, Wo, stride);
  ODVAE_LAUNCH_CHECK("col2im4x4");
  return ODVAE_OK;
}

// to_gemm = 1: OIHW -> [Cout][(kh,kw,ci)]; to_gemm = 0: the inverse (weight gradients back to OIHW)
int odvae_weight4x4_reorder_f32(const float* src, float* dst, int Cout, int Cin, int to_gemm, void* stream) {
  ODVAE_CHECK_ARG(src && dst && Cout > 0 && Cin > 0, "weight4x4_reorder: bad arguments");
  hipLaunchKernelGGL(weight4x4_reorder_kernel, dim3(grid_1d((int64_t)Cout * Cin * 16)), dim3(256), 0, static_cast<hipStream_t>(stream), src, dst, Cout, Cin, to_gemm);
  ODVAE_LAUNCH_CHECK("weight4x4_reorder");
  return ODVAE_OK;
}

size_t odvae_batchnorm_workspace_bytes(int64_t rows, int C) { return ((size_t)stat_blocks(rows) * 2 * C + 2 * C) * sizeof(float); }

// x,y: [rows][C] (NHWC flattened).  train=1: batch statistics into mean/rstd (+ running stats update when given);
// train=0: mean/rstd must already hold the running estimates (rstd = 1/sqrt(running_var+eps)).
int odvae_batchnorm_lrelu_fwd_f32(const float* x, int64_t rows, int C, const float* gamma, const float* beta, float eps,
                                  float momentum, float slope, int train, float* mean, float* rstd,
                                  float* running_mean, float* running_var, float* y,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && gamma && beta && mean && rstd && y && rows > 0 && C > 0, "batchnorm_lrelu_fwd: bad arguments");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (train) {
    const size_t need = odvae_batchnorm_workspace_bytes(rows, C);
    if (!workspace || workspace_bytes < need) { odvae_set_error("batchnorm_lrelu_fwd: needs %zu workspace bytes", need); return ODVAE_ERR_WORKSPACE; }
    float* part = static_cast<float*>(workspace);
    const int nblk = stat_blocks(rows);
    const int rpb = (int)ceil_div64(rows, nblk);
    const int nb = (int)ceil_div64(rows, rpb);
    hipLaunchKernelGGL((bn_colstats_kernel<0>), dim3(nb), dim3(256), 0, st, x, nullptr, nullptr, nullptr, nullptr, nullptr, slope, rows, C, rpb, part);
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(ceil_div(C, 4)), dim3(256), 0, st, part, x, nb, C, rows, eps, momentum, mean, rstd, running_mean, running_var);
  }
  hipLaunchKernelGGL(bn_lrelu_apply_kernel, dim3(grid_1d(rows * C)), dim3(256), 0, st, x, mean, rstd, gamma, beta, slope, rows * C, C, y);
  ODVAE_LAUNCH_CHECK("batchnorm_lrelu_fwd");
  return ODVAE_OK;
}

int odvae_batchnorm_lrelu_bwd_f32(const float* x, const float* dy, int64_t rows, int C, const float* gamma, const float* beta,
                                  const float* mean, const float* rstd, float slope, int train,
                                  float* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && dy && gamma && beta && mean && rstd && dx && dgamma && dbeta && rows > 0 && C > 0, "batchnorm_lrelu_bwd: bad arguments");
  const size_t need = odvae_batchnorm_workspace_bytes(rows, C);
  if (!workspace || workspace_bytes < need) { odvae_set_error("batchnorm_lrelu_bwd: needs %zu workspace bytes", need); return ODVAE_ERR_WORKSPACE; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  const int nblk = stat_blocks(rows);
  const int rpb = (int)ceil_div64(rows, nblk);
  const int nb = (int)ceil_div64(rows, rpb);
  float* sums = part + (size_t)nblk * 2 * C;
  hipLaunchKernelGGL((bn_colstats_kernel<1>), dim3(nb), dim3(256), 0, st, x, dy, mean, rstd, gamma, beta, slope, rows, C, rpb, part);
  hipLaunchKernelGGL(bn_sum_partials_kernel, dim3(ceil_div(2 * C, 4)), dim3(256), 0, st, part, nb, C, sums);
  // dbeta = sum g ; dgamma = sum g*xhat
  hipMemcpyAsync(dbeta, sums, (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, st);
  hipMemcpyAsync(dgamma, sums + C, (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, st);
  hipLaunchKernelGGL(bn_lrelu_bwd_apply_kernel, dim3(grid_1d(rows * C)), dim3(256), 0, st, x, dy, mean, rstd, gamma, beta, sums, slope, rows, nullptr, C, train, dx);
  ODVAE_LAUNCH_CHECK("batchnorm_lrelu_bwd");
  return ODVAE_OK;
}

// ---- synchronised BatchNorm + LeakyReLU: the forward and the backward cut where the ranks exchange ---------------------------------
// forward: stats_record (each rank) -> exchange -> stats_merge -> odvae_batchnorm_lrelu_fwd_f32(train = 0) with the merged mean / rstd;
// backward: bwd_sums (each rank) -> exchange -> bwd_dx.  Workspace of the three that take one: odvae_batchnorm_workspace_bytes(rows, C).
size_t odvae_batchnorm_sync_record_bytes(int C) { return (size_t)C * 3 * sizeof(double); }
size_t odvae_batchnorm_sync_sums_bytes(int C) { return (size_t)C * 2 * sizeof(double); }

int odvae_batchnorm_sync_stats_record_f32(const float* x, int64_t rows, int C, double* record, size_t record_bytes,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && rows > 0 && C > 0, "batchnorm_sync_stats_record: bad arguments");
  const size_t need_rec = odvae_batchnorm_sync_record_bytes(C);
  if (!record || record_bytes < need_rec) { odvae_set_error("batchnorm_sync_stats_record: the record needs %zu bytes", need_rec); return ODVAE_ERR_WORKSPACE; }
  const size_t need = odvae_batchnorm_workspace_bytes(rows, C);
  if (!workspace || workspace_bytes < need) { odvae_set_error("batchnorm_sync_stats_record: needs %zu workspace bytes", need); return ODVAE_ERR_WORKSPACE; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  const int nblk = stat_blocks(rows);
  const int rpb = (int)ceil_div64(rows, nblk);
  const int nb = (int)ceil_div64(rows, rpb);
  hipLaunchKernelGGL((bn_colstats_kernel<0>), dim3(nb), dim3(256), 0, st, x, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, rows, C, rpb, part);
  hipLaunchKernelGGL(bn_record_kernel, dim3(ceil_div(C, 4)), dim3(256), 0, st, part, x, nb, C, rows, record);
  ODVAE_LAUNCH_CHECK("batchnorm_sync_stats_record");
  return ODVAE_OK;
}

// records: [world][C][3] f64, rank-major; running_mean / running_var may be NULL (no running statistics); total_rows (one f64 on the
// device, may be NULL): the rows of all ranks, what bwd_dx divides by -- it never passes through the host.  f32 and bf16 activations alike.
int odvae_batchnorm_sync_stats_merge(const double* records, size_t records_bytes, int world, int C, float eps, float momentum,
                                     float* mean, float* rstd, float* running_mean, float* running_var, double* total_rows, void* stream) {
  ODVAE_CHECK_ARG(mean && rstd && world > 0 && C > 0, "batchnorm_sync_stats_merge: bad arguments");
  ODVAE_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "batchnorm_sync_stats_merge: running_mean and running_var are given together or not at all");
  const size_t need = (size_t)world * odvae_batchnorm_sync_record_bytes(C);
  if (!records || records_bytes < need) { odvae_set_error("batchnorm_sync_stats_merge: the records need %zu bytes", need); return ODVAE_ERR_WORKSPACE; }
  hipLaunchKernelGGL(bn_merge_records_kernel, dim3(ceil_div(C, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), records, world, C, eps, momentum,
                     mean, rstd, running_mean, running_var, total_rows);
  ODVAE_LAUNCH_CHECK("batchnorm_sync_stats_merge");
  return ODVAE_OK;
}

// sums: [2][C] f64 = (sum g, sum g*xhat) over this rank's rows; dbeta, dgamma: the same local sums in f32
int odvae_batchnorm_sync_bwd_sums_f32(const float* x, const float* dy, int64_t rows, int C, const float* gamma, const float* beta,
                                      const float* mean, const float* rstd, float slope, double* sums, size_t sums_bytes,
                                      float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && dy && gamma && beta && mean && rstd && dgamma && dbeta && rows > 0 && C > 0, "batchnorm_sync_bwd_sums: bad arguments");
  const size_t need_sums = odvae_batchnorm_sync_sums_bytes(C);
  if (!sums || sums_bytes < need_sums) { odvae_set_error("batchnorm_sync_bwd_sums: the sums need %zu bytes", need_sums); return ODVAE_ERR_WORKSPACE; }
  const size_t need = odvae_batchnorm_workspace_bytes(rows, C);
  if (!workspace || workspace_bytes < need) { odvae_set_error("batchnorm_sync_bwd_sums: needs %zu workspace bytes", need); return ODVAE_ERR_WORKSPACE; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  const int nblk = stat_blocks(rows);
  const int rpb = (int)ceil_div64(rows, nblk);
  const int nb = (int)ceil_div64(rows, rpb);
  hipLaunchKernelGGL((bn_colstats_kernel<1>), dim3(nb), dim3(256), 0, st, x, dy, mean, rstd, gamma, beta, slope, rows, C, rpb, part);
  hipLaunchKernelGGL(bn_sum_partials_f64_kernel, dim3(ceil_div(2 * C, 4)), dim3(256), 0, st, part, nb, C, sums, dgamma, dbeta);
  ODVAE_LAUNCH_CHECK("batchnorm_sync_bwd_sums");
  return ODVAE_OK;
}

// sums_all: [world][2][C] f64, rank-major; m_total: the rows of all ranks, on the device (stats_merge's total_rows).  dx of this rank's rows by bn_lrelu_bwd_apply_kernel.
int odvae_batchnorm_sync_bwd_dx_f32(const float* x, const float* dy, int64_t rows, int C, const float* gamma, const float* beta,
                                    const float* mean, const float* rstd, float slope, const double* sums_all, size_t sums_bytes,
                                    int world, const double* m_total, float* dx, void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && dy && gamma && beta && mean && rstd && dx && rows > 0 && C > 0 && world > 0 && m_total, "batchnorm_sync_bwd_dx: bad arguments");
  const size_t need_sums = (size_t)world * odvae_batchnorm_sync_sums_bytes(C);
  if (!sums_all || sums_bytes < need_sums) { odvae_set_error("batchnorm_sync_bwd_dx: the sums need %zu bytes", need_sums); return ODVAE_ERR_WORKSPACE; }
  const size_t need = odvae_batchnorm_workspace_bytes(rows, C);
  if (!workspace || workspace_bytes < need) { odvae_set_error("batchnorm_sync_bwd_dx: needs %zu workspace bytes", need); return ODVAE_ERR_WORKSPACE; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* sums = static_cast<float*>(workspace) + (size_t)stat_blocks(rows) * 2 * C;
  hipLaunchKernelGGL(bn_merge_sums_kernel, dim3(ceil_div(2 * C, 256)), dim3(256), 0, st, sums_all, world, C, sums);
  hipLaunchKernelGGL(bn_lrelu_bwd_apply_kernel, dim3(grid_1d(rows * C)), dim3(256), 0, st, x, dy, mean, rstd, gamma, beta, sums, slope, rows, m_total, C, 1, dx);
  ODVAE_LAUNCH_CHECK("batchnorm_sync_bwd_dx");
  return ODVAE_OK;
}

// ---- ActNorm + LeakyReLU ------------------------------------------------------------------------------------------------------------
size_t odvae_actnorm_workspace_bytes(int64_t rows, int C) {
  const size_t init = (size_t)stat_blocks(rows) * 2 * C;
  const size_t bwd = (size_t)std::max(an_bwd_blocks(rows, C, 1), C % 4 == 0 ? an_bwd_blocks(rows, C, 4) : 1) * 2 * C;
  return std::max(init, bwd) * sizeof(float);
}

// loc[c] = -mean_c, scale[c] = 1 / (std_c + eps), std_c the unbiased standard deviation over the rows; both written on the device
int odvae_actnorm_init_f32(const float* x, int64_t rows, int C, float eps, float* loc, float* scale,
                           void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && loc && scale && C > 0, "actnorm_init: bad arguments");
  ODVAE_CHECK_ARG(rows >= 2, "actnorm_init: the unbiased standard deviation needs at least 2 rows (N*H*W), got %lld", (long long)rows);
  const size_t need = odvae_actnorm_workspace_bytes(rows, C);
  if (!workspace || workspace_bytes < need) { odvae_set_error("actnorm_init: needs %zu workspace bytes", need); return ODVAE_ERR_WORKSPACE; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  const int nblk = stat_blocks(rows);
  const int rpb = (int)ceil_div64(rows, nblk);
  const int nb = (int)ceil_div64(rows, rpb);
  hipLaunchKernelGGL((bn_colstats_kernel<0>), dim3(nb), dim3(256), 0, st, x, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, rows, C, rpb, part);
  hipLaunchKernelGGL(an_init_finalize_kernel, dim3(ceil_div(C, 4)), dim3(256), 0, st, part, x, nb, C, rows, eps, loc, scale);
  ODVAE_LAUNCH_CHECK("actnorm_init");
  return ODVAE_OK;
}

int odvae_actnorm_lrelu_fwd_f32(const float* x, int64_t rows, int C, const float* loc, const float* scale, float slope, float* y, void* stream) {
  ODVAE_CHECK_ARG(x && loc && scale && y && rows > 0 && C > 0, "actnorm_lrelu_fwd: bad arguments");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (an_vec4(C, x, y, loc, scale, nullptr))
    hipLaunchKernelGGL((an_lrelu_kernel<4, 0>), dim3(grid_1d(rows * C / 4, 2048)), dim3(256), 0, st, x, nullptr, loc, scale, slope, rows * C / 4, C / 4, y);
  else
    hipLaunchKernelGGL((an_lrelu_kernel<1, 0>), dim3(grid_1d(rows * C, 2048)), dim3(256), 0, st, x, nullptr, loc, scale, slope, rows * C, C, y);
  ODVAE_LAUNCH_CHECK("actnorm_lrelu_fwd");
  return ODVAE_OK;
}

// dloc == dscale == NULL: the dx-only form (no partials, no workspace)
int odvae_actnorm_lrelu_bwd_f32(const float* x, const float* dy, int64_t rows, int C, const float* loc, const float* scale, float slope,
                                float* dx, float* dloc, float* dscale, void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && dy && loc && scale && dx && rows > 0 && C > 0, "actnorm_lrelu_bwd: bad arguments");
  ODVAE_CHECK_ARG((dloc == nullptr) == (dscale == nullptr), "actnorm_lrelu_bwd: dloc and dscale are given together or not at all");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool v4 = an_vec4(C, x, dy, dx, loc, scale);
  if (!dloc) {
    if (v4) hipLaunchKernelGGL((an_lrelu_kernel<4, 1>), dim3(grid_1d(rows * C / 4, 2048)), dim3(256), 0, st, x, dy, loc, scale, slope, rows * C / 4, C / 4, dx);
    else hipLaunchKernelGGL((an_lrelu_kernel<1, 1>), dim3(grid_1d(rows * C, 2048)), dim3(256), 0, st, x, dy, loc, scale, slope, rows * C, C, dx);
    ODVAE_LAUNCH_CHECK("actnorm_lrelu_bwd");
    return ODVAE_OK;
  }
  const size_t need = odvae_actnorm_workspace_bytes(rows, C);
  if (!workspace || workspace_bytes < need) { odvae_set_error("actnorm_lrelu_bwd: needs %zu workspace bytes", need); return ODVAE_ERR_WORKSPACE; }
  float* part = static_cast<float*>(workspace);
  const int nblk = an_bwd_blocks(rows, C, v4 ? 4 : 1);
  const int rpb = (int)ceil_div64(rows, nblk);
  const int nb = (int)ceil_div64(rows, rpb);
  if (v4) hipLaunchKernelGGL((an_lrelu_bwd_kernel<4>), dim3(nb), dim3(256), 0, st, x, dy, loc, scale, slope, rows, C, rpb, dx, part);
  else hipLaunchKernelGGL((an_lrelu_bwd_kernel<1>), dim3(nb), dim3(256), 0, st, x, dy, loc, scale, slope, rows, C, rpb, dx, part);
  hipLaunchKernelGGL(an_sum_partials_kernel, dim3(ceil_div(2 * C, 4)), dim3(256), 0, st, part, scale, nb, C, dloc, dscale);
  ODVAE_LAUNCH_CHECK("actnorm_lrelu_bwd");
  return ODVAE_OK;
}

int odvae_leaky_relu_f32(const float* x, float* y, float slope, int64_t n, void* stream) {
  ODVAE_CHECK_ARG(x && y && n > 0, "leaky_relu: bad arguments");
  hipLaunchKernelGGL(lrelu_kernel, dim3(grid_1d(n)), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, slope, n);
  ODVAE_LAUNCH_CHECK("leaky_relu");
  return ODVAE_OK;
}

int odvae_leaky_relu_bwd_f32(const float* x, const float* dy, float* dx, float slope, int64_t n, void* stream) {
  ODVAE_CHECK_ARG(x && dy && dx && n > 0, "leaky_relu_bwd: bad arguments");
  hipLaunchKernelGGL(lrelu_bwd_kernel, dim3(grid_1d(n)), dim3(256), 0, static_cast<hipStream_t>(stream), x, dy, dx, slope, n);
  ODVAE_LAUNCH_CHECK("leaky_relu_bwd");
  return ODVAE_OK;
}

size_t odvae_gan_logit_terms_workspace_bytes(int64_t n_real, int64_t n_fake) {
  return (size_t)logit_blocks(n_real, n_fake) * 6 * sizeof(double);
}

int odvae_gan_logit_terms_f32(const float* real, int64_t n_real, const float* fake, int64_t n_fake, float* out6,
                              void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(fake && out6 && n_fake > 0, "gan_logit_terms: bad arguments (fake logits and out6 are needed)");
  ODVAE_CHECK_ARG(n_real >= 0 && (real || n_real == 0), "gan_logit_terms: n_real = %lld but real is %s", (long long)n_real, real ? "given" : "null");
  const int nblk = logit_blocks(n_real, n_fake);
  const size_t need = (size_t)nblk * 6 * sizeof(double);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7) != 0) {
    odvae_set_error("gan_logit_terms: needs %zu workspace bytes, 8-byte aligned", need);
    return ODVAE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(logit_terms_partial_kernel, dim3(nblk), dim3(256), 0, st, real, n_real, fake, n_fake, part);
  hipLaunchKernelGGL(logit_terms_final_kernel, dim3(1), dim3(384), 0, st, part, nblk, n_real, n_fake, out6);
  ODVAE_LAUNCH_CHECK("gan_logit_terms");
  return ODVAE_OK;
}

int odvae_gan_logit_terms_bwd_f32(const float* real, int64_t n_real, const float* fake, int64_t n_fake, const float* dout6,
                                  float* dreal, float* dfake, void* stream) {
  ODVAE_CHECK_ARG(fake && dout6 && n_fake > 0 && (dreal || dfake), "gan_logit_terms_bwd: bad arguments");
  ODVAE_CHECK_ARG(n_real >= 0 && (real || n_real == 0) && (!dreal || n_real > 0), "gan_logit_terms_bwd: dreal needs real logits (n_real = %lld)", (long long)n_real);
  hipLaunchKernelGGL(logit_terms_bwd_kernel, dim3(grid_1d(std::max(n_real, n_fake))), dim3(256), 0, static_cast<hipStream_t>(stream),
                     real, n_real, fake, n_fake, dout6, dreal, dfake);
  ODVAE_LAUNCH_CHECK("gan_logit_terms_bwd");
  return ODVAE_OK;
}

}  // extern "C"
