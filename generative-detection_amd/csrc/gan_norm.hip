// The PatchGAN discriminator's normalisation layers, NHWC [rows][C], gfx950.  All HBM-bound.
//
// BatchNorm2d + LeakyReLU ([UPSTREAM] taming/modules/discriminator/model.py NLayerDiscriminator: Conv2d -> BatchNorm2d -> LeakyReLU(0.2)):
// batch statistics in training (biased variance for normalisation, unbiased for the running estimate, momentum 0.1), fused with the
// LeakyReLU that follows it; its synchronised form, cut where the ranks exchange; ActNorm + LeakyReLU (use_actnorm).
// BatchNorm runs on f32 or on bf16 activations (opt-in: NLayerDiscriminator.set_precision("bf16")): one set of kernels, templated on the
// element type T of x, y, dy, dx.  Everything per channel -- mean, rstd, the running statistics, gamma, beta, dgamma, dbeta -- is f32
// either way.  With bf16 the statistics are those of the values AS STORED (what the convolution in front wrote), every output element is
// computed in f32 from the stored values and rounded to bf16 once.  f32 passes take one element per thread; bf16 passes two adjacent
// channels per thread in the column pass (C even) and eight per thread in the apply passes (vec8), else one.
#include "bf16_common.h"

namespace {

// V consecutive elements of a row as f32, and back with one rounding.  col_v / run_v: the widest V of the column pass / the apply passes.
template <typename T> struct elem;
template <> struct elem<float> {
  static constexpr int col_v = 1, run_v = 1;      // BatchNorm; ActNorm takes V = 4 (one 16-byte access) where it can
  template <int V> static __device__ __forceinline__ void load(const float* p, float (&v)[V]) {
    static_assert(V == 1 || V == 4, "f32: one element or one f32x4");
    if constexpr (V == 1) v[0] = *p; else { const f32x4 t = *reinterpret_cast<const f32x4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
  }
  template <int V> static __device__ __forceinline__ void store(float* p, const float (&v)[V]) {
    static_assert(V == 1 || V == 4, "f32: one element or one f32x4");
    if constexpr (V == 1) *p = v[0]; else { f32x4 t; t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3]; *reinterpret_cast<f32x4*>(p) = t; }
  }
};
template <> struct elem<bf16_t> {
  static constexpr int col_v = 2, run_v = 8;
  template <int V> static __device__ __forceinline__ void load(const bf16_t* p, float (&v)[V]) { load_run<V>(p, v); }
  template <int V> static __device__ __forceinline__ void store(bf16_t* p, const float (&v)[V]) { store_run_rne<V>(p, v); }
};

// the first element of channel c, the pivot of the statistics
template <typename T> __device__ __forceinline__ float pivot_of(const T* x, int c) {
  float v[1];
  elem<T>::template load<1>(x + c, v);
  return v[0];
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
// A thread keeps V adjacent channels and walks every `lanes`-th row of the block's row range; lanes = 256 / (channel groups of this
// pass) fixes which rows a thread sums and in what order, so V is part of the result's bits.
template <typename T, int MODE, int V>
__global__ __launch_bounds__(256) void bn_colstats_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float slope, int64_t rows, int C, int rows_per_block,
                                                          float* __restrict__ part) {
  __shared__ float sh[2 * V][256];
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = std::min<int64_t>(rows, r0 + rows_per_block);
  const int CV = C / V;
  for (int cbase = 0; cbase < CV; cbase += 256) {
    const int cw = min(256, CV - cbase);
    const int lanes = 256 / cw;
    const int cg = cbase + threadIdx.x % cw, rl = threadIdx.x / cw;
    float a[V], b[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { a[j] = 0.f; b[j] = 0.f; }
    if (rl < lanes) {
      float mu[V], rs[V], ga[V], be[V], pivot[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int c = cg * V + j;
        mu[j] = rs[j] = ga[j] = be[j] = pivot[j] = 0.f;
        if (MODE == 1) { mu[j] = mean[c]; rs[j] = rstd[c]; ga[j] = gamma[c]; be[j] = beta[c]; }
        else pivot[j] = pivot_of(x, c);
      }
      for (int64_t r = r0 + rl; r < r1; r += lanes) {
        float v[V], d[V];
        elem<T>::template load<V>(x + r * C + cg * V, v);
        if (MODE == 1) elem<T>::template load<V>(dy + r * C + cg * V, d);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          if (MODE == 0) { const float dd = v[j] - pivot[j]; a[j] += dd; b[j] += dd * dd; }
          else {
            const float xh = (v[j] - mu[j]) * rs[j];
            const float u = xh * ga[j] + be[j];
            const float g = d[j] * (u > 0.f ? 1.f : slope);
            a[j] += g; b[j] += g * xh;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) { sh[j][threadIdx.x] = a[j]; sh[V + j][threadIdx.x] = b[j]; }
    __syncthreads();
    if (threadIdx.x < cw) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float ta = 0.f, tb = 0.f;
        for (int k = 0; k < lanes; ++k) { ta += sh[j][k * cw + threadIdx.x]; tb += sh[V + j][k * cw + threadIdx.x]; }
        part[((int64_t)blockIdx.x * 2 + 0) * C + (cbase + threadIdx.x) * V + j] = ta;
        part[((int64_t)blockIdx.x * 2 + 1) * C + (cbase + threadIdx.x) * V + j] = tb;
      }
    }
    __syncthreads();
  }
}

// t[j] = the total of part[.][which + j][c] over the nblk blocks of a column pass, in every lane of the calling wavefront: the partials
// are summed lane-strided in f64, then by a fixed butterfly (deterministic).  One thread per channel walking all nblk partials was a
// chain of ~1 000 dependent loads: 125 us per launch for 4 KB of output.
template <int N>
__device__ __forceinline__ void part_totals(const float* __restrict__ part, int nblk, int C, int which, int c, double (&t)[N]) {
  static_assert(N == 1 || N == 2, "one total, or the pair (which, which + 1)");
  double a = 0.0, b = 0.0;
  for (int k = (int)(threadIdx.x & 63); k < nblk; k += 64) {
    a += (double)part[((int64_t)k * 2 + which) * C + c];
    if constexpr (N == 2) b += (double)part[((int64_t)k * 2 + which + 1) * C + c];
  }
  t[0] = wave_sum_f64(a);
  if constexpr (N == 2) t[1] = wave_sum_f64(b);
}

// training-mode forward statistics: mean, rstd and the running estimates (momentum update, unbiased variance) from the sums about
// the pivot x[0][c]: mean = pivot + E[d], var = E[d^2] - E[d]^2.  One wavefront per channel.
template <typename T>
__global__ void bn_finalize_kernel(const float* __restrict__ part, const T* __restrict__ x, int nblk, int C, int64_t rows, float eps, float momentum,
                                   float* __restrict__ mean, float* __restrict__ rstd,
                                   float* __restrict__ running_mean, float* __restrict__ running_var) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (c >= C) return;
  double t[2];
  part_totals(part, nblk, C, 0, c, t);
  if (lane != 0) return;
  const double m = (double)rows;
  const double dm = t[0] / m;
  const double mu = (double)pivot_of(x, c) + dm;
  double var = t[1] / m - dm * dm;
  if (var < 0.0) var = 0.0;
  mean[c] = (float)mu;
  rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) {
    const double unbiased = rows > 1 ? var * m / (m - 1.0) : var;
    running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mu);
    running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unbiased);
  }
}

// sums[2][C] = column totals of the partials (backward: sum g, sum g*xhat); one wavefront per (which, channel)
__global__ void bn_sum_partials_kernel(const float* __restrict__ part, int nblk, int C, float* __restrict__ sums) {
  const int lane = threadIdx.x & 63;
  const int idx = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (idx >= 2 * C) return;
  double t[1];
  part_totals(part, nblk, C, idx / C, idx % C, t);
  if (lane == 0) sums[idx] = (float)t[0];
}

// ---- synchronised BatchNorm: the statistics and the backward sums of one rank as f64 records, merged over ranks in index order -------
// record[c] = {rows, mean_c, M2_c}, M2 = sum (x - mean_c)^2, from the partials of bn_colstats_kernel<T, 0, V> about the pivot x[0][c]:
// mean = pivot + a / m, M2 = b - a^2 / m.  One wavefront per channel, f64, the order of bn_finalize_kernel.
template <typename T>
__global__ void bn_record_kernel(const float* __restrict__ part, const T* __restrict__ x, int nblk, int C, int64_t rows,
                                 double* __restrict__ record) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (c >= C) return;
  double t[2];
  part_totals(part, nblk, C, 0, c, t);
  if (lane != 0) return;
  const double m = (double)rows;
  const double dm = t[0] / m;
  double m2 = t[1] - t[0] * dm;
  if (m2 < 0.0) m2 = 0.0;
  record[(int64_t)c * 3 + 0] = m;
  record[(int64_t)c * 3 + 1] = (double)pivot_of(x, c) + dm;
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
  double t[1];
  part_totals(part, nblk, C, which, c, t);
  if (lane != 0) return;
  sums64[idx] = t[0];
  if (which == 0) dbeta[c] = (float)t[0]; else dgamma[c] = (float)t[0];
}

// sums[2][C] (f32, what bn_lrelu_bwd_apply_kernel reads) = the ranks' sums64[world][2][C] added in index order in f64
__global__ void bn_merge_sums_kernel(const double* __restrict__ sums64, int world, int C, float* __restrict__ sums) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * C) return;
  double a = sums64[idx];
  for (int w = 1; w < world; ++w) a += sums64[(int64_t)w * 2 * C + idx];
  sums[idx] = (float)a;
}

// y = lrelu((x-mean)*rstd*gamma+beta); a thread takes V consecutive elements of one row (V = 8: C % 8 == 0, so they never wrap a row)
template <typename T, int V>
__global__ __launch_bounds__(256) void bn_lrelu_apply_kernel(const T* __restrict__ x, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float slope, int64_t total, int C,
                                                             T* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i * V < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t idx = i * V;
    const int c0 = (int)(idx % C);
    float xv[V], yv[V];
    elem<T>::template load<V>(x + idx, xv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int c = c0 + j;
      const float u = (xv[j] - mean[c]) * rstd[c] * gamma[c] + beta[c];
      yv[j] = u > 0.f ? u : slope * u;
    }
    elem<T>::template store<V>(y + idx, yv);
  }
}

// training: dx = gamma*rstd/M * (M*g - sum_g - xhat*sum_gxhat); eval (train=0): dx = gamma*rstd*g.  M = m: the rows the sums were
// taken over -- `rows`, or *m_total (device), all ranks' rows, when the sums are the merged ones (synchronised BatchNorm)
template <typename T, int V>
__global__ __launch_bounds__(256) void bn_lrelu_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                                 const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 const float* __restrict__ sums, float slope, int64_t rows, const double* __restrict__ m_total,
                                                                 int C, int train, T* __restrict__ dx) {
  const int64_t total = rows * C;
  const float inv_m = 1.f / (m_total ? (float)*m_total : (float)rows);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i * V < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t idx = i * V;
    const int c0 = (int)(idx % C);
    float xv[V], gv[V], ov[V];
    elem<T>::template load<V>(x + idx, xv);
    elem<T>::template load<V>(dy + idx, gv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int c = c0 + j;
      const float xh = (xv[j] - mean[c]) * rstd[c];
      const float u = xh * gamma[c] + beta[c];
      const float g = gv[j] * (u > 0.f ? 1.f : slope);
      float v = g;
      if (train) v = g - (sums[c] + xh * sums[C + c]) * inv_m;
      ov[j] = gamma[c] * rstd[c] * v;
    }
    elem<T>::template store<V>(dx + idx, ov);
  }
}

// ---- ActNorm + LeakyReLU ([UPSTREAM] taming/modules/util.py ActNorm, NLayerDiscriminator(use_actnorm=True)) -----------------------
// h = scale[c] * (x + loc[c]), y = lrelu(h).  loc and scale are parameters: nothing is reduced in the forward, and in the backward dx
// does not depend on the parameter sums, so the activations are read once (BatchNorm in training mode: 3 tensor passes forward, 5
// backward; here 2 and 3).  V = 4: 16-byte accesses (C % 4 == 0 and 16-byte aligned pointers, every real layer); V = 1: scalar.
// BWD = 0: y = lrelu(scale * (x + loc)).  BWD = 1 (neither parameter needs a gradient): dx = scale * dy * lrelu'(scale * (x + loc)).
// Both evaluate h by the same two f32 operations, so the backward sees the sign the forward saw.
template <int V, int BWD>
__global__ __launch_bounds__(256) void an_lrelu_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                       const float* __restrict__ loc, const float* __restrict__ scale, float slope,
                                                       int64_t total_v, int CV, float* __restrict__ out) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total_v; idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % CV) * V;
    float xv[V], lo[V], sc[V], dv[V], o[V];
    elem<float>::load<V>(x + idx * V, xv); elem<float>::load<V>(loc + c, lo); elem<float>::load<V>(scale + c, sc);
    if (BWD) elem<float>::load<V>(dy + idx * V, dv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float h = sc[j] * (xv[j] + lo[j]);
      o[j] = BWD ? sc[j] * (dv[j] * (h > 0.f ? 1.f : slope)) : (h > 0.f ? h : slope * h);
    }
    elem<float>::store<V>(out + idx * V, o);
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
      elem<float>::load<V>(loc + c, lo); elem<float>::load<V>(scale + c, sc);
      for (int64_t r = r0 + rl; r < r1; r += lanes) {
        float xv[V], dv[V], o[V];
        elem<float>::load<V>(x + r * C + c, xv); elem<float>::load<V>(dy + r * C + c, dv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float t = xv[j] + lo[j];
          const float h = sc[j] * t;
          const float g = dv[j] * (h > 0.f ? 1.f : slope);
          a[j] += g; b[j] += g * t;
          o[j] = sc[j] * g;
        }
        elem<float>::store<V>(dx + r * C + c, o);
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

// dloc = scale * sum g, dscale = sum g (x + loc): one wavefront per (which, channel), as bn_sum_partials_kernel
__global__ void an_sum_partials_kernel(const float* __restrict__ part, const float* __restrict__ scale, int nblk, int C,
                                       float* __restrict__ dloc, float* __restrict__ dscale) {
  const int lane = threadIdx.x & 63;
  const int idx = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (idx >= 2 * C) return;
  const int which = idx / C, c = idx % C;
  double t[1];
  part_totals(part, nblk, C, which, c, t);
  if (lane != 0) return;
  if (which == 0) dloc[c] = (float)((double)scale[c] * t[0]); else dscale[c] = (float)t[0];
}

// data-dependent initialisation from the partials of bn_colstats_kernel<float, 0, 1> (sums of d and d^2 about the pivot x[0][c]):
// loc = -mean, scale = 1 / (std + eps) with the unbiased (rows - 1) std, written into the parameters' own storage.
// One wavefront per channel, as bn_finalize_kernel.
__global__ void an_init_finalize_kernel(const float* __restrict__ part, const float* __restrict__ x, int nblk, int C, int64_t rows, float eps,
                                        float* __restrict__ loc, float* __restrict__ scale) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (c >= C) return;
  double t[2];
  part_totals(part, nblk, C, 0, c, t);
  if (lane != 0) return;
  const double m = (double)rows;
  const double dm = t[0] / m;
  double var = (t[1] - t[0] * dm) / (m - 1.0);
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

// ---- host side: one function per f32 / bf16 pair of entry points; `name` is what the pair's messages begin with ----------------------
bool workspace_short(const char* name, const void* workspace, size_t workspace_bytes, size_t need) {
  if (workspace && workspace_bytes >= need) return false;
  odvae_set_error("%s: needs %zu workspace bytes", name, need);
  return true;
}

// The column pass over `rows` in a workspace of odvae_batchnorm_workspace_bytes: nb blocks of rpb rows leave part[nb][2][C]; sums[2][C]
// lies behind the partials of stat_blocks blocks, the count the workspace is sized by, whatever nb <= that comes to.
struct StatPass { float* part; float* sums; int nb, rpb; };
StatPass stat_pass(int64_t rows, int C, void* workspace) {
  const int nblk = stat_blocks(rows);
  const int rpb = (int)ceil_div64(rows, nblk);
  float* part = static_cast<float*>(workspace);
  return {part, part + (size_t)nblk * 2 * C, (int)ceil_div64(rows, rpb), rpb};
}

template <typename T, int MODE>
void launch_colstats(hipStream_t st, const StatPass& p, const T* x, const T* dy, const float* mean, const float* rstd, const float* gamma,
                     const float* beta, float slope, int64_t rows, int C) {
  constexpr int W = elem<T>::col_v;
  if (W > 1 && C % W == 0) hipLaunchKernelGGL((bn_colstats_kernel<T, MODE, W>), dim3(p.nb), dim3(256), 0, st, x, dy, mean, rstd, gamma, beta, slope, rows, C, p.rpb, p.part);
  else                     hipLaunchKernelGGL((bn_colstats_kernel<T, MODE, 1>), dim3(p.nb), dim3(256), 0, st, x, dy, mean, rstd, gamma, beta, slope, rows, C, p.rpb, p.part);
}

template <typename T>
void launch_bwd_apply(hipStream_t st, const T* x, const T* dy, const float* mean, const float* rstd, const float* gamma, const float* beta,
                      const float* sums, float slope, int64_t rows, const double* m_total, int C, int train, T* dx) {
  constexpr int W = elem<T>::run_v;
  const int64_t total = rows * C;
  if (W > 1 && vec8(total, C, x, dy, dx))
    hipLaunchKernelGGL((bn_lrelu_bwd_apply_kernel<T, W>), dim3(grid_1d(total / W)), dim3(256), 0, st, x, dy, mean, rstd, gamma, beta, sums, slope, rows, m_total, C, train, dx);
  else
    hipLaunchKernelGGL((bn_lrelu_bwd_apply_kernel<T, 1>), dim3(grid_1d(total)), dim3(256), 0, st, x, dy, mean, rstd, gamma, beta, sums, slope, rows, m_total, C, train, dx);
}

// a bf16 column pass reads a channel pair as one dword: its operands are 4-byte aligned or refused (the f32 entry points make no such check)
template <typename T> bool pair_aligned(const T* a, const T* b = nullptr, const T* c = nullptr) {
  return elem<T>::col_v == 1 || (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 3) == 0;
}

template <typename T>
int bn_fwd(const char* name, const T* x, int64_t rows, int C, const float* gamma, const float* beta, float eps, float momentum, float slope, int train,
           float* mean, float* rstd, float* running_mean, float* running_var, T* y, void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && gamma && beta && mean && rstd && y && rows > 0 && C > 0, "%s: bad arguments", name);
  ODVAE_CHECK_ARG(pair_aligned(x, y), "%s: misaligned operand", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (train) {
    if (workspace_short(name, workspace, workspace_bytes, odvae_batchnorm_workspace_bytes(rows, C))) return ODVAE_ERR_WORKSPACE;
    const StatPass p = stat_pass(rows, C, workspace);
    launch_colstats<T, 0>(st, p, x, nullptr, nullptr, nullptr, nullptr, nullptr, slope, rows, C);
    hipLaunchKernelGGL(bn_finalize_kernel<T>, dim3(ceil_div(C, 4)), dim3(256), 0, st, p.part, x, p.nb, C, rows, eps, momentum, mean, rstd, running_mean, running_var);
  }
  constexpr int W = elem<T>::run_v;
  const int64_t total = rows * C;
  if (W > 1 && vec8(total, C, x, y, nullptr))
    hipLaunchKernelGGL((bn_lrelu_apply_kernel<T, W>), dim3(grid_1d(total / W)), dim3(256), 0, st, x, mean, rstd, gamma, beta, slope, total, C, y);
  else
    hipLaunchKernelGGL((bn_lrelu_apply_kernel<T, 1>), dim3(grid_1d(total)), dim3(256), 0, st, x, mean, rstd, gamma, beta, slope, total, C, y);
  ODVAE_LAUNCH_CHECK(name);
  return ODVAE_OK;
}

template <typename T>
int bn_bwd(const char* name, const T* x, const T* dy, int64_t rows, int C, const float* gamma, const float* beta, const float* mean, const float* rstd,
           float slope, int train, T* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && dy && gamma && beta && mean && rstd && dx && dgamma && dbeta && rows > 0 && C > 0, "%s: bad arguments", name);
  ODVAE_CHECK_ARG(pair_aligned(x, dy, dx), "%s: misaligned operand", name);
  if (workspace_short(name, workspace, workspace_bytes, odvae_batchnorm_workspace_bytes(rows, C))) return ODVAE_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const StatPass p = stat_pass(rows, C, workspace);
  launch_colstats<T, 1>(st, p, x, dy, mean, rstd, gamma, beta, slope, rows, C);
  hipLaunchKernelGGL(bn_sum_partials_kernel, dim3(ceil_div(2 * C, 4)), dim3(256), 0, st, p.part, p.nb, C, p.sums);
  // dbeta = sum g ; dgamma = sum g*xhat
  hipMemcpyAsync(dbeta, p.sums, (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, st);
  hipMemcpyAsync(dgamma, p.sums + C, (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, st);
  launch_bwd_apply<T>(st, x, dy, mean, rstd, gamma, beta, p.sums, slope, rows, nullptr, C, train, dx);
  ODVAE_LAUNCH_CHECK(name);
  return ODVAE_OK;
}

template <typename T>
int bn_sync_record(const char* name, const T* x, int64_t rows, int C, double* record, size_t record_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && rows > 0 && C > 0, "%s: bad arguments", name);
  ODVAE_CHECK_ARG(pair_aligned(x), "%s: misaligned operand", name);
  const size_t need_rec = odvae_batchnorm_sync_record_bytes(C);
  if (!record || record_bytes < need_rec) { odvae_set_error("%s: the record needs %zu bytes", name, need_rec); return ODVAE_ERR_WORKSPACE; }
  if (workspace_short(name, workspace, workspace_bytes, odvae_batchnorm_workspace_bytes(rows, C))) return ODVAE_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const StatPass p = stat_pass(rows, C, workspace);
  launch_colstats<T, 0>(st, p, x, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, rows, C);
  hipLaunchKernelGGL(bn_record_kernel<T>, dim3(ceil_div(C, 4)), dim3(256), 0, st, p.part, x, p.nb, C, rows, record);
  ODVAE_LAUNCH_CHECK(name);
  return ODVAE_OK;
}

template <typename T>
int bn_sync_bwd_sums(const char* name, const T* x, const T* dy, int64_t rows, int C, const float* gamma, const float* beta, const float* mean, const float* rstd,
                     float slope, double* sums, size_t sums_bytes, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && dy && gamma && beta && mean && rstd && dgamma && dbeta && rows > 0 && C > 0, "%s: bad arguments", name);
  ODVAE_CHECK_ARG(pair_aligned(x, dy), "%s: misaligned operand", name);
  const size_t need_sums = odvae_batchnorm_sync_sums_bytes(C);
  if (!sums || sums_bytes < need_sums) { odvae_set_error("%s: the sums need %zu bytes", name, need_sums); return ODVAE_ERR_WORKSPACE; }
  if (workspace_short(name, workspace, workspace_bytes, odvae_batchnorm_workspace_bytes(rows, C))) return ODVAE_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const StatPass p = stat_pass(rows, C, workspace);
  launch_colstats<T, 1>(st, p, x, dy, mean, rstd, gamma, beta, slope, rows, C);
  hipLaunchKernelGGL(bn_sum_partials_f64_kernel, dim3(ceil_div(2 * C, 4)), dim3(256), 0, st, p.part, p.nb, C, sums, dgamma, dbeta);
  ODVAE_LAUNCH_CHECK(name);
  return ODVAE_OK;
}

template <typename T>
int bn_sync_bwd_dx(const char* name, const T* x, const T* dy, int64_t rows, int C, const float* gamma, const float* beta, const float* mean, const float* rstd,
                   float slope, const double* sums_all, size_t sums_bytes, int world, const double* m_total, T* dx, void* workspace, size_t workspace_bytes,
                   void* stream) {
  ODVAE_CHECK_ARG(x && dy && gamma && beta && mean && rstd && dx && rows > 0 && C > 0 && world > 0 && m_total, "%s: bad arguments", name);
  ODVAE_CHECK_ARG(pair_aligned(x, dy, dx), "%s: misaligned operand", name);
  const size_t need_sums = (size_t)world * odvae_batchnorm_sync_sums_bytes(C);
  if (!sums_all || sums_bytes < need_sums) { odvae_set_error("%s: the sums need %zu bytes", name, need_sums); return ODVAE_ERR_WORKSPACE; }
  if (workspace_short(name, workspace, workspace_bytes, odvae_batchnorm_workspace_bytes(rows, C))) return ODVAE_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* sums = stat_pass(rows, C, workspace).sums;
  hipLaunchKernelGGL(bn_merge_sums_kernel, dim3(ceil_div(2 * C, 256)), dim3(256), 0, st, sums_all, world, C, sums);
  launch_bwd_apply<T>(st, x, dy, mean, rstd, gamma, beta, sums, slope, rows, m_total, C, 1, dx);
  ODVAE_LAUNCH_CHECK(name);
  return ODVAE_OK;
}

// the bf16 entry points take their activations as void*
const bf16_t* bf(const void* p) { return static_cast<const bf16_t*>(p); }

}  // namespace

extern "C" {

size_t odvae_batchnorm_workspace_bytes(int64_t rows, int C) { return ((size_t)stat_blocks(rows) * 2 * C + 2 * C) * sizeof(float); }

// x,y: [rows][C] (NHWC flattened).  train=1: batch statistics into mean/rstd (+ running stats update when given);
// train=0: mean/rstd must already hold the running estimates (rstd = 1/sqrt(running_var+eps)).  Workspace (train = 1 only):
// odvae_batchnorm_workspace_bytes(rows, C).  _bf16: x, y (and dy, dx below) bf16, everything per channel f32.
int odvae_batchnorm_lrelu_fwd_f32(const float* x, int64_t rows, int C, const float* gamma, const float* beta, float eps, float momentum, float slope, int train,
                                  float* mean, float* rstd, float* running_mean, float* running_var, float* y, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  return bn_fwd<float>("batchnorm_lrelu_fwd", x, rows, C, gamma, beta, eps, momentum, slope, train, mean, rstd, running_mean, running_var, y, workspace, workspace_bytes, stream);
}
int odvae_batchnorm_lrelu_fwd_bf16(const void* x, int64_t rows, int C, const float* gamma, const float* beta, float eps, float momentum, float slope, int train,
                                   float* mean, float* rstd, float* running_mean, float* running_var, void* y, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  return bn_fwd<bf16_t>("batchnorm_lrelu_fwd_bf16", bf(x), rows, C, gamma, beta, eps, momentum, slope, train, mean, rstd, running_mean, running_var,
                        static_cast<bf16_t*>(y), workspace, workspace_bytes, stream);
}

int odvae_batchnorm_lrelu_bwd_f32(const float* x, const float* dy, int64_t rows, int C, const float* gamma, const float* beta, const float* mean, const float* rstd,
                                  float slope, int train, float* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream) {
  return bn_bwd<float>("batchnorm_lrelu_bwd", x, dy, rows, C, gamma, beta, mean, rstd, slope, train, dx, dgamma, dbeta, workspace, workspace_bytes, stream);
}
int odvae_batchnorm_lrelu_bwd_bf16(const void* x, const void* dy, int64_t rows, int C, const float* gamma, const float* beta, const float* mean, const float* rstd,
                                   float slope, int train, void* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream) {
  return bn_bwd<bf16_t>("batchnorm_lrelu_bwd_bf16", bf(x), bf(dy), rows, C, gamma, beta, mean, rstd, slope, train, static_cast<bf16_t*>(dx), dgamma, dbeta,
                        workspace, workspace_bytes, stream);
}

// ---- synchronised BatchNorm + LeakyReLU: the forward and the backward cut where the ranks exchange ---------------------------------
// forward: stats_record (each rank) -> exchange -> stats_merge -> odvae_batchnorm_lrelu_fwd_*(train = 0) with the merged mean / rstd;
// backward: bwd_sums (each rank) -> exchange -> bwd_dx.  Workspace of the three that take one: odvae_batchnorm_workspace_bytes(rows, C).
size_t odvae_batchnorm_sync_record_bytes(int C) { return (size_t)C * 3 * sizeof(double); }
size_t odvae_batchnorm_sync_sums_bytes(int C) { return (size_t)C * 2 * sizeof(double); }

int odvae_batchnorm_sync_stats_record_f32(const float* x, int64_t rows, int C, double* record, size_t record_bytes, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  return bn_sync_record<float>("batchnorm_sync_stats_record", x, rows, C, record, record_bytes, workspace, workspace_bytes, stream);
}
int odvae_batchnorm_sync_stats_record_bf16(const void* x, int64_t rows, int C, double* record, size_t record_bytes, void* workspace, size_t workspace_bytes,
                                           void* stream) {
  return bn_sync_record<bf16_t>("batchnorm_sync_stats_record_bf16", bf(x), rows, C, record, record_bytes, workspace, workspace_bytes, stream);
}

// records: [world][C][3] f64, rank-major; running_mean / running_var may be NULL (no running statistics); total_rows (one f64 on the
// device, may be NULL): the rows of all ranks, what bwd_dx divides by -- it never passes through the host.  f32 and bf16 activations alike.
int odvae_batchnorm_sync_stats_merge(const double* records, size_t records_bytes, int world, int C, float eps, float momentum, float* mean, float* rstd,
                                     float* running_mean, float* running_var, double* total_rows, void* stream) {
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
int odvae_batchnorm_sync_bwd_sums_f32(const float* x, const float* dy, int64_t rows, int C, const float* gamma, const float* beta, const float* mean,
                                      const float* rstd, float slope, double* sums, size_t sums_bytes, float* dgamma, float* dbeta, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  return bn_sync_bwd_sums<float>("batchnorm_sync_bwd_sums", x, dy, rows, C, gamma, beta, mean, rstd, slope, sums, sums_bytes, dgamma, dbeta, workspace, workspace_bytes, stream);
}
int odvae_batchnorm_sync_bwd_sums_bf16(const void* x, const void* dy, int64_t rows, int C, const float* gamma, const float* beta, const float* mean,
                                       const float* rstd, float slope, double* sums, size_t sums_bytes, float* dgamma, float* dbeta, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  return bn_sync_bwd_sums<bf16_t>("batchnorm_sync_bwd_sums_bf16", bf(x), bf(dy), rows, C, gamma, beta, mean, rstd, slope, sums, sums_bytes, dgamma, dbeta,
                                  workspace, workspace_bytes, stream);
}

// sums_all: [world][2][C] f64, rank-major; m_total: the rows of all ranks, on the device (stats_merge's total_rows).  dx of this rank's rows by bn_lrelu_bwd_apply_kernel.
int odvae_batchnorm_sync_bwd_dx_f32(const float* x, const float* dy, int64_t rows, int C, const float* gamma, const float* beta, const float* mean,
                                    const float* rstd, float slope, const double* sums_all, size_t sums_bytes, int world, const double* m_total, float* dx,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  return bn_sync_bwd_dx<float>("batchnorm_sync_bwd_dx", x, dy, rows, C, gamma, beta, mean, rstd, slope, sums_all, sums_bytes, world, m_total, dx, workspace, workspace_bytes, stream);
}
int odvae_batchnorm_sync_bwd_dx_bf16(const void* x, const void* dy, int64_t rows, int C, const float* gamma, const float* beta, const float* mean, const float* rstd,
                                     float slope, const double* sums_all, size_t sums_bytes, int world, const double* m_total, void* dx, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  return bn_sync_bwd_dx<bf16_t>("batchnorm_sync_bwd_dx_bf16", bf(x), bf(dy), rows, C, gamma, beta, mean, rstd, slope, sums_all, sums_bytes, world, m_total,
                                static_cast<bf16_t*>(dx), workspace, workspace_bytes, stream);
}

// ---- ActNorm + LeakyReLU ------------------------------------------------------------------------------------------------------------
size_t odvae_actnorm_workspace_bytes(int64_t rows, int C) {
  const size_t init = (size_t)stat_blocks(rows) * 2 * C;
  const size_t bwd = (size_t)std::max(an_bwd_blocks(rows, C, 1), C % 4 == 0 ? an_bwd_blocks(rows, C, 4) : 1) * 2 * C;
  return std::max(init, bwd) * sizeof(float);
}

// loc[c] = -mean_c, scale[c] = 1 / (std_c + eps), std_c the unbiased standard deviation over the rows; both written on the device
int odvae_actnorm_init_f32(const float* x, int64_t rows, int C, float eps, float* loc, float* scale, void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && loc && scale && C > 0, "actnorm_init: bad arguments");
  ODVAE_CHECK_ARG(rows >= 2, "actnorm_init: the unbiased standard deviation needs at least 2 rows (N*H*W), got %lld", (long long)rows);
  if (workspace_short("actnorm_init", workspace, workspace_bytes, odvae_actnorm_workspace_bytes(rows, C))) return ODVAE_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const StatPass p = stat_pass(rows, C, workspace);
  launch_colstats<float, 0>(st, p, x, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, rows, C);
  hipLaunchKernelGGL(an_init_finalize_kernel, dim3(ceil_div(C, 4)), dim3(256), 0, st, p.part, x, p.nb, C, rows, eps, loc, scale);
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
int odvae_actnorm_lrelu_bwd_f32(const float* x, const float* dy, int64_t rows, int C, const float* loc, const float* scale, float slope, float* dx, float* dloc,
                                float* dscale, void* workspace, size_t workspace_bytes, void* stream) {
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
  if (workspace_short("actnorm_lrelu_bwd", workspace, workspace_bytes, odvae_actnorm_workspace_bytes(rows, C))) return ODVAE_ERR_WORKSPACE;
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

}  // extern "C"
