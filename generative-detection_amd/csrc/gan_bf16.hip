// PatchGAN discriminator support kernels on bf16 activations, gfx950 (opt-in: NLayerDiscriminator.set_precision("bf16")).  HBM-bound.
//
// BatchNorm2d + LeakyReLU: the twins of bn_colstats_kernel / bn_finalize_kernel / bn_lrelu_apply_kernel / bn_lrelu_bwd_apply_kernel of
// gan_f32.hip with x, y, dy, dx in bf16 ([rows][C], NHWC flattened) and everything per channel -- mean, rstd, the running statistics,
// gamma, beta, dgamma, dbeta -- in f32.  The statistics are those of the bf16 values AS STORED (what the convolution in front wrote),
// summed in f32 about the pivot x[0][c] exactly as the f32 kernels do (gan_f32.hip: why a pivot), the partials added in f64 in a fixed
// order.  Every output element is computed in f32 from the stored values and rounded to bf16 once.
// The 4x4 convolutions themselves are modes 5 / 6 / 7 of conv_bf16.hip and modes 5 / 6 of conv_wgrad_bf16.hip.
#include "bf16_common.h"

namespace {

// part[blk][2][C] as bn_colstats_kernel: MODE 0 sums of (d, d^2), d = x - x[0][c]; MODE 1 sums of (g, g * xhat).
// V = 2 (C even): a thread keeps two adjacent channels and reads them as one dword.
template <int MODE, int V>
__global__ __launch_bounds__(256) void bn_colstats_bf16_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
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
        else pivot[j] = bf16_to_f32(x[c]);
      }
      for (int64_t r = r0 + rl; r < r1; r += lanes) {
        float v[V], d[V];
        if (V == 2) {
          const unsigned w = *reinterpret_cast<const unsigned*>(x + r * C + 2 * cg);
          v[0] = bf16_lo(w); v[V - 1] = bf16_hi(w);
          if (MODE == 1) { const unsigned g = *reinterpret_cast<const unsigned*>(dy + r * C + 2 * cg); d[0] = bf16_lo(g); d[V - 1] = bf16_hi(g); }
        } else {
          v[0] = bf16_to_f32(x[r * C + cg]);
          if (MODE == 1) d[0] = bf16_to_f32(dy[r * C + cg]);
        }
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

// bn_finalize_kernel with a bf16 pivot: mean = pivot + E[d], var = E[d^2] - E[d]^2; one wavefront per channel, f64, fixed order
__global__ void bn_finalize_bf16_kernel(const float* __restrict__ part, const bf16_t* __restrict__ x, int nblk, int C, int64_t rows, float eps,
                                        float momentum, float* __restrict__ mean, float* __restrict__ rstd,
                                        float* __restrict__ running_mean, float* __restrict__ running_var) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (c >= C) return;
  double a = 0.0, b = 0.0;
  for (int k = lane; k < nblk; k += 64) { a += (double)part[((int64_t)k * 2 + 0) * C + c]; b += (double)part[((int64_t)k * 2 + 1) * C + c]; }
  a = wave_sum_f64(a); b = wave_sum_f64(b);
  if (lane != 0) return;
  const double m = (double)rows;
  const double dm = a / m;
  const double mu = (double)bf16_to_f32(x[c]) + dm;
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

__global__ void bn_sum_partials_b_kernel(const float* __restrict__ part, int nblk, int C, float* __restrict__ sums) {
  const int lane = threadIdx.x & 63;
  const int idx = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (idx >= 2 * C) return;
  const int which = idx / C, c = idx % C;
  double a = 0.0;
  for (int k = lane; k < nblk; k += 64) a += (double)part[((int64_t)k * 2 + which) * C + c];
  a = wave_sum_f64(a);
  if (lane == 0) sums[idx] = (float)a;
}

// bn_record_kernel / bn_sum_partials_f64_kernel / bn_merge_sums_kernel of gan_f32.hip (synchronised BatchNorm) with a bf16 pivot
__global__ void bn_record_bf16_kernel(const float* __restrict__ part, const bf16_t* __restrict__ x, int nblk, int C, int64_t rows,
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
  record[(int64_t)c * 3 + 1] = (double)bf16_to_f32(x[c]) + dm;
  record[(int64_t)c * 3 + 2] = m2;
}

__global__ void bn_sum_partials_f64_b_kernel(const float* __restrict__ part, int nblk, int C, double* __restrict__ sums64,
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

__global__ void bn_merge_sums_b_kernel(const double* __restrict__ sums64, int world, int C, float* __restrict__ sums) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * C) return;
  double a = sums64[idx];
  for (int w = 1; w < world; ++w) a += sums64[(int64_t)w * 2 * C + idx];
  sums[idx] = (float)a;
}

// V consecutive elements of one row per thread: V = 8 (one 16-byte vector; C % 8 == 0, so the eight never wrap a row) or 1
template <int V> __device__ __forceinline__ void ld_bf16(const bf16_t* p, float (&v)[V]) {
  if (V == 8) {
    const u32x4 q = *reinterpret_cast<const u32x4*>(p);
    v[0] = bf16_lo(q.x); v[1 % V] = bf16_hi(q.x); v[2 % V] = bf16_lo(q.y); v[3 % V] = bf16_hi(q.y);
    v[4 % V] = bf16_lo(q.z); v[5 % V] = bf16_hi(q.z); v[6 % V] = bf16_lo(q.w); v[7 % V] = bf16_hi(q.w);
  } else v[0] = bf16_to_f32(*p);
}
template <int V> __device__ __forceinline__ void st_bf16(bf16_t* p, const float (&v)[V]) {
  if (V == 8) {
    u32x4 q;
    q.x = cvt_pk_bf16(v[0], v[1 % V]); q.y = cvt_pk_bf16(v[2 % V], v[3 % V]); q.z = cvt_pk_bf16(v[4 % V], v[5 % V]); q.w = cvt_pk_bf16(v[6 % V], v[7 % V]);
    *reinterpret_cast<u32x4*>(p) = q;
  } else *p = f32_to_bf16(v[0]);
}

// y = lrelu((x - mean) * rstd * gamma + beta), the f32 kernel's expression on the stored bf16 x, rounded once
template <int V>
__global__ __launch_bounds__(256) void bn_lrelu_apply_bf16_kernel(const bf16_t* __restrict__ x, const float* __restrict__ mean,
                                                                  const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float slope, int64_t total, int C,
                                                                  bf16_t* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i * V < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t idx = i * V;
    const int c0 = (int)(idx % C);
    float xv[V], yv[V];
    ld_bf16<V>(x + idx, xv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int c = c0 + j;
      const float u = (xv[j] - mean[c]) * rstd[c] * gamma[c] + beta[c];
      yv[j] = u > 0.f ? u : slope * u;
    }
    st_bf16<V>(y + idx, yv);
  }
}

// training: dx = gamma * rstd * (g - (sum_g + xhat * sum_gxhat) / M); eval (train = 0): dx = gamma * rstd * g.  M = rows, or *m_total (device): all
// ranks' rows with merged sums
template <int V>
__global__ __launch_bounds__(256) void bn_lrelu_bwd_apply_bf16_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                      const float* __restrict__ sums, float slope, int64_t rows, const double* __restrict__ m_total,
                                                                      int C, int train, bf16_t* __restrict__ dx) {
  const int64_t total = rows * C;
  const float inv_m = 1.f / (m_total ? (float)*m_total : (float)rows);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i * V < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t idx = i * V;
    const int c0 = (int)(idx % C);
    float xv[V], gv[V], ov[V];
    ld_bf16<V>(x + idx, xv);
    ld_bf16<V>(dy + idx, gv);
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
    st_bf16<V>(dx + idx, ov);
  }
}

// dx = dy * (y > 0 ? 1 : slope) given the POST-activation y (slope > 0: y has the sign of the pre-activation)
template <int V>
__global__ __launch_bounds__(256) void lrelu_bwd_bf16_kernel(const bf16_t* __restrict__ y, const bf16_t* __restrict__ dy, bf16_t* __restrict__ dx,
                                                             float slope, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i * V < n; i += (int64_t)gridDim.x * blockDim.x) {
    float yv[V], gv[V], ov[V];
    ld_bf16<V>(y + i * V, yv);
    ld_bf16<V>(dy + i * V, gv);
#pragma unroll
    for (int j = 0; j < V; ++j) ov[j] = gv[j] * (yv[j] > 0.f ? 1.f : slope);
    st_bf16<V>(dx + i * V, ov);
  }
}

bool vec8(int64_t n, int C, const void* a, const void* b, const void* c) {
  return n % 8 == 0 && C % 8 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

}  // namespace

extern "C" {

// odvae_batchnorm_lrelu_fwd_f32 with x, y bf16 [rows][C]; workspace: odvae_batchnorm_workspace_bytes(rows, C) (train = 1 only)
int odvae_batchnorm_lrelu_fwd_bf16(const void* x, int64_t rows, int C, const float* gamma, const float* beta, float eps,
                                   float momentum, float slope, int train, float* mean, float* rstd,
                                   float* running_mean, float* running_var, void* y,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && gamma && beta && mean && rstd && y && rows > 0 && C > 0, "batchnorm_lrelu_fwd_bf16: bad arguments");
  ODVAE_CHECK_ARG((((uintptr_t)x | (uintptr_t)y) & 3) == 0, "batchnorm_lrelu_fwd_bf16: misaligned operand");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bf16_t* xb = static_cast<const bf16_t*>(x);
  if (train) {
    const size_t need = odvae_batchnorm_workspace_bytes(rows, C);
    if (!workspace || workspace_bytes < need) { odvae_set_error("batchnorm_lrelu_fwd_bf16: needs %zu workspace bytes", need); return ODVAE_ERR_WORKSPACE; }
    float* part = static_cast<float*>(workspace);
    const int nblk = stat_blocks(rows);
    const int rpb = (int)ceil_div64(rows, nblk);
    const int nb = (int)ceil_div64(rows, rpb);
    if (C % 2 == 0) hipLaunchKernelGGL((bn_colstats_bf16_kernel<0, 2>), dim3(nb), dim3(256), 0, st, xb, nullptr, nullptr, nullptr, nullptr, nullptr, slope, rows, C, rpb, part);
    else            hipLaunchKernelGGL((bn_colstats_bf16_kernel<0, 1>), dim3(nb), dim3(256), 0, st, xb, nullptr, nullptr, nullptr, nullptr, nullptr, slope, rows, C, rpb, part);
    hipLaunchKernelGGL(bn_finalize_bf16_kernel, dim3(ceil_div(C, 4)), dim3(256), 0, st, part, xb, nb, C, rows, eps, momentum, mean, rstd, running_mean, running_var);
  }
  const int64_t total = rows * C;
  if (vec8(total, C, x, y, nullptr))
    hipLaunchKernelGGL((bn_lrelu_apply_bf16_kernel<8>), dim3(grid_1d(total / 8)), dim3(256), 0, st, xb, mean, rstd, gamma, beta, slope, total, C, static_cast<bf16_t*>(y));
  else
    hipLaunchKernelGGL((bn_lrelu_apply_bf16_kernel<1>), dim3(grid_1d(total)), dim3(256), 0, st, xb, mean, rstd, gamma, beta, slope, total, C, static_cast<bf16_t*>(y));
  ODVAE_LAUNCH_CHECK("batchnorm_lrelu_fwd_bf16");
  return ODVAE_OK;
}

// odvae_batchnorm_lrelu_bwd_f32 with x, dy, dx bf16; dgamma, dbeta f32
int odvae_batchnorm_lrelu_bwd_bf16(const void* x, const void* dy, int64_t rows, int C, const float* gamma, const float* beta,
                                   const float* mean, const float* rstd, float slope, int train,
                                   void* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && dy && gamma && beta && mean && rstd && dx && dgamma && dbeta && rows > 0 && C > 0, "batchnorm_lrelu_bwd_bf16: bad arguments");
  ODVAE_CHECK_ARG((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 3) == 0, "batchnorm_lrelu_bwd_bf16: misaligned operand");
  const size_t need = odvae_batchnorm_workspace_bytes(rows, C);
  if (!workspace || workspace_bytes < need) { odvae_set_error("batchnorm_lrelu_bwd_bf16: needs %zu workspace bytes", need); return ODVAE_ERR_WORKSPACE; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bf16_t* xb = static_cast<const bf16_t*>(x);
  const bf16_t* gb = static_cast<const bf16_t*>(dy);
  float* part = static_cast<float*>(workspace);
  const int nblk = stat_blocks(rows);
  const int rpb = (int)ceil_div64(rows, nblk);
  const int nb = (int)ceil_div64(rows, rpb);
  float* sums = part + (size_t)nblk * 2 * C;
  if (C % 2 == 0) hipLaunchKernelGGL((bn_colstats_bf16_kernel<1, 2>), dim3(nb), dim3(256), 0, st, xb, gb, mean, rstd, gamma, beta, slope, rows, C, rpb, part);
  else            hipLaunchKernelGGL((bn_colstats_bf16_kernel<1, 1>), dim3(nb), dim3(256), 0, st, xb, gb, mean, rstd, gamma, beta, slope, rows, C, rpb, part);
  hipLaunchKernelGGL(bn_sum_partials_b_kernel, dim3(ceil_div(2 * C, 4)), dim3(256), 0, st, part, nb, C, sums);
  hipMemcpyAsync(dbeta, sums, (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, st);
  hipMemcpyAsync(dgamma, sums + C, (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, st);
  const int64_t total = rows * C;
  if (vec8(total, C, x, dy, dx))
    hipLaunchKernelGGL((bn_lrelu_bwd_apply_bf16_kernel<8>), dim3(grid_1d(total / 8)), dim3(256), 0, st, xb, gb, mean, rstd, gamma, beta, sums, slope, rows, nullptr, C, train, static_cast<bf16_t*>(dx));
  else
    hipLaunchKernelGGL((bn_lrelu_bwd_apply_bf16_kernel<1>), dim3(grid_1d(total)), dim3(256), 0, st, xb, gb, mean, rstd, gamma, beta, sums, slope, rows, nullptr, C, train, static_cast<bf16_t*>(dx));
  ODVAE_LAUNCH_CHECK("batchnorm_lrelu_bwd_bf16");
  return ODVAE_OK;
}

// ---- synchronised BatchNorm on bf16 activations: the twins of odvae_batchnorm_sync_*_f32 (merge: odvae_batchnorm_sync_stats_merge) ----
int odvae_batchnorm_sync_stats_record_bf16(const void* x, int64_t rows, int C, double* record, size_t record_bytes,
                                           void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && rows > 0 && C > 0, "batchnorm_sync_stats_record_bf16: bad arguments");
  ODVAE_CHECK_ARG(((uintptr_t)x & 3) == 0, "batchnorm_sync_stats_record_bf16: misaligned operand");
  const size_t need_rec = odvae_batchnorm_sync_record_bytes(C);
  if (!record || record_bytes < need_rec) { odvae_set_error("batchnorm_sync_stats_record_bf16: the record needs %zu bytes", need_rec); return ODVAE_ERR_WORKSPACE; }
  const size_t need = odvae_batchnorm_workspace_bytes(rows, C);
  if (!workspace || workspace_bytes < need) { odvae_set_error("batchnorm_sync_stats_record_bf16: needs %zu workspace bytes", need); return ODVAE_ERR_WORKSPACE; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bf16_t* xb = static_cast<const bf16_t*>(x);
  float* part = static_cast<float*>(workspace);
  const int nblk = stat_blocks(rows);
  const int rpb = (int)ceil_div64(rows, nblk);
  const int nb = (int)ceil_div64(rows, rpb);
  if (C % 2 == 0) hipLaunchKernelGGL((bn_colstats_bf16_kernel<0, 2>), dim3(nb), dim3(256), 0, st, xb, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, rows, C, rpb, part);
  else            hipLaunchKernelGGL((bn_colstats_bf16_kernel<0, 1>), dim3(nb), dim3(256), 0, st, xb, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, rows, C, rpb, part);
  hipLaunchKernelGGL(bn_record_bf16_kernel, dim3(ceil_div(C, 4)), dim3(256), 0, st, part, xb, nb, C, rows, record);
  ODVAE_LAUNCH_CHECK("batchnorm_sync_stats_record_bf16");
  return ODVAE_OK;
}

int odvae_batchnorm_sync_bwd_sums_bf16(const void* x, const void* dy, int64_t rows, int C, const float* gamma, const float* beta,
                                       const float* mean, const float* rstd, float slope, double* sums, size_t sums_bytes,
                                       float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && dy && gamma && beta && mean && rstd && dgamma && dbeta && rows > 0 && C > 0, "batchnorm_sync_bwd_sums_bf16: bad arguments");
  ODVAE_CHECK_ARG((((uintptr_t)x | (uintptr_t)dy) & 3) == 0, "batchnorm_sync_bwd_sums_bf16: misaligned operand");
  const size_t need_sums = odvae_batchnorm_sync_sums_bytes(C);
  if (!sums || sums_bytes < need_sums) { odvae_set_error("batchnorm_sync_bwd_sums_bf16: the sums need %zu bytes", need_sums); return ODVAE_ERR_WORKSPACE; }
  const size_t need = odvae_batchnorm_workspace_bytes(rows, C);
  if (!workspace || workspace_bytes < need) { odvae_set_error("batchnorm_sync_bwd_sums_bf16: needs %zu workspace bytes", need); return ODVAE_ERR_WORKSPACE; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bf16_t* xb = static_cast<const bf16_t*>(x);
  const bf16_t* gb = static_cast<const bf16_t*>(dy);
  float* part = static_cast<float*>(workspace);
  const int nblk = stat_blocks(rows);
  const int rpb = (int)ceil_div64(rows, nblk);
  const int nb = (int)ceil_div64(rows, rpb);
  if (C % 2 == 0) hipLaunchKernelGGL((bn_colstats_bf16_kernel<1, 2>), dim3(nb), dim3(256), 0, st, xb, gb, mean, rstd, gamma, beta, slope, rows, C, rpb, part);
  else            hipLaunchKernelGGL((bn_colstats_bf16_kernel<1, 1>), dim3(nb), dim3(256), 0, st, xb, gb, mean, rstd, gamma, beta, slope, rows, C, rpb, part);
  hipLaunchKernelGGL(bn_sum_partials_f64_b_kernel, dim3(ceil_div(2 * C, 4)), dim3(256), 0, st, part, nb, C, sums, dgamma, dbeta);
  ODVAE_LAUNCH_CHECK("batchnorm_sync_bwd_sums_bf16");
  return ODVAE_OK;
}

int odvae_batchnorm_sync_bwd_dx_bf16(const void* x, const void* dy, int64_t rows, int C, const float* gamma, const float* beta,
                                     const float* mean, const float* rstd, float slope, const double* sums_all, size_t sums_bytes,
                                     int world, const double* m_total, void* dx, void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && dy && gamma && beta && mean && rstd && dx && rows > 0 && C > 0 && world > 0 && m_total, "batchnorm_sync_bwd_dx_bf16: bad arguments");
  ODVAE_CHECK_ARG((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 3) == 0, "batchnorm_sync_bwd_dx_bf16: misaligned operand");
  const size_t need_sums = (size_t)world * odvae_batchnorm_sync_sums_bytes(C);
  if (!sums_all || sums_bytes < need_sums) { odvae_set_error("batchnorm_sync_bwd_dx_bf16: the sums need %zu bytes", need_sums); return ODVAE_ERR_WORKSPACE; }
  const size_t need = odvae_batchnorm_workspace_bytes(rows, C);
  if (!workspace || workspace_bytes < need) { odvae_set_error("batchnorm_sync_bwd_dx_bf16: needs %zu workspace bytes", need); return ODVAE_ERR_WORKSPACE; }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bf16_t* xb = static_cast<const bf16_t*>(x);
  const bf16_t* gb = static_cast<const bf16_t*>(dy);
  float* sums = static_cast<float*>(workspace) + (size_t)stat_blocks(rows) * 2 * C;
  hipLaunchKernelGGL(bn_merge_sums_b_kernel, dim3(ceil_div(2 * C, 256)), dim3(256), 0, st, sums_all, world, C, sums);
  const int64_t total = rows * C;
  if (vec8(total, C, x, dy, dx))
    hipLaunchKernelGGL((bn_lrelu_bwd_apply_bf16_kernel<8>), dim3(grid_1d(total / 8)), dim3(256), 0, st, xb, gb, mean, rstd, gamma, beta, sums, slope, rows, m_total, C, 1, static_cast<bf16_t*>(dx));
  else
    hipLaunchKernelGGL((bn_lrelu_bwd_apply_bf16_kernel<1>), dim3(grid_1d(total)), dim3(256), 0, st, xb, gb, mean, rstd, gamma, beta, sums, slope, rows, m_total, C, 1, static_cast<bf16_t*>(dx));
  ODVAE_LAUNCH_CHECK("batchnorm_sync_bwd_dx_bf16");
  return ODVAE_OK;
}

// dx = dy * (y > 0 ? 1 : slope), all bf16, y the LeakyReLU's OUTPUT (the backward of the conv epilogue of odvae_conv4x4_bf16)
int odvae_leaky_relu_bwd_bf16(const void* y, const void* dy, void* dx, float slope, int64_t n, void* stream) {
  ODVAE_CHECK_ARG(y && dy && dx && n > 0 && slope > 0.f, "leaky_relu_bwd_bf16: bad arguments");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec8(n, 8, y, dy, dx))
    hipLaunchKernelGGL((lrelu_bwd_bf16_kernel<8>), dim3(grid_1d(n / 8)), dim3(256), 0, st, static_cast<const bf16_t*>(y), static_cast<const bf16_t*>(dy), static_cast<bf16_t*>(dx), slope, n);
  else
    hipLaunchKernelGGL((lrelu_bwd_bf16_kernel<1>), dim3(grid_1d(n)), dim3(256), 0, st, static_cast<const bf16_t*>(y), static_cast<const bf16_t*>(dy), static_cast<bf16_t*>(dx), slope, n);
  ODVAE_LAUNCH_CHECK("leaky_relu_bwd_bf16");
  return ODVAE_OK;
}

}  // extern "C"
