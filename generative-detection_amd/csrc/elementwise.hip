// HBM-bound streaming / reduction kernels of the OD-VAE training step, f32, gfx950.
// All are float4-vectorised where the layout allows, wave64 shuffle reductions, fixed-order
// (deterministic) second stages.  Reference call sites are cited per kernel.
#include "common.h"

namespace {

// block-wide sum of one float per thread (256 threads); result valid in thread 0
__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  float r = 0.f;
  if (threadIdx.x == 0) for (int w = 0; w < (int)(blockDim.x >> 6); ++w) r += sh[w];
  __syncthreads();
  return r;
}

// ---- row softmax ---------------------------------------------------------------------------------
// AttnBlock.forward: w_ = softmax(bmm(q,k) * C^-0.5, dim=keys)  ([UPSTREAM] ldm .../model.py AttnBlock)
// one block per row; cols % 4 == 0.  y may alias x.
// Folded-softmax fallbacks taken since the library was loaded (odvae_device_health): a predicated softmax launch that found its flag set
// counts itself once.  Not an error -- the fallback is exact -- but a run that takes it often is paying three extra passes per block.
__device__ unsigned g_attn_fallbacks = 0;
typedef __attribute__((address_space(1))) unsigned ew_gu32_t;
__device__ __forceinline__ void count_fallback(const int* pred) {
  if (pred && blockIdx.x == 0 && threadIdx.x == 0)
    __hip_atomic_fetch_add((ew_gu32_t*)&g_attn_fallbacks, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// pred (nullable): the launch does nothing unless *pred != 0; ones (nullable): ones[row] = 1 for every row done (the folded-softmax
// fallback of ops.attention: the probabilities it writes are normalised, their row factor is 1)
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* x, float* y, int64_t rows, int cols, float scale,
                                                           const int* pred, float* ones) {
  __shared__ float sh[8];
  if (pred && *pred == 0) return;
  count_fallback(pred);
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    if (ones && threadIdx.x == 0) ones[row] = 1.f;
    const float* xr = x + row * cols;
    float* yr = y + row * cols;
    float mx = -INFINITY;
    for (int c = threadIdx.x * 4; c < cols; c += 1024) {
      const float4 v = *reinterpret_cast<const float4*>(xr + c);
      mx = fmaxf(mx, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
    __syncthreads();
    // softmax(scale*x): the max of scale*x is scale*max(x) for scale > 0
    float sum = 0.f;
    for (int c = threadIdx.x * 4; c < cols; c += 1024) {
      const float4 v = *reinterpret_cast<const float4*>(xr + c);
      sum += __expf((v.x - mx) * scale) + __expf((v.y - mx) * scale) + __expf((v.z - mx) * scale) + __expf((v.w - mx) * scale);
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) sh[4 + (threadIdx.x >> 6)] = sum;
    __syncthreads();
    const float inv = 1.f / (sh[4] + sh[5] + sh[6] + sh[7]);
    for (int c = threadIdx.x * 4; c < cols; c += 1024) {
      const float4 v = *reinterpret_cast<const float4*>(xr + c);
      float4 o;
      o.x = __expf((v.x - mx) * scale) * inv; o.y = __expf((v.y - mx) * scale) * inv;
      o.z = __expf((v.z - mx) * scale) * inv; o.w = __expf((v.w - mx) * scale) * inv;
      *reinterpret_cast<float4*>(yr + c) = o;
    }
    __syncthreads();
  }
}

// dS = scale * P * (dP - sum_j dP_j P_j);  ds may alias dp
__global__ __launch_bounds__(256) void softmax_rows_bwd_kernel(const float* p, const float* dp, float* ds, int64_t rows, int cols, float scale) {
  __shared__ float sh[4];
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const float* pr = p + row * cols;
    const float* dr = dp + row * cols;
    float* sr = ds + row * cols;
    float dot = 0.f;
    for (int c = threadIdx.x * 4; c < cols; c += 1024) {
      const float4 a = *reinterpret_cast<const float4*>(pr + c);
      const float4 b = *reinterpret_cast<const float4*>(dr + c);
      dot += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
    }
    dot = wave_sum(dot);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = dot;
    __syncthreads();
    dot = sh[0] + sh[1] + sh[2] + sh[3];
    for (int c = threadIdx.x * 4; c < cols; c += 1024) {
      const float4 a = *reinterpret_cast<const float4*>(pr + c);
      const float4 b = *reinterpret_cast<const float4*>(dr + c);
      float4 o;
      o.x = scale * a.x * (b.x - dot); o.y = scale * a.y * (b.y - dot);
      o.z = scale * a.z * (b.z - dot); o.w = scale * a.w * (b.w - dot);
      *reinterpret_cast<float4*>(sr + c) = o;
    }
    __syncthreads();
  }
}

// Register-resident forms: the whole row (NV float4 per thread, cols <= 1024*NV) is read ONCE, reduced, and written
// once: 2 HBM passes instead of 4 (forward) and 3 instead of 5 (backward).  Used whenever the row fits.
template <int NV>
__global__ __launch_bounds__(256) void softmax_rows_reg_kernel(const float* x, float* y, int64_t rows, int cols, float scale,
                                                               const int* pred, float* ones) {
  __shared__ float sh[8];
  if (pred && *pred == 0) return;
  count_fallback(pred);
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    if (ones && threadIdx.x == 0) ones[row] = 1.f;
    const float* xr = x + row * cols;
    float4 v[NV];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (threadIdx.x + 256 * i) * 4;
      // branch-free: clamp the address, select afterwards (a guarded load makes hipcc wait vmcnt(0) per load)
      const float4 ld = *reinterpret_cast<const float4*>(xr + min(c, cols - 4));
      v[i] = c < cols ? ld : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      mx = fmaxf(mx, fmaxf(fmaxf(v[i].x, v[i].y), fmaxf(v[i].z, v[i].w)));
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      v[i].x = __expf((v[i].x - mx) * scale); v[i].y = __expf((v[i].y - mx) * scale);
      v[i].z = __expf((v[i].z - mx) * scale); v[i].w = __expf((v[i].w - mx) * scale);
      sum += v[i].x + v[i].y + v[i].z + v[i].w;      // exp(-inf) = 0 for the padding lanes
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) sh[4 + (threadIdx.x >> 6)] = sum;
    __syncthreads();
    const float inv = 1.f / (sh[4] + sh[5] + sh[6] + sh[7]);
    float* yr = y + row * cols;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (threadIdx.x + 256 * i) * 4;
      if (c < cols) *reinterpret_cast<float4*>(yr + c) = make_float4(v[i].x * inv, v[i].y * inv, v[i].z * inv, v[i].w * inv);
    }
    __syncthreads();
  }
}

template <int NV>
__global__ __launch_bounds__(256) void softmax_rows_bwd_reg_kernel(const float* p, const float* dp, float* ds, int64_t rows, int cols, float scale) {
  __shared__ float sh[4];
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const float* pr = p + row * cols;
    const float* dr = dp + row * cols;
    float4 a[NV], b[NV];
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (threadIdx.x + 256 * i) * 4;
      const float4 la = *reinterpret_cast<const float4*>(pr + min(c, cols - 4));
      const float4 lb = *reinterpret_cast<const float4*>(dr + min(c, cols - 4));
      a[i] = c < cols ? la : make_float4(0.f, 0.f, 0.f, 0.f);
      b[i] = c < cols ? lb : make_float4(0.f, 0.f, 0.f, 0.f);
      dot += a[i].x * b[i].x + a[i].y * b[i].y + a[i].z * b[i].z + a[i].w * b[i].w;
    }
    dot = wave_sum(dot);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = dot;
    __syncthreads();
    dot = sh[0] + sh[1] + sh[2] + sh[3];
    float* sr = ds + row * cols;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (threadIdx.x + 256 * i) * 4;
      if (c < cols)
        *reinterpret_cast<float4*>(sr + c) = make_float4(scale * a[i].x * (b[i].x - dot), scale * a[i].y * (b[i].y - dot),
                                                         scale * a[i].z * (b[i].z - dot), scale * a[i].w * (b[i].w - dot));
    }
    __syncthreads();
  }
}

// ---- backward of nearest 2x upsample: dX[n][y][x][c] = sum of the 2x2 block of dU --------------------
// (Upsample.forward: F.interpolate(scale_factor=2.0, mode="nearest"), [UPSTREAM] ldm .../model.py)
__global__ __launch_bounds__(256) void upsample2x_bwd_kernel(const float* __restrict__ du, float* __restrict__ dx,
                                                             int N, int H, int W, int C) {
  const int quads = C / 4;
  const int64_t total = (int64_t)N * H * W * quads;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int q = (int)(idx % quads);
    int64_t r = idx / quads;
    const int xw = (int)(r % W); r /= W;
    const int yh = (int)(r % H); const int n = (int)(r / H);
    const float* s = du + (((int64_t)n * 2 * H + 2 * yh) * 2 * W + 2 * xw) * C + 4 * q;
    const float4 a = *reinterpret_cast<const float4*>(s);
    const float4 b = *reinterpret_cast<const float4*>(s + C);
    const float4 c = *reinterpret_cast<const float4*>(s + (int64_t)2 * W * C);
    const float4 d = *reinterpret_cast<const float4*>(s + (int64_t)2 * W * C + C);
    *reinterpret_cast<float4*>(dx + idx * 4) =
        make_float4(a.x + b.x + c.x + d.x, a.y + b.y + c.y + d.y, a.z + b.z + c.z + d.z, a.w + b.w + c.w + d.w);
  }
}

// ---- conv-less resamplers (ddconfig.resamp_with_conv = False) and Decoder(tanh_out=True) ----------------
// streaming accesses, as the GroupNorm apply passes: every byte is touched once here and next by another kernel
typedef float ew_f4 __attribute__((ext_vector_type(4)));
struct RsF32 {
  typedef float elem_t;
  static constexpr int W = 4;
  static __device__ __forceinline__ void load(const float* p, float (&f)[4]) {
    const ew_f4 v = __builtin_nontemporal_load(reinterpret_cast<const ew_f4*>(p));
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  }
  static __device__ __forceinline__ void store(float* p, float (&f)[4]) {
    __builtin_nontemporal_store(ew_f4{f[0], f[1], f[2], f[3]}, reinterpret_cast<ew_f4*>(p));
  }
};
#include "resample.h"

// y = tanh(x) on a flat array ([UPSTREAM] Decoder.forward: `if self.tanh_out: h = torch.tanh(h)`); float4 body where the pointers allow
// Plain (cached) accesses, unlike the resamplers' streaming ones: the reconstruction is 3 channels (25 MB at B = 32, 256 x 256) and the loss kernels
// read it next, y again in the backward -- it should stay in the cache, not pass it by.
__global__ __launch_bounds__(256) void tanh_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, int vec) {
  const int64_t n4 = vec ? n / 4 : 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    reinterpret_cast<float4*>(y)[i] = make_float4(tanhf(v.x), tanhf(v.y), tanhf(v.z), tanhf(v.w));
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) y[i] = tanhf(x[i]);
}
// dx = dy * (1 - y^2): only y is kept
__global__ __launch_bounds__(256) void tanh_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy, float* __restrict__ dx,
                                                       int64_t n, int vec) {
  const int64_t n4 = vec ? n / 4 : 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(y)[i], g = reinterpret_cast<const float4*>(dy)[i];
    reinterpret_cast<float4*>(dx)[i] = make_float4(g.x * (1.f - v.x * v.x), g.y * (1.f - v.y * v.y), g.z * (1.f - v.z * v.z), g.w * (1.f - v.w * v.w));
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dx[i] = dy[i] * (1.f - y[i] * y[i]);
}

// ---- batch min/max rescale: 2(x-min)/(max-min)-1  (src/models/autoencoder.py:434-436) -----------------
__global__ __launch_bounds__(256) void minmax_partial_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ part) {
  __shared__ float sh[8];
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = x[i];
    mn = fminf(mn, v); mx = fmaxf(mx, v);
  }
  mn = wave_min(mn); mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = mn; sh[4 + (threadIdx.x >> 6)] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = fminf(fminf(sh[0], sh[1]), fminf(sh[2], sh[3]));
    part[2 * blockIdx.x + 1] = fmaxf(fmaxf(sh[4], sh[5]), fmaxf(sh[6], sh[7]));
  }
}
__global__ void minmax_final_kernel(const float* __restrict__ part, int nblocks, float* __restrict__ out) {
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < nblocks; i += 64) { mn = fminf(mn, part[2 * i]); mx = fmaxf(mx, part[2 * i + 1]); }
  mn = wave_min(mn); mx = wave_max(mx);
  if (threadIdx.x == 0) { out[0] = mn; out[1] = mx; }
}
// x: NCHW [N][C][HW] -> y: NHWC [N][HW][C], y = 2(x-min)/(max-min)-1 (same operation order as the reference)
__global__ __launch_bounds__(256) void rescale_nchw_to_nhwc_kernel(const float* __restrict__ x, const float* __restrict__ mm,
                                                                   float* __restrict__ y, int N, int C, int HW) {
  const float mn = mm[0], range = mm[1] - mm[0];
  const int64_t total = (int64_t)N * HW * C;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    const int64_t r = idx / C;
    const int hw = (int)(r % HW); const int n = (int)(r / HW);
    const float v = x[((int64_t)n * C + c) * HW + hw];
    y[idx] = 2.f * (v - mn) / range - 1.f;
  }
}

// ---- diagonal Gaussian posterior (src/util/distributions.py:5-41 + [UPSTREAM] ldm distributions) -----
// moments: NHWC [N][HW][2*Cz]; mean = channels [0,Cz), logvar = channels [Cz,2Cz) clamped to [-30,20].
// z = mean + exp(0.5*logvar)*eps  (eps: [N][HW][Cz], injected by the host)
__global__ __launch_bounds__(256) void gaussian_sample_kernel(const float* __restrict__ mom, const float* __restrict__ eps,
                                                              float* __restrict__ z, int64_t npix, int Cz) {
  const int64_t total = npix * Cz;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % Cz); const int64_t px = idx / Cz;
    const float mu = mom[px * 2 * Cz + c];
    const float lv = fminf(fmaxf(mom[px * 2 * Cz + Cz + c], -30.f), 20.f);
    z[idx] = mu + expf(0.5f * lv) * eps[idx];
  }
}
// kl[n] = 0.5 * sum_{hw,c} (mean^2 + var - 1 - logvar); one block per sample
__global__ __launch_bounds__(256) void gaussian_kl_kernel(const float* __restrict__ mom, float* __restrict__ kl, int HW, int Cz) {
  __shared__ float sh[4];
  const int n = blockIdx.x;
  const int64_t per = (int64_t)HW * Cz;
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < per; i += blockDim.x) {
    const int c = (int)(i % Cz); const int64_t px = (int64_t)n * HW + i / Cz;
    const float mu = mom[px * 2 * Cz + c];
    const float lv = fminf(fmaxf(mom[px * 2 * Cz + Cz + c], -30.f), 20.f);
    s += mu * mu + expf(lv) - 1.f - lv;
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) kl[n] = 0.5f * s;
}
// dmom from dz (may be null), eps (null iff dz null) and dkl[n] (may be null)
__global__ __launch_bounds__(256) void gaussian_bwd_kernel(const float* __restrict__ mom, const float* __restrict__ eps,
                                                           const float* __restrict__ dz, const float* __restrict__ dkl,
                                                           float* __restrict__ dmom, int N, int HW, int Cz) {
  const int64_t total = (int64_t)N * HW * Cz;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % Cz); const int64_t px = idx / Cz;
    const int n = (int)(px / HW);
    const float mu = mom[px * 2 * Cz + c];
    const float lraw = mom[px * 2 * Cz + Cz + c];
    const float lv = fminf(fmaxf(lraw, -30.f), 20.f);
    const bool pass = lraw >= -30.f && lraw <= 20.f;  // d clamp / d x
    float dmu = 0.f, dlv = 0.f;
    if (dz) { const float g = dz[idx]; dmu += g; dlv += g * eps[idx] * 0.5f * expf(0.5f * lv); }
    if (dkl) { const float g = dkl[n]; dmu += g * mu; dlv += g * 0.5f * (expf(lv) - 1.f); }
    dmom[px * 2 * Cz + c] = dmu;
    dmom[px * 2 * Cz + Cz + c] = pass ? dlv : 0.f;
  }
}

// ---- masked L1 reconstruction term (src/modules/losses/contperceptual.py:134-145,252-257) ------------
// s[n] = sum_{hw,c} | x*m - xr*m |, x/xr NHWC [N][HW][C], m [N][HW] or null.  Stage 1: partial[n][blk]
__global__ __launch_bounds__(256) void l1_partial_kernel(const float* __restrict__ x, const float* __restrict__ xr,
                                                         const float* __restrict__ m, float* __restrict__ part, int HW, int C) {
  __shared__ float sh[4];
  const int n = blockIdx.y;
  const int64_t per = (int64_t)HW * C;
  const float* xa = x + n * per; const float* xb = xr + n * per;
  const float* mk = m ? m + (int64_t)n * HW : nullptr;
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (int64_t)gridDim.x * blockDim.x) {
    const float w = mk ? mk[i / C] : 1.f;
    s += fabsf(xa[i] * w - xb[i] * w);
  }
  s = block_sum(s, sh);
  if (threadIdx.x == 0) part[(int64_t)n * gridDim.x + blockIdx.x] = s;
}
__global__ void rowsum_final_kernel(const float* __restrict__ part, int nblk, float* __restrict__ out) {
  const int n = blockIdx.x;
  double s = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 64) s += (double)part[(int64_t)n * nblk + i];
  s = wave_sum_f64(s);
  if (threadIdx.x == 0) out[n] = (float)s;
}
// dxr = g[n] * sign(xr*m - x*m) * m
__global__ __launch_bounds__(256) void l1_bwd_kernel(const float* __restrict__ x, const float* __restrict__ xr,
                                                     const float* __restrict__ m, const float* __restrict__ g,
                                                     float* __restrict__ dxr, int N, int HW, int C) {
  const int64_t per = (int64_t)HW * C, total = per * N;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(idx / per);
    const float w = m ? m[idx / C] : 1.f;
    const float d = xr[idx] * w - x[idx] * w;
    const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    dxr[idx] = g[n] * sg * w;
  }
}

// ---- RGBA reconstruction terms (image_mask_key: contperceptual.py:230-257,166-174 on a 4-channel reconstruction) ----------------
// One pass over rec [N][HW][4] (one 16-byte load per pixel), rgb [N][HW][3] (three 4-byte loads: any 4-byte aligned base), alpha [N][HW]
// and box [N][HW] (nullable = 1).  Per pixel, every operation separately rounded (plain operators under
// `fp contract(off)`: hipcc fuses xm - rec * w into one multiply-add otherwise, and __fmul_rn does not stop it):
//   xm_c = rgb_c * w, rm_c = rec_c * w (c < 3), am = alpha * w, ra = rec_3 * w
//   l1 += |xm_0 - rm_0| + |xm_1 - rm_1| + |xm_2 - rm_2|  (added in this order),  d = am - ra,  mask += |d| (l1) or d * d (l2)
// and the four masked copies, each skipped when its pointer is null.  Stage 1 leaves part[0][n][blk] (l1) and part[1][n][blk] (mask);
// rgba_final_kernel adds a sample's partials in f64 in a fixed order: no atomics.
__global__ __launch_bounds__(256) void rgba_terms_kernel(const float4* __restrict__ rec, const float* __restrict__ rgb, const float* __restrict__ alpha,
                                                         const float* __restrict__ box, float* __restrict__ part, float* __restrict__ rec_rgb_m,
                                                         float* __restrict__ gt_rgb_m, float4* __restrict__ rec_rgba_m, float4* __restrict__ gt_rgba_m,
                                                         int HW, int l2) {
#pragma clang fp contract(off)
  __shared__ float sh[4];
  const int n = blockIdx.y, N = gridDim.y;
  const int64_t base = (int64_t)n * HW;
  float s1 = 0.f, s2 = 0.f;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < HW; p += (int64_t)gridDim.x * 256) {
    const int64_t px = base + p;
    const float4 r = rec[px];
    const float w = box ? box[px] : 1.f;
    const float x0 = rgb[px * 3] * w, x1 = rgb[px * 3 + 1] * w, x2 = rgb[px * 3 + 2] * w;
    const float am = alpha[px] * w;
    const float4 rm = make_float4(r.x * w, r.y * w, r.z * w, r.w * w);
    float t = fabsf(x0 - rm.x);
    t = t + fabsf(x1 - rm.y);
    t = t + fabsf(x2 - rm.z);
    s1 = s1 + t;
    const float d = am - rm.w;
    s2 = s2 + (l2 ? d * d : fabsf(d));
    if (rec_rgb_m) { rec_rgb_m[px * 3] = rm.x; rec_rgb_m[px * 3 + 1] = rm.y; rec_rgb_m[px * 3 + 2] = rm.z; }
    if (gt_rgb_m) { gt_rgb_m[px * 3] = x0; gt_rgb_m[px * 3 + 1] = x1; gt_rgb_m[px * 3 + 2] = x2; }
    if (rec_rgba_m) rec_rgba_m[px] = rm;
    if (gt_rgba_m) gt_rgba_m[px] = make_float4(x0, x1, x2, am);
  }
  if (!part) return;      // (block-uniform) the caller wants the masked copies alone: the discriminator phase
  s1 = block_sum(s1, sh);
  s2 = block_sum(s2, sh);
  if (threadIdx.x == 0) {
    part[(int64_t)n * gridDim.x + blockIdx.x] = s1;
    part[((int64_t)N + n) * gridDim.x + blockIdx.x] = s2;
  }
}
// grid (N, 2): out0[n] / out1[n] = the sum of the sample's nblk partials
__global__ void rgba_final_kernel(const float* __restrict__ part, int nblk, float* __restrict__ out0, float* __restrict__ out1) {
  const int n = blockIdx.x, which = blockIdx.y, N = gridDim.x;
  const float* p = part + ((int64_t)which * N + n) * nblk;
  double s = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 64) s += (double)p[i];
  s = wave_sum_f64(s);
  if (threadIdx.x == 0) (which ? out1 : out0)[n] = (float)s;
}
// d_rec [N][HW][4], overwritten.  c < 3: ((g_l1[n] * sign(rm_c - xm_c)) * w + g_rgb_c * w) + g_rgba_c * w (l1_bwd_kernel's sign rule);
// c = 3: (g_mask[n] * (sign(ra - am) or 2 * (ra - am))) * w + g_rgba_3 * w.  A null gradient is a zero and adds nothing.
__global__ __launch_bounds__(256) void rgba_terms_bwd_kernel(const float4* __restrict__ rec, const float* __restrict__ rgb, const float* __restrict__ alpha,
                                                             const float* __restrict__ box, const float* __restrict__ g_l1, const float* __restrict__ g_mask,
                                                             const float* __restrict__ g_rgb, const float4* __restrict__ g_rgba, float4* __restrict__ d_rec,
                                                             int HW, int l2) {
#pragma clang fp contract(off)
  const int n = blockIdx.y;      // grid (blocks, N), as the forward: no division per pixel
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < HW; q += (int64_t)gridDim.x * 256) {
    const int64_t px = (int64_t)n * HW + q;
    const float w = box ? box[px] : 1.f;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (g_l1) {
      const float4 r = rec[px];
      const float g = g_l1[n];
      const float rv[3] = {r.x, r.y, r.z};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float a = rv[c] * w, b = rgb[px * 3 + c] * w;
        const float d = a - b;
        const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        o[c] = (g * sg) * w;
      }
    }
    if (g_mask) {
      const float a = rec[px].w * w, b = alpha[px] * w;
      const float d = a - b;
      const float e = l2 ? 2.f * d : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
      o[3] = (g_mask[n] * e) * w;
    }
    if (g_rgb) {
#pragma unroll
      for (int c = 0; c < 3; ++c) { const float t = g_rgb[px * 3 + c] * w; o[c] = o[c] + t; }
    }
    if (g_rgba) {
      const float4 g = g_rgba[px];
      const float t0 = g.x * w, t1 = g.y * w, t2 = g.z * w, t3 = g.w * w;
      o[0] = o[0] + t0; o[1] = o[1] + t1; o[2] = o[2] + t2; o[3] = o[3] + t3;
    }
    d_rec[px] = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// ---- weighted L1 sums (the `weights` argument of the losses: contperceptual.py:147-158 with a weight map) ------------------------------
// One pass over x [N][HW][C], the first C channels of xr [N][HW][Cr], box [N][HW] (nullable = 1) and wgt ([N][HW], or [N][HW][C] when
// per_channel).  Per element, every operation separately rounded, as in rgba_terms_kernel:
//   xm = x * b, rm = xr * b, t = |xm - rm|,  l1 += t,  wl1 += wgt * t,  w += wgt   (a per-pixel weight is added once per channel)
// x == null (then xr is not read either): the weight sums alone.  Stage 1 leaves part[k][n][blk], k = 0 (l1), 1 (wl1), 2 (w); sums3_final_kernel
// adds a sample's partials in f64 in a fixed order: no atomics.  CC: the channel count when it is known at compile time (0 = C_rt);
// V4 (CC > 0, Cr == 4, xr 16-byte aligned): the reconstruction's pixel is one 16-byte load.
template <int CC, bool V4>
__global__ __launch_bounds__(256) void l1_weighted_kernel(const float* __restrict__ x, const float* __restrict__ xr, const float* __restrict__ box,
                                                          const float* __restrict__ wgt, float* __restrict__ part, int HW, int C_rt, int Cr,
                                                          int per_channel) {
#pragma clang fp contract(off)
  __shared__ float sh[4];
  const int C = CC ? CC : C_rt;
  const int n = blockIdx.y, N = gridDim.y;
  const int64_t base = (int64_t)n * HW;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < HW; p += (int64_t)gridDim.x * 256) {
    const int64_t px = base + p;
    const float wp = per_channel ? 0.f : wgt[px];
    if (!x) {      // (block-uniform) the pixel term is off: W[n] alone
      for (int c = 0; c < C; ++c) s2 = s2 + (per_channel ? wgt[px * C + c] : wp);
      continue;
    }
    const float b = box ? box[px] : 1.f;
    if constexpr (V4) {
      const float4 r = reinterpret_cast<const float4*>(xr)[px];
      const float rv[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int c = 0; c < CC; ++c) {
        const float w = per_channel ? wgt[px * CC + c] : wp;
        const float xm = x[px * CC + c] * b, rm = rv[c] * b;
        const float t = fabsf(xm - rm);
        const float wt = w * t;
        s0 = s0 + t; s1 = s1 + wt; s2 = s2 + w;
      }
    } else {
      for (int c = 0; c < C; ++c) {
        const float w = per_channel ? wgt[px * C + c] : wp;
        const float xm = x[px * C + c] * b, rm = xr[px * Cr + c] * b;
        const float t = fabsf(xm - rm);
        const float wt = w * t;
        s0 = s0 + t; s1 = s1 + wt; s2 = s2 + w;
      }
    }
  }
  s0 = block_sum(s0, sh);
  s1 = block_sum(s1, sh);
  s2 = block_sum(s2, sh);
  if (threadIdx.x == 0) {
    part[(int64_t)n * gridDim.x + blockIdx.x] = s0;
    part[((int64_t)N + n) * gridDim.x + blockIdx.x] = s1;
    part[((int64_t)2 * N + n) * gridDim.x + blockIdx.x] = s2;
  }
}
// grid (N, 3): out_k[n] = the sum of the sample's nblk partials of term k; a null out_k is skipped
__global__ void sums3_final_kernel(const float* __restrict__ part, int nblk, float* __restrict__ out0, float* __restrict__ out1,
                                   float* __restrict__ out2) {
  const int n = blockIdx.x, which = blockIdx.y, N = gridDim.x;
  float* out = which == 0 ? out0 : (which == 1 ? out1 : out2);
  if (!out) return;
  const float* p = part + ((int64_t)which * N + n) * nblk;
  double s = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 64) s += (double)p[i];
  s = wave_sum_f64(s);
  if (threadIdx.x == 0) out[n] = (float)s;
}
// dxr [N][HW][Cr], overwritten.  c < C: ((g_l1[n] + g_wl1[n] * wgt) * sign(rm - xm)) * b (l1_bwd_kernel's sign rule: 0 at a tie), a null
// gradient a zero; c >= C: 0.  V4: dxr and xr are 16-byte aligned and Cr == 4.
template <int CC, bool V4>
__global__ __launch_bounds__(256) void l1_weighted_bwd_kernel(const float* __restrict__ x, const float* __restrict__ xr, const float* __restrict__ box,
                                                              const float* __restrict__ wgt, const float* __restrict__ g_l1,
                                                              const float* __restrict__ g_wl1, float* __restrict__ dxr, int HW, int C_rt, int Cr,
                                                              int per_channel) {
#pragma clang fp contract(off)
  const int C = CC ? CC : C_rt;
  const int n = blockIdx.y;
  const float gl = g_l1 ? g_l1[n] : 0.f, gw = g_wl1 ? g_wl1[n] : 0.f;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < HW; q += (int64_t)gridDim.x * 256) {
    const int64_t px = (int64_t)n * HW + q;
    const float b = box ? box[px] : 1.f;
    const float wp = per_channel ? 0.f : wgt[px];
    if constexpr (V4) {
      const float4 r = reinterpret_cast<const float4*>(xr)[px];
      const float rv[4] = {r.x, r.y, r.z, r.w};
      float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < CC; ++c) {
        const float w = per_channel ? wgt[px * CC + c] : wp;
        const float d = rv[c] * b - x[px * CC + c] * b;
        const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        const float gwt = gw * w;
        const float g = gl + gwt;
        o[c] = (g * sg) * b;
      }
      reinterpret_cast<float4*>(dxr)[px] = make_float4(o[0], o[1], o[2], o[3]);
    } else {
      for (int c = 0; c < C; ++c) {
        const float w = per_channel ? wgt[px * C + c] : wp;
        const float d = xr[px * Cr + c] * b - x[px * C + c] * b;
        const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        const float gwt = gw * w;
        const float g = gl + gwt;
        dxr[px * Cr + c] = (g * sg) * b;
      }
      for (int c = C; c < Cr; ++c) dxr[px * Cr + c] = 0.f;
    }
  }
}

// ---- discriminator input under disc_conditional: y = cat(x * box, cond) along the channels (contperceptual.py:283-289,354-361) ----------
// x [N][HW][Cx], box [N][HW] (nullable = 1), cond [N][HW][Cc], y [N][HW][Cy], Cy = Cx + Cc.  One thread per OUTPUT element: consecutive
// lanes store consecutive floats, and read x / cond nearly so.  grid (blocks, N); a sample's HW * Cy elements are counted in 32 bits (the
// launcher checks), so the pixel of an element is one 32-bit division -- by a constant where CY names the row width (0 = Cy_rt).
template <int CY>
__global__ __launch_bounds__(256) void cat_mask_kernel(const float* __restrict__ x, const float* __restrict__ box, const float* __restrict__ cond,
                                                       float* __restrict__ y, int HW, int Cx, int Cy_rt) {
  const uint32_t Cy = CY ? (uint32_t)CY : (uint32_t)Cy_rt, cx = (uint32_t)Cx, cc = Cy - cx;
  const int n = blockIdx.y;
  const float* xa = x + (int64_t)n * HW * cx;
  const float* ca = cond + (int64_t)n * HW * cc;
  const float* bx = box ? box + (int64_t)n * HW : nullptr;
  float* ya = y + (int64_t)n * HW * Cy;
  const uint32_t per = (uint32_t)HW * Cy;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < per; i += gridDim.x * 256u) {
    const uint32_t p = i / Cy, c = i - p * Cy;
    float v;
    if (c < cx) { v = xa[(int64_t)p * cx + c]; if (bx) v = v * bx[p]; }
    else v = ca[(int64_t)p * cc + (c - cx)];
    ya[i] = v;
  }
}
// Cy == 4 and y 16-byte aligned: one thread per pixel, one 16-byte store
__global__ __launch_bounds__(256) void cat_mask_px4_kernel(const float* __restrict__ x, const float* __restrict__ box, const float* __restrict__ cond,
                                                           float4* __restrict__ y, int HW, int Cx) {
  const int n = blockIdx.y, Cc = 4 - Cx;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < HW; q += (int64_t)gridDim.x * 256) {
    const int64_t px = (int64_t)n * HW + q;
    const float b = box ? box[px] : 1.f;
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = c < Cx ? x[px * Cx + c] * b : cond[px * Cc + (c - Cx)];
    y[px] = make_float4(v[0], v[1], v[2], v[3]);
  }
}
// dx [N][HW][Cx] = dy[..., :Cx] * box: one thread per element of dx (CX: the row width of dx when known at compile time, 0 = Cx_rt)
template <int CX>
__global__ __launch_bounds__(256) void cat_mask_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ box, float* __restrict__ dx,
                                                           int HW, int Cx_rt, int Cy) {
  const uint32_t cx = CX ? (uint32_t)CX : (uint32_t)Cx_rt;
  const int n = blockIdx.y;
  const float* ga = dy + (int64_t)n * HW * Cy;
  const float* bx = box ? box + (int64_t)n * HW : nullptr;
  float* da = dx + (int64_t)n * HW * cx;
  const uint32_t per = (uint32_t)HW * cx;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < per; i += gridDim.x * 256u) {
    const uint32_t p = i / cx, c = i - p * cx;
    float v = ga[(int64_t)p * Cy + c];
    if (bx) v = v * bx[p];
    da[i] = v;
  }
}

// ---- column sums (bias gradient of the 1x1 convolutions): out[c] = sum_rows x[row][c] ------------------
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ x, int64_t rows, int C,
                                                             int rows_per_block, float* __restrict__ part) {
  // thread t handles column (t % C) for C <= 256 (several row lanes), else strides over columns
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = std::min<int64_t>(rows, r0 + rows_per_block);
  if ((C & 3) == 0 && C <= 1024 && (((uintptr_t)x) & 15) == 0) {
    // channel quads: thread = (quad, row lane); 16-byte loads, four rows in flight per thread (the scalar form below runs
    // one dependent 4-byte load at a time: 2 TB/s on the 1x1 convolutions' 0.1-0.5 GB inputs)
    __shared__ float4 sh4[256];
    const int Q = C >> 2, lanes = 256 / Q;
    const int q = threadIdx.x % Q, rl = threadIdx.x / Q;
    float4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rl < lanes) {
      const float4* xq = reinterpret_cast<const float4*>(x) + q;
      int64_t r = r0 + rl;
      for (; r + 3 * lanes < r1; r += 4 * lanes) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = xq[(r + (int64_t)u * lanes) * Q];
#pragma unroll
        for (int u = 0; u < 4; ++u) { acc[u].x += v[u].x; acc[u].y += v[u].y; acc[u].z += v[u].z; acc[u].w += v[u].w; }
      }
      for (; r < r1; r += lanes) { const float4 v = xq[r * Q]; acc[0].x += v.x; acc[0].y += v.y; acc[0].z += v.z; acc[0].w += v.w; }
    }
    sh4[threadIdx.x] = make_float4((acc[0].x + acc[1].x) + (acc[2].x + acc[3].x), (acc[0].y + acc[1].y) + (acc[2].y + acc[3].y),
                                   (acc[0].z + acc[1].z) + (acc[2].z + acc[3].z), (acc[0].w + acc[1].w) + (acc[2].w + acc[3].w));
    __syncthreads();
    if (threadIdx.x < Q) {
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k = 0; k < lanes; ++k) { const float4 v = sh4[k * Q + threadIdx.x]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
      *reinterpret_cast<float4*>(part + (int64_t)blockIdx.x * C + 4 * threadIdx.x) = t;
    }
  } else if (C <= 256) {
    __shared__ float sh[256];
    const int lanes = 256 / C;
    const int c = threadIdx.x % C, rl = threadIdx.x / C;
    float s = 0.f;
    if (rl < lanes) for (int64_t r = r0 + rl; r < r1; r += lanes) s += x[r * C + c];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < C) {
      float t = 0.f;
      for (int k = 0; k < lanes; ++k) t += sh[k * C + threadIdx.x];
      part[(int64_t)blockIdx.x * C + threadIdx.x] = t;
    }
  } else {
    for (int c = threadIdx.x; c < C; c += 256) {
      float s = 0.f;
      for (int64_t r = r0; r < r1; ++r) s += x[r * C + c];
      part[(int64_t)blockIdx.x * C + c] = s;
    }
  }
}
// one wavefront per column: lanes stride over the partial blocks, f64 wave reduction (fixed order => deterministic)
__global__ void colsum_final_kernel(const float* __restrict__ part, int nblk, int C, float* __restrict__ out) {
  const int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (c >= C) return;
  double s = 0.0;
  for (int b = threadIdx.x & 63; b < nblk; b += 64) s += (double)part[(int64_t)b * C + c];
  s = wave_sum_f64(s);
  if ((threadIdx.x & 63) == 0) out[c] = (float)s;
}

// ---- optimizer: global grad norm + Adam over one flat arena (src/models/autoencoder.py:365-377, yaml:140)
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ part) {
  __shared__ float sh[4];
  float s = 0.f;
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(g)[i];
    s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  if (blockIdx.x == 0) for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) s += g[i] * g[i];
  s = block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
// out[0] = total norm, out[1] = clip coefficient min(1, max_norm/(norm+1e-6)) (torch clip_grad_norm_)
__global__ void norm_final_kernel(const float* __restrict__ part, int nblk, float max_norm, float* __restrict__ out) {
  double s = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 64) s += (double)part[i];
  s = wave_sum_f64(s);
  if (threadIdx.x == 0) {
    const float nrm = (float)sqrt(s);
    out[0] = nrm;
    float coef = 1.f;
    if (max_norm > 0.f) { coef = max_norm / (nrm + 1e-6f); if (coef > 1.f) coef = 1.f; }
    out[1] = coef;
  }
}
// torch.optim.Adam (no weight decay, no amsgrad).  CLAMP = false: grads are scaled by *clip (device scalar) when non-null.  CLAMP = true
// (gradient_clip_algorithm: value): grads go through torch.clamp(g, -clamp, +clamp) instead -- two compares and selects, so NaN stays NaN,
// +-inf becomes +-clamp and -0.0 stays -0.0 (fminf / fmaxf would turn NaN into the bound)
template <bool CLAMP>
__device__ __forceinline__ float adam_grad(float g, float cs) {
  if (CLAMP) return g < -cs ? -cs : (g > cs ? cs : g);
  return g * cs;
}
template <bool CLAMP>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                   float lr, float beta1, float beta2, float eps,
                                                   float bc1, float bc2_sqrt, const float* __restrict__ clip, float clamp) {
  const float cs = CLAMP ? clamp : (clip ? clip[1] : 1.f);
  const float step = lr / bc1;
  const int64_t n4 = n / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float pp[4] = {pv.x, pv.y, pv.z, pv.w}, gg[4] = {gv.x, gv.y, gv.z, gv.w};
    float mm[4] = {mv.x, mv.y, mv.z, mv.w}, ww[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gr = adam_grad<CLAMP>(gg[j], cs);
      mm[j] = beta1 * mm[j] + (1.f - beta1) * gr;
      ww[j] = beta2 * ww[j] + (1.f - beta2) * gr * gr;
      pp[j] -= step * mm[j] / (sqrtf(ww[j]) / bc2_sqrt + eps);
    }
    reinterpret_cast<float4*>(p)[i] = make_float4(pp[0], pp[1], pp[2], pp[3]);
    reinterpret_cast<float4*>(m)[i] = make_float4(mm[0], mm[1], mm[2], mm[3]);
    reinterpret_cast<float4*>(v)[i] = make_float4(ww[0], ww[1], ww[2], ww[3]);
  }
  if (blockIdx.x == 0)
    for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) {
      const float gr = adam_grad<CLAMP>(g[i], cs);
      const float mi = beta1 * m[i] + (1.f - beta1) * gr;
      const float vi = beta2 * v[i] + (1.f - beta2) * gr * gr;
      m[i] = mi; v[i] = vi;
      p[i] -= step * mi / (sqrtf(vi) / bc2_sqrt + eps);
    }
}

// ---- segmented p-norms of one flat arena (Trainer(track_grad_norm=p), optim.FusedAdam.grad_norms): per-segment norms and their total.
// Stage 1 (one launch per kSegNormSegs segments, the table a by-value kernel argument): a segment is cut into chunks of kSegNormChunk floats,
// one block reduces one chunk to one double in the workspace; the block of a segment's first chunk also writes that segment's
// {first partial, partials, counts} record there, so the later stages need no table.  Stage 2: one wavefront per segment folds its partials
// and writes out[seg].  Stage 3: one block folds the f32-rounded out[] of the counting segments into out[n_seg].  Everything is summed in
// f64 in an order fixed by the chunk grid alone (thread -> wave butterfly -> waves in order; partials lane-strided -> butterfly): no atomics,
// the same bits on any launch grid.  A chunk never reads outside its segment: float4 up to the last whole one, then at most 3 scalars.
constexpr int kSegNormSegs = 160;
constexpr int kSegNormChunk = 4096;      // floats: four float4 per thread of a 256-thread block
enum { kNormMax = 0, kNormL1 = 1, kNormL2 = 2, kNormP = 3 };
struct SegNormTable {
  int64_t off[kSegNormSegs];
  int64_t len[kSegNormSegs];
  unsigned chunk_prefix[kSegNormSegs + 1];
  unsigned char counts[kSegNormSegs];
  int count;
  int seg_base;            // index of this launch's first segment in out[] / the records
  unsigned chunk_base;     // partials in front of this launch's first chunk
};
static_assert(sizeof(SegNormTable) <= 3900, "the segment table travels in the kernel arguments (4 KiB) beside four scalars");
struct SegNormRecord { unsigned first, chunks, counts, pad; };

// torch.norm(inf) propagates NaN; fmax drops it
__device__ __forceinline__ double nan_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
template <int KIND>
__device__ __forceinline__ double norm_take(double s, float x, double p) {
  const double a = (double)fabsf(x);
  if (KIND == kNormMax) return nan_max(s, a);
  if (KIND == kNormL1) return s + a;
  if (KIND == kNormL2) return s + a * a;      // (the product of two f32 is exact in f64)
  return s + pow(a, p);
}
template <int KIND>
__device__ __forceinline__ double norm_fold(double a, double b) { return KIND == kNormMax ? nan_max(a, b) : a + b; }
template <int KIND>
__device__ __forceinline__ double norm_wave(double v) {      // fixed butterfly order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = norm_fold<KIND>(v, __shfl_xor(v, o, 64));
  return v;
}
template <int KIND>
__device__ __forceinline__ float norm_finish(double s, double p) {
  if (KIND == kNormL2) return (float)sqrt(s);
  if (KIND == kNormP) return (float)pow(s, 1.0 / p);
  return (float)s;
}
// 256 threads -> one value in thread 0 (waves folded in order 0..3)
template <int KIND>
__device__ __forceinline__ double norm_block(double s, double* sh) {
  s = norm_wave<KIND>(s);
  __syncthreads();      // (sh may still be read from the previous chunk)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  return norm_fold<KIND>(norm_fold<KIND>(norm_fold<KIND>(sh[0], sh[1]), sh[2]), sh[3]);
}

template <int KIND>
__global__ __launch_bounds__(256) void seg_norm_partial_kernel(const float* __restrict__ g, const SegNormTable t, double p,
                                                               double* __restrict__ part, SegNormRecord* __restrict__ rec) {
  __shared__ double sh[4];
  const unsigned total = t.chunk_prefix[t.count];
  for (unsigned c = blockIdx.x; c < total; c += gridDim.x) {
    int lo = 0, hi = t.count - 1;            // last segment whose prefix <= c
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (t.chunk_prefix[mid] <= c) lo = mid; else hi = mid - 1;
    }
    const int64_t base = (int64_t)(c - t.chunk_prefix[lo]) * kSegNormChunk;
    const float* __restrict__ s = g + t.off[lo] + base;      // 16-byte aligned: the offset is, and so is a whole number of chunks
    const int64_t left = t.len[lo] - base;
    const int n = left < kSegNormChunk ? (int)left : kSegNormChunk;
    const int n4 = n >> 2;
    double acc = 0.0;
    if (n4 == kSegNormChunk / 4) {           // full chunk: all four loads in flight before the first add
      float4 a[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] = reinterpret_cast<const float4*>(s)[threadIdx.x + 256 * k];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        acc = norm_take<KIND>(acc, a[k].x, p); acc = norm_take<KIND>(acc, a[k].y, p);
        acc = norm_take<KIND>(acc, a[k].z, p); acc = norm_take<KIND>(acc, a[k].w, p);
      }
    } else {
      for (int i = threadIdx.x; i < n4; i += 256) {
        const float4 a = reinterpret_cast<const float4*>(s)[i];
        acc = norm_take<KIND>(acc, a.x, p); acc = norm_take<KIND>(acc, a.y, p);
        acc = norm_take<KIND>(acc, a.z, p); acc = norm_take<KIND>(acc, a.w, p);
      }
      for (int i = n4 * 4 + threadIdx.x; i < n; i += 256) acc = norm_take<KIND>(acc, s[i], p);
    }
    acc = norm_block<KIND>(acc, sh);
    if (threadIdx.x == 0) {
      part[t.chunk_base + c] = acc;
      if (c == t.chunk_prefix[lo]) {
        SegNormRecord r;
        r.first = t.chunk_base + c; r.chunks = t.chunk_prefix[lo + 1] - c; r.counts = t.counts[lo]; r.pad = 0;
        rec[t.seg_base + lo] = r;
      }
    }
  }
}
// one wavefront per segment
template <int KIND>
__global__ __launch_bounds__(256) void seg_norm_final_kernel(const double* __restrict__ part, const SegNormRecord* __restrict__ rec, int n_seg,
                                                             double p, float* __restrict__ out) {
  const int seg = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= n_seg) return;
  const SegNormRecord r = rec[seg];
  double s = 0.0;
  for (unsigned i = threadIdx.x & 63; i < r.chunks; i += 64) s = norm_fold<KIND>(s, part[r.first + i]);
  s = norm_wave<KIND>(s);
  if ((threadIdx.x & 63) == 0) out[seg] = norm_finish<KIND>(s, p);
}
// out[n_seg] = the same norm of the f32 values out[0 .. n_seg) of the segments that count (one block)
template <int KIND>
__global__ __launch_bounds__(256) void seg_norm_total_kernel(const SegNormRecord* __restrict__ rec, int n_seg, double p, float* __restrict__ out) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_seg; i += 256)
    if (rec[i].counts) s = norm_take<KIND>(s, out[i], p);
  s = norm_block<KIND>(s, sh);
  if (threadIdx.x == 0) out[n_seg] = norm_finish<KIND>(s, p);
}

// ---- gradient accumulation: arena[dst_off[i] + j] += src[i][j] over up to kGradAccSegs tensors per launch (Trainer(accumulate_grad_batches=N),
// optim.FusedAdam.gather_grads(accumulate=True)).  The segment table is a by-value kernel argument: no upload, no device allocation.  A segment is
// cut into chunks of kGradAccChunk floats; chunk_prefix[i] = chunks in front of segment i, so a block finds the segment of its chunk by a
// (block-uniform) binary search.  Every element is read and written by exactly one thread: plain f32 adds, no atomics, the same bits on any grid.
constexpr int kGradAccSegs = 128;
constexpr int kGradAccChunk = 4096;      // floats: four float4 per thread of a 256-thread block
struct GradAccTable {
  float* dst[kGradAccSegs];
  const float* src[kGradAccSegs];
  int64_t numel[kGradAccSegs];
  unsigned chunk_prefix[kGradAccSegs + 1];
  int count;
};
static_assert(sizeof(GradAccTable) <= 4000, "the segment table travels in the kernel arguments (4 KiB)");

__global__ __launch_bounds__(256) void grad_accumulate_kernel(const GradAccTable t) {
  const unsigned total = t.chunk_prefix[t.count];
  for (unsigned c = blockIdx.x; c < total; c += gridDim.x) {
    int lo = 0, hi = t.count - 1;            // last segment whose prefix <= c
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (t.chunk_prefix[mid] <= c) lo = mid; else hi = mid - 1;
    }
    const int64_t base = (int64_t)(c - t.chunk_prefix[lo]) * kGradAccChunk;
    float* __restrict__ d = t.dst[lo] + base;
    const float* __restrict__ s = t.src[lo] + base;
    const int64_t left = t.numel[lo] - base;
    const int n = left < kGradAccChunk ? (int)left : kGradAccChunk;
    if ((((uintptr_t)d | (uintptr_t)s) & 15) == 0) {
      const int n4 = n >> 2;
      if (n4 == kGradAccChunk / 4) {         // full chunk: all eight loads in flight before the first add
        float4 a[4], b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          a[k] = reinterpret_cast<const float4*>(d)[threadIdx.x + 256 * k];
          b[k] = reinterpret_cast<const float4*>(s)[threadIdx.x + 256 * k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
          reinterpret_cast<float4*>(d)[threadIdx.x + 256 * k] = make_float4(a[k].x + b[k].x, a[k].y + b[k].y, a[k].z + b[k].z, a[k].w + b[k].w);
      } else {
        for (int i = threadIdx.x; i < n4; i += 256) {
          const float4 a = reinterpret_cast<const float4*>(d)[i], b = reinterpret_cast<const float4*>(s)[i];
          reinterpret_cast<float4*>(d)[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
        }
        for (int i = n4 * 4 + threadIdx.x; i < n; i += 256) d[i] += s[i];
      }
    } else {
      for (int i = threadIdx.x; i < n; i += 256) d[i] += s[i];
    }
  }
}

// ---- exponential moving average of the weights ([UPSTREAM] ldm.modules.ema.LitEma; ema.py) -------------------------------------------------
// tick: the counter step and the decay schedule on the device, one thread; state = [1 - d, d].  num_updates < 0: the schedule is off.
__global__ void ema_tick_kernel(const float* __restrict__ decay, int* __restrict__ num_updates, float* __restrict__ state) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const float dec = decay[0];
  int n = num_updates[0];
  float d = dec;
  if (n >= 0) {
    n += 1;
    num_updates[0] = n;
    const float q = __fdiv_rn((float)(1 + n), (float)(10 + n));      // torch: int32 / int32 -> both converted to f32, one rounded division
    d = q < dec ? q : dec;
  }
  state[0] = __fsub_rn(1.f, d);
  state[1] = d;
}

// How a pair of f32 arrays is walked with 16-byte accesses: `head` leading floats one by one until both pointers are 16-byte aligned (all n
// when the two are misaligned differently), n4 float4, then the rest one by one.  Every element belongs to exactly one thread.
struct PairSpan { int64_t head, n4, tail0, nscalar; };
static PairSpan pair_span(const void* a, const void* b, int64_t n) {
  PairSpan s;
  const uintptr_t ma = (uintptr_t)a & 15, mb = (uintptr_t)b & 15;
  s.head = ma == mb ? std::min<int64_t>(n, (int64_t)(((16 - ma) & 15) / 4)) : n;
  s.n4 = (n - s.head) / 4;
  s.tail0 = s.head + 4 * s.n4;
  s.nscalar = s.head + (n - s.tail0);
  return s;
}
__device__ __forceinline__ int64_t pair_scalar_index(const PairSpan& sp, int64_t j) { return j < sp.head ? j : sp.tail0 + (j - sp.head); }

// s <- s - omd * (s - p): three separately rounded f32 operations, as torch's sub / mul / sub_.  hipcc contracts by default, and HIP's
// __fmul_rn / __fsub_rn are header functions built under that default (written with them, the last two came out as one v_fma_f32, with
// or without the pragma): plain operators under contract(off) are what keeps them apart.
__device__ __forceinline__ float ema_one(float s, float p, float omd) {
#pragma clang fp contract(off)
  const float t = s - p;
  const float u = omd * t;
  return s - u;
}

__global__ __launch_bounds__(256) void ema_update_kernel(const float* __restrict__ p, float* __restrict__ s, const PairSpan sp,
                                                         const float* __restrict__ state) {
  const float omd = state[0];
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  const float4* p4 = reinterpret_cast<const float4*>(p + sp.head);
  float4* s4 = reinterpret_cast<float4*>(s + sp.head);
  for (int64_t i = t0; i < sp.n4; i += stride) {
    const float4 pv = p4[i], sv = s4[i];
    s4[i] = make_float4(ema_one(sv.x, pv.x, omd), ema_one(sv.y, pv.y, omd), ema_one(sv.z, pv.z, omd), ema_one(sv.w, pv.w, omd));
  }
  for (int64_t j = t0; j < sp.nscalar; j += stride) {
    const int64_t i = pair_scalar_index(sp, j);
    s[i] = ema_one(s[i], p[i], omd);
  }
}

// a <-> b in one pass (ema_scope: the parameters take the averaged values, the shadows keep the trained ones, and back)
__global__ __launch_bounds__(256) void ema_swap_kernel(float* __restrict__ a, float* __restrict__ b, const PairSpan sp) {
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  float4* a4 = reinterpret_cast<float4*>(a + sp.head);
  float4* b4 = reinterpret_cast<float4*>(b + sp.head);
  for (int64_t i = t0; i < sp.n4; i += stride) {
    const float4 av = a4[i], bv = b4[i];
    a4[i] = bv;
    b4[i] = av;
  }
  for (int64_t j = t0; j < sp.nscalar; j += stride) {
    const int64_t i = pair_scalar_index(sp, j);
    const float av = a[i], bv = b[i];
    a[i] = bv;
    b[i] = av;
  }
}

// ---- layout: NHWC -> NCHW copy (reconstructions handed back to NCHW callers) ---------------------------
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int C, int HW) {
  const int64_t total = (int64_t)N * C * HW;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int hw = (int)(idx % HW);
    const int64_t r = idx / HW;
    const int c = (int)(r % C); const int n = (int)(r / C);
    y[idx] = x[((int64_t)n * HW + hw) * C + c];
  }
}

// ---- y = x * m[n][hw] (mask_2d_bbox products, contperceptual.py:252-255); its own backward with x = dy ----
__global__ __launch_bounds__(256) void mul_mask_kernel(const float* __restrict__ x, const float* __restrict__ m,
                                                       float* __restrict__ y, int64_t npix, int C) {
  const int64_t total = npix * C;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x)
    y[idx] = x[idx] * m[idx / C];
}

// ---- latent mixing: out = z * mask + add (dropout on z_obj, + N(0,1) noise, + enc_pose; autoencoder.py:233-253)
__global__ __launch_bounds__(256) void latent_combine_kernel(const float* __restrict__ z, const float* __restrict__ mask,
                                                             const float* __restrict__ add, float* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float v = z[i];
    if (mask) v *= mask[i];
    if (add) v += add[i];
    out[i] = v;
  }
}

}  // namespace

extern "C" {

int odvae_mul_mask_f32(const float* x, const float* mask, float* y, int64_t npix, int C, void* stream) {
  ODVAE_CHECK_ARG(x && mask && y && npix > 0 && C > 0, "mul_mask: bad arguments");
  hipLaunchKernelGGL(mul_mask_kernel, dim3(grid_1d(npix * C)), dim3(256), 0, static_cast<hipStream_t>(stream), x, mask, y, npix, C);
  ODVAE_LAUNCH_CHECK("mul_mask");
  return ODVAE_OK;
}

int odvae_latent_combine_f32(const float* z, const float* mask, const float* add, float* out, int64_t n, void* stream) {
  ODVAE_CHECK_ARG(z && out && n > 0, "latent_combine: bad arguments");
  hipLaunchKernelGGL(latent_combine_kernel, dim3(grid_1d(n)), dim3(256), 0, static_cast<hipStream_t>(stream), z, mask, add, out, n);
  ODVAE_LAUNCH_CHECK("latent_combine");
  return ODVAE_OK;
}

static int softmax_rows_impl(const float* x, float* y, int64_t rows, int cols, float scale, const int* pred, float* ones, void* stream) {
  ODVAE_CHECK_ARG(x && y && rows > 0 && cols > 0 && cols % 4 == 0, "softmax_rows: need cols %% 4 == 0 (rows=%lld cols=%d)", (long long)rows, cols);
  ODVAE_CHECK_ARG(scale > 0.f, "softmax_rows: scale must be positive");
  // (under a predicate: a small grid that walks the rows, so that finding out there is nothing to do is a 2 048-block launch)
  const dim3 grid((unsigned)std::min<int64_t>(rows, pred ? 2048 : 65536 * 4)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (cols <= 1024)       hipLaunchKernelGGL((softmax_rows_reg_kernel<1>), grid, block, 0, st, x, y, rows, cols, scale, pred, ones);
  else if (cols <= 2048)  hipLaunchKernelGGL((softmax_rows_reg_kernel<2>), grid, block, 0, st, x, y, rows, cols, scale, pred, ones);
  else if (cols <= 4096)  hipLaunchKernelGGL((softmax_rows_reg_kernel<4>), grid, block, 0, st, x, y, rows, cols, scale, pred, ones);
  else if (cols <= 16384) hipLaunchKernelGGL((softmax_rows_reg_kernel<16>), grid, block, 0, st, x, y, rows, cols, scale, pred, ones);
  else                    hipLaunchKernelGGL(softmax_rows_kernel, grid, block, 0, st, x, y, rows, cols, scale, pred, ones);
  ODVAE_LAUNCH_CHECK("softmax_rows");
  return ODVAE_OK;
}

int odvae_softmax_rows_f32(const float* x, float* y, int64_t rows, int cols, float scale, void* stream) {
  return softmax_rows_impl(x, y, rows, cols, scale, nullptr, nullptr, stream);
}

// The same under a device-side predicate (nothing happens unless *pred != 0), also writing ones[row] = 1: the fallback of the folded
// attention softmax (odvae_gemm_exp_bound_f32 / odvae_gemm_rownorm_f32) where a row's bound was too loose.
int odvae_softmax_rows_pred_f32(const float* x, float* y, int64_t rows, int cols, float scale, const int* pred, float* ones, void* stream) {
  ODVAE_CHECK_ARG(pred && ones, "softmax_rows_pred: null predicate / row-factor array");
  return softmax_rows_impl(x, y, rows, cols, scale, pred, ones, stream);
}

// Device-side counter of the folded-softmax fallbacks; add > 0 is a TEST HOOK that bumps it (synchronises the device).  -1 on a HIP error.
int odvae_attn_softmax_fallbacks(int add) {
  unsigned v = 0;
  if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_attn_fallbacks), sizeof(v)) != hipSuccess) return -1;
  if (add > 0) {
    v += (unsigned)add;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_attn_fallbacks), &v, sizeof(v)) != hipSuccess) return -1;
  }
  return (int)v;
}

// ---- folded attention softmax: the per-row bound of the scores, and the backward's row dot product with dO / l beside it ----
// qkv [rows][3C] (q | k | v per token).  nq[row] = |q_row|, nk[row] = |k_row|: one wavefront per token.
__global__ __launch_bounds__(256) void attn_rownorm_kernel(const float* __restrict__ qkv, int64_t rows, int C,
                                                           float* __restrict__ nq, float* __restrict__ nk) {
  const int lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
    const float4* pq = reinterpret_cast<const float4*>(qkv + row * 3 * C);
    const float4* pk = reinterpret_cast<const float4*>(qkv + row * 3 * C + C);
    float a = 0.f, b = 0.f;
    for (int i = lane; i < C / 4; i += 64) {
      const float4 x = pq[i], y = pk[i];
      a += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
      b += y.x * y.x + y.y * y.y + y.z * y.z + y.w * y.w;
    }
    a = wave_sum(a); b = wave_sum(b);
    if (lane == 0) { nq[row] = sqrtf(a); nk[row] = sqrtf(b); }
  }
}
// one block per image: bound[i] = |q_i| * max_j |k_j| (>= q_i . k_j for every j, Cauchy-Schwarz; a hair above for the rounding of the
// norms), in place over nq; block 0 clears the fallback flag
__global__ __launch_bounds__(256) void attn_bound_kernel(float* __restrict__ nq, const float* __restrict__ nk, int T, int* flag) {
  __shared__ float sh[4];
  const int n = blockIdx.x;
  float m = 0.f;
  for (int i = threadIdx.x; i < T; i += 256) m = fmaxf(m, nk[(int64_t)n * T + i]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3])) * 1.000001f;
  for (int i = threadIdx.x; i < T; i += 256) nq[(int64_t)n * T + i] *= m;
  if (n == 0 && threadIdx.x == 0 && flag) *flag = 0;
}

// out[row] = a[row] . b[row] and as[row][:] = a[row][:] * rs[row]  (attention backward with P = E / l: D_i = dO_i . O_i, dO_i / l_i)
__global__ __launch_bounds__(256) void rowdot_scale_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ rs,
                                                           int64_t rows, int cols, float* __restrict__ out, float* __restrict__ as) {
  const int lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
    const float4* pa = reinterpret_cast<const float4*>(a + row * cols);
    const float4* pb = reinterpret_cast<const float4*>(b + row * cols);
    float4* po = reinterpret_cast<float4*>(as + row * cols);
    const float r = rs[row];
    float s = 0.f;
    for (int q = lane; q < cols / 4; q += 64) {
      const float4 x = pa[q], y = pb[q];
      s += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
      po[q] = make_float4(x.x * r, x.y * r, x.z * r, x.w * r);
    }
    s = wave_sum(s);
    if (lane == 0) out[row] = s;
  }
}

// bound[N * T] for odvae_gemm_exp_bound_f32 from qkv [N][T][3C]; nk_scratch [N * T]; *flag (nullable) is cleared
int odvae_attn_row_bound_f32(const float* qkv, int N, int T, int C, float* bound, float* nk_scratch, int* flag, void* stream) {
  ODVAE_CHECK_ARG(qkv && bound && nk_scratch && N > 0 && T > 0 && C > 0 && C % 4 == 0, "attn_row_bound: bad arguments (C %% 4 == 0 needed)");
  ODVAE_CHECK_ARG(((uintptr_t)qkv & 15) == 0, "attn_row_bound: qkv must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t rows = (int64_t)N * T;
  hipLaunchKernelGGL(attn_rownorm_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(rows, 4), 65536)), dim3(256), 0, st, qkv, rows, C, bound, nk_scratch);
  ODVAE_LAUNCH_CHECK("attn_rownorm");
  hipLaunchKernelGGL(attn_bound_kernel, dim3(N), dim3(256), 0, st, bound, nk_scratch, T, flag);
  ODVAE_LAUNCH_CHECK("attn_bound");
  return ODVAE_OK;
}

int odvae_rowdot_scale_f32(const float* a, const float* b, const float* row_scale, int64_t rows, int cols, float* out, float* a_scaled, void* stream) {
  ODVAE_CHECK_ARG(a && b && row_scale && out && a_scaled && rows > 0 && cols > 0 && cols % 4 == 0, "rowdot_scale: need cols %% 4 == 0");
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div64(rows, 4), 65536)), block(256);
  hipLaunchKernelGGL(rowdot_scale_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a, b, row_scale, rows, cols, out, a_scaled);
  ODVAE_LAUNCH_CHECK("rowdot_scale");
  return ODVAE_OK;
}

// out[row] = sum_c a[row][c] * b[row][c]: one wavefront per row, float4 lanes (attention backward: dO[i] . O[i])
__global__ __launch_bounds__(256) void rowdot_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                     int64_t rows, int cols, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
    const float4* pa = reinterpret_cast<const float4*>(a + row * cols);
    const float4* pb = reinterpret_cast<const float4*>(b + row * cols);
    float s = 0.f;
    for (int q = lane; q < cols / 4; q += 64) {
      const float4 x = pa[q], y = pb[q];
      s += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
    }
    s = wave_sum(s);
    if (lane == 0) out[row] = s;
  }
}

int odvae_rowdot_f32(const float* a, const float* b, int64_t rows, int cols, float* out, void* stream) {
  ODVAE_CHECK_ARG(a && b && out && rows > 0 && cols > 0 && cols % 4 == 0, "rowdot: need cols %% 4 == 0");
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div64(rows, 4), 65536)), block(256);
  hipLaunchKernelGGL(rowdot_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a, b, rows, cols, out);
  ODVAE_LAUNCH_CHECK("rowdot");
  return ODVAE_OK;
}

int odvae_softmax_rows_bwd_f32(const float* p, const float* dp, float* ds, int64_t rows, int cols, float scale, void* stream) {
  ODVAE_CHECK_ARG(p && dp && ds && rows > 0 && cols > 0 && cols % 4 == 0, "softmax_rows_bwd: need cols %% 4 == 0");
  const dim3 grid((unsigned)std::min<int64_t>(rows, 65536 * 4)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (cols <= 1024)       hipLaunchKernelGGL((softmax_rows_bwd_reg_kernel<1>), grid, block, 0, st, p, dp, ds, rows, cols, scale);
  else if (cols <= 2048)  hipLaunchKernelGGL((softmax_rows_bwd_reg_kernel<2>), grid, block, 0, st, p, dp, ds, rows, cols, scale);
  else if (cols <= 4096)  hipLaunchKernelGGL((softmax_rows_bwd_reg_kernel<4>), grid, block, 0, st, p, dp, ds, rows, cols, scale);
  else if (cols <= 8192)  hipLaunchKernelGGL((softmax_rows_bwd_reg_kernel<8>), grid, block, 0, st, p, dp, ds, rows, cols, scale);
  else                    hipLaunchKernelGGL(softmax_rows_bwd_kernel, grid, block, 0, st, p, dp, ds, rows, cols, scale);
  ODVAE_LAUNCH_CHECK("softmax_rows_bwd");
  return ODVAE_OK;
}

int odvae_upsample2x_bwd_f32(const float* du, float* dx, int N, int H, int W, int C, void* stream) {
  ODVAE_CHECK_ARG(du && dx && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "upsample2x_bwd: need C %% 4 == 0");
  hipLaunchKernelGGL(upsample2x_bwd_kernel, dim3(grid_1d((int64_t)N * H * W * (C / 4))), dim3(256), 0, static_cast<hipStream_t>(stream), du, dx, N, H, W, C);
  ODVAE_LAUNCH_CHECK("upsample2x_bwd");
  return ODVAE_OK;
}

// Downsample(with_conv=False): y [N][H/2][W/2][C] = F.avg_pool2d(x [N][H][W][C], 2, 2) (an odd last row / column is dropped).
// gn_partial (nullable): [N][chunks][gn_groups][2] = (sum, sum of squares) of y, every slot written -- what odvae_groupnorm_fwd_partials_f32 takes
int odvae_avgpool2x2_f32(const float* x, float* y, int N, int H, int W, int C, float* gn_partial, int gn_groups, int chunks, void* stream) {
  return rs_avgpool<RsF32>(x, y, N, H, W, C, gn_partial, gn_groups, chunks, stream);
}

// dx [N][H][W][C] (overwritten, zeros in a dropped row / column) from dy [N][H/2][W/2][C]
int odvae_avgpool2x2_bwd_f32(const float* dy, float* dx, int N, int H, int W, int C, void* stream) {
  return rs_avgpool_bwd<RsF32>(dy, dx, N, H, W, C, stream);
}

// Upsample(with_conv=False): u [N][2H][2W][C] = F.interpolate(x [N][H][W][C], scale_factor=2, mode="nearest"); gn_partial as above, the
// statistics of u (4 x those of x).  Backward: odvae_upsample2x_bwd_f32
int odvae_upsample2x_f32(const float* x, float* u, int N, int H, int W, int C, float* gn_partial, int gn_groups, int chunks, void* stream) {
  return rs_upsample<RsF32>(x, u, N, H, W, C, gn_partial, gn_groups, chunks, stream);
}

int odvae_tanh_f32(const float* x, float* y, int64_t n, void* stream) {
  ODVAE_CHECK_ARG(x && y && n > 0, "tanh: bad arguments");
  const int vec = (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
  hipLaunchKernelGGL(tanh_kernel, dim3(grid_1d(n / 4 + 1)), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, n, vec);
  ODVAE_LAUNCH_CHECK("tanh");
  return ODVAE_OK;
}

int odvae_tanh_bwd_f32(const float* y, const float* dy, float* dx, int64_t n, void* stream) {
  ODVAE_CHECK_ARG(y && dy && dx && n > 0, "tanh_bwd: bad arguments");
  const int vec = (((uintptr_t)y | (uintptr_t)dy | (uintptr_t)dx) & 15) == 0;
  hipLaunchKernelGGL(tanh_bwd_kernel, dim3(grid_1d(n / 4 + 1)), dim3(256), 0, static_cast<hipStream_t>(stream), y, dy, dx, n, vec);
  ODVAE_LAUNCH_CHECK("tanh_bwd");
  return ODVAE_OK;
}

// workspace: >= 2*1024+2 floats.  minmax_out[2] receives (min, max).
int odvae_rescale_minmax_f32(const float* x_nchw, float* y_nhwc, int N, int C, int HW, float* minmax_out,
                             void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x_nchw && y_nhwc && minmax_out && N > 0 && C > 0 && HW > 0, "rescale_minmax: bad arguments");
  const int nblk = 1024;
  if (!workspace || workspace_bytes < (size_t)2 * nblk * sizeof(float)) {
    odvae_set_error("rescale_minmax: needs %zu workspace bytes", (size_t)2 * nblk * sizeof(float));
    return ODVAE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  const int64_t n = (int64_t)N * C * HW;
  hipLaunchKernelGGL(minmax_partial_kernel, dim3(nblk), dim3(256), 0, st, x_nchw, n, part);
  hipLaunchKernelGGL(minmax_final_kernel, dim3(1), dim3(64), 0, st, part, nblk, minmax_out);
  hipLaunchKernelGGL(rescale_nchw_to_nhwc_kernel, dim3(grid_1d(n)), dim3(256), 0, st, x_nchw, minmax_out, y_nhwc, N, C, HW);
  ODVAE_LAUNCH_CHECK("rescale_minmax");
  return ODVAE_OK;
}

int odvae_gaussian_sample_f32(const float* moments, const float* eps, float* z, int N, int HW, int Cz, void* stream) {
  ODVAE_CHECK_ARG(moments && eps && z && N > 0 && HW > 0 && Cz > 0, "gaussian_sample: bad arguments");
  const int64_t npix = (int64_t)N * HW;
  hipLaunchKernelGGL(gaussian_sample_kernel, dim3(grid_1d(npix * Cz)), dim3(256), 0, static_cast<hipStream_t>(stream), moments, eps, z, npix, Cz);
  ODVAE_LAUNCH_CHECK("gaussian_sample");
  return ODVAE_OK;
}

int odvae_gaussian_kl_f32(const float* moments, float* kl, int N, int HW, int Cz, void* stream) {
  ODVAE_CHECK_ARG(moments && kl && N > 0 && HW > 0 && Cz > 0, "gaussian_kl: bad arguments");
  hipLaunchKernelGGL(gaussian_kl_kernel, dim3(N), dim3(256), 0, static_cast<hipStream_t>(stream), moments, kl, HW, Cz);
  ODVAE_LAUNCH_CHECK("gaussian_kl");
  return ODVAE_OK;
}

// dmoments (overwritten) from dz/eps (both null or both set) and dkl (may be null)
int odvae_gaussian_bwd_f32(const float* moments, const float* eps, const float* dz, const float* dkl,
                           float* dmoments, int N, int HW, int Cz, void* stream) {
  ODVAE_CHECK_ARG(moments && dmoments && N > 0 && HW > 0 && Cz > 0, "gaussian_bwd: bad arguments");
  ODVAE_CHECK_ARG((dz == nullptr) == (eps == nullptr), "gaussian_bwd: dz and eps must both be set or both null");
  hipLaunchKernelGGL(gaussian_bwd_kernel, dim3(grid_1d((int64_t)N * HW * Cz)), dim3(256), 0, static_cast<hipStream_t>(stream), moments, eps, dz, dkl, dmoments, N, HW, Cz);
  ODVAE_LAUNCH_CHECK("gaussian_bwd");
  return ODVAE_OK;
}

// out[n] = sum |x*m - xr*m| over (hw, c).  workspace: N*256 floats
int odvae_l1_masked_sum_f32(const float* x, const float* xr, const float* mask, float* out, int N, int HW, int C,
                            void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && xr && out && N > 0 && HW > 0 && C > 0, "l1_masked_sum: bad arguments");
  const int nblk = 256;
  if (!workspace || workspace_bytes < (size_t)N * nblk * sizeof(float)) {
    odvae_set_error("l1_masked_sum: needs %zu workspace bytes", (size_t)N * nblk * sizeof(float));
    return ODVAE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(l1_partial_kernel, dim3(nblk, N), dim3(256), 0, st, x, xr, mask, part, HW, C);
  hipLaunchKernelGGL(rowsum_final_kernel, dim3(N), dim3(64), 0, st, part, nblk, out);
  ODVAE_LAUNCH_CHECK("l1_masked_sum");
  return ODVAE_OK;
}

int odvae_l1_masked_bwd_f32(const float* x, const float* xr, const float* mask, const float* g, float* dxr,
                            int N, int HW, int C, void* stream) {
  ODVAE_CHECK_ARG(x && xr && g && dxr && N > 0 && HW > 0 && C > 0, "l1_masked_bwd: bad arguments");
  hipLaunchKernelGGL(l1_bwd_kernel, dim3(grid_1d((int64_t)N * HW * C)), dim3(256), 0, static_cast<hipStream_t>(stream), x, xr, mask, g, dxr, N, HW, C);
  ODVAE_LAUNCH_CHECK("l1_masked_bwd");
  return ODVAE_OK;
}

// the sample's pixels are cut over at most this many blocks (the kernel's grid cap); the workspace holds 2 * N * that many floats
static const int kRgbaBlocks = 256;

size_t odvae_rgba_terms_workspace_bytes(int N) { return (size_t)2 * (size_t)std::max(N, 0) * kRgbaBlocks * sizeof(float); }

int odvae_rgba_terms_f32(const float* rec, const float* rgb_gt, const float* mask_gt, const float* box, int l2, float* l1_sum, float* mask_sum,
                         float* rec_rgb_m, float* gt_rgb_m, float* rec_rgba_m, float* gt_rgba_m, int N, int HW,
                         void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(rec && rgb_gt && mask_gt && N > 0 && N <= 65535 && HW > 0, "rgba_terms: bad arguments");
  ODVAE_CHECK_ARG((l1_sum == nullptr) == (mask_sum == nullptr), "rgba_terms: l1_sum and mask_sum must both be set or both null");
  const bool sums = l1_sum != nullptr;
  ODVAE_CHECK_ARG(sums || rec_rgb_m || gt_rgb_m || rec_rgba_m || gt_rgba_m, "rgba_terms: nothing to compute");
  ODVAE_CHECK_ARG((((uintptr_t)rec | (uintptr_t)rec_rgba_m | (uintptr_t)gt_rgba_m) & 15) == 0,
                  "rgba_terms: rec, rec_rgba_m and gt_rgba_m must be 16-byte aligned");
  ODVAE_CHECK_ARG((((uintptr_t)rgb_gt | (uintptr_t)mask_gt | (uintptr_t)box | (uintptr_t)rec_rgb_m | (uintptr_t)gt_rgb_m) & 3) == 0,
                  "rgba_terms: a float array is not 4-byte aligned");
  if (sums && (!workspace || workspace_bytes < odvae_rgba_terms_workspace_bytes(N))) {
    odvae_set_error("rgba_terms: needs %zu workspace bytes", odvae_rgba_terms_workspace_bytes(N));
    return ODVAE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = sums ? static_cast<float*>(workspace) : nullptr;
  const int nblk = (int)std::min<int64_t>(ceil_div64(HW, 256), kRgbaBlocks);
  hipLaunchKernelGGL(rgba_terms_kernel, dim3(nblk, N), dim3(256), 0, st, reinterpret_cast<const float4*>(rec), rgb_gt, mask_gt, box, part,
                     rec_rgb_m, gt_rgb_m, reinterpret_cast<float4*>(rec_rgba_m), reinterpret_cast<float4*>(gt_rgba_m), HW, l2 ? 1 : 0);
  ODVAE_LAUNCH_CHECK("rgba_terms");
  if (!sums) return ODVAE_OK;
  hipLaunchKernelGGL(rgba_final_kernel, dim3(N, 2), dim3(64), 0, st, part, nblk, l1_sum, mask_sum);
  ODVAE_LAUNCH_CHECK("rgba_terms(final)");
  return ODVAE_OK;
}

int odvae_rgba_terms_bwd_f32(const float* rec, const float* rgb_gt, const float* mask_gt, const float* box, int l2, const float* g_l1,
                             const float* g_mask, const float* g_rec_rgb_m, const float* g_rec_rgba_m, float* d_rec, int N, int HW, void* stream) {
  ODVAE_CHECK_ARG(rec && rgb_gt && mask_gt && d_rec && N > 0 && N <= 65535 && HW > 0, "rgba_terms_bwd: bad arguments");
  ODVAE_CHECK_ARG((((uintptr_t)rec | (uintptr_t)g_rec_rgba_m | (uintptr_t)d_rec) & 15) == 0,
                  "rgba_terms_bwd: rec, g_rec_rgba_m and d_rec must be 16-byte aligned");
  ODVAE_CHECK_ARG((((uintptr_t)rgb_gt | (uintptr_t)mask_gt | (uintptr_t)box | (uintptr_t)g_l1 | (uintptr_t)g_mask | (uintptr_t)g_rec_rgb_m) & 3) == 0,
                  "rgba_terms_bwd: a float array is not 4-byte aligned");
  hipLaunchKernelGGL(rgba_terms_bwd_kernel, dim3(grid_1d(HW, std::max(1, 8192 / N)), N), dim3(256), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const float4*>(rec), rgb_gt, mask_gt, box, g_l1, g_mask, g_rec_rgb_m,
                     reinterpret_cast<const float4*>(g_rec_rgba_m), reinterpret_cast<float4*>(d_rec), HW, l2 ? 1 : 0);
  ODVAE_LAUNCH_CHECK("rgba_terms_bwd");
  return ODVAE_OK;
}

// the stage-1 grid cap of the weighted sums; the workspace holds 3 * N * that many floats
static const int kL1wBlocks = 256;

size_t odvae_l1_weighted_workspace_bytes(int N) { return (size_t)3 * (size_t)std::max(N, 0) * kL1wBlocks * sizeof(float); }

// which instantiation of the weighted-L1 kernels a call takes: the 16-byte forms need Cr == 4 and 16-byte aligned 4-channel arrays
#define ODVAE_L1W_DISPATCH(KERNEL, v4, ...)                                                                   \
  do {                                                                                                        \
    if ((v4) && C == 3) hipLaunchKernelGGL((KERNEL<3, true>), __VA_ARGS__);                                   \
    else if ((v4) && C == 4) hipLaunchKernelGGL((KERNEL<4, true>), __VA_ARGS__);                              \
    else if (C == 3) hipLaunchKernelGGL((KERNEL<3, false>), __VA_ARGS__);                                     \
    else hipLaunchKernelGGL((KERNEL<0, false>), __VA_ARGS__);                                                 \
  } while (0)

int odvae_l1_weighted_sums_f32(const float* x, const float* xr, const float* box, const float* wgt, int wgt_per_channel, float* l1_sum,
                               float* wl1_sum, float* w_sum, int N, int HW, int C, int Cr, void* workspace, size_t workspace_bytes,
                               void* stream) {
  ODVAE_CHECK_ARG(N > 0 && HW > 0 && C > 0 && Cr >= C, "l1_weighted_sums: needs N > 0, HW > 0, 0 < C <= Cr (got N %d, HW %d, C %d, Cr %d)", N, HW, C, Cr);
  ODVAE_CHECK_ARG(N <= 65535, "l1_weighted_sums: N %d is beyond the grid's 65535 samples", N);
  ODVAE_CHECK_ARG(wgt != nullptr, "l1_weighted_sums: wgt is null");
  ODVAE_CHECK_ARG(l1_sum || wl1_sum || w_sum, "l1_weighted_sums: nothing to compute (every output is null)");
  ODVAE_CHECK_ARG((x == nullptr) == (xr == nullptr), "l1_weighted_sums: x and xr must both be set or both null");
  ODVAE_CHECK_ARG(x || (!l1_sum && !wl1_sum), "l1_weighted_sums: without x and xr only w_sum can be asked for");
  ODVAE_CHECK_ARG((((uintptr_t)x | (uintptr_t)xr | (uintptr_t)box | (uintptr_t)wgt) & 3) == 0, "l1_weighted_sums: a float array is not 4-byte aligned");
  if (!workspace || workspace_bytes < odvae_l1_weighted_workspace_bytes(N)) {
    odvae_set_error("l1_weighted_sums: needs %zu workspace bytes", odvae_l1_weighted_workspace_bytes(N));
    return ODVAE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  const int nblk = (int)std::min<int64_t>(ceil_div64(HW, 256), kL1wBlocks);
  const bool v4 = x && Cr == 4 && ((uintptr_t)xr & 15) == 0;
  ODVAE_L1W_DISPATCH(l1_weighted_kernel, v4, dim3(nblk, N), dim3(256), 0, st, x, xr, box, wgt, part, HW, C, Cr, wgt_per_channel ? 1 : 0);
  ODVAE_LAUNCH_CHECK("l1_weighted_sums");
  hipLaunchKernelGGL(sums3_final_kernel, dim3(N, 3), dim3(64), 0, st, part, nblk, l1_sum, wl1_sum, w_sum);
  ODVAE_LAUNCH_CHECK("l1_weighted_sums(final)");
  return ODVAE_OK;
}

int odvae_l1_weighted_bwd_f32(const float* x, const float* xr, const float* box, const float* wgt, int wgt_per_channel, const float* g_l1,
                              const float* g_wl1, float* dxr, int N, int HW, int C, int Cr, void* stream) {
  ODVAE_CHECK_ARG(N > 0 && HW > 0 && C > 0 && Cr >= C, "l1_weighted_bwd: needs N > 0, HW > 0, 0 < C <= Cr (got N %d, HW %d, C %d, Cr %d)", N, HW, C, Cr);
  ODVAE_CHECK_ARG(N <= 65535, "l1_weighted_bwd: N %d is beyond the grid's 65535 samples", N);
  ODVAE_CHECK_ARG(x && xr && wgt && dxr, "l1_weighted_bwd: x, xr, wgt and dxr are required");
  ODVAE_CHECK_ARG((((uintptr_t)x | (uintptr_t)xr | (uintptr_t)box | (uintptr_t)wgt | (uintptr_t)g_l1 | (uintptr_t)g_wl1 | (uintptr_t)dxr) & 3) == 0,
                  "l1_weighted_bwd: a float array is not 4-byte aligned");
  const bool v4 = Cr == 4 && (((uintptr_t)xr | (uintptr_t)dxr) & 15) == 0;
  ODVAE_L1W_DISPATCH(l1_weighted_bwd_kernel, v4, dim3(grid_1d(HW, std::max(1, 8192 / N)), N), dim3(256), 0, static_cast<hipStream_t>(stream),
                     x, xr, box, wgt, g_l1, g_wl1, dxr, HW, C, Cr, wgt_per_channel ? 1 : 0);
  ODVAE_LAUNCH_CHECK("l1_weighted_bwd");
  return ODVAE_OK;
}
#undef ODVAE_L1W_DISPATCH

static int cat_mask_check(const char* what, int N, int HW, int Cx, int Cc) {
  ODVAE_CHECK_ARG(N > 0 && HW > 0 && Cx > 0 && Cc > 0, "%s: needs N, HW, Cx, Cc > 0 (got %d, %d, %d, %d)", what, N, HW, Cx, Cc);
  ODVAE_CHECK_ARG(N <= 65535, "%s: N %d is beyond the grid's 65535 samples", what, N);
  ODVAE_CHECK_ARG((int64_t)HW * ((int64_t)Cx + Cc) < ((int64_t)1 << 31), "%s: a sample of %d x %lld floats is beyond the 32-bit element index",
                  what, HW, (long long)Cx + Cc);
  return ODVAE_OK;
}

int odvae_cat_mask_f32(const float* x, const float* box, const float* cond, float* y, int N, int HW, int Cx, int Cc, void* stream) {
  if (int rc = cat_mask_check("cat_mask", N, HW, Cx, Cc)) return rc;
  ODVAE_CHECK_ARG(x && cond && y, "cat_mask: x, cond and y are required");
  ODVAE_CHECK_ARG((((uintptr_t)x | (uintptr_t)box | (uintptr_t)cond | (uintptr_t)y) & 3) == 0, "cat_mask: a float array is not 4-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int Cy = Cx + Cc, cap = std::max(1, 8192 / N);
  if (Cy == 4 && ((uintptr_t)y & 15) == 0) {
    hipLaunchKernelGGL(cat_mask_px4_kernel, dim3(grid_1d(HW, cap), N), dim3(256), 0, st, x, box, cond, reinterpret_cast<float4*>(y), HW, Cx);
  } else {
    const dim3 grid(grid_1d((int64_t)HW * Cy, cap), N);
    switch (Cy) {
      case 4: hipLaunchKernelGGL(cat_mask_kernel<4>, grid, dim3(256), 0, st, x, box, cond, y, HW, Cx, Cy); break;
      case 5: hipLaunchKernelGGL(cat_mask_kernel<5>, grid, dim3(256), 0, st, x, box, cond, y, HW, Cx, Cy); break;
      case 6: hipLaunchKernelGGL(cat_mask_kernel<6>, grid, dim3(256), 0, st, x, box, cond, y, HW, Cx, Cy); break;
      default: hipLaunchKernelGGL(cat_mask_kernel<0>, grid, dim3(256), 0, st, x, box, cond, y, HW, Cx, Cy);
    }
  }
  ODVAE_LAUNCH_CHECK("cat_mask");
  return ODVAE_OK;
}

int odvae_cat_mask_bwd_f32(const float* dy, const float* box, float* dx, int N, int HW, int Cx, int Cc, void* stream) {
  if (int rc = cat_mask_check("cat_mask_bwd", N, HW, Cx, Cc)) return rc;
  ODVAE_CHECK_ARG(dy && dx, "cat_mask_bwd: dy and dx are required");
  ODVAE_CHECK_ARG((((uintptr_t)dy | (uintptr_t)box | (uintptr_t)dx) & 3) == 0, "cat_mask_bwd: a float array is not 4-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(grid_1d((int64_t)HW * Cx, std::max(1, 8192 / N)), N);
  switch (Cx) {
    case 3: hipLaunchKernelGGL(cat_mask_bwd_kernel<3>, grid, dim3(256), 0, st, dy, box, dx, HW, Cx, Cx + Cc); break;
    case 4: hipLaunchKernelGGL(cat_mask_bwd_kernel<4>, grid, dim3(256), 0, st, dy, box, dx, HW, Cx, Cx + Cc); break;
    default: hipLaunchKernelGGL(cat_mask_bwd_kernel<0>, grid, dim3(256), 0, st, dy, box, dx, HW, Cx, Cx + Cc);
  }
  ODVAE_LAUNCH_CHECK("cat_mask_bwd");
  return ODVAE_OK;
}

size_t odvae_colsum_workspace_bytes(int64_t rows, int C) {
  const int nblk = (int)std::min<int64_t>(std::max<int64_t>(rows / 64, 1), 1024);
  return (size_t)nblk * C * sizeof(float);
}

int odvae_colsum_f32(const float* x, int64_t rows, int C, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && out && rows > 0 && C > 0, "colsum: bad arguments");
  const int nblk = (int)std::min<int64_t>(std::max<int64_t>(rows / 64, 1), 1024);
  if (!workspace || workspace_bytes < (size_t)nblk * C * sizeof(float)) {
    odvae_set_error("colsum: needs %zu workspace bytes", (size_t)nblk * C * sizeof(float));
    return ODVAE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  const int rpb = (int)ceil_div64(rows, nblk);
  const int nb = (int)ceil_div64(rows, rpb);
  hipLaunchKernelGGL(colsum_partial_kernel, dim3(nb), dim3(256), 0, st, x, rows, C, rpb, part);
  hipLaunchKernelGGL(colsum_final_kernel, dim3(ceil_div(C, 4)), dim3(256), 0, st, part, nb, C, out);
  ODVAE_LAUNCH_CHECK("colsum");
  return ODVAE_OK;
}

// out[0] = ||g||_2, out[1] = min(1, max_norm/(norm+1e-6)) (1 when max_norm <= 0).  workspace: 1024 floats
int odvae_grad_norm_f32(const float* g, int64_t n, float max_norm, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(g && out && n > 0, "grad_norm: bad arguments");
  ODVAE_CHECK_ARG(((uintptr_t)g & 15) == 0, "grad_norm: g must be 16-byte aligned");
  const int nblk = 1024;
  if (!workspace || workspace_bytes < (size_t)nblk * sizeof(float)) {
    odvae_set_error("grad_norm: needs %zu workspace bytes", (size_t)nblk * sizeof(float));
    return ODVAE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nblk), dim3(256), 0, st, g, n, part);
  hipLaunchKernelGGL(norm_final_kernel, dim3(1), dim3(64), 0, st, part, nblk, max_norm, out);
  ODVAE_LAUNCH_CHECK("grad_norm");
  return ODVAE_OK;
}

// one Adam step over a flat arena; step >= 1; clip = device pointer written by odvae_grad_norm_f32 or null
int odvae_adam_step_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                        float eps, int step, const float* clip, void* stream) {
  ODVAE_CHECK_ARG(p && g && m && v && n > 0 && step >= 1, "adam_step: bad arguments");
  ODVAE_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "adam_step: arenas must be 16-byte aligned");
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const float bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  hipLaunchKernelGGL(adam_kernel<false>, dim3(grid_1d(n / 4 + 1)), dim3(256), 0, static_cast<hipStream_t>(stream), p, g, m, v, n, lr, beta1, beta2, eps, bc1, bc2_sqrt, clip, 0.f);
  ODVAE_LAUNCH_CHECK("adam_step");
  return ODVAE_OK;
}

// the same step with gr = clamp(g, -clamp, +clamp) in place of g * coefficient (torch.nn.utils.clip_grad_value_ folded into the step)
int odvae_adam_step_clamp_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                              float eps, int step, float clamp, void* stream) {
  ODVAE_CHECK_ARG(p && g && m && v && n > 0 && step >= 1, "adam_step_clamp: bad arguments");
  ODVAE_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "adam_step_clamp: arenas must be 16-byte aligned");
  ODVAE_CHECK_ARG(clamp > 0.f, "adam_step_clamp: the clamp must be > 0, got %g", (double)clamp);      // (a NaN fails the comparison too)
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const float bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
  hipLaunchKernelGGL(adam_kernel<true>, dim3(grid_1d(n / 4 + 1)), dim3(256), 0, static_cast<hipStream_t>(stream), p, g, m, v, n, lr, beta1, beta2, eps, bc1, bc2_sqrt,
                     (const float*)nullptr, clamp);
  ODVAE_LAUNCH_CHECK("adam_step_clamp");
  return ODVAE_OK;
}

int odvae_grad_seg_norms_segments_per_launch(void) { return kSegNormSegs; }

// chunks of all segments, or -1 when a length is <= 0 or the chunks do not fit the 31-bit chunk index
static int64_t seg_norm_chunks(const int64_t* len, int n_seg) {
  int64_t chunks = 0;
  for (int i = 0; i < n_seg; ++i) {
    if (len[i] <= 0 || len[i] > (int64_t)0x7fffffff * kSegNormChunk) return -1;
    chunks += ceil_div64(len[i], kSegNormChunk);
    if (chunks > 0x7fffffffll) return -1;
  }
  return chunks;
}

// one record per segment, then one double per chunk; 0 for arguments odvae_grad_seg_norms_f32 refuses
size_t odvae_grad_seg_norms_workspace_bytes(const int64_t* len, int n_seg) {
  if (!len || n_seg <= 0) return 0;
  const int64_t chunks = seg_norm_chunks(len, n_seg);
  if (chunks < 0) return 0;
  return (size_t)n_seg * sizeof(SegNormRecord) + (size_t)chunks * sizeof(double);
}

extern "C++" {
template <int KIND>
static void seg_norm_launch(const float* g, const int64_t* off, const int64_t* len, const unsigned char* counts, int n_seg, double p, float* out,
                            SegNormRecord* rec, double* part, hipStream_t st) {
  SegNormTable t;
  uint64_t chunk_base = 0;
  for (int i = 0; i < n_seg;) {
    uint64_t chunks = 0;
    int k = 0;
    t.seg_base = i;
    for (; k < kSegNormSegs && i < n_seg; ++k, ++i) {
      t.off[k] = off[i];
      t.len[k] = len[i];
      t.counts[k] = counts ? (counts[i] != 0) : 1;
      t.chunk_prefix[k] = (unsigned)chunks;
      chunks += (uint64_t)ceil_div64(len[i], kSegNormChunk);
    }
    for (int j = k; j <= kSegNormSegs; ++j) t.chunk_prefix[j] = (unsigned)chunks;
    for (int j = k; j < kSegNormSegs; ++j) { t.off[j] = 0; t.len[j] = 0; t.counts[j] = 0; }
    t.count = k;
    t.chunk_base = (unsigned)chunk_base;
    hipLaunchKernelGGL(seg_norm_partial_kernel<KIND>, dim3((unsigned)std::min<uint64_t>(chunks, 65536)), dim3(256), 0, st, g, t, p, part, rec);
    chunk_base += chunks;
  }
  hipLaunchKernelGGL(seg_norm_final_kernel<KIND>, dim3(ceil_div(n_seg, 4)), dim3(256), 0, st, (const double*)part, (const SegNormRecord*)rec, n_seg, p, out);
  hipLaunchKernelGGL(seg_norm_total_kernel<KIND>, dim3(1), dim3(256), 0, st, (const SegNormRecord*)rec, n_seg, p, out);
}
}  // extern "C++"

// out[i] = p-norm of g[off[i] .. off[i] + len[i]), i < n_seg; out[n_seg] = the same norm of the f32 values out[i] with counts[i] != 0
// (counts null: all).  off / len / counts are host arrays.  ceil(n_seg / K) + 2 launches; everything is validated before the first
int odvae_grad_seg_norms_f32(const float* g, int64_t n, const int64_t* off, const int64_t* len, const unsigned char* counts, int n_seg,
                             int kind, double p, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(g && out && off && len && n > 0, "grad_seg_norms: null arena / table / out");
  ODVAE_CHECK_ARG(n_seg > 0, "grad_seg_norms: n_seg %d <= 0", n_seg);
  ODVAE_CHECK_ARG(((uintptr_t)g & 15) == 0 && ((uintptr_t)out & 3) == 0, "grad_seg_norms: g must be 16-byte, out 4-byte aligned");
  ODVAE_CHECK_ARG(kind == kNormMax || kind == kNormL1 || kind == kNormL2 || kind == kNormP, "grad_seg_norms: unknown kind %d", kind);
  ODVAE_CHECK_ARG(kind != kNormP || (p > 0.0 && p <= 1.7976931348623157e308), "grad_seg_norms: the general kind needs a finite p > 0, got %g", p);
  for (int i = 0; i < n_seg; ++i) {
    ODVAE_CHECK_ARG(len[i] > 0, "grad_seg_norms: segment %d has length %lld", i, (long long)len[i]);
    ODVAE_CHECK_ARG(off[i] >= 0 && (off[i] & 3) == 0, "grad_seg_norms: segment %d starts at float %lld, not on a 16-byte boundary", i, (long long)off[i]);
    ODVAE_CHECK_ARG(off[i] <= n && len[i] <= n - off[i], "grad_seg_norms: segment %d [%lld, +%lld) leaves the arena of %lld floats", i,
                    (long long)off[i], (long long)len[i], (long long)n);
  }
  const size_t need = odvae_grad_seg_norms_workspace_bytes(len, n_seg);
  ODVAE_CHECK_ARG(need > 0, "grad_seg_norms: the segments have too many chunks of %d floats", kSegNormChunk);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) != 0) {
    odvae_set_error("grad_seg_norms: needs %zu workspace bytes, 16-byte aligned", need);
    return ODVAE_ERR_WORKSPACE;
  }
  SegNormRecord* rec = static_cast<SegNormRecord*>(workspace);
  double* part = reinterpret_cast<double*>(rec + n_seg);
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (kind) {
    case kNormMax: seg_norm_launch<kNormMax>(g, off, len, counts, n_seg, p, out, rec, part, st); break;
    case kNormL1: seg_norm_launch<kNormL1>(g, off, len, counts, n_seg, p, out, rec, part, st); break;
    case kNormL2: seg_norm_launch<kNormL2>(g, off, len, counts, n_seg, p, out, rec, part, st); break;
    default: seg_norm_launch<kNormP>(g, off, len, counts, n_seg, p, out, rec, part, st); break;
  }
  ODVAE_LAUNCH_CHECK("grad_seg_norms");
  return ODVAE_OK;
}

int odvae_grad_accumulate_segments_per_launch(void) { return kGradAccSegs; }

// arena[dst_off[i] + j] += src[i][j] for count disjoint segments (dst_off / numel: host arrays, src: host array of device pointers);
// ceil(count / K) launches, K = odvae_grad_accumulate_segments_per_launch(); nothing is launched unless every segment is valid
int odvae_grad_accumulate_f32(float* arena, int64_t arena_numel, const int64_t* dst_off, const float* const* src, const int64_t* numel,
                              int count, void* stream) {
  ODVAE_CHECK_ARG(count >= 0, "grad_accumulate: count %d < 0", count);
  if (count == 0) return ODVAE_OK;
  ODVAE_CHECK_ARG(arena && arena_numel > 0 && dst_off && src && numel, "grad_accumulate: null arena / table");
  for (int i = 0; i < count; ++i) {
    ODVAE_CHECK_ARG(src[i] != nullptr, "grad_accumulate: segment %d has a null source", i);
    ODVAE_CHECK_ARG(numel[i] > 0, "grad_accumulate: segment %d has numel %lld", i, (long long)numel[i]);
    ODVAE_CHECK_ARG(dst_off[i] >= 0 && dst_off[i] <= arena_numel && numel[i] <= arena_numel - dst_off[i],
                    "grad_accumulate: segment %d [%lld, +%lld) leaves the arena of %lld floats", i, (long long)dst_off[i], (long long)numel[i],
                    (long long)arena_numel);
    ODVAE_CHECK_ARG(ceil_div64(numel[i], kGradAccChunk) <= 0x7fffffffll, "grad_accumulate: segment %d of %lld floats is too large", i, (long long)numel[i]);
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  GradAccTable t;
  int i = 0;
  while (i < count) {
    uint64_t chunks = 0;
    int k = 0;
    for (; k < kGradAccSegs && i < count; ++k, ++i) {
      const uint64_t c = (uint64_t)ceil_div64(numel[i], kGradAccChunk);
      if (k > 0 && chunks + c > 0x7fffffffull) break;      // (the prefix is 32-bit: a launch closes early; one segment alone always fits)
      t.dst[k] = arena + dst_off[i];
      t.src[k] = src[i];
      t.numel[k] = numel[i];
      t.chunk_prefix[k] = (unsigned)chunks;
      chunks += c;
    }
    for (int j = k; j <= kGradAccSegs; ++j) t.chunk_prefix[j] = (unsigned)chunks;
    for (int j = k; j < kGradAccSegs; ++j) { t.dst[j] = nullptr; t.src[j] = nullptr; t.numel[j] = 0; }
    t.count = k;
    hipLaunchKernelGGL(grad_accumulate_kernel, dim3((unsigned)std::min<uint64_t>(chunks, 8192)), dim3(256), 0, st, t);
    ODVAE_LAUNCH_CHECK("grad_accumulate");
  }
  return ODVAE_OK;
}

// LitEma's counter and decay schedule, on the device: nothing is read back.  state (2 floats) receives [1 - d, d]
int odvae_ema_tick(const float* decay, int* num_updates, float* state, void* stream) {
  ODVAE_CHECK_ARG(decay && num_updates && state, "ema_tick: bad arguments");
  ODVAE_CHECK_ARG((((uintptr_t)decay | (uintptr_t)num_updates | (uintptr_t)state) & 3) == 0, "ema_tick: pointers must be 4-byte aligned");
  hipLaunchKernelGGL(ema_tick_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), decay, num_updates, state);
  ODVAE_LAUNCH_CHECK("ema_tick");
  return ODVAE_OK;
}

static bool f32_ranges_overlap(const float* a, const float* b, int64_t n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, len = (uintptr_t)n * sizeof(float);
  return x < y + len && y < x + len;
}

// shadow[i] <- shadow[i] - omd[0] * (shadow[i] - p[i]), i < n: three f32 roundings per element; omd = the state odvae_ema_tick wrote
int odvae_ema_update_f32(const float* p, float* shadow, int64_t n, const float* omd, void* stream) {
  ODVAE_CHECK_ARG(p && shadow && omd && n > 0, "ema_update: bad arguments");
  ODVAE_CHECK_ARG((((uintptr_t)p | (uintptr_t)shadow | (uintptr_t)omd) & 3) == 0, "ema_update: pointers must be 4-byte aligned");
  ODVAE_CHECK_ARG(!f32_ranges_overlap(p, shadow, n), "ema_update: the parameters and their shadow overlap");
  const PairSpan sp = pair_span(p, shadow, n);
  hipLaunchKernelGGL(ema_update_kernel, dim3(grid_1d(std::max(sp.n4, sp.nscalar))), dim3(256), 0, static_cast<hipStream_t>(stream), p, shadow, sp, omd);
  ODVAE_LAUNCH_CHECK("ema_update");
  return ODVAE_OK;
}

// a[i] <-> b[i], i < n, in one pass over two disjoint arrays
int odvae_ema_swap_f32(float* a, float* b, int64_t n, void* stream) {
  ODVAE_CHECK_ARG(a && b && n > 0, "ema_swap: bad arguments");
  ODVAE_CHECK_ARG((((uintptr_t)a | (uintptr_t)b) & 3) == 0, "ema_swap: pointers must be 4-byte aligned");
  ODVAE_CHECK_ARG(!f32_ranges_overlap(a, b, n), "ema_swap: the two arrays overlap");
  const PairSpan sp = pair_span(a, b, n);
  hipLaunchKernelGGL(ema_swap_kernel, dim3(grid_1d(std::max(sp.n4, sp.nscalar))), dim3(256), 0, static_cast<hipStream_t>(stream), a, b, sp);
  ODVAE_LAUNCH_CHECK("ema_swap");
  return ODVAE_OK;
}

int odvae_nhwc_to_nchw_f32(const float* x, float* y, int N, int C, int HW, void* stream) {
  ODVAE_CHECK_ARG(x && y && N > 0 && C > 0 && HW > 0, "nhwc_to_nchw: bad arguments");
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(grid_1d((int64_t)N * C * HW)), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, N, C, HW);
  ODVAE_LAUNCH_CHECK("nhwc_to_nchw");
  return ODVAE_OK;
}

}  // extern "C"
