// LPIPS-style perceptual distance support kernels, NHWC f32, gfx950.  All HBM-bound.
//
// [UPSTREAM] taming/modules/losses/lpips.py (reference call site src/modules/losses/contperceptual.py:143):
//   ScalingLayer  (x - shift) / scale                           -> scaling_layer_kernel
//   VGG16 slices  conv3x3+ReLU (conv3x3_f32.hip, act = 1), MaxPool2d(2,2) -> maxpool2x2_*_kernel
//   per tap k     normalize_tensor(f) = f / (sqrt(sum_c f^2) + 1e-10); lin_k((n0 - n1)^2); spatial mean
//                                                               -> lpips_distance_*_kernel (one wavefront per pixel)
#include "common.h"

namespace {

// y = (x - shift[c]) / scale[c];  bwd (INV): y = x / scale[c]
template <bool BWD>
__global__ __launch_bounds__(256) void scaling_layer_kernel(const float* __restrict__ x, const float* __restrict__ shift,
                                                            const float* __restrict__ scale, float* __restrict__ y, int64_t total, int C) {
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    y[idx] = BWD ? x[idx] / scale[c] : (x[idx] - shift[c]) / scale[c];
  }
}

// y[n][oy][ox][c] = max over the 2x2 window of x [N][H][W][C], Ho = H / 2, Wo = W / 2: an odd last row / column is dropped (torch floors).
// A window that holds a NaN yields NaN (torch's scan keeps the last one); fmaxf alone would return the window's largest number.
__device__ __forceinline__ float max4_nan(float a, float b, float c, float d) {
  float m = fmaxf(fmaxf(a, b), fmaxf(c, d));
  m = a != a ? a : m; m = b != b ? b : m; m = c != c ? c : m; m = d != d ? d : m;
  return m;
}
__global__ __launch_bounds__(256) void maxpool2x2_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W, int C) {
  const int q = C / 4, Ho = H / 2, Wo = W / 2;
  const int64_t row = (int64_t)W * C;
  const int64_t total = (int64_t)N * Ho * Wo * q;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int cq = (int)(idx % q);
    int64_t r = idx / q;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho); const int n = (int)(r / Ho);
    const float* s = x + (((int64_t)n * H + 2 * oy) * W + 2 * ox) * C + 4 * cq;
    const float4 a = *reinterpret_cast<const float4*>(s), b = *reinterpret_cast<const float4*>(s + C);
    const float4 c = *reinterpret_cast<const float4*>(s + row), d = *reinterpret_cast<const float4*>(s + row + C);
    float4 o;
    o.x = max4_nan(a.x, b.x, c.x, d.x); o.y = max4_nan(a.y, b.y, c.y, d.y);
    o.z = max4_nan(a.z, b.z, c.z, d.z); o.w = max4_nan(a.w, b.w, c.w, d.w);
    *reinterpret_cast<float4*>(y + idx * 4) = o;
  }
}

// dx: dy goes to the first element of the window (row-major scan) that equals the max, zero elsewhere (torch rule); where the max is
// NaN, to the window's first NaN.  One thread per 2x2 cell of the input and channel, the cells of an odd last row / column included:
// those hold one or two pixels that no window covers, and get 0, so every element of dx is written.
__global__ __launch_bounds__(256) void maxpool2x2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ dy, float* __restrict__ dx,
                                                             int N, int H, int W, int C) {
  const int Ho = H / 2, Wo = W / 2, Hc = (H + 1) / 2, Wc = (W + 1) / 2;
  const int64_t row = (int64_t)W * C;
  const int64_t total = (int64_t)N * Hc * Wc * C;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    int64_t r = idx / C;
    const int cx = (int)(r % Wc); r /= Wc;
    const int cy = (int)(r % Hc); const int n = (int)(r / Hc);
    const int64_t base = (((int64_t)n * H + 2 * cy) * W + 2 * cx) * C + c;
    if (cy < Ho && cx < Wo) {
      const int64_t off[4] = {0, C, row, row + C};
      const int64_t o = (((int64_t)n * Ho + cy) * Wo + cx) * C + c;
      const float m = y[o], g = dy[o];
      bool done = false;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float v = x[base + off[k]];
        const bool hit = !done && (v == m || (m != m && v != v));
        dx[base + off[k]] = hit ? g : 0.f;
        done = done || hit;
      }
    } else {      // cy == Ho (H odd) and / or cx == Wo (W odd): the cell's pixels that exist
      dx[base] = 0.f;
      if (2 * cx + 1 < W) dx[base + C] = 0.f;
      if (2 * cy + 1 < H) dx[base + row] = 0.f;
    }
  }
}

// One wavefront per pixel, lanes over channels (C <= 512: <= 8 channels per lane).
// d(pixel) = sum_c w[c] * (f0/n0 - f1/n1)^2, n = sqrt(sum f^2) + 1e-10.  part[n][blk] = sum of d over the block's pixels
constexpr int MAXCPL = 8;
__global__ __launch_bounds__(256) void lpips_distance_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                                             const float* __restrict__ w, int HW, int C, float* __restrict__ part) {
  __shared__ float sh[4];
  const int n = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cpl = C / 64 > 0 ? (C + 63) / 64 : 1;
  float acc = 0.f;
  for (int px = blockIdx.x * 4 + wave; px < HW; px += gridDim.x * 4) {
    const float* a = f0 + ((int64_t)n * HW + px) * C;
    const float* b = f1 + ((int64_t)n * HW + px) * C;
    float va[MAXCPL], vb[MAXCPL], sa = 0.f, sb = 0.f;
#pragma unroll
    for (int k = 0; k < MAXCPL; ++k) {
      const int c = lane + 64 * k;
      va[k] = (k < cpl && c < C) ? a[c] : 0.f;
      vb[k] = (k < cpl && c < C) ? b[c] : 0.f;
      sa += va[k] * va[k]; sb += vb[k] * vb[k];
    }
    sa = wave_sum(sa); sb = wave_sum(sb);
    const float ia = 1.f / (sqrtf(sa) + 1e-10f), ib = 1.f / (sqrtf(sb) + 1e-10f);
    float d = 0.f;
#pragma unroll
    for (int k = 0; k < MAXCPL; ++k) {
      const int c = lane + 64 * k;
      if (k < cpl && c < C) { const float t = va[k] * ia - vb[k] * ib; d += w[c] * t * t; }
    }
    acc += d;   // lane-partial; reduced once at the end
  }
  acc = wave_sum(acc);
  if (lane == 0) sh[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[(int64_t)n * gridDim.x + blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ void lpips_mean_final_kernel(const float* __restrict__ part, int nblk, float inv_hw, float* __restrict__ out) {
  const int n = blockIdx.x;
  double s = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 64) s += (double)part[(int64_t)n * nblk + i];
  s = wave_sum_f64(s);
  if (threadIdx.x == 0) out[n] = (float)(s * (double)inv_hw);
}

// gradient w.r.t. f1 (the reconstruction branch): g[n] = d loss / d out[n]
__global__ __launch_bounds__(256) void lpips_distance_bwd_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                                                 const float* __restrict__ w, const float* __restrict__ g,
                                                                 int HW, int C, float* __restrict__ df1) {
  const int n = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cpl = (C + 63) / 64;
  const float gs = g[n] / (float)HW;
  for (int px = blockIdx.x * 4 + wave; px < HW; px += gridDim.x * 4) {
    const int64_t base = ((int64_t)n * HW + px) * C;
    float va[MAXCPL], vb[MAXCPL], sa = 0.f, sb = 0.f;
#pragma unroll
    for (int k = 0; k < MAXCPL; ++k) {
      const int c = lane + 64 * k;
      va[k] = (k < cpl && c < C) ? f0[base + c] : 0.f;
      vb[k] = (k < cpl && c < C) ? f1[base + c] : 0.f;
      sa += va[k] * va[k]; sb += vb[k] * vb[k];
    }
    sa = wave_sum(sa); sb = wave_sum(sb);
    const float s1 = sqrtf(sb);
    const float n1 = s1 + 1e-10f;
    const float ia = 1.f / (sqrtf(sa) + 1e-10f), ib = 1.f / n1;
    // gb[c] = d d / d b_c = -2 w (a_c - b_c);  df1_k = gb_k / n1 - (sum_c gb_c f1_c) f1_k / (n1^2 s1)
    float gb[MAXCPL], dot = 0.f;
#pragma unroll
    for (int k = 0; k < MAXCPL; ++k) {
      const int c = lane + 64 * k;
      gb[k] = (k < cpl && c < C) ? -2.f * w[c] * (va[k] * ia - vb[k] * ib) : 0.f;
      dot += gb[k] * vb[k];
    }
    dot = wave_sum(dot);
    const float coef = s1 > 0.f ? dot / (n1 * n1 * s1) : 0.f;   // torch gives NaN at an all-zero feature vector; 0 here
#pragma unroll
    for (int k = 0; k < MAXCPL; ++k) {
      const int c = lane + 64 * k;
      if (k < cpl && c < C) df1[base + c] = gs * (gb[k] * ib - coef * vb[k]);
    }
  }
}

}  // namespace

extern "C" {

// ScalingLayer: y = (x - shift[c]) / scale[c]; backward = 1: y = x / scale[c] (x = dy)
int odvae_scaling_layer_f32(const float* x, const float* shift, const float* scale, float* y, int64_t npix, int C, int backward, void* stream) {
  ODVAE_CHECK_ARG(x && shift && scale && y && npix > 0 && C > 0, "scaling_layer: bad arguments");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (backward) hipLaunchKernelGGL((scaling_layer_kernel<true>), dim3(grid_1d(npix * C)), dim3(256), 0, st, x, shift, scale, y, npix * C, C);
  else hipLaunchKernelGGL((scaling_layer_kernel<false>), dim3(grid_1d(npix * C)), dim3(256), 0, st, x, shift, scale, y, npix * C, C);
  ODVAE_LAUNCH_CHECK("scaling_layer");
  return ODVAE_OK;
}

// x [N][Hi][Wi][C] -> y [N][Ho][Wo][C], Ho = Hi / 2, Wo = Wi / 2 (floor, as torch.nn.MaxPool2d(2, 2))
int odvae_maxpool2x2_f32(const float* x, float* y, int N, int Hi, int Wi, int C, int Ho, int Wo, void* stream) {
  ODVAE_CHECK_ARG(x && y && N > 0 && Hi >= 2 && Wi >= 2 && C > 0 && C % 4 == 0, "maxpool2x2: need Hi, Wi >= 2 and C %% 4 == 0");
  ODVAE_CHECK_ARG(Ho == Hi / 2 && Wo == Wi / 2, "maxpool2x2: Ho/Wo must be Hi / 2, Wi / 2 (floor): got %d x %d for %d x %d", Ho, Wo, Hi, Wi);
  hipLaunchKernelGGL(maxpool2x2_kernel, dim3(grid_1d((int64_t)N * Ho * Wo * (C / 4))), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, N, Hi, Wi, C);
  ODVAE_LAUNCH_CHECK("maxpool2x2");
  return ODVAE_OK;
}

// writes all of dx [N][Hi][Wi][C]: an odd last row / column gets 0
int odvae_maxpool2x2_bwd_f32(const float* x, const float* y, const float* dy, float* dx, int N, int Hi, int Wi, int C, int Ho, int Wo, void* stream) {
  ODVAE_CHECK_ARG(x && y && dy && dx && N > 0 && Hi >= 2 && Wi >= 2 && C > 0, "maxpool2x2_bwd: bad arguments");
  ODVAE_CHECK_ARG(Ho == Hi / 2 && Wo == Wi / 2, "maxpool2x2_bwd: Ho/Wo must be Hi / 2, Wi / 2 (floor): got %d x %d for %d x %d", Ho, Wo, Hi, Wi);
  const int64_t cells = (int64_t)N * ((Hi + 1) / 2) * ((Wi + 1) / 2) * C;
  hipLaunchKernelGGL(maxpool2x2_bwd_kernel, dim3(grid_1d(cells)), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, dy, dx, N, Hi, Wi, C);
  ODVAE_LAUNCH_CHECK("maxpool2x2_bwd");
  return ODVAE_OK;
}

// out[n] = mean over pixels of sum_c w[c]*(normalize(f0) - normalize(f1))^2.  workspace: N*256 floats.  C <= 512
int odvae_lpips_distance_f32(const float* f0, const float* f1, const float* w, float* out, int N, int HW, int C,
                             void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(f0 && f1 && w && out && N > 0 && HW > 0 && C > 0 && C <= 64 * MAXCPL, "lpips_distance: need C <= %d", 64 * MAXCPL);
  const int nblk = (int)std::min<int64_t>(256, std::max<int64_t>(1, HW / 4));
  if (!workspace || workspace_bytes < (size_t)N * nblk * sizeof(float)) {
    odvae_set_error("lpips_distance: needs %zu workspace bytes", (size_t)N * nblk * sizeof(float));
    return ODVAE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(lpips_distance_kernel, dim3(nblk, N), dim3(256), 0, st, f0, f1, w, HW, C, part);
  hipLaunchKernelGGL(lpips_mean_final_kernel, dim3(N), dim3(64), 0, st, part, nblk, 1.f / (float)HW, out);
  ODVAE_LAUNCH_CHECK("lpips_distance");
  return ODVAE_OK;
}

int odvae_lpips_distance_bwd_f32(const float* f0, const float* f1, const float* w, const float* g, float* df1,
                                 int N, int HW, int C, void* stream) {
  ODVAE_CHECK_ARG(f0 && f1 && w && g && df1 && N > 0 && HW > 0 && C > 0 && C <= 64 * MAXCPL, "lpips_distance_bwd: bad arguments");
  const int nblk = (int)std::min<int64_t>(2048, std::max<int64_t>(1, HW / 4));
  hipLaunchKernelGGL(lpips_distance_bwd_kernel, dim3(nblk, N), dim3(256), 0, static_cast<hipStream_t>(stream), f0, f1, w, g, HW, C, df1);
  ODVAE_LAUNCH_CHECK("lpips_distance_bwd");
  return ODVAE_OK;
}

}  // extern "C"
