// LPIPS-style perceptual distance support kernels on bf16 NHWC features, gfx950: the bf16 forms of lpips_f32.hip for the opt-in bf16
// perceptual net (LPIPSStyle.set_precision("bf16")).  Features and their gradients are bf16 in HBM, rounded to nearest even exactly once
// per store; every sum, norm and product in between is f32.  All HBM-bound.  The conv + ReLU layers are conv_bf16.hip (RELU / MASK).
//
// ReLU masks.  The VGG stack is conv+ReLU layers, pools and distance taps; a ReLU's backward, dy * (y > 0), is folded into whichever
// kernel PRODUCES dy, i.e. into the backward of the layer that consumed y: the masked conv data gradient, the pool backward and the
// distance backward below all take the consumed ReLU output as `mask` and write `mask > 0 ? value : 0`.  What they leave in HBM is the
// gradient at the pre-activation, and no separate mask pass runs.
#include "bf16_common.h"

namespace {

// y bf16 [npix][8] = ((x - shift[c]) / scale[c], c < C; 0 for the padding channels), x f32 [npix][C], C <= 8
__global__ __launch_bounds__(256) void scaling_layer_bf16_kernel(const float* __restrict__ x, const float* __restrict__ shift,
                                                                 const float* __restrict__ scale, bf16_t* __restrict__ y, int64_t npix, int C) {
  float sh[8], sc[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) { sh[c] = c < C ? shift[c] : 0.f; sc[c] = c < C ? scale[c] : 1.f; }
  for (int64_t px = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; px < npix; px += (int64_t)gridDim.x * blockDim.x) {
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = c < C ? (x[px * C + c] - sh[c]) / sc[c] : 0.f;
    u32x4 o;
    o.x = cvt_pk_bf16(v[0], v[1]); o.y = cvt_pk_bf16(v[2], v[3]); o.z = cvt_pk_bf16(v[4], v[5]); o.w = cvt_pk_bf16(v[6], v[7]);
    *reinterpret_cast<u32x4*>(y + px * 8) = o;
  }
}

// dx = y > 0 ? dy : 0 (the backward of a ReLU whose consumer did not fold the mask in), 4 elements per thread
__global__ __launch_bounds__(256) void relu_bwd_bf16_kernel(const bf16_t* __restrict__ y, const bf16_t* __restrict__ dy, bf16_t* __restrict__ dx, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const u32x2 m = *reinterpret_cast<const u32x2*>(y + 4 * i);
    u32x2 g = *reinterpret_cast<const u32x2*>(dy + 4 * i);
    g.x = (bf16_lo(m.x) > 0.f ? g.x & 0xFFFFu : 0u) | (bf16_hi(m.x) > 0.f ? g.x & 0xFFFF0000u : 0u);
    g.y = (bf16_lo(m.y) > 0.f ? g.y & 0xFFFFu : 0u) | (bf16_hi(m.y) > 0.f ? g.y & 0xFFFF0000u : 0u);
    *reinterpret_cast<u32x2*>(dx + 4 * i) = g;
  }
}

// the window's maximum as torch's scan finds it; a window that holds a NaN yields (its last) NaN
__device__ __forceinline__ float max4_nan(float a, float b, float c, float d) {
  float m = fmaxf(fmaxf(a, b), fmaxf(c, d));
  m = a != a ? a : m; m = b != b ? b : m; m = c != c ? c : m; m = d != d ? d : m;
  return m;
}
__device__ __forceinline__ void unpack4(u32x2 v, float (&f)[4]) { f[0] = bf16_lo(v.x); f[1] = bf16_hi(v.x); f[2] = bf16_lo(v.y); f[3] = bf16_hi(v.y); }
// the values are bf16 already: the upper halves are the exact bits (a NaN keeps its payload)
__device__ __forceinline__ u32x2 pack4_exact(const float (&f)[4]) {
  u32x2 v;
  v.x = (__float_as_uint(f[0]) >> 16) | (__float_as_uint(f[1]) & 0xFFFF0000u);
  v.y = (__float_as_uint(f[2]) >> 16) | (__float_as_uint(f[3]) & 0xFFFF0000u);
  return v;
}

// y[n][oy][ox][c] = max over the 2x2 window of x [N][H][W][C], Ho = H / 2, Wo = W / 2 (an odd last row / column is dropped); C % 4 == 0
__global__ __launch_bounds__(256) void maxpool2x2_bf16_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, int N, int H, int W, int C) {
  const int q = C / 4, Ho = H / 2, Wo = W / 2;
  const int64_t row = (int64_t)W * C;
  const int64_t total = (int64_t)N * Ho * Wo * q;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int cq = (int)(idx % q);
    int64_t r = idx / q;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho); const int n = (int)(r / Ho);
    const bf16_t* s = x + (((int64_t)n * H + 2 * oy) * W + 2 * ox) * C + 4 * cq;
    float a[4], b[4], c[4], d[4], o[4];
    unpack4(*reinterpret_cast<const u32x2*>(s), a); unpack4(*reinterpret_cast<const u32x2*>(s + C), b);
    unpack4(*reinterpret_cast<const u32x2*>(s + row), c); unpack4(*reinterpret_cast<const u32x2*>(s + row + C), d);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = max4_nan(a[j], b[j], c[j], d[j]);
    *reinterpret_cast<u32x2*>(y + idx * 4) = pack4_exact(o);
  }
}

// dx: dy goes to the first element of the window (row-major scan) that equals the max, zero elsewhere (torch rule); where the max is NaN,
// to the window's first NaN.  With a mask (the pool's input is a ReLU output: mask = that output) the element is kept only where
// mask > 0.  One thread per 2x2 cell of the input and 4 channels, the cells of an odd last row / column included: those get 0, so every
// element of dx is written.  The window's max is recomputed from x (no read of y).
__global__ __launch_bounds__(256) void maxpool2x2_bwd_bf16_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                                  const bf16_t* __restrict__ mask, bf16_t* __restrict__ dx,
                                                                  int N, int H, int W, int C) {
  const int q = C / 4, Ho = H / 2, Wo = W / 2, Hc = (H + 1) / 2, Wc = (W + 1) / 2;
  const int64_t row = (int64_t)W * C;
  const int64_t total = (int64_t)N * Hc * Wc * q;
  const u32x2 zero = {0u, 0u};
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int cq = (int)(idx % q);
    int64_t r = idx / q;
    const int cx = (int)(r % Wc); r /= Wc;
    const int cy = (int)(r % Hc); const int n = (int)(r / Hc);
    const int64_t base = (((int64_t)n * H + 2 * cy) * W + 2 * cx) * C + 4 * cq;
    if (cy < Ho && cx < Wo) {
      const int64_t off[4] = {0, C, row, row + C};
      float v[4][4], mk[4][4], g[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) unpack4(*reinterpret_cast<const u32x2*>(x + base + off[k]), v[k]);
      if (mask) {
#pragma unroll
        for (int k = 0; k < 4; ++k) unpack4(*reinterpret_cast<const u32x2*>(mask + base + off[k]), mk[k]);
      }
      unpack4(*reinterpret_cast<const u32x2*>(dy + (((int64_t)n * Ho + cy) * Wo + cx) * C + 4 * cq), g);
      float o[4][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float m = max4_nan(v[0][j], v[1][j], v[2][j], v[3][j]);
        bool done = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const bool hit = !done && (v[k][j] == m || (m != m && v[k][j] != v[k][j]));
          const bool keep = hit && (!mask || mk[k][j] > 0.f);
          o[k][j] = keep ? g[j] : 0.f;
          done = done || hit;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) *reinterpret_cast<u32x2*>(dx + base + off[k]) = pack4_exact(o[k]);
    } else {      // cy == Ho (H odd) and / or cx == Wo (W odd): the cell's pixels that exist
      *reinterpret_cast<u32x2*>(dx + base) = zero;
      if (2 * cx + 1 < W) *reinterpret_cast<u32x2*>(dx + base + C) = zero;
      if (2 * cy + 1 < H) *reinterpret_cast<u32x2*>(dx + base + row) = zero;
    }
  }
}

// A lane keeps CPL consecutive channels of one pixel (C = 64 * CPL), one load_run / store_run_rne (bf16_common.h) each.
// One wavefront per pixel.  d(pixel) = sum_c w[c] * (f0/n0 - f1/n1)^2, n = sqrt(sum f^2) + 1e-10, in f32 as lpips_distance_kernel.
// part[n][blk] = sum of d over the block's pixels
template <int CPL>
__global__ __launch_bounds__(256) void lpips_distance_bf16_kernel(const bf16_t* __restrict__ f0, const bf16_t* __restrict__ f1,
                                                                  const float* __restrict__ w, int HW, float* __restrict__ part) {
  constexpr int C = 64 * CPL;
  __shared__ float sh[4];
  const int n = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float wv[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) wv[k] = w[lane * CPL + k];
  float acc = 0.f;
  for (int px = blockIdx.x * 4 + wave; px < HW; px += gridDim.x * 4) {
    const int64_t base = ((int64_t)n * HW + px) * C + lane * CPL;
    float va[CPL], vb[CPL], sa = 0.f, sb = 0.f;
    load_run<CPL>(f0 + base, va); load_run<CPL>(f1 + base, vb);
#pragma unroll
    for (int k = 0; k < CPL; ++k) { sa += va[k] * va[k]; sb += vb[k] * vb[k]; }
    sa = wave_sum(sa); sb = wave_sum(sb);
    const float ia = 1.f / (sqrtf(sa) + 1e-10f), ib = 1.f / (sqrtf(sb) + 1e-10f);
    float d = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) { const float t = va[k] * ia - vb[k] * ib; d += wv[k] * t * t; }
    acc += d;   // lane-partial; reduced once at the end
  }
  acc = wave_sum(acc);
  if (lane == 0) sh[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[(int64_t)n * gridDim.x + blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ void lpips_mean_final_bf16_kernel(const float* __restrict__ part, int nblk, float inv_hw, float* __restrict__ out) {
  const int n = blockIdx.x;
  double s = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 64) s += (double)part[(int64_t)n * nblk + i];
  s = wave_sum_f64(s);
  if (threadIdx.x == 0) out[n] = (float)(s * (double)inv_hw);
}

// Gradient w.r.t. f1 (the reconstruction branch) at the tap, g[n] = d loss / d out[n]:
//   df1 = round_bf16( mask > 0 ? (distance gradient, f32 as lpips_distance_bwd_kernel) + dnext : 0 )
// dnext (or null): the bf16 gradient arriving at the same tensor from the next slice's pool; mask (or null): the tap's own ReLU output.
// One f32 sum, one mask, one rounding.
template <int CPL>
__global__ __launch_bounds__(256) void lpips_distance_bwd_bf16_kernel(const bf16_t* __restrict__ f0, const bf16_t* __restrict__ f1,
                                                                      const float* __restrict__ w, const float* __restrict__ g,
                                                                      const bf16_t* __restrict__ dnext, const bf16_t* __restrict__ mask,
                                                                      int HW, bf16_t* __restrict__ df1) {
  constexpr int C = 64 * CPL;
  const int n = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float gs = g[n] / (float)HW;
  float wv[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) wv[k] = w[lane * CPL + k];
  for (int px = blockIdx.x * 4 + wave; px < HW; px += gridDim.x * 4) {
    const int64_t base = ((int64_t)n * HW + px) * C + lane * CPL;
    float va[CPL], vb[CPL], sa = 0.f, sb = 0.f;
    load_run<CPL>(f0 + base, va); load_run<CPL>(f1 + base, vb);
#pragma unroll
    for (int k = 0; k < CPL; ++k) { sa += va[k] * va[k]; sb += vb[k] * vb[k]; }
    sa = wave_sum(sa); sb = wave_sum(sb);
    const float s1 = sqrtf(sb);
    const float n1 = s1 + 1e-10f;
    const float ia = 1.f / (sqrtf(sa) + 1e-10f), ib = 1.f / n1;
    // gb[c] = d d / d b_c = -2 w (a_c - b_c);  df1_k = gb_k / n1 - (sum_c gb_c f1_c) f1_k / (n1^2 s1)
    float gb[CPL], dot = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) { gb[k] = -2.f * wv[k] * (va[k] * ia - vb[k] * ib); dot += gb[k] * vb[k]; }
    dot = wave_sum(dot);
    const float coef = s1 > 0.f ? dot / (n1 * n1 * s1) : 0.f;   // torch gives NaN at an all-zero feature vector; 0 here
    float o[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) o[k] = gs * (gb[k] * ib - coef * vb[k]);
    if (dnext) {
      float dn[CPL];
      load_run<CPL>(dnext + base, dn);
#pragma unroll
      for (int k = 0; k < CPL; ++k) o[k] += dn[k];
    }
    if (mask) {
      float mk[CPL];
      if (mask == f1) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) mk[k] = vb[k];
      } else {
        load_run<CPL>(mask + base, mk);
      }
#pragma unroll
      for (int k = 0; k < CPL; ++k) o[k] = mk[k] > 0.f ? o[k] : 0.f;
    }
    store_run_rne<CPL>(df1 + base, o);
  }
}

bool lpips_c_ok(int C) { return C == 64 || C == 128 || C == 256 || C == 512; }

}  // namespace

extern "C" {

// ScalingLayer + the hand-off into the bf16 net in one pass: y bf16 [npix][8] = (x - shift[c]) / scale[c] for c < C, 0 for c >= C
int odvae_scaling_layer_bf16(const float* x, const float* shift, const float* scale, void* y, int64_t npix, int C, void* stream) {
  ODVAE_CHECK_ARG(x && shift && scale && y && npix > 0 && C > 0 && C <= 8, "scaling_layer_bf16: need 1 <= C <= 8, got %d", C);
  ODVAE_CHECK_ARG(((uintptr_t)y & 15) == 0, "scaling_layer_bf16: misaligned output");
  hipLaunchKernelGGL(scaling_layer_bf16_kernel, dim3(grid_1d(npix)), dim3(256), 0, static_cast<hipStream_t>(stream), x, shift, scale,
                     static_cast<bf16_t*>(y), npix, C);
  ODVAE_LAUNCH_CHECK("scaling_layer_bf16");
  return ODVAE_OK;
}

int odvae_relu_bwd_bf16(const void* y, const void* dy, void* dx, int64_t n, void* stream) {
  ODVAE_CHECK_ARG(y && dy && dx && n > 0 && n % 4 == 0, "relu_bwd_bf16: need n %% 4 == 0");
  ODVAE_CHECK_ARG((((uintptr_t)y | (uintptr_t)dy | (uintptr_t)dx) & 7) == 0, "relu_bwd_bf16: misaligned operand");
  hipLaunchKernelGGL(relu_bwd_bf16_kernel, dim3(grid_1d(n / 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(y), static_cast<const bf16_t*>(dy), static_cast<bf16_t*>(dx), n / 4);
  ODVAE_LAUNCH_CHECK("relu_bwd_bf16");
  return ODVAE_OK;
}

int odvae_maxpool2x2_bf16(const void* x, void* y, int N, int Hi, int Wi, int C, int Ho, int Wo, void* stream) {
  ODVAE_CHECK_ARG(x && y && N > 0 && Hi >= 2 && Wi >= 2 && C > 0 && C % 4 == 0, "maxpool2x2_bf16: need Hi, Wi >= 2 and C %% 4 == 0");
  ODVAE_CHECK_ARG(Ho == Hi / 2 && Wo == Wi / 2, "maxpool2x2_bf16: Ho/Wo must be Hi / 2, Wi / 2 (floor): got %d x %d for %d x %d", Ho, Wo, Hi, Wi);
  ODVAE_CHECK_ARG((((uintptr_t)x | (uintptr_t)y) & 7) == 0, "maxpool2x2_bf16: misaligned operand");
  hipLaunchKernelGGL(maxpool2x2_bf16_kernel, dim3(grid_1d((int64_t)N * Ho * Wo * (C / 4))), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(x), static_cast<bf16_t*>(y), N, Hi, Wi, C);
  ODVAE_LAUNCH_CHECK("maxpool2x2_bf16");
  return ODVAE_OK;
}

int odvae_maxpool2x2_bwd_bf16(const void* x, const void* dy, const void* mask, void* dx, int N, int Hi, int Wi, int C, int Ho, int Wo, void* stream) {
  ODVAE_CHECK_ARG(x && dy && dx && N > 0 && Hi >= 2 && Wi >= 2 && C > 0 && C % 4 == 0, "maxpool2x2_bwd_bf16: need Hi, Wi >= 2 and C %% 4 == 0");
  ODVAE_CHECK_ARG(Ho == Hi / 2 && Wo == Wi / 2, "maxpool2x2_bwd_bf16: Ho/Wo must be Hi / 2, Wi / 2 (floor): got %d x %d for %d x %d", Ho, Wo, Hi, Wi);
  ODVAE_CHECK_ARG((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)mask | (uintptr_t)dx) & 7) == 0, "maxpool2x2_bwd_bf16: misaligned operand");
  const int64_t cells = (int64_t)N * ((Hi + 1) / 2) * ((Wi + 1) / 2) * (C / 4);
  hipLaunchKernelGGL(maxpool2x2_bwd_bf16_kernel, dim3(grid_1d(cells)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(x), static_cast<const bf16_t*>(dy), static_cast<const bf16_t*>(mask), static_cast<bf16_t*>(dx), N, Hi, Wi, C);
  ODVAE_LAUNCH_CHECK("maxpool2x2_bwd_bf16");
  return ODVAE_OK;
}

int odvae_lpips_distance_bf16(const void* f0, const void* f1, const float* w, float* out, int N, int HW, int C,
                              void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(f0 && f1 && w && out && N > 0 && HW > 0 && lpips_c_ok(C), "lpips_distance_bf16: need C in {64, 128, 256, 512}, got %d", C);
  ODVAE_CHECK_ARG((((uintptr_t)f0 | (uintptr_t)f1) & 15) == 0, "lpips_distance_bf16: misaligned operand");
  const int nblk = (int)std::min<int64_t>(256, std::max<int64_t>(1, HW / 4));
  if (!workspace || workspace_bytes < (size_t)N * nblk * sizeof(float)) {
    odvae_set_error("lpips_distance_bf16: needs %zu workspace bytes", (size_t)N * nblk * sizeof(float));
    return ODVAE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(workspace);
  const bf16_t* a = static_cast<const bf16_t*>(f0);
  const bf16_t* b = static_cast<const bf16_t*>(f1);
  switch (C) {
    case 64:  hipLaunchKernelGGL((lpips_distance_bf16_kernel<1>), dim3(nblk, N), dim3(256), 0, st, a, b, w, HW, part); break;
    case 128: hipLaunchKernelGGL((lpips_distance_bf16_kernel<2>), dim3(nblk, N), dim3(256), 0, st, a, b, w, HW, part); break;
    case 256: hipLaunchKernelGGL((lpips_distance_bf16_kernel<4>), dim3(nblk, N), dim3(256), 0, st, a, b, w, HW, part); break;
    default:  hipLaunchKernelGGL((lpips_distance_bf16_kernel<8>), dim3(nblk, N), dim3(256), 0, st, a, b, w, HW, part); break;
  }
  hipLaunchKernelGGL(lpips_mean_final_bf16_kernel, dim3(N), dim3(64), 0, st, part, nblk, 1.f / (float)HW, out);
  ODVAE_LAUNCH_CHECK("lpips_distance_bf16");
  return ODVAE_OK;
}

int odvae_lpips_distance_bwd_bf16(const void* f0, const void* f1, const float* w, const float* g, const void* dnext, const void* mask,
                                  void* df1, int N, int HW, int C, void* stream) {
  ODVAE_CHECK_ARG(f0 && f1 && w && g && df1 && N > 0 && HW > 0 && lpips_c_ok(C), "lpips_distance_bwd_bf16: need C in {64, 128, 256, 512}, got %d", C);
  ODVAE_CHECK_ARG((((uintptr_t)f0 | (uintptr_t)f1 | (uintptr_t)dnext | (uintptr_t)mask | (uintptr_t)df1) & 15) == 0,
                  "lpips_distance_bwd_bf16: misaligned operand");
  const int nblk = (int)std::min<int64_t>(2048, std::max<int64_t>(1, HW / 4));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bf16_t* a = static_cast<const bf16_t*>(f0);
  const bf16_t* b = static_cast<const bf16_t*>(f1);
  const bf16_t* dn = static_cast<const bf16_t*>(dnext);
  const bf16_t* mk = static_cast<const bf16_t*>(mask);
  bf16_t* o = static_cast<bf16_t*>(df1);
  switch (C) {
    case 64:  hipLaunchKernelGGL((lpips_distance_bwd_bf16_kernel<1>), dim3(nblk, N), dim3(256), 0, st, a, b, w, g, dn, mk, HW, o); break;
    case 128: hipLaunchKernelGGL((lpips_distance_bwd_bf16_kernel<2>), dim3(nblk, N), dim3(256), 0, st, a, b, w, g, dn, mk, HW, o); break;
    case 256: hipLaunchKernelGGL((lpips_distance_bwd_bf16_kernel<4>), dim3(nblk, N), dim3(256), 0, st, a, b, w, g, dn, mk, HW, o); break;
    default:  hipLaunchKernelGGL((lpips_distance_bwd_bf16_kernel<8>), dim3(nblk, N), dim3(256), 0, st, a, b, w, g, dn, mk, HW, o); break;
  }
  ODVAE_LAUNCH_CHECK("lpips_distance_bwd_bf16");
  return ODVAE_OK;
}

}  // extern "C"
