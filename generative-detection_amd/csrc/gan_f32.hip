// PatchGAN discriminator support kernels, NHWC f32, gfx950.  All HBM-bound.
//
// [UPSTREAM] taming/modules/discriminator/model.py NLayerDiscriminator (reference call sites
// src/modules/losses/contperceptual.py:285,355-356): Conv2d(4x4, stride 2|1, pad 1) -> BatchNorm2d -> LeakyReLU(0.2).
// The 4x4 convolutions run as im2col + the f32 MFMA GEMM (gemm_f32.hip) -- BASELINE.json's north_star allows the matrix
// cores for "im2col dense contractions"; 288 GB of HBM makes the column matrices (<= 1 GB at B = 32) a non-issue.
//   fwd   cols = im2col(x)           y    = cols . W'^T     (W' = weight reordered to [Cout][kh][kw][Cin])
//   dgrad dcols = dy . W'            dx   = col2im(dcols)   (gather form: no atomics, deterministic)
//   wgrad dW'  = dy^T . cols
// BatchNorm2d / ActNorm + LeakyReLU, f32 and bf16: gan_norm.hip.
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
