// Device-side latent noise (model.params.device_noise): the seeded fill and the latent stage as one launch each way.
// The draws are latent_noise.h's pure function of (key, global step, tag, element index): nothing random is uploaded, and the backward
// makes its draws again from the same words instead of reading saved tensors.
//
// Fused stage, forward:   z = ((mean + std * eps) * m + noise) + add
// bit for bit what the chain gaussian_sample -> latent_combine(mask) -> latent_combine(add = noise) -> latent_combine(add = enc_pose) of
// elementwise.hip gives when it is fed the fill's tensors for the same words: the same operations in the same order, one rounding each.
// What that chain's kernels compile to decides the order: gaussian_sample_kernel's `mu + expf(0.5f * lv) * eps` is one fused
// multiply-add, latent_combine's product and sums are launches of their own (never fused), and gaussian_bwd_kernel's dz branch is
// dmu = 0 + g, dlv = 0 + ((g * eps) * 0.5) * e with every product rounded (the 0 + turns a -0 into +0, which a dropped element's
// gradient is).  hipcc contracts by default and __fmul_rn / __fadd_rn do not stop it (elementwise.hip, ema_one): the separately rounded
// operations are plain operators under `#pragma clang fp contract(off)`, the one fused operation is written as fmaf.
#include "common.h"
#include "latent_noise.h"

namespace {

enum { LS_SAMPLE = 1, LS_DROPOUT = 2, LS_NOISE = 4 };

__device__ __forceinline__ unsigned ls_tag(const LnDraw& d, unsigned stream) { return (stream << 29) | d.tag; }

__device__ __forceinline__ float ls_clamped_logvar(float lraw) { return fminf(fmaxf(lraw, -30.f), 20.f); }

// one element of the forward: z0 = fma(e, eps, mu) | mu;  z1 = z0 * m;  z2 = z1 + noise;  z3 = z2 + add
__device__ __forceinline__ float ls_forward_one(float mu, float lraw, float eps, float m, float noise, float add, int flags, bool has_add) {
#pragma clang fp contract(off)
  float v = mu;
  if (flags & LS_SAMPLE) v = fmaf(expf(0.5f * ls_clamped_logvar(lraw)), eps, mu);
  if (flags & LS_DROPOUT) v = v * m;
  if (flags & LS_NOISE) v = v + noise;
  if (has_add) v = v + add;
  return v;
}

// one element of the backward: g = dz * m;  dmu = 0 + g;  dlogvar = 0 + ((g * eps) * 0.5) * std inside the clamp, 0 outside.
// Mode instead of sample: z0 is the mean itself, so dmu = g and dlogvar = 0.
__device__ __forceinline__ void ls_backward_one(float lraw, float dz, float eps, float m, int flags, float& dmu, float& dlv) {
#pragma clang fp contract(off)
  float g = dz;
  if (flags & LS_DROPOUT) g = g * m;
  if (flags & LS_SAMPLE) {
    const bool pass = lraw >= -30.f && lraw <= 20.f;  // d clamp / d x
    const float e = expf(0.5f * ls_clamped_logvar(lraw));
    const float t = g * eps * 0.5f * e;
    dmu = 0.f + g;
    dlv = pass ? 0.f + t : 0.f;
  } else {
    dmu = g;
    dlv = 0.f;
  }
}

// out[e], e in [0, n): element `first + e` of the stream in d.tag.  One thread per quad of the stream, so an unaligned `first` and a last
// quad that is partly used cost nothing special: a thread stores the lanes that fall inside [first, first + n).
template <int KIND>
__global__ __launch_bounds__(256) void ln_fill_kernel(float* __restrict__ out, int64_t n, int64_t first, const LnDraw d) {
  const int64_t g0 = first >> 2, nq = ((first + n - 1) >> 2) - g0 + 1;
  const int64_t lead = first & 3;      // lanes of quad g0 before `first`
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    float x[4];
    if (KIND == LN_KIND_NORMAL) ln_normal_quad(d, d.tag, g0 + q, x);
    else ln_dropout_quad(d, d.tag, g0 + q, x);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t e = 4 * q + j - lead;
      if (e >= 0 && e < n) out[e] = x[j];
    }
  }
}

// mom: NHWC [npix][2 Cz]; add (may be null), z: [npix][Cz].  One thread per quad of z's flat index (any Cz: a quad may span two pixels,
// and the last one may be partly used).
__global__ __launch_bounds__(256) void latent_stage_kernel(const float* __restrict__ mom, const float* __restrict__ add, float* __restrict__ z,
                                                           int64_t npix, int Cz, int flags, const LnDraw d) {
  const int64_t total = npix * Cz, nq = (total + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    float eps[4] = {0.f, 0.f, 0.f, 0.f}, m[4] = {0.f, 0.f, 0.f, 0.f}, nz[4] = {0.f, 0.f, 0.f, 0.f};
    if (flags & LS_SAMPLE) ln_normal_quad(d, ls_tag(d, LN_STREAM_EPS), q, eps);
    if (flags & LS_DROPOUT) ln_dropout_quad(d, ls_tag(d, LN_STREAM_DROPOUT), q, m);
    if (flags & LS_NOISE) ln_normal_quad(d, ls_tag(d, LN_STREAM_NOISE), q, nz);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t idx = 4 * q + j;
      if (idx < total) {
        const int c = (int)(idx % Cz); const int64_t px = idx / Cz;
        const float mu = mom[px * 2 * Cz + c];
        const float lraw = (flags & LS_SAMPLE) ? mom[px * 2 * Cz + Cz + c] : 0.f;
        z[idx] = ls_forward_one(mu, lraw, eps[j], m[j], nz[j], add ? add[idx] : 0.f, flags, add != nullptr);
      }
    }
  }
}

// dmom from mom and dz alone: eps and m are drawn again
__global__ __launch_bounds__(256) void latent_stage_bwd_kernel(const float* __restrict__ mom, const float* __restrict__ dz, float* __restrict__ dmom,
                                                               int64_t npix, int Cz, int flags, const LnDraw d) {
  const int64_t total = npix * Cz, nq = (total + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    float eps[4] = {0.f, 0.f, 0.f, 0.f}, m[4] = {0.f, 0.f, 0.f, 0.f};
    if (flags & LS_SAMPLE) ln_normal_quad(d, ls_tag(d, LN_STREAM_EPS), q, eps);
    if (flags & LS_DROPOUT) ln_dropout_quad(d, ls_tag(d, LN_STREAM_DROPOUT), q, m);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t idx = 4 * q + j;
      if (idx < total) {
        const int c = (int)(idx % Cz); const int64_t px = idx / Cz;
        const float lraw = (flags & LS_SAMPLE) ? mom[px * 2 * Cz + Cz + c] : 0.f;
        float dmu, dlv;
        ls_backward_one(lraw, dz[idx], eps[j], m[j], flags, dmu, dlv);
        dmom[px * 2 * Cz + c] = dmu;
        dmom[px * 2 * Cz + Cz + c] = dlv;
      }
    }
  }
}

// Blocks of the fused stage: a thread makes up to three Philox calls and eight transcendentals per quad, so 2048 blocks of 256 (eight per
// compute unit) keep the device busy and the grid-stride loop takes the rest.
constexpr int kStageBlocks = 2048;

bool ln_words_ok(uint64_t step_word, uint64_t tag, double p) { return step_word <= 0xFFFFFFFFull && tag <= 0xFFFFFFFFull && p >= 0.0 && p <= 1.0; }

}  // namespace

extern "C" {

int odvae_noise_fill_f32(float* out, int64_t n, uint64_t first, uint64_t seed, uint64_t step_word, uint64_t tag, int kind, double p, void* stream) {
  ODVAE_CHECK_ARG(out && n > 0 && first < (1ull << 62) && n < (1ll << 62), "noise_fill: bad arguments");
  ODVAE_CHECK_ARG(ln_words_ok(step_word, tag, p), "noise_fill: step word and tag are 32-bit words, p lies in [0, 1]");
  ODVAE_CHECK_ARG(kind == LN_KIND_NORMAL || kind == LN_KIND_DROPOUT, "noise_fill: kind is 0 (normal) or 1 (dropout multiplier), got %d", kind);
  const LnDraw d = make_ln_draw(seed, (unsigned)step_word, (unsigned)tag, p);
  const int64_t nq = (int64_t)((first + (uint64_t)n - 1) >> 2) - (int64_t)(first >> 2) + 1;
  if (kind == LN_KIND_NORMAL)
    hipLaunchKernelGGL((ln_fill_kernel<LN_KIND_NORMAL>), dim3(grid_1d(nq)), dim3(256), 0, static_cast<hipStream_t>(stream), out, n, (int64_t)first, d);
  else
    hipLaunchKernelGGL((ln_fill_kernel<LN_KIND_DROPOUT>), dim3(grid_1d(nq)), dim3(256), 0, static_cast<hipStream_t>(stream), out, n, (int64_t)first, d);
  ODVAE_LAUNCH_CHECK("noise_fill");
  return ODVAE_OK;
}

int odvae_latent_stage_f32(const float* moments, const float* add, float* z, int N, int HW, int Cz, uint64_t seed, uint64_t step_word, uint64_t tag,
                           int flags, double p, void* stream) {
  ODVAE_CHECK_ARG(moments && z && N > 0 && HW > 0 && Cz > 0 && (flags & ~7) == 0, "latent_stage: bad arguments");
  ODVAE_CHECK_ARG(ln_words_ok(step_word, tag, p) && (tag >> 29) == 0, "latent_stage: step word and tag are 32-bit words, the tag's stream bits are the kernel's, p lies in [0, 1]");
  const LnDraw d = make_ln_draw(seed, (unsigned)step_word, (unsigned)tag, p);
  const int64_t npix = (int64_t)N * HW;
  hipLaunchKernelGGL(latent_stage_kernel, dim3(grid_1d((npix * Cz + 3) / 4, kStageBlocks)), dim3(256), 0, static_cast<hipStream_t>(stream), moments, add, z, npix, Cz, flags, d);
  ODVAE_LAUNCH_CHECK("latent_stage");
  return ODVAE_OK;
}

int odvae_latent_stage_bwd_f32(const float* moments, const float* dz, float* dmoments, int N, int HW, int Cz, uint64_t seed, uint64_t step_word,
                               uint64_t tag, int flags, double p, void* stream) {
  ODVAE_CHECK_ARG(moments && dz && dmoments && N > 0 && HW > 0 && Cz > 0 && (flags & ~7) == 0, "latent_stage_bwd: bad arguments");
  ODVAE_CHECK_ARG(ln_words_ok(step_word, tag, p) && (tag >> 29) == 0, "latent_stage_bwd: step word and tag are 32-bit words, the tag's stream bits are the kernel's, p lies in [0, 1]");
  const LnDraw d = make_ln_draw(seed, (unsigned)step_word, (unsigned)tag, p);
  const int64_t npix = (int64_t)N * HW;
  hipLaunchKernelGGL(latent_stage_bwd_kernel, dim3(grid_1d((npix * Cz + 3) / 4, kStageBlocks)), dim3(256), 0, static_cast<hipStream_t>(stream), moments, dz, dmoments, npix, Cz, flags, d);
  ODVAE_LAUNCH_CHECK("latent_stage_bwd");
  return ODVAE_OK;
}

}  // extern "C"
