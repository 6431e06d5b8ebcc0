// HBM-bound pieces of the bf16 path (BASELINE.json configs[4]): GroupNorm(32, eps 1e-6) + swish forward / backward with bf16
// activations and f32 statistics ([UPSTREAM] ldm Normalize / nonlinearity; under torch.autocast group_norm itself runs in f32, so
// "read bf16, compute f32, round once on the way out" is the same arithmetic), dtype hand-offs at the f32 ends of the network
// (input image, latent, reconstruction), the 2x2 sum-pool of the Upsample data gradient and the bias-gradient column sum.
#include "bf16_common.h"
#include "dropout_mask.h"

namespace {

#include "gn_finalize.h"

struct GnB {
  int N, HW, C, G, cpg, octs, pix_per_pass, chunks, pix_per_chunk;
};

__device__ __forceinline__ float act_grad_f(float u, bool swish) {
  if (!swish) return 1.f;
  const float sg = sigmoid_f(u);
  return sg * (1.f + u * (1.f - sg));
}
__device__ __forceinline__ void unpack8(const u32x4 v, float (&f)[8]) {
  f[0] = bf16_lo(v.x); f[1] = bf16_hi(v.x); f[2] = bf16_lo(v.y); f[3] = bf16_hi(v.y);
  f[4] = bf16_lo(v.z); f[5] = bf16_hi(v.z); f[6] = bf16_lo(v.w); f[7] = bf16_hi(v.w);
}
__device__ __forceinline__ u32x4 pack8(const float (&f)[8]) {
  u32x4 v;
  v.x = pack_bf16x2(f[0], f[1]); v.y = pack_bf16x2(f[2], f[3]); v.z = pack_bf16x2(f[4], f[5]); v.w = pack_bf16x2(f[6], f[7]);
  return v;
}

// partial [N][chunks][G][2] (sum, sum of squares), f32 per-thread sums over <= a few hundred values, LDS tree, f64 finalize
__global__ __launch_bounds__(256) void gnb_stats_kernel(const bf16_t* __restrict__ x, GnB s, float* __restrict__ partial) {
  __shared__ float red[2][256 * 8];
  const int tid = threadIdx.x, q = tid % s.octs, psub = tid / s.octs;
  const int n = blockIdx.y, chunk = blockIdx.x;
  const int p_beg = chunk * s.pix_per_chunk, p_end = min(s.HW, p_beg + s.pix_per_chunk);
  float sm[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (psub < s.pix_per_pass) {
    const bf16_t* xn = x + (int64_t)n * s.HW * s.C + 8 * q;
    int px = p_beg + psub;
    for (; px + 3 * s.pix_per_pass < p_end; px += 4 * s.pix_per_pass) {     // four 16-byte loads in flight per thread
      const u32x4 v0 = *reinterpret_cast<const u32x4*>(xn + (int64_t)px * s.C);
      const u32x4 v1 = *reinterpret_cast<const u32x4*>(xn + (int64_t)(px + s.pix_per_pass) * s.C);
      const u32x4 v2 = *reinterpret_cast<const u32x4*>(xn + (int64_t)(px + 2 * s.pix_per_pass) * s.C);
      const u32x4 v3 = *reinterpret_cast<const u32x4*>(xn + (int64_t)(px + 3 * s.pix_per_pass) * s.C);
      float a[8], b[8], c[8], d[8];
      unpack8(v0, a); unpack8(v1, b); unpack8(v2, c); unpack8(v3, d);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        sm[j] += (a[j] + b[j]) + (c[j] + d[j]);
        sq[j] += (a[j] * a[j] + b[j] * b[j]) + (c[j] * c[j] + d[j] * d[j]);
      }
    }
    for (; px < p_end; px += s.pix_per_pass) {
      float a[8];
      unpack8(*reinterpret_cast<const u32x4*>(xn + (int64_t)px * s.C), a);
#pragma unroll
      for (int j = 0; j < 8; ++j) { sm[j] += a[j]; sq[j] += a[j] * a[j]; }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[0][psub * s.C + 8 * q + j] = sm[j]; red[1][psub * s.C + 8 * q + j] = sq[j]; }
  }
  __syncthreads();
  for (int c = tid; c < s.C; c += 256) {
    float a = 0.f, b = 0.f;
    for (int ps = 0; ps < s.pix_per_pass; ++ps) { a += red[0][ps * s.C + c]; b += red[1][ps * s.C + c]; }
    red[0][c] = a; red[1][c] = b;
  }
  __syncthreads();
  if (tid < s.G) {
    float a = 0.f, b = 0.f;
    for (int j = 0; j < s.cpg; ++j) { a += red[0][tid * s.cpg + j]; b += red[1][tid * s.cpg + j]; }
    float* o = partial + (((int64_t)n * s.chunks + chunk) * s.G + tid) * 2;
    o[0] = a; o[1] = b;
  }
}

struct Oct { float g[8], b[8], mu[8], rs[8], ds1[8], ds2[8]; };
__device__ __forceinline__ void load_oct(const GnB& s, int n, int q, const float* gamma, const float* beta, const float* mean,
                                         const float* rstd, const float* grp, Oct& k) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = 8 * q + j, g = c / s.cpg;
    k.g[j] = gamma[c]; k.b[j] = beta[c];
    k.mu[j] = mean[n * s.G + g]; k.rs[j] = rstd[n * s.G + g];
    if (grp) { k.ds1[j] = grp[((int64_t)n * s.G + g) * 2]; k.ds2[j] = grp[((int64_t)n * s.G + g) * 2 + 1]; }
  }
}

// grid (blocks, N); a thread keeps one channel octet (256 % octs == 0), so the affine constants are loop-invariant registers
// streaming accesses (`nt`): every byte of these passes is touched once here and next by another kernel a gigabyte later; measured on the
// f32 twins -4 % (backward apply) / -6 % (forward apply) per launch
typedef unsigned int gnb_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 ldnt(const u32x4* p) { return __builtin_nontemporal_load(reinterpret_cast<const gnb_u4*>(p)); }
__device__ __forceinline__ void stnt(u32x4* p, u32x4 v) { __builtin_nontemporal_store(v, reinterpret_cast<gnb_u4*>(p)); }

// ResnetBlock dropout (dropout_mask.h): a 16-byte load is exactly one octet, so a thread makes one Philox call per load.  The DROP = false
// instantiations of the three kernels (D = GnNoDrop, an empty last argument) have the instruction streams they had before the dropout existed.
template <bool DROP, typename D>
__device__ __forceinline__ void drop8(float (&a)[8], const D& d, int64_t oct) {
  if constexpr (DROP) {
    // contract(off): products of their own, rounded to f32 -- never contracted into an fma with the sum they feed (the identity form's
    // `b += du`), so that the backward on dy equals the plain backward on a rounded dy * keep * scale
#pragma clang fp contract(off)
    float m[8];
    gn_drop_octet(d, oct, m);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] *= m[j];
  }
}

// DROP: y = keep * scale * act(u), multiplied in f32 before the single rounding
template <bool DROP = false, typename D = GnNoDrop>
__global__ __launch_bounds__(256) void gnb_apply_kernel(const bf16_t* __restrict__ x, GnB s, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, int swish, bf16_t* __restrict__ y, D d) {
  const int n = blockIdx.y, per_n = s.HW * s.octs;
  const int64_t o0 = (int64_t)n * per_n;      // index of the sample's first octet in the tensor
  const u32x4* xn = reinterpret_cast<const u32x4*>(x) + (int64_t)n * per_n;
  u32x4* yn = reinterpret_cast<u32x4*>(y) + (int64_t)n * per_n;
  const int stride = gridDim.x * 256;
  Oct k;
  load_oct(s, n, threadIdx.x % s.octs, gamma, beta, mean, rstd, nullptr, k);
  auto f = [&](const u32x4 v, int at) {
    float a[8];
    unpack8(v, a);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float u = (a[j] - k.mu[j]) * k.rs[j] * k.g[j] + k.b[j];
      a[j] = swish ? swish_f(u) : u;
    }
    drop8<DROP>(a, d, o0 + at);
    return pack8(a);
  };
  int i = blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < per_n; i += 4 * stride) {
    const u32x4 v0 = ldnt(xn + i), v1 = ldnt(xn + i + stride), v2 = ldnt(xn + i + 2 * stride), v3 = ldnt(xn + i + 3 * stride);
    stnt(yn + i, f(v0, i)); stnt(yn + i + stride, f(v1, i + stride)); stnt(yn + i + 2 * stride, f(v2, i + 2 * stride)); stnt(yn + i + 3 * stride, f(v3, i + 3 * stride));
  }
  for (; i < per_n; i += stride) stnt(yn + i, f(ldnt(xn + i), i));
}

// partial [N][chunks][2][C]: per channel sums of du*xhat and du over the chunk's pixels.  DROP: dy_eff = dy * keep * scale first (f32, not
// rounded), the rest runs on it unchanged
template <bool DROP = false, typename D = GnNoDrop>
__global__ __launch_bounds__(256) void gnb_bwd_reduce_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, GnB s,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd, int swish,
                                                             float* __restrict__ partial, D d) {
  __shared__ float red[2][256 * 8];
  const int tid = threadIdx.x, q = tid % s.octs, psub = tid / s.octs;
  const int n = blockIdx.y, chunk = blockIdx.x;
  const int p_beg = chunk * s.pix_per_chunk, p_end = min(s.HW, p_beg + s.pix_per_chunk);
  if (psub < s.pix_per_pass) {
    Oct k;
    load_oct(s, n, q, gamma, beta, mean, rstd, nullptr, k);
    float a[8] = {0, 0, 0, 0, 0, 0, 0, 0}, b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t base = (int64_t)n * s.HW * s.C + 8 * q;
    auto accum = [&](const u32x4 xv, const u32x4 dv, int px) {
      float xi[8], di[8];
      unpack8(xv, xi); unpack8(dv, di);
      drop8<DROP>(di, d, ((int64_t)n * s.HW + px) * s.octs + q);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xh = (xi[j] - k.mu[j]) * k.rs[j];
        const float du = di[j] * act_grad_f(xh * k.g[j] + k.b[j], swish);
        a[j] += du * xh; b[j] += du;
      }
    };
    int px = p_beg + psub;
    for (; px + s.pix_per_pass < p_end; px += 2 * s.pix_per_pass) {         // four 16-byte loads in flight per thread
      const u32x4 x0 = ldnt(reinterpret_cast<const u32x4*>(x + base + (int64_t)px * s.C));
      const u32x4 d0 = ldnt(reinterpret_cast<const u32x4*>(dy + base + (int64_t)px * s.C));
      const u32x4 x1 = ldnt(reinterpret_cast<const u32x4*>(x + base + (int64_t)(px + s.pix_per_pass) * s.C));
      const u32x4 d1 = ldnt(reinterpret_cast<const u32x4*>(dy + base + (int64_t)(px + s.pix_per_pass) * s.C));
      accum(x0, d0, px);
      accum(x1, d1, px + s.pix_per_pass);
    }
    for (; px < p_end; px += s.pix_per_pass)
      accum(*reinterpret_cast<const u32x4*>(x + base + (int64_t)px * s.C), *reinterpret_cast<const u32x4*>(dy + base + (int64_t)px * s.C), px);
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[0][psub * s.C + 8 * q + j] = a[j]; red[1][psub * s.C + 8 * q + j] = b[j]; }
  }
  __syncthreads();
  float* o = partial + ((int64_t)n * s.chunks + chunk) * 2 * s.C;
  for (int cc = tid; cc < s.C; cc += 256) {
    float sa = 0.f, sb = 0.f;
    for (int ps = 0; ps < s.pix_per_pass; ++ps) { sa += red[0][ps * s.C + cc]; sb += red[1][ps * s.C + cc]; }
    o[cc] = sa; o[s.C + cc] = sb;
  }
}

// dx = rstd * (du*gamma - (ds2 + xhat*ds1)/m) (+ the skip connection's gradient, folded in)
template <bool DROP = false, typename D = GnNoDrop>
__global__ __launch_bounds__(256) void gnb_bwd_apply_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, GnB s,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ grp, int swish, const bf16_t* __restrict__ dx_add,
                                                            bf16_t* __restrict__ dx, D d) {
  const int n = blockIdx.y, per_n = s.HW * s.octs;
  const int64_t o0 = (int64_t)n * per_n;
  const u32x4* xn = reinterpret_cast<const u32x4*>(x) + (int64_t)n * per_n;
  const u32x4* dn = reinterpret_cast<const u32x4*>(dy) + (int64_t)n * per_n;
  const u32x4* an = dx_add ? reinterpret_cast<const u32x4*>(dx_add) + (int64_t)n * per_n : nullptr;
  u32x4* on = reinterpret_cast<u32x4*>(dx) + (int64_t)n * per_n;
  const float inv_m = 1.f / ((float)s.HW * (float)s.cpg);
  const int stride = gridDim.x * 256;
  Oct k;
  load_oct(s, n, threadIdx.x % s.octs, gamma, beta, mean, rstd, grp, k);
  auto f = [&](const u32x4 xv, const u32x4 dv, int at) {
    float xi[8], di[8], ad[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unpack8(xv, xi); unpack8(dv, di);
    if (an) unpack8(ldnt(an + at), ad);
    drop8<DROP>(di, d, o0 + at);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xh = (xi[j] - k.mu[j]) * k.rs[j];
      const float du = di[j] * act_grad_f(xh * k.g[j] + k.b[j], swish);
      xi[j] = k.rs[j] * (du * k.g[j] - (k.ds2[j] + xh * k.ds1[j]) * inv_m) + ad[j];
    }
    return pack8(xi);
  };
  int i = blockIdx.x * 256 + threadIdx.x;
  for (; i + stride < per_n; i += 2 * stride) {
    const u32x4 x0 = ldnt(xn + i), x1 = ldnt(xn + i + stride), d0 = ldnt(dn + i), d1 = ldnt(dn + i + stride);
    stnt(on + i, f(x0, d0, i)); stnt(on + i + stride, f(x1, d1, i + stride));
  }
  for (; i < per_n; i += stride) stnt(on + i, f(ldnt(xn + i), ldnt(dn + i), i));
}

bool make_shape(int N, int HW, int C, int G, GnB& s) {
  if (N <= 0 || HW <= 0 || C <= 0 || G <= 0 || C % G != 0 || C % 8 != 0) return false;
  s.N = N; s.HW = HW; s.C = C; s.G = G; s.cpg = C / G; s.octs = C / 8;
  if (s.octs > 256 || 256 % s.octs != 0 || G > 256 || (int64_t)HW * s.octs >= ((int64_t)1 << 31) || N > 65535) return false;
  s.pix_per_pass = 256 / s.octs;
  int chunks = ceil_div(2048, N);
  const int max_chunks = ceil_div(HW, 64);
  if (chunks > max_chunks) chunks = max_chunks;
  if (chunks < 1) chunks = 1;
  s.pix_per_chunk = ceil_div(HW, chunks);
  s.chunks = ceil_div(HW, s.pix_per_chunk);
  return true;
}
int apply_blocks(const GnB& s) { return (int)std::min<int64_t>(std::max<int64_t>(ceil_div64((int64_t)s.HW * s.octs, 256 * 8), 1), 65535); }

// drop == nullptr launches exactly what the plain entry points always launched
void launch_gnb_apply(const GnB& s, hipStream_t st, const bf16_t* x, const float* gamma, const float* beta, const float* mean,
                      const float* rstd, int swish, bf16_t* y, const GnDrop* drop) {
  if (drop) hipLaunchKernelGGL((gnb_apply_kernel<true, GnDrop>), dim3(apply_blocks(s), s.N), dim3(256), 0, st, x, s, gamma, beta, mean, rstd, swish, y, *drop);
  else      hipLaunchKernelGGL((gnb_apply_kernel<>), dim3(apply_blocks(s), s.N), dim3(256), 0, st, x, s, gamma, beta, mean, rstd, swish, y, GnNoDrop{});
}

int gnb_drop_args(const char* who, double p) {      // (C % 8 == 0 is part of every bf16 GroupNorm shape)
  ODVAE_CHECK_ARG(p >= 0.0 && p <= 1.0, "%s: dropout probability has to be between 0 and 1, got %g", who, p);
  return ODVAE_OK;
}

int gnb_fwd_impl(const char* who, const void* x, int N, int HW, int C, int G, const float* gamma, const float* beta, float eps, int swish,
                 void* y, float* mean, float* rstd, void* workspace, size_t workspace_bytes, void* stream, const GnDrop* drop) {
  GnB s;
  ODVAE_CHECK_ARG(make_shape(N, HW, C, G, s), "%s: unsupported shape N=%d HW=%d C=%d G=%d (need C%%G==0, C%%8==0, 256%%(C/8)==0)", who, N, HW, C, G);
  ODVAE_CHECK_ARG(x && gamma && beta && y && mean && rstd, "%s: null operand", who);
  ODVAE_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0, "%s: operands must be 16-byte aligned", who);
  const size_t need = (size_t)N * s.chunks * G * 2 * sizeof(float);
  if (!workspace || workspace_bytes < need) {
    odvae_set_error("%s: needs %zu workspace bytes, got %zu", who, need, workspace_bytes);
    return ODVAE_ERR_WORKSPACE;
  }
  unsigned* recentred = odvae_gn_recentred_counter();
  ODVAE_CHECK_ARG(recentred, "%s: cannot find the recentring counter on the device", who);
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(workspace);
  hipLaunchKernelGGL(gnb_stats_kernel, dim3(s.chunks, N), dim3(256), 0, st, static_cast<const bf16_t*>(x), s, partial);
  hipLaunchKernelGGL((gn_finalize_kernel<GnB, bf16_t>), dim3(ceil_div(N * G, 4)), dim3(256), 0, st, partial, static_cast<const bf16_t*>(x), s, eps, mean, rstd, recentred);
  launch_gnb_apply(s, st, static_cast<const bf16_t*>(x), gamma, beta, mean, rstd, swish, static_cast<bf16_t*>(y), drop);
  ODVAE_LAUNCH_CHECK(who);
  return ODVAE_OK;
}

int gnb_fwd_partials_impl(const char* who, const void* x, int N, int HW, int C, int G, const float* gamma, const float* beta, float eps, int swish,
                          void* y, float* mean, float* rstd, const float* partial, int chunks, void* stream, const GnDrop* drop) {
  GnB s;
  ODVAE_CHECK_ARG(make_shape(N, HW, C, G, s), "%s: unsupported shape N=%d HW=%d C=%d G=%d", who, N, HW, C, G);
  ODVAE_CHECK_ARG(x && gamma && beta && y && mean && rstd && partial && chunks > 0, "%s: null operand", who);
  ODVAE_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)partial & 7) == 0, "%s: misaligned operand", who);
  unsigned* recentred = odvae_gn_recentred_counter();
  ODVAE_CHECK_ARG(recentred, "%s: cannot find the recentring counter on the device", who);
  hipStream_t st = static_cast<hipStream_t>(stream);
  GnB sf = s;
  sf.chunks = chunks;
  hipLaunchKernelGGL((gn_finalize_kernel<GnB, bf16_t>), dim3(ceil_div(N * G, 4)), dim3(256), 0, st, partial, static_cast<const bf16_t*>(x), sf, eps, mean, rstd, recentred);
  launch_gnb_apply(s, st, static_cast<const bf16_t*>(x), gamma, beta, mean, rstd, swish, static_cast<bf16_t*>(y), drop);
  ODVAE_LAUNCH_CHECK(who);
  return ODVAE_OK;
}

int gnb_apply_impl(const char* who, const void* x, int N, int HW, int C, int G, const float* gamma, const float* beta,
                   const float* mean, const float* rstd, int swish, void* y, void* stream, const GnDrop* drop) {
  GnB s;
  ODVAE_CHECK_ARG(make_shape(N, HW, C, G, s), "%s: unsupported shape N=%d HW=%d C=%d G=%d", who, N, HW, C, G);
  ODVAE_CHECK_ARG(x && gamma && beta && y && mean && rstd, "%s: null operand", who);
  ODVAE_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0, "%s: misaligned operand", who);
  launch_gnb_apply(s, static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(x), gamma, beta, mean, rstd, swish, static_cast<bf16_t*>(y), drop);
  ODVAE_LAUNCH_CHECK(who);
  return ODVAE_OK;
}

// ---- dtype hand-offs ---------------------------------------------------------------------------------------------------------
// y[row][0..CP) bf16 = x[row][0..C) f32, zero for c >= C   (CP % 8 == 0)
__global__ void cast_pad_kernel(const float* __restrict__ x, int64_t rows, int C, int CP, bf16_t* __restrict__ y) {
  const int octs = CP / 8;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * octs; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / octs;
    const int c0 = (int)(i % octs) * 8;
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = c0 + j < C ? x[r * C + c0 + j] : 0.f;
    *reinterpret_cast<u32x4*>(y + r * CP + c0) = pack8(f);
  }
}
__global__ void cast_f32_kernel(const bf16_t* __restrict__ x, int64_t n8, float* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    float f[8];
    unpack8(*reinterpret_cast<const u32x4*>(x + 8 * i), f);
    *reinterpret_cast<float4*>(y + 8 * i) = make_float4(f[0], f[1], f[2], f[3]);
    *reinterpret_cast<float4*>(y + 8 * i + 4) = make_float4(f[4], f[5], f[6], f[7]);
  }
}
// dx[n][y][x][c] = sum of the 2x2 block of du (data gradient of nearest-2x upsampling)
__global__ void sumpool2x2_bf16_kernel(const bf16_t* __restrict__ du, bf16_t* __restrict__ dx, int N, int H, int W, int C) {
  const int octs = C / 8;
  const int64_t total = (int64_t)N * H * W * octs;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int q = (int)(i % octs);
    int64_t r = i / octs;
    const int xx = (int)(r % W); r /= W;
    const int yy = (int)(r % H); const int n = (int)(r / H);
    const bf16_t* src = du + (((int64_t)n * 2 * H + 2 * yy) * 2 * W + 2 * xx) * C + 8 * q;
    float a[8], b[8], c[8], d[8];
    unpack8(*reinterpret_cast<const u32x4*>(src), a);
    unpack8(*reinterpret_cast<const u32x4*>(src + C), b);
    unpack8(*reinterpret_cast<const u32x4*>(src + (int64_t)2 * W * C), c);
    unpack8(*reinterpret_cast<const u32x4*>(src + (int64_t)2 * W * C + C), d);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = (a[j] + b[j]) + (c[j] + d[j]);
    *reinterpret_cast<u32x4*>(dx + 8 * i) = pack8(a);
  }
}
// dx = dy * (y > 0 ? 1 : slope) given the POST-activation y (slope > 0: y has the sign of the pre-activation); V = 8 (vec8) or 1 per thread
template <int V>
__global__ __launch_bounds__(256) void lrelu_bwd_bf16_kernel(const bf16_t* __restrict__ y, const bf16_t* __restrict__ dy, bf16_t* __restrict__ dx,
                                                             float slope, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i * V < n; i += (int64_t)gridDim.x * blockDim.x) {
    float yv[V], gv[V], ov[V];
    load_run<V>(y + i * V, yv);
    load_run<V>(dy + i * V, gv);
#pragma unroll
    for (int j = 0; j < V; ++j) ov[j] = gv[j] * (yv[j] > 0.f ? 1.f : slope);
    store_run_rne<V>(dx + i * V, ov);
  }
}
// ---- conv-less resamplers on bf16 activations: f32 arithmetic, one rounding on the way out; the statistics are those of the rounded values ----
struct RsBF16 {
  typedef bf16_t elem_t;
  static constexpr int W = 8;
  static __device__ __forceinline__ void load(const bf16_t* p, float (&f)[8]) { unpack8(ldnt(reinterpret_cast<const u32x4*>(p)), f); }
  static __device__ __forceinline__ void store(bf16_t* p, float (&f)[8]) {
    const u32x4 v = pack8(f);
    stnt(reinterpret_cast<u32x4*>(p), v);
    unpack8(v, f);
  }
};
#include "resample.h"

// partial[block][C] column sums of a [rows][C] bf16 matrix; second kernel adds the blocks in order
__global__ __launch_bounds__(256) void colsum_bf16_kernel(const bf16_t* __restrict__ x, int64_t rows, int C, int rows_per_block, float* __restrict__ partial) {
  __shared__ float red[256 * 8];
  const int octs = C / 8, tid = threadIdx.x, q = tid % octs, psub = tid / octs, ppp = 256 / octs;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(rows, r0 + rows_per_block);
  float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (psub < ppp)
    for (int64_t r = r0 + psub; r < r1; r += ppp) {
      float a[8];
      unpack8(*reinterpret_cast<const u32x4*>(x + r * C + 8 * q), a);
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += a[j];
    }
  if (psub < ppp)
#pragma unroll
    for (int j = 0; j < 8; ++j) red[psub * C + 8 * q + j] = s[j];
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float a = 0.f;
    for (int ps = 0; ps < ppp; ++ps) a += red[ps * C + c];
    partial[(int64_t)blockIdx.x * C + c] = a;
  }
}
// one wave per channel: lanes stride over the blocks, fixed-order tree (deterministic)
__global__ void colsum_finish_kernel(const float* __restrict__ partial, int blocks, int C, float* __restrict__ out) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= C) return;
  float a = 0.f;
  for (int b = lane; b < blocks; b += 64) a += partial[(int64_t)b * C + c];
  a = wave_sum(a);
  if (lane == 0) out[c] = a;
}

int colsum_blocks(int64_t rows) { return (int)std::min<int64_t>(512, std::max<int64_t>(1, ceil_div64(rows, 512))); }

}  // namespace

extern "C" {

size_t odvae_groupnorm_bf16_workspace_bytes(int N, int HW, int C, int G) {
  GnB s;
  if (!make_shape(N, HW, C, G, s)) return 0;
  const size_t fwd = (size_t)N * s.chunks * G * 2;
  const size_t bwd = (size_t)N * s.chunks * 2 * C + (size_t)N * 2 * C + (size_t)N * G * 2;
  return (fwd > bwd ? fwd : bwd) * sizeof(float);
}

// y = act(GroupNorm(x)), x / y bf16 [N][HW][C]; gamma / beta f32; mean / rstd f32 [N][G] saved for the backward
int odvae_groupnorm_fwd_bf16(const void* x, int N, int HW, int C, int G, const float* gamma, const float* beta, float eps, int swish,
                             void* y, float* mean, float* rstd, void* workspace, size_t workspace_bytes, void* stream) {
  return gnb_fwd_impl("groupnorm_fwd_bf16", x, N, HW, C, G, gamma, beta, eps, swish, y, mean, rstd, workspace, workspace_bytes, stream, nullptr);
}

// The dropout form (odvae_groupnorm_fwd_drop_f32's twin): y = round(keep * scale * act(GroupNorm(x))), the mask of dropout_mask.h from (seed, p)
int odvae_groupnorm_fwd_drop_bf16(const void* x, int N, int HW, int C, int G, const float* gamma, const float* beta, float eps, int swish,
                                  double p, unsigned long long seed, void* y, float* mean, float* rstd,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  if (const int rc = gnb_drop_args("groupnorm_fwd_drop_bf16", p)) return rc;
  const GnDrop d = make_gn_drop(p, seed);
  return gnb_fwd_impl("groupnorm_fwd_drop_bf16", x, N, HW, C, G, gamma, beta, eps, swish, y, mean, rstd, workspace, workspace_bytes, stream, &d);
}

// The same without the statistics pass: partial [N][chunks][G][2] = (sum, sum of squares) of x per chunk and channel group as the conv
// that produced x left them (odvae_conv_bf16_stats: one chunk per output tile).  finalize (f64, fixed order over the chunks) + apply.
int odvae_groupnorm_fwd_partials_bf16(const void* x, int N, int HW, int C, int G, const float* gamma, const float* beta, float eps, int swish,
                                      void* y, float* mean, float* rstd, const float* partial, int chunks, void* stream) {
  return gnb_fwd_partials_impl("groupnorm_fwd_partials_bf16", x, N, HW, C, G, gamma, beta, eps, swish, y, mean, rstd, partial, chunks, stream, nullptr);
}

int odvae_groupnorm_fwd_partials_drop_bf16(const void* x, int N, int HW, int C, int G, const float* gamma, const float* beta, float eps, int swish,
                                           double p, unsigned long long seed, void* y, float* mean, float* rstd,
                                           const float* partial, int chunks, void* stream) {
  if (const int rc = gnb_drop_args("groupnorm_fwd_partials_drop_bf16", p)) return rc;
  const GnDrop d = make_gn_drop(p, seed);
  return gnb_fwd_partials_impl("groupnorm_fwd_partials_drop_bf16", x, N, HW, C, G, gamma, beta, eps, swish, y, mean, rstd, partial, chunks, stream, &d);
}

// The apply pass alone with mean / rstd given (odvae_groupnorm_apply_f32's bf16 twin)
int odvae_groupnorm_apply_bf16(const void* x, int N, int HW, int C, int G, const float* gamma, const float* beta,
                               const float* mean, const float* rstd, int swish, void* y, void* stream) {
  return gnb_apply_impl("groupnorm_apply_bf16", x, N, HW, C, G, gamma, beta, mean, rstd, swish, y, stream, nullptr);
}

int odvae_groupnorm_apply_drop_bf16(const void* x, int N, int HW, int C, int G, const float* gamma, const float* beta,
                                    const float* mean, const float* rstd, int swish, double p, unsigned long long seed, void* y, void* stream) {
  if (const int rc = gnb_drop_args("groupnorm_apply_drop_bf16", p)) return rc;
  const GnDrop d = make_gn_drop(p, seed);
  return gnb_apply_impl("groupnorm_apply_drop_bf16", x, N, HW, C, G, gamma, beta, mean, rstd, swish, y, stream, &d);
}

// dx bf16 (+ dx_add bf16, the folded skip gradient, or NULL), dgamma / dbeta f32 [C]
static int gnb_bwd_impl(const void* x, const void* dy, int N, int HW, int C, int G, const float* gamma, const float* beta,
                        const float* mean, const float* rstd, int swish, void* dx, float* dgamma, float* dbeta, const void* dx_add,
                        void* workspace, size_t workspace_bytes, void* stream, const GnDrop* drop) {
  GnB s;
  ODVAE_CHECK_ARG(make_shape(N, HW, C, G, s), "groupnorm_bwd_bf16: unsupported shape N=%d HW=%d C=%d G=%d", N, HW, C, G);
  ODVAE_CHECK_ARG(x && dy && gamma && beta && mean && rstd && dx && dgamma && dbeta, "groupnorm_bwd_bf16: null operand");
  ODVAE_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)dy & 15) == 0 && ((uintptr_t)dx & 15) == 0 && ((uintptr_t)dx_add & 15) == 0,
                  "groupnorm_bwd_bf16: operands must be 16-byte aligned");
  const size_t need = odvae_groupnorm_bf16_workspace_bytes(N, HW, C, G);
  if (!workspace || workspace_bytes < need) {
    odvae_set_error("groupnorm_bwd_bf16: needs %zu workspace bytes, got %zu", need, workspace_bytes);
    return ODVAE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(workspace);
  float* chan = partial + (size_t)N * s.chunks * 2 * C;
  float* grp = chan + (size_t)N * 2 * C;
  const bf16_t* xb = static_cast<const bf16_t*>(x);
  const bf16_t* db = static_cast<const bf16_t*>(dy);
  if (drop) hipLaunchKernelGGL((gnb_bwd_reduce_kernel<true, GnDrop>), dim3(s.chunks, N), dim3(256), 0, st, xb, db, s, gamma, beta, mean, rstd, swish, partial, *drop);
  else      hipLaunchKernelGGL((gnb_bwd_reduce_kernel<>), dim3(s.chunks, N), dim3(256), 0, st, xb, db, s, gamma, beta, mean, rstd, swish, partial, GnNoDrop{});
  if (s.cpg <= 64) hipLaunchKernelGGL(gn_bwd_finalize_kernel<GnB>, dim3(N, ceil_div(C, (64 / s.cpg) * s.cpg)), dim3(256), 0, st, partial, s, gamma, chan, grp);
  else hipLaunchKernelGGL(gn_bwd_finalize_wide_kernel<GnB>, dim3(N), dim3(256), 2 * C * sizeof(float), st, partial, s, gamma, chan, grp);
  hipLaunchKernelGGL(gn_bwd_param_kernel, dim3(ceil_div(C, 64)), dim3(256), 0, st, chan, N, C, dgamma, dbeta);
  if (drop) hipLaunchKernelGGL((gnb_bwd_apply_kernel<true, GnDrop>), dim3(apply_blocks(s), N), dim3(256), 0, st, xb, db, s, gamma, beta, mean, rstd, grp, swish,
                               static_cast<const bf16_t*>(dx_add), static_cast<bf16_t*>(dx), *drop);
  else      hipLaunchKernelGGL((gnb_bwd_apply_kernel<>), dim3(apply_blocks(s), N), dim3(256), 0, st, xb, db, s, gamma, beta, mean, rstd, grp, swish,
                               static_cast<const bf16_t*>(dx_add), static_cast<bf16_t*>(dx), GnNoDrop{});
  ODVAE_LAUNCH_CHECK("groupnorm_bwd_bf16");
  return ODVAE_OK;
}

int odvae_groupnorm_bwd_bf16(const void* x, const void* dy, int N, int HW, int C, int G, const float* gamma, const float* beta,
                             const float* mean, const float* rstd, int swish, void* dx, float* dgamma, float* dbeta, const void* dx_add,
                             void* workspace, size_t workspace_bytes, void* stream) {
  return gnb_bwd_impl(x, dy, N, HW, C, G, gamma, beta, mean, rstd, swish, dx, dgamma, dbeta, dx_add, workspace, workspace_bytes, stream, nullptr);
}

// Backward of the dropout forms: dy_eff = dy * keep * scale in f32 (the mask re-made from the forward call's seed and p), then
// odvae_groupnorm_bwd_bf16's arithmetic on dy_eff
int odvae_groupnorm_bwd_drop_bf16(const void* x, const void* dy, int N, int HW, int C, int G, const float* gamma, const float* beta,
                                  const float* mean, const float* rstd, int swish, double p, unsigned long long seed,
                                  void* dx, float* dgamma, float* dbeta, const void* dx_add,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  if (const int rc = gnb_drop_args("groupnorm_bwd_drop_bf16", p)) return rc;
  const GnDrop d = make_gn_drop(p, seed);
  return gnb_bwd_impl(x, dy, N, HW, C, G, gamma, beta, mean, rstd, swish, dx, dgamma, dbeta, dx_add, workspace, workspace_bytes, stream, &d);
}

// y bf16 [rows][CP] = x f32 [rows][C], zero-padded channels (CP >= C, CP % 8 == 0): the f32 -> bf16 hand-off (input image,
// latent, reconstruction gradient; CP > C gives 3-channel tensors the 16-byte channel vectors the conv kernels read)
int odvae_cast_pad_bf16(const float* x, int64_t rows, int C, int CP, void* y, void* stream) {
  ODVAE_CHECK_ARG(x && y && rows > 0 && C > 0 && CP >= C && CP % 8 == 0, "cast_pad_bf16: bad arguments (rows=%lld C=%d CP=%d)", (long long)rows, C, CP);
  ODVAE_CHECK_ARG(((uintptr_t)y & 15) == 0, "cast_pad_bf16: y must be 16-byte aligned");
  const int64_t work = rows * (CP / 8);
  hipLaunchKernelGGL(cast_pad_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(work, 256), 8192)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), x, rows, C, CP, static_cast<bf16_t*>(y));
  ODVAE_LAUNCH_CHECK("cast_pad_bf16");
  return ODVAE_OK;
}

int odvae_cast_f32_from_bf16(const void* x, int64_t n, float* y, void* stream) {
  ODVAE_CHECK_ARG(x && y && n > 0 && n % 8 == 0, "cast_f32_from_bf16: n = %lld must be a positive multiple of 8", (long long)n);
  ODVAE_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0, "cast_f32_from_bf16: operands must be 16-byte aligned");
  hipLaunchKernelGGL(cast_f32_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(n / 8, 256), 8192)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(x), n / 8, y);
  ODVAE_LAUNCH_CHECK("cast_f32_from_bf16");
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

// dx [N][H][W][C] = 2x2 sum-pool of du [N][2H][2W][C] (bf16): data gradient of F.interpolate(scale 2, nearest)
int odvae_upsample2x_bwd_bf16(const void* du, void* dx, int N, int H, int W, int C, void* stream) {
  ODVAE_CHECK_ARG(du && dx && N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "upsample2x_bwd_bf16: bad arguments");
  const int64_t work = (int64_t)N * H * W * (C / 8);
  hipLaunchKernelGGL(sumpool2x2_bf16_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(work, 256), 16384)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(du), static_cast<bf16_t*>(dx), N, H, W, C);
  ODVAE_LAUNCH_CHECK("upsample2x_bwd_bf16");
  return ODVAE_OK;
}

// The bf16 forms of odvae_avgpool2x2_f32 / _bwd_f32 / odvae_upsample2x_f32 (C % 8 == 0): f32 arithmetic, one rounding on the way out;
// gn_partial holds the statistics of the bf16-rounded values, as odvae_conv_bf16_stats leaves them
int odvae_avgpool2x2_bf16(const void* x, void* y, int N, int H, int W, int C, float* gn_partial, int gn_groups, int chunks, void* stream) {
  return rs_avgpool<RsBF16>(x, y, N, H, W, C, gn_partial, gn_groups, chunks, stream);
}

int odvae_avgpool2x2_bwd_bf16(const void* dy, void* dx, int N, int H, int W, int C, void* stream) {
  return rs_avgpool_bwd<RsBF16>(dy, dx, N, H, W, C, stream);
}

int odvae_upsample2x_bf16(const void* x, void* u, int N, int H, int W, int C, float* gn_partial, int gn_groups, int chunks, void* stream) {
  return rs_upsample<RsBF16>(x, u, N, H, W, C, gn_partial, gn_groups, chunks, stream);
}

size_t odvae_colsum_bf16_workspace_bytes(int64_t rows, int C) { return (size_t)colsum_blocks(rows) * C * sizeof(float); }

// out f32 [C] = column sums of x bf16 [rows][C] (bias gradients); deterministic
int odvae_colsum_bf16(const void* x, int64_t rows, int C, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && out && rows > 0 && C > 0 && C % 8 == 0 && C / 8 <= 256, "colsum_bf16: unsupported shape rows=%lld C=%d (C %% 8 == 0, C <= 2048)", (long long)rows, C);
  const int blocks = colsum_blocks(rows);
  if (!workspace || workspace_bytes < (size_t)blocks * C * sizeof(float)) {
    odvae_set_error("colsum_bf16: needs %zu workspace bytes, got %zu", (size_t)blocks * C * sizeof(float), workspace_bytes);
    return ODVAE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* partial = static_cast<float*>(workspace);
  hipLaunchKernelGGL(colsum_bf16_kernel, dim3(blocks), dim3(256), 0, st, static_cast<const bf16_t*>(x), rows, C, (int)ceil_div64(rows, blocks), partial);
  hipLaunchKernelGGL(colsum_finish_kernel, dim3(ceil_div(C, 4)), dim3(256), 0, st, partial, blocks, C, out);
  ODVAE_LAUNCH_CHECK("colsum_bf16");
  return ODVAE_OK;
}

}  // extern "C"
