// Linear attention ([UPSTREAM] ldm/modules/attention.py LinearAttention, heads = 1, dim_head = C) for gfx950, f32, NHWC.
//
//   k' = softmax(k over the T tokens, per (image, channel));  ctx[d][e] = sum_n k'[n][d] v[n][e];  out[n][e] = sum_d ctx[d][e] q[n][d]
//
// Tokens are rows of the packed [N][T][3C] projection (pixel stride ld = 3C); q, k, v are its channel thirds.  This file holds what the
// GEMM entry point cannot do: the column statistics of k, the context product with exp(k - m) applied on the way into the matrix core,
// and the backward for k and v.  out = q ctx, dctx = q^T dOut and dq = dOut ctx^T are odvae_gemm_f32 calls, g[d] = ctx[d] . dctx[d] is
// odvae_rowdot_f32 (ops.py _LinearAttention).  Softmaxed k never reaches HBM and nothing of size T x T exists.
//
// Matrix core: v_mfma_f32_32x32x2_f32 (common.h mfma32).  Lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31], so
//   * in the context product (depth T) a wave's A operand is 2 token rows x 32 channels of k and its B operand 2 token rows x 32
//     channels of v: both are contiguous 128-byte row pieces read straight into the operand registers, no LDS;
//   * in the backward (depth C) the A operand's lanes are tokens: each lane reads 4 consecutive channels of its own row (16 bytes) and
//     spends them on 4 MFMA steps; lane half h takes channels 8g + 4h + j in step j, and the B operand follows the same order.
// Every reduction has a fixed order: no atomics anywhere, two runs give the same bits.
#include "common.h"

namespace {

constexpr int CTX_SPLIT = 1024;    // tokens per workgroup of the context product (odvae_linattn_ctx_split())
constexpr int STAT_SPLIT = 512;    // tokens per workgroup of the column statistics
constexpr float NEG_BIG = -3.0e38f;

__device__ __forceinline__ void online_merge(float& m, float& l, float m2, float l2) {
  const float mn = fmaxf(m, m2);
  l = l * expf(m - mn) + l2 * expf(m2 - mn);
  m = mn;
}

// ---- 1. column statistics --------------------------------------------------------------------------------------------------------
// grid (C / 32, nsplit, N), 256 threads = 32 channel lanes x 8 row lanes: every row read is 128 contiguous bytes.
// part [N][nsplit][C][2] = (max, sum exp(k - max)) of the split's rows.
__global__ __launch_bounds__(256) void linattn_colstats_partial_kernel(const float* __restrict__ k, int ld, int64_t stride, int T, int C,
                                                                        int nsplit, float* __restrict__ part) {
  __shared__ float sm[8][32], sl[8][32];
  const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cx, s = blockIdx.y, n = blockIdx.z;
  const int t0 = s * STAT_SPLIT, t1 = min(T, t0 + STAT_SPLIT);
  const float* kp = k + (int64_t)n * stride + c;
  float m = NEG_BIG, l = 0.f;
  for (int t = t0 + ry; t < t1; t += 8) {
    const float x = kp[(int64_t)t * ld];
    if (x > m) { l = l * expf(m - x) + 1.f; m = x; }
    else l += expf(x - m);
  }
  sm[ry][cx] = m; sl[ry][cx] = l;
  __syncthreads();
  if (ry == 0) {
#pragma unroll
    for (int i = 1; i < 8; ++i) online_merge(m, l, sm[i][cx], sl[i][cx]);
    float* o = part + (((int64_t)n * nsplit + s) * C + c) * 2;
    o[0] = m; o[1] = l;
  }
}

// one thread per (image, channel): the splits in order -> m, 1 / l
__global__ void linattn_colstats_final_kernel(const float* __restrict__ part, int C, int nsplit, int total, float* __restrict__ mx,
                                              float* __restrict__ rinv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int n = i / C, c = i - n * C;
  float m = NEG_BIG, l = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float* p = part + (((int64_t)n * nsplit + s) * C + c) * 2;
    online_merge(m, l, p[0], p[1]);
  }
  mx[i] = m;
  rinv[i] = 1.f / l;
}

// ---- 2. context product ----------------------------------------------------------------------------------------------------------
// grid ((C / 32)^2, nsplit, N), one wave per workgroup: the 32 x 32 tile (dt, et) of sum_{n in split} exp(k[n][d] - m[d]) v[n][e].
// part [N][nsplit][C][C]
__global__ __launch_bounds__(64) void linattn_ctx_partial_kernel(const float* __restrict__ k, const float* __restrict__ v, int ld,
                                                                  int64_t stride, const float* __restrict__ mx, int T, int C, int nsplit,
                                                                  float* __restrict__ part) {
  const int lane = threadIdx.x, col = lane & 31, half = lane >> 5;
  const int tiles = C >> 5;
  const int dt = blockIdx.x / tiles, et = blockIdx.x - dt * tiles, s = blockIdx.y, n = blockIdx.z;
  const int t0 = s * CTX_SPLIT, t1 = min(T, t0 + CTX_SPLIT);
  const float* kp = k + (int64_t)n * stride + dt * 32 + col;
  const float* vp = v + (int64_t)n * stride + et * 32 + col;
  const float m = mx[(int64_t)n * C + dt * 32 + col];
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  int t = t0;
  for (; t + 16 <= t1; t += 16) {               // whole chunks of 16 tokens: 16 loads in flight, then 8 exp, then 8 MFMA steps
    float a[8], b[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t off = (int64_t)(t + 2 * u + half) * ld;
      a[u] = kp[off];
      b[u] = vp[off];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] = expf(a[u] - m);
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = mfma32(a[u], b[u], acc);
  }
  if (t < t1) {                                 // the ragged last chunk
    float a[8], b[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int row = t + 2 * u + half;
      const int rc = min(row, t1 - 1);          // rows past the split read its last row and count as zero
      a[u] = kp[(int64_t)rc * ld];
      b[u] = vp[(int64_t)rc * ld];
      const bool ok = row < t1;
      a[u] = ok ? expf(a[u] - m) : 0.f;
      b[u] = ok ? b[u] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = mfma32(a[u], b[u], acc);
  }
  float* o = part + (((int64_t)n * nsplit + s) * C + dt * 32) * C + et * 32 + col;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[(int64_t)acc_row(r, lane) * C] = acc[r];
}

// ctx[n][d][e] = (sum_s part[n][s][d][e], s ascending) / l[n][d]
__global__ void linattn_ctx_reduce_kernel(const float* __restrict__ part, const float* __restrict__ rinv, int C, int nsplit, int64_t total,
                                          float* __restrict__ ctx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int64_t cc = (int64_t)C * C;
  const int64_t n = i / cc, de = i - n * cc;
  const int d = (int)(de / C);
  float sum = 0.f;
  for (int s = 0; s < nsplit; ++s) sum += part[(n * nsplit + s) * cc + de];
  ctx[i] = sum * rinv[n * C + d];
}

// ---- 5. backward for k and v -----------------------------------------------------------------------------------------------------
// s = exp(k - m) / l;  dv[n][e] = sum_d s[n][d] dctx[d][e];  dk[n][d] = s[n][d] (sum_e v[n][e] dctx[d][e] - g[d])
// grid (ceil(T / 32), ceil(2 (C / 32) / 4), N), 4 waves: each wave one 32-token x 32-channel tile of dv (jobs 0 .. C/32 - 1) or of dk
// (the rest).  The four waves of a workgroup share the token rows; no LDS, no barrier.
__global__ __launch_bounds__(256) void linattn_dkv_kernel(const float* __restrict__ k, const float* __restrict__ v, int ld, int64_t stride,
                                                           const float* __restrict__ mx, const float* __restrict__ rinv,
                                                           const float* __restrict__ dctx, const float* __restrict__ g,
                                                           float* __restrict__ dk, float* __restrict__ dv, int ldo, int64_t stride_o,
                                                           int T, int C) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, half = lane >> 5;
  const int tiles = C >> 5;
  const int job = blockIdx.y * 4 + wave;
  if (job >= 2 * tiles) return;
  const int n = blockIdx.z, row0 = blockIdx.x * 32;
  const bool is_dk = job >= tiles;
  const int ot = is_dk ? job - tiles : job;
  const int ar = min(row0 + col, T - 1);                       // this lane's token as an A operand row (clamped: never stored past T)
  const float* dc = dctx + (int64_t)n * C * C;
  const float* mn = mx + (int64_t)n * C;
  const float* rn = rinv + (int64_t)n * C;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  if (!is_dk) {
    const float* arow = k + (int64_t)n * stride + (int64_t)ar * ld;
    const float* bcol = dc + ot * 32 + col;
    for (int d0 = 0; d0 < C; d0 += 8) {
      const int dd = d0 + 4 * half;
      const float4 kk = *reinterpret_cast<const float4*>(arow + dd);
      const float4 mm = *reinterpret_cast<const float4*>(mn + dd);
      const float4 ri = *reinterpret_cast<const float4*>(rn + dd);
      const float a0 = expf(kk.x - mm.x) * ri.x, a1 = expf(kk.y - mm.y) * ri.y, a2 = expf(kk.z - mm.z) * ri.z, a3 = expf(kk.w - mm.w) * ri.w;
      const float b0 = bcol[(int64_t)(dd + 0) * C], b1 = bcol[(int64_t)(dd + 1) * C], b2 = bcol[(int64_t)(dd + 2) * C], b3 = bcol[(int64_t)(dd + 3) * C];
      acc = mfma32(a0, b0, acc);
      acc = mfma32(a1, b1, acc);
      acc = mfma32(a2, b2, acc);
      acc = mfma32(a3, b3, acc);
    }
    float* o = dv + (int64_t)n * stride_o + ot * 32 + col;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row0 + acc_row(r, lane);
      if (row < T) o[(int64_t)row * ldo] = acc[r];
    }
  } else {
    const float* arow = v + (int64_t)n * stride + (int64_t)ar * ld;
    const float* brow = dc + (int64_t)(ot * 32 + col) * C;
    for (int e0 = 0; e0 < C; e0 += 8) {
      const int ee = e0 + 4 * half;
      const float4 vv = *reinterpret_cast<const float4*>(arow + ee);
      const float4 bb = *reinterpret_cast<const float4*>(brow + ee);
      acc = mfma32(vv.x, bb.x, acc);
      acc = mfma32(vv.y, bb.y, acc);
      acc = mfma32(vv.z, bb.z, acc);
      acc = mfma32(vv.w, bb.w, acc);
    }
    const int c = ot * 32 + col;
    const float m = mn[c], ri = rn[c], gc = g[(int64_t)n * C + c];
    const float* kc = k + (int64_t)n * stride + c;
    float* o = dk + (int64_t)n * stride_o + c;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row0 + acc_row(r, lane);
      if (row < T) {
        const float sv = expf(kc[(int64_t)row * ld] - m) * ri;
        o[(int64_t)row * ldo] = sv * (acc[r] - gc);
      }
    }
  }
}

inline int stat_splits(int T) { return ceil_div(T, STAT_SPLIT); }
inline int ctx_splits(int T) { return ceil_div(T, CTX_SPLIT); }

inline bool shape_ok(const char* what, int N, int T, int C) {
  if (N < 1 || N > 65535 || T < 1 || C < 32 || C % 32 != 0 || ceil_div(T, 32) > 0x7FFFFFF || ctx_splits(T) > 65535 || stat_splits(T) > 65535) {
    odvae_set_error("%s: needs 1 <= N <= 65535, T >= 1, C a positive multiple of 32 (N=%d T=%d C=%d)", what, N, T, C);
    return false;
  }
  return true;
}

}  // namespace

extern "C" {

int odvae_linattn_ctx_split(void) { return CTX_SPLIT; }

size_t odvae_linattn_colstats_workspace_bytes(int N, int T, int C) {
  if (N < 1 || T < 1 || C < 1) return 0;
  return (size_t)N * stat_splits(T) * C * 2 * sizeof(float);
}

int odvae_linattn_colstats_f32(const float* k, int ld, int64_t stride, int N, int T, int C, float* mx, float* rinv,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!shape_ok("linattn_colstats", N, T, C)) return ODVAE_ERR_ARG;
  ODVAE_CHECK_ARG(k && mx && rinv && workspace, "linattn_colstats: null pointer");
  ODVAE_CHECK_ARG(ld >= C && stride >= (int64_t)(T - 1) * ld + C, "linattn_colstats: ld %d / stride %lld too small for T=%d C=%d", ld, (long long)stride, T, C);
  const size_t need = odvae_linattn_colstats_workspace_bytes(N, T, C);
  if (workspace_bytes < need) {
    odvae_set_error("linattn_colstats: workspace %zu < %zu bytes", workspace_bytes, need);
    return ODVAE_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int ns = stat_splits(T);
  float* part = (float*)workspace;
  hipLaunchKernelGGL(linattn_colstats_partial_kernel, dim3(C / 32, ns, N), dim3(256), 0, st, k, ld, stride, T, C, ns, part);
  ODVAE_LAUNCH_CHECK("linattn_colstats_partial");
  const int total = N * C;
  hipLaunchKernelGGL(linattn_colstats_final_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, st, part, C, ns, total, mx, rinv);
  ODVAE_LAUNCH_CHECK("linattn_colstats_final");
  return ODVAE_OK;
}

size_t odvae_linattn_ctx_workspace_bytes(int N, int T, int C) {
  if (N < 1 || T < 1 || C < 1) return 0;
  return (size_t)N * ctx_splits(T) * C * C * sizeof(float);
}

int odvae_linattn_ctx_f32(const float* k, const float* v, int ld, int64_t stride, const float* mx, const float* rinv, int N, int T, int C,
                          float* ctx, void* workspace, size_t workspace_bytes, void* stream) {
  if (!shape_ok("linattn_ctx", N, T, C)) return ODVAE_ERR_ARG;
  ODVAE_CHECK_ARG(k && v && mx && rinv && ctx && workspace, "linattn_ctx: null pointer");
  ODVAE_CHECK_ARG(ld >= C && stride >= (int64_t)(T - 1) * ld + C, "linattn_ctx: ld %d / stride %lld too small for T=%d C=%d", ld, (long long)stride, T, C);
  ODVAE_CHECK_ARG((C / 32) * (C / 32) <= 0x7FFFFFF, "linattn_ctx: C %d too large", C);
  const size_t need = odvae_linattn_ctx_workspace_bytes(N, T, C);
  if (workspace_bytes < need) {
    odvae_set_error("linattn_ctx: workspace %zu < %zu bytes", workspace_bytes, need);
    return ODVAE_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int ns = ctx_splits(T);
  float* part = (float*)workspace;
  hipLaunchKernelGGL(linattn_ctx_partial_kernel, dim3((C / 32) * (C / 32), ns, N), dim3(64), 0, st, k, v, ld, stride, mx, T, C, ns, part);
  ODVAE_LAUNCH_CHECK("linattn_ctx_partial");
  const int64_t total = (int64_t)N * C * C;
  ODVAE_CHECK_ARG(ceil_div64(total, 256) <= 0x7FFFFFFF, "linattn_ctx: N C^2 too large");
  hipLaunchKernelGGL(linattn_ctx_reduce_kernel, dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, st, part, rinv, C, ns, total, ctx);
  ODVAE_LAUNCH_CHECK("linattn_ctx_reduce");
  return ODVAE_OK;
}

int odvae_linattn_dkv_f32(const float* k, const float* v, int ld, int64_t stride, const float* mx, const float* rinv, const float* dctx,
                          const float* g, int N, int T, int C, float* dk, float* dv, int ldo, int64_t stride_o, void* stream) {
  if (!shape_ok("linattn_dkv", N, T, C)) return ODVAE_ERR_ARG;
  ODVAE_CHECK_ARG(k && v && mx && rinv && dctx && g && dk && dv, "linattn_dkv: null pointer");
  ODVAE_CHECK_ARG(ld >= C && stride >= (int64_t)(T - 1) * ld + C && ldo >= C && stride_o >= (int64_t)(T - 1) * ldo + C,
                  "linattn_dkv: leading dimensions / strides too small for T=%d C=%d", T, C);
  ODVAE_CHECK_ARG(ld % 4 == 0 && stride % 4 == 0, "linattn_dkv: ld and stride must be multiples of 4 floats");
  ODVAE_CHECK_ARG((((uintptr_t)k | (uintptr_t)v | (uintptr_t)mx | (uintptr_t)rinv | (uintptr_t)dctx) & 15) == 0,
                  "linattn_dkv: k, v, m, 1/l and dctx must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(linattn_dkv_kernel, dim3(ceil_div(T, 32), ceil_div(2 * (C / 32), 4), N), dim3(256), 0, st, k, v, ld, stride, mx, rinv,
                     dctx, g, dk, dv, ldo, stride_o, T, C);
  ODVAE_LAUNCH_CHECK("linattn_dkv");
  return ODVAE_OK;
}

}  // extern "C"
