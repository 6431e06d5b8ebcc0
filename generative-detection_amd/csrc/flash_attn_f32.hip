// Fused single-head attention forward + backward in f32, gfx950: softmax(q k^T * scale) v of [UPSTREAM] AttnBlock.forward with the
// T x T scores kept on the CU (the f32 GEMM path, gemm_f32.hip + ops._Attention, writes P [N][T][T] to HBM and keeps it for the backward).
//
// Input is the packed projection qkv f32 [N][T][3C] (q | k | v); outputs o f32 [N][T][C] and lse2 f32 [N][T] = log2 sum_j exp(s_ij * scale),
// the base-2 log-sum-exp of the scaled scores with the same meaning as in flash_attn_bf16.hip.  C = D in {64, 128, 256, 512}, any T >= 1.
//
// Every product runs on the exact-f32 matrix core, v_mfma_f32_16x16x4_f32 (an fmaf chain, one rounding per product).  Its operands are one
// f32 per lane: A[i = l&15][k = l>>4], B[k = l>>4][j = l&15]; result register r of lane l is D[row = 4 (l>>4) + r][col = l&15].
// A wave owns 16 rows of the stationary side (16 query rows in the forward and dQ kernels, 16 keys in the dK/dV kernel) and streams the
// other side in tiles of 32 rows straight from global memory (L1 / L2 hits: the 4 waves of a block walk the same rows).  The channel
// dimension of the score products is taken 16 at a time as float4 loads: lane group g = l>>4 holds channels 4g .. 4g+3 and MFMA step e
// uses channel 4g + e, a permutation of the 16 that both operands share.
//
// Forward / dQ: scores are formed transposed, S^T = K Q^T, so the query sits on the lane: the probability tile is directly the B operand
// of O^T += V^T P^T (and dQ^T += K^T dS^T); row max / sum are register reductions plus two lane exchanges (lane^16, lane^32).
// dK / dV: S = Q K^T and dP = dO V^T put the key on the lane, so P and dS feed dV^T += dO^T P and dK^T += Q^T dS directly.
// Accumulators are C/4 registers per lane per output; at C = 512 dK and dV do not fit together and run as two launches of the same kernel.
// No atomics: every output element is written by exactly one lane, so two runs give identical bits.
#include "common.h"

namespace {

constexpr int WAVE_ROWS = 16;              // stationary rows per wave
constexpr int WAVES = 4;                   // waves per block
constexpr int BLOCK_ROWS = WAVE_ROWS * WAVES;
constexpr int TILE = 32;                   // streamed rows per step (two 16-row MFMA tiles)
constexpr float LOG2E = 1.4426950408889634f;

struct FlashF32P {
  const float* qkv;     // [N][T][3C]
  const float* o;       // [N][T][C]   backward: forward output
  const float* d_o;     // [N][T][C]   backward
  float* out;           // forward: o [N][T][C]; backward: dqkv [N][T][3C]
  float* lse2;          // [N][T]
  const float* delta;   // [N][T]      backward: rowsum(dO * O)
  int T;
  float scale;
};

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
#else
  (void)a; (void)b; return c;
#endif
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// reduction over the four lane groups that hold the same column (lanes j, j+16, j+32, j+48)
__device__ __forceinline__ float col_max(float x) {
  x = fmaxf(x, __shfl_xor(x, 16));
  return fmaxf(x, __shfl_xor(x, 32));
}
__device__ __forceinline__ float col_sum(float x) {
  x += __shfl_xor(x, 16);
  return x + __shfl_xor(x, 32);
}

// acc[u] += A_rows[u] . B_row over C channels: A row (l&15) of tile u, B row (l&15); both row pointers already offset by this lane's 4g.
template <int C>
__device__ __forceinline__ void score_pair(const float* a0, const float* a1, const float* b, f32x4& s0, f32x4& s1) {
#pragma unroll 4
  for (int t = 0; t < C / 16; ++t) {
    const f32x4 bv = ld4(b + 16 * t), av0 = ld4(a0 + 16 * t), av1 = ld4(a1 + 16 * t);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s0 = mfma16(av0[e], bv[e], s0);
      s1 = mfma16(av1[e], bv[e], s1);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Forward: grid (ceil(T / 64), N), 256 threads; wave w owns queries q0 .. q0+15.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void flash_f32_fwd_kernel(FlashF32P p) {
  const int T = p.T, lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * BLOCK_ROWS + (threadIdx.x >> 6) * WAVE_ROWS;
  if (q0 >= T) return;
  const int64_t img = (int64_t)blockIdx.y * T;
  const float* base = p.qkv + img * 3 * C;
  const int q = min(q0 + j, T - 1);
  const float* qrow = base + (int64_t)q * 3 * C + 4 * g;
  const float sc = p.scale * LOG2E;

  f32x4 acc[C / 16];
#pragma unroll
  for (int d = 0; d < C / 16; ++d) acc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;   // running maximum (base-2 scaled) of query j; this lane's part of the running sum

  for (int kt = 0; kt < T; kt += TILE) {
    f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    score_pair<C>(base + (int64_t)min(kt + j, T - 1) * 3 * C + C + 4 * g, base + (int64_t)min(kt + 16 + j, T - 1) * 3 * C + C + 4 * g,
                  qrow, s[0], s[1]);
    // s[u][r]: score of query j against key kt + 16u + 4g + r
    float mt = -INFINITY;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[u][r] = kt + 16 * u + 4 * g + r < T ? s[u][r] * sc : -INFINITY;
        mt = fmaxf(mt, s[u][r]);
      }
    const float mn = fmaxf(m, col_max(mt));     // finite: key kt is always in range
    const float alpha = exp2f(m - mn);
    m = mn;
    float ls = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[u][r] = exp2f(s[u][r] - mn);
        ls += s[u][r];
      }
    l = l * alpha + ls;
    // O^T[d][query] += V^T[d][key] P^T[key][query]; lane (j, g) supplies V[key 16u + 4g + r][16 dt + j] and P^T[that key][query j]
    const float* vrow[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) vrow[u][r] = base + (int64_t)min(kt + 16 * u + 4 * g + r, T - 1) * 3 * C + 2 * C + j;
#pragma unroll
    for (int dt = 0; dt < C / 16; ++dt) {
      f32x4 a = acc[dt] * alpha;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) a = mfma16(vrow[u][r][16 * dt], s[u][r], a);
      acc[dt] = a;
    }
  }
  l = col_sum(l);
  if (q0 + j < T) {
    const float inv = 1.f / l;
    float* orow = p.out + (img + q0 + j) * C + 4 * g;
#pragma unroll
    for (int dt = 0; dt < C / 16; ++dt) st4(orow + 16 * dt, acc[dt] * inv);   // register r: channel 16 dt + 4g + r
    if (g == 0) p.lse2[img + q0 + j] = m + log2f(l);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// dQ: query-stationary, grid (ceil(T / 64), N).  dQ = scale * dS K, dS = P .* (dO V^T - delta), P = exp2(s * scale * log2e - lse2).
// ---------------------------------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void flash_f32_dq_kernel(FlashF32P p) {
  const int T = p.T, lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * BLOCK_ROWS + (threadIdx.x >> 6) * WAVE_ROWS;
  if (q0 >= T) return;
  const int64_t img = (int64_t)blockIdx.y * T;
  const float* base = p.qkv + img * 3 * C;
  const int q = min(q0 + j, T - 1);
  const float* qrow = base + (int64_t)q * 3 * C + 4 * g;
  const float* dorow = p.d_o + (img + q) * C + 4 * g;
  const float sc = p.scale * LOG2E, lse = p.lse2[img + q], dl = p.delta[img + q];

  f32x4 acc[C / 16];
#pragma unroll
  for (int c = 0; c < C / 16; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kt = 0; kt < T; kt += TILE) {
    const int64_t k0 = (int64_t)min(kt + j, T - 1) * 3 * C + 4 * g, k1 = (int64_t)min(kt + 16 + j, T - 1) * 3 * C + 4 * g;
    f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    f32x4 dp[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    score_pair<C>(base + k0 + C, base + k1 + C, qrow, s[0], s[1]);          // S^T = K Q^T
    score_pair<C>(base + k0 + 2 * C, base + k1 + 2 * C, dorow, dp[0], dp[1]);  // dP^T = V dO^T
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pr = kt + 16 * u + 4 * g + r < T ? exp2f(s[u][r] * sc - lse) : 0.f;
        s[u][r] = pr * (dp[u][r] - dl);                                      // dS^T[key][query j]
      }
    const float* krow[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) krow[u][r] = base + (int64_t)min(kt + 16 * u + 4 * g + r, T - 1) * 3 * C + C + j;
#pragma unroll
    for (int ct = 0; ct < C / 16; ++ct) {
      f32x4 a = acc[ct];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) a = mfma16(krow[u][r][16 * ct], s[u][r], a);
      acc[ct] = a;
    }
  }
  if (q0 + j < T) {
    float* dqrow = p.out + (img + q0 + j) * 3 * C + 4 * g;
#pragma unroll
    for (int ct = 0; ct < C / 16; ++ct) st4(dqrow + 16 * ct, acc[ct] * p.scale);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// dK / dV: key-stationary, grid (ceil(T / 64), N); wave w owns keys k0 .. k0+15.  dV = P^T dO, dK = scale * dS^T Q.
// DK / DV select the outputs (C = 512: one launch each, the two accumulators do not fit together).
// ---------------------------------------------------------------------------------------------------------------------------------
template <int C, bool DK, bool DV>
__global__ __launch_bounds__(256) void flash_f32_dkv_kernel(FlashF32P p) {
  const int T = p.T, lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int k0 = blockIdx.x * BLOCK_ROWS + (threadIdx.x >> 6) * WAVE_ROWS;
  if (k0 >= T) return;
  const int64_t img = (int64_t)blockIdx.y * T;
  const float* base = p.qkv + img * 3 * C;
  const float* dob = p.d_o + img * C;
  const float* keyrow = base + (int64_t)min(k0 + j, T - 1) * 3 * C + 4 * g;
  const float sc = p.scale * LOG2E;

  f32x4 ak[DK ? C / 16 : 1], av[DV ? C / 16 : 1];
#pragma unroll
  for (int c = 0; c < C / 16; ++c) {
    if (DK) ak[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (DV) av[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  for (int qt = 0; qt < T; qt += TILE) {
    const int qa = min(qt + j, T - 1), qb = min(qt + 16 + j, T - 1);
    f32x4 s[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    f32x4 dp[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    score_pair<C>(base + (int64_t)qa * 3 * C + 4 * g, base + (int64_t)qb * 3 * C + 4 * g, keyrow + C, s[0], s[1]);   // S = Q K^T
    if (DK) score_pair<C>(dob + (int64_t)qa * C + 4 * g, dob + (int64_t)qb * C + 4 * g, keyrow + 2 * C, dp[0], dp[1]);  // dP = dO V^T
    // s[u][r]: query qt + 16u + 4g + r against key k0 + j
    int qr[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qi = qt + 16 * u + 4 * g + r;
        qr[u][r] = min(qi, T - 1);
        const float pr = qi < T ? exp2f(s[u][r] * sc - p.lse2[img + qr[u][r]]) : 0.f;
        s[u][r] = pr;
        if (DK) dp[u][r] = pr * (dp[u][r] - p.delta[img + qr[u][r]]);   // dS[query][key j]
      }
#pragma unroll
    for (int ct = 0; ct < C / 16; ++ct) {
      if (DV) {
        f32x4 a = av[ct];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r) a = mfma16(dob[(int64_t)qr[u][r] * C + 16 * ct + j], s[u][r], a);   // dV^T += dO^T P
        av[ct] = a;
      }
      if (DK) {
        f32x4 a = ak[ct];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r) a = mfma16(base[(int64_t)qr[u][r] * 3 * C + 16 * ct + j], dp[u][r], a);  // dK^T += Q^T dS
        ak[ct] = a;
      }
    }
  }
  if (k0 + j < T) {
    float* drow = p.out + (img + k0 + j) * 3 * C + 4 * g;
#pragma unroll
    for (int ct = 0; ct < C / 16; ++ct) {
      if (DK) st4(drow + C + 16 * ct, ak[ct] * p.scale);
      if (DV) st4(drow + 2 * C + 16 * ct, av[ct]);
    }
  }
}

bool shape_ok(int N, int T, int C) {
  return N > 0 && N <= 65535 && T > 0 && (C == 64 || C == 128 || C == 256 || C == 512);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename K>
void launch(K kernel, int N, int T, hipStream_t st, const FlashF32P& p) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div(T, BLOCK_ROWS), (unsigned)N), dim3(WAVES * 64), 0, st, p);
}

}  // namespace

extern "C" {

int odvae_flash_attn_f32_supported(int N, int T, int C) { return shape_ok(N, T, C) ? 1 : 0; }

// o = softmax(q k^T * scale) v, lse2 = log2 sum exp(scores * scale).  qkv f32 [N][T][3C], o f32 [N][T][C], lse2 f32 [N][T].
int odvae_flash_attn_fwd_f32(const float* qkv, int N, int T, int C, float scale, float* o, float* lse2, void* stream) {
  ODVAE_CHECK_ARG(qkv && o && lse2, "flash_attn_fwd_f32: null operand");
  ODVAE_CHECK_ARG(shape_ok(N, T, C), "flash_attn_fwd_f32: unsupported shape N=%d T=%d C=%d (C in 64/128/256/512)", N, T, C);
  ODVAE_CHECK_ARG(aligned16(qkv) && aligned16(o), "flash_attn_fwd_f32: misaligned operand");
  FlashF32P p{};
  p.qkv = qkv; p.out = o; p.lse2 = lse2; p.T = T; p.scale = scale;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (C) {
    case 64:  launch(flash_f32_fwd_kernel<64>, N, T, st, p); break;
    case 128: launch(flash_f32_fwd_kernel<128>, N, T, st, p); break;
    case 256: launch(flash_f32_fwd_kernel<256>, N, T, st, p); break;
    default:  launch(flash_f32_fwd_kernel<512>, N, T, st, p); break;
  }
  ODVAE_LAUNCH_CHECK("flash_attn_fwd_f32");
  return ODVAE_OK;
}

// dqkv [N][T][3C] (dq | dk | dv) from d_o, the forward's o and lse2; delta f32 [N*T] receives rowsum(d_o * o).
int odvae_flash_attn_bwd_f32(const float* qkv, const float* o, const float* d_o, const float* lse2, int N, int T, int C, float scale,
                             float* dqkv, float* delta, void* stream) {
  ODVAE_CHECK_ARG(qkv && o && d_o && lse2 && dqkv && delta, "flash_attn_bwd_f32: null operand");
  ODVAE_CHECK_ARG(shape_ok(N, T, C), "flash_attn_bwd_f32: unsupported shape N=%d T=%d C=%d (C in 64/128/256/512)", N, T, C);
  ODVAE_CHECK_ARG(aligned16(qkv) && aligned16(o) && aligned16(d_o) && aligned16(dqkv), "flash_attn_bwd_f32: misaligned operand");
  const int r = odvae_rowdot_f32(d_o, o, (int64_t)N * T, C, delta, stream);
  if (r != ODVAE_OK) return r;
  FlashF32P p{};
  p.qkv = qkv; p.o = o; p.d_o = d_o; p.out = dqkv; p.lse2 = const_cast<float*>(lse2); p.delta = delta; p.T = T; p.scale = scale;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (C) {
    case 64:
      launch(flash_f32_dq_kernel<64>, N, T, st, p);
      launch(flash_f32_dkv_kernel<64, true, true>, N, T, st, p); break;
    case 128:
      launch(flash_f32_dq_kernel<128>, N, T, st, p);
      launch(flash_f32_dkv_kernel<128, true, true>, N, T, st, p); break;
    case 256:
      launch(flash_f32_dq_kernel<256>, N, T, st, p);
      launch(flash_f32_dkv_kernel<256, true, true>, N, T, st, p); break;
    default:
      launch(flash_f32_dq_kernel<512>, N, T, st, p);
      launch(flash_f32_dkv_kernel<512, true, false>, N, T, st, p);
      launch(flash_f32_dkv_kernel<512, false, true>, N, T, st, p); break;
  }
  ODVAE_LAUNCH_CHECK("flash_attn_bwd_f32");
  return ODVAE_OK;
}

}  // extern "C"
