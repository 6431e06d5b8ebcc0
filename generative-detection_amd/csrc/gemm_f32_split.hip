// The f32 products of the attention on the bf16 matrix pipe: the T-deep ones (O = P V, dQ = dS K: NN; dV = P^T dO, dK = dS^T Q: TN) and
// the two that write T x T (E = exp(alpha (Q K^T - bound)), dS = alpha E rinv (dO V^T - D): NT, both operands k-contiguous).
//
// An f32 number x is exactly hi + mid + lo with hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid) (round to nearest even;
// both differences are exact in f32: 8 + 8 + 8 significand bits).  Of the nine cross products of two split operands six are kept,
// accumulated in f32 by v_mfma_f32_32x32x16_bf16, smallest first within every 16 k:
//     a_lo b_hi, a_hi b_lo, a_mid b_mid, a_mid b_hi, a_hi b_mid, a_hi b_hi
// The dropped ones (mid lo, lo mid, lo lo) are below 2^-22 of sum_k |a_k| |b_k|.  Six bf16 MFMAs take 6/16 of the cycles of the f32
// MFMAs they replace.  No atomics in the sums and a fixed order: two runs give the same bits.  An Inf operand gives x - hi = NaN, so
// Inf and NaN inputs both come out as NaN (never as a finite number).
//
// float32_matmul_precision (odvae_gemm_select_precision; torch's three levels, on a chip without an xf32 / TF32 matrix instruction):
// the kernel is a template on the number of planes kept, NP.  hi and mid are always the numbers above; what changes is what is dropped.
//     level 0 "highest"  NP = 3  the six products above                      48 KB of LDS, 48 fragment registers per 16 k
//     level 1 "high"     NP = 2  a_mid b_hi, a_hi b_mid, a_hi b_hi           32 KB, 32: "each float32 number as the sum of two bfloat16"
//     level 2 "medium"   NP = 1  a_hi b_hi                                   16 KB, 16: "the bfloat16 datatype for internal computations"
// The kept products are a suffix of the order above, still smallest first within every 16 k.  Dropped at high: mid mid, lo hi, hi lo and
// what highest drops, below 3 * 2^-16 + 2^-21 of sum_k |a_k| |b_k| together; at medium also mid hi and hi mid, below 2^-7 + 2^-13.
// At medium the loader is one v_cvt_pk_bf16_f32 per pair and no subtraction: an Inf operand stays Inf, so Inf times a finite non-zero
// value is Inf and Inf times zero NaN; at high x - hi = NaN as at highest.  A non-finite operand never gives a finite output.
// The ROWNORM row sums come from the unsplit f32 values at every level; the EXPB / SMB row terms join the finished sum.  The dispatch
// (split_eligible, split_tt_eligible) does not look at the level.  NP = 3 is the code it was before the template.
//
// Block = 256 threads = 4 waves (2x2), block tile 128x128, wave tile 64x64, 32 k per step -- gemm_f32.hip's geometry, whose output
// tails (gemm_f32_tile.h) are used as they are.  The operands are split in the loader, in registers: a thread fetches eight
// consecutive k of one row (k-contiguous operand: two 16-byte loads; row-contiguous operand: eight 4-byte loads, lane = row, so a
// wave reads 256 contiguous bytes per k), splits them and writes one ds_write_b128 per plane.  LDS holds [operand][plane][row][32 k]
// in bf16, rows of 64 bytes = four 16-byte slots, XOR-swizzled by the row (tile_byte) so that neither the fragment reads nor the
// loader's writes meet a bank conflict.  One fragment = one ds_read_b128; the
// transposition of a row-contiguous operand costs nothing.  One LDS stage of 48 KB, the next step's operands wait in registers while
// this step's MFMAs run; two or three blocks share a CU and cover each other's split / store phases.
#include "gemm_f32_tile.h"

namespace {

using namespace gemm_tile;

constexpr unsigned PLANE_B = BM * BK * 2;        // 8 192: one bf16 plane of one operand tile
template <int NP> constexpr unsigned OPER_B = NP * PLANE_B;      // the planes kept: hi, mid, lo (3), hi, mid (2) or hi (1)
// the products kept are the last 6 / 3 / 1 of split3::ORDER: all six; a_mid b_hi, a_hi b_mid, a_hi b_hi; a_hi b_hi
template <int NP> constexpr int FIRST_PRODUCT = NP == 3 ? 0 : (NP == 2 ? 3 : 5);
// Blocks per CU asked of the compiler.  Three planes: three (168 registers, 3 x 48 KB of LDS), see the kernel.  Two planes and one: LDS
// (32 / 16 KB) admits a fourth, and asked for three hipcc already stays at or below 128 registers, without scratch, in four of the five
// one-plane kernels and the two-plane ROWNORM one -- those run four blocks per CU as they are.  Asked for four, every two-plane
// kernel but ROWNORM and the one-plane SMB kernel go to scratch (12 to 196 bytes per lane, tools/spill_report.py).  So: three everywhere.
template <int NP> constexpr int BLOCKS_PER_CU = 3;
constexpr unsigned OOB = 0x7FFFFFF0u;
using namespace split3;      // HI, MID, LO, ORDER

// byte of (row, 16-byte slot) inside one plane.  The XOR pattern f(row) = bit 2 of the row | (bit 1 ^ bit 3) << 1 is the one (found by
// enumeration over the lane groups of MI355X_MICROARCH.md, LDS) that serves both sides: the sixteen rows of every ds_read_b128 lane
// group fall on sixteen different 16-byte columns of the 256-byte bank row, and the eight consecutive rows of a ds_write_b128 lane
// group (row-contiguous loader: lane = row, one slot) on the eight columns of the 128-byte one.
__device__ __forceinline__ unsigned tile_byte(int row, int slot) {
  const int f = ((row >> 2) & 1) | ((((row >> 1) ^ (row >> 3)) & 1) << 1);
  return (unsigned)(row * 64 + ((slot ^ f) << 4));
}

template <int NP>
__device__ __forceinline__ void store_unit(unsigned lds_oper, int row, int slot, const float (&x)[8]) {
  u32x4 pl[NP];
  if constexpr (NP == 3) split8(x, pl);
  else if constexpr (NP == 2) split8_hi_mid(x, pl);
  else split8_hi(x, pl);
  const unsigned a = lds_oper + tile_byte(row, slot);
#pragma unroll
  for (int q = 0; q < NP; ++q) lds_st128(a + q * PLANE_B, pl[q]);
}

// One operand's loader.  A unit = eight consecutive k of one row; 128 rows x 4 slots = 512 units, two per thread.
// KC (G[row][k]): unit u = tid + 256 i is row u >> 2, slot u & 3.   RC (G[k][row]): row tid & 127, slot (tid >> 7) + 2 i.
// Rows past the operand and k past K are never fetched: their offsets are replaced by one past num_records (reads as 0).
template <bool KC>
struct SplitLoader {
  __amdgpu_buffer_rsrc_t rsrc;
  unsigned voff[2];
  unsigned ld_bytes;
  int kvalid;
  float x[2][8];

  __device__ __forceinline__ void init(const float* G, int ld, int row0, int nrows, int K) {
    const int tid = threadIdx.x;
    kvalid = K;
    ld_bytes = (unsigned)ld * 4u;
    if (KC) {
      const int rows = min(BM, nrows - row0);
      const int64_t bytes = ((int64_t)(rows - 1) * ld + K) * 4;
      rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(G) + (int64_t)row0 * ld, 0, (int)(bytes < 0x7FFFFFF0ll ? bytes : 0x7FFFFFF0ll), 0x00020000);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int u = tid + 256 * i;
        voff[i] = (u >> 2) < rows ? (unsigned)(((u >> 2) * ld + 8 * (u & 3)) * 4) : OOB;
      }
    } else {
      const int64_t bytes = ((int64_t)(K - 1) * ld + (nrows - row0)) * 4;
      rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(G) + row0, 0, (int)(bytes < 0x7FFFFFF0ll ? bytes : 0x7FFFFFF0ll), 0x00020000);
      const int row = tid & 127;
      voff[0] = row0 + row < nrows ? (unsigned)((tid >> 7) * 8 * ld + row) * 4u : OOB;
      voff[1] = 0;
    }
  }
  // k0 = first k of the step (uniform).  TAIL: the step may reach past K (the first and the last step are fetched this way; every
  // other one carries no compare and no select)
  template <bool TAIL>
  __device__ __forceinline__ void load(int k0) {
    const int tid = threadIdx.x;
    const bool tail = TAIL && k0 + BK > kvalid;
    if (KC) {
      const unsigned soff = (unsigned)__builtin_amdgcn_readfirstlane(k0) * 4u;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 2; ++q) {     // K % 4 == 0: a 16-byte load is inside or outside as a whole
          unsigned vo = voff[i] + 16u * q;
          if (tail && k0 + 8 * ((tid + 256 * i) & 3) + 4 * q >= kvalid) vo = OOB;
          const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, vo, soff, 0);
          x[i][4 * q] = __uint_as_float(v.x); x[i][4 * q + 1] = __uint_as_float(v.y);
          x[i][4 * q + 2] = __uint_as_float(v.z); x[i][4 * q + 3] = __uint_as_float(v.w);
        }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const unsigned soff = (unsigned)__builtin_amdgcn_readfirstlane(k0 + 16 * i + j) * ld_bytes;
          unsigned vo = voff[0];
          if (tail && k0 + 8 * (tid >> 7) + 16 * i + j >= kvalid) vo = OOB;
          x[i][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, vo, soff, 0));
        }
    }
  }
  template <int NP>
  __device__ __forceinline__ void store(unsigned lds_oper) const {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (KC) store_unit<NP>(lds_oper, (tid + 256 * i) >> 2, tid & 3, x[i]);
      else    store_unit<NP>(lds_oper, tid & 127, (tid >> 7) + 2 * i, x[i]);
    }
  }
};

template <bool A_KC, bool B_KC, int EPI, int NP>
// three blocks per CU (168 registers, 3 x 48 KB of LDS): 5 % faster than two on the T-deep attention shapes, 5-6 % on the T x T ones at
// K = 256 and 11-27 % at K = 128 (few steps deep: two other blocks' MFMAs cover a block's first split and its 64 KB tail);
// s_setprio around the MFMAs: nothing
__global__ __launch_bounds__(256, BLOCKS_PER_CU<NP>) void gemm_f32_split_kernel(GemmParams p) {
  constexpr bool ROWNORM = EPI == EPI_ROWNORM, EXPB = EPI == EPI_EXPB, SMB = EPI == EPI_SMB;
  static_assert(NP >= 1 && NP <= 3, "one, two or three bf16 planes");
  static_assert(!ROWNORM || A_KC, "the row sums are taken by the k-contiguous loader");
  static_assert(!(EXPB || SMB) || (A_KC && B_KC), "the T x T tails belong to the NT form");
  __shared__ __attribute__((aligned(16))) char smem[2 * OPER_B<NP>];
  const int tile_m = blockIdx.x % p.tiles_m, tile_n = blockIdx.x / p.tiles_m, batch = blockIdx.z;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const float* A = p.A + batch * p.sA;
  const float* B = p.B + batch * p.sB;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1, li = lane & 31, h = lane >> 5;

  TileOut out;
  out.init(p.M, p.N, p.ldc, m0, n0);

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const unsigned ldsA = lds_addr_of(smem), ldsB = ldsA + OPER_B<NP>;
  // fragment of 32-row tile t, 16-k half kk, plane q: adr[kk] + t * 2048 + q * PLANE_B (rows t*32 + li share li's swizzle: it looks at row bits 1..3)
  unsigned adrA[2], adrB[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    adrA[kk] = ldsA + tile_byte(wm * 64 + li, 2 * kk + h);
    adrB[kk] = ldsB + tile_byte(wn * 64 + li, 2 * kk + h);
  }

  SplitLoader<A_KC> fa;
  SplitLoader<B_KC> fb;
  fa.init(A, p.lda, m0, p.M, p.K);
  fb.init(B, p.ldb, n0, p.N, p.K);
  float rowl[2] = {0.f, 0.f};      // ROWNORM: this thread's share (its 8 of every 32 k) of the sums of rows (tid >> 2) + {0, 64}
  auto stage = [&]() {
    if constexpr (ROWNORM) {       // from the unsplit values, fixed order; k past K reads as 0
#pragma unroll
      for (int i = 0; i < 2; ++i)
        rowl[i] += ((fa.x[i][0] + fa.x[i][1]) + (fa.x[i][2] + fa.x[i][3])) + ((fa.x[i][4] + fa.x[i][5]) + (fa.x[i][6] + fa.x[i][7]));
    }
    fa.template store<NP>(ldsA);
    fb.template store<NP>(ldsB);
  };
  auto products = [&]() {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 a[2][NP], b[2][NP];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < NP; ++q) {
          a[t][q] = frag_from_u32x4(lds_ld128(adrA[kk] + t * 2048u + q * PLANE_B));
          b[t][q] = frag_from_u32x4(lds_ld128(adrB[kk] + t * 2048u + q * PLANE_B));
        }
#pragma unroll
      for (int o = FIRST_PRODUCT<NP>; o < 6; ++o)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = mfma_bf16(a[mt][ORDER.p[o][0]], b[nt][ORDER.p[o][1]], acc[mt][nt]);
    }
  };
  fa.template load<true>(0);
  fb.template load<true>(0);
  stage();
  __syncthreads();
  int k0 = BK;      // first k of the step being fetched
  for (; k0 + BK <= p.K; k0 += BK) {
    fa.template load<false>(k0);
    fb.template load<false>(k0);
    products();
    __syncthreads();
    stage();
    __syncthreads();
  }
  if (k0 < p.K) {      // a last, partial step
    fa.template load<true>(k0);
    fb.template load<true>(k0);
    products();
    __syncthreads();
    stage();
    __syncthreads();
  }
  products();
  __syncthreads();

  const __amdgpu_buffer_rsrc_t crsrc = out.rsrc(p.C + batch * p.sC + (int64_t)m0 * p.ldc);
  if constexpr (ROWNORM) {
    float* rl = reinterpret_cast<float*>(smem);      // [128]; the operand tiles are dead: the loop ended on a barrier
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      rowl[i] += __shfl_xor(rowl[i], 1, 64);
      rowl[i] += __shfl_xor(rowl[i], 2, 64);
    }
    if ((threadIdx.x & 3) == 0) { rl[threadIdx.x >> 2] = rowl[0]; rl[64 + (threadIdx.x >> 2)] = rowl[1]; }
    __syncthreads();
    store_rownorm(out, crsrc, acc, rl, p, batch, m0, tile_n);
  } else if constexpr (EXPB || SMB) {
    // -rowsub[row] joins the finished sum (the f32 kernel starts its accumulators there): the six products of every 16 k stay
    // "smallest first" among themselves, the subtraction rounds once, and the row vectors take registers only after the loop
    f32x16 nsub[2][2];
    float rmv[2][16];
    if constexpr (SMB) __builtin_amdgcn_sched_barrier(0);      // the tail's 96 loads stay behind the last MFMAs' operands (else: one spill)
    GEMM_TILE_FETCH_ROW_VECTORS(out, wm, lane, p, batch, m0, SMB, nsub, rmv);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][nt][r] += nsub[mt][nt][r];
    if constexpr (EXPB) {
      GEMM_TILE_STORE_EXPB(out, crsrc, acc, p.alpha);
    } else {
      const __amdgpu_buffer_rsrc_t ersrc = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(p.emul) + batch * p.sC + (int64_t)m0 * p.ldc, 0, out.tile_bytes, 0x00020000);
      GEMM_TILE_STORE_SMB(out, crsrc, ersrc, acc, p.alpha, rmv);
    }
  } else {
    const float bv[2] = {0.f, 0.f};
    store_plain(out, crsrc, acc, p.alpha, bv);
  }
}

int g_precision = 0;      // float32_matmul_precision, set by odvae_gemm_select_precision: 0 three planes, 1 two, 2 one

template <int NP>
void launch_planes(const GemmParams& p, int transA, int epi, dim3 grid, dim3 block, hipStream_t st) {
  if (epi == EPI_EXPB)          hipLaunchKernelGGL((gemm_f32_split_kernel<true, true, EPI_EXPB, NP>), grid, block, 0, st, p);
  else if (epi == EPI_SMB)      hipLaunchKernelGGL((gemm_f32_split_kernel<true, true, EPI_SMB, NP>), grid, block, 0, st, p);
  else if (epi == EPI_ROWNORM)  hipLaunchKernelGGL((gemm_f32_split_kernel<true, false, EPI_ROWNORM, NP>), grid, block, 0, st, p);
  else if (!transA)             hipLaunchKernelGGL((gemm_f32_split_kernel<true, false, EPI_NONE, NP>), grid, block, 0, st, p);
  else                          hipLaunchKernelGGL((gemm_f32_split_kernel<false, false, EPI_NONE, NP>), grid, block, 0, st, p);
}

}  // namespace

extern "C" int odvae_gemm_select_precision(int level) {
  const int prev = g_precision;
  g_precision = level < 0 ? 0 : (level > 2 ? 2 : level);
  return prev;
}

namespace gemm_tile {

// The dispatch rule of odvae_gemm_f32 and odvae_gemm_rownorm_f32: the bf16-split form runs where the contraction is deep and the
// launch is neither tuned by hand nor anything but a plain batched product:
//   staging per shape (a forced staging mode means "the f32 MFMA kernel"), no split-K, B row-contiguous (NN / TN),
//   K >= 1024, no bias, no residual.
bool split_eligible(int staging_mode, int transB, int M, int N, int K, int batch, const float* bias, const float* residual) {
  return staging_mode == -1 && choose_splits(M, N, K, batch) == 1 && transB == 0 && K >= 1024 && !bias && !residual;
}

// The dispatch rule of the two T x T products (odvae_gemm_exp_bound_f32, odvae_gemm_softmax_bwd[_scaled]_f32; NT, K = the channels):
//   staging per shape (a forced staging mode means "the f32 MFMA kernel" here too), enough 128 x 128 blocks to fill the chip
//   twice over (512, choose_splits' threshold: the T = 256 mid blocks stay where they are), K >= 64.
// The lower bound on K, measured at T = 4096, batch 32 (ms per launch, split vs f32 MFMA; E first, dS second): K = 256 1.50 vs 2.15 and
// 1.67 vs 2.36, K = 128 0.87 vs 1.22 and 1.06 vs 1.45, K = 64 0.59 vs 0.73 and 0.88 vs 0.97, K = 32 0.53 vs 0.52 and 0.80 vs 0.83: a
// single step deep both forms take what the 2.1 GB store takes (4 TB/s) and the second form buys nothing.
constexpr int SPLIT_TT_MIN_K = 64;
bool split_tt_eligible(int staging_mode, int M, int N, int K, int batch) {
  return staging_mode == -1 && (int64_t)ceil_div(M, BM) * ceil_div(N, BN) * batch >= 512 && K >= SPLIT_TT_MIN_K;
}

int launch_split(const GemmParams& p, int transA, int epi, int batch, hipStream_t st) {
  const dim3 grid(p.tiles_m * ceil_div(p.N, BN), 1, batch), block(256);
  if (g_precision == 0)       launch_planes<3>(p, transA, epi, grid, block, st);
  else if (g_precision == 1)  launch_planes<2>(p, transA, epi, grid, block, st);
  else                        launch_planes<1>(p, transA, epi, grid, block, st);
  ODVAE_LAUNCH_CHECK("gemm_f32 (bf16 split)");
  return ODVAE_OK;
}

}  // namespace gemm_tile
