// What the f32 MFMA GEMM (gemm_f32.hip) and its bf16-split form (gemm_f32_split.hip) share: the block geometry, the launch
// parameters, the split-K rule, and the output side of a block -- both instructions leave a 32x32 product in the same
// accumulator layout (column on the lane, rows in the 16 registers), so the store, alpha / bias and row-norm tails are one code.
#pragma once
#include "bf16_common.h"

namespace gemm_tile {

constexpr int BM = 128, BN = 128, BK = 32;   // block tile; 256 threads = 4 waves (2x2) of 64x64 = 2x2 MFMA tiles

struct GemmParams {
  const float* A; const float* B; float* C;
  const float* bias; const float* residual;
  float* partial;      // split-K slabs [split][batch][M][N] or nullptr
  int M, N, K;
  int lda, ldb, ldc;
  int64_t sA, sB, sC;
  float alpha;
  int splits, k_per_split;
  int tiles_m;
  // softmax-backward epilogue (EPI_SMB kernels only): C = alpha * emul .* (A B^T - rowsub[row]) (* rowmul[row]); emul has C's layout
  const float* rowsub; const float* emul; int64_t sRow;
  const float* rowmul;   // EPI_SMB: optional second row factor (1 / l_i when emul holds unnormalised exponentials), or null
  // EPI_EXPB: C = exp(alpha * (A B^T - rowsub[row])) -- attention scores leave the QK^T product as exponentials relative to a per-row
  //           upper bound of the scores instead of the row maximum: no separate softmax pass over the T x T tensor
  // EPI_ROWNORM (A k-contiguous, unsplit): l[row] = sum_k A[row][k] is accumulated beside the products, C = A B / l[row];
  //           rowout[row] = 1 / l[row] (written by the first column tile); *flag |= 1 where l is not a normal number >= 1e-30
  float* rowout; int* flag;
  const int* pred;       // gemm_f32_pred_kernel: nothing happens unless *pred != 0
};
constexpr int EPI_NONE = 0, EPI_SMB = 1, EPI_EXPB = 2, EPI_ROWNORM = 3;

inline int choose_splits(int M, int N, int K, int batch) {
  const int64_t tiles = (int64_t)ceil_div(M, BM) * ceil_div(N, BN) * batch;
  if (tiles >= 512 || K <= 1024) return 1;
  int64_t s = 512 / tiles;           // two blocks per CU; 1024 / 256 measured 8-12 % slower
  const int64_t max_by_k = K / 512;  // at least 16 k-tiles per split
  if (s > max_by_k) s = max_by_k;
  if (s < 1) s = 1;
  return (int)s;
}

// Output addressing of one lane: 32-bit byte offsets into a buffer descriptor that starts at the block's first row; rows >= M
// and columns >= N get an offset past num_records (loads return 0, stores are dropped): no compares, no 64-bit math per element.
// The lane owns columns n0 + wn*64 + nt*32 + li; its rows come from the accumulator register index (acc_row).
struct TileOut {
  static constexpr unsigned OOB = 0x7FFFFFF0u;
  int rows_here, ldc, tile_bytes, wm, lane;
  unsigned colbyte[2];
  __device__ __forceinline__ void init(int M, int N, int ldc_, int m0, int n0) {
    lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6, wn = wave & 1, li = lane & 31;
    wm = wave >> 1;
    ldc = ldc_;
    rows_here = min(BM, M - m0);
    tile_bytes = ((rows_here - 1) * ldc + N) * 4;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int col = n0 + wn * 64 + nt * 32 + li;
      colbyte[nt] = col < N ? (unsigned)col * 4u : OOB;
    }
  }
  __device__ __forceinline__ int row(int mt, int r) const { return wm * 64 + mt * 32 + acc_row(r, lane); }   // within the block tile
  __device__ __forceinline__ unsigned row_byte(int mt, int r) const {
    const int rw = row(mt, r);
    return rw < rows_here ? (unsigned)(rw * ldc) * 4u : OOB;
  }
  __device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(float* tile_origin) const {
    return __builtin_amdgcn_make_buffer_rsrc(tile_origin, 0, tile_bytes, 0x00020000);
  }
};

// C = acc * alpha + bias[col]; stores only
__device__ __forceinline__ void store_plain(const TileOut& o, __amdgpu_buffer_rsrc_t crsrc, const f32x16 (&acc)[2][2], float alpha, const float (&bv)[2]) {
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const unsigned rb_ = o.row_byte(mt, r);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[mt][nt][r] * alpha + bv[nt]), crsrc, rb_ + o.colbyte[nt], 0, 0);
    }
}

// EPI_ROWNORM tail: rl[128] (LDS, published and barrier-ed by the caller) holds the block's row sums l; C = acc / l, rowout = 1 / l
// (first column tile), *flag |= 1 where l is not a normal number >= 1e-30
__device__ __forceinline__ void store_rownorm(const TileOut& o, __amdgpu_buffer_rsrc_t crsrc, const f32x16 (&acc)[2][2], const float* rl,
                                              const GemmParams& p, int batch, int m0, int tile_n) {
  const int wn = (threadIdx.x >> 6) & 1, li = o.lane & 31;
  bool bad = false;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = o.row(mt, r);
      const float l = rl[row];
      const float rinv = 1.f / l;
      bad |= row < o.rows_here && !(l >= 1e-30f && l < 3.0e38f);
      const unsigned rb_ = o.row_byte(mt, r);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[mt][nt][r] * rinv), crsrc, rb_ + o.colbyte[nt], 0, 0);
      if (tile_n == 0 && wn == 0 && li == 0 && row < o.rows_here) p.rowout[batch * p.sRow + m0 + row] = rinv;
    }
  if (p.flag && __any(bad) && o.lane == 0) atomicOr(p.flag, 1);
}

// The EPI_EXPB / EPI_SMB pieces below are shared as TEXT, not as functions: hipcc optimises a callee on its own before it inlines it,
// and the tails of the f32 kernels then come out with one v_mul_lo_u32 per output row (41 against 9, as store_plain's do) instead of
// the add chains they were measured with.  Expanded in place they assemble to the same instructions as when they were written there.
// `o` is the block's TileOut, `p` its GemmParams, `wm` and `lane` the thread's wave row and lane.

// The per-row vectors of this block tile as the lane's accumulator registers see them: seed[mt][nt][r] = -rowsub[row] (f32x16 [2][2]),
// and, where MUL, rmv[mt][r] = rowmul[row] (1 when rowmul is null).  Buffer loads whose descriptor ends at the tile's last row -- rows
// past it read 0, no guard (32 guarded loads per lane, each waited for on its own, cost ~4 us per block: 8 % of a QK^T-shaped tile)
#define GEMM_TILE_FETCH_ROW_VECTORS(o, wm, lane, p, batch, m0, MUL, seed, rmv)                                                            \
  {                                                                                                                                      \
    const __amdgpu_buffer_rsrc_t srs_ =                                                                                                  \
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>((p).rowsub) + (batch) * (p).sRow + (m0), 0, (o).rows_here * 4, 0x00020000);  \
    const bool has_mul_ = (MUL) && (p).rowmul != nullptr;                                                                                \
    const __amdgpu_buffer_rsrc_t mrs_ = __builtin_amdgcn_make_buffer_rsrc(                                                               \
        const_cast<float*>(has_mul_ ? (p).rowmul : (p).rowsub) + (batch) * (p).sRow + (m0), 0, has_mul_ ? (o).rows_here * 4 : 0, 0x00020000); \
    _Pragma("unroll") for (int mt_ = 0; mt_ < 2; ++mt_)                                                                                  \
      _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) {                                                                                \
        const int row_ = (wm) * 64 + mt_ * 32 + acc_row(r_, lane);                                                                       \
        const float d_ = -__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(srs_, row_ * 4, 0, 0));                                   \
        (seed)[mt_][0][r_] = d_; (seed)[mt_][1][r_] = d_;                                                                                \
        if constexpr (MUL) {                                                                                                             \
          const float m_ = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(mrs_, row_ * 4, 0, 0));                                  \
          (rmv)[mt_][r_] = has_mul_ ? m_ : 1.f;                                                                                          \
        }                                                                                                                                \
      }                                                                                                                                  \
  }

// EPI_EXPB tail: acc holds score - row bound; C = exp(alpha * acc) as exp2 of one product.  Stores only.
#define GEMM_TILE_STORE_EXPB(o, crsrc, acc, alpha)                                                                                       \
  {                                                                                                                                      \
    const float a2_ = (alpha) * 1.44269504088896f;                                                                                       \
    _Pragma("unroll") for (int mt_ = 0; mt_ < 2; ++mt_)                                                                                  \
      _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) {                                                                                \
        const unsigned rb_ = (o).row_byte(mt_, r_);                                                                                      \
        _Pragma("unroll") for (int nt_ = 0; nt_ < 2; ++nt_)                                                                              \
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(__builtin_amdgcn_exp2f((acc)[mt_][nt_][r_] * a2_)), crsrc,               \
                                                rb_ + (o).colbyte[nt_], 0, 0);                                                           \
      }                                                                                                                                  \
  }

// EPI_SMB tail: acc holds dP - D; C = acc * (alpha * rmv[row]) * emul (ersrc: emul's descriptor, laid out like C's).  Per 32-row half:
// all loads of the multiplier tile first, then its stores (one half's 32 values live at a time: the kernels fit 168 registers and three
// blocks share a CU, so that a block's epilogue runs under two others' MFMAs).  C may alias emul: a lane reads what it then writes.
#define GEMM_TILE_STORE_SMB(o, crsrc, ersrc, acc, alpha, rmv)                                                                            \
  {                                                                                                                                      \
    _Pragma("unroll") for (int mt_ = 0; mt_ < 2; ++mt_) {                                                                                \
      float pv_[2][16];                                                                                                                  \
      _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) {                                                                                \
        const unsigned rb_ = (o).row_byte(mt_, r_);                                                                                      \
        _Pragma("unroll") for (int nt_ = 0; nt_ < 2; ++nt_)                                                                              \
          pv_[nt_][r_] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ersrc, rb_ + (o).colbyte[nt_], 0, 0));                     \
      }                                                                                                                                  \
      _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) {                                                                                \
        const unsigned rb_ = (o).row_byte(mt_, r_);                                                                                      \
        _Pragma("unroll") for (int nt_ = 0; nt_ < 2; ++nt_)                                                                              \
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint((acc)[mt_][nt_][r_] * ((alpha) * (rmv)[mt_][r_]) * pv_[nt_][r_]), crsrc, \
                                                rb_ + (o).colbyte[nt_], 0, 0);                                                           \
      }                                                                                                                                  \
    }                                                                                                                                    \
  }

// The bf16-split form (gemm_f32_split.hip): true when this product runs there, see split_eligible (NN / TN, deep K) and
// split_tt_eligible (the NT products with the EPI_EXPB / EPI_SMB tails)
bool split_eligible(int staging_mode, int transB, int M, int N, int K, int batch, const float* bias, const float* residual);
bool split_tt_eligible(int staging_mode, int M, int N, int K, int batch);
// launches it; epi = EPI_NONE (transA selects NN / TN), EPI_ROWNORM (NN), EPI_EXPB or EPI_SMB (NT)
int launch_split(const GemmParams& p, int transA, int epi, int batch, hipStream_t st);

}  // namespace gemm_tile
