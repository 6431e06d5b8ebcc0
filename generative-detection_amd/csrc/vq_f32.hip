// Vector quantiser ([UPSTREAM] taming VectorQuantizer2, the quantiser of ldm's VQModel) for gfx950, f32.
//
//   idx[m] = argmin_k s_k,  s_k = |e_k|^2 - 2 z_m . e_k   (the row constant |z_m|^2 of upstream's distance is dropped; ties: lowest k)
//   z_q[m] = E[idx[m]],  loss = (1 + beta) sum (z_q - z)^2 / (M D)
//   dz = g_q + g_l (2 c_z / (M D)) (z - z_q),  dE[k] = g_l (2 c_e / (M D)) sum_{idx[m] = k} (e_k - z_m)
//
// A row m = (n, p) is one position of a logical [N, D, H, W] tensor, addressed by element strides (sn, sc, sp): n sn + d sc + p sp.  Both
// layouts of such a tensor fit without a copy: NCHW (sc = HW, sp = 1) and the NHWC memory the conv kernels write (sc = 1, sp = D).
// Nothing of size M x K exists: the search keeps a running (best score, best index) per row.
//
// Search: a 256-thread workgroup owns 64 rows and walks its share of the codebook in chunks of 64 codes; a thread holds a 4 x 4 tile of
// dot products (rows ty*4.., codes tx*4..) fed from two LDS slabs [depth][64] of z and E, depth DS = 4, 8, 16 or 32 per pass over D.
// With few row tiles the codebook is split across gridDim.y; every split leaves (score, index) per row and the finish kernel takes the
// splits in code order under the same `s < best` rule, so the lowest index wins there too.
// Scores: one fmaf chain over d (ascending), |e_k|^2 likewise, one subtraction: D + 1 roundings per score.
//
// dE without float atomics: a stable counting sort of the rows by code (integer atomics only in the histogram; ranks inside a code are
// by row number), then one workgroup per code sums its rows in a fixed order in f64.  Two runs give the same bits.
#include "common.h"

namespace {

constexpr int TILE_ROWS = 64, CHUNK = 64, LDS_LD = 68;       // LDS slab rows padded to 68 floats: 16-byte aligned float4 reads
constexpr int SEARCH_TILE_CAP = 16384;                        // row tiles per launch dimension; further tiles by a grid-stride loop
constexpr int FINISH_CAP = 4096;                              // workgroups (and f64 partial sums) of the finish kernel
constexpr int SORT_KB_MIN = 32, SORT_BLOCKS = 256, SORT_KB_MAX = 4096;
constexpr int VQ_MAX_D = 512, VQ_MAX_K = 1 << 20;

struct Strides { int64_t n, c, p; };

__device__ __forceinline__ int64_t row_base(int64_t m, int64_t HW, const Strides& s) {
  const int64_t n = m / HW, p = m - n * HW;
  return n * s.n + p * s.p;
}

__device__ __forceinline__ int64_t clamp_index(int64_t i, int K) { return i < 0 ? 0 : (i > K - 1 ? (int64_t)(K - 1) : i); }

// |e_k|^2 as an fmaf chain over d
__global__ void vq_norms_kernel(const float* __restrict__ E, int K, int D, float* __restrict__ norms) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const float* e = E + (int64_t)k * D;
  float a = 0.f;
  for (int d = 0; d < D; ++d) a = fmaf(e[d], e[d], a);
  norms[k] = a;
}

__device__ __forceinline__ void take_lower(float& b, int& bi, float s, int i) {     // lexicographic (score, index); NaN never wins
  if (s < b || (s == b && i < bi)) { b = s; bi = i; }
}

template <int DS>
__global__ __launch_bounds__(256) void vq_search_kernel(const float* __restrict__ z, Strides zs, int64_t M, int64_t HW, int D,
                                                        const float* __restrict__ E, const float* __restrict__ norms, int K,
                                                        int codes_per_split, int64_t ntiles, float* __restrict__ pscore,
                                                        int* __restrict__ pidx) {
  __shared__ __attribute__((aligned(16))) float zl[DS][LDS_LD];
  __shared__ __attribute__((aligned(16))) float el[DS][LDS_LD];
  __shared__ float nl[CHUNK];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int split = blockIdx.y;
  const int kbeg = split * codes_per_split, kend = min(K, kbeg + codes_per_split);
  const int nslabs = (D + DS - 1) / DS;
  const bool d_fast = zs.c == 1;        // NHWC memory: consecutive threads take consecutive d; else consecutive rows
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t m0 = tile * TILE_ROWS;
    float best[4];
    int bidx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { best[i] = INFINITY; bidx[i] = 0; }
    for (int c0 = kbeg; c0 < kend; c0 += CHUNK) {
      float acc[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
      for (int slab = 0; slab < nslabs; ++slab) {
        const int dbase = slab * DS;
        __syncthreads();                                  // the previous pass has read both slabs
        if (nslabs > 1 || c0 == kbeg) {                   // a single slab holds the whole row tile: loaded once per tile
          for (int e = tid; e < DS * TILE_ROWS; e += 256) {
            const int dd = d_fast ? e % DS : e / TILE_ROWS, r = d_fast ? e / DS : e % TILE_ROWS;
            const int64_t m = m0 + r;
            const int d = dbase + dd;
            zl[dd][r] = (m < M && d < D) ? z[row_base(m, HW, zs) + (int64_t)d * zs.c] : 0.f;
          }
        }
        for (int e = tid; e < DS * CHUNK; e += 256) {
          const int dd = e % DS, c = e / DS;
          const int k = c0 + c, d = dbase + dd;
          el[dd][c] = (k < kend && d < D) ? E[(int64_t)k * D + d] : 0.f;
        }
        if (slab == 0 && tid < CHUNK) nl[tid] = c0 + tid < kend ? norms[c0 + tid] : 0.f;
        __syncthreads();
#pragma unroll
        for (int dd = 0; dd < DS; ++dd) {
          const f32x4 zv = *reinterpret_cast<const f32x4*>(&zl[dd][ty * 4]);
          const f32x4 ev = *reinterpret_cast<const f32x4*>(&el[dd][tx * 4]);
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(zv[i], ev[j], acc[i][j]);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {                       // codes in ascending order: `<` keeps the lowest index
        const int k = c0 + tx * 4 + j;
        if (k < kend) {
          const float nk = nl[tx * 4 + j];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float s = nk - 2.f * acc[i][j];
            if (s < best[i]) { best[i] = s; bidx[i] = k; }
          }
        }
      }
    }
    // the 16 threads of a row group are 16 consecutive lanes
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        const float s2 = __shfl_xor(best[i], o, 64);
        const int i2 = __shfl_xor(bidx[i], o, 64);
        take_lower(best[i], bidx[i], s2, i2);
      }
      const int64_t m = m0 + ty * 4 + i;
      if (tx == 0 && m < M) {
        pscore[(int64_t)split * M + m] = best[i];
        pidx[(int64_t)split * M + m] = bidx[i];
      }
    }
  }
}

__device__ __forceinline__ double block_sum_f64(double v, double* red) {     // 256 threads, fixed order; result valid on thread 0
  v = wave_sum_f64(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) t = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return t;
}

// splits in code order -> idx (int64), z_q = E[idx], partial[blockIdx.x] = sum (z_q - z)^2 in f64 (difference and square in f64)
__global__ __launch_bounds__(256) void vq_finish_kernel(const float* __restrict__ z, Strides zs, float* __restrict__ zq, Strides qs,
                                                        int64_t M, int64_t HW, int D, const float* __restrict__ E, int K, int nsplit,
                                                        const float* __restrict__ pscore, const int* __restrict__ pidx,
                                                        int64_t* __restrict__ idx, double* __restrict__ partial) {
  __shared__ double red[4];
  double sum = 0.0;
  for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
    float b = INFINITY;
    int bi = 0;
    for (int s = 0; s < nsplit; ++s) {
      const float sc = pscore[(int64_t)s * M + m];
      if (sc < b) { b = sc; bi = pidx[(int64_t)s * M + m]; }
    }
    bi = min(max(bi, 0), K - 1);
    idx[m] = bi;
    const float* e = E + (int64_t)bi * D;
    const int64_t zb = row_base(m, HW, zs), qb = row_base(m, HW, qs);
    for (int d = 0; d < D; ++d) {
      const float ev = e[d];
      zq[qb + (int64_t)d * qs.c] = ev;
      const double df = (double)ev - (double)z[zb + (int64_t)d * zs.c];
      sum += df * df;
    }
  }
  const double t = block_sum_f64(sum, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void vq_loss_final_kernel(const double* __restrict__ partial, int nparts, double scale, float* __restrict__ loss) {
  __shared__ double red[4];
  double a = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) a += partial[i];
  const double t = block_sum_f64(a, red);
  if (threadIdx.x == 0) *loss = (float)(t * scale);
}

// dz = g_q + g_l * scale_z * (z - E[idx]), one rounding (the arithmetic is in f64)
__global__ __launch_bounds__(256) void vq_dz_kernel(const float* __restrict__ z, const float* __restrict__ gq, float* __restrict__ dz, Strides zs,
                                                    int64_t M, int64_t HW, int D, const float* __restrict__ E, int K,
                                                    const int64_t* __restrict__ idx, const float* __restrict__ gl, double scale_z) {
#pragma clang fp contract(off)      // the product rounds on its own: g + coef * diff is the two-rounding f64 expression a host evaluates
  const double coef = gl ? (double)*gl * scale_z : 0.0;
  for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
    const int64_t i = clamp_index(idx[m], K);
    const float* e = E + i * D;
    const int64_t zb = row_base(m, HW, zs);
    for (int d = 0; d < D; ++d) {
      const int64_t a = zb + (int64_t)d * zs.c;
      const double g = gq ? (double)gq[a] : 0.0;
      dz[a] = (float)(g + coef * ((double)z[a] - (double)e[d]));
    }
  }
}

// ---- stable counting sort of the rows by code ------------------------------------------------------------------------------------------
// grid (code ranges of KB codes, row segments of RS rows).  FILL = false: seg[s][k] = rows of segment s with code k.  FILL = true: perm gets
// the rows of every code in ascending row order, starting at off[k] + seg[s][k] (seg then holds the exclusive prefix over the segments).
template <bool FILL>
__global__ __launch_bounds__(256) void vq_sort_kernel(const int64_t* __restrict__ idx, int64_t M, int K, int KB, int64_t RS, int* __restrict__ seg,
                                                      const int* __restrict__ off, int* __restrict__ perm) {
  __shared__ int cursor[SORT_KB_MAX];
  __shared__ int lrow[256], lcode[256], wcnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k0 = blockIdx.x * KB, nk = min(K, k0 + KB) - k0;
  const int64_t r0 = (int64_t)blockIdx.y * RS, r1 = r0 + RS < M ? r0 + RS : M;
  int* segrow = seg + (int64_t)blockIdx.y * K + k0;
  for (int c = tid; c < nk; c += 256) cursor[c] = FILL ? off[k0 + c] + segrow[c] : 0;
  __syncthreads();
  for (int64_t base = r0; base < r1; base += 256) {
    const int64_t row = base + tid;
    int c = -1;
    if (row < r1) {
      const int64_t i = idx[row];
      if (i >= k0 && i < k0 + nk) c = (int)(i - k0);
    }
    if constexpr (!FILL) {
      if (c >= 0) atomicAdd(&cursor[c], 1);
    } else {
      const unsigned long long bal = __ballot(c >= 0);
      if (lane == 0) wcnt[wave] = __popcll(bal);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        before += w < wave ? wcnt[w] : 0;
        total += wcnt[w];
      }
      const int slot = before + __popcll(bal & ((1ull << lane) - 1ull));
      if (c >= 0) { lrow[slot] = (int)(row - r0); lcode[slot] = c; }
      __syncthreads();
      int pos = -1;
      bool last = false;
      if (tid < total) {                                  // entry tid of the compacted list (row order): its rank among its code's entries
        const int mc = lcode[tid];
        int rank = 0;
        last = true;
        for (int j = 0; j < total; ++j) {
          const bool same = lcode[j] == mc;
          rank += (same && j < tid) ? 1 : 0;
          last = last && !(same && j > tid);
        }
        pos = cursor[mc] + rank;
        perm[pos] = (int)(r0 + lrow[tid]);
      }
      __syncthreads();                                    // every cursor read of this step is done
      if (last) cursor[lcode[tid]] = pos + 1;
    }
  }
  if constexpr (!FILL) {
    __syncthreads();
    for (int c = tid; c < nk; c += 256) segrow[c] = cursor[c];
  }
}

// one workgroup of 1024: seg[s][k] -> exclusive prefix over s, cnt[k] = total, off[k] = exclusive prefix of cnt over k
__global__ __launch_bounds__(1024) void vq_sort_scan_kernel(int* __restrict__ seg, int K, int S, int* __restrict__ cnt, int* __restrict__ off) {
  __shared__ int part[1024];
  const int tid = threadIdx.x;
  const int span = (K + 1023) / 1024;
  const int ka = min(K, tid * span), kb = min(K, ka + span);
  int local = 0;
  for (int k = ka; k < kb; ++k) {
    int run = 0;
    for (int s = 0; s < S; ++s) {
      int* p = seg + (int64_t)s * K + k;
      const int v = *p;
      *p = run;
      run += v;
    }
    cnt[k] = run;
    local += run;
  }
  part[tid] = local;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < 1024; ++t) { const int v = part[t]; part[t] = run; run += v; }
  }
  __syncthreads();
  int run = part[tid];
  for (int k = ka; k < kb; ++k) { off[k] = run; run += cnt[k]; }
}

// one workgroup per code: dE[k][d] = g_l scale_e sum_j (e_k[d] - z[perm[off + j]][d]); row slot g takes j = g, g + G, ... and the slots are
// added in slot order: a fixed order, in f64
__global__ __launch_bounds__(256) void vq_segsum_kernel(const float* __restrict__ z, Strides zs, int64_t HW, int D, const float* __restrict__ E,
                                                        const int* __restrict__ cnt, const int* __restrict__ off, const int* __restrict__ perm,
                                                        const float* __restrict__ gl, double scale_e, int DP, float* __restrict__ dE) {
  __shared__ double red[256];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int c = cnt[k], o = off[k];
  const int G = 256 / DP, d0 = tid % DP, g = tid / DP;
  const double coef = gl ? (double)*gl * scale_e : 0.0;
  for (int dbase = 0; dbase < D; dbase += DP) {
    const int d = dbase + d0;
    double a = 0.0;
    if (d < D) {
      const double e = (double)E[(int64_t)k * D + d];
      for (int j = g; j < c; j += G) a += e - (double)z[row_base(perm[o + j], HW, zs) + (int64_t)d * zs.c];
    }
    red[tid] = a;
    __syncthreads();
    if (g == 0 && d < D) {
      double t = 0.0;
      for (int gg = 0; gg < G; ++gg) t += red[gg * DP + d0];
      dE[(int64_t)k * D + d] = (float)(coef * t);
    }
    __syncthreads();
  }
}

// out = E[clamp(idx, 0, K - 1)]
__global__ __launch_bounds__(256) void vq_gather_kernel(const int64_t* __restrict__ idx, int64_t M, int64_t HW, const float* __restrict__ E, int K,
                                                        int D, float* __restrict__ out, Strides os) {
  for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
    const int64_t i = clamp_index(idx[m], K);
    const float* e = E + i * D;
    const int64_t ob = row_base(m, HW, os);
    for (int d = 0; d < D; ++d) out[ob + (int64_t)d * os.c] = e[d];
  }
}

__global__ __launch_bounds__(256) void vq_count_kernel(const int64_t* __restrict__ idx, int64_t M, int K, int* __restrict__ counts) {
  for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < M; m += (int64_t)gridDim.x * 256) {
    const int64_t i = idx[m];
    if (i >= 0 && i < K) atomicAdd(&counts[i], 1);       // integer adds: the result does not depend on their order
  }
}

// out[0] = exp(-sum p log(p + 1e-10)), p = count / M; out[1] = number of codes with count > 0.  f64, fixed order
__global__ __launch_bounds__(256) void vq_usage_final_kernel(const int* __restrict__ counts, int K, double inv_m, float* __restrict__ out) {
  __shared__ double red[4];
  double h = 0.0, used = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) {
    const int c = counts[k];
    const double p = (double)c * inv_m;
    h += p * log(p + 1e-10);
    used += c > 0 ? 1.0 : 0.0;
  }
  const double th = block_sum_f64(h, red);
  const double tu = block_sum_f64(used, red);
  if (threadIdx.x == 0) {
    out[0] = (float)exp(-th);
    out[1] = (float)tu;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
struct Plan { int ds, nslabs, nsplit, codes_per_split, grid_x, finish_blocks; int64_t ntiles; };

bool sizes_ok(const char* what, int64_t M, int K, int D) {
  if (M < 1 || M > 0x7FFFFFFFLL || K < 1 || K > VQ_MAX_K || D < 1 || D > VQ_MAX_D) {
    odvae_set_error("%s: needs 1 <= M < 2^31 rows, 1 <= K <= 2^20 codes, 1 <= D <= 512, got M=%lld K=%d D=%d", what, (long long)M, K, D);
    return false;
  }
  return true;
}

Plan make_plan(int64_t M, int K, int D) {
  Plan p;
  p.ds = D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : 32;
  p.nslabs = ceil_div(D, p.ds);
  p.ntiles = ceil_div64(M, TILE_ROWS);
  // few row tiles against many codes: the codebook is split until about two workgroups per CU exist, at least four chunks per split
  int64_t s = p.ntiles >= 256 ? 1 : 512 / p.ntiles;
  s = std::min<int64_t>(s, std::max(1, K / (4 * CHUNK)));
  p.codes_per_split = round_up(ceil_div(K, (int)std::max<int64_t>(s, 1)), CHUNK);
  p.nsplit = ceil_div(K, p.codes_per_split);
  p.grid_x = (int)std::min<int64_t>(p.ntiles, SEARCH_TILE_CAP);
  p.finish_blocks = (int)std::min<int64_t>(ceil_div64(M, 256), FINISH_CAP);
  return p;
}

struct SortPlan { int kb, nb, S; int64_t rs; };

SortPlan make_sort_plan(int64_t M, int K) {
  SortPlan p;
  p.kb = std::max(SORT_KB_MIN, ceil_div(K, SORT_BLOCKS));
  p.nb = ceil_div(K, p.kb);
  int64_t s = std::max<int64_t>(1, std::min<int64_t>(2 * SORT_BLOCKS / p.nb, ceil_div64(M, 1024)));
  p.rs = ceil_div64(ceil_div64(M, s), 256) * 256;
  p.S = (int)ceil_div64(M, p.rs);
  return p;
}

size_t align256(size_t n) { return (n + 255) / 256 * 256; }

// assign workspace: [f64 partial sums FINISH_CAP][norms K][scores nsplit M][indices nsplit M]
struct AssignWs { double* partial; float* norms; float* pscore; int* pidx; size_t bytes; };
AssignWs assign_ws(void* base, int64_t M, int K, const Plan& p) {
  AssignWs w;
  char* b = (char*)base;
  size_t o = 0;
  w.partial = (double*)(b + o); o += align256(sizeof(double) * FINISH_CAP);
  w.norms = (float*)(b + o); o += align256(sizeof(float) * (size_t)K);
  w.pscore = (float*)(b + o); o += align256(sizeof(float) * (size_t)p.nsplit * (size_t)M);
  w.pidx = (int*)(b + o); o += align256(sizeof(int) * (size_t)p.nsplit * (size_t)M);
  w.bytes = o;
  return w;
}

// backward workspace: [seg S K][cnt K][off K][perm M]
struct BackwardWs { int* seg; int* cnt; int* off; int* perm; size_t bytes; };
BackwardWs backward_ws(void* base, int64_t M, int K, const SortPlan& p) {
  BackwardWs w;
  char* b = (char*)base;
  size_t o = 0;
  w.seg = (int*)(b + o); o += align256(sizeof(int) * (size_t)p.S * (size_t)K);
  w.cnt = (int*)(b + o); o += align256(sizeof(int) * (size_t)K);
  w.off = (int*)(b + o); o += align256(sizeof(int) * (size_t)K);
  w.perm = (int*)(b + o); o += align256(sizeof(int) * (size_t)M);
  w.bytes = o;
  return w;
}

// the largest element offset of a row-strided tensor must fit the 64-bit arithmetic trivially; what is checked here is the sign
bool strides_ok(int64_t sn, int64_t sc, int64_t sp) { return sn >= 0 && sc >= 1 && sp >= 1; }

template <int DS>
void launch_search(const Plan& p, const float* z, Strides zs, int64_t M, int64_t HW, int D, const float* E, int K, const AssignWs& w, hipStream_t st) {
  hipLaunchKernelGGL(vq_search_kernel<DS>, dim3(p.grid_x, p.nsplit), dim3(256), 0, st, z, zs, M, HW, D, E, w.norms, K, p.codes_per_split,
                     p.ntiles, w.pscore, w.pidx);
}

}  // namespace

extern "C" {

int odvae_vq_plan(int64_t M, int K, int D, int* out) {
  if (!sizes_ok("vq_plan", M, K, D)) return ODVAE_ERR_ARG;
  ODVAE_CHECK_ARG(out, "vq_plan: null pointer");
  const Plan p = make_plan(M, K, D);
  const SortPlan sp = make_sort_plan(M, K);
  out[0] = TILE_ROWS; out[1] = CHUNK; out[2] = p.ds; out[3] = p.nslabs; out[4] = p.nsplit; out[5] = p.codes_per_split;
  out[6] = p.grid_x; out[7] = SEARCH_TILE_CAP; out[8] = p.finish_blocks; out[9] = FINISH_CAP;
  out[10] = sp.kb; out[11] = sp.nb; out[12] = sp.S; out[13] = (int)std::min<int64_t>(sp.rs, 0x7FFFFFFF); out[14] = GRID_1D_CAP; out[15] = 0;
  return ODVAE_OK;
}

size_t odvae_vq_assign_workspace_bytes(int64_t M, int K, int D) {
  if (M < 1 || M > 0x7FFFFFFFLL || K < 1 || K > VQ_MAX_K || D < 1 || D > VQ_MAX_D) return 0;
  return assign_ws(nullptr, M, K, make_plan(M, K, D)).bytes;
}

int odvae_vq_assign_f32(const float* z, int64_t z_sn, int64_t z_sc, int64_t z_sp, int64_t N, int64_t HW, int D, const float* E, int K,
                        int64_t* idx, float* zq, int64_t q_sn, int64_t q_sc, int64_t q_sp, void* workspace, size_t workspace_bytes,
                        void* stream) {
  ODVAE_CHECK_ARG(N >= 1 && HW >= 1 && N <= 0x7FFFFFFFLL / HW, "vq_assign: N=%lld HW=%lld: needs 1 <= N HW < 2^31", (long long)N, (long long)HW);
  const int64_t M = N * HW;
  if (!sizes_ok("vq_assign", M, K, D)) return ODVAE_ERR_ARG;
  ODVAE_CHECK_ARG(z && E && idx && zq && workspace, "vq_assign: null pointer");
  ODVAE_CHECK_ARG(strides_ok(z_sn, z_sc, z_sp) && strides_ok(q_sn, q_sc, q_sp), "vq_assign: strides must be positive");
  const Plan p = make_plan(M, K, D);
  const AssignWs w = assign_ws(workspace, M, K, p);
  if (workspace_bytes < w.bytes) {
    odvae_set_error("vq_assign: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
    return ODVAE_ERR_WORKSPACE;
  }
  ODVAE_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "vq_assign: workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const Strides zs{z_sn, z_sc, z_sp}, qs{q_sn, q_sc, q_sp};
  hipLaunchKernelGGL(vq_norms_kernel, dim3(ceil_div(K, 256)), dim3(256), 0, st, E, K, D, w.norms);
  ODVAE_LAUNCH_CHECK("vq_norms");
  switch (p.ds) {
    case 4: launch_search<4>(p, z, zs, M, HW, D, E, K, w, st); break;
    case 8: launch_search<8>(p, z, zs, M, HW, D, E, K, w, st); break;
    case 16: launch_search<16>(p, z, zs, M, HW, D, E, K, w, st); break;
    default: launch_search<32>(p, z, zs, M, HW, D, E, K, w, st); break;
  }
  ODVAE_LAUNCH_CHECK("vq_search");
  hipLaunchKernelGGL(vq_finish_kernel, dim3(p.finish_blocks), dim3(256), 0, st, z, zs, zq, qs, M, HW, D, E, K, p.nsplit, w.pscore, w.pidx, idx,
                     w.partial);
  ODVAE_LAUNCH_CHECK("vq_finish");
  return ODVAE_OK;
}

int odvae_vq_loss_finalize(const void* workspace, size_t workspace_bytes, int64_t M, int K, int D, float beta, float* loss, void* stream) {
  if (!sizes_ok("vq_loss_finalize", M, K, D)) return ODVAE_ERR_ARG;
  ODVAE_CHECK_ARG(workspace && loss, "vq_loss_finalize: null pointer");
  const Plan p = make_plan(M, K, D);
  if (workspace_bytes < sizeof(double) * FINISH_CAP) {
    odvae_set_error("vq_loss_finalize: workspace %zu < %zu bytes", workspace_bytes, sizeof(double) * FINISH_CAP);
    return ODVAE_ERR_WORKSPACE;
  }
  const double scale = (1.0 + (double)beta) / ((double)M * (double)D);
  hipLaunchKernelGGL(vq_loss_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, p.finish_blocks, scale, loss);
  ODVAE_LAUNCH_CHECK("vq_loss_final");
  return ODVAE_OK;
}

size_t odvae_vq_backward_workspace_bytes(int64_t M, int K, int D) {
  if (M < 1 || M > 0x7FFFFFFFLL || K < 1 || K > VQ_MAX_K || D < 1 || D > VQ_MAX_D) return 0;
  return backward_ws(nullptr, M, K, make_sort_plan(M, K)).bytes;
}

int odvae_vq_backward_f32(const float* z, const float* gq, float* dz, int64_t sn, int64_t sc, int64_t sp, int64_t N, int64_t HW, int D,
                          const float* E, int K, const int64_t* idx, const float* gl, float beta, int legacy, float* dE, void* workspace,
                          size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(N >= 1 && HW >= 1 && N <= 0x7FFFFFFFLL / HW, "vq_backward: N=%lld HW=%lld: needs 1 <= N HW < 2^31", (long long)N, (long long)HW);
  const int64_t M = N * HW;
  if (!sizes_ok("vq_backward", M, K, D)) return ODVAE_ERR_ARG;
  ODVAE_CHECK_ARG(z && E && idx, "vq_backward: null pointer");
  ODVAE_CHECK_ARG(strides_ok(sn, sc, sp), "vq_backward: strides must be positive");
  hipStream_t st = (hipStream_t)stream;
  const Strides zs{sn, sc, sp};
  const double md = (double)M * (double)D;
  const double cz = legacy ? 1.0 : (double)beta, ce = legacy ? (double)beta : 1.0;
  if (dE) {       // checked before anything is launched
    ODVAE_CHECK_ARG(workspace, "vq_backward: null workspace");
    const size_t need = backward_ws(nullptr, M, K, make_sort_plan(M, K)).bytes;
    if (workspace_bytes < need) {
      odvae_set_error("vq_backward: workspace %zu < %zu bytes", workspace_bytes, need);
      return ODVAE_ERR_WORKSPACE;
    }
  }
  if (dz) {
    hipLaunchKernelGGL(vq_dz_kernel, dim3(grid_1d(M)), dim3(256), 0, st, z, gq, dz, zs, M, HW, D, E, K, idx, gl, 2.0 * cz / md);
    ODVAE_LAUNCH_CHECK("vq_dz");
  }
  if (dE) {
    const SortPlan p = make_sort_plan(M, K);
    const BackwardWs w = backward_ws(workspace, M, K, p);
    hipLaunchKernelGGL(vq_sort_kernel<false>, dim3(p.nb, p.S), dim3(256), 0, st, idx, M, K, p.kb, p.rs, w.seg, (const int*)nullptr, (int*)nullptr);
    ODVAE_LAUNCH_CHECK("vq_sort_count");
    hipLaunchKernelGGL(vq_sort_scan_kernel, dim3(1), dim3(1024), 0, st, w.seg, K, p.S, w.cnt, w.off);
    ODVAE_LAUNCH_CHECK("vq_sort_scan");
    hipLaunchKernelGGL(vq_sort_kernel<true>, dim3(p.nb, p.S), dim3(256), 0, st, idx, M, K, p.kb, p.rs, w.seg, (const int*)w.off, w.perm);
    ODVAE_LAUNCH_CHECK("vq_sort_fill");
    int dp = 1;
    while (dp < D && dp < 256) dp <<= 1;
    hipLaunchKernelGGL(vq_segsum_kernel, dim3(K), dim3(256), 0, st, z, zs, HW, D, E, (const int*)w.cnt, (const int*)w.off, (const int*)w.perm, gl,
                       2.0 * ce / md, dp, dE);
    ODVAE_LAUNCH_CHECK("vq_segsum");
  }
  return ODVAE_OK;
}

int odvae_vq_gather_f32(const int64_t* idx, int64_t N, int64_t HW, const float* E, int K, int D, float* out, int64_t o_sn, int64_t o_sc,
                        int64_t o_sp, void* stream) {
  ODVAE_CHECK_ARG(N >= 1 && HW >= 1 && N <= 0x7FFFFFFFLL / HW, "vq_gather: N=%lld HW=%lld: needs 1 <= N HW < 2^31", (long long)N, (long long)HW);
  const int64_t M = N * HW;
  if (!sizes_ok("vq_gather", M, K, D)) return ODVAE_ERR_ARG;
  ODVAE_CHECK_ARG(idx && E && out, "vq_gather: null pointer");
  ODVAE_CHECK_ARG(strides_ok(o_sn, o_sc, o_sp), "vq_gather: strides must be positive");
  const Strides os{o_sn, o_sc, o_sp};
  hipLaunchKernelGGL(vq_gather_kernel, dim3(grid_1d(M)), dim3(256), 0, (hipStream_t)stream, idx, M, HW, E, K, D, out, os);
  ODVAE_LAUNCH_CHECK("vq_gather");
  return ODVAE_OK;
}

int odvae_vq_usage(const int64_t* idx, int64_t M, int K, int* counts, float* out, void* stream) {
  if (!sizes_ok("vq_usage", M, K, 1)) return ODVAE_ERR_ARG;
  ODVAE_CHECK_ARG(idx && counts && out, "vq_usage: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, sizeof(int) * (size_t)K, st) != hipSuccess) {
    odvae_set_error("vq_usage: hipMemsetAsync failed");
    return ODVAE_ERR_HIP;
  }
  hipLaunchKernelGGL(vq_count_kernel, dim3(grid_1d(M)), dim3(256), 0, st, idx, M, K, counts);
  ODVAE_LAUNCH_CHECK("vq_count");
  hipLaunchKernelGGL(vq_usage_final_kernel, dim3(1), dim3(256), 0, st, (const int*)counts, K, 1.0 / (double)M, out);
  ODVAE_LAUNCH_CHECK("vq_usage_final");
  return ODVAE_OK;
}

}  // extern "C"
