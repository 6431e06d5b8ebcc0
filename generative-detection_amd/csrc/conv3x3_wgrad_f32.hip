// Weight (and bias) gradient of the 3x3 convolutions, NHWC, exact f32 on the matrix cores.
//
// dW[co][ci][kh][kw] = sum over (n, oy, ox) of xs(n,oy,ox;kh,kw)[ci] * dy[n][oy][ox][co], where xs
// is the input pixel the forward pass of that mode reads (zero outside the image):
//   MODE 0 stride 1 pad 1 | MODE 1 pad(0,1,0,1)+stride 2 | MODE 2 nearest-2x-upsample + stride 1 pad 1
// ([UPSTREAM] ldm/modules/diffusionmodules/model.py ResnetBlock / Downsample / Upsample convs; what
// loss.backward() computes for them in the reference, src/models/autoencoder.py:295-330).
//
// GEMM view per tap: M = ci, N = co, K = pixels (up to N*Ho*Wo = 2M).  A block owns a ci x co slice of all taps and a
// contiguous range of pixel tiles (split = blockIdx.x); blocks write partial slabs [split][tap][CinP][CoutP], a second
// kernel sums them in a fixed order (deterministic) and writes OIHW.  db = column sums of dy ride along in the
// ci-tile-0 blocks.
//
// Map of the file.  kind is what odvae_conv3x3_wgrad_plan reports; make_plan chooses it from the mode and the channel counts alone:
//   kind | kernel(s)                                   | block, pixel tile                | chosen when
//   0    | conv3x3_wgrad_thin_kernel, thin_colsum_kernel,| 128 wide channels, whole image   | thin_applies: mode 0, Cin <= 4 or Cout <= 4 (conv_in,
//        | conv3x3_wgrad_thin_reduce_kernel             | rows, no LDS                     | conv_out), W % 16 == 0, the wide side % 4 == 0 and >= 32
//   1 v1 | conv3x3_wgrad_kernel<MODE, TH>               | 64 ci x 64 co, 8 x 16 (mode 1:   | everything else: Cin % 4 or Cout % 4 != 0, or Cout <= 64;
//        |                                              | 4 x 16), 256 threads, 1024 blocks| mode 5 with such channel counts runs MODE 2
//   2 v2 | conv3x3_wgrad_dma_kernel<MODE, TH>           | 64 ci x 128 co, 4 x 16 (mode 1:  | modes 0, 1, 2 with Cin % 4 == Cout % 4 == 0 and Cout > 64
//        | conv3x3_wgrad_down_split_kernel (mode 1)     | 2 x 16), 512 threads, 256 blocks | split form: selector 1, or -1 and direct_split_by_shape
//   3 up | conv3x3_wgrad_up_kernel                      | 64 ci x 64 co x 4 parity classes,| mode 5 with Cin % 4 == Cout % 4 == 0
//        | conv3x3_wgrad_up_split_kernel                | 2 x 16 low-res, 512 thr, 256 blk | split form: as for kind 2
// Kinds 1 and 2 end in conv3x3_wgrad_reduce_kernel (9 taps, 1 bias row per split), kind 3 in conv3x3_wgrad_up_reduce_kernel
// (16 parity taps, 4 bias rows per split): slab_taps / bias_rows.  The split forms keep their f32 kernel's plan, slabs and
// reduction and replace each f32 product by six bf16 products of exactly split operands (bf16_common.h, split3);
// odvae_conv3x3_wgrad_select sets the selector (default -1: by shape).  Helpers shared by the block kernels come first.
#include "bf16_common.h"

namespace {

constexpr int TW = 16;
constexpr int BC = 64;  // channels per block on both axes

struct WgradParams {
  const float* x;    // [N][Hi][Wi][Cin]
  const float* dy;   // [N][Ho][Wo][Cout]
  float* slab;       // [nsplit][9][CinP][CoutP]
  float* bslab;      // [nsplit][CoutP] or null
  int N, Hi, Wi, Cin, Ho, Wo, Cout, CinP, CoutP;
  int tiles_x, tiles_y, ntiles, tiles_per_split, ci_tiles;
};

template <int MODE, int TH> struct Halo;
template <int TH> struct Halo<0, TH> { static constexpr int H = TH + 2, W = TW + 2; };
template <int TH> struct Halo<1, TH> { static constexpr int H = 2 * TH + 1, W = 2 * TW + 1; };
template <int TH> struct Halo<2, TH> { static constexpr int H = TH / 2 + 2, W = TW / 2 + 2; };

template <int MODE, int TH>
__device__ __forceinline__ int halo_index(int r, int c, int kh, int kw) {
  if (MODE == 0) return (r + kh) * Halo<0, TH>::W + (c + kw);
  if (MODE == 1) return (2 * r + kh) * Halo<1, TH>::W + (2 * c + kw);
  return ((r + kh + 1) >> 1) * Halo<2, TH>::W + ((c + kw + 1) >> 1);
}

// ---- steps every block kernel takes ------------------------------------------------------------------------------
// pixel tile `tile` of the plan: image n, tile row ty, tile column tx
struct Tile { int n, ty, tx; };
__device__ __forceinline__ Tile tile_decode(const WgradParams& p, int tile) {
  Tile t;
  t.tx = tile % p.tiles_x; tile /= p.tiles_x;
  t.ty = tile % p.tiles_y; t.n = tile / p.tiles_y;
  return t;
}

// raw buffer over `bytes` bytes (below 2 GiB) from base: a lane whose offset is >= bytes, OOB for one, loads 0 and stores nothing
constexpr unsigned OOB = 0x7FFFFFF0u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t f32_rsrc(const float* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, bytes, 0x00020000);
}
// image n of x and of dy (the launcher keeps one image below 2 GiB)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t x_rsrc(const WgradParams& p, int n) {
  return f32_rsrc(p.x + (int64_t)n * p.Hi * p.Wi * p.Cin, p.Hi * p.Wi * p.Cin * 4);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t dy_rsrc(const WgradParams& p, int n) {
  return f32_rsrc(p.dy + (int64_t)n * p.Ho * p.Wo * p.Cout, p.Ho * p.Wo * p.Cout * 4);
}

template <int NT>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
}

// Slab stores of the LDS-DMA family: this split's slab [taps][CinP][CoutP] as one buffer, 32-bit offsets into it, the tap
// stride in the scalar offset (no per-element address arithmetic).  Precondition, checked by the launcher (slab_fits): one
// split's slab, taps * CinP * CoutP * 4 bytes, stays below 2^31, or num_records and the offsets would wrap.
// store_taps: NT taps from tap0 on of the 32 x 32 sub-tile at rows ci_base.., column co (lane = co).
template <int NT>
__device__ __forceinline__ void store_taps(__amdgpu_buffer_rsrc_t srsrc, const WgradParams& p, const f32x16 (&acc)[NT],
                                           int tap0, int ci_base, int co, int lane) {
  const int tap_stride = p.CinP * p.CoutP * 4;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const unsigned rowoff = (unsigned)((ci_base + acc_row(r, lane)) * p.CoutP + co) * 4u;
#pragma unroll
    for (int t = 0; t < NT; ++t)
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[t][r]), srsrc, rowoff, (tap0 + t) * tap_stride, 0);
  }
}
// slab [split][tap][CinP][CoutP]
__device__ __forceinline__ void store_slab9(const WgradParams& p, int split, const f32x16 (&acc)[9], int ci_base, int co, int lane) {
  store_taps(f32_rsrc(p.slab + (int64_t)split * 9 * p.CinP * p.CoutP, 9 * p.CinP * p.CoutP * 4), p, acc, 0, ci_base, co, lane);
}
// slab [split][cls * 4 + tap][CinP][CoutP]: both ci sub-tiles of parity class cls
__device__ __forceinline__ void store_slab_parity(const WgradParams& p, int split, const f32x16 (&acc)[2][4], int cls, int ci0, int co, int lane) {
  const __amdgpu_buffer_rsrc_t srsrc = f32_rsrc(p.slab + (int64_t)split * 16 * p.CinP * p.CoutP, 16 * p.CinP * p.CoutP * 4);
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) store_taps(srsrc, p, acc[mt], cls * 4, ci0 + mt * 32, co, lane);
}

// the lane halves hold the sums over the even and the odd pixels of column co: added, lane half 0 stores row `row` of the bias slab
__device__ __forceinline__ void store_bias(const WgradParams& p, int row, int co, int h, float bsum) {
  bsum += __shfl_xor(bsum, 32, 64);
  if (h == 0) p.bslab[(int64_t)row * p.CoutP + co] = bsum;
}

template <int MODE, int TH>
__global__ __launch_bounds__(256) void conv3x3_wgrad_kernel(WgradParams p) {
  constexpr int HPIX = Halo<MODE, TH>::H * Halo<MODE, TH>::W;
  constexpr int NPIX = TH * TW;
  constexpr int HALO_F4 = HPIX * (BC / 4), HALO_IT = (HALO_F4 + 255) / 256;
  constexpr int DY_F4 = NPIX * (BC / 4), DY_IT = (DY_F4 + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Xs = smem;                 // [HPIX][BC]
  float* Ds = smem + HPIX * BC;     // [NPIX][BC]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, h = lane >> 5;
  const int split = blockIdx.x;
  const int ci_tile = blockIdx.y % p.ci_tiles, co_tile = blockIdx.y / p.ci_tiles;
  const int ci0 = ci_tile * BC, co0 = co_tile * BC;
  const bool xvec = (p.Cin & 3) == 0, dvec = (p.Cout & 3) == 0;
  const bool do_bias = p.bslab != nullptr && ci_tile == 0 && wm == 0;

  f32x16 acc[9];
  zero_acc(acc);
  float bsum = 0.f;

  const int t_beg = split * p.tiles_per_split;
  const int t_end = min(p.ntiles, t_beg + p.tiles_per_split);
  for (int tile = t_beg; tile < t_end; ++tile) {
    const Tile tl = tile_decode(p, tile);
    const int oy0 = tl.ty * TH, ox0 = tl.tx * TW;
    int iy0, ix0;
    if (MODE == 0) { iy0 = oy0 - 1; ix0 = ox0 - 1; }
    else if (MODE == 1) { iy0 = 2 * oy0; ix0 = 2 * ox0; }
    else { iy0 = oy0 / 2 - 1; ix0 = ox0 / 2 - 1; }
    const float* xn = p.x + (int64_t)tl.n * p.Hi * p.Wi * p.Cin;
    const float* dn = p.dy + (int64_t)tl.n * p.Ho * p.Wo * p.Cout;

    __syncthreads();  // previous tile's reads are done
#pragma unroll
    for (int i = 0; i < HALO_IT; ++i) {
      const int f = tid + 256 * i;
      if (f < HALO_F4) {
        const int hp = f / (BC / 4), q = f % (BC / 4);
        const int iy = iy0 + hp / Halo<MODE, TH>::W, ix = ix0 + hp % Halo<MODE, TH>::W;
        const int c = ci0 + 4 * q;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi && c < p.Cin) {
          const float* src = xn + ((int64_t)iy * p.Wi + ix) * p.Cin + c;
          if (xvec) v = *reinterpret_cast<const float4*>(src);
          else {
            v.x = src[0];
            if (c + 1 < p.Cin) v.y = src[1];
            if (c + 2 < p.Cin) v.z = src[2];
            if (c + 3 < p.Cin) v.w = src[3];
          }
        }
        *reinterpret_cast<float4*>(Xs + hp * BC + 4 * q) = v;
      }
    }
#pragma unroll
    for (int i = 0; i < DY_IT; ++i) {
      const int f = tid + 256 * i;
      if (f < DY_F4) {
        const int px = f / (BC / 4), q = f % (BC / 4);
        const int oy = oy0 + px / TW, ox = ox0 + px % TW;
        const int c = co0 + 4 * q;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (oy < p.Ho && ox < p.Wo && c < p.Cout) {
          const float* src = dn + ((int64_t)oy * p.Wo + ox) * p.Cout + c;
          if (dvec) v = *reinterpret_cast<const float4*>(src);
          else {
            v.x = src[0];
            if (c + 1 < p.Cout) v.y = src[1];
            if (c + 2 < p.Cout) v.z = src[2];
            if (c + 3 < p.Cout) v.w = src[3];
          }
        }
        *reinterpret_cast<float4*>(Ds + px * BC + 4 * q) = v;
      }
    }
    __syncthreads();

    const float* xa = Xs + wm * 32 + li;
    const float* db = Ds + wn * 32 + li;
#pragma unroll 4
    for (int s = 0; s < NPIX / 2; ++s) {
      const int px = 2 * s + h;
      const int r = px / TW, c = px % TW;
      const float b = db[px * BC];
      if (do_bias) bsum += b;
#pragma unroll
      for (int t9 = 0; t9 < 9; ++t9) {
        const float a = xa[halo_index<MODE, TH>(r, c, t9 / 3, t9 % 3) * BC];
        acc[t9] = mfma32(a, b, acc[t9]);
      }
    }
  }

  // partial slab: [split][tap][ci][co], lane = co
  const int co = co0 + wn * 32 + li;
  float* sl = p.slab + (int64_t)split * 9 * p.CinP * p.CoutP;
#pragma unroll
  for (int t9 = 0; t9 < 9; ++t9)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ci = ci0 + wm * 32 + acc_row(r, lane);
      sl[((int64_t)t9 * p.CinP + ci) * p.CoutP + co] = acc[t9][r];
    }
  if (do_bias) {      // store_bias, written out: through the helper this kernel takes 8 to 10 VGPRs more (profiles/wgrad_direct_refactor.md)
    bsum += __shfl_xor(bsum, 32, 64);
    if (h == 0) p.bslab[(int64_t)split * p.CoutP + co] = bsum;
  }
}

// ---- v2: LDS-DMA staging, double-buffered -------------------------------------------------------------------
// Block = 512 threads = 8 waves (2 ci x 4 co sub-tiles of 32x32, all 9 taps each): 64 ci x 128 co per block.
// The halo patch [HPIX][64 ci] and the dy tile [NPIX][128 co] of the NEXT pixel tile are fetched by
// buffer_load ... lds (1 KiB per wave-instruction, straight into LDS, no staging registers; out-of-image lanes
// point past the buffer's num_records and therefore write zeros) while the current tile is multiplied:
// one barrier per tile, every byte of a tile in flight at once, 2 waves per SIMD.  Needs Cin % 4 == Cout % 4 == 0.
constexpr int BCI2 = 64, BCO2 = 128;

template <int MODE, int TH>
struct DmaGeom {
  static constexpr int HPIX = Halo<MODE, TH>::H * Halo<MODE, TH>::W;
  static constexpr int NPIX = TH * TW;
  static constexpr int NH = (HPIX * (BCI2 / 4) + 63) / 64;   // 1 KiB pieces of the halo image
  static constexpr int ND = NPIX * (BCO2 / 4) / 64;          // 1 KiB pieces of the dy image
  static constexpr int XS_F = NH * 256;                      // floats (halo image padded to whole pieces)
  static constexpr int BUF_F = XS_F + NPIX * BCO2;
};

typedef __attribute__((address_space(3))) void* lds_ptr_t;

template <int MODE, int TH>
__global__ __launch_bounds__(512, 2) void conv3x3_wgrad_dma_kernel(WgradParams p) {
  using G = DmaGeom<MODE, TH>;
  extern __shared__ __attribute__((aligned(16))) float smem[];   // 2 * BUF_F floats

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int li = lane & 31, h = lane >> 5;
  const int split = blockIdx.x;
  const int ci_tile = blockIdx.y % p.ci_tiles, co_tile = blockIdx.y / p.ci_tiles;
  const int ci0 = ci_tile * BCI2, co0 = co_tile * BCO2;
  const bool do_bias = p.bslab != nullptr && ci_tile == 0 && wm == 0;

  f32x16 acc[9];
  zero_acc(acc);
  float bsum = 0.f;

  auto issue = [&](int tile, int buf) {
    const Tile tl = tile_decode(p, tile);
    const int oy0 = tl.ty * TH, ox0 = tl.tx * TW;
    int iy0, ix0;
    if (MODE == 0) { iy0 = oy0 - 1; ix0 = ox0 - 1; }
    else if (MODE == 1) { iy0 = 2 * oy0; ix0 = 2 * ox0; }
    else { iy0 = oy0 / 2 - 1; ix0 = ox0 / 2 - 1; }
    const __amdgpu_buffer_rsrc_t rx = x_rsrc(p, tl.n), rd = dy_rsrc(p, tl.n);
    float* base = smem + buf * G::BUF_F;
    for (int j = wave; j < G::NH + G::ND; j += 8) {
      if (j < G::NH) {
        const int f = j * 64 + lane;
        const int hp = f >> 4, q = f & 15;
        const int iy = iy0 + hp / Halo<MODE, TH>::W, ix = ix0 + hp % Halo<MODE, TH>::W;
        const int c = ci0 + 4 * q;
        const bool ok = hp < G::HPIX && iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi && c < p.Cin;
        const unsigned voff = ok ? (unsigned)(((iy * p.Wi + ix) * p.Cin + c) * 4) : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_ptr_t)(base + j * 256), 16, voff, 0, 0, 0);
      } else {
        const int jj = j - G::NH;
        const int f = jj * 64 + lane;
        const int px = f >> 5, q = f & 31;
        const int oy = oy0 + px / TW, ox = ox0 + px % TW;
        const int c = co0 + 4 * q;
        const bool ok = oy < p.Ho && ox < p.Wo && c < p.Cout;
        const unsigned voff = ok ? (unsigned)(((oy * p.Wo + ox) * p.Cout + c) * 4) : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, (lds_ptr_t)(base + G::XS_F + jj * 256), 16, voff, 0, 0, 0);
      }
    }
  };

  const int t_beg = split * p.tiles_per_split;
  const int ntl = min(p.ntiles, t_beg + p.tiles_per_split) - t_beg;
  if (ntl > 0) issue(t_beg, 0);
  for (int it = 0; it < ntl; ++it) {
    const int cur = it & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of tile `it` have landed
    __syncthreads();                                    // everyone's have; buffer cur^1 is free again
    if (it + 1 < ntl) issue(t_beg + it + 1, cur ^ 1);
    // lane half h takes pixel 2s+h of k-step s; TW is even, so both halves sit in the same tile row
    const float* xa = smem + cur * G::BUF_F + wm * 32 + li + h * BCI2;            // [HPIX][64]
    const float* db = smem + cur * G::BUF_F + G::XS_F + wn * 32 + li + h * BCO2;  // [NPIX][128]
    auto load_step = [&](int s, float (&a)[9], float& b) {
      const int r = (2 * s) / TW, c = (2 * s) % TW;   // compile-time after unrolling
      b = db[2 * s * BCO2];
#pragma unroll
      for (int t9 = 0; t9 < 9; ++t9) {
        // halo_index is affine in c for every mode's even/odd pixel pair except MODE 2 (c >> 1): handle h there
        int idx;
        if (MODE == 2) idx = ((r + t9 / 3 + 1) >> 1) * Halo<2, TH>::W;   // column part added per lane below
        else idx = halo_index<MODE, TH>(r, c, t9 / 3, t9 % 3);
        if (MODE == 2) a[t9] = (xa - h * BCI2)[(idx + ((c + h + t9 % 3 + 1) >> 1)) * BCI2];
        else a[t9] = xa[idx * BCI2 + (MODE == 1 ? h * BCI2 : 0)];        // MODE 1: pixel step is 2 halo columns
      }
    };
    float ac[9], an[9], bc, bn = 0.f;
    load_step(0, ac, bc);
#pragma unroll
    for (int s = 0; s < G::NPIX / 2; ++s) {
      // software pipeline, pinned: k-step s+1's ten LDS reads are in flight behind step s's nine MFMAs
      if (s + 1 < G::NPIX / 2) load_step(s + 1, an, bn);
      __builtin_amdgcn_sched_barrier(0);
      if (do_bias) bsum += bc;
#pragma unroll
      for (int t9 = 0; t9 < 9; ++t9) acc[t9] = mfma32(ac[t9], bc, acc[t9]);
      __builtin_amdgcn_sched_barrier(0);
      bc = bn;
#pragma unroll
      for (int t9 = 0; t9 < 9; ++t9) ac[t9] = an[t9];
    }
  }

  const int co = co0 + wn * 32 + li;
  store_slab9(p, split, acc, ci0 + wm * 32, co, lane);
  if (do_bias) store_bias(p, split, co, h, bsum);
}

// bias tail of both reduce kernels: dbias[co] = the bias slab's rows (brows per split), added in their order
__device__ __forceinline__ float bias_sum(const float* __restrict__ bslab, int rows, int co, int CoutP) {
  float s = 0.f;
  for (int sp = 0; sp < rows; ++sp) s += bslab[(int64_t)sp * CoutP + co];
  return s;
}

__global__ void conv3x3_wgrad_reduce_kernel(const float* __restrict__ slab, const float* __restrict__ bslab,
                                            int nsplit, int brows, int Cin, int Cout, int CinP, int CoutP,
                                            float* __restrict__ dw, float* __restrict__ dbias) {
  const int64_t per = (int64_t)9 * CinP * CoutP;
  const int64_t total = per + (dbias ? CoutP : 0);
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    if (idx < per) {
      const int co = (int)(idx % CoutP);
      const int ci = (int)((idx / CoutP) % CinP);
      const int tap = (int)(idx / ((int64_t)CoutP * CinP));
      if (co < Cout && ci < Cin) {
        float sk[4] = {0.f, 0.f, 0.f, 0.f};      // four independent chains: one chain of nsplit dependent round trips otherwise
        int sp = 0;
        for (; sp + 3 < nsplit; sp += 4) {
#pragma unroll
          for (int j = 0; j < 4; ++j) sk[j] += slab[(sp + j) * per + idx];
        }
        for (; sp < nsplit; ++sp) sk[0] += slab[sp * per + idx];
        dw[((int64_t)co * Cin + ci) * 9 + tap] = (sk[0] + sk[1]) + (sk[2] + sk[3]);
      }
    } else {
      const int co = (int)(idx - per);
      if (co < Cout) dbias[co] = bias_sum(bslab, nsplit * brows, co, CoutP);
    }
  }
}

// ---- Upsample conv (nearest 2x + 3x3) by output parity class ---------------------------------------------------
// dWeff[cls][a][b] = sum over low-res pixels (y, x) of x[y + py - 1 + a][x + px - 1 + b]^T dy[2y + py][2x + px], cls = 2 py + px:
// 16 tap-products per low-res pixel instead of the 36 of the dense form (the forward pass multiplies the same
// pre-summed weights, conv3x3_f32.hip mode 5); dW[kh][kw] is the sum of the four dWeff entries whose pre-sum contains
// W[kh][kw].  Block = 64 ci x 64 co, 8 waves = 4 classes x 2 co sub-tiles, each wave both ci sub-tiles x 4 taps
// (128 accumulator registers); pixel tile = 2 x 16 low-res pixels: halo [4 x 18][64 ci] and the four parity planes of
// the 4 x 32 dy patch [cls][32 px][64 co] arrive by LDS-DMA, double-buffered, one barrier per tile.
constexpr int UP_TH = 2, UP_BC = 64;
struct UpGeom {
  static constexpr int HALO_W = TW + 2, HPIX = (UP_TH + 2) * HALO_W;   // 72
  static constexpr int NPIX = UP_TH * TW;                             // 32 low-res pixels
  static constexpr int NH = (HPIX * (UP_BC / 4) + 63) / 64;           // 1 KiB pieces of the halo image
  static constexpr int ND = 4 * NPIX * (UP_BC / 4) / 64;              // 1 KiB pieces of the dy planes
  static constexpr int XS_F = NH * 256;
  static constexpr int BUF_F = XS_F + 4 * NPIX * UP_BC;
};

__global__ __launch_bounds__(512, 2) void conv3x3_wgrad_up_kernel(WgradParams p) {
  using G = UpGeom;
  extern __shared__ __attribute__((aligned(16))) float smem[];   // 2 * BUF_F floats

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cls = wave >> 1, wn = wave & 1, py = cls >> 1, px = cls & 1;
  const int li = lane & 31, h = lane >> 5;
  const int split = blockIdx.x;
  const int ci_tile = blockIdx.y % p.ci_tiles, co_tile = blockIdx.y / p.ci_tiles;
  const int ci0 = ci_tile * UP_BC, co0 = co_tile * UP_BC;
  const bool do_bias = p.bslab != nullptr && ci_tile == 0;

  f32x16 acc[2][4];
  zero_acc(acc[0]); zero_acc(acc[1]);
  float bsum = 0.f;

  auto issue = [&](int tile, int buf) {
    const Tile tl = tile_decode(p, tile);
    const int ly0 = tl.ty * UP_TH, lx0 = tl.tx * TW;
    const __amdgpu_buffer_rsrc_t rx = x_rsrc(p, tl.n), rd = dy_rsrc(p, tl.n);
    float* base = smem + buf * G::BUF_F;
    for (int j = wave; j < G::NH + G::ND; j += 8) {
      if (j < G::NH) {
        const int f = j * 64 + lane;
        const int hp = f >> 4, q = f & 15;
        const int iy = ly0 - 1 + hp / G::HALO_W, ix = lx0 - 1 + hp % G::HALO_W;
        const int c = ci0 + 4 * q;
        const bool ok = hp < G::HPIX && iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi && c < p.Cin;
        const unsigned voff = ok ? (unsigned)(((iy * p.Wi + ix) * p.Cin + c) * 4) : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_ptr_t)(base + j * 256), 16, voff, 0, 0, 0);
      } else {
        const int jj = j - G::NH;
        const int f = jj * 64 + lane;
        const int pp = f >> 4, q = f & 15;              // pp = plane * 32 + low-res pixel of the tile
        const int plane = pp >> 5, pl = pp & 31;
        const int oy = 2 * (ly0 + pl / TW) + (plane >> 1), ox = 2 * (lx0 + pl % TW) + (plane & 1);
        const int c = co0 + 4 * q;
        const bool ok = oy < p.Ho && ox < p.Wo && c < p.Cout;
        const unsigned voff = ok ? (unsigned)(((oy * p.Wo + ox) * p.Cout + c) * 4) : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rd, (lds_ptr_t)(base + G::XS_F + jj * 256), 16, voff, 0, 0, 0);
      }
    }
  };

  const int t_beg = split * p.tiles_per_split;
  const int ntl = min(p.ntiles, t_beg + p.tiles_per_split) - t_beg;
  if (ntl > 0) issue(t_beg, 0);
  for (int it = 0; it < ntl; ++it) {
    const int cur = it & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of tile `it` have landed
    __syncthreads();                                    // everyone's have; buffer cur^1 is free again
    if (it + 1 < ntl) issue(t_beg + it + 1, cur ^ 1);
    // lane half h takes low-res pixel 2s+h of k-step s (same tile row: TW is even); the class offset is wave-uniform
    const float* xa = smem + cur * G::BUF_F + ((py * G::HALO_W + px) + h) * UP_BC + li;                 // [HPIX][64]
    const float* db = smem + cur * G::BUF_F + G::XS_F + (cls * G::NPIX + h) * UP_BC + wn * 32 + li;     // [4][32][64]
    auto load_step = [&](int s, float (&a)[2][4], float& b) {
      const int r = (2 * s) / TW, c = (2 * s) % TW;   // compile-time after unrolling
      b = db[2 * s * UP_BC];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) a[mt][t] = xa[((r + t / 2) * G::HALO_W + c + t % 2) * UP_BC + mt * 32];
    };
    float ac[2][4], an[2][4], bc, bn = 0.f;
    load_step(0, ac, bc);
#pragma unroll
    for (int s = 0; s < G::NPIX / 2; ++s) {
      if (s + 1 < G::NPIX / 2) load_step(s + 1, an, bn);
      __builtin_amdgcn_sched_barrier(0);
      bsum += bc;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) acc[mt][t] = mfma32(ac[mt][t], bc, acc[mt][t]);
      __builtin_amdgcn_sched_barrier(0);
      bc = bn;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) ac[mt][t] = an[mt][t];
    }
  }

  const int co = co0 + wn * 32 + li;
  store_slab_parity(p, split, acc, cls, ci0, co, lane);
  if (do_bias) store_bias(p, split * 4 + cls, co, h, bsum);
}

// dW[kh][kw] = sum of the dWeff entries (py, a) x (px, b) with kh in R(py, a), kw in R(px, b):
// kh = 0: (0,0) (1,0) | kh = 1: (0,1) (1,0) | kh = 2: (0,1) (1,1); splits summed in a fixed order
__global__ void conv3x3_wgrad_up_reduce_kernel(const float* __restrict__ slab, const float* __restrict__ bslab,
                                               int nsplit, int brows, int Cin, int Cout, int CinP, int CoutP,
                                               float* __restrict__ dw, float* __restrict__ dbias) {
  const int64_t mat = (int64_t)CinP * CoutP;
  const int64_t per = 9 * mat;
  const int64_t total = per + (dbias ? CoutP : 0);
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    if (idx < per) {
      const int co = (int)(idx % CoutP);
      const int ci = (int)((idx / CoutP) % CinP);
      const int tap = (int)(idx / mat);
      if (co < Cout && ci < Cin) {
        const int kh = tap / 3, kw = tap % 3;
        const int pa[2][2] = {{0, kh == 0 ? 0 : 1}, {1, kh == 2 ? 1 : 0}};   // (py, a) pairs for kh
        const int pb[2][2] = {{0, kw == 0 ? 0 : 1}, {1, kw == 2 ? 1 : 0}};   // (px, b) pairs for kw
        float sq[2][2] = {{0.f, 0.f}, {0.f, 0.f}};      // one chain per (i, j) term: four loads in flight per split instead of one chain
        for (int sp = 0; sp < nsplit; ++sp)
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const int t16 = (pa[i][0] * 2 + pb[j][0]) * 4 + pa[i][1] * 2 + pb[j][1];
              sq[i][j] += slab[((int64_t)sp * 16 + t16) * mat + (int64_t)ci * CoutP + co];
            }
        dw[((int64_t)co * Cin + ci) * 9 + tap] = (sq[0][0] + sq[0][1]) + (sq[1][0] + sq[1][1]);
      }
    } else {
      const int co = (int)(idx - per);
      if (co < Cout) dbias[co] = bias_sum(bslab, nsplit * brows, co, CoutP);
    }
  }
}

// ---- Upsample conv by output parity class, bf16-split form -------------------------------------------------------
// conv3x3_wgrad_up_kernel's plan, blocks, wave roles, slabs and reduction; only a tile's products change: every f32 value of the
// halo and of the dy patch is split exactly into three bf16 (split8's arithmetic), and per tap the six products of
// gemm_f32_split.hip, in its order (smallest first), go through v_mfma_f32_32x32x16_bf16 with f32 accumulation.  That instruction
// wants 8 consecutive k in a lane, k being the pixel along a tile row.  Any one-to-one map of k to pixels will do as long as x and dy
// agree; the map here is k = 8 h + j <-> low-res tile column 2 j + h (h = lane half), the f32 kernel's own pairing of lane halves and
// pixels.  Two things follow:
//   dy: the thread that holds B's fragment for (class, row, co, h) is the one that fetches those eight pixels: lane = co, 128
//       contiguous bytes per lane half.  dy never goes through LDS, and the thread's values, added in the order they were loaded,
//       are the f32 kernel's bias chain: dbias keeps its bits.
//   x:  tap column shift s = px + b reads halo columns 2 j + h + s: the even columns E[0..8] or the odd ones O[0..8] of the 18, from
//       element 0 or 1.  A thread fetches one parity of one halo row of one channel (9 loads, lane = channel: 256 contiguous bytes
//       per wave instruction), splits each value once and writes the runs [0..7] and [1..8] (the second is the first's packed words
//       moved on by 16 bits): LDS holds [buffer][plane][run E0 O0 E1 O1][halo row][channel][8 k] bf16 = 48 KB per buffer; lane
//       (li, h) reads run h + s, 512 contiguous bytes per lane half, so neither side has bank conflicts to arrange around.
// Two LDS buffers and the next tile's raw values in registers: one barrier per tile.
constexpr unsigned USP_RUN_B = 4 * 64 * 16;          // one run: 4 halo rows x 64 channels x 8 k
constexpr unsigned USP_PLANE_B = 4 * USP_RUN_B;      // 16 384
constexpr unsigned USP_BUF_B = 3 * USP_PLANE_B;      // 49 152

// dr[j] = dy row oy at tile column c = col0 + 2 j + h of `width` columns, which is dy pixel xs * c + xo; dch holds the lane's channel
// and its lane half's column.  A row or a column outside the image reads as 0 (offset past num_records; the scalar offset stays inside).
__device__ __forceinline__ void fetch_dy_row(__amdgpu_buffer_rsrc_t rd, const WgradParams& p, int oy, int col0, int width, int xs, int xo,
                                             unsigned dch, int h, float (&dr)[8]) {
  const int wleft = width - col0 - h;                        // columns 2 j + h < wleft are inside the image
  const bool row_ok = oy < p.Ho;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const bool sok = row_ok && col0 + 2 * j < width;         // wave-uniform: the h = 0 column is inside
    const unsigned soff = sok ? (unsigned)(oy * p.Wo + xs * (col0 + 2 * j) + xo) * ((unsigned)p.Cout * 4u) : 0u;
    dr[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rd, (sok && 2 * j < wleft) ? dch : OOB, soff, 0));
  }
}

__global__ __launch_bounds__(512, 2) void conv3x3_wgrad_up_split_kernel(WgradParams p) {
  extern __shared__ __attribute__((aligned(16))) char ssm[];   // 2 * USP_BUF_B

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cls = wave >> 1, wn = wave & 1, py = cls >> 1, px = cls & 1;
  const int li = lane & 31, h = lane >> 5;
  const int split = blockIdx.x;
  const int ci_tile = blockIdx.y % p.ci_tiles, co_tile = blockIdx.y / p.ci_tiles;
  const int ci0 = ci_tile * UP_BC, co0 = co_tile * UP_BC;
  const bool do_bias = p.bslab != nullptr && ci_tile == 0;

  f32x16 acc[2][4];
  zero_acc(acc[0]); zero_acc(acc[1]);
  float bsum = 0.f;

  // loader roles.  x: halo row xrow, column parity xu, channel ci0 + lane.  dy: this wave's class, rows 0 and 1, channel co0 + wn * 32
  // + li, low-res columns 2 j + h.  A lane past the channel count, a row or a column outside the image reads as 0 (offset past
  // num_records; the scalar offset stays inside the image).
  const int xrow = wave >> 1, xu = wave & 1;
  const unsigned cin4 = (unsigned)p.Cin * 4u;
  const unsigned xch = ci0 + lane < p.Cin ? (unsigned)(ci0 + lane) * 4u : OOB;
  const int co_l = co0 + wn * 32 + li;
  const unsigned dch = co_l < p.Cout ? (unsigned)co_l * 4u + (unsigned)h * 2u * ((unsigned)p.Cout * 4u) : OOB;

  float xr[9], dr[2][8];
  auto fetch = [&](int tile) {
    const Tile tl = tile_decode(p, tile);
    const int ly0 = tl.ty * UP_TH, lx0 = tl.tx * TW;
    const __amdgpu_buffer_rsrc_t rx = x_rsrc(p, tl.n), rd = dy_rsrc(p, tl.n);
    const int iy = ly0 - 1 + xrow;
    const bool xrow_ok = iy >= 0 && iy < p.Hi;
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      const int ix = lx0 - 1 + 2 * e + xu;
      const bool ok = xrow_ok && ix >= 0 && ix < p.Wi;      // wave-uniform
      const unsigned soff = ok ? (unsigned)(iy * p.Wi + ix) * cin4 : 0u;
      xr[e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, ok ? xch : OOB, soff, 0));
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) fetch_dy_row(rd, p, 2 * (ly0 + r) + py, lx0, p.Wi, 2, px, dch, h, dr[r]);
  };

  const unsigned lds0 = lds_addr_of(ssm);
  const unsigned xw = lds0 + (unsigned)(xu * 4 + xrow) * 1024u + (unsigned)lane * 16u;                 // run xu; run xu + 2 is 2 * USP_RUN_B on
  const unsigned adrA = lds0 + (unsigned)((h + px) * 4 + py) * 1024u + (unsigned)li * 16u;            // run h + px + b, halo row py + a + r
  constexpr split3::Order ORDER = split3::ORDER;      // (x plane, dy plane); the kernel's own copy: read in place, six VGPRs more (profiles/wgrad_direct_refactor.md)

  const int t_beg = split * p.tiles_per_split;
  const int ntl = min(p.ntiles, t_beg + p.tiles_per_split) - t_beg;
  if (ntl > 0) fetch(t_beg);
  for (int it = 0; it < ntl; ++it) {
    const unsigned buf = (unsigned)(it & 1) * USP_BUF_B;
    // the bias gradient's terms, unsplit, in the f32 kernel's order: pixel 2 s + h of k-step s = 0..15
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int j = 0; j < 8; ++j) bsum += dr[r][j];
    u32x4 bfr[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r) split8(dr[r], bfr[r]);
    {
      unsigned w[5][3];
#pragma unroll
      for (int i = 0; i < 4; ++i) split_pair(xr[2 * i], xr[2 * i + 1], w[i]);
      split_pair(xr[8], 0.f, w[4]);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        u32x4 v0, v1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v0[i] = w[i][q];
          v1[i] = __builtin_amdgcn_alignbit(w[i + 1][q], w[i][q], 16);
        }
        lds_st128(xw + buf + q * USP_PLANE_B, v0);
        lds_st128(xw + buf + q * USP_PLANE_B + 2 * USP_RUN_B, v1);
      }
    }
    if (it + 1 < ntl) fetch(t_beg + it + 1);
    __syncthreads();      // this tile's x runs are written; the other buffer's readers passed the previous barrier
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      bf16x8 b[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) b[q] = frag_from_u32x4(bfr[r][q]);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        bf16x8 a[2][3];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int q = 0; q < 3; ++q)
            a[mt][q] = frag_from_u32x4(lds_ld128(adrA + buf + q * USP_PLANE_B + (t % 2) * USP_RUN_B + (r + t / 2) * 1024u + mt * 512u));
#pragma unroll
        for (int o = 0; o < 6; ++o)
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) acc[mt][t] = mfma_bf16(a[mt][ORDER.p[o][0]], b[ORDER.p[o][1]], acc[mt][t]);
      }
    }
  }

  const int co = co0 + wn * 32 + li;
  store_slab_parity(p, split, acc, cls, ci0, co, lane);
  if (do_bias) store_bias(p, split * 4 + cls, co, h, bsum);
}

// ---- Downsample conv (pad (0, 1, 0, 1), stride 2), bf16-split form -------------------------------------------------
// conv3x3_wgrad_dma_kernel<1, 2>'s plan, blocks (64 ci x 128 co, 2 x 16 output pixels per tile), wave roles, slabs and reduction with
// the products of conv3x3_wgrad_up_split_kernel, and its k map: k = 8 h + j <-> tile column 2 j + h.  dy stays in the registers of the
// thread that fetched it (both ci halves fetch the same dy: the second read hits the cache) and gives the f32 kernel's bias chain.
// Tap column kw of lane half h reads halo columns 2 (2 j + h) + kw = 4 j + m, m = 2 h + kw = 0..4: the 33 halo columns by residue
// modulo 4, Q0[0..8], Q1, Q2, Q3[0..7]; m = 4 is Q0 from element 1.  With 144 accumulator registers per lane a whole tile's raw and
// split values do not fit beside them, so the loop steps by tile ROW (one k-step of nine taps): three halo rows per stage, the middle
// halo row of a tile fetched and split by both of its stages.  A loader unit is one (halo row, residue) of the 64 channels (lane =
// channel), 12 units over 8 waves; LDS holds [buffer][plane][run m][halo row][channel][8 k] bf16 = 45 KB per buffer, two buffers,
// one barrier per stage.
constexpr unsigned DSP_RUN_B = 3 * 64 * 16;          // one run: 3 halo rows x 64 channels x 8 k
constexpr unsigned DSP_PLANE_B = 5 * DSP_RUN_B;      // 15 360
constexpr unsigned DSP_BUF_B = 3 * DSP_PLANE_B;      // 46 080

__global__ __launch_bounds__(512, 2) void conv3x3_wgrad_down_split_kernel(WgradParams p) {
  extern __shared__ __attribute__((aligned(16))) char ssm[];   // 2 * DSP_BUF_B

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int li = lane & 31, h = lane >> 5;
  const int split = blockIdx.x;
  const int ci_tile = blockIdx.y % p.ci_tiles, co_tile = blockIdx.y / p.ci_tiles;
  const int ci0 = ci_tile * BCI2, co0 = co_tile * BCO2;
  const bool do_bias = p.bslab != nullptr && ci_tile == 0 && wm == 0;

  f32x16 acc[9];
  zero_acc(acc);
  float bsum = 0.f;

  const unsigned cin4 = (unsigned)p.Cin * 4u;
  const unsigned xch = ci0 + lane < p.Cin ? (unsigned)(ci0 + lane) * 4u : OOB;
  const int co_l = co0 + wn * 32 + li;
  const unsigned dch = co_l < p.Cout ? (unsigned)co_l * 4u + (unsigned)h * ((unsigned)p.Cout * 4u) : OOB;

  const int t_beg = split * p.tiles_per_split;
  const int nst = 2 * (min(p.ntiles, t_beg + p.tiles_per_split) - t_beg);      // stages: tile row st & 1 of tile t_beg + st / 2

  float xr[2][9], dr[8];      // x: units wave, wave + 8 (< 12): halo row unit >> 2 of the stage's three, residue unit & 3
  auto fetch = [&](int st) {
    const Tile tl = tile_decode(p, t_beg + (st >> 1));
    const int oy = tl.ty * 2 + (st & 1), ox0 = tl.tx * TW;
    const __amdgpu_buffer_rsrc_t rx = x_rsrc(p, tl.n), rd = dy_rsrc(p, tl.n);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int u = wave + 8 * i;
      if (u < 12) {
        const int iy = 2 * oy + (u >> 2), res = u & 3;
        const bool xrow_ok = iy < p.Hi;                        // the pad row below the image, and rows of a ragged tile, read as 0
#pragma unroll
        for (int e = 0; e < 9; ++e) {
          const int ix = 2 * ox0 + 4 * e + res;
          const bool ok = xrow_ok && ix < p.Wi && (e < 8 || res == 0);      // wave-uniform; the pad column right of the image reads as 0
          const unsigned soff = ok ? (unsigned)(iy * p.Wi + ix) * cin4 : 0u;
          xr[i][e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, ok ? xch : OOB, soff, 0));
        }
      }
    }
    fetch_dy_row(rd, p, oy, ox0, p.Wo, 1, 0, dch, h, dr);
  };

  const unsigned lds0 = lds_addr_of(ssm);
  const unsigned xw = lds0 + (unsigned)lane * 16u;
  const unsigned adrA = lds0 + (unsigned)h * 2u * DSP_RUN_B + (unsigned)(wm * 32 + li) * 16u;      // run 2 h + kw, halo row kh
  using namespace split3;      // ORDER: (x plane, dy plane)

  if (nst > 0) fetch(0);
  for (int st = 0; st < nst; ++st) {
    const unsigned buf = (unsigned)(st & 1) * DSP_BUF_B;
    if (do_bias) {      // the f32 kernel's chain: pixel 2 s + h of k-step s = 0..15, tile row st & 1 is s = 8 (st & 1) .. + 7
#pragma unroll
      for (int j = 0; j < 8; ++j) bsum += dr[j];
    }
    u32x4 bfr[3];
    split8(dr, bfr);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int u = wave + 8 * i;
      if (u < 12) {
        const int res = u & 3;
        const unsigned dst = xw + buf + (unsigned)(res * 3 + (u >> 2)) * 1024u;
        unsigned w[5][3];
#pragma unroll
        for (int k = 0; k < 4; ++k) split_pair(xr[i][2 * k], xr[i][2 * k + 1], w[k]);
        split_pair(xr[i][8], 0.f, w[4]);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          u32x4 v0;
#pragma unroll
          for (int k = 0; k < 4; ++k) v0[k] = w[k][q];
          lds_st128(dst + q * DSP_PLANE_B, v0);
        }
        if (res == 0) {      // run 4: Q0 from element 1
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            u32x4 v1;
#pragma unroll
            for (int k = 0; k < 4; ++k) v1[k] = __builtin_amdgcn_alignbit(w[k + 1][q], w[k][q], 16);
            lds_st128(dst + q * DSP_PLANE_B + 4 * DSP_RUN_B, v1);
          }
        }
      }
    }
    if (st + 1 < nst) fetch(st + 1);
    __syncthreads();      // this stage's x runs are written; the other buffer's readers passed the previous barrier
    bf16x8 b[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) b[q] = frag_from_u32x4(bfr[q]);
#pragma unroll
    for (int t9 = 0; t9 < 9; ++t9) {
      bf16x8 a[3];
#pragma unroll
      for (int q = 0; q < 3; ++q)
        a[q] = frag_from_u32x4(lds_ld128(adrA + buf + q * DSP_PLANE_B + (t9 % 3) * DSP_RUN_B + (t9 / 3) * 1024u));
#pragma unroll
      for (int o = 0; o < 6; ++o) acc[t9] = mfma_bf16(a[ORDER.p[o][0]], b[ORDER.p[o][1]], acc[t9]);
    }
  }

  const int co = co0 + wn * 32 + li;
  store_slab9(p, split, acc, ci0 + wm * 32, co, lane);
  if (do_bias) store_bias(p, split, co, h, bsum);
}

// ---- thin side: conv_in (3 -> C) and conv_out (C -> 3) ----------------------------------------------------------
// With <= 3 channels on one side the nine taps of that side fit ONE 32-wide MFMA operand: out[c][j] = sum over pixels
// of big[pixel][c] * small[pixel shifted by tap(j)][cs(j)], j = tap * Cs + cs < 27 -- a [C x pixels] x [pixels x 32]
// product that reads the wide tensor exactly once (HBM-bound: 1 GiB at 128 ch, 256^2, B=32).
//   conv_in : big = dy, small = x read at (y + kh - 1, x + kw - 1); column 27 multiplies 1.0, i.e. the bias gradient
//   conv_out: big = x,  small = dy read at (y - kh + 1, x - kw + 1)   (the same sum re-indexed by the input pixel)
// No LDS, no barriers: A fragments are coalesced 128-byte channel rows, B fragments gathers from the 25 MB tensor (cache
// resident); a wave owns whole image rows, eight k-steps (16 pixels) of loads in flight behind eight steps of MFMAs.
struct ThinParams {
  const float* big;     // [N][H][W][Cb]
  const float* small;   // [N][H][W][Cs]
  float* slab;          // [waves][CbP][32 * NT]
  int N, H, W, Cb, Cs, CbP, sign, ones_col;   // ones_col: column index that multiplies 1.0 (bias gradient), or -1
};

// One 16-byte load per lane is a pixel's channels 4i..4i+3: component t feeds channel tile t, whose row i is therefore
// channel c0 + 4i + t (any channel order will do, the slab store undoes it) -- a wave reads whole 512-byte pixel rows.
// NT column tiles of 32: one for Cs <= 3 (27 tap columns + the ones column), two for Cs = 4 (36 + 1: image_mask_key's 4-channel conv_out
// and a 4-channel conv_in); the wide tensor is still read once, each of its fragments feeds NT MFMA chains.
template <int NT>
__global__ __launch_bounds__(256) void conv3x3_wgrad_thin_kernel(ThinParams p) {
  const int lane = threadIdx.x & 63, li = lane & 31, kk = lane >> 5;
  const int wave_in_grid = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  const int c0 = blockIdx.y * 128;
  // this lane's B columns (one per column tile): tap and channel of the thin side
  int cs[NT], dyj[NT], dxj[NT];
  bool jtap[NT], ones[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int j = 32 * t + li, tap = j / p.Cs;
    cs[t] = j % p.Cs;
    jtap[t] = j < 9 * p.Cs;
    dyj[t] = p.sign * (tap / 3 - 1); dxj[t] = p.sign * (tap % 3 - 1);
    ones[t] = j == p.ones_col;
  }
  // channel quads past Cb (Cb not a multiple of 128): clamped address + select, never a guarded load
  const bool cok = c0 + 4 * li < p.Cb;
  const int coff = min(c0 + 4 * li, p.Cb - 4);
  f32x16 acc[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][ct][r] = 0.f;

  const int rows = p.N * p.H;
  constexpr int CH = 8;   // k-steps per chunk (16 pixels)
  float4 a_cur[CH], a_nxt[CH];
  float b_cur[NT][CH], b_nxt[NT][CH];
  for (int row = wave_in_grid; row < rows; row += nwaves) {
    const int y = row % p.H;
    bool rowok[NT];
    const float* srow[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int ys = y + dyj[t];
      rowok[t] = jtap[t] && ys >= 0 && ys < p.H;
      srow[t] = p.small + ((int64_t)(row - y + min(max(ys, 0), p.H - 1)) * p.W) * p.Cs + cs[t];
    }
    const float* brow = p.big + (int64_t)row * p.W * p.Cb + coff;
    auto load_chunk = [&](int x0, float4 (&a)[CH], float (&b)[NT][CH]) {
#pragma unroll
      for (int s = 0; s < CH; ++s) {
        const int x = x0 + 2 * s + kk;
        const float4 v4 = *reinterpret_cast<const float4*>(brow + (int64_t)x * p.Cb);
        a[s] = cok ? v4 : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int xs = x + dxj[t];
          const float v = srow[t][(int64_t)min(max(xs, 0), p.W - 1) * p.Cs];
          b[t][s] = ones[t] ? 1.f : ((rowok[t] && xs >= 0 && xs < p.W) ? v : 0.f);
        }
      }
    };
    load_chunk(0, a_cur, b_cur);
    for (int x0 = 0; x0 < p.W; x0 += 2 * CH) {
      if (x0 + 2 * CH < p.W) load_chunk(x0 + 2 * CH, a_nxt, b_nxt);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < CH; ++s) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          acc[t][0] = mfma32(a_cur[s].x, b_cur[t][s], acc[t][0]);
          acc[t][1] = mfma32(a_cur[s].y, b_cur[t][s], acc[t][1]);
          acc[t][2] = mfma32(a_cur[s].z, b_cur[t][s], acc[t][2]);
          acc[t][3] = mfma32(a_cur[s].w, b_cur[t][s], acc[t][3]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < CH; ++s) {
        a_cur[s] = a_nxt[s];
#pragma unroll
        for (int t = 0; t < NT; ++t) b_cur[t][s] = b_nxt[t][s];
      }
    }
  }
  float* sl = p.slab + (int64_t)wave_in_grid * p.CbP * (32 * NT);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = c0 + 4 * acc_row(r, lane) + ct;
        if (c < p.Cb) sl[c * (32 * NT) + 32 * t + li] = acc[t][ct][r];
      }
}

// partial column sums of the thin tensor (bias gradient of conv_out): part[block][Cs]
__global__ __launch_bounds__(256) void thin_colsum_kernel(const float* __restrict__ t, int64_t npix, int Cs, float* __restrict__ part) {
  __shared__ float red[4][4];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t px = (int64_t)blockIdx.x * 256 + threadIdx.x; px < npix; px += (int64_t)gridDim.x * 256)
    for (int c = 0; c < Cs; ++c) s[c] += t[px * Cs + c];
  for (int c = 0; c < 4; ++c) s[c] = wave_sum(s[c]);
  if ((threadIdx.x & 63) == 0) for (int c = 0; c < 4; ++c) red[threadIdx.x >> 6][c] = s[c];
  __syncthreads();
  if (threadIdx.x < Cs) part[blockIdx.x * Cs + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// sum the per-wave slabs in a fixed order and scatter into OIHW; sign +1: c = co, thin = ci; sign -1: c = ci, thin = co
__global__ void conv3x3_wgrad_thin_reduce_kernel(const float* __restrict__ slab, int nwaves, int Cb, int Cs, int CbP, int JW, int sign,
                                                 const float* __restrict__ bpart, int nbpart, int Cin, int Cout,
                                                 float* __restrict__ dw, float* __restrict__ dbias) {
  // block = 16 outputs x 16 parts: part q sums slabs q, q+16, ... (eight loads in flight), then the 16 parts are added in
  // a fixed order -- 2048 slabs are far too long a chain for one thread per output
  __shared__ float red[16][17];
  const int part = threadIdx.x >> 4;
  const int idx = blockIdx.x * 16 + (threadIdx.x & 15);
  if (idx < Cb * JW) {      // JW: the slab's columns per channel, 32 per column tile of the thin kernel
    const int c = idx / JW, j = idx % JW;
    float ps = 0.f;
    const float* src = slab + (int64_t)c * JW + j;
    const int64_t wstride = (int64_t)CbP * JW;
    int w = part;
    for (; w + 7 * 16 < nwaves; w += 8 * 16) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = src[(w + 16 * u) * wstride];
#pragma unroll
      for (int u = 0; u < 8; ++u) ps += v[u];
    }
    for (; w < nwaves; w += 16) ps += src[w * wstride];
    red[part][threadIdx.x & 15] = ps;
  }
  __syncthreads();
  if (part == 0 && idx < Cb * JW) {
    const int c = idx / JW, j = idx % JW;
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += red[q][threadIdx.x & 15];
    if (j < 9 * Cs) {
      const int tap = j / Cs, cs = j % Cs;
      const int co = sign > 0 ? c : cs, ci = sign > 0 ? cs : c;
      dw[((int64_t)co * Cin + ci) * 9 + tap] = s;
    } else if (sign > 0 && dbias && j == 9 * Cs) dbias[c] = s;
  } else if (part == 0 && sign < 0 && dbias && idx >= Cb * JW && idx - Cb * JW < Cout) {
    const int co = idx - Cb * JW;
    float s = 0.f;
    for (int b = 0; b < nbpart; ++b) s += bpart[b * Cs + co];
    dbias[co] = s;
  }
}

struct Plan { int v2, up, th, tiles_x, tiles_y, ntiles, nsplit, tiles_per_split, CinP, CoutP, ci_tiles, co_tiles; };

// up (parity classes) for mode 5, v2 (LDS-DMA) for the other modes, whenever both channel counts allow 16-byte pieces; v2 also only
// where the 128-wide co tile is not mostly padding.  Mode 5 with other channel counts runs the dense form, mode 2.
Plan make_plan(int mode, int N, int Ho, int Wo, int Cin, int Cout) {
  Plan pl;
  const bool c4 = Cin % 4 == 0 && Cout % 4 == 0;
  pl.up = mode == 5 && c4;
  pl.v2 = pl.up || (c4 && Cout > 64);
  int bci = BC, bco = BC;
  if (pl.up) {   // tiles of 2 x 16 LOW-RES pixels (Ho, Wo are the output's: twice the input's)
    bci = bco = UP_BC; pl.th = UP_TH;
    Ho /= 2; Wo /= 2;
  } else if (pl.v2) {
    bci = BCI2; bco = BCO2; pl.th = mode == 1 ? 2 : 4;
  } else pl.th = mode == 1 ? 4 : 8;
  pl.tiles_x = ceil_div(Wo, TW);
  pl.tiles_y = ceil_div(Ho, pl.th);
  pl.ntiles = pl.tiles_x * pl.tiles_y * N;
  pl.CinP = ceil_div(Cin, bci) * bci;
  pl.CoutP = ceil_div(Cout, bco) * bco;
  pl.ci_tiles = pl.CinP / bci;
  pl.co_tiles = pl.CoutP / bco;
  // the 8-wave kernels run one block per CU, one round: fewer slabs to write and sum (512: -3..-10 %)
  int nsplit = ceil_div(pl.v2 ? 256 : 1024, pl.ci_tiles * pl.co_tiles);
  if (nsplit > pl.ntiles) nsplit = pl.ntiles;
  if (nsplit < 1) nsplit = 1;
  pl.tiles_per_split = ceil_div(pl.ntiles, nsplit);
  pl.nsplit = ceil_div(pl.ntiles, pl.tiles_per_split);
  return pl;
}
// slab taps and bias-slab rows of one split: the parity kernels keep 4 classes x 4 taps and one bias row per class
int slab_taps(const Plan& pl) { return pl.up ? 16 : 9; }
int bias_rows(const Plan& pl) { return pl.up ? 4 : 1; }
// what store_taps relies on: one split's slab stays below 2^31 bytes
bool slab_fits(const Plan& pl) { return (int64_t)slab_taps(pl) * pl.CinP * pl.CoutP * 4 < 0x80000000ll; }

// thin-side kernel: stride-1 conv whose input or output has <= 4 channels (conv_in / conv_out; 4: an RGBA reconstruction)
constexpr int THIN_BLOCKS = 1024, THIN_BIAS_BLOCKS = 256, THIN_MAX = 4;
// column tiles of 32 the thin side's 9 * Cs tap columns (+ the ones column) take
int thin_col_tiles(int Cin, int Cout) { return std::min(Cin, Cout) <= 3 ? 1 : 2; }
bool thin_applies(int mode, int Hi, int Wi, int Cin, int Cout) {
  const int cb = Cin <= THIN_MAX ? Cout : Cin;
  return mode == 0 && (Cin <= THIN_MAX) != (Cout <= THIN_MAX) && Wi % 16 == 0 && cb % 4 == 0 && cb >= 32 &&
         (int64_t)Hi * Wi * cb * 4 < 0x7FFFFFF0ll;
}
size_t thin_workspace_floats(int Cin, int Cout) {
  const int cb = Cin <= THIN_MAX ? Cout : Cin;
  return (size_t)THIN_BLOCKS * 4 * cb * 32 * thin_col_tiles(Cin, Cout) + (size_t)THIN_BIAS_BLOCKS * std::max(3, std::min(Cin, Cout));
}
// grid of the thin kernel: channel groups of 128 on y, four waves (= four image rows in flight) per block on x
struct ThinPlan { int groups, blocks; };
ThinPlan make_thin_plan(int N, int Hi, int Cin, int Cout) {
  ThinPlan tp;
  tp.groups = ceil_div(Cin <= THIN_MAX ? Cout : Cin, 128);
  tp.blocks = std::max(1, std::min(THIN_BLOCKS / tp.groups, ceil_div(N * Hi, 4)));
  return tp;
}

// the block kernel of a tiled call: function, threads per block, dynamic LDS bytes
struct BlockKernel { void (*fn)(WgradParams); int threads; size_t smem; };
template <int MODE, int TH>
BlockKernel v1_kernel() {
  return {conv3x3_wgrad_kernel<MODE, TH>, 256, (size_t)(Halo<MODE, TH>::H * Halo<MODE, TH>::W + TH * TW) * BC * sizeof(float)};
}
template <int MODE, int TH>
BlockKernel dma_kernel() { return {conv3x3_wgrad_dma_kernel<MODE, TH>, 512, (size_t)2 * DmaGeom<MODE, TH>::BUF_F * sizeof(float)}; }
// mode: 0, 1 or 2 unless pl.up; split: the bf16-split form was chosen and serves this call
BlockKernel pick_kernel(const Plan& pl, int mode, bool split) {
  if (pl.up) return split ? BlockKernel{conv3x3_wgrad_up_split_kernel, 512, (size_t)2 * USP_BUF_B}
                          : BlockKernel{conv3x3_wgrad_up_kernel, 512, (size_t)2 * UpGeom::BUF_F * sizeof(float)};
  if (pl.v2 && mode == 1 && split) return {conv3x3_wgrad_down_split_kernel, 512, (size_t)2 * DSP_BUF_B};
  if (pl.v2) return mode == 0 ? dma_kernel<0, 4>() : mode == 1 ? dma_kernel<1, 2>() : dma_kernel<2, 4>();
  return mode == 0 ? v1_kernel<0, 8>() : mode == 1 ? v1_kernel<1, 4>() : v1_kernel<2, 8>();
}

// The bf16-split form serves the parity-class kernel (mode 5 with both channel counts multiples of 4: any other mode 5 call runs the
// dense form) and the Downsample conv where it gets the LDS-DMA kernel (mode 1, v2 of make_plan).
bool direct_split_supported(int mode, int Cin, int Cout) {
  return (mode == 5 || (mode == 1 && Cout > 64)) && Cin % 4 == 0 && Cout % 4 == 0;
}
// The shape rule (form -1): what was measured faster, slowest split launch of ten below the fastest f32 launch of ten, per launch at B = 32
// on the eight Upsample / Downsample layers of the headline step (profiles/wgrad_direct_split.md section 1): 128, 256 and 512 channels,
// 64 to 512 tiles per block at 0.58-0.64 (mode 5) and 32 to 512 tiles per block at 0.75-0.82 (mode 1) of the f32 kernel's time.  At 8
// tiles per block (256 -> 256, 32^2 -> 16^2) launch, slab stores and reduction, which the forms share, leave a gain that one launch in
// thirty did not show: fewer than 16 tiles per block keep the f32 kernel, and so do channel counts below those measured or with a
// ragged last channel tile.
bool direct_split_by_shape(const Plan& pl, int Cin, int Cout) {
  return pl.tiles_per_split >= 16 && Cin >= 128 && Cout >= 128 && Cin == pl.CinP && Cout == pl.CoutP;
}
int g_direct_form = -1;      // set by odvae_conv3x3_wgrad_select

}  // namespace

extern "C" {

// Which form of a tile's products odvae_conv3x3_wgrad_f32 runs: -1 by the shape rule (default), 0 the f32 MFMA kernels everywhere, 1 the
// bf16-split form wherever it supports the call (the f32 kernels elsewhere).  Returns the previous setting.
int odvae_conv3x3_wgrad_select(int form) {
  const int prev = g_direct_form;
  g_direct_form = form < 0 ? -1 : (form > 1 ? 1 : form);
  return prev;
}

// 1 when odvae_conv3x3_wgrad_select(1) makes this call run the bf16-split form; host only
int odvae_conv3x3_wgrad_split_supported(int mode, int N, int Hi, int Wi, int Cin, int Cout) {
  if (N <= 0 || Hi <= 0 || Wi <= 0 || Cin <= 0 || Cout <= 0) return 0;
  return direct_split_supported(mode, Cin, Cout) ? 1 : 0;
}

size_t odvae_conv3x3_wgrad_workspace_bytes(int mode, int N, int Ho, int Wo, int Cin, int Cout) {
  if (thin_applies(mode, Ho, Wo, Cin, Cout)) return thin_workspace_floats(Cin, Cout) * sizeof(float);
  const Plan pl = make_plan(mode, N, Ho, Wo, Cin, Cout);
  return ((size_t)pl.nsplit * slab_taps(pl) * pl.CinP * pl.CoutP + (size_t)pl.nsplit * bias_rows(pl) * pl.CoutP) * sizeof(float);
}

// Which kernel a call gets and how its pixels are split over blocks; host only, launches nothing.
// out = {kind, ntiles, nsplit, tiles_per_split, ci_tiles, co_tiles, tile_rows, effective_mode}; kind 0 thin, 1 v1, 2 v2 (LDS-DMA), 3 up.
// thin: {0, blocks per channel group, waves (= slabs), channel groups, 0, 0, 1, 0}.
int odvae_conv3x3_wgrad_plan(int mode, int N, int Hi, int Wi, int Cin, int Cout, int out[8]) {
  ODVAE_CHECK_ARG(out, "conv3x3_wgrad_plan: null out");
  ODVAE_CHECK_ARG((mode >= 0 && mode <= 2) || mode == 5, "conv3x3_wgrad_plan: mode %d", mode);
  ODVAE_CHECK_ARG(N > 0 && Hi > 0 && Wi > 0 && Cin > 0 && Cout > 0, "conv3x3_wgrad_plan: empty shape");
  if (mode == 1) ODVAE_CHECK_ARG(Hi % 2 == 0 && Wi % 2 == 0, "conv3x3_wgrad_plan mode 1: need even Hi,Wi");
  if (thin_applies(mode, Hi, Wi, Cin, Cout)) {
    const ThinPlan tp = make_thin_plan(N, Hi, Cin, Cout);
    const int v[8] = {0, tp.blocks, tp.blocks * 4, tp.groups, 0, 0, 1, 0};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return ODVAE_OK;
  }
  const int Ho = mode == 0 ? Hi : mode == 1 ? Hi / 2 : 2 * Hi, Wo = mode == 0 ? Wi : mode == 1 ? Wi / 2 : 2 * Wi;
  const Plan pl = make_plan(mode, N, Ho, Wo, Cin, Cout);
  ODVAE_CHECK_ARG(slab_fits(pl), "conv3x3_wgrad_plan: one split's slab must stay below 2 GiB");
  const int v[8] = {pl.up ? 3 : pl.v2 ? 2 : 1, pl.ntiles, pl.nsplit, pl.tiles_per_split, pl.ci_tiles, pl.co_tiles, pl.th,
                    (mode == 5 && !pl.up) ? 2 : mode};
  for (int i = 0; i < 8; ++i) out[i] = v[i];
  return ODVAE_OK;
}

// dw: OIHW [Cout][Cin][3][3] (overwritten).  dbias: [Cout] or null.
int odvae_conv3x3_wgrad_f32(int mode, const float* x, const float* dy, int N, int Hi, int Wi, int Cin,
                            int Ho, int Wo, int Cout, float* dw, float* dbias,
                            void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && dy && dw, "conv3x3_wgrad: null operand");
  ODVAE_CHECK_ARG((mode >= 0 && mode <= 2) || mode == 5, "conv3x3_wgrad: mode %d", mode);
  ODVAE_CHECK_ARG(N > 0 && Hi > 0 && Wi > 0 && Cin > 0 && Cout > 0, "conv3x3_wgrad: empty shape");
  if (mode == 0) ODVAE_CHECK_ARG(Ho == Hi && Wo == Wi, "conv3x3_wgrad mode 0: Ho,Wo must equal Hi,Wi");
  if (mode == 1) ODVAE_CHECK_ARG(Hi % 2 == 0 && Wi % 2 == 0 && Ho == Hi / 2 && Wo == Wi / 2, "conv3x3_wgrad mode 1: need even Hi,Wi");
  if (mode == 2 || mode == 5) ODVAE_CHECK_ARG(Ho == 2 * Hi && Wo == 2 * Wi, "conv3x3_wgrad mode %d: need Ho=2*Hi", mode);
  ODVAE_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)dy & 15) == 0, "conv3x3_wgrad: x/dy must be 16-byte aligned");
  ODVAE_CHECK_ARG((int64_t)Hi * Wi * Cin * 4 < 0x7FFFFFF0ll && (int64_t)Ho * Wo * Cout * 4 < 0x7FFFFFF0ll, "conv3x3_wgrad: one image must stay below 2 GiB");
  const Plan pl = make_plan(mode, N, Ho, Wo, Cin, Cout);
  const bool thin = thin_applies(mode, Hi, Wi, Cin, Cout);
  ODVAE_CHECK_ARG(thin || slab_fits(pl), "conv3x3_wgrad: one split's slab must stay below 2 GiB");
  const size_t need = odvae_conv3x3_wgrad_workspace_bytes(mode, N, Ho, Wo, Cin, Cout);
  if (!workspace || workspace_bytes < need) {
    odvae_set_error("conv3x3_wgrad: needs %zu workspace bytes, got %zu", need, workspace_bytes);
    return ODVAE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (thin) {
    ThinParams t;
    const bool in_thin = Cin <= THIN_MAX;   // conv_in: big = dy, small = x; conv_out: big = x, small = dy
    t.big = in_thin ? dy : x; t.small = in_thin ? x : dy;
    t.slab = static_cast<float*>(workspace);
    t.N = N; t.H = Hi; t.W = Wi; t.Cb = in_thin ? Cout : Cin; t.Cs = in_thin ? Cin : Cout; t.CbP = t.Cb;
    t.sign = in_thin ? 1 : -1; t.ones_col = (in_thin && dbias) ? 9 * t.Cs : -1;
    const ThinPlan tp = make_thin_plan(N, Hi, Cin, Cout);
    const int groups = tp.groups, blocks = tp.blocks;
    const int nt = thin_col_tiles(Cin, Cout), jw = 32 * nt;
    if (nt == 1) hipLaunchKernelGGL(conv3x3_wgrad_thin_kernel<1>, dim3(blocks, groups), dim3(256), 0, st, t);
    else hipLaunchKernelGGL(conv3x3_wgrad_thin_kernel<2>, dim3(blocks, groups), dim3(256), 0, st, t);
    ODVAE_LAUNCH_CHECK("conv3x3_wgrad thin");
    float* bpart = t.slab + (size_t)THIN_BLOCKS * 4 * t.Cb * jw;
    if (!in_thin && dbias) {
      hipLaunchKernelGGL(thin_colsum_kernel, dim3(THIN_BIAS_BLOCKS), dim3(256), 0, st, dy, (int64_t)N * Hi * Wi, Cout, bpart);
      ODVAE_LAUNCH_CHECK("conv3x3_wgrad thin bias");
    }
    const int items = t.Cb * jw + (in_thin ? 0 : Cout);
    hipLaunchKernelGGL(conv3x3_wgrad_thin_reduce_kernel, dim3(ceil_div(items, 16)), dim3(256), 0, st,
                       t.slab, blocks * 4, t.Cb, t.Cs, t.CbP, jw, t.sign, bpart, THIN_BIAS_BLOCKS, Cin, Cout, dw, dbias);
    ODVAE_LAUNCH_CHECK("conv3x3_wgrad thin reduce");
    return ODVAE_OK;
  }
  WgradParams p;
  p.x = x; p.dy = dy;
  p.slab = static_cast<float*>(workspace);
  p.bslab = dbias ? p.slab + (size_t)pl.nsplit * slab_taps(pl) * pl.CinP * pl.CoutP : nullptr;
  if (mode == 5 && !pl.up) mode = 2;
  p.N = N; p.Hi = Hi; p.Wi = Wi; p.Cin = Cin; p.Ho = Ho; p.Wo = Wo; p.Cout = Cout;
  p.CinP = pl.CinP; p.CoutP = pl.CoutP;
  p.tiles_x = pl.tiles_x; p.tiles_y = pl.tiles_y; p.ntiles = pl.ntiles;
  p.tiles_per_split = pl.tiles_per_split; p.ci_tiles = pl.ci_tiles;
  const bool split = g_direct_form != 0 && direct_split_supported(mode, Cin, Cout) &&
                     (g_direct_form == 1 || direct_split_by_shape(pl, Cin, Cout));
  const BlockKernel k = pick_kernel(pl, mode, split);
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.smem);
  if (e != hipSuccess) {
    odvae_set_error("conv3x3_wgrad: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    return ODVAE_ERR_HIP;
  }
  hipLaunchKernelGGL(k.fn, dim3(pl.nsplit, pl.ci_tiles * pl.co_tiles), dim3(k.threads), k.smem, st, p);
  ODVAE_LAUNCH_CHECK("conv3x3_wgrad");
  const int64_t total = (int64_t)9 * pl.CinP * pl.CoutP + pl.CoutP;
  hipLaunchKernelGGL(pl.up ? conv3x3_wgrad_up_reduce_kernel : conv3x3_wgrad_reduce_kernel,
                     dim3((int)std::min<int64_t>(ceil_div64(total, 256), 4096)), dim3(256), 0, st,
                     p.slab, p.bslab, pl.nsplit, bias_rows(pl), Cin, Cout, pl.CinP, pl.CoutP, dw, dbias);
  ODVAE_LAUNCH_CHECK("conv3x3_wgrad reduce");
  return ODVAE_OK;
}

}  // extern "C"
