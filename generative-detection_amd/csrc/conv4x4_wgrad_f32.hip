// Weight (and bias) gradient of Conv2d(k=4, pad=1, stride 1|2), NHWC, exact f32 on the matrix cores: the PatchGAN
// discriminator's convs ([UPSTREAM] taming NLayerDiscriminator) without a cols matrix.
//
// dW[co][ci][kh][kw] = sum over (n, oy, ox) of x[n][S oy - 1 + kh][S ox - 1 + kw][ci] * dy[n][oy][ox][co], zero outside the image.
//
// The register-staged form of conv3x3_wgrad_kernel (conv3x3_wgrad_f32.hip) generalised to 16 taps.  GEMM view per tap: M = ci,
// N = co, K = pixels.  Sixteen 32x32 accumulator tiles per wave do not fit (nine already take 144 registers), so the taps go in two
// halves of eight -- blockIdx.z = half, tap rows kh in {2 half, 2 half + 1} -- and a wave keeps 128 accumulator registers.  A block
// owns a 64(ci) x 64(co) slice of its eight taps and a contiguous range of TH x 16 output-pixel tiles; per tile it stages the rows of
// the input halo its tap rows read ([TH + 1 | 2 TH rows][19 | 34 px][64 ci]) and the dy tile [px][64 co] in LDS; both are read with
// lanes = consecutive channels (conflict-free b32), one dy read feeds eight MFMAs.  Blocks write partial slabs
// [split][16][CinP][CoutP]; a second kernel sums the splits in a fixed order (deterministic) and writes OIHW.  db = column sums of
// dy ride along in the blocks with ci_tile == 0, half == 0.
#include "common.h"

namespace {

constexpr int TW = 16;
constexpr int BC = 64;  // channels per block on both axes

struct Wgrad4Params {
  const float* x;    // [N][Hi][Wi][Cin]
  const float* dy;   // [N][Ho][Wo][Cout]
  float* slab;       // [nsplit][16][CinP][CoutP]
  float* bslab;      // [nsplit][CoutP] or null
  int N, Hi, Wi, Cin, Ho, Wo, Cout, CinP, CoutP;
  int tiles_x, tiles_y, ntiles, tiles_per_split, ci_tiles;
};

// the halo rows of ONE half of the taps: local row S r + khl, khl in {0, 1}; local column S c + kw, kw in 0..3
template <int S, int TH>
struct Geom {
  static constexpr int HH = S == 1 ? TH + 1 : 2 * TH;
  static constexpr int HW = S == 1 ? TW + 3 : 2 * TW + 2;
  static constexpr int HPIX = HH * HW;
  static constexpr int NPIX = TH * TW;
};

template <int S, int TH>
__global__ __launch_bounds__(256) void conv4x4_wgrad_kernel(Wgrad4Params p) {
  using G = Geom<S, TH>;
  constexpr int HALO_F4 = G::HPIX * (BC / 4), HALO_IT = (HALO_F4 + 255) / 256;
  constexpr int DY_F4 = G::NPIX * (BC / 4), DY_IT = (DY_F4 + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Xs = smem;                    // [HPIX][BC]
  float* Ds = smem + G::HPIX * BC;     // [NPIX][BC]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, h = lane >> 5;
  const int split = blockIdx.x;
  const int half = blockIdx.z;
  const int ci_tile = blockIdx.y % p.ci_tiles, co_tile = blockIdx.y / p.ci_tiles;
  const int ci0 = ci_tile * BC, co0 = co_tile * BC;
  const bool xvec = (p.Cin & 3) == 0, dvec = (p.Cout & 3) == 0;
  const bool do_bias = p.bslab != nullptr && ci_tile == 0 && half == 0 && wm == 0;

  f32x16 acc[8];
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum = 0.f;

  const int t_beg = split * p.tiles_per_split;
  const int t_end = min(p.ntiles, t_beg + p.tiles_per_split);
  for (int tile = t_beg; tile < t_end; ++tile) {
    int t = tile;
    const int tx = t % p.tiles_x; t /= p.tiles_x;
    const int ty = t % p.tiles_y; const int n = t / p.tiles_y;
    const int oy0 = ty * TH, ox0 = tx * TW;
    const int iy0 = S * oy0 - 1 + 2 * half, ix0 = S * ox0 - 1;
    const float* xn = p.x + (int64_t)n * p.Hi * p.Wi * p.Cin;
    const float* dn = p.dy + (int64_t)n * p.Ho * p.Wo * p.Cout;

    __syncthreads();  // previous tile's reads are done
#pragma unroll
    for (int i = 0; i < HALO_IT; ++i) {
      const int f = tid + 256 * i;
      if (f < HALO_F4) {
        const int hp = f / (BC / 4), q = f % (BC / 4);
        const int iy = iy0 + hp / G::HW, ix = ix0 + hp % G::HW;
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
    for (int s = 0; s < G::NPIX / 2; ++s) {
      const int px = 2 * s + h;
      const int r = px / TW, c = px % TW;
      const float b = db[px * BC];
      if (do_bias) bsum += b;
#pragma unroll
      for (int t8 = 0; t8 < 8; ++t8) {
        const float a = xa[((S * r + t8 / 4) * G::HW + S * c + t8 % 4) * BC];
        acc[t8] = mfma32(a, b, acc[t8]);
      }
    }
  }

  // partial slab: [split][tap][ci][co], lane = co; this block's taps are 8 half .. 8 half + 7
  const int co = co0 + wn * 32 + li;
  float* sl = p.slab + ((int64_t)split * 16 + 8 * half) * p.CinP * p.CoutP;
#pragma unroll
  for (int t8 = 0; t8 < 8; ++t8)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ci = ci0 + wm * 32 + acc_row(r, lane);
      sl[((int64_t)t8 * p.CinP + ci) * p.CoutP + co] = acc[t8][r];
    }
  if (do_bias) {
    bsum += __shfl_xor(bsum, 32, 64);
    if (h == 0) p.bslab[(int64_t)split * p.CoutP + co] = bsum;
  }
}

// sum the splits in a fixed order; one thread per element of dw in OIHW order (the 16 taps of a (co, ci) pair are contiguous)
__global__ void conv4x4_wgrad_reduce_kernel(const float* __restrict__ slab, const float* __restrict__ bslab,
                                            int nsplit, int Cin, int Cout, int CinP, int CoutP,
                                            float* __restrict__ dw, float* __restrict__ dbias) {
  const int64_t mat = (int64_t)CinP * CoutP, per = 16 * mat;
  const int64_t ndw = (int64_t)Cout * Cin * 16;
  const int64_t total = ndw + (dbias ? Cout : 0);
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    if (idx < ndw) {
      const int tap = (int)(idx & 15);
      const int ci = (int)((idx >> 4) % Cin), co = (int)((idx >> 4) / Cin);
      const float* src = slab + tap * mat + (int64_t)ci * CoutP + co;
      float sk[4] = {0.f, 0.f, 0.f, 0.f};      // four independent chains, as conv3x3_wgrad_reduce_kernel
      int sp = 0;
      for (; sp + 3 < nsplit; sp += 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) sk[j] += src[(sp + j) * per];
      }
      for (; sp < nsplit; ++sp) sk[0] += src[sp * per];
      dw[idx] = (sk[0] + sk[1]) + (sk[2] + sk[3]);
    } else {
      const int co = (int)(idx - ndw);
      float s = 0.f;
      for (int sp = 0; sp < nsplit; ++sp) s += bslab[(int64_t)sp * CoutP + co];
      dbias[co] = s;
    }
  }
}

struct Plan4 { int th, tiles_x, tiles_y, ntiles, nsplit, tiles_per_split, CinP, CoutP, ci_tiles, co_tiles; };

// tiles of 8 x 16 (stride 1) / 4 x 16 (stride 2) output pixels; about 512 blocks (two per CU) over (split, ci tile, co tile, half)
Plan4 make_plan4(int stride, int N, int Ho, int Wo, int Cin, int Cout) {
  Plan4 pl;
  pl.th = stride == 1 ? 8 : 4;
  pl.tiles_x = ceil_div(Wo, TW);
  pl.tiles_y = ceil_div(Ho, pl.th);
  pl.ntiles = pl.tiles_x * pl.tiles_y * N;
  pl.CinP = ceil_div(Cin, BC) * BC;
  pl.CoutP = ceil_div(Cout, BC) * BC;
  pl.ci_tiles = pl.CinP / BC;
  pl.co_tiles = pl.CoutP / BC;
  int nsplit = ceil_div(256, pl.ci_tiles * pl.co_tiles);
  if (nsplit > pl.ntiles) nsplit = pl.ntiles;
  if (nsplit < 1) nsplit = 1;
  pl.tiles_per_split = ceil_div(pl.ntiles, nsplit);
  pl.nsplit = ceil_div(pl.ntiles, pl.tiles_per_split);
  return pl;
}

template <int S, int TH>
size_t smem_bytes() { return (size_t)(Geom<S, TH>::HPIX + Geom<S, TH>::NPIX) * BC * sizeof(float); }

bool geometry_ok(int stride, int Hi, int Wi, int Ho, int Wo) {
  return (stride == 1 || stride == 2) && Hi >= 2 && Wi >= 2 && Ho == (Hi - 2) / stride + 1 && Wo == (Wi - 2) / stride + 1;
}

}  // namespace

extern "C" {

size_t odvae_conv4x4_wgrad_workspace_bytes(int stride, int N, int Ho, int Wo, int Cin, int Cout) {
  if ((stride != 1 && stride != 2) || N <= 0 || Ho <= 0 || Wo <= 0 || Cin <= 0 || Cout <= 0) return 0;
  if ((int64_t)ceil_div(Wo, TW) * ceil_div(Ho, stride == 1 ? 8 : 4) * N >= (1ll << 31)) return 0;
  const Plan4 pl = make_plan4(stride, N, Ho, Wo, Cin, Cout);
  return ((size_t)pl.nsplit * 16 * pl.CinP * pl.CoutP + (size_t)pl.nsplit * pl.CoutP) * sizeof(float);
}

// How a call's pixels are split over blocks; host only, launches nothing.  Hi, Wi are the input's.
// out = {kind (1: the register-staged kernel), ntiles, nsplit, tiles_per_split, ci_tiles, co_tiles, tile_rows, stride}; split s owns
// tiles [s * tiles_per_split, min(ntiles, (s + 1) * tiles_per_split)), and every (split, ci tile, co tile) runs as two blocks (tap halves).
int odvae_conv4x4_wgrad_plan(int stride, int N, int Hi, int Wi, int Cin, int Cout, int out[8]) {
  ODVAE_CHECK_ARG(out, "conv4x4_wgrad_plan: null out");
  ODVAE_CHECK_ARG(stride == 1 || stride == 2, "conv4x4_wgrad_plan: stride %d", stride);
  ODVAE_CHECK_ARG(N > 0 && Hi >= 2 && Wi >= 2 && Cin > 0 && Cout > 0, "conv4x4_wgrad_plan: empty shape");
  const int Ho = (Hi - 2) / stride + 1, Wo = (Wi - 2) / stride + 1;
  ODVAE_CHECK_ARG((int64_t)ceil_div(Wo, TW) * ceil_div(Ho, stride == 1 ? 8 : 4) * N < (1ll << 31), "conv4x4_wgrad_plan: too many tiles");
  const Plan4 pl = make_plan4(stride, N, Ho, Wo, Cin, Cout);
  const int v[8] = {1, pl.ntiles, pl.nsplit, pl.tiles_per_split, pl.ci_tiles, pl.co_tiles, pl.th, stride};
  for (int i = 0; i < 8; ++i) out[i] = v[i];
  return ODVAE_OK;
}

// dw: OIHW [Cout][Cin][4][4] (overwritten).  dbias: [Cout] or null.
int odvae_conv4x4_wgrad_f32(int stride, const float* x, const float* dy, int N, int Hi, int Wi, int Cin, int Ho, int Wo, int Cout,
                            float* dw, float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
  ODVAE_CHECK_ARG(x && dy && dw, "conv4x4_wgrad: null operand");
  ODVAE_CHECK_ARG(stride == 1 || stride == 2, "conv4x4_wgrad: stride %d", stride);
  ODVAE_CHECK_ARG(N > 0 && Hi > 0 && Wi > 0 && Cin > 0 && Cout > 0, "conv4x4_wgrad: empty shape");
  ODVAE_CHECK_ARG(geometry_ok(stride, Hi, Wi, Ho, Wo), "conv4x4_wgrad: need Hi, Wi >= 2 and Ho = (Hi - 2) / stride + 1");
  ODVAE_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)dy & 15) == 0, "conv4x4_wgrad: x/dy must be 16-byte aligned");
  ODVAE_CHECK_ARG((int64_t)Hi * Wi * Cin * 4 < 0x7FFFFFF0ll && (int64_t)Ho * Wo * Cout * 4 < 0x7FFFFFF0ll, "conv4x4_wgrad: one image must stay below 2 GiB");
  ODVAE_CHECK_ARG((int64_t)ceil_div(Wo, TW) * ceil_div(Ho, stride == 1 ? 8 : 4) * N < (1ll << 31), "conv4x4_wgrad: too many tiles");
  const Plan4 pl = make_plan4(stride, N, Ho, Wo, Cin, Cout);
  const size_t need = odvae_conv4x4_wgrad_workspace_bytes(stride, N, Ho, Wo, Cin, Cout);
  if (!workspace || workspace_bytes < need) {
    odvae_set_error("conv4x4_wgrad: needs %zu workspace bytes, got %zu", need, workspace_bytes);
    return ODVAE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  Wgrad4Params p;
  p.x = x; p.dy = dy;
  p.slab = static_cast<float*>(workspace);
  p.bslab = dbias ? p.slab + (size_t)pl.nsplit * 16 * pl.CinP * pl.CoutP : nullptr;
  p.N = N; p.Hi = Hi; p.Wi = Wi; p.Cin = Cin; p.Ho = Ho; p.Wo = Wo; p.Cout = Cout;
  p.CinP = pl.CinP; p.CoutP = pl.CoutP;
  p.tiles_x = pl.tiles_x; p.tiles_y = pl.tiles_y; p.ntiles = pl.ntiles;
  p.tiles_per_split = pl.tiles_per_split; p.ci_tiles = pl.ci_tiles;
  dim3 grid(pl.nsplit, pl.ci_tiles * pl.co_tiles, 2);
  const size_t smem = stride == 1 ? smem_bytes<1, 8>() : smem_bytes<2, 4>();
  const void* fn = stride == 1 ? reinterpret_cast<const void*>(conv4x4_wgrad_kernel<1, 8>) : reinterpret_cast<const void*>(conv4x4_wgrad_kernel<2, 4>);
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) {
    odvae_set_error("conv4x4_wgrad: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
    return ODVAE_ERR_HIP;
  }
  if (stride == 1) hipLaunchKernelGGL((conv4x4_wgrad_kernel<1, 8>), grid, dim3(256), smem, st, p);
  else hipLaunchKernelGGL((conv4x4_wgrad_kernel<2, 4>), grid, dim3(256), smem, st, p);
  ODVAE_LAUNCH_CHECK("conv4x4_wgrad");
  const int64_t total = (int64_t)Cout * Cin * 16 + Cout;
  const int blocks = (int)std::min<int64_t>(ceil_div64(total, 256), 4096);
  hipLaunchKernelGGL(conv4x4_wgrad_reduce_kernel, dim3(blocks), dim3(256), 0, st,
                     p.slab, p.bslab, pl.nsplit, Cin, Cout, pl.CinP, pl.CoutP, dw, dbias);
  ODVAE_LAUNCH_CHECK("conv4x4_wgrad reduce");
  return ODVAE_OK;
}

}  // extern "C"
