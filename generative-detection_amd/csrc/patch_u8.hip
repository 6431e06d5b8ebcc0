// Object-patch extraction on the device: crop (zero fill outside the camera image) -> Pillow-exact BILINEAR resize of the
// u8 crop to S x S -> ToTensor (u8 / 255 as f32), plus the NEAREST-resized 2-d box mask.  HBM-bound byte work, gfx950.
//
// Replaces the per-instance PIL path of the reference's dataset, src/data/datasets/nuscenes.py:159-192
//   patch = img_pil.crop((x1, y1, x2, y2))                                          (:159)
//   patch.resize((w, h), resample=BILINEAR, reducing_gap=1.0)                       (:176)
//   mask_bool[y1p:y2p, x1p:x2p] = True; Image.fromarray(mask_bool).resize(.., NEAREST)  (:178-189)
//   transforms.ToTensor()                                                           (:190-192)
// Pillow (third-party, 12.2.0 in this image) resamples 8-bit images in fixed point: per output index a window
// [xmin, xmin+n) of <= 5 taps with integer coefficients k = round(w * 2^22) (triangle filter, renormalised at the crop
// border), the horizontal pass rounded to u8 before the vertical pass, each as (2^21 + sum p*k) >> 22 clamped to 0..255.
// The coefficient / nearest-index tables depend only on (crop size, S); the host builds them once per crop size in f64
// exactly as Pillow's precompute_coeffs does (patches.py) and this kernel does integer arithmetic only, so the result is
// bit-identical to PIL.
//
// Crops with size >= 2*S: `reducing_gap=1.0` makes Pillow box-reduce the crop by the integer factor f = int(size / S) first
// (Reduce.c: side r = ceil(size / f); each byte is ((sum + n/2) * mult(n)) >> 24 in unsigned 32-bit arithmetic, n = crop pixels in
// the box, fewer in the last column / row when size % f != 0; mult(n) is a float32 quotient the host supplies per crop size) and run
// the bilinear pass from the reduced image with the fractional source box [0, (float32)(size / f)).  patch_crop_resize_kernel below
// knows nothing of this (its callers refuse such crops); patch_reduce_resize_kernel takes any f >= 1 per instance: a block stages
// the window of reduced pixels that its 64 x 4 outputs need in LDS, each made once from its f x f source bytes, and both resampling
// passes run from LDS.  The box mask is never reduced (NEAREST): its source index is the one of the unreduced size -> S walk.
#include "common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;   // Pillow Resample.c, 8 bits per channel
constexpr int TAB_INTS = 8;                  // per output index: k[0..4], first source index, taps, nearest source index

struct PatchParams {
  const uint8_t* const* images;   // [B] device pointers, u8 HWC RGB
  const int32_t* geom;            // [B][8]: img_h, img_w, crop_x1, crop_y1, crop_size, table_slot, reduce factor f (0 = 1), 0
  const int32_t* mask_rect;       // [B][4]: x_start, x_stop, y_start, y_stop in crop coordinates (slice-normalised)
  const int32_t* tables;          // [n_slots][S][TAB_INTS]
  const uint32_t* mults;          // [n_slots][4]: mult(f*f), mult(f*rem), mult(rem*rem), 0 (reduce kernel only; rem = width of the last box)
  float* patch;                   // [B][S][S][3]  (NHWC; logical NCHW channels_last)
  float* mask;                    // [B][S][S]
  int B, S, n_slots;
};

__device__ __forceinline__ int clip8(int v) { return min(max(v >> PRECISION_BITS, 0), 255); }

// block = 64 x 4 output pixels (one wave per output row); 3 contiguous floats per lane -> coalesced stores; source bytes
// come through L1/L2; 32-bit index arithmetic only (the host checks H*W*3 < 2^31)
__global__ __launch_bounds__(256) void patch_crop_resize_kernel(PatchParams p) {
  const int ox = blockIdx.x * 64 + (threadIdx.x & 63);
  const int oy = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int b = blockIdx.z;
  if (ox >= p.S || oy >= p.S) return;
  const int4 g0 = reinterpret_cast<const int4*>(p.geom)[b * 2];
  const int4 g1 = reinterpret_cast<const int4*>(p.geom)[b * 2 + 1];
  const int H = g0.x, W = g0.y, cx1 = g0.z, cy1 = g0.w;
  const int slot = min(max(g1.y, 0), p.n_slots - 1);
  const int4* tab = reinterpret_cast<const int4*>(p.tables) + slot * p.S * 2;
  const int4 tx0 = tab[ox * 2], tx1 = tab[ox * 2 + 1], ty0 = tab[oy * 2], ty1 = tab[oy * 2 + 1];
  const int kx[5] = {tx0.x, tx0.y, tx0.z, tx0.w, tx1.x}, ky[5] = {ty0.x, ty0.y, ty0.z, ty0.w, ty1.x};
  const int xmin = tx1.y, nx = min(tx1.z, 5), ymin = ty1.y, ny = min(ty1.z, 5);
  const uint8_t* img = p.images[b];
  const int last_dword = H * W * 3 - 4;   // a pixel is fetched as one unaligned dword that never leaves the image
  int xoff[5], kxm[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int sx = cx1 + xmin + j;
    xoff[j] = min(max(sx, 0), W - 1) * 3;
    kxm[j] = (j < nx && sx >= 0 && sx < W) ? kx[j] : 0;   // outside the camera image the crop is 0
  }
  int acc0 = 1 << (PRECISION_BITS - 1), acc1 = acc0, acc2 = acc0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    if (i < ny) {
      const int sy = cy1 + ymin + i;
      const int row = min(max(sy, 0), H - 1) * W * 3;
      int h0 = 0, h1 = 0, h2 = 0;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        if (j < nx) {
          const int off = row + xoff[j];
          const int at = min(off, last_dword);
          uint32_t rgb;
          __builtin_memcpy(&rgb, img + at, 4);
          rgb >>= 8 * (off - at);
          h0 += (int)(rgb & 255u) * kxm[j]; h1 += (int)((rgb >> 8) & 255u) * kxm[j]; h2 += (int)((rgb >> 16) & 255u) * kxm[j];
        }
      }
      const int half = 1 << (PRECISION_BITS - 1);
      const int kyi = (sy >= 0 && sy < H) ? ky[i] : 0;       // a row outside the image is all zeros: clip8(half) = 0
      acc0 += clip8(h0 + half) * kyi; acc1 += clip8(h1 + half) * kyi; acc2 += clip8(h2 + half) * kyi;
    }
  }
  const int idx = (b * p.S + oy) * p.S + ox;
  float* o = p.patch + (int64_t)idx * 3;
  o[0] = __fdiv_rn((float)clip8(acc0), 255.0f);
  o[1] = __fdiv_rn((float)clip8(acc1), 255.0f);
  o[2] = __fdiv_rn((float)clip8(acc2), 255.0f);
  const int4 mr = reinterpret_cast<const int4*>(p.mask_rect)[b];
  const int nxs = tx1.w, nys = ty1.w;
  p.mask[idx] = (nxs >= mr.x && nxs < mr.y && nys >= mr.z && nys < mr.w) ? 1.0f : 0.0f;
}

// Window of reduced pixels behind one 64 x 4 output block.  After the reduce scale = (size / f) / S < 2 and support = max(scale, 1),
// so the first and last window of 64 consecutive outputs span < 63 * 2 + 2 * 2 + 1 = 131 columns and those of 4 rows < 11 rows.
constexpr int RED_W = 136, RED_H = 13;

// Same block shape and the same bits as patch_crop_resize_kernel for f = 1 (mult(1) = 2^24: the "reduce" is a copy).  Pixels live in
// LDS as one dword each (r | g << 8 | b << 16); a pixel of the crop outside the camera image is a zero that counts in n, as in
// Image.crop -> Image.reduce.  Every LDS index is clamped, so a malformed table can give wrong bytes but no stray access.
__global__ __launch_bounds__(256) void patch_reduce_resize_kernel(PatchParams p) {
  __shared__ uint32_t red[RED_H][RED_W];
  __shared__ uint32_t hor[RED_H][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ox0 = blockIdx.x * 64, oy0 = blockIdx.y * 4, b = blockIdx.z;
  const bool live = ox0 + lane < p.S && oy0 + wave < p.S;
  const int ox = min(ox0 + lane, p.S - 1), oy = min(oy0 + wave, p.S - 1);   // idle lanes redo the last column / row and store nothing
  const int4 g0 = reinterpret_cast<const int4*>(p.geom)[b * 2];
  const int4 g1 = reinterpret_cast<const int4*>(p.geom)[b * 2 + 1];
  const int H = g0.x, W = g0.y, cx1 = g0.z, cy1 = g0.w, size = g1.x, f = max(g1.z, 1);
  const int slot = min(max(g1.y, 0), p.n_slots - 1);
  const uint4 mult = reinterpret_cast<const uint4*>(p.mults)[slot];
  const int4* tab = reinterpret_cast<const int4*>(p.tables) + slot * p.S * 2;
  const int4 tx0 = tab[ox * 2], tx1 = tab[ox * 2 + 1], ty0 = tab[oy * 2], ty1 = tab[oy * 2 + 1];
  const int4 wxa = tab[ox0 * 2 + 1], wxb = tab[min(ox0 + 63, p.S - 1) * 2 + 1];
  const int4 wya = tab[oy0 * 2 + 1], wyb = tab[min(oy0 + 3, p.S - 1) * 2 + 1];
  const int rx0 = wxa.y, wx = min(max(wxb.y + wxb.z - rx0, 0), RED_W);
  const int ry0 = wya.y, wy = min(max(wyb.y + wyb.z - ry0, 0), RED_H);
  const uint8_t* img = p.images[b];
  const int last_dword = H * W * 3 - 4;   // a pixel is fetched as one unaligned dword that never leaves the image
  // 1. the window of reduced pixels, each from its box of the zero-filled crop
  for (int item = threadIdx.x; item < wx * wy; item += 256) {
    const int iy = item / wx, ix = item - iy * wx;
    const int bx = (rx0 + ix) * f, by = (ry0 + iy) * f;           // the box in crop coordinates
    const int bw = min(f, size - bx), bh = min(f, size - by);   // the last column / row averages over the pixels it has
    uint32_t px = 0;
    if (bx >= 0 && by >= 0 && bw > 0 && bh > 0) {
      const int xa = max(cx1 + bx, 0), xb = min(cx1 + bx + bw, W), ya = max(cy1 + by, 0), yb = min(cy1 + by + bh, H);
      uint32_t s0 = 0, s1 = 0, s2 = 0;
      for (int sy = ya; sy < yb; ++sy) {
        const int row = sy * W * 3;
        for (int sx = xa; sx < xb; ++sx) {
          const int off = row + sx * 3;
          const int at = min(off, last_dword);
          uint32_t rgb;
          __builtin_memcpy(&rgb, img + at, 4);
          rgb >>= 8 * (off - at);
          s0 += rgb & 255u; s1 += (rgb >> 8) & 255u; s2 += (rgb >> 16) & 255u;
        }
      }
      const uint32_t amend = (uint32_t)(bw * bh) >> 1;
      const uint32_t m = bw == f ? (bh == f ? mult.x : mult.y) : (bh == f ? mult.y : mult.z);
      px = ((s0 + amend) * m >> 24) | ((s1 + amend) * m >> 24) << 8 | ((s2 + amend) * m >> 24) << 16;
    }
    red[iy][ix] = px;
  }
  __syncthreads();
  // 2. horizontal pass, rounded to u8: this lane's output column for every window row (wave w takes rows w, w + 4, w + 8)
  const int half = 1 << (PRECISION_BITS - 1);
  {
    const int kx[5] = {tx0.x, tx0.y, tx0.z, tx0.w, tx1.x};
    const int xmin = tx1.y, nx = min(tx1.z, 5);
    int xi[5], kxm[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      xi[j] = min(max(xmin - rx0 + j, 0), RED_W - 1);
      kxm[j] = j < nx ? kx[j] : 0;
    }
    for (int iy = wave; iy < wy; iy += 4) {
      int h0 = half, h1 = half, h2 = half;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const uint32_t px = red[iy][xi[j]];
        h0 += (int)(px & 255u) * kxm[j]; h1 += (int)((px >> 8) & 255u) * kxm[j]; h2 += (int)((px >> 16) & 255u) * kxm[j];
      }
      hor[iy][lane] = (uint32_t)clip8(h0) | (uint32_t)clip8(h1) << 8 | (uint32_t)clip8(h2) << 16;
    }
  }
  __syncthreads();
  // 3. vertical pass
  const int ky[5] = {ty0.x, ty0.y, ty0.z, ty0.w, ty1.x};
  const int ymin = ty1.y, ny = min(ty1.z, 5);
  int acc0 = half, acc1 = half, acc2 = half;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const uint32_t px = hor[min(max(ymin - ry0 + i, 0), RED_H - 1)][lane];
    const int kyi = i < ny ? ky[i] : 0;
    acc0 += (int)(px & 255u) * kyi; acc1 += (int)((px >> 8) & 255u) * kyi; acc2 += (int)((px >> 16) & 255u) * kyi;
  }
  if (!live) return;
  const int idx = (b * p.S + oy) * p.S + ox;
  float* o = p.patch + (int64_t)idx * 3;
  o[0] = __fdiv_rn((float)clip8(acc0), 255.0f);
  o[1] = __fdiv_rn((float)clip8(acc1), 255.0f);
  o[2] = __fdiv_rn((float)clip8(acc2), 255.0f);
  const int4 mr = reinterpret_cast<const int4*>(p.mask_rect)[b];
  const int nxs = tx1.w, nys = ty1.w;
  p.mask[idx] = (nxs >= mr.x && nxs < mr.y && nys >= mr.z && nys < mr.w) ? 1.0f : 0.0f;
}

}  // namespace

extern "C" int odvae_patch_table_ints(int S) { return S * TAB_INTS; }

extern "C" int odvae_patch_crop_resize_u8(const void* d_images, const void* d_geom, const void* d_mask_rect, const void* d_tables,
                                          int n_slots, int B, int S, void* patch, void* mask, void* stream) {
  ODVAE_CHECK_ARG(d_images && d_geom && d_mask_rect && d_tables && patch && mask, "patch_crop_resize: null pointer");
  ODVAE_CHECK_ARG(B > 0 && S > 0 && S <= 4096 && n_slots > 0, "patch_crop_resize: bad sizes");   // images: >= 2 pixels each
  PatchParams p;
  p.images = (const uint8_t* const*)d_images; p.geom = (const int32_t*)d_geom; p.mask_rect = (const int32_t*)d_mask_rect;
  p.tables = (const int32_t*)d_tables; p.mults = nullptr; p.patch = (float*)patch; p.mask = (float*)mask;
  p.B = B; p.S = S; p.n_slots = n_slots;
  ODVAE_CHECK_ARG(B <= 65535 && (int64_t)B * S * S < (int64_t)1 << 31, "patch_crop_resize: batch too large for one launch");
  hipLaunchKernelGGL(patch_crop_resize_kernel, dim3(ceil_div(S, 64), ceil_div(S, 4), B), dim3(256), 0, static_cast<hipStream_t>(stream), p);
  ODVAE_LAUNCH_CHECK("patch_crop_resize_kernel");
  return 0;
}

extern "C" int odvae_patch_reduce_resize_u8(const void* d_images, const void* d_geom, const void* d_mask_rect, const void* d_tables,
                                            const void* d_mults, int n_slots, int B, int S, void* patch, void* mask, void* stream) {
  ODVAE_CHECK_ARG(d_images && d_geom && d_mask_rect && d_tables && d_mults && patch && mask, "patch_reduce_resize: null pointer");
  ODVAE_CHECK_ARG(B > 0 && S > 0 && S <= 4096 && n_slots > 0, "patch_reduce_resize: bad sizes");
  PatchParams p;
  p.images = (const uint8_t* const*)d_images; p.geom = (const int32_t*)d_geom; p.mask_rect = (const int32_t*)d_mask_rect;
  p.tables = (const int32_t*)d_tables; p.mults = (const uint32_t*)d_mults; p.patch = (float*)patch; p.mask = (float*)mask;
  p.B = B; p.S = S; p.n_slots = n_slots;
  ODVAE_CHECK_ARG(B <= 65535 && (int64_t)B * S * S < (int64_t)1 << 31, "patch_reduce_resize: batch too large for one launch");
  hipLaunchKernelGGL(patch_reduce_resize_kernel, dim3(ceil_div(S, 64), ceil_div(S, 4), B), dim3(256), 0, static_cast<hipStream_t>(stream), p);
  ODVAE_LAUNCH_CHECK("patch_reduce_resize_kernel");
  return 0;
}
