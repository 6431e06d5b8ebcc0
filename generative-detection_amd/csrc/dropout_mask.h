// ResnetBlock dropout as a pure function of (seed, element index, p), shared by the f32 and bf16 GroupNorm kernels.
// dropout_mask.py restates it in numpy; the two must stay in step.
//
// One Philox4x32-10 call (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants) covers the 8
// consecutive channels of one pixel of the NHWC tensor [N][HW][C], C % 8 == 0:
//   octet   g = ((n * HW + px) * C + c) / 8                      (64-bit)
//   counter = (lo32(g), hi32(g), 0, 0),  key = (lo32(seed), hi32(seed))
//   the four output words are eight 16-bit lanes: channel 8g + 2j is the low half of word j, channel 8g + 2j + 1 the high half
//   dropped iff lane < thr, thr = round(p * 65536) in [0, 65536] (a 32-bit compare, so p = 1 drops everything);
//   kept elements are multiplied by scale = f32(1 / (1 - p)), and scale = 0 at p = 1 (no inf * 0).
// 16-bit lanes: v_mul_hi_u32 / v_mul_lo_u32 are quarter rate, and one call per 8 elements is half the integer work of 32-bit lanes.
#pragma once
#include <math.h>
#include <stdint.h>

struct GnDrop {
  unsigned thr;        // lane < thr: dropped
  float scale;         // multiplier of the kept elements
  unsigned key0, key1; // the seed's low / high word
};

// What a DROP = false kernel takes in GnDrop's place: an empty last argument, so those instantiations have the instruction streams they
// had before the dropout existed.  File-local like the kernels it parametrises (each includer keeps them in its unnamed namespace).
namespace { struct GnNoDrop {}; }

// p in [0, 1] (checked by the caller)
static inline GnDrop make_gn_drop(double p, unsigned long long seed) {
  GnDrop d;
  double t = nearbyint(p * 65536.0);      // round half to even, as numpy.rint
  t = t < 0.0 ? 0.0 : (t > 65536.0 ? 65536.0 : t);
  d.thr = (unsigned)t;
  d.scale = p < 1.0 ? (float)(1.0 / (1.0 - p)) : 0.f;
  d.key0 = (unsigned)(seed & 0xFFFFFFFFull);
  d.key1 = (unsigned)(seed >> 32);
  return d;
}

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&out)[4]) {
  constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += W0; k1 += W1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// multipliers (0 or scale) of the 8 channels of octet g
__device__ __forceinline__ void gn_drop_octet(const GnDrop& d, int64_t g, float (&m)[8]) {
  unsigned w[4];
  philox4x32_10((unsigned)((uint64_t)g & 0xFFFFFFFFull), (unsigned)((uint64_t)g >> 32), 0u, 0u, d.key0, d.key1, w);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    m[2 * j] = (w[j] & 0xFFFFu) < d.thr ? 0.f : d.scale;
    m[2 * j + 1] = (w[j] >> 16) < d.thr ? 0.f : d.scale;
  }
}

// the same for one channel quad (f32 kernels: a thread holds 4 channels): quad index i = (n * HW + px) * C / 4 + c / 4 lies in octet
// i / 2 and takes words 0, 1 (even i) or 2, 3 (odd i) of its call
__device__ __forceinline__ void gn_drop_quad(const GnDrop& d, int64_t quad, float (&m)[4]) {
  unsigned w[4];
  philox4x32_10((unsigned)((uint64_t)(quad >> 1) & 0xFFFFFFFFull), (unsigned)((uint64_t)(quad >> 1) >> 32), 0u, 0u, d.key0, d.key1, w);
  const bool odd = quad & 1;
  const unsigned a = odd ? w[2] : w[0], b = odd ? w[3] : w[1];
  m[0] = (a & 0xFFFFu) < d.thr ? 0.f : d.scale;
  m[1] = (a >> 16) < d.thr ? 0.f : d.scale;
  m[2] = (b & 0xFFFFu) < d.thr ? 0.f : d.scale;
  m[3] = (b >> 16) < d.thr ? 0.f : d.scale;
}
