// The latent stage's random draws as a pure function of (key, global step, tag, element index), made on the device.
// latent_noise.py restates it in numpy; the two must stay in step.
//
// One Philox4x32-10 call (dropout_mask.h) covers a quad of four consecutive elements of a stream:
//   element e = flat index in the output's memory order (NHWC for the latent), quad g = (first + e) >> 2, lane = (first + e) & 3
//   counter = (lo32(g), hi32(g), lo32(global_step), tag),  key = (lo32(s), hi32(s)),  s = (seed + rank * 0x9E3779B97F4A7C15) mod 2^64
//   tag     = stream << 29 | training << 28 | (call & 0x0FFFFFFF)
//             streams: 0 posterior_eps, 1 dropout, 2 z_noise, 3 bbox_eps, 4 samples_eps
// Normal (Box-Muller): lanes 0, 1 take words 0, 1 and lanes 2, 3 words 2, 3 as (wa, wb):
//   u1 = ((wa >> 9) + 0.5) * 2^-23, u2 = ((wb >> 9) + 0.5) * 2^-23   (exact in f32, never 0 or 1)
//   r = sqrt(-2 ln u1); even lane r cos(2 pi u2), odd lane r sin(2 pi u2).  u1 >= 2^-24, so |x| <= sqrt(48 ln 2) = 5.77.
//   logf / sqrtf / sincospif in full precision: the fast intrinsics' errors grow with the argument (README, the pose head's history).
// Dropout multiplier: lane j takes word j; kept iff (uint64)w >= thr, thr = rint(p * 2^32) in [0, 2^32]; kept elements are multiplied by
//   scale = f32(1 / (1 - p)), and scale = 0 at p = 1 (no inf * 0).
#pragma once
#include <math.h>
#include <stdint.h>
#include "dropout_mask.h"

enum { LN_STREAM_EPS = 0, LN_STREAM_DROPOUT = 1, LN_STREAM_NOISE = 2 };
enum { LN_KIND_NORMAL = 0, LN_KIND_DROPOUT = 1 };

struct LnDraw {
  unsigned key0, key1;  // the key's low / high word
  unsigned step;        // lo32(global_step)
  unsigned tag;         // the whole tag, or its low 29 bits where a kernel adds the stream itself
  uint64_t thr;         // dropout: word < thr is dropped (2^32 drops everything)
  float scale;          // dropout: multiplier of the kept elements
};

// p in [0, 1] (checked by the caller)
static inline LnDraw make_ln_draw(unsigned long long key, unsigned step, unsigned tag, double p) {
  LnDraw d;
  d.key0 = (unsigned)(key & 0xFFFFFFFFull);
  d.key1 = (unsigned)(key >> 32);
  d.step = step;
  d.tag = tag;
  double t = nearbyint(p * 4294967296.0);      // round half to even, as numpy.rint
  t = t < 0.0 ? 0.0 : (t > 4294967296.0 ? 4294967296.0 : t);
  d.thr = (uint64_t)t;
  d.scale = p < 1.0 ? (float)(1.0 / (1.0 - p)) : 0.f;
  return d;
}

__device__ __forceinline__ void ln_words(const LnDraw& d, unsigned tag, int64_t g, unsigned (&w)[4]) {
  philox4x32_10((unsigned)((uint64_t)g & 0xFFFFFFFFull), (unsigned)((uint64_t)g >> 32), d.step, tag, d.key0, d.key1, w);
}

// the two normals of one word pair.  Plain operators under contract(off): every product here is rounded on its own, wherever the
// function is inlined (the fill and the fused stage must give the same bits).
__device__ __forceinline__ void ln_normal_pair(unsigned wa, unsigned wb, float& even, float& odd) {
#pragma clang fp contract(off)
  const float u1 = ((float)(wa >> 9) + 0.5f) * 1.1920928955078125e-7f;
  const float u2 = ((float)(wb >> 9) + 0.5f) * 1.1920928955078125e-7f;
  const float r = sqrtf(-2.f * logf(u1));
  float s, c;
  sincospif(2.f * u2, &s, &c);
  even = r * c;
  odd = r * s;
}

// the four normals of quad g of the stream in `tag`
__device__ __forceinline__ void ln_normal_quad(const LnDraw& d, unsigned tag, int64_t g, float (&x)[4]) {
  unsigned w[4];
  ln_words(d, tag, g, w);
  ln_normal_pair(w[0], w[1], x[0], x[1]);
  ln_normal_pair(w[2], w[3], x[2], x[3]);
}

// the four dropout multipliers (0 or scale) of quad g of the stream in `tag`
__device__ __forceinline__ void ln_dropout_quad(const LnDraw& d, unsigned tag, int64_t g, float (&m)[4]) {
  unsigned w[4];
  ln_words(d, tag, g, w);
#pragma unroll
  for (int j = 0; j < 4; ++j) m[j] = (uint64_t)w[j] < d.thr ? 0.f : d.scale;
}
