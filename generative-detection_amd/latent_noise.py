"""The latent stage's device-side draws on the host: a numpy restatement of csrc/latent_noise.h.  No GPU is needed.  The header and
this module must stay in step.

With `model.params.device_noise = <seed>` the kernels make posterior_eps, the z_obj dropout mask, z_noise, bbox_eps and samples_eps from
(key, global step, tag, element index) and keep no tensor of them; this module rebuilds what a forward pass drew:

  one Philox4x32-10 call (dropout_mask.philox4x32_10) covers a quad of four consecutive elements of a stream:
    element e = flat index in the output's memory order (NHWC for the latent), quad g = (first + e) >> 2, lane = (first + e) & 3
    counter = (lo32(g), hi32(g), lo32(global_step), tag),  key = (lo32(s), hi32(s)),  s = (seed + rank * 0x9E3779B97F4A7C15) mod 2^64
    tag     = stream << 29 | training << 28 | (call & 0x0FFFFFFF); `call` counts the model's forwards since global_step or training
              last changed
  normal (Box-Muller): lanes 0, 1 take words 0, 1 and lanes 2, 3 words 2, 3 as (wa, wb):
    u1 = ((wa >> 9) + 0.5) * 2^-23, u2 = ((wb >> 9) + 0.5) * 2^-23   (exact in float32, never 0 or 1)
    r = sqrt(-2 ln u1); even lane r cos(2 pi u2), odd lane r sin(2 pi u2).  u1 >= 2^-24: the tail ends at sqrt(48 ln 2) = 5.77 sigma.
  dropout multiplier: lane j takes word j; kept iff word >= thr, thr = round-half-even(p * 2^32) clipped to [0, 2^32]; kept elements are
    multiplied by scale = float32(1 / (1 - p)), and scale = 0 at p = 1.

The words and the dropout multipliers are the kernels' bit for bit.  The normals are computed here in float64 from the same (exact)
uniforms: the yardstick the kernels' float32 logf / sqrtf / sincospif are measured against (profiles/device_noise.md).
"""
from collections import namedtuple

import numpy as np

from .dropout_mask import philox4x32_10

STREAMS = {"posterior_eps": 0, "dropout": 1, "z_noise": 2, "bbox_eps": 3, "samples_eps": 4}
RANK_STRIDE = 0x9E3779B97F4A7C15      # 2^64 / golden ratio: the keys of neighbouring ranks differ in every byte
KIND_NORMAL, KIND_DROPOUT = 0, 1
CALL_MASK = 0x0FFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF

# What a kernel call needs to name its draws: the 64-bit Philox key, lo32(global_step) and the tag (of stream 0: with_stream moves it)
Draw = namedtuple("Draw", ["key", "step", "tag"])


def device_key(seed, rank=0):
    """s = (seed + rank * RANK_STRIDE) mod 2^64: the key's two words are lo32(s), hi32(s)."""
    return (int(seed) + int(rank) * RANK_STRIDE) & _M64


def make_tag(stream, training, call):
    stream = STREAMS[stream] if isinstance(stream, str) else int(stream)
    if not 0 <= stream < 8:
        raise ValueError("stream id %r does not fit the tag's three bits" % (stream,))
    return (stream << 29) | (int(bool(training)) << 28) | (int(call) & CALL_MASK)


def make_draw(seed, rank, global_step, training, call):
    """The descriptor of one forward: stream 0's tag; the other streams of the same forward are with_stream(draw, ...)."""
    return Draw(device_key(seed, rank), int(global_step) & 0xFFFFFFFF, make_tag(0, training, call))


def with_stream(draw, stream):
    stream = STREAMS[stream] if isinstance(stream, str) else int(stream)
    return Draw(draw.key, draw.step, (draw.tag & 0x1FFFFFFF) | (stream << 29))


def words(draw, first, n):
    """The Philox words of elements first .. first + n - 1 (python ints: the index is 64-bit): four uint32 arrays [quads] and the lane of
    every element -- (w0, w1, w2, w3), quad index per element (into the arrays), lane per element."""
    first, n = int(first), int(n)
    e = np.arange(n, dtype=np.uint64) + np.uint64(first)
    g0 = first >> 2
    nq = ((first + n - 1) >> 2) - g0 + 1
    g = np.arange(nq, dtype=np.uint64) + np.uint64(g0)
    w = philox4x32_10((g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), draw.step & 0xFFFFFFFF, draw.tag & 0xFFFFFFFF),
                      (draw.key & 0xFFFFFFFF, (draw.key >> 32) & 0xFFFFFFFF))
    return w, ((e >> np.uint64(2)) - np.uint64(g0)).astype(np.int64), (e & np.uint64(3)).astype(np.int64)


def uniforms(w):
    """((w >> 9) + 0.5) * 2^-23 in float64: the float32 value the kernels hold, exactly."""
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normals(draw, first, n):
    """Elements first .. first + n - 1 of the normal stream in draw.tag, float64 (the yardstick of the kernels' float32)."""
    w, q, lane = words(draw, first, n)
    pair = lane >> 1
    wa = np.where(pair == 0, w[0][q], w[2][q])
    wb = np.where(pair == 0, w[1][q], w[3][q])
    r = np.sqrt(-2.0 * np.log(uniforms(wa)))
    ang = 2.0 * np.pi * uniforms(wb)
    return np.where((lane & 1) == 0, r * np.cos(ang), r * np.sin(ang))


def dropout_threshold(p):
    """thr of the kernels: a 32-bit word below it is dropped (2^32 drops everything)."""
    if not 0.0 <= p <= 1.0:
        raise ValueError("dropout probability has to be between 0 and 1, but got %r" % (p,))
    return int(min(max(np.rint(float(p) * 4294967296.0), 0.0), 4294967296.0))


def dropout_scale(p):
    """Multiplier of the kept elements, as the kernels round it: float32(1 / (1 - p)), 0 at p = 1."""
    if not 0.0 <= p <= 1.0:
        raise ValueError("dropout probability has to be between 0 and 1, but got %r" % (p,))
    return np.float32(1.0 / (1.0 - float(p))) if p < 1.0 else np.float32(0.0)


def dropout_multipliers(draw, first, n, p):
    """Elements first .. first + n - 1 of the dropout stream in draw.tag: float32, 0 where dropped, scale where kept -- the kernels' bits."""
    w, q, lane = words(draw, first, n)
    word = np.choose(lane, [w[0][q], w[1][q], w[2][q], w[3][q]]).astype(np.uint64)
    return np.where(word >= np.uint64(dropout_threshold(p)), dropout_scale(p), np.float32(0.0)).astype(np.float32)


class CallCounter:
    """`call` of the tag: the model's forwards since global_step or training last changed.  It keeps the micro-batches of an accumulation
    window, validation batches and log_images apart, and it is not state: a resumed run starts the step it resumes at with call 0, as the
    uninterrupted run did."""

    def __init__(self):
        self.at = None
        self.call = 0

    def next(self, global_step, training):
        at = (int(global_step), bool(training))
        if at != self.at:
            self.at, self.call = at, 0
        call = self.call
        self.call += 1
        return call
