"""The ResnetBlock dropout mask on the host: a numpy restatement of csrc/dropout_mask.h, bit for bit.  No GPU is needed.

The HIP GroupNorm kernels make the mask of `ddconfig.dropout` from (seed, element index, p) and keep no mask tensor; with the seed a
block drew (`ResnetBlock.last_dropout_seed`) this module rebuilds the very mask a forward pass used:

  one Philox4x32-10 call (Salmon et al., SC'11; the Random123 constants) covers the 8 consecutive channels of one pixel of the NHWC
  tensor [N][HW][C], C % 8 == 0:
    octet   g = ((n * HW + px) * C + c) // 8                      (64-bit)
    counter = (lo32(g), hi32(g), 0, 0),  key = (lo32(seed), hi32(seed))
    the four output words are eight 16-bit lanes: channel 8g + 2j is the low half of word j, channel 8g + 2j + 1 the high half
  an element is dropped iff lane < thr, thr = round-half-even(p * 65536) clipped to [0, 65536]  (p = 1 drops everything);
  kept elements are multiplied by scale = float32(1 / (1 - p)), and scale = 0 at p = 1.
"""
import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57      # round multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85      # Weyl increments of the key
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds.  counter: four and key: two arrays (or scalars) of 32-bit words, broadcast against each other;
    returns the four output words as a tuple of uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK32 for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & _MASK32 for v in key]
    if len(c) != 4 or len(k) != 2:
        raise ValueError("philox4x32_10 takes a 4-word counter and a 2-word key")
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    s32 = np.uint64(32)
    for r in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & _MASK32, (p0 >> s32) ^ c[3] ^ k[1], p0 & _MASK32]
        k = [(k[0] + np.uint64(PHILOX_W0)) & _MASK32, (k[1] + np.uint64(PHILOX_W1)) & _MASK32]
    return tuple(v.astype(np.uint32) for v in c)


def dropout_threshold(p):
    """thr of the kernels: a 16-bit lane below it is dropped."""
    if not 0.0 <= p <= 1.0:
        raise ValueError("dropout probability has to be between 0 and 1, but got %r" % (p,))
    return int(min(max(np.rint(float(p) * 65536.0), 0.0), 65536.0))


def dropout_scale(p):
    """Multiplier of the kept elements, as the kernels round it: float32(1 / (1 - p)), 0 at p = 1."""
    if not 0.0 <= p <= 1.0:
        raise ValueError("dropout probability has to be between 0 and 1, but got %r" % (p,))
    return np.float32(1.0 / (1.0 - float(p))) if p < 1.0 else np.float32(0.0)


def dropout_lanes(seed, first_octet, octets):
    """The 16-bit lanes of `octets` consecutive octets starting at octet index `first_octet` (python ints: the index is 64-bit):
    uint32 array [octets][8], lane j of an octet belongs to its channel j."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    g = np.arange(int(octets), dtype=np.uint64) + np.uint64(int(first_octet))
    w = philox4x32_10((g & _MASK32, g >> np.uint64(32), 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
    lanes = np.empty((int(octets), 8), dtype=np.uint32)
    for j in range(4):
        lanes[:, 2 * j] = w[j] & np.uint32(0xFFFF)
        lanes[:, 2 * j + 1] = w[j] >> np.uint32(16)
    return lanes


def resnet_dropout_keep_nhwc(seed, p, n, c, h, w):
    """The scaled keep mask in the kernels' memory order: float32 numpy array [n][h][w][c], 0 where dropped, scale where kept."""
    if c % 8 != 0:
        raise ValueError("the dropout mask is defined for C %% 8 == 0, got C=%d" % c)
    lanes = dropout_lanes(seed, 0, n * h * w * c // 8)
    keep = lanes >= np.uint32(dropout_threshold(p)) if dropout_threshold(p) < 65536 else np.zeros(lanes.shape, dtype=bool)
    return np.where(keep, dropout_scale(p), np.float32(0.0)).astype(np.float32).reshape(n, h, w, c)


def resnet_dropout_keep(seed, p, n, c, h, w):
    """The scaled keep mask of a [n, c, h, w] activation as a logical-NCHW float32 torch tensor (CPU): multiply the undropped
    activation by it to get what the kernels computed with (seed, p)."""
    import torch
    return torch.from_numpy(resnet_dropout_keep_nhwc(seed, p, n, c, h, w)).permute(0, 3, 1, 2)
