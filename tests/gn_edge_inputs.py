"""GroupNorm at the shapes the model never runs: case tables, inputs with a bit-for-bit answer, host-built partial sums.

Every other GroupNorm test uses 32 groups and a power-of-two channel count.  The kernels (csrc/groupnorm.hip, csrc/bf16_ops.hip,
csrc/gn_finalize.h) have whole branches for other shapes -- a generic apply path where 256 % (C / 4) != 0, channel slices of
CB = (64 / cpg) * cpg < 64 in the backward finalize, a serial finalize for groups wider than 64 channels, statistics picked per element
where a group is narrower than a thread's quad or octet -- and this module names a case for each (`F32_CASES`, `BF16_CASES`, every
row with the branch facts it claims; tests/test_gn_edge_inputs.py recomputes them from `shape_f32` / `shape_bf16`, the host
restatements of the two `make_shape`).  All tensors here are [N][HW][C], the C ABI's layout; `nchw` / `nhwc` go to and from the
[n, c, hw, 1] that tests/gn_offset_inputs.py (references, acceptance rule: reused, not copied) works on.

Exact inputs (`exact_case`): per (sample, group) an integer offset m and a power-of-two spread s; the group holds m + s and m - s in
equal numbers (and one m where its size is odd), shuffled.  All values are integers of at most 8 significant bits, every partial sum
of x and x^2 is an integer below 2^24, so the f32 sums of any kernel are exact in any order and so is the float64 finalize:
mean = m, var = s^2 (count - odd) / count, and with gamma = +-2^k, beta = 0 and no swish
    y = f32(f64(x - m) * f64(rstd_f32)) * gamma            (one rounding; the power of two changes no bit)
whether or not the compiler contracts the multiply-add.  Two regimes: "near" (|m| <= 3 s: the recentring of gn_finalize_kernel must
not run) and "far" (|m| = 32 s: it must run for every group); the prediction is the same, the centred sums being exact too.
Plain module: torch / numpy on the host only.
"""
import numpy as np
import torch

import gn_offset_inputs as G

EPS = G.EPS
RECENTRE_RATIO = 8.0                       # GN_RECENTRE_RATIO of csrc/gn_finalize.h
FWD_CHUNK_COUNTS = (1, 3, 64, 65, 130)     # caller-supplied [N][chunks][G][2]: both sides of one wavefront of gn_finalize_kernel
BWD_CHUNK_COUNTS = (1, 3, 4, 5, 9)         # caller-supplied [N][chunks][2][C]: the four wavefronts of gn_bwd_finalize_kernel take every fourth
DROP_PS = (0.0, 0.5, 1.0)
DROP_SEED = 0x9E3779B97F4A7C15
REGIMES = ("near", "far")
RULE_RATIOS = (0, 4)                       # gn_offset_inputs.make_input(r=...): the regime training is in

# ---- case tables: (n, c, g, hw, claimed branch facts) --------------------------------------------------------------------------------
# facts (all recomputed by `facts`): vec = C / 4 (f32: quads) or C / 8 (bf16: octs); generic = 256 % vec != 0 (f32 apply kernels reload
# the constants per element); ppp = pix_per_pass = 256 // vec (256 - ppp * vec threads of the statistics / reduce kernels idle); cpg;
# cb = (64 // cpg) * cpg, the channel slice of gn_bwd_finalize_kernel; wide = cpg > 64 (gn_bwd_finalize_wide_kernel); chunks and
# last = length of the last chunk of the library's own split; read_once = the default backward takes the read-once kernel
F32_CASES = [
    (2, 96, 32, 70, dict(generic=True, vec=24, ppp=10, idle=16, cpg=3, cb=63, chunks=2, last=35)),      # generic path, cpg 3, one dead lane per slice
    (1, 160, 32, 33, dict(generic=True, vec=40, ppp=6, idle=16, cpg=5, cb=60, chunks=1, last=33)),      # cpg 5, quads 40, HW < 64
    (2, 192, 32, 65, dict(generic=True, vec=48, ppp=5, idle=16, cpg=6, cb=60, chunks=2, last=32)),      # cpg 6, HW just past 64
    (1, 384, 32, 130, dict(generic=True, vec=96, ppp=2, idle=64, cpg=12, cb=60, chunks=3, last=42)),    # quads 96: a whole wavefront idle, three ragged chunks
    (1, 640, 32, 7, dict(generic=True, vec=160, ppp=1, idle=96, cpg=20, cb=60, chunks=1, last=7)),      # cpg 20, 96 idle threads, one pixel per pass
    (3, 4, 1, 300, dict(generic=False, vec=1, ppp=256, cpg=4, cb=64, chunks=5, last=60, read_once=False)),   # one quad, one group; N * G = 3 leaves a finalize wavefront without work
    (2, 4, 4, 5, dict(generic=False, vec=1, ppp=256, cpg=1, chunks=1, last=5)),                          # cpg 1 inside a quad, HW < pix_per_pass
    (1, 256, 256, 64, dict(generic=False, vec=64, ppp=4, cpg=1, cb=64, chunks=1, read_once=True)),       # G at its limit
    (2, 1024, 32, 17, dict(generic=False, vec=256, ppp=1, cpg=32, cb=64, chunks=1, read_once=True)),     # quads 256: C at its limit, four-load loop + one tail load
    (1, 1024, 8, 66, dict(cpg=128, wide=True, chunks=2, last=33, read_once=False)),                      # wide finalize over two chunks
    (2, 512, 4, 9, dict(cpg=128, wide=True, chunks=1, read_once=False)),                                 # wide finalize, power-of-two path
    (5, 64, 2, 255, dict(cpg=32, wide=False, cb=64, chunks=4, last=63, read_once=True)),                 # read-once by default, last pixel row short
    (5, 64, 2, 256, dict(cpg=32, chunks=4, last=64, read_once=True)),                                    # read-once by default, a block exactly full
    (5, 64, 2, 257, dict(cpg=32, chunks=5, last=49, read_once=False)),                                   # one pixel past it: the two-kernel form
    (2, 128, 64, 1, dict(cpg=2, ppp=8, chunks=1, last=1, read_once=True)),                               # HW = 1: two values per group
    (600, 32, 32, 129, dict(cpg=1, vec=8, ppp=32, chunks=3, last=43, read_once=True)),                   # many samples, few chunks; more items than resident blocks
    (1100, 32, 8, 3, dict(cpg=4, chunks=1, last=3, read_once=True)),                                     # read-once with more than two items per resident block: its registers are refilled
]
BF16_CASES = [
    (2, 8, 1, 70, dict(vec=1, ppp=256, cpg=8, cb=64, chunks=2, last=35)),          # one octet
    (2, 8, 8, 5, dict(vec=1, cpg=1, chunks=1, last=5)),                            # cpg 1 inside an octet, HW < pix_per_pass
    (1, 16, 4, 33, dict(vec=2, ppp=128, cpg=4, chunks=1)),                         # cpg 4: two groups per octet
    (2, 64, 32, 65, dict(vec=8, ppp=32, cpg=2, chunks=2, last=32)),                # cpg 2
    (1, 128, 32, 130, dict(vec=16, ppp=16, cpg=4, chunks=3, last=42)),             # cpg 4, ragged chunks
    (1, 2048, 32, 9, dict(vec=256, ppp=1, cpg=64, cb=64, wide=False, chunks=1)),   # octs 256: C at its limit, the widest group of the sliced finalize
    (2, 2048, 256, 3, dict(vec=256, cpg=8, chunks=1, last=3)),                     # G at its limit
    (2, 512, 4, 66, dict(cpg=128, wide=True, chunks=2, last=33)),                  # wide finalize over two chunks
    (1, 1024, 2, 17, dict(cpg=512, wide=True, chunks=1)),                          # wide finalize, 512 channels per group
    (3, 64, 32, 1, dict(cpg=2, chunks=1, last=1)),                                 # HW = 1 (a group needs two values: cpg 2)
]
CASES = {"f32": F32_CASES, "bf16": BF16_CASES}

# ---- refused shapes: (n, c, g, hw, why); `drop_only`: the plain forms take the shape, the dropout forms do not -------------------------
F32_REFUSED = [
    (1, 6, 1, 8, "C % 4"), (1, 1028, 4, 4, "C > 1024"), (1, 1028, 257, 4, "G = 257"), (1, 512, 512, 4, "G > 256"),
    (1, 96, 36, 8, "C % G"), (65536, 4, 1, 1, "N > 65535"),
]
F32_REFUSED_DROP_ONLY = [(1, 100, 25, 8, "the dropout mask needs C % 8 == 0")]
BF16_REFUSED = [
    (1, 96, 32, 8, "256 % (C / 8)"), (1, 4, 1, 8, "C % 8"), (1, 4096, 32, 2, "C > 2048"), (1, 1024, 512, 4, "G > 256"),
    (1, 64, 24, 8, "C % G"), (65536, 8, 1, 1, "N > 65535"),
]
REFUSED = {"f32": F32_REFUSED, "bf16": BF16_REFUSED}


def case_id(case):
    return "n%d-c%d-g%d-hw%d" % tuple(case[:4])


def _ceil_div(a, b):
    return -(-a // b)


def _shape(n, hw, c, g, lanes, cmax_vec):
    """make_shape of csrc/groupnorm.hip (lanes = 4) and csrc/bf16_ops.hip (lanes = 8), restated; None where the library refuses"""
    if n <= 0 or hw <= 0 or c <= 0 or g <= 0 or c % g or c % lanes:
        return None
    vec = c // lanes
    if vec > cmax_vec or (lanes == 8 and 256 % vec) or g > 256 or hw * vec >= 2 ** 31 or n > 65535:
        return None
    chunks = max(1, min(_ceil_div(2048, n), _ceil_div(hw, 64)))
    ppc = _ceil_div(hw, chunks)
    chunks = _ceil_div(hw, ppc)
    return dict(n=n, hw=hw, c=c, g=g, cpg=c // g, vec=vec, ppp=256 // vec, chunks=chunks, ppc=ppc, last=hw - (chunks - 1) * ppc)


def shape_f32(n, hw, c, g):
    return _shape(n, hw, c, g, 4, 256)


def shape_bf16(n, hw, c, g):
    return _shape(n, hw, c, g, 8, 256)


def shape_of(dt, n, hw, c, g):
    return shape_bf16(n, hw, c, g) if dt == "bf16" else shape_f32(n, hw, c, g)


def read_once_by_default(s):
    """gn_fused_plan with T = 1 (f32 only): 32-channel slabs of whole groups, one block holds a sample's pixels"""
    return s["c"] % 32 == 0 and s["cpg"] <= 32 and 32 % s["cpg"] == 0 and s["hw"] <= 256


def facts(dt, n, c, g, hw):
    s = shape_of(dt, n, hw, c, g)
    out = dict(vec=s["vec"], generic=256 % s["vec"] != 0, ppp=s["ppp"], idle=256 - s["ppp"] * s["vec"], cpg=s["cpg"], wide=s["cpg"] > 64,
               cb=(64 // s["cpg"]) * s["cpg"] if s["cpg"] <= 64 else None, chunks=s["chunks"], last=s["last"])
    if dt == "f32":
        out["read_once"] = read_once_by_default(s)
    return out


def workspace_floats(s, which):
    """what the kernels of one entry point write, in floats: "fwd" [N][chunks][G][2]; "bwd" [N][chunks][2][C] + chan [N][2][C] + grp
    [N][G][2]; "bwd_partials" chan + grp"""
    n, c, g = s["n"], s["c"], s["g"]
    tail = n * 2 * c + n * g * 2
    return {"fwd": n * s["chunks"] * g * 2, "bwd": n * s["chunks"] * 2 * c + tail, "bwd_partials": tail}[which]


def workspace_bytes(dt, s):
    """odvae_groupnorm_workspace_bytes / odvae_groupnorm_bf16_workspace_bytes restated: the larger of forward and backward, and for f32
    what the read-once backward needs where the library plans it (arrival counters rounded to 256 bytes + its one-member partials)"""
    need = 4 * max(workspace_floats(s, "fwd"), workspace_floats(s, "bwd"))
    if dt == "f32" and s["c"] % 32 == 0 and s["cpg"] <= 32 and 32 % s["cpg"] == 0:
        # gn_fused_plan: teams of T = ceil(HW / 256) blocks (T far below the resident blocks of the device for every shape of the tables);
        # one counter per (sample, 32-channel slab), partials [N][T][2][C]
        items, team = s["n"] * (s["c"] // 32), _ceil_div(s["hw"], 256)
        need = max(need, _ceil_div(items * 4, 256) * 256 + 4 * (s["n"] * team * 2 * s["c"] + workspace_floats(s, "bwd_partials")))
    return need


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------
def nchw(t):
    """[n, hw, c] -> [n, c, hw, 1], what gn_offset_inputs' references take"""
    return t.permute(0, 2, 1).unsqueeze(3).contiguous()


def nhwc(t):
    """[n, c, hw, 1] -> [n, hw, c]"""
    return t.squeeze(3).permute(0, 2, 1).contiguous()


# ---- bf16 ------------------------------------------------------------------------------------------------------------------------------
def bf16_bits(t):
    """round-to-nearest-even of finite f32 values to bf16: the 16 bits, as int32"""
    u = t.detach().float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).to(torch.int32)


def bf16_round(t):
    """the f32 values of `bf16_bits`"""
    return (bf16_bits(t).to(torch.int64) << 16).to(torch.int32).view(torch.float32).reshape(t.shape)


def is_bf16(t):
    return bool(torch.equal(bf16_round(t), t.float()))


def half_ulp_bf16(q):
    """half a unit in the last place of bf16 at |q| (float64 tensor): bf16 keeps 8 significant bits, so for 2^e <= |q| < 2^(e+1) a
    unit is 2^(e-7) and a round-to-nearest moves a value by at most 2^(e-8); e >= -126 (below, the subnormal spacing)"""
    _, exp = torch.frexp(q.double().abs())            # |q| = mant 2^exp, mant in [0.5, 1): e = exp - 1
    exp = torch.where(q == 0, torch.full_like(exp, -1000), exp)      # (frexp gives 0 an exponent of 0)
    return torch.ldexp(torch.ones_like(q, dtype=torch.float64), torch.clamp(exp - 1, min=-126) - 8)


# ---- exact inputs ------------------------------------------------------------------------------------------------------------------------
def exact_gamma(c):
    """gamma_c = +-2^k, k in -6..5: the eight channels of an octet (so the four of a quad) all differ, neighbouring octets differ in k
    and in sign"""
    ch = torch.arange(c)
    k = (ch % 8) + ((ch // 8) % 5) - 6
    sign = 1.0 - 2.0 * (((ch // 4) + (ch // 8)) % 2).float()
    return (sign * torch.pow(torch.tensor(2.0), k.float())).float()


class ExactCase:
    """x [n, hw, c] (f32 tensor of small integers) and everything the kernels must make of it, for one case and regime"""

    def __init__(self, n, c, g, hw, regime):
        assert regime in REGIMES
        cpg, count = c // g, (c // g) * hw
        assert count >= 2
        self.n, self.c, self.g, self.hw, self.cpg, self.count, self.regime = n, c, g, hw, cpg, count, regime
        lim = int(np.floor(np.sqrt((2 ** 24 - 1) / count)))      # |x| <= lim keeps count * x^2 below 2^24
        ni, gi = np.meshgrid(np.arange(n), np.arange(g), indexing="ij")
        shift = (ni + 2 * gi) % 3
        if regime == "far":
            smax = min(4, 1 << int(np.log2(lim // 33)))
            s = np.maximum(1, smax >> shift)
            m = 32 * s * (1 - 2 * ((ni + gi) % 2))
        else:
            # |m| <= 3 s, not 4 s: an odd group of 5 values has std = s sqrt(4 / 5), and |m| / std has to stay at or below half the threshold
            smax = min(16, 1 << int(np.log2(lim // 4)))
            s = np.maximum(1, smax >> shift)
            m = (3 * gi + 5 * ni + 1) % (6 * s + 1) - 3 * s
        assert (np.abs(m) + s).max() <= min(lim, 256)
        self.m, self.s = m.astype(np.int64), s.astype(np.int64)
        rng = np.random.default_rng(1000003 * n + 7919 * c + 31 * g + hw + (17 if regime == "far" else 0))
        pattern = np.concatenate([np.ones(count // 2), -np.ones(count // 2), np.zeros(count % 2)]).astype(np.int64)
        pat = rng.permuted(np.tile(pattern, (n, g, 1)), axis=2)
        xg = self.m[:, :, None] + self.s[:, :, None] * pat                                # [n, g, count], count = hw x cpg
        x = xg.reshape(n, g, hw, cpg).transpose(0, 2, 1, 3).reshape(n, hw, c)
        self.x64 = x                                                                      # int64 numpy
        self.x = torch.from_numpy(x.astype(np.float32))
        self.gamma, self.beta = exact_gamma(c), torch.zeros(c)
        # the prediction
        self.var = (self.s * self.s * (count - count % 2)).astype(np.float64) / np.float64(count)
        self.mean = torch.from_numpy(self.m.astype(np.float32))
        rstd = (1.0 / np.sqrt(self.var + np.float64(np.float32(EPS)))).astype(np.float32)
        self.rstd = torch.from_numpy(rstd)
        d = (x - np.repeat(self.m, cpg, axis=1)[:, None, :]).astype(np.float64)           # x - m, exact
        prod = (d * np.repeat(rstd.astype(np.float64), cpg, axis=1)[:, None, :]).astype(np.float32)
        self.y = torch.from_numpy(prod) * self.gamma                                      # f32; a power of two: exact
        self.y_bf16 = bf16_round(self.y)
        self.recentred = n * g if regime == "far" else 0

    def y64(self):
        """the same by a float64 evaluation of (x - mean) / sqrt(var + eps) * gamma from the f32 statistics, not yet rounded"""
        cpg = self.cpg
        d = self.x64.astype(np.float64) - np.repeat(self.mean.numpy().astype(np.float64), cpg, axis=1)[:, None, :]
        return torch.from_numpy(d * np.repeat(self.rstd.numpy().astype(np.float64), cpg, axis=1)[:, None, :]) * self.gamma.double()

    def dropped(self, p, dt="f32"):
        """y * keep * scale with the mask of odvae_amd/dropout_mask.py (scale 1, 2 and 0 at p = 0, 0.5 and 1: exact)"""
        from odvae_amd import dropout_mask as dm
        keep = torch.from_numpy(dm.resnet_dropout_keep_nhwc(DROP_SEED, p, self.n, self.c, self.hw, 1)).reshape(self.n, self.hw, self.c)
        y = self.y * keep
        return bf16_round(y) if dt == "bf16" else y


_EXACT = {}


def exact_case(case, regime):
    key = tuple(case[:4]) + (regime,)
    if key not in _EXACT:
        _EXACT[key] = ExactCase(*case[:4], regime)
    return _EXACT[key]


# ---- caller-supplied partial sums ----------------------------------------------------------------------------------------------------------
def cuts(hw, chunks, seed):
    """chunks + 1 non-decreasing pixel boundaries from 0 to hw at arbitrary places (chunks may be empty: their sums are zero)"""
    rng = np.random.default_rng(seed)
    inner = np.sort(rng.integers(0, hw + 1, size=chunks - 1))
    return np.concatenate([[0], inner, [hw]]).astype(np.int64)


def _chunk_sums(per_pixel, chunks, seed):
    """per_pixel [n, hw, k] float64 -> [n, chunks, k] f32: sums over the pixels of each chunk in float64, rounded once"""
    n, hw, k = per_pixel.shape
    cum = torch.cat([torch.zeros(n, 1, k, dtype=torch.float64), torch.cumsum(per_pixel, 1)], 1)
    b = torch.from_numpy(cuts(hw, chunks, seed))
    return (cum[:, b[1:]] - cum[:, b[:-1]]).float()


def fwd_partials(x, g, chunks, seed=0):
    """[N][chunks][G][2] f32 = (sum, sum of squares) of x [n, hw, c] per chunk of pixels and channel group"""
    n, hw, c = x.shape
    xg = x.double().reshape(n, hw, g, c // g)
    both = torch.stack([xg.sum(3), (xg * xg).sum(3)], 3).reshape(n, hw, 2 * g)
    return _chunk_sums(both, chunks, seed + 101 * chunks).reshape(n, chunks, g, 2).contiguous()


def act_grad64(u, swish):
    if not swish:
        return torch.ones_like(u)
    sg = torch.sigmoid(u)
    return sg * (1.0 + u * (1.0 - sg))


def bwd_pixel_sums(x, dy, gamma, beta, swish, g):
    """float64 [n, hw, 2, c]: per element du * xhat and du, du = dy act'(xhat gamma + beta), statistics of x in float64"""
    n, hw, c = x.shape
    mean, rstd = G.stats64(nchw(x), g)
    xhat = (x.double().reshape(n, hw, g, c // g) - mean.reshape(n, 1, g, 1)) * rstd.reshape(n, 1, g, 1)
    xhat = xhat.reshape(n, hw, c)
    du = dy.double() * act_grad64(xhat * gamma.double() + beta.double(), swish)
    return torch.stack([du * xhat, du], 2)


def bwd_partials(x, dy, gamma, beta, swish, g, chunks, seed=0):
    """[N][chunks][2][C] f32 = per chunk of pixels and channel (sum du * xhat, sum du)"""
    n, hw, c = x.shape
    per = bwd_pixel_sums(x, dy, gamma, beta, swish, g).reshape(n, hw, 2 * c)
    return _chunk_sums(per, chunks, seed + 211 * chunks).reshape(n, chunks, 2, c).contiguous()


# ---- rule-based inputs -----------------------------------------------------------------------------------------------------------------
def rule_affine(c, seed=11):
    """gamma: c distinct values of magnitude 0.5 .. 2 with mixed signs, so that a wrong-channel or wrong-group pick is an O(1) error; beta: randn"""
    gen = torch.Generator().manual_seed(seed + c)
    mag = 0.5 + 1.5 * (torch.randperm(c, generator=gen).float() + 0.5) / c
    sign = 1.0 - 2.0 * (torch.arange(c) % 3 == 1).float()
    return (mag * sign).float(), torch.randn(c, generator=gen)


class RuleCase:
    """Random inputs of one (dtype, case, ratio) in [n, hw, c], held in the dtype's values (bf16: rounded first), and float64 / torch-f32
    references on demand (cached)."""

    def __init__(self, dt, n, c, g, hw, r):
        self.dt, self.n, self.c, self.g, self.hw, self.r = dt, n, c, g, hw, r
        rnd = bf16_round if dt == "bf16" else (lambda t: t)
        shape = (n, c, hw, 1)
        gen = torch.Generator().manual_seed(G.seed_of(shape, r, 1.0, 9) + g)
        count = (c // g) * hw
        if count >= 8:
            x4 = G.make_input(shape, r, 1.0, groups=g)
        else:
            # A handful of normal values can lie so close together that rstd nears its cap of 1000 and every rounding of x - mean is
            # amplified by it, in torch f32 as much as in a kernel (two bf16 values can even coincide).  Such a group says nothing about
            # the kernels, so groups of fewer than 8 values get a spread by construction: evenly spaced values of step a / count,
            # a in 1 .. 3, in shuffled order about the same offset r sign_g.
            z = (torch.arange(count).float() - (count - 1) / 2.0) / count
            order = torch.argsort(torch.rand(n, g, count, generator=gen), dim=2)
            xg = z[order] * (1.0 + 2.0 * torch.rand(n, g, 1, generator=gen))
            x4 = xg.reshape(n, g, hw, c // g).permute(0, 1, 3, 2).reshape(shape) + r * G.group_signs(c, g).view(1, c, 1, 1)
        self.x4 = rnd(x4.float())
        self.dy4 = rnd(torch.randn(shape, generator=gen))
        self.dskip4 = rnd(torch.randn(shape, generator=gen))
        self.gamma, self.beta = rule_affine(c)
        self.x, self.dy, self.dskip = nhwc(self.x4), nhwc(self.dy4), nhwc(self.dskip4)
        self.mean64, self.rstd64 = G.stats64(self.x4, g)
        self._fwd, self._bwd = {}, {}

    def forward_refs(self, swish):
        """(y64, y32, mean32, rstd32), y in [n, hw, c]"""
        if swish not in self._fwd:
            y32, mean32, rstd32 = G.ref32(self.x4, self.gamma, self.beta, swish, self.g)
            self._fwd[swish] = (nhwc(G.ref64(self.x4, self.gamma, self.beta, swish, self.g)), nhwc(y32), mean32, rstd32)
        return self._fwd[swish]

    def backward_refs(self, swish, mask=None):
        """{64: (dx, dgamma, dbeta), 32: ...} without the skip gradient, dx in [n, hw, c]; mask [n, hw, c]: of dy * mask (cached for one mask)"""
        key = (swish, mask is not None)
        if key not in self._bwd:
            dy4 = self.dy4 if mask is None else self.dy4 * nchw(mask)
            refs = G.backward_refs(self.x4, self.gamma, self.beta, dy4, swish, None, self.g)
            self._bwd[key] = {b: (nhwc(v[0]), v[1], v[2]) for b, v in refs.items()}
        return self._bwd[key]


_RULE = {}


def rule_case(dt, case, r):
    key = (dt,) + tuple(case[:4]) + (r,)
    if key not in _RULE:
        _RULE[key] = RuleCase(dt, *case[:4], r)
    return _RULE[key]


def bf16_elementwise(name, got, q64, q32, floor):
    """A bf16 output under the rule: |got - q64| <= half_ulp_bf16(q64) + bound elementwise, bound = gn_offset_inputs.bound of the same
    quantity (eight times torch f32's own error or the floor).  Returns a figure dict for gn_offset_inputs.check whose `err` is the
    largest excess over the half ulp, so that `inside` is exactly the elementwise statement."""
    got = got.detach().float().cpu().double()
    assert tuple(got.shape) == tuple(q64.shape), "%s: shape %s vs %s" % (name, tuple(got.shape), tuple(q64.shape))
    err_t = G.maxerr(q32, q64)
    excess = ((got - q64.double()).abs() - half_ulp_bf16(q64)).clamp(min=0.0).max().item()
    return {"name": name + " (bf16: excess over half an ulp)", "err": excess, "err_torch": err_t,
            "bound": G.bound(err_t, G.maxabs(q64), floor), "finite": bool(torch.isfinite(got).all())}
