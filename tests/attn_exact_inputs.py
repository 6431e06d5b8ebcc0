"""Attention inputs with closed-form answers for the bf16 flash-attention kernels: generators, float64 references, the two
preconditions, the checkers.

softmax(q k^T C^-1/2) v averages T values when q and k are Gaussian: one key is 1/T of an output, and a dropped key, a tile read from
the wrong ring stage or a row constant of the neighbouring tile stay under any max-abs tolerance.  Here the softmax is made to SELECT:
keys carry a +-1 code of their identity on a few columns, a query repeats the code of the key (or the group of keys) it wants, and
every other key lands >= 160 log2-units below -- its probability is 0 in f32, also under flush-to-zero.  What is left is arithmetic on
small integers, which the kernels (bf16 products, f32 sums, one bf16 rounding at the store) must get right bit for bit.

family  operands                                                          exact (bits)       closed form, toleranced
  A     q_i = k_pi(i): permutation, or many-to-one with unselected keys   o, dv, dq = dk = 0  lse2
  B     groups of g / g/2 keys share a code, different v, ~T/g apart      o, dv               lse2, dk, dq (0 for g <= 2)
  C     q = 0, k Gaussian: P = 1/T everywhere                             dk = 0, o (T = 2^n) lse2, o (1 ulp), dv, dq
  D     one key at level 0 + 128 keys at -9 / -6 log2-units               --                  o, lse2, dq, dk, dv
v and dO are integers in [-8, 8] drawn per (image, row, column).  The code columns sit at a seeded random subset of the C columns; on
the other columns q and k carry integer decoys on DISJOINT column sets, so they add nothing to any score unless columns are mixed up.

Preconditions (`assert_preconditions`, on the very tensors used; c = C^-1/2 log2 e):
  (P1) every non-selected scaled score lies >= 160 below the selected one, and the selected group spans <= 10: with the reference
       point m lagging by up to 8, a non-selected exponent is <= -142 < -126 -- v_exp_f32 returns 0.
  (P2) |s_sel c| < 2^13: one f32 rounding of m or lse2 is then <= 2^-11 absolute, the selected probability 2^(+-2^-11) is within 2^-11
       of its value, rounds to exactly 1 (1/g) in bf16, and x (1 +- 2^-10) rounds back to a bf16 x of <= 7 significant bits.

Plain module: no fixtures, no device.  Tensors are float64 [N, T, C] on the host.
"""
import math

import torch

BF = torch.bfloat16
LOG2E = 1.4426950408889634
A_CODE = 16.0               # amplitude of a code column: a selected score is A_CODE^2 per code column
GAP = 160.0                 # (P1)
SPREAD = 10.0               # (P1) widest selected group (family D: 9)
SEL_MAX = float(2 ** 13)    # (P2)
REL = 2.0 ** -7             # the derived bound's factor, see `bound` below
FLOOR = 2.0 ** -22          # f32 cancellation floor of fmaf(dP, scale, -round(delta scale)), per unit of (|dP| + |delta|) scale
RNE_GROWTH = 1.0 + 2.0 ** -8
D_LOW_KEYS = 128


def scale_of(c):
    return float(c) ** -0.5


def c_of(c):
    """log2-units per unit of raw score"""
    return scale_of(c) * LOG2E


def scale_is_power_of_two(c):
    return math.log2(c) % 2 == 0


def repeats_for(c):
    """how often the bit pattern of a key's identity is repeated: two codes differ in >= r columns, their scores by 2 r A_CODE^2"""
    return int(math.ceil(GAP / (2.0 * A_CODE * A_CODE * c_of(c))))


def rne(t):
    """float64 -> bf16, one rounding to nearest-even"""
    return t.float().to(BF)


# ------------------------------------------------------------------------------------------------------------------------------
# generators
# ------------------------------------------------------------------------------------------------------------------------------
def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _group_layout(t, gsize):
    """Family B: code id per key.  Group u has gsize members (u even) or gsize / 2 (u odd), so that lse2 differs between rows;
    members are dealt slot by slot, i.e. the members of one group lie about `groups` keys apart.  Keys left over get ids of their own."""
    while gsize > 1 and gsize > t:
        gsize //= 2
    small = max(1, gsize // 2)
    groups = 0
    while True:      # the largest number of groups whose members fit into t keys
        nxt = groups + 1
        need = sum(gsize if u % 2 == 0 else small for u in range(nxt))
        if need > t:
            break
        groups = nxt
    cid = torch.empty(t, dtype=torch.long)
    j = 0
    for slot in range(gsize):
        for u in range(groups):
            if u % 2 == 0 or slot % (gsize // small) == 0:      # an odd group sits out every other slot
                cid[j] = u
                j += 1
    extra = t - j
    cid[j:] = groups + torch.arange(extra)
    return cid, groups, groups + extra


def make_case(family, n, t, c, seed=0, many_to_one=False, group=2, level=9, high_first=True):
    """One attention case: dict q, k, v, do [n, t, c] float64 (all bf16 numbers), cid [t] the code id of every key, qcode [n, t] the
    code id every query selects (its keys: cid == qcode), and the recipe's parameters."""
    fam = {"A": 1, "B": 2, "C": 3, "D": 4}[family]
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * fam + 131 * c + 17 * t + n + 3 * group + 5 * level + int(many_to_one) + 2 * int(high_first))
    case = {"family": family, "n": n, "t": t, "c": c, "group": 1, "level": None}
    v, do = _ints(g, (n, t, c), -8, 8), _ints(g, (n, t, c), -8, 8)
    q, k = torch.zeros(n, t, c, dtype=torch.float64), torch.zeros(n, t, c, dtype=torch.float64)
    if family == "C":
        k = torch.randn(n, t, c, generator=g).to(BF).double()
        case.update(q=q, k=k, v=v, do=do, cid=torch.zeros(t, dtype=torch.long), qcode=torch.zeros(n, t, dtype=torch.long))
        return case
    levels = torch.zeros(t, dtype=torch.float64)
    if family == "A":
        cid, ncodes = torch.arange(t), t
        if many_to_one:     # a random half of the keys is never selected
            pool = torch.randperm(t, generator=g)[: max(1, t // 2)]
            qcode = pool[torch.randint(0, pool.numel(), (n, t), generator=g)]
        else:
            qcode = torch.stack([torch.randperm(t, generator=g) for _ in range(n)])
    elif family == "B":
        cid, groups, ncodes = _group_layout(t, group)
        qcode = torch.randint(0, groups, (n, t), generator=g)
        case["group"] = group
    elif family == "D":
        groups = t // (D_LOW_KEYS + 1)
        assert groups >= 1, "family D needs T >= %d" % (D_LOW_KEYS + 1)
        used = groups * (D_LOW_KEYS + 1)
        cid = torch.empty(t, dtype=torch.long)
        low = torch.arange(groups * D_LOW_KEYS) % groups
        lo_level = rne(torch.tensor(-float(level) / c_of(c), dtype=torch.float64)).double().item()
        if high_first:      # the level-0 keys in the first tile, the low keys behind them, the spare keys last
            cid[:groups], cid[groups:used] = torch.arange(groups), low
            levels[groups:used] = lo_level
            cid[used:] = groups + torch.arange(t - used)
            lowmask = torch.zeros(t, dtype=torch.bool)
            lowmask[groups:used] = True
        else:               # the spare keys first, the low keys, the level-0 keys in the last tile
            spare = t - used
            cid[:spare] = groups + torch.arange(spare)
            cid[spare:t - groups], cid[t - groups:] = low, torch.arange(groups)
            levels[spare:t - groups] = lo_level
            lowmask = torch.zeros(t, dtype=torch.bool)
            lowmask[spare:t - groups] = True
        v[:, lowmask] = _ints(g, (n, int(lowmask.sum()), c), 1, 8)       # positive: the low keys' ~20 % share of o is visible
        ncodes = groups + (t - used)
        qcode = torch.randint(0, groups, (n, t), generator=g)
        case["level"] = level
    else:
        raise ValueError("family %r" % (family,))
    nbits = max(1, int(math.ceil(math.log2(ncodes)))) if ncodes > 1 else 1
    r = repeats_for(c)
    ncol = nbits * r
    assert ncol + 1 <= c, "the code needs %d columns and one for the level: C = %d is too narrow" % (ncol, c)
    perm = torch.randperm(c, generator=g)
    code_cols, level_col, rest = perm[:ncol], perm[ncol], perm[ncol + 1:]
    q_cols, k_cols = rest[: rest.numel() // 2], rest[rest.numel() // 2:]
    ids = torch.arange(ncodes)
    bits = ((ids[:, None] >> torch.arange(nbits)[None, :]) & 1).double() * 2.0 - 1.0
    code = A_CODE * bits.repeat_interleave(r, dim=1)            # [ncodes, ncol]
    k[:, :, code_cols] = code[cid][None].expand(n, t, ncol)
    q[:, :, code_cols] = code[qcode]
    q[:, :, q_cols] = _ints(g, (n, t, q_cols.numel()), -8, 8)   # decoys: q lives where k is zero and the other way round
    k[:, :, k_cols] = _ints(g, (n, ncodes, k_cols.numel()), -8, 8)[:, cid]     # per code id: the keys of a group are identical
    if family == "D":
        q[:, :, level_col] = 1.0
        k[:, :, level_col] = levels[None].expand(n, t)
    case.update(q=q, k=k, v=v, do=do, cid=cid, qcode=qcode)
    return case


def pack_qkv(case):
    """the packed projection the kernels read: bf16 [n, t, 3c] (q | k | v)"""
    return torch.cat([case["q"], case["k"], case["v"]], 2).float().to(BF)


def member(case, b, rows=slice(None)):
    """[rows, t] bool: key j belongs to what query i selects"""
    return case["cid"][None, :] == case["qcode"][b, rows, None]


# ------------------------------------------------------------------------------------------------------------------------------
# the preconditions
# ------------------------------------------------------------------------------------------------------------------------------
def assert_preconditions(case, block=512):
    """(P1), (P2) and representability, on the tensors a test uses.  Returns (smallest gap, largest |s_sel c|)."""
    for name in ("q", "k", "v", "do"):
        assert torch.equal(rne(case[name]).double(), case[name]), "%s is not made of bf16 numbers" % name
    cc, t = c_of(case["c"]), case["t"]
    gap, top = float("inf"), 0.0
    for b in range(case["n"]):
        for r0 in range(0, t, block):
            rows = slice(r0, min(t, r0 + block))
            s = case["q"][b, rows] @ case["k"][b].T * cc
            m = member(case, b, rows)
            assert m.any(1).all(), "a query selects no key"
            sel_hi = s.masked_fill(~m, -float("inf")).max(1).values
            sel_lo = s.masked_fill(~m, float("inf")).min(1).values
            other = s.masked_fill(m, -float("inf")).max(1).values
            gap = min(gap, (sel_hi - other).min().item())
            top = max(top, sel_hi.abs().max().item(), sel_lo.abs().max().item())
            spread = (sel_hi - sel_lo).max().item()
            assert spread <= SPREAD, "(P1) the selected keys span %.1f log2-units, more than %.0f" % (spread, SPREAD)
    assert gap >= GAP, "(P1) a non-selected key lies %.1f log2-units below the selected one, not >= %.0f: its probability may survive" % (gap, GAP)
    assert top < SEL_MAX, "(P2) |s_sel c| = %.1f is not below 2^13: the rounding of m / lse2 may move a selected probability by more than 2^-11" % top
    return gap, top


# ------------------------------------------------------------------------------------------------------------------------------
# float64 references
# ------------------------------------------------------------------------------------------------------------------------------
def references(case, o_used=None, dense=None):
    """Closed forms in float64.  o, lse2 depend on the case alone.  The backward is a function of (qkv, o, dO, lse2): delta is
    rowsum(dO * o_used) with o_used the very o handed to the backward kernel (float64 of its bf16 values; default: the exact o).
    Per quantity X in (o, dq, dk, dv) also X_abs, the sum of |terms| the element is made of, and for dq / dk X_floor, the sum of
    P (|dP| + |delta|) scale |q or k|.  Family A never forms a T x T matrix (dense=False); the others do."""
    fam, n, t, c = case["family"], case["n"], case["t"], case["c"]
    q, k, v, do = case["q"], case["k"], case["v"], case["do"]
    scale, cc = scale_of(c), c_of(c)
    if dense is None:
        dense = fam != "A"
    r = {}
    if not dense:
        assert fam == "A"
        pi = case["qcode"]                                           # cid = arange: the code id is the key index
        idx = pi[:, :, None].expand(n, t, c)
        ksel, vsel = k.gather(1, idx), v.gather(1, idx)
        r["o"], r["o_abs"] = vsel.clone(), vsel.abs()
        r["lse2"] = (q * ksel).sum(2) * cc
        r["sel"] = r["lse2"].clone()
        o_b = r["o"] if o_used is None else o_used
        delta = (do * o_b).sum(2)
        dp = (do * vsel).sum(2)
        ds = (dp - delta) * scale                                    # P = 1
        fl = (dp.abs() + delta.abs()) * scale
        r["dq"], r["dq_abs"], r["dq_floor"] = ds[:, :, None] * ksel, ds.abs()[:, :, None] * ksel.abs(), fl[:, :, None] * ksel.abs()
        for name, src in (("dk", ds[:, :, None] * q), ("dk_abs", ds.abs()[:, :, None] * q.abs()), ("dk_floor", fl[:, :, None] * q.abs()),
                          ("dv", do), ("dv_abs", do.abs())):
            r[name] = torch.zeros(n, t, c, dtype=torch.float64).scatter_add_(1, idx, src)
        return r
    for name in ("o", "o_abs", "dq", "dq_abs", "dq_floor", "dk", "dk_abs", "dk_floor", "dv", "dv_abs"):
        r[name] = torch.empty(n, t, c, dtype=torch.float64)
    r["lse2"], r["sel"] = torch.empty(n, t, dtype=torch.float64), torch.empty(n, t, dtype=torch.float64)
    for b in range(n):
        m = member(case, b)
        z = (q[b] @ k[b].T * cc).masked_fill(~m, -float("inf"))     # non-selected keys: probability 0 by (P1)
        top = z.max(1, keepdim=True).values
        e = torch.exp2(z - top)
        den = e.sum(1, keepdim=True)
        p = e / den
        r["o"][b], r["o_abs"][b] = (e @ v[b]) / den, p @ v[b].abs()     # tie groups, uniform: e = 1, an exact integer sum divided once
        r["lse2"][b], r["sel"][b] = (top + torch.log2(den))[:, 0], top[:, 0]
        o_b = r["o"][b] if o_used is None else o_used[b]
        delta = (do[b] * o_b).sum(1, keepdim=True)
        dp = do[b] @ v[b].T
        ds = p * (dp - delta) * scale
        fl = p * (dp.abs() + delta.abs()) * scale
        r["dq"][b], r["dq_abs"][b], r["dq_floor"][b] = ds @ k[b], ds.abs() @ k[b].abs(), fl @ k[b].abs()
        r["dk"][b], r["dk_abs"][b], r["dk_floor"][b] = ds.T @ q[b], ds.abs().T @ q[b].abs(), fl.T @ q[b].abs()
        r["dv"][b], r["dv_abs"][b] = p.T @ do[b], p.T @ do[b].abs()
    return r


# ------------------------------------------------------------------------------------------------------------------------------
# the checkers
# ------------------------------------------------------------------------------------------------------------------------------
def _bits16(t):
    return t.contiguous().view(torch.int16).to(torch.int32)


def assert_bits_equal(got, want, what):
    """bf16 tensors agree in every bit (-0.0 counts as +0.0: the sign of an exactly zero sum depends on the order of its terms)"""
    assert got.dtype == BF and want.dtype == BF, "%s: dtypes %s, %s" % (what, got.dtype, want.dtype)
    assert tuple(got.shape) == tuple(want.shape), "%s: shape %s, expected %s" % (what, tuple(got.shape), tuple(want.shape))
    got, want = got + 0.0, want + 0.0
    bad = _bits16(got) != _bits16(want)
    nbad = int(bad.sum())
    if nbad:
        idx = bad.nonzero()
        first = ["(%s): got %r, want %r" % (", ".join(str(int(x)) for x in i), got[tuple(i)].item(), want[tuple(i)].item()) for i in idx[:6]]
        rows = sorted(set(int(i[1]) for i in idx))
        raise AssertionError("%s: %d of %d elements differ in bits; first %s | rows %s%s" % (
            what, nbad, bad.numel(), "; ".join(first), rows[:12], " ..." if len(rows) > 12 else ""))


def assert_within_one_ulp(got, want, what):
    """bf16 tensors at most one step of the bf16 grid apart"""
    def ordinal(x):
        b = _bits16(x + 0.0)
        return torch.where(b < 0, -(b & 0x7FFF), b)
    assert torch.isfinite(got.float()).all(), what + ": non-finite values"
    dist = (ordinal(got) - ordinal(want)).abs()
    assert int(dist.max()) <= 1, "%s: %d elements are more than one bf16 ulp off (worst %d steps)" % (what, int((dist > 1).sum()), int(dist.max()))


def assert_under_bound(got, ref, bound, what):
    """|got - ref| <= bound for every element; returns the worst err / bound (0 where both are 0)"""
    gotd = got.double()
    assert torch.isfinite(gotd).all(), what + ": non-finite values"
    err = (gotd - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = ratio.max().item() if ratio.numel() else 0.0
    if not worst <= 1.0:
        i = tuple(int(x) for x in (ratio == ratio.max()).nonzero()[0])
        raise AssertionError("%s: %d of %d elements exceed the derived bound; worst err / bound %.3g at %s (got %r, ref %r, bound %.3g)" % (
            what, int((ratio > 1.0).sum()), ratio.numel(), worst, i, gotd[i].item(), ref[i].item(), bound[i].item()))
    return worst


def bound(r, name):
    """Derived per-element bound of a quantity that is not bit-exact: 2^-7 sum|terms| + floor.
    2^-7: the probability carries 2^-9 from its rounding to bf16 and < 2^-10 from the rounding of m / lse2 (P2); dS is rounded to bf16
    once more (2^-9); the output is rounded once (2^-9 of the result <= 2^-9 sum|terms|): 3.5 * 2^-9 < 2^-7, nothing fitted.  2^-9 is
    the rounding of a value in the upper half of its binade; right above a power of two it is 2^-8, so 2^-7 is also exactly two
    worst-case roundings (o and dv, and dk of the tie groups, whose P = 1 / g is exact, have two) -- the three-rounding quantities
    (dq, dk of families C, D) are sums of tens of terms whose roundings do not all sit at the worst case: profiles/flash_attn_exact.md
    lists what was seen (<= 0.55 of the bound for those, <= 0.96 for the two-rounding ones).
    floor (dq, dk): the pair kernels form dS as P * fmaf(dP, scale, -round(delta scale)); the rounding of delta scale is 2^-24 of it,
    the f32 P another 2^-24: 2^-22 (|dP| + |delta|) scale per term covers both fourfold; (1 + 2^-8) for the rounding of the output."""
    b = REL * r[name + "_abs"]
    if name in ("dq", "dk"):
        b = b + FLOOR * RNE_GROWTH * r[name + "_floor"]
    return b


def lse2_tolerance(r):
    """lse2 = m + log2f(l) against its float64 value.  With the selected scaled score z = s_sel c: c = round(round(C^-1/2) round(log2 e))
    is three roundings of 2^-24 relative, m = round(s c) a fourth -- whose residual the exponent s c - m keeps and log2f(l) hands back, up
    to the errors of v_exp_f32 and log2f near 1 (<= 2 ulps of 1 each, absolute) -- and the final sum rounds a fifth time: 5 * 2^-24 |z| +
    4 * 2^-23, held as 8 * 2^-24 max(|z|, |lse2|, 1) + 2^-21."""
    mag = torch.maximum(torch.maximum(r["sel"].abs(), r["lse2"].abs()), torch.ones_like(r["lse2"]))
    return 8.0 * 2.0 ** -24 * mag + 2.0 ** -21


def check_case(case, got, o_used=None):
    """Every element of every output of one case against its family's rule.  got: o, dq, dk, dv bf16 [n, t, c], lse2 f32 [n, t] (host
    tensors); o_used: the o the backward was given (default got["o"]).  Returns {quantity: worst err / bound} for what is toleranced."""
    fam, c, t = case["family"], case["c"], case["t"]
    tag = "family %s N=%d T=%d C=%d" % (fam, case["n"], t, c)
    r = references(case, (got["o"] if o_used is None else o_used).double())
    margins = {}
    margins["lse2"] = assert_under_bound(got["lse2"], r["lse2"], lse2_tolerance(r), tag + " lse2")
    if fam in ("A", "B") or (fam == "C" and t & (t - 1) == 0):
        assert_bits_equal(got["o"], rne(r["o"]), tag + " o")
    elif fam == "C":      # 1 / l, then O * (1 / l), then the store: the product of two rounded factors is rounded again
        assert_within_one_ulp(got["o"], rne(r["o"]), tag + " o")
    else:
        margins["o"] = assert_under_bound(got["o"], r["o"], bound(r, "o"), tag + " o")
    if fam in ("A", "B"):
        assert_bits_equal(got["dv"], rne(r["dv"]), tag + " dv")
    else:
        margins["dv"] = assert_under_bound(got["dv"], r["dv"], bound(r, "dv"), tag + " dv")
    zero = torch.zeros_like(got["dq"])
    # dq: zero in exact arithmetic for A, B.  With scale a power of two every dS of A is fmaf(x, scale, -x scale) = 0; of a group of two,
    # the two dS are exact negatives on identical k.  Larger groups: the bf16 roundings of g different dS no longer cancel.
    if fam == "A" and scale_is_power_of_two(c):
        assert_bits_equal(got["dq"], zero, tag + " dq")
        assert_bits_equal(got["dk"], zero, tag + " dk")
    elif fam == "B" and scale_is_power_of_two(c) and case["group"] <= 2:
        assert_bits_equal(got["dq"], zero, tag + " dq")
        margins["dk"] = assert_under_bound(got["dk"], r["dk"], bound(r, "dk"), tag + " dk")
    else:
        margins["dq"] = assert_under_bound(got["dq"], r["dq"], bound(r, "dq"), tag + " dq")
        if fam == "C":
            assert_bits_equal(got["dk"], zero, tag + " dk")
        else:
            margins["dk"] = assert_under_bound(got["dk"], r["dk"], bound(r, "dk"), tag + " dk")
    return margins


# ------------------------------------------------------------------------------------------------------------------------------
# the shapes of the GPU test (tests/test_flash_attn_bf16_exact_gpu.py); the host model is held to the same list
# ------------------------------------------------------------------------------------------------------------------------------
CS = (64, 128, 256, 512)       # 64-key LDS stages | wave-pair kernels | 4 forward / dQ slices, 8 dK-dV slices
TS = (1, 31, 32, 33, 45, 64, 65, 96, 97, 127, 128, 129, 160, 257, 300)     # 1 .. 10 key tiles, ragged last tile, 1 .. 3 query blocks
NS = (1, 3, 8)                 # 8: the XCD-grouped block order of the pair kernels
D_TS = (129, 160, 257, 300)
BIG = ((4100, 64), (4100, 256))


def cases_for(c, t):
    """the cases of one (C, T): selector with a permutation and with a many-to-one map, tie groups, uniform, and -- where 129 keys
    fit -- two levels at -9 / -6 with the level-0 key in the first / last tile.  N and the group size rotate over the grid."""
    i = CS.index(c) + (TS.index(t) if t in TS else 0)
    if (t, c) in BIG:
        return [dict(family="A", n=1, t=t, c=c, many_to_one=(c == 256))]
    out = [dict(family="A", n=NS[i % 3], t=t, c=c),
           dict(family="A", n=NS[(i + 1) % 3], t=t, c=c, many_to_one=True),
           dict(family="B", n=NS[(i + 2) % 3], t=t, c=c, group=(2, 4, 8)[i % 3]),
           dict(family="C", n=NS[i % 3], t=t, c=c)]
    if t in D_TS:
        out += [dict(family="D", n=NS[(i + k) % 3], t=t, c=c, level=level, high_first=first)
                for k, (level, first) in enumerate(((9, True), (9, False), (6, True), (6, False)))]
    return out


def grid():
    return [(c, t) for c in CS for t in TS] + [(c, t) for t, c in BIG]
