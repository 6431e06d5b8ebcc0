"""Attention inputs with closed-form answers for the bf16 flash-attention kernels and (section "f32 routes" below) the f32 attention
routes: generators, float64 references, the preconditions, the checkers.

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

f32 routes
----------
The same case tensors, packed as f32 (`pack_qkv(case, torch.float32)`), pin the four f32 routes of ops/attention.py: the fused kernels
(csrc/flash_attn_f32.hip), the GEMM route with the separate and with the folded softmax, and the recompute route.  Every product of
q, k, v, dO is a sum of small integers (family D: of multiples of 2^-3 below 2^15), exact in f32 in any order.
  (P1) as above, with a simpler argument: the f32 kernels take the true running / row maximum, which does not lag, and 2^-160 is below
       f32's smallest subnormal 2^-149 -- a non-selected probability is 0 whatever the flush mode.
  (P2-f32) |z| < 2^13, z = s_sel c: ulp(|z|) <= 2^-11.  The fused backward forms p = exp2f(s sc - lse2), which hipcc contracts to an
       fma (it does, on gfx950); lse2 = round(s sc) + log2 g then leaves the rounding residual of s sc in the exponent and a selected
       p is 2^delta / g, |delta| <= ulp(|z|) / 2: relative error ln 2 ulp(|z|) / 2 <= 1.7e-4.  A_CODE stays 16: the largest |z| used is
       ~1200 (C = 64, T = 4100), ulp 2^-13; the gap is what must hold.
  (folded) slack_i = (1.000001 |q_i| max_j |k_j| - s_sel,i) c, norms over the row's own image (`folded_slack`): E_sel = 2^-slack.
       "bound holds": slack <= 90 on every row, l >= 2^-90, a normal number far above 1e-30 ~ 2^-99.7; "bound underflows": slack >= 110
       on some row, l <= T 2^-110 < 1e-30 there and the flag must rise.  The decoy amplitude (`make_case(decoy=...)`, 1/4 and 4) moves
       |q|, |k| and no score; `folded_side` decides from the tensors alone.
Bit-exact, from the code (eps = 2^-24):
  fused forward: s sc is rounded BEFORE the maximum is taken off (mul, then sub: no contraction across the select), so the selected
    exponent is exactly 0, p = 1, l = g, acc an integer sum, 1 / l an IEEE division: o is exact for A, B (g = 2^n) and C at T = 2^n; C at
    other T: o = fl(fl(1 / T) S), S an integer, against fl(S / T): three half-ulp errors, the first scaled by mant(o) < 2 -- strictly
    less than 2 ulps between two grid points, i.e. at most one step.
  fused backward, A: dP_sel and delta = rowdot(dO, o) are the same exact integer, dS = p * 0: dq = dk = 0 whatever p is (the subtraction
    comes before the scale: no "scale is a power of two" condition).  Family C: q = 0, dk = 0.
  fused backward, B with g <= 2: NOT bit-exact.  dS_1 = -dS_2 = p (dP_1 - dP_2) / 2 exactly and k_1 = k_2, but the MFMA chain computes
    fma(k, -dS, fl(k dS)) = fl(k dS) - k dS: the rounding residual of the first product, non-zero on decoy columns (k = 3, 5, ...) once
    p = 2^delta has a full mantissa.  dq of B is toleranced on every route (0 <= bound where the products happen to be exact).
  separate softmax / recompute: exp((s - max) scale) is exp(0) = 1 for the selected keys, P = 1 / g: o, dv exact for A, B, C at T = 2^n;
    dP - delta is an exact 0 for A (delta an integer seeds the accumulator; the row pass forms sum_j P dP = dP): dq = dk = 0.
  folded softmax: E = exp2((s - bound) a2) is not 1, o = fl(fl(E v) / E) is not v: everything is toleranced, also dq / dk of A (delta is
    no integer any more).  After a fallback the result IS the separate route's.
Bounds (`f32_rules`, `bound_f32`): per element (eps_p + k_sum eps) sum|terms|, for o once more with k_l, plus k_x eps X for dq / dk.
  kmax = the largest number of non-zero terms in any sum of the case (keys per query, queries per key): adding an exact 0 does not round.
  k_sum = kmax + 4: one rounding per non-zero fma of the chain, dS (2), the final scale or rinv (1), the store (0) -- one spare.
  k_l = kmax + nt + 2: the row sum's additions, on the fused route one rescale per 32-key tile (nt = ceil(T / 32); alpha is 1 or 0 for a
    selecting softmax, a real factor in D) and the two lane exchanges; 1 / l.
  eps_p, the relative error of a probability as the products see it, per query row (zmag_i = max(|z_i|, |lse2_i|, 1)):
    fused: ln 2 u ulp(zmag) + 24 eps, u by family -- only the roundings that occur together, for the contracted exponent
      fma(s, sc, -lse2) and for the plain fl(s sc) - lse2 alike (e_x: the rounding error of fl(x sc), <= ulp / 2):
        A  u = 1/2.  l = 1, log2f(1) = 0, lse2 = m = fl(s sc).  Contracted: the exponent is s sc - m = -e_m.  Plain: fl(s sc) - m = 0.
        B  u = 1.    lse2 = fl(m + n), l = g = 2^n: the sum's rounding (1/2) on top of A's.
        C  u = 1.    z = 0, m = 0, lse2 = log2f(T), within 1 ulp of log2 T (OCML's documented accuracy); nothing else rounds.
        D  u = 3/2.  The forward's low-key exponents fl(s_low sc) - m carry e_low - e_m and make up a share w <= 1 of l.  Contracted,
                     either level: -(1 - w) e_m - w e_low (1/2) and the sum (1/2).  Plain, low key: e_low (1/2), (1 - w) e_m and
                     w e_low' (1/2 together), the sum (1/2); plain, level-0 key: w (e_low' - e_m) and the sum, also <= 3/2.
      24 eps: the rounding of the exponent itself (|x| < 32: 16 eps of x, 11 of p), exp2f (1 ulp: 2), log2f of l <= 8 (3), spare.
      D only, (kmax + nt + 20) eps more: l's own additions and rescales (its terms are no integers there), and c = fl(fl(C^-1/2)
      fl(log2 e)) against the float64 c on the 9 log2-units between the levels (3 eps * 9 * ln 2 < 20 eps).  A, B, C: l is an exact
      integer and c's error cancels between s sc and lse2.
    separate, recompute: (kmax + 40) eps: (s - max) is exact, times scale (1), __expf = exp2(x log2 e) (1, and |x| <= SPREAD: 30 eps of
      argument error), the sum (kmax), 1 / sum, the product.
    folded: (kmax + 8) eps for A, B, C -- the members of a tie group have identical k rows, hence identical E, and P = E / (g E) does
      not see E's error; family D's levels differ in one product of the chain s - bound, which is seeded with -bound and rounds at
      magnitude |bound| in each of up to C steps: 2 ln 2 (C ulp(|bound|) / 2 c + 2 eps (slack + SPREAD)) more.
  k_x eps X, X = sum P scale (dpa + sum_j P dpa) |k or q|, dpa_ij = sum_c |dO_ic| |v_jc|: the cancellation floor of dP - delta, at the
    magnitude the two sums run at.  delta = rowdot(dO, o): 4 ceil(C / 256) products and additions per lane, 6 exchange steps, the
    subtraction: k_delta = 4 ceil(C / 256) + 8 (fused); the GEMM routes seed the accumulator with -delta and add C products: C + k_delta;
    the row pass forms delta as sum_j P dP from the rounded P: 2 kmax + 60 (kmax terms, eps_p / eps, the block reduction).
  lse2 (fused): 6 eps mag for c = fl(fl(C^-1/2) fl(log2 e)) (3), m (1), the final sum (1) and a spare, + ulp(zmag) for D's low keys
    + k_l eps / ln 2 + 2^-19 for log2f at log2 l < 16.
Nothing here was fitted to a device result; profiles/attn_f32_exact.md lists the worst err / bound seen.
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


def make_case(family, n, t, c, seed=0, many_to_one=False, group=2, level=9, high_first=True, decoy=None):
    """One attention case: dict q, k, v, do [n, t, c] float64 (all bf16 numbers), cid [t] the code id of every key, qcode [n, t] the
    code id every query selects (its keys: cid == qcode), and the recipe's parameters.
    decoy (f32 cases; None: the recipe as it is, the seed formula does not see it): amplitude of the integer decoys on q_cols / k_cols,
    one number or one per image.  The decoys sit on disjoint columns and change no score; they lengthen |q| and |k|, i.e. the
    Cauchy-Schwarz row bound of the folded softmax (`folded_slack`).  Powers of two: the decoys stay exact in f32 (and bf16)."""
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
    if decoy is not None:
        amp = torch.as_tensor(decoy, dtype=torch.float64).reshape(-1, 1, 1).expand(n, 1, 1)
        q[:, :, q_cols] = q[:, :, q_cols] * amp
        k[:, :, k_cols] = k[:, :, k_cols] * amp
        case["decoy"] = decoy
    case.update(q=q, k=k, v=v, do=do, cid=cid, qcode=qcode)
    return case


def pack_qkv(case, dtype=BF):
    """the packed projection the kernels read: [n, t, 3c] (q | k | v) in bf16 or f32"""
    return torch.cat([case["q"], case["k"], case["v"]], 2).float().to(dtype)


def member(case, b, rows=slice(None)):
    """[rows, t] bool: key j belongs to what query i selects"""
    return case["cid"][None, :] == case["qcode"][b, rows, None]


# ------------------------------------------------------------------------------------------------------------------------------
# the preconditions
# ------------------------------------------------------------------------------------------------------------------------------
def assert_preconditions(case, block=512, dtype=BF):
    """(P1), (P2) and representability, on the tensors a test uses.  Returns (smallest gap, largest |s_sel c|)."""
    for name in ("q", "k", "v", "do"):
        assert torch.equal(case[name].float().to(dtype).double(), case[name]), "%s is not made of %s numbers" % (name, "bf16" if dtype == BF else dtype)
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
        x = 2.0 * (do.abs() * vsel.abs()).sum(2) * scale            # the f32 rules' X, see below (P = 1: dpa + sum_j P dpa = 2 dpa)
        r["dq_x"] = x[:, :, None] * ksel.abs()
        for name, src in (("dk", ds[:, :, None] * q), ("dk_abs", ds.abs()[:, :, None] * q.abs()), ("dk_floor", fl[:, :, None] * q.abs()),
                          ("dv", do), ("dv_abs", do.abs()), ("dk_x", x[:, :, None] * q.abs())):
            r[name] = torch.zeros(n, t, c, dtype=torch.float64).scatter_add_(1, idx, src)
        r["k_row"] = torch.ones(n, t, dtype=torch.float64)
        r["k_col"] = torch.zeros(n, t, dtype=torch.float64).scatter_add_(1, pi, torch.ones(n, t, dtype=torch.float64))
        return r
    for name in ("o", "o_abs", "dq", "dq_abs", "dq_floor", "dk", "dk_abs", "dk_floor", "dv", "dv_abs", "dq_x", "dk_x"):
        r[name] = torch.empty(n, t, c, dtype=torch.float64)
    for name in ("lse2", "sel", "k_row", "k_col"):
        r[name] = torch.empty(n, t, dtype=torch.float64)
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
        # the f32 rules: X = sum over the terms of P scale (dpa + sum_j P dpa) |k or q|, dpa_ij = sum_c |dO_ic| |v_jc| the magnitude at
        # which the sums dP_ij and delta_i run; k_row / k_col: how many keys a query gives weight to / how many queries weigh a key
        dpa = do[b].abs() @ v[b].abs().T
        x = p * (dpa + (p * dpa).sum(1, keepdim=True)) * scale
        r["dq_x"][b], r["dk_x"][b] = x @ k[b].abs(), x.T @ q[b].abs()
        r["k_row"][b], r["k_col"][b] = m.sum(1).double(), m.sum(0).double()
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


# ==============================================================================================================================
# f32: the same cases for the four f32 attention routes of ops/attention.py (module docstring: "f32 routes")
# ==============================================================================================================================
F32 = torch.float32
EPS = 2.0 ** -24                    # one f32 rounding to nearest, relative to the result
LN2 = 0.6931471805599453
BOUND_GROW = 1.000001               # attn_bound_kernel's factor on max_j |k_j|
SLACK_HOLDS, SLACK_UNDERFLOWS = 90.0, 110.0
DECOY_HOLDS, DECOY_UNDERFLOWS = 0.25, 4.0
ROUTES = ("fused", "separate", "separate_unfused", "recompute", "folded")


def ulp32(x):
    """the f32 grid step at |x| (normal numbers)"""
    return 2.0 ** (math.floor(math.log2(abs(x))) - 23)


def folded_decoy(n, underflows):
    """Decoy amplitudes of a folded-softmax case.  Holds: 1/4 on every image.  Underflows: 4 on every image BUT the first (one image:
    on that one), so that a row bound taken from image 0 for every image would hold everywhere and leave the flag down."""
    if not underflows:
        return DECOY_HOLDS
    return DECOY_UNDERFLOWS if n == 1 else (DECOY_HOLDS,) + (DECOY_UNDERFLOWS,) * (n - 1)


def folded_slack(case):
    """[n, t] float64: slack_i = (1.000001 |q_i| max_j |k_j| - s_sel,i) c in log2-units, norms over the row's own image: how far the
    folded route's Cauchy-Schwarz bound lies above the row's selected score.  E_sel = 2^-slack and l >= E_sel.  Also the bounds
    themselves (raw score units).  The kernel's norms carry a few f32 roundings: ~2^-21 |bound| c < 0.01 log2-units here."""
    cc = c_of(case["c"])
    slack, bnd = torch.empty(case["n"], case["t"], dtype=torch.float64), torch.empty(case["n"], case["t"], dtype=torch.float64)
    for b in range(case["n"]):
        q, k = case["q"][b], case["k"][b]
        bnd[b] = q.norm(dim=1) * (k.norm(dim=1).max() * BOUND_GROW)
        sel = (q @ k.T).masked_fill(~member(case, b), -float("inf")).max(1).values
        slack[b] = (bnd[b] - sel) * cc
    return slack, bnd


def assert_folded_precondition(case, underflows):
    """holds: slack <= 90 on every row (l >= 2^-90, a normal number far above 1e-30 ~ 2^-99.7: the flag stays down);
    underflows: slack >= 110 on at least one row (there every E <= 2^-110, l <= T 2^-110 < 1e-30: the flag must rise).
    Conditions on the case's own tensors, not measurements.  Returns (smallest, largest) slack."""
    slack, _ = folded_slack(case)
    lo, hi = slack.min().item(), slack.max().item()
    assert lo >= -1e-9, "the row bound lies below a selected score (slack %.3g): Cauchy-Schwarz broken" % lo
    if underflows:
        assert hi >= SLACK_UNDERFLOWS, "no row's bound lies >= %.0f log2-units above its selected score (largest slack %.1f)" % (SLACK_UNDERFLOWS, hi)
        assert math.log2(case["t"]) - hi < -100.0      # T 2^-slack < 1e-30
    else:
        assert hi <= SLACK_HOLDS, "a row's bound lies %.1f log2-units above its selected score, more than %.0f" % (hi, SLACK_HOLDS)
    return lo, hi


def folded_side(case):
    """"holds" / "underflows" / None (in between: no folded-route case) by the two conditions above, from the case's tensors alone.
    Families A and B land where their decoy amplitude puts them (tests/test_attn_f32_exact_inputs.py shows it for every (C, T) used);
    family C (q = 0: bound 0) always holds; family D's low keys carry the level 9 / c or 6 / c on one column, which alone lengthens
    max_j |k_j|.  With the 1/4 decoys a level-6 D case holds at C = 32 and, but for one T, at 48, and lies in between at C = 64 (no
    "holds" run); at level 9, and at C = 256 at either level, it underflows already.  With the 4 decoys every D case underflows, so
    each D recipe does run as a fallback case at every T it exists for."""
    hi = folded_slack(case)[0].max().item()
    if hi <= SLACK_HOLDS:
        return "holds"
    if hi >= SLACK_UNDERFLOWS and math.log2(case["t"]) - hi < -100.0:
        return "underflows"
    return None


def _bits32(t):
    return (t.contiguous() + 0.0).view(torch.int32)


def assert_bits_equal_f32(got, want, what):
    """f32 tensors agree in every bit (int32 view; -0.0 counts as +0.0)"""
    assert got.dtype == F32 and want.dtype == F32, "%s: dtypes %s, %s" % (what, got.dtype, want.dtype)
    assert tuple(got.shape) == tuple(want.shape), "%s: shape %s, expected %s" % (what, tuple(got.shape), tuple(want.shape))
    bad = _bits32(got) != _bits32(want)
    nbad = int(bad.sum())
    if nbad:
        idx = bad.nonzero()
        first = ["(%s): got %r, want %r" % (", ".join(str(int(x)) for x in i), got[tuple(i)].item(), want[tuple(i)].item()) for i in idx[:6]]
        rows = sorted(set(int(i[1]) for i in idx)) if idx.shape[1] > 1 else []
        raise AssertionError("%s: %d of %d elements differ in bits; first %s | rows %s%s" % (
            what, nbad, bad.numel(), "; ".join(first), rows[:12], " ..." if len(rows) > 12 else ""))


def assert_within_one_ulp_f32(got, want, what):
    """f32 tensors at most one step of the f32 grid apart"""
    def ordinal(x):
        b = _bits32(x).to(torch.int64)
        return torch.where(b < 0, -(b & 0x7FFFFFFF), b)
    assert torch.isfinite(got).all(), what + ": non-finite values"
    dist = (ordinal(got) - ordinal(want)).abs()
    assert int(dist.max()) <= 1, "%s: %d elements are more than one f32 ulp off (worst %d steps)" % (what, int((dist > 1).sum()), int(dist.max()))


FUSED_ULPS = {"A": 0.5, "B": 1.0, "C": 1.0, "D": 1.5}      # ulps of zmag in a fused-route exponent, module docstring "eps_p, fused"


def ulp32_of(x):
    """the f32 grid step at every element of a float64 tensor of magnitudes >= 1, a hair (2^-20) up: the kernel's own z differs from
    the float64 one by the rounding of c and may lie in the next binade"""
    return torch.exp2(torch.floor(torch.log2(x * (1.0 + 2.0 ** -20))) - 23.0)


def f32_rules(case, r, route):
    """The factors of the f32 bounds of one (case, route), every one a count of roundings (module docstring, "f32 routes"):
    eps_p [n, t]  relative error of a probability of query row i as the products see it;  k_sum  roundings of a sum of products and its
    tail;  k_x  roundings at the magnitude X of the difference dP - delta;  k_l  roundings of the forward's row sum;  zmag [n, t]."""
    fam, t, c = case["family"], case["t"], case["c"]
    kmax = max(r["k_row"].max().item(), r["k_col"].max().item())
    zmag = torch.maximum(torch.maximum(r["sel"].abs(), r["lse2"].abs()), torch.ones_like(r["lse2"]))
    nt = -(-t // 32) if route == "fused" else 0
    k_delta = 4 * (-(-c // 256)) + 8
    if route == "fused":
        eps_p = LN2 * FUSED_ULPS[fam] * ulp32_of(zmag) + (24 + (kmax + nt + 20 if fam == "D" else 0)) * EPS
        k_x = k_delta
    elif route == "folded":
        e = (kmax + 8) * EPS
        if fam == "D":
            slack, bnd = folded_slack(case)
            e += 2.0 * LN2 * (c * 0.5 * ulp32(bnd.max().item()) * c_of(c) + 2.0 * EPS * (slack.max().item() + SPREAD))
        eps_p, k_x = torch.full_like(zmag, e), c + k_delta
    elif route == "separate_unfused":
        eps_p, k_x = torch.full_like(zmag, (kmax + 40) * EPS), 2 * kmax + 60
    else:
        eps_p, k_x = torch.full_like(zmag, (kmax + 40) * EPS), c + k_delta
    return {"eps_p": eps_p, "k_sum": kmax + 4, "k_x": k_x, "k_l": kmax + nt + 2, "zmag": zmag}


def bound_f32(r, name, rules):
    """The per-element bound of one toleranced quantity (module docstring, "Bounds").  o and dq are sums over the keys of ONE query:
    that row's eps_p.  dv and dk are sums over the queries that weigh a key: the largest eps_p of the image's rows (every row of an
    image carries nearly the same |z|; the step of ulp() is what can differ)."""
    e = rules["eps_p"][:, :, None] if name in ("o", "dq") else rules["eps_p"].max(1).values[:, None, None]
    b = (e + rules["k_sum"] * EPS) * r[name + "_abs"]
    if name == "o":
        b = b + (e + rules["k_l"] * EPS) * r["o_abs"]
    if name in ("dq", "dk"):
        b = b + rules["k_x"] * EPS * r[name + "_x"]
    return b


def lse2_tolerance_f32(case, r, rules):
    """lse2 = m + log2f(l) of the fused forward against float64, per row (module docstring, "lse2 (fused)")"""
    low = ulp32_of(rules["zmag"]) if case["family"] == "D" else 0.0
    return 6.0 * EPS * rules["zmag"] + low + rules["k_l"] * EPS / LN2 + 2.0 ** -19


def check_case_f32(case, got, route, o_used=None):
    """Every element of every output of one f32 case against its family's rule on `route` (one of ROUTES; a folded forward whose
    fallback ran is "separate").  got: o, dq, dk, dv f32 [n, t, c] host tensors, and lse2 f32 [n, t] on the fused route; o_used: the o
    the backward's delta was formed from (default got["o"]; "separate_unfused" forms sum_j P dP from P itself: the exact o).
    Returns {quantity: worst err / bound} for what is toleranced."""
    fam, c, t = case["family"], case["c"], case["t"]
    assert route in ROUTES
    tag = "f32 %s family %s N=%d T=%d C=%d" % (route, fam, case["n"], t, c)
    if route == "separate_unfused":
        r = references(case, None)
    else:
        r = references(case, (got["o"] if o_used is None else o_used).double())
    rules = f32_rules(case, r, route)
    margins = {}
    if route == "fused":
        margins["lse2"] = assert_under_bound(got["lse2"], r["lse2"], lse2_tolerance_f32(case, r, rules), tag + " lse2")
    exact_p = fam in ("A", "B") or (fam == "C" and t & (t - 1) == 0)        # every probability is 1 / 2^n
    if route != "folded" and exact_p:
        assert_bits_equal_f32(got["o"], r["o"].float(), tag + " o")
    elif route == "fused" and fam == "C":
        assert_within_one_ulp_f32(got["o"], r["o"].float(), tag + " o")
    else:
        margins["o"] = assert_under_bound(got["o"], r["o"], bound_f32(r, "o", rules), tag + " o")
    if route not in ("fused", "folded") and exact_p:
        assert_bits_equal_f32(got["dv"], r["dv"].float(), tag + " dv")
    else:
        margins["dv"] = assert_under_bound(got["dv"], r["dv"], bound_f32(r, "dv", rules), tag + " dv")
    zero = torch.zeros_like(got["dq"])
    if fam == "A" and route != "folded":
        assert_bits_equal_f32(got["dq"], zero, tag + " dq")
        assert_bits_equal_f32(got["dk"], zero, tag + " dk")
    else:
        margins["dq"] = assert_under_bound(got["dq"], r["dq"], bound_f32(r, "dq", rules), tag + " dq")
        if fam == "C":
            assert_bits_equal_f32(got["dk"], zero, tag + " dk")
        else:
            margins["dk"] = assert_under_bound(got["dk"], r["dk"], bound_f32(r, "dk", rules), tag + " dk")
    return margins


# ------------------------------------------------------------------------------------------------------------------------------
# the shapes of the f32 GPU tests; the host models are held to the same lists
# ------------------------------------------------------------------------------------------------------------------------------
F32_TS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 96, 97, 129, 160, 257, 300)    # a wave's 16 rows, a tile's 32 keys and a
#                                                                      block's 64 rows from both sides, one to five blocks (fused route)
GEMM_CS = (32, 48, 64, 256)
GEMM_TS_EDGES = (1, 45, 127, 128, 129, 180, 257, 300)     # the 128-wide GEMM tiles from both sides
GEMM_TS = tuple(sorted(set(GEMM_TS_EDGES + (4, 44, 124, 132, 256, 260))))     # ... and the multiples of 4 beside them: the GEMM routes
#                                                     take T % 4 == 0 only (float4 rows of P) and must REFUSE the others, not fall back
SPLIT_TT = dict(n=57, t=300, c=64)      # ceil(300 / 128)^2 * 57 = 513 >= 512 blocks, K = 64: the T x T products run on the bf16-split kernels


def cases_for_f32(c, t):
    """as `cases_for`, for the fused f32 kernels: the rotation runs over F32_TS"""
    i = CS.index(c) + (F32_TS.index(t) if t in F32_TS else 0)
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


def grid_f32():
    return [(c, t) for c in CS for t in F32_TS] + [(c, t) for t, c in BIG]


def gemm_cases_for(c, t):
    """the cases of one (C, T) on the GEMM routes: A (permutation, many-to-one) and B everywhere, C and D where 129 keys fit.  Cases
    `make_case` refuses (C too narrow for the code) are left out; the gap is not weakened for them."""
    i = GEMM_CS.index(c) + GEMM_TS.index(t)
    out = [dict(family="A", n=NS[i % 3], t=t, c=c),
           dict(family="A", n=NS[(i + 1) % 3], t=t, c=c, many_to_one=True),
           dict(family="B", n=NS[(i + 2) % 3], t=t, c=c, group=(2, 4, 8)[i % 3])]
    if t >= D_LOW_KEYS + 1:
        out += [dict(family="C", n=NS[i % 3], t=t, c=c),
                dict(family="D", n=NS[(i + 1) % 3], t=t, c=c, level=9, high_first=bool(i % 2)),
                dict(family="D", n=NS[(i + 2) % 3], t=t, c=c, level=6, high_first=not i % 2)]
    kept = []
    for kw in out:
        try:
            make_case(**kw)
        except AssertionError as e:
            assert "too narrow" in str(e)
            continue
        kept.append(kw)
    return kept


def folded_variants(kw):
    """[(case, side)] of one recipe for the folded route: at most one case per side, with the decoy amplitudes of `folded_decoy` and
    the side the host arithmetic shows (`folded_side`).  A and B give both sides; C holds; D lands where its level column puts it."""
    out = []
    for underflows in (False, True):
        case = make_case(decoy=folded_decoy(kw["n"], underflows), **kw)
        side = folded_side(case)
        if kw["family"] in ("A", "B"):
            assert side == ("underflows" if underflows else "holds"), (kw, side)
        if side is not None and not any(side == s for _, s in out):
            out.append((case, side))
    return out


RECOMPUTE_N = 5        # budgets of 2 and of 1 image: forward groups 2 + 2 + 1 and five of 1, backward groups of 1 (the halved group)


def recompute_cases_for(c, t):
    """every family of `gemm_cases_for`, five images each"""
    return [dict(kw, n=RECOMPUTE_N) for kw in gemm_cases_for(c, t)]


def gemm_grid():
    return [(c, t) for c in GEMM_CS for t in GEMM_TS]
