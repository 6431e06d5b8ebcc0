"""float32_matmul_precision on exactly summable inputs: what the bf16-split kernel (gemm_f32_split.hip) must give, bit for bit, at
each level.  Built on tests/gemm_exact_inputs.py (its split recipes, its restatement of the three-way split), which stays as it is.

level                planes kept      products kept (A plane, B plane), smallest first
0 highest (default)  hi, mid, lo      lo hi, hi lo, mid mid, mid hi, hi mid, hi hi
1 high               hi, mid          mid hi, hi mid, hi hi
2 medium             hi               hi hi

On the split recipes every plane is a whole number of units and the sum of |terms| of the kept products stays below 2^24 units
(`assert_level_summable`), so no f32 addition rounds in any order and the kernel's output must EQUAL `level_reference`.

Plain module: no fixtures, no device.  Everything is float64 on the host."""
import torch

import gemm_exact_inputs as G

HI, MID, LO = 0, 1, 2
NAMES = ("highest", "high", "medium")      # index = level of odvae_gemm_select_precision
KEPT = {0: ((LO, HI), (HI, LO), (MID, MID), (MID, HI), (HI, MID), (HI, HI)),
        1: ((MID, HI), (HI, MID), (HI, HI)),
        2: ((HI, HI),)}
LEVELS = (0, 1, 2)


def planes(c):
    """((a_hi, a_mid, a_lo), (b_hi, b_mid, b_lo)), float64"""
    return G.split3(c["a"]), G.split3(c["b"])


def sum_of_pairs(pa, pb, pairs):
    out = 0.0
    for p, q in pairs:
        out = out + torch.matmul(pa[p], pb[q])
    return out


def level_reference(c, level):
    """float64 sum, over the kept (p, q), of a_p b_q: [batch][M][N].  (alpha and the row vectors of an epilogue are the caller's.)"""
    pa, pb = planes(c)
    return sum_of_pairs(pa, pb, KEPT[level])


def level_references(c):
    """[level_reference(c, 0), (c, 1), (c, 2)] from six products instead of ten: each level adds its own pairs to the next one's sum
    (float64 sums of whole units below 2^53: exact in any order, so these EQUAL level_reference)"""
    pa, pb = planes(c)
    r2 = sum_of_pairs(pa, pb, KEPT[2])
    r1 = r2 + sum_of_pairs(pa, pb, KEPT[1][:2])
    r0 = r1 + sum_of_pairs(pa, pb, KEPT[0][:3])
    return [r0, r1, r2]


def assert_level_summable(c, level):
    """Every plane is made of whole multiples of its operand's unit (G.assert_exactly_summable has asserted that), and the kept
    products' sum of |terms| stays below 2^24 units: the f32 accumulation of this level is exact in any order."""
    pa, pb = planes(c)
    worst = sum_of_pairs([p.abs() for p in pa], [p.abs() for p in pb], KEPT[level]).max().item() / (c["units"]["a"] * c["units"]["b"])
    assert worst < G.LIMIT, "level %d: the kept products sum to %.4g units, not below 2^24" % (level, worst)
    ref = level_reference(c, level)
    assert torch.equal(ref.float().double(), ref), "level %d: the reference is not made of f32 numbers" % level
    return worst


def accepts(got, c, level):
    """The acceptance rule: `got` (f32 [batch][M][N]) equals the level reference in every bit (-0.0 counts as +0.0: a sum)."""
    want = level_reference(c, level).float()
    if got.dtype != want.dtype or tuple(got.shape) != tuple(want.shape):
        return False
    return torch.equal((got + 0.0).view(torch.int32), (want + 0.0).view(torch.int32))


def truncated_mid(t):
    """the mid plane a loader would make if it chopped x - hi to bf16 (toward zero) where split8 rounds to nearest even"""
    x = t.float()
    r = x - x.to(G.BF).float()
    return (r.view(torch.int32) & -65536).view(torch.float32).double()


def rownorm_level_reference(c, level):
    """(A B at this level) / l, l = the row sums of the unsplit A (a power of two on G.make_rownorm_case)"""
    return level_reference(c, level) / c["a"].sum(2)[:, :, None]


def smb_level_reference(c, level):
    """G.smb_reference with the level's product in place of the float64 one"""
    s = level_reference(c, level) - c["rowdot"][:, :, None]
    f = c["alpha"] * (c["rowmul"][:, :, None] if c["rowmul"] is not None else 1.0)
    return s * f * c["p"]


def rel_err_bounds():
    """b_L of e_L <= e_f32 + b_L, e = max |C - C64| / sum_k |a_k| |b_k|, from the planes alone.  Round to nearest even: |mid| <= 2^-8 |x|
    (half an ulp of an 8-bit significand, relative to x), |lo| <= 2^-16 |x|, |hi| <= (1 + 2^-8) |x|.
      highest drops mid lo, lo mid, lo lo:   2 * 2^-24 + 2^-32                              < 2^-22
      high also drops mid mid, lo hi, hi lo: 2^-16 + 2 * 2^-16 (1 + 2^-8) = 3 * 2^-16 + 2^-23; with the above < 3 * 2^-16 + 2^-21
      medium also drops mid hi, hi mid:      2 * 2^-8 (1 + 2^-8) = 2^-7 + 2^-15;             with the above < 2^-7 + 2^-13
    The bounds returned are these sums rounded up to two terms: 0.75 and 0.52 of the round figures 2^-14 and 2^-6."""
    drop0 = 2.0 * 2.0 ** -24 + 2.0 ** -32
    drop1 = drop0 + 3.0 * 2.0 ** -16 + 2.0 ** -23
    drop2 = drop1 + 2.0 ** -7 + 2.0 ** -15
    b = {0: 2.0 ** -22, 1: 3.0 * 2.0 ** -16 + 2.0 ** -21, 2: 2.0 ** -7 + 2.0 ** -13}
    assert drop0 < b[0] and drop1 < b[1] <= 2.0 ** -14 and drop2 < b[2] <= 2.0 ** -6
    return b
