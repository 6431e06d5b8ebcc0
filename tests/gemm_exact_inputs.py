"""Exactly summable inputs for the f32 GEMM family (gemm_f32.hip, gemm_f32_split.hip, gemm_f32_tile.h): generators, the poisoned
operand layout, float64 references, a Python mirror of the dispatch and the case lists of tests/test_gemm_f32_exact_gpu.py.

The f32 MFMA kernels multiply f32 numbers and add in f32; the bf16-split kernel multiplies the exact bf16 planes hi + mid + lo of its
operands and adds in f32.  If every product is a whole number of units and the sum of |terms| -- alpha, bias, residual and row vectors
included -- stays below 2^24 units (`exact_inputs.LIMIT`), no f32 addition rounds in any order and the output must EQUAL float64.

recipe  A (logical [batch][M][K])                B (logical [batch][K][N])                          unit of a product
  A     integers in [-8, 8]                      multiples of 1/4 in [-2, 2]                        2^-2   "deep": good to K = 16384
  B     odd integers, |a| <= 511                 odd k / 128, |k| <= 255                            2^-7   wide significands, K <= 128
  S1    odd integers, |a| <= 4095 (hi, mid)      {-1, 0, 1}                                         1      bf16 planes: a_mid b_hi
  S2    odd integers, 513 <= |a| <= 1023         odd integers like A, <= 8 non-zeros per column     1      ... mid mid
  S3    odd integers, 2^16 < |a| < 2^18 (lo)     {-1, 0, 1}, <= 32 non-zeros per column             1      ... a_lo b_hi
  S3T   {-1, 0, 1}, <= 32 non-zeros per row      odd integers, 2^16 < |b| < 2^18                    1      ... a_hi b_lo
bias: multiples of 1/8 in [-2, 2]; residual: integers in [-8, 8]; alpha in {1, 0.5} (a residual needs alpha == 1).
In S1-S3T the three cross products the split kernel drops (mid lo, lo mid, lo lo) are identically zero (`assert_planes`).

Plain module: no fixtures, no device.  Everything is float64 (values) or float32 (poisoned buffers) on the host.
"""
import math

import torch

from exact_inputs import LIMIT, _ints, _odd, assert_bits_equal  # noqa: F401  (re-exported for the tests)

BF = torch.bfloat16
NAN = float("nan")
BM = BN = 128
BK = 32
LAYOUTS = {"NN": (0, 0), "NT": (0, 1), "TN": (1, 0), "TT": (1, 1)}
EPILOGUES = ("plain", "alpha_bias", "bias_res")
STAGINGS = (-1, 0, 1, 2)


# ------------------------------------------------------------------------------------------------------------------------------
# the dispatch, mirrored (gemm_tile::choose_splits / split_eligible / split_tt_eligible, the staging rule of gemm_f32_impl)
# ------------------------------------------------------------------------------------------------------------------------------
def ceil_div(a, b):
    return -(-a // b)


def tiles_of(m, n):
    return ceil_div(m, BM) * ceil_div(n, BN)


def choose_splits(m, n, k, batch):
    tiles = tiles_of(m, n) * batch
    if tiles >= 512 or k <= 1024:
        return 1
    return max(1, min(512 // tiles, k // 512))


def k_per_split(k, splits):
    return ceil_div(ceil_div(k, splits), BK) * BK


def split_eligible(staging, tb, m, n, k, batch, bias=False, residual=False):
    return staging == -1 and choose_splits(m, n, k, batch) == 1 and tb == 0 and k >= 1024 and not bias and not residual


def split_tt_eligible(staging, m, n, k, batch):
    return staging == -1 and tiles_of(m, n) * batch >= 512 and k >= 64


def workspace_bytes(m, n, k, batch):
    s = choose_splits(m, n, k, batch)
    return s * batch * m * n * 4 if s > 1 else 0


def gemm_forms(layout, m, n, k, batch, staging, bias=False, residual=False):
    """the set of kernel instantiations one odvae_gemm_f32 call launches: (form, layout, epilogue) and ("splitk_reduce",)"""
    ta, tb = LAYOUTS[layout]
    if split_eligible(staging, tb, m, n, k, batch, bias, residual):
        return {("split", layout, "none")}
    splits = choose_splits(m, n, k, batch)
    bkt = (32 if ta else 0) if staging < 0 else {0: 0, 1: 32, 2: 16}[staging]
    if bkt:
        form = "dma%d" % bkt
    else:
        form = "reg_batched" if (layout == "TN" and splits == 1 and batch > 1) else "reg"
    out = {(form, layout, "none")}
    if splits > 1:
        out.add(("splitk_reduce",))
    return out


def pred_forms(layout):
    return {("pred", layout)}


def smb_forms(m, n, k, batch, staging):
    if split_tt_eligible(staging, m, n, k, batch):
        return {("split", "NT", "smb")}
    return {({2: "dma16", 1: "dma32"}.get(staging, "reg"), "NT", "smb")}


def expb_forms(m, n, k, batch, staging):
    return {("split" if split_tt_eligible(staging, m, n, k, batch) else "reg", "NT", "expb")}


def rownorm_forms(m, n, k, batch, staging):
    return {("split" if split_eligible(staging, 0, m, n, k, batch) else "reg", "NN", "rownorm")}


ALL_FORMS = ({(f, l, "none") for f in ("reg", "dma32", "dma16") for l in LAYOUTS} | {("reg_batched", "TN", "none")}
             | {("pred", l) for l in LAYOUTS} | {("splitk_reduce",)}
             | {(f, "NT", "smb") for f in ("reg", "dma32", "dma16", "split")} | {(f, "NT", "expb") for f in ("reg", "split")}
             | {(f, "NN", "rownorm") for f in ("reg", "split")} | {("split", "NN", "none"), ("split", "TN", "none")})


# ------------------------------------------------------------------------------------------------------------------------------
# the bf16 planes (a torch restatement of split8 in bf16_common.h: round to nearest even three times)
# ------------------------------------------------------------------------------------------------------------------------------
def split3(t):
    """(hi, mid, lo) of the f32 values of t, float64; hi + mid + lo == t exactly for every f32 number of ordinary range"""
    x = t.float()
    hi = x.to(BF).float()
    r = x - hi
    mid = r.to(BF).float()
    lo = (r - mid).to(BF).float()
    return hi.double(), mid.double(), lo.double()


def _abs_planes(t):
    hi, mid, lo = split3(t)
    return hi.abs() + mid.abs() + lo.abs()


def plane_products(a, b):
    """For the nine plane pairs (p, q), p, q in 'hi', 'mid', 'lo': sum over batch and k of max_row |a_p[row][k]| * max_col |b_q[k][col]|.
    Zero exactly when every product a_p[row][k] b_q[k][col] the kernel could form is zero; positive when one is not."""
    pa = {p: v.abs().amax(dim=1) for p, v in zip(("hi", "mid", "lo"), split3(a))}      # [batch][K]
    pb = {q: v.abs().amax(dim=2) for q, v in zip(("hi", "mid", "lo"), split3(b))}      # [batch or 1][K]
    return {(p, q): (pa[p] * pb[q]).sum().item() for p in pa for q in pb}


PLANES_OF = {"S1": ("mid", "hi"), "S2": ("mid", "mid"), "S3": ("lo", "hi"), "S3T": ("hi", "lo")}


def assert_planes(c):
    """The split recipes: hi + mid + lo restores both operands, the three dropped cross products are identically zero, and the plane
    pair the recipe is named for carries something."""
    for name in ("a", "b"):
        assert torch.equal(sum(split3(c[name])), c[name]), "%s is not hi + mid + lo" % name
    pp = plane_products(c["a"], c["b"])
    for pair in (("mid", "lo"), ("lo", "mid"), ("lo", "lo")):
        assert pp[pair] == 0.0, "recipe %s: the dropped product %s x %s is not identically zero" % (c["recipe"], pair[0], pair[1])
    want = PLANES_OF[c["recipe"]]
    assert pp[want] > 0.0, "recipe %s does not reach %s x %s" % (c["recipe"], want[0], want[1])
    return pp


# ------------------------------------------------------------------------------------------------------------------------------
# generators: logical operands a [batch][M][K], b [batch or 1][K][N] (one b for all batches: batch stride 0)
# ------------------------------------------------------------------------------------------------------------------------------
def _seed(recipe, m, n, k, batch, seed):
    return 1000003 * seed + 7919 * sum(ord(ch) for ch in recipe) + 131 * m + 17 * n + 3 * k + batch


def _sparse_cols(g, t, keep):
    """keep at most `keep` non-zeros per column of t [.., K, N]: positions chosen at random"""
    k = t.shape[-2]
    if k <= keep:
        return t
    rank = torch.rand(t.shape, generator=g).argsort(dim=-2).argsort(dim=-2)
    return t * (rank < keep)


def _odd_between(g, shape, lo, hi):
    """odd integers with lo < |v| <= hi, both signs (lo even, hi odd)"""
    mag = lo + 2 * torch.randint(0, (hi - lo + 1) // 2, shape, generator=g) + 1
    sign = 2 * torch.randint(0, 2, shape, generator=g) - 1
    return (mag * sign).double()


def make_case(recipe, m, n, k, batch, epi="plain", seed=0, shared_b=False):
    """dict: a, b, bias | None, res | None, alpha, units {a, b, bias, res}, recipe, epi"""
    g = torch.Generator().manual_seed(_seed(recipe, m, n, k, batch, seed))
    sa, sb = (batch, m, k), (1 if shared_b else batch, k, n)
    c = {"recipe": recipe, "epi": epi, "units": {"a": 1.0, "b": 1.0, "bias": 0.125, "res": 1.0}}
    if recipe == "A":
        c["a"], c["b"] = _ints(g, sa, -8, 8), _ints(g, sb, -8, 8) / 4
        c["units"]["b"] = 0.25
    elif recipe == "B":
        assert k <= 128
        c["a"], c["b"] = _odd(g, sa, 511), _odd(g, sb, 255) / 128
        c["units"]["b"] = 2.0 ** -7
    elif recipe == "S1":
        c["a"], c["b"] = _odd(g, sa, 4095), _ints(g, sb, -1, 1)
    elif recipe == "S2":
        c["a"] = _odd_between(g, sa, 512, 1023)
        c["b"] = _sparse_cols(g, _odd_between(g, sb, 512, 1023), 8)
    elif recipe == "S3":
        c["a"] = _odd_between(g, sa, 2 ** 16, 2 ** 18 - 1)
        c["b"] = _sparse_cols(g, _ints(g, sb, -1, 1), 32)
    elif recipe == "S3T":
        c["a"] = _sparse_cols(g, _ints(g, (batch, k, m), -1, 1), 32).transpose(1, 2).contiguous()
        c["b"] = _odd_between(g, sb, 2 ** 16, 2 ** 18 - 1)
    else:
        raise ValueError("recipe %r" % (recipe,))
    c["alpha"] = 0.5 if epi == "alpha_bias" else 1.0
    c["bias"] = _ints(g, (n,), -16, 16) / 8 if epi in ("alpha_bias", "bias_res") else None
    c["res"] = _ints(g, (batch, m, n), -8, 8) if epi == "bias_res" else None
    return c


def reference(c):
    """float64: alpha a b + bias + res, [batch][M][N]"""
    y = c["alpha"] * torch.matmul(c["a"], c["b"])
    if c["bias"] is not None:
        y = y + c["bias"]
    if c["res"] is not None:
        y = y + c["res"]
    return y


def output_unit(c):
    u = c["units"]
    unit = u["a"] * u["b"] * c["alpha"]
    if c["bias"] is not None:
        unit = min(unit, u["bias"])
    if c["res"] is not None:
        unit = min(unit, u["res"])
    return unit


def summability(c):
    """sum of |terms| in units, per kind of sum the kernels form.  `product`: the accumulators before alpha (f32 kernels: sum |a| |b|;
    split kernel: the same over all nine plane pairs, an upper bound of the six it adds); `output`: alpha, bias and residual joined."""
    u = c["units"]
    sab = torch.matmul(_abs_planes(c["a"]), _abs_planes(c["b"]))      # >= |a| |b| summed over k
    out = {"product": sab.max().item() / (u["a"] * u["b"])}
    tot = c["alpha"] * sab
    if c["bias"] is not None:
        tot = tot + c["bias"].abs()
    if c["res"] is not None:
        tot = tot + c["res"].abs()
    out["output"] = tot.max().item() / output_unit(c)
    return out


def _assert_multiples(t, unit, what):
    assert torch.equal(t.float().double(), t), "%s is not made of f32 numbers" % what
    assert torch.equal(torch.round(t / unit) * unit, t), "%s is not made of multiples of %g" % (what, unit)


def assert_exactly_summable(c):
    """(1) every operand is made of f32 numbers that are whole multiples of its unit -- and so is each of its bf16 planes, which is what
    the split kernel multiplies; (2) every sum stays below 2^24 units with |terms| in place of terms."""
    for name in ("a", "b", "bias", "res"):
        if c[name] is None:
            continue
        _assert_multiples(c[name], c["units"][name], name)
        if name in ("a", "b"):
            for plane in split3(c[name]):
                _assert_multiples(plane, c["units"][name], "a bf16 plane of " + name)
    assert c["res"] is None or c["alpha"] == 1.0
    assert math.frexp(c["alpha"])[0] == 0.5, "alpha must be a power of two"
    s = summability(c)
    for kind, units in s.items():
        assert units < LIMIT, "%s: sum of |terms| is %.4g units, not below 2^24: f32 additions may round" % (kind, units)
    return s


# ------------------------------------------------------------------------------------------------------------------------------
# row-vector epilogues
# ------------------------------------------------------------------------------------------------------------------------------
SMB_ALPHA = 2.0 ** -3


def make_smb_case(m, n, k, batch, scaled, seed=0):
    """dS = alpha P .* (A B^T - rowdot) (* rowmul): a, b as recipe A (b logical [batch][K][N], the kernel reads its transpose),
    rowdot integers in [-8, 8], p multiples of 1/8 in [0, 1], rowmul powers of two 2^-2 .. 2^2 (scaled) or None"""
    c = make_case("A", m, n, k, batch, "plain", seed=seed + 50)
    g = torch.Generator().manual_seed(_seed("SMB", m, n, k, batch, seed))
    c["rowdot"] = _ints(g, (batch, m), -8, 8)
    c["p"] = _ints(g, (batch, m, n), 0, 8) / 8
    c["rowmul"] = 2.0 ** _ints(g, (batch, m), -2, 2) if scaled else None
    c["alpha"] = SMB_ALPHA
    return c


def smb_reference(c):
    s = torch.matmul(c["a"], c["b"]) - c["rowdot"][:, :, None]
    f = c["alpha"] * (c["rowmul"][:, :, None] if c["rowmul"] is not None else 1.0)
    return s * f * c["p"]


def assert_smb_exact(c):
    """the sums (products and -rowdot, unit 1/4) stay below 2^24 units; the tail multiplies by powers of two (exact) and by p = j / 8,
    j <= 8: a 4-bit factor, exact while |sum| < 2^20 units"""
    for name, unit in (("a", 1.0), ("b", 0.25), ("rowdot", 1.0), ("p", 0.125)):
        _assert_multiples(c[name], unit, name)
    assert c["p"].min().item() >= 0.0 and c["p"].max().item() <= 1.0
    if c["rowmul"] is not None:
        assert all(math.frexp(v)[0] == 0.5 for v in c["rowmul"].unique().tolist()), "rowmul must hold powers of two"
    worst = (torch.matmul(_abs_planes(c["a"]), _abs_planes(c["b"])) + c["rowdot"].abs()[:, :, None]).max().item() / 0.25
    assert worst < LIMIT / 16, "softmax-backward tail: %g units leave no room for the 4-bit factor" % worst
    assert torch.equal(smb_reference(c).float().double(), smb_reference(c))
    return worst


EXPB_ALPHA = 2.0 ** -3
EXPB_FAR = 2048.0      # alpha * 2048 * log2(e) = 369.3: exp2 of the negative is 0 in f32, denormals included (2^-149)


def make_expb_case(m, n, k, batch, seed=0):
    """E = exp(alpha (A B^T - bound)), integer scores.  Columns come in three classes (c["cls"], [N]):
      0 "one":   B's column is the vector v every bound is made from (bound_i = a_i . v): score - bound == 0, E == 1.0
      1 "far":   v with -64 in its last k (a's last k is 64 everywhere): score - bound == -4096, E == 0.0
      2 "near":  v plus three entries of +-1: score - bound = a_i . delta, |.| <= 12 -- compared form against form only"""
    g = torch.Generator().manual_seed(_seed("EXPB", m, n, k, batch, seed))
    a = _ints(g, (batch, m, k), -4, 4)
    a[:, :, k - 1] = 64.0
    v = _ints(g, (batch, k, 1), -4, 4)
    v[:, k - 1] = 0.0
    cls = torch.randint(0, 3, (n,), generator=g)
    cls[:3] = torch.tensor([0, 1, 2])
    cls[n - 3:] = torch.tensor([2, 1, 0])      # every class in the ragged last column tile too
    b = v.repeat(1, 1, n)
    b[:, k - 1, cls == 1] = -64.0
    delta = _sparse_cols(g, _odd(g, (batch, k - 1, n), 1), 3)
    b[:, :k - 1] += delta * (cls == 2)
    bound = torch.matmul(a, v)[:, :, 0]
    return {"a": a, "b": b, "bound": bound, "cls": cls, "alpha": EXPB_ALPHA}


def assert_expb_exact(c):
    for name in ("a", "b", "bound"):
        _assert_multiples(c[name], 1.0, name)
    worst = (torch.matmul(c["a"].abs(), c["b"].abs()) + c["bound"].abs()[:, :, None]).max().item()
    assert worst < LIMIT
    d = torch.matmul(c["a"], c["b"]) - c["bound"][:, :, None]
    assert (d[:, :, c["cls"] == 0] == 0).all()
    assert (d[:, :, c["cls"] == 1] <= -EXPB_FAR).all()
    assert c["alpha"] * EXPB_FAR * math.log2(math.e) > 149 + 24
    near = d[:, :, c["cls"] == 2]
    assert (near != 0).any() and near.abs().max().item() <= 12
    return d


def make_rownorm_case(m, n, k, batch, seed=0, shared_b=False):
    """C = (A B) / l, l = row sums of A: a non-negative integers in [0, 8] whose last element makes the row sum a power of two;
    b multiples of 1/4 in [-2, 2]"""
    g = torch.Generator().manual_seed(_seed("RN", m, n, k, batch, seed))
    a = _ints(g, (batch, m, k), 0, 8)
    part = a[:, :, :k - 1].sum(2)
    a[:, :, k - 1] = 2.0 ** torch.ceil(torch.log2(part + 1.0)) - part
    b = _ints(g, (1 if shared_b else batch, k, n), -8, 8) / 4
    return {"a": a, "b": b, "recipe": "A", "units": {"a": 1.0, "b": 0.25}}


def assert_rownorm_exact(c):
    _assert_multiples(c["a"], 1.0, "a")
    _assert_multiples(c["b"], 0.25, "b")
    assert c["a"].min().item() >= 0.0
    l = c["a"].sum(2)
    assert all(math.frexp(v)[0] == 0.5 for v in l.unique().tolist()), "a row sum is no power of two"
    assert l.max().item() < LIMIT and l.min().item() >= 1.0
    assert torch.matmul(_abs_planes(c["a"]), _abs_planes(c["b"])).max().item() / 0.25 < LIMIT
    return l


# ------------------------------------------------------------------------------------------------------------------------------
# poisoned layouts: every element an operand's descriptor must not read, and every output element a kernel must not write, is NaN
# ------------------------------------------------------------------------------------------------------------------------------
LEAD = 4       # floats in front of an operand (keeps 16-byte alignment)


class Embedded(object):
    """A logical [batch][rows][cols] matrix inside a NaN-filled flat f32 buffer: element (b, r, c) at LEAD + b * stride + r * ld + c,
    ld > cols, stride > rows * ld (stride 0: one matrix for every batch), NaN rows behind the last matrix.  `index` addresses the
    logical elements, `mask` marks them."""

    def __init__(self, batch, rows, cols, ld_pad=4, gap=8, fill=NAN, shared=False):
        self.batch, self.rows, self.cols = batch, rows, cols
        self.ld = ceil_div(cols, 4) * 4 + ld_pad
        self.stride = 0 if shared else rows * self.ld + gap
        nb = 1 if shared else batch
        self.numel = LEAD + nb * (rows * self.ld + gap) + 2 * self.ld
        self.index = (LEAD + torch.arange(nb)[:, None, None] * (rows * self.ld + gap) + torch.arange(rows)[None, :, None] * self.ld
                      + torch.arange(cols)[None, None, :])
        self.fill = fill

    def buffer(self, values=None):
        buf = torch.full((self.numel,), self.fill, dtype=torch.float32)
        if values is not None:
            assert tuple(values.shape) == tuple(self.index.shape), (values.shape, self.index.shape)
            buf[self.index.reshape(-1)] = values.reshape(-1).float()
        return buf

    def mask(self):
        m = torch.zeros(self.numel, dtype=torch.bool)
        m[self.index.reshape(-1)] = True
        return m


def stored(layout_t, logical):
    """the stored form of a logical [batch][R][C] operand: transposed when the layout flag says so"""
    return logical.transpose(1, 2).contiguous() if layout_t else logical


def embed_operands(layout, c):
    """(Embedded A, buffer A, Embedded B, buffer B) for logical a [batch][M][K], b [batch or 1][K][N] under layout NN / NT / TN / TT"""
    ta, tb = LAYOUTS[layout]
    sa = stored(ta, c["a"])              # [M][K] or [K][M]
    sb = stored(tb, c["b"])              # [K][N] or [N][K]
    ea = Embedded(sa.shape[0], sa.shape[1], sa.shape[2])
    eb = Embedded(c["a"].shape[0], sb.shape[1], sb.shape[2], shared=sb.shape[0] == 1 and c["a"].shape[0] > 1)
    return ea, ea.buffer(sa), eb, eb.buffer(sb)


# ------------------------------------------------------------------------------------------------------------------------------
# the case lists of tests/test_gemm_f32_exact_gpu.py (the coverage meta-test in tests/test_gemm_exact_inputs.py reads them)
# ------------------------------------------------------------------------------------------------------------------------------
def _unsplit_cases():
    out = []
    for layout in LAYOUTS:
        shapes = [(128, 128, 32, 1), (132, 260, 100, 3), (4, 260, 36, 1)]
        if layout == "NT":
            shapes.append((1, 132, 8, 2))
        if layout == "TN":
            shapes += [(132, 132, kk, 1) for kk in (1, 33, 37)] + [(132, 132, 36, 3)]
        else:
            shapes += [(132, 132, kk, 1) for kk in (4, 8, 12)]
        for shape in shapes:
            for recipe in ("A", "B"):
                for epi in EPILOGUES:
                    out.append((layout, recipe, epi) + shape)
    return out


UNSPLIT_CASES = _unsplit_cases()          # (layout, recipe, epilogue, M, N, K, batch); every one runs under the four staging modes

# (layout, M, N, K, batch, splits): one 128 x 128 tile; every one with the three epilogues and the four staging modes
SPLITK_CASES = ([(l, 128, 128, 1027 if l == "TN" else 1028, 1, 2) for l in LAYOUTS] + [(l, 128, 128, 3000, 1, 5) for l in LAYOUTS]
                + [(l, 128, 128, 9220, 1, 18) for l in LAYOUTS] + [(l, 128, 128, 3000, 2, 5) for l in ("NT", "TN")])

PRED_CASES = [(l, 132, 132, 36, b) for l in LAYOUTS for b in (2, 260)]      # (layout, M, N, K, batch): 8 and 1040 (tile, batch) pairs

# (layout, M, N, K, batch, shared B).  K = 1024 opens split_eligible at any tile count; past it choose_splits must say 1, which takes
# 512 (tile, batch) pairs: the batch-2 shapes at K = 1028 / 1051 run split-K on the f32 kernels (and must be exact there), the
# batch-128 ones are the bf16-split kernel's partial last step.
SPLIT_CASES = ([(l, m, n, 1024, 2, False) for l in ("NN", "TN") for m, n in ((128, 128), (132, 200))]
               + [(l, m, n, 1028 if l == "NN" else 1051, 2, False) for l in ("NN", "TN") for m, n in ((128, 128), (132, 200))]
               + [("NN", 132, 200, 1028, 128, True), ("TN", 132, 200, 1051, 128, True)])
SPLIT_RECIPES = ("A", "S1", "S2", "S3", "S3T")

TT_SHAPES = [(132, 132, 36, 3), (132, 132, 68, 128)]      # (M, N, K, batch): the f32 forms; the split-TT form (4 tiles x 128 = 512)
SMB_STAGINGS = {(132, 132, 36, 3): (-1, 0, 1, 2), (132, 132, 68, 128): (-1, 1)}
EXPB_STAGINGS = {(132, 132, 36, 3): (-1, 1), (132, 132, 68, 128): (-1, 1)}
# (M, N, K, batch, shared B): the register form; the split form at K = 1024; K = 1028 at batch 2 stays on the register form
# (choose_splits says 2), at 4 tiles x 128 it is the split form's partial last step
ROWNORM_CASES = [(132, 132, 100, 3, False), (132, 132, 1024, 2, False), (132, 132, 1028, 2, False), (132, 132, 1028, 128, True)]

CONV1X1_CASES = [(3, 36, 20, 5, 7), (2, 128, 132, 16, 9), (2, 32, 64, 24, 24), (1, 32, 64, 32, 32)]      # (n, cin, cout, h, w)


def make_conv1x1_case(n, cin, cout, h, w, seed=0):
    """ops.conv1x1 on recipe A: x, dy, res integers in [-8, 8], w multiples of 1/4 in [-2, 2], b multiples of 1/8 (float64 NCHW)"""
    g = torch.Generator().manual_seed(_seed("C1", n, cin, cout, h * w, seed))
    return {"x": _ints(g, (n, cin, h, w), -8, 8), "w": _ints(g, (cout, cin, 1, 1), -8, 8) / 4, "b": _ints(g, (cout,), -16, 16) / 8,
            "res": _ints(g, (n, cout, h, w), -8, 8), "dy": _ints(g, (n, cout, h, w), -8, 8)}


def conv1x1_references(c):
    w2 = c["w"][:, :, 0, 0]
    return {"y": torch.einsum("nchw,oc->nohw", c["x"], w2) + c["b"][None, :, None, None] + c["res"],
            "dx": torch.einsum("nohw,oc->nchw", c["dy"], w2), "dw": torch.einsum("nohw,nchw->oc", c["dy"], c["x"])[:, :, None, None],
            "db": c["dy"].sum((0, 2, 3))}


def assert_conv1x1_exactly_summable(c):
    for name, unit in (("x", 1.0), ("w", 0.25), ("b", 0.125), ("res", 1.0), ("dy", 1.0)):
        _assert_multiples(c[name], unit, name)
        if name != "b":
            assert torch.equal(c[name].float().to(BF).double(), c[name]), "%s has more than a hi plane" % name
    a = {k: v.abs() for k, v in c.items()}
    r = conv1x1_references(a)
    worst = {"y": r["y"].max().item() / 0.125, "dx": r["dx"].max().item() / 0.25, "dw": r["dw"].max().item(), "db": r["db"].max().item()}
    for kind, units in worst.items():
        assert units < LIMIT, "%s: %g units" % (kind, units)
    return worst


def conv1x1_forms(n, cin, cout, h, w):
    """the three products of ops.conv1x1 (staging per shape): forward NT with bias, dx NN, dw TN"""
    px = n * h * w
    return {"forward": gemm_forms("NT", px, cout, cin, 1, -1, bias=True), "dx": gemm_forms("NN", px, cin, cout, 1, -1),
            "dw": gemm_forms("TN", cout, cin, px, 1, -1)}


def forms_reached():
    got = set()
    for layout, recipe, epi, m, n, k, batch in UNSPLIT_CASES:
        for st in STAGINGS:
            got |= gemm_forms(layout, m, n, k, batch, st, epi != "plain", epi == "bias_res")
    for layout, m, n, k, batch, splits in SPLITK_CASES:
        for st in STAGINGS:
            for epi in EPILOGUES:
                got |= gemm_forms(layout, m, n, k, batch, st, epi != "plain", epi == "bias_res")
    for layout, m, n, k, batch in PRED_CASES:
        got |= pred_forms(layout)
    for layout, m, n, k, batch, shared in SPLIT_CASES:
        got |= gemm_forms(layout, m, n, k, batch, -1)
    for shape in TT_SHAPES:
        for st in SMB_STAGINGS[shape]:
            got |= smb_forms(*shape, st)
        for st in EXPB_STAGINGS[shape]:
            got |= expb_forms(*shape, st)
    for m, n, k, batch, shared in ROWNORM_CASES:
        got |= rownorm_forms(m, n, k, batch, -1)
    for case in CONV1X1_CASES:
        for forms in conv1x1_forms(*case).values():
            got |= forms
    return got
