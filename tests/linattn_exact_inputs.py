"""Linear-attention inputs with a closed-form answer for csrc/linattn_f32.hip (column statistics, context product, backward for k
and v) and for ops.linear_attention_qkv around them: the generator, the float64 closed form, the condition under which equality is the
right assertion, and a host model of the kernels' index space with faults that can be planted in it.

The softmax over the tokens is made to SELECT.  For image n and channel d a token set S(n, d) of 2^j tokens is chosen and

    k[n][d][t] = a(n, d) on S,  a(n, d) - GAP elsewhere,      a a multiple of 1/4, |a| <= 16, GAP = 128.

exp(-128) = 2.6e-56 lies below f32's smallest subnormal 1.4e-45, so in f32, in any order and by any merge of partial (max, sum) pairs,
exp(k - m) is exactly 1 on S and 0 off it once m = a has been seen, and a partial whose maximum is a - 128 is scaled by exp(-128) = 0
when it meets one whose maximum is a: m = a, l = 2^j, 1 / l = 2^-j and the softmaxed k is 2^-j on S, 0 elsewhere.  q and dOut are whole
numbers in [-1, 1], v in [-2, 2]: ctx, out, dctx, dq, g, dv and dk are short dyadic numbers, every reduction is exact in f32 in any
order (`assert_exactly_summable`, on the very tensors of a case) and float64 gives the same values.  So each quantity must EQUAL the
closed form: torch.equal, no tolerance.  (Float64 itself keeps exp(-128): its softmax differs from the closed form by 1e-56 relative,
which no f32 number sees; tests/test_linattn_exact_inputs.py holds the closed form to float64 autograd after one rounding to f32.)

What a wrong index must change (asserted by `assert_covers_edges`): the set sizes run through every j with 2^j <= min(T, 32), differently
in every image; over the channels of every 32-channel tile the sets hold the last token, a token of the final partial 16-token chunk,
and the first and last token of every context split (1 024) and statistics split (512); tokens of both lane halves of the context
loop (even and odd); and channel 1 of every tile selects token 9 alone (T >= 10): its maximum is first seen by row lane 1 of the
statistics kernel, after that lane has taken the non-selected token 1.  v, q and dOut are drawn per (image, channel, token).

Plain module: no fixtures, no device.  Host tensors are [N, C, T] (channel d, token t), float64; ctx and dctx are [N, C, C] ([d][e]).
"""
import math

import torch

GAP = 128.0
CTX_SPLIT = 1024         # linattn_f32.hip CTX_SPLIT (odvae_linattn_ctx_split())
STAT_SPLIT = 512         # linattn_f32.hip STAT_SPLIT
CHUNK = 16               # tokens per step of the context loop
TILE = 32
J_MAX = 5
LIMIT = float(2 ** 24)
Q_AMP, V_AMP = 1, 2

# (N, C, T): each the smallest shape that reaches its edge
CASES = (
    (2, 32, 1),                                   # one token
    (1, 32, 15), (1, 32, 16), (1, 32, 17),        # the 16-token chunk of the context loop from both sides
    (2, 64, 33),                                  # a partial 32-token tile in dkv, 2 x 2 context tiles
    (1, 160, 40),                                 # 5 tiles: 25 context tiles, 10 dkv jobs, the last workgroup half empty
    (2, 32, 511), (2, 32, 512), (2, 32, 513),     # the statistics split from both sides
    (2, 128, 1025),                               # 2 context splits x 16 tiles x 2 images, 8 dkv jobs
    (3, 96, 2051),                                # 3 context splits, 5 statistics splits, 9 tiles, 3 images
)
SINGLE = tuple(c for c in CASES if c[1] == TILE and c[2] <= STAT_SPLIT)       # one tile, one split of either kind


def ceil_div(a, b):
    return -(-a // b)


def must_tokens(t):
    """the tokens every 32-channel tile has to select somewhere: sorted, without repeats"""
    must = {t - 1, (t - 1) // CHUNK * CHUNK}
    for split in (CTX_SPLIT, STAT_SPLIT):
        for s in range(ceil_div(t, split)):
            must.update((s * split, min(t, (s + 1) * split) - 1))
    return sorted(must)


def make_case(n, c, t, seed=0):
    """dict q, k, v, do float64 [n, c, t]; a [n, c]; j [n, c] (set sizes 2^j); sel bool [n, c, t]"""
    assert c % TILE == 0 and n >= 1 and t >= 1
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * n + 131 * c + t)
    q = torch.randint(-Q_AMP, Q_AMP + 1, (n, c, t), generator=g).double()
    do = torch.randint(-Q_AMP, Q_AMP + 1, (n, c, t), generator=g).double()
    v = torch.randint(-V_AMP, V_AMP + 1, (n, c, t), generator=g).double()
    a = torch.randint(-64, 65, (n, c), generator=g).double() / 4.0
    must = must_tokens(t)
    jcap = min(J_MAX, int(math.floor(math.log2(t))))
    j = torch.empty(n, c, dtype=torch.long)
    sel = torch.zeros(n, c, t, dtype=torch.bool)
    for b in range(n):
        for d in range(c):
            dl = d % TILE
            jj = (dl + b) % (J_MAX + 1)
            first = must[(dl + 5 * b + d // TILE) % len(must)]
            if dl == 1 and t >= 10:
                jj, first = 0, 9
            jj = min(jj, jcap)
            rest = torch.randperm(t, generator=g)
            rest = rest[rest != first][: 2 ** jj - 1]
            sel[b, d, first] = True
            sel[b, d, rest] = True
            j[b, d] = jj
    k = torch.where(sel, a[:, :, None], a[:, :, None] - GAP)
    return dict(n=n, c=c, t=t, q=q, k=k, v=v, do=do, a=a, j=j, sel=sel)


def assert_covers_edges(case):
    """the properties of the module docstring, on the case's own sets"""
    n, c, t, sel, j = case["n"], case["c"], case["t"], case["sel"], case["j"]
    assert torch.equal(sel.sum(-1), 2 ** j)
    jcap = min(J_MAX, int(math.floor(math.log2(t))))
    for b in range(n):
        assert set(j[b].tolist()) == set(range(jcap + 1)), "image %d: set sizes %s" % (b, sorted(set(j[b].tolist())))
        for tile in range(c // TILE):
            any_d = sel[b, tile * TILE:(tile + 1) * TILE].any(0)
            for tok in must_tokens(t):
                assert any_d[tok], "image %d tile %d: token %d is selected by no channel" % (b, tile, tok)
            if t >= 2:
                assert any_d[0::2].any() and any_d[1::2].any()
            if t >= 10:
                d = tile * TILE + 1
                assert sel[b, d].nonzero().flatten().tolist() == [9]
    if n > 1 and jcap > 0:
        assert not torch.equal(j[0], j[1])


# ------------------------------------------------------------------------------------------------------------------------------
# the closed form
# ------------------------------------------------------------------------------------------------------------------------------
def closed_form(case):
    """float64 dict m, rinv [N, C]; s [N, C, T]; ctx, dctx [N, C, C]; g [N, C]; out, dq, dk, dv [N, C, T] with the softmaxed k taken as
    what it is in f32: 2^-j on S, 0 off it"""
    q, v, do = case["q"], case["v"], case["do"]
    rinv = 2.0 ** -case["j"].double()
    s = case["sel"].double() * rinv[:, :, None]
    ctx = torch.einsum("bdn,ben->bde", s, v)
    out = torch.einsum("bde,bdn->ben", ctx, q)
    dctx = torch.einsum("bdn,ben->bde", q, do)
    dq = torch.einsum("bde,ben->bdn", ctx, do)
    g = (ctx * dctx).sum(-1)
    dv = torch.einsum("bdn,bde->ben", s, dctx)
    dk = s * (torch.einsum("ben,bde->bdn", v, dctx) - g[:, :, None])
    return dict(m=case["a"].clone(), rinv=rinv, s=s, ctx=ctx, out=out, dctx=dctx, dq=dq, g=g, dv=dv, dk=dk)


NAMES = ("m", "rinv", "ctx", "out", "dq", "dk", "dv")


def float64_autograd(case):
    """the same quantities from the definition (tests/linattn_ref.py core) in float64, gradients by autograd"""
    import linattn_ref as R
    return R.core_refs(case["q"], case["k"], case["v"], case["do"])[64]


# ------------------------------------------------------------------------------------------------------------------------------
# the condition
# ------------------------------------------------------------------------------------------------------------------------------
def _multiples(t, unit, name):
    assert torch.equal(t.float().double(), t), "%s is not made of f32 numbers" % name
    assert torch.equal(torch.round(t / unit) * unit, t), "%s is not made of multiples of %g" % (name, unit)


def summability(case, ref=None):
    """{reduction: largest sum of |terms| in units of the reduction's grid}.  The grid of everything that carries a softmax weight
    is 2^-J_MAX (the common last place of the 2^-j); sums of whole numbers have the grid 1."""
    r = ref or closed_form(case)
    q, v, do, s = case["q"].abs(), case["v"].abs(), case["do"].abs(), r["s"]
    fine = 2.0 ** -J_MAX
    ctx, dctx = r["ctx"].abs(), r["dctx"].abs()
    u_abs = torch.einsum("ben,bde->bdn", v, dctx)
    return {
        "l": float(case["t"]),                                                                     # a sum of ones
        "ctx partial": torch.einsum("bdn,ben->bde", case["sel"].double(), v).max().item(),        # exp(k - m) = 1 on S
        "out": torch.einsum("bde,bdn->ben", ctx, q).max().item() / fine,
        "dctx": torch.einsum("bdn,ben->bde", q, do).max().item(),
        "dq": torch.einsum("bde,ben->bdn", ctx, do).max().item() / fine,
        "g": (ctx * dctx).sum(-1).max().item() / fine,
        "dv": torch.einsum("bdn,bde->ben", s, dctx).max().item() / fine,
        "dk": (u_abs + r["g"].abs()[:, :, None]).max().item() / fine,                              # u - g before the weight 2^-j
    }


def assert_exactly_summable(case, ref=None):
    """The condition under which equality is the right assertion, on the very tensors of the case: operands are f32 numbers on their
    grids, a non-selected token lies exactly GAP below its column's maximum and exp(-GAP) is 0 in f32, and for every reduction the sum
    of |terms| is below 2^24 units of its grid -- so every product and every partial sum, in any order, is an f32 number."""
    for name in ("q", "do", "v"):
        _multiples(case[name], 1.0, name)
    _multiples(case["a"], 0.25, "a")
    _multiples(case["k"], 0.25, "k")
    assert case["q"].abs().max() <= Q_AMP and case["do"].abs().max() <= Q_AMP and case["v"].abs().max() <= V_AMP
    assert case["a"].abs().max() <= 16.0
    assert torch.exp(torch.tensor(-GAP, dtype=torch.float32)).item() == 0.0
    top = case["k"].max(-1, keepdim=True).values
    assert torch.equal(top.squeeze(-1), case["a"])
    assert torch.equal(case["k"] == top, case["sel"]) and torch.equal(torch.where(case["sel"], top, top - GAP), case["k"])
    assert torch.equal(case["sel"].sum(-1), 2 ** case["j"]) and int(case["j"].max()) <= J_MAX
    s = summability(case, ref)
    for kind, units in s.items():
        assert units < LIMIT, "(%d, %d, %d) %s: sum of |terms| is %.4g units, not below 2^24: f32 operations may round" % (
            case["n"], case["c"], case["t"], kind, units)
    return s


# ------------------------------------------------------------------------------------------------------------------------------
# a host model of the kernels' index space, f32, with faults that can be planted in it
# ------------------------------------------------------------------------------------------------------------------------------
FAULTS = ("split_dropped", "image_stride_of_one_split", "tiles_exchanged_on_store", "tiles_exchanged_on_load", "ragged_rows_counted",
          "last_stat_split_ignored", "rinv_of_column_e", "g_of_another_image", "dk_dv_exchanged")
NEEDS_SEVERAL = FAULTS[:4]         # no-ops on one tile and one split: only a case with several can reject them
NEG_BIG = -3.0e38


def _merge(m, l, m2, l2):
    mn = torch.maximum(m, m2)
    return mn, l * torch.exp(m - mn) + l2 * torch.exp(m2 - mn)


def host_model(case, fault=None):
    """The three entry points and the op around them as the kernels index them: statistics partials [N][nstat][C][2] merged in split
    order; context partial tiles stored to a flat workspace at ((n nsplit + s) C + dt 32 + r) C + et 32 + col, summed in split order and
    scaled by 1 / l of the row; dkv as its job list (jobs 0 .. C/32 - 1 a tile of dv, the rest of dk, four jobs per workgroup).
    fault: None or one of FAULTS.  Returns the dict of `closed_form` (f32 tensors, without s)."""
    assert fault is None or fault in FAULTS
    n, c, t = case["n"], case["c"], case["t"]
    q, k, v, do = (case[x].float() for x in ("q", "k", "v", "do"))
    tiles = c // TILE
    # 1. column statistics
    nstat = ceil_div(t, STAT_SPLIT)
    part = torch.empty(n, nstat, c, 2)
    for s in range(nstat):
        ks = k[:, :, s * STAT_SPLIT:min(t, (s + 1) * STAT_SPLIT)]
        ms = ks.max(-1).values
        part[:, s, :, 0], part[:, s, :, 1] = ms, torch.exp(ks - ms[:, :, None]).sum(-1)
    m, l = torch.full((n, c), NEG_BIG), torch.zeros(n, c)
    for s in range(nstat - 1 if fault == "last_stat_split_ignored" and nstat > 1 else nstat):
        m, l = _merge(m, l, part[:, s, :, 0], part[:, s, :, 1])
    rinv = 1.0 / l
    # 2. context product: the statistics as the entry point is given them
    nsplit = ceil_div(t, CTX_SPLIT)
    ws = torch.full((n * nsplit * c * c,), float("nan"))
    r32, c32 = torch.arange(TILE)[:, None], torch.arange(TILE)[None, :]

    def tile_at(b, s, dt, et, ns=nsplit):
        return ((b * ns + s) * c + dt * TILE + r32) * c + et * TILE + c32

    for b in range(n):
        for s in range(nsplit):
            t0, t1 = s * CTX_SPLIT, min(t, (s + 1) * CTX_SPLIT)
            e = torch.exp(k[b, :, t0:t1] - m[b, :, None])
            vs = v[b, :, t0:t1]
            if fault == "ragged_rows_counted" and (t1 - t0) % CHUNK:        # rows past the split read its last row, and count
                extra = CHUNK - (t1 - t0) % CHUNK
                e = torch.cat([e, e[:, -1:].expand(c, extra)], 1)
                vs = torch.cat([vs, vs[:, -1:].expand(c, extra)], 1)
            full = e @ vs.t()
            for dt in range(tiles):
                for et in range(tiles):
                    tile = full[dt * TILE:(dt + 1) * TILE, et * TILE:(et + 1) * TILE]
                    if fault == "tiles_exchanged_on_store":
                        idx = tile_at(b, s, et, dt)
                    elif fault == "image_stride_of_one_split":
                        idx = tile_at(b, 0, dt, et, 1) + s * c * c            # (n * 1 + s): inside the workspace, n + s <= n nsplit + s
                    else:
                        idx = tile_at(b, s, dt, et)
                    ws[idx] = tile
    i = torch.arange(n * c * c)
    cc = c * c
    b_i, de = i // cc, i % cc
    d_i, e_i = de // c, de % c
    if fault == "tiles_exchanged_on_load":
        de = ((e_i // TILE) * TILE + d_i % TILE) * c + (d_i // TILE) * TILE + e_i % TILE
    total = torch.zeros(n * cc)
    for s in range(nsplit):
        if fault == "split_dropped" and s == 1:
            continue
        total = total + ws[(b_i * nsplit + s) * cc + de]
    ctx = (total * rinv.flatten()[b_i * c + (e_i if fault == "rinv_of_column_e" else d_i)]).view(n, c, c)
    # 3, 4. the GEMM and rowdot calls of the op
    out = torch.einsum("bde,bdn->ben", ctx, q)
    dctx = torch.einsum("bdn,ben->bde", q, do)
    dq = torch.einsum("bde,ben->bdn", ctx, do)
    g = (ctx * dctx).sum(-1)
    # 5. backward for k and v
    sm = torch.exp(k - m[:, :, None]) * rinv[:, :, None]
    dk, dv = torch.full((n, c, t), float("nan")), torch.full((n, c, t), float("nan"))
    for b in range(n):
        gb = g[(b + 1) % n] if fault == "g_of_another_image" else g[b]
        for wg in range(ceil_div(2 * tiles, 4)):
            for wave in range(4):
                job = wg * 4 + wave
                if job >= 2 * tiles:
                    continue
                is_dk = job >= tiles
                ot = job - tiles if is_dk else job
                ch = slice(ot * TILE, (ot + 1) * TILE)
                if is_dk:
                    res = sm[b, ch] * (dctx[b, ch] @ v[b] - gb[ch, None])
                else:
                    res = dctx[b][:, ch].t() @ sm[b]
                (dk if is_dk != (fault == "dk_dv_exchanged") else dv)[b, ch] = res
    return dict(m=m, rinv=rinv, ctx=ctx, out=out, dctx=dctx, dq=dq, g=g, dv=dv, dk=dk)


def differs(got, ref):
    """names of NAMES on which a model's f32 result is not the closed form (NaN counts as a difference)"""
    return [name for name in NAMES if not torch.equal(got[name].double(), ref[name])]
