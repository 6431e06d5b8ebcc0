"""Exactly summable inputs, float64 references and cases for the f32 3x3 conv forward and data-gradient kernels
(csrc/conv3x3_f32.hip, conv3x3_wino_f32.hip, conv3x3_wino4_f32.hip), for tests/test_conv_f32_exact_inputs.py (host) and
tests/test_conv3x3_f32_exact_gpu.py.  Plain module: no fixtures, no device.  All tensors are float64 NCHW on the host.

The kernels multiply f32 by f32 on the f32 MFMA and add in f32; the Winograd transforms use whole (B^T, A^T) or dyadic (F(2x2): G) or
k/24 (F(4x4): G) coefficients.  If every partial sum a kernel could form -- in any order -- is a whole multiple of one unit 2^-s and
stays below 2^24 units, no f32 operation rounds and the output must EQUAL the float64 convolution: no tolerance.

    route     operands (tests/exact_inputs.py recipes)                                          unit of y
    direct    recipe A: x, dy integers in [-4, 4], w multiples of 1/4, bias of 1/8, residual whole  2^-3
    wino2     recipe A; U = G g G^T has multiples of 1/16                                           2^-4
    wino4     x, dy in {-1, 0, 1}; w = 576 m 2^-10 = 9 m / 16 with m in {-1, 0, 1}: G's entries are   2^-10
              k / 24, so U = G g G^T = 2^-10 (24 G) m (24 G)^T is dyadic; bias, residual multiples of 1/2
    stats     wino4 with 8 / Cin of the weights kept (recipe C's thinning; 2 / Cin at 16 channels per group, where a sum has 8192
              squares and 8 / Cin reaches 2.65e7 units), so that sum y^2 per tile and group stays summable

`assert_exactly_summable(case, route)` checks the condition on the very tensors a test uses.  For the direct kernels it is the bound of
exact_inputs: conv(|x|, |w|) + |b| + |res| in units.  For the Winograd kernels the transforms are evaluated on the host (`winograd`)
and two sums are bounded: sum over Cin of |V| |U| (what the MFMA accumulates per xi) and |A^T| |M| |A| + |b| + |res| (what the output
transform adds up), the latter on the actual M.

The references are nine shifted products each (`conv_ref`, `dgrad_ref`): no torch.nn.functional convolution, no autograd -- the host
test compares them with both.

    mode 0  stride 1, pad 1           mode 1  pad (0, 1, 0, 1), stride 2           mode 2  nearest 2x, then stride 1, pad 1
    The C ABI's mode 3 is the data gradient of mode 1, mode 5 is mode 2 by output parity class, mode 6 the data gradient of 2 / 5.
"""
import torch
import torch.nn.functional as F

import exact_inputs as E

LIMIT = E.LIMIT                 # 2^24
W4_SCALE = 576.0 * 2.0 ** -10   # F(4x4) weights are m * W4_SCALE
W4_UNIT = 2.0 ** -10

# Winograd matrices (csrc/conv3x3_wino_f32.hip, conv3x3_wino4_f32.hip)
BT2 = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
G2 = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
AT2 = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)
BT4 = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                    [0, 4, 0, -5, 0, 1]], dtype=torch.float64)
G4_24 = torch.tensor([[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]], dtype=torch.float64)   # 24 G: whole numbers
G4 = G4_24 / 24.0
AT4 = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=torch.float64)
WINO = {2: (BT2, G2, AT2), 4: (BT4, G4, AT4)}


# ------------------------------------------------------------------------------------------------------------------------------
# float64 references: nine shifted products, no convolution routine
# ------------------------------------------------------------------------------------------------------------------------------
def out_hw(mode, h, w):
    if mode == 1:
        assert h % 2 == 0 and w % 2 == 0
        return h // 2, w // 2
    if mode == 2:
        return 2 * h, 2 * w
    assert mode == 0, mode
    return h, w


def upsample2x(x):
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def pool2x2(t):
    return t[:, :, 0::2, 0::2] + t[:, :, 0::2, 1::2] + t[:, :, 1::2, 0::2] + t[:, :, 1::2, 1::2]


def _taps_input(mode, x):
    """(the padded tensor the nine taps slide over, stride)"""
    if mode == 0:
        return F.pad(x, (1, 1, 1, 1)), 1
    if mode == 1:
        return F.pad(x, (0, 1, 0, 1)), 2
    assert mode == 2, mode
    return F.pad(upsample2x(x), (1, 1, 1, 1)), 1


def conv_ref(mode, x, w, b=None, res=None, relu=False):
    """y = act(conv(x) + b + res), float64: y[:, co] = sum over (kh, kw, ci) of xs(kh, kw)[:, ci] w[co, ci, kh, kw]"""
    xin, s = _taps_input(mode, x.double())
    ho, wo = out_hw(mode, x.shape[2], x.shape[3])
    w = w.double()
    y = torch.zeros(x.shape[0], w.shape[0], ho, wo, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            xs = xin[:, :, kh:kh + s * (ho - 1) + 1:s, kw:kw + s * (wo - 1) + 1:s]
            y += torch.einsum("nchw,oc->nohw", xs, w[:, :, kh, kw])
    if b is not None:
        y = y + b.double().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double()
    return y.clamp_min(0.0) if relu else y


def dgrad_full_ref(mode, dy, w, x_shape):
    """Gradient w.r.t. the tensor the taps slide over, without its padding: for mode 2 that is the UPSAMPLED image [n, cin, 2h, 2w].
    Tap (kh, kw) scatters dy[:, co] w[co, ci, kh, kw] to the input positions it read."""
    n, cin, h, wd = x_shape
    xin, s = _taps_input(mode, torch.zeros(n, cin, h, wd, dtype=torch.float64))
    ho, wo = out_hw(mode, h, wd)
    assert tuple(dy.shape[2:]) == (ho, wo)
    g = torch.zeros_like(xin)
    w, dy = w.double(), dy.double()
    for kh in range(3):
        for kw in range(3):
            g[:, :, kh:kh + s * (ho - 1) + 1:s, kw:kw + s * (wo - 1) + 1:s] += torch.einsum("nohw,oc->nchw", dy, w[:, :, kh, kw])
    if mode == 1:
        return g[:, :, :h, :wd].contiguous()
    return g[:, :, 1:-1, 1:-1].contiguous()


def dgrad_ref(mode, dy, w, x_shape):
    """Gradient w.r.t. x itself: mode 2 adds the 2x2 sum-pool that nearest upsampling's backward takes."""
    g = dgrad_full_ref(mode, dy, w, x_shape)
    return pool2x2(g) if mode == 2 else g


def tile_group_sums(y, groups, tile):
    return E.tile_group_sums(y, groups, tile)


# ------------------------------------------------------------------------------------------------------------------------------
# Winograd on the host
# ------------------------------------------------------------------------------------------------------------------------------
def flipped(w):
    """the data gradient's weights: taps flipped, channel roles swapped"""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def winograd_U(w, m):
    """U[a][b][co][ci] = (G g G^T)[a][b], float64.  F(4x4): as (24 G) g (24 G)^T / 576 -- whole coefficients, one correctly rounded
    division: exact wherever the quotient is a float64 number, which 1/24 itself is not"""
    if m == 4:
        return torch.einsum("ai,ocij,bj->aboc", G4_24, w.double(), G4_24) / 576.0
    return torch.einsum("ai,ocij,bj->aboc", G2, w.double(), G2)


def winograd(x, w, m):
    """Stride-1 pad-1 conv of x [n, c, h, w] (h, w multiples of m) by F(m x m, 3x3) in float64: dict(y, V, U, M)."""
    BT, G, AT = WINO[m]
    n, c, h, wd = x.shape
    assert h % m == 0 and wd % m == 0
    t = m + 2
    d = F.pad(x.double(), (1, 1, 1, 1)).unfold(2, t, m).unfold(3, t, m)          # [n, c, ty, tx, t, t]
    U = winograd_U(w, m)
    V = torch.einsum("ai,nctuij,bj->nctuab", BT, d, BT)
    M = torch.einsum("nctuab,aboc->notuab", V, U)
    return {"V": V, "U": U, "M": M, "y": _output_transform(M, AT)}


def _output_transform(M, AT, absolute=False):
    if absolute:
        M, AT = M.abs(), AT.abs()
    Y = torch.einsum("ia,notuab,jb->notiuj", AT, M, AT)
    n, o, ty, m, tx, _ = Y.shape
    return Y.reshape(n, o, ty * m, tx * m)


def winograd_bounds(x, w, m, extra=None, pooled=False):
    """(sum over Cin of |V| |U|, |A^T| |M| |A| (+ extra) on the actual M), both as the largest value over all elements, in the
    operands' own scale.  pooled: the output transform's values are 2x2-summed (EPI_POOL) -- bound the sums of four."""
    r = winograd(x, w, m)
    mac = torch.einsum("nctuab,aboc->notuab", r["V"].abs(), r["U"].abs()).max().item()
    out = _output_transform(r["M"], WINO[m][2], absolute=True)
    if extra is not None:
        out = out + extra
    if pooled:
        out = pool2x2(out)
    return mac, out.max().item()


def wino4_pack_f64(w):
    """(fwd, dgrad) F(4x4) packs of w [cout, cin, 3, 3] in float64, flat, in the layout conv3x3_pack_wino4_kernel documents:
    [xi = 6a + b][redP / 4][outP][4] with the reduction axis padded to 8 and the output axis to 64, padding zero.
    fwd: reduce = cin, out = cout, U = G g G^T.  dgrad: reduce = cout, out = cin, g with flipped taps."""
    packs = []
    for g in (w.double(), flipped(w.double())):
        out_c, red_c = g.shape[0], g.shape[1]
        redP, outP = -(-red_c // 8) * 8, -(-out_c // 64) * 64
        U = winograd_U(g, 4).reshape(36, out_c, red_c)                     # [xi][out][red]
        P = torch.zeros(36, redP, outP, dtype=torch.float64)
        P[:, :red_c, :out_c] = U.transpose(1, 2)
        packs.append(P.reshape(36, redP // 4, 4, outP).transpose(2, 3).contiguous().reshape(-1))
    return packs[0], packs[1]


def wino4_pack_abs_f64(w):
    """|G| |g| |G|^T in the layout of wino4_pack_f64: the scale of the device pack's forward error"""
    packs = []
    Ga = G4_24.abs()
    for g in (w.double().abs(), flipped(w.double().abs())):
        out_c, red_c = g.shape[0], g.shape[1]
        redP, outP = -(-red_c // 8) * 8, -(-out_c // 64) * 64
        U = (torch.einsum("ai,ocij,bj->aboc", Ga, g, Ga) / 576.0).reshape(36, out_c, red_c)
        P = torch.zeros(36, redP, outP, dtype=torch.float64)
        P[:, :red_c, :out_c] = U.transpose(1, 2)
        packs.append(P.reshape(36, redP // 4, 4, outP).transpose(2, 3).contiguous().reshape(-1))
    return packs[0], packs[1]


# Roundings on the longest path of conv3x3_pack_wino4_kernel, per pass (both passes run the same six expressions):
#   rows 3, 4:  f = x0 * c24 + x2 * c6;  f +- x1 * c12     x0, x2: constant, product, sum f, last sum = 4;  x1: constant, product, sum = 3
#   rows 1, 2:  -((x0 + x2) +- x1) * c6                    x0, x2: sum, sum, constant, product = 4;        x1: sum, constant, product = 3
#   rows 0, 5:  0.25 x0, x2                                 none
# (c6, c12, c24 are 1/6, 1/12, 1/24 rounded to f32: one rounding each; a contraction to fma only removes roundings.)  Every term of an
# entry of U carries at most 4 + 4 = 8 factors (1 + d), |d| <= 2^-24.
W4_PACK_ROUNDINGS = 8


# ------------------------------------------------------------------------------------------------------------------------------
# the persistent forms (conv3x3_wino_f32.hip: odvae_conv3x3_wino_f32, Cout % 128 == 0; conv3x3_wino4_f32.hip: wino4_launch)
# ------------------------------------------------------------------------------------------------------------------------------
WINO_TILE = {2: (8, 16), 4: (16, 32)}       # output pixels per block tile
WINO_BN = {2: 128, 4: 64}                   # output channels per block (F(2x2): the 8-wave kernel)
WINO_KC = {2: 16, 4: 8}


def tiles_of(m, n, h, w):
    th, tw = WINO_TILE[m]
    return n * (-(-h // th)) * (-(-w // tw))


def persistent_plan(m, cus, n, h, w, cin, cout):
    """dict(persistent, blocks_per_co, tiles, uneven) by the launchers' rule.  F(2x2) (8-wave kernel only, Cout % 128 == 0): even chunk
    count >= 4, G % (8 ny) == 0, tiles >= 2 G / ny.  F(4x4): the same without the chunk condition.  G = CU count, ny = co blocks."""
    bn, kc = WINO_BN[m], WINO_KC[m]
    ny = -(-cout // bn)
    tiles = tiles_of(m, n, h, w)
    ok = cus % (8 * ny) == 0 and tiles >= 2 * (cus // ny)
    if m == 2:
        nchunks = -(-cin // kc)
        ok = ok and cout % bn == 0 and nchunks >= 4 and nchunks % 2 == 0
    per = cus // ny if cus % ny == 0 else 0
    return {"persistent": bool(ok), "blocks_per_co": per, "tiles": tiles, "uneven": bool(ok) and tiles % per != 0}


def persistent_n(m, cus, h, w, cin, cout):
    """the smallest N at which the layer runs persistently with an UNEVEN number of tiles per block (some blocks walk one tile more than
    others), or None where no N does (a CU count the rule never accepts for this Cout)"""
    for n in range(1, 4097):
        p = persistent_plan(m, cus, n, h, w, cin, cout)
        if p["persistent"] and p["uneven"]:
            return n
    return None


# ------------------------------------------------------------------------------------------------------------------------------
# cases.  hi, wi: the forward conv's INPUT size.  Every case runs the forward call(s) and the data-gradient call.
# ------------------------------------------------------------------------------------------------------------------------------
def _c(route, mode, n, cin, cout, h, w, reaches, **kw):
    d = dict(route=route, mode=mode, n=n, cin=cin, cout=cout, hi=h, wi=w, reaches=reaches)
    d.update(kw)
    return d


# direct: odvae_conv3x3_f32.  abi = the C ABI's forward mode (0, 1, 2 or 5); the data-gradient call is mode 0 / 3 / 0 at 2h x 2w / 6.
DIRECT_CASES = {
    "m0-wide-ragged": _c("direct", 0, 2, 40, 160, 11, 21, "v2<0,32> 128-wide; ragged on both axes, Cin 40 padded to 64, Cout 160 = 128 + 32; dgrad v2<0,32> 128-wide (Cout' 40), five chunks", abi=0),
    "m0-narrow-ragged": _c("direct", 0, 2, 40, 24, 11, 21, "v2<0,32> 32-wide; dgrad: Cin' 24, Cout' 40 (wide)", abi=0),
    "m0-cin3-off-thin-in-narrow": _c("direct", 0, 2, 3, 24, 5, 21, "W % 32 != 0: Cin 3 on the generic kernel's scalar halo path, 32-wide; dgrad Cout' 3", abi=0),
    "m0-cin3-off-thin-in-wide": _c("direct", 0, 2, 3, 160, 5, 21, "the same, 128-wide", abi=0),
    "m0-cout2-off-thin-out": _c("direct", 0, 2, 40, 2, 9, 33, "Cout 2 with Cin != 128: thin output on the generic 32-wide kernel; dgrad Cin' 2 (scalar halo path)", abi=0),
    "m1-wide": _c("direct", 1, 2, 20, 160, 22, 36, "v2<1,8> 128-wide, Ho x Wo 11 x 18: pad row and column inside a ragged tile, KC 8 with a padded last chunk; dgrad v2<3,32> 32-wide (Cout' 20)", abi=1),
    "m1-narrow": _c("direct", 1, 2, 20, 24, 22, 36, "v2<1,8> 32-wide; dgrad v2<3,32> 32-wide, Cin' 24", abi=1),
    "m1-cin160": _c("direct", 1, 2, 160, 20, 22, 36, "v2<1,8> 32-wide, 20 chunks; dgrad v2<3,32> 128-wide (Cout' 160), ragged", abi=1),
    "m2-wide": _c("direct", 2, 2, 40, 160, 5, 9, "v2<2,32> 128-wide dense Upsample conv, 10 x 18 output; dgrad = mode 0 at 10 x 18", abi=2),
    "m2-narrow": _c("direct", 2, 2, 40, 24, 5, 9, "v2<2,32> 32-wide", abi=2),
    "m5-wide": _c("direct", 2, 2, 40, 160, 11, 21, "v2<5,32> 128-wide, four parity classes ragged; dgrad v2<6,8> 128-wide (Cout' 40)", abi=5),
    "m5-narrow": _c("direct", 2, 2, 40, 24, 11, 21, "v2<5,32> 32-wide; dgrad v2<6,8> 128-wide, Cin' 24", abi=5),
    "m5-cin24": _c("direct", 2, 2, 24, 40, 11, 21, "v2<5,32> 128-wide; dgrad v2<6,8> 32-wide (Cout' 24), Cin' 40 = five chunks of 8", abi=5),
}
# thin input: Cin 3, W % 32 == 0 -> conv3x3_thin_in_kernel (at most 1024 blocks of 4 waves: the tile loop wraps past 4096 tiles)
THIN_IN_CASES = {
    "thin-in-5x32": _c("thin_in", 0, 3, 3, 160, 5, 32, "15 tiles, two co blocks (the second 32 of 128 wide)", abi=0),
    "thin-in-3x64": _c("thin_in", 0, 3, 3, 160, 3, 64, "18 tiles, two segments per row", abi=0),
    "thin-in-wraps": _c("thin_in", 0, 2, 3, 40, 33, 2048, "4224 tiles over 4096 waves: waves 0 .. 127 run a second pass", abi=0),
}
# thin output: Cin 128, Cout <= 3, no residual, no activation -> conv3x3_thin_out_kernel<128>
THIN_OUT_CASES = {
    "thin-out-c%d-%dx%d" % (co, h, w): _c("thin_out", 0, 2, 128, co, h, w,
                                          "%s; dgrad: %s" % ({(8, 32): "one whole 8 x 32 tile", (9, 33): "four tiles, ragged by one row and one column",
                                                              (3, 5): "one ragged tile"}[(h, w)],
                                                             "thin-in kernel (Cin' 3, W 32)" if (co, w) == (3, 32) else "generic 128-wide, scalar halo path"), abi=0)
    for co in (1, 2, 3) for (h, w) in ((8, 32), (9, 33), (3, 5))
}
# F(2x2): odvae_conv3x3_wino_f32.  n=None: from persistent_n at the device's CU count
WINO2_CASES = {
    "w2-4wave": _c("wino2", 0, 2, 36, 72, 10, 18, "conv3x3_wino_kernel (Cout % 128 != 0): Cin padded to 48, Cout to 128, ragged tiles; dgrad 4-wave, Cin' 72"),
    "w2-8wave-6x10": _c("wino2", 0, 2, 20, 128, 6, 10, "conv3x3_wino8_kernel<false>, one ragged tile per image, Cin padded to 32; dgrad 4-wave"),
    "w2-8wave-20x12": _c("wino2", 0, 1, 20, 128, 20, 12, "conv3x3_wino8_kernel<false>, three tiles, ragged on both axes; dgrad 4-wave"),
    "w2-8wave-persistent": _c("wino2", 0, None, 64, 512, 8, 24, "conv3x3_wino8_kernel<true>: four co blocks, four chunks, two tiles per image (one ragged), uneven tiles per block; dgrad 4-wave, 32 chunks",
                              persistent=True),
}
# F(4x4) on the host-made pack.  groups: the statistics launch (gn_groups); keep: share of the weights kept (None: all)
WINO4_CASES = {
    "w4-16x32": _c("wino4", 0, 2, 64, 64, 16, 32, "conv3x3_wino4_kernel<EPI_NONE,false>: one whole tile per image"),
    "w4-20x36-ragged": _c("wino4", 0, 2, 72, 88, 20, 36, "four tiles per image, ragged on both axes, Cout 88 = 64 + 24, nine chunks; dgrad Cin' 88"),
    "w4-persistent": _c("wino4", 0, None, 64, 512, 16, 36, "persistent: eight co blocks, two tiles per image (one ragged), uneven tiles per block; dgrad: 64 chunks, one tile per block",
                        persistent=True),
}
WINO4_STATS_CASES = {
    "w4-stats-cpg2": _c("wino4_stats", 0, 2, 64, 64, 16, 32, "conv3x3_wino4_kernel<EPI_STATS,false>, 2 channels per group", groups=32, keep=8),
    "w4-stats-cpg4": _c("wino4_stats", 0, 2, 64, 128, 16, 32, "4 channels per group, two co blocks", groups=32, keep=8),
    "w4-stats-ragged": _c("wino4_stats", 0, 2, 72, 64, 20, 36, "ragged tiles: partial sums over the pixels inside the image only", groups=32, keep=8),
    "w4-stats-persistent": _c("wino4_stats", 0, None, 64, 512, 16, 36, "persistent, 16 channels per group", groups=32, keep=2, persistent=True),
}
# the Upsample form: h, w the LOW-resolution input
WINO4_UP_CASES = {
    "w4-up-8x16": _c("wino4_up", 2, 2, 64, 64, 8, 16, "conv3x3_wino4_kernel<EPI_NONE,true> / <EPI_STATS,true>: one whole 16 x 32 tile", groups=32, keep=8),
    "w4-up-10x18": _c("wino4_up", 2, 2, 64, 64, 10, 18, "20 x 36 output: ragged, halo rows and columns of x read twice", groups=32, keep=8),
}
WINO4_POOL_CASES = {
    "w4-pool-20x36": _c("wino4_pool", 2, 2, 64, 72, 10, 18, "conv3x3_wino4_kernel<EPI_POOL,false>: dy 20 x 36 -> dx 10 x 18, Cin' 72, ragged"),
}
WINO4_GNBWD_CASES = {
    "w4-gnbwd-20x36": _c("wino4_gnbwd", 0, 2, 64, 72, 20, 36, "conv3x3_wino4_kernel<EPI_GNBWD,false>: da 20 x 36 of 64 channels in 32 groups, Cin' 72", groups=32),
}
CASES = {}
for _t in (DIRECT_CASES, THIN_IN_CASES, THIN_OUT_CASES, WINO2_CASES, WINO4_CASES, WINO4_STATS_CASES, WINO4_UP_CASES, WINO4_POOL_CASES,
           WINO4_GNBWD_CASES):
    CASES.update(_t)
# random-normal operands, one per kernel kind
PRECISION_CASES = ["m0-wide-ragged", "m0-narrow-ragged", "m1-wide", "m1-cin160", "m2-wide", "m5-wide", "m5-cin24", "thin-in-5x32",
                   "thin-out-c3-9x33", "w2-4wave", "w2-8wave-20x12", "w4-20x36-ragged"]
REFERENCE_CUS = 256     # MI355X


def case_seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % (2 ** 31 - 1)


def case_n(case, cus=REFERENCE_CUS):
    """N of a case; the persistent cases take the smallest N that gives a persistent, uneven plan at this CU count (None: no such N)"""
    if case["n"] is not None:
        return case["n"]
    m = 2 if case["route"] == "wino2" else 4
    return persistent_n(m, cus, case["hi"], case["wi"], case["cin"], case["cout"])


def _wino_m(route):
    return 2 if route == "wino2" else 4


def make_exact(name, cus=REFERENCE_CUS):
    """Operands of one case: dict x, w, b, res, dy (float64 NCHW), mode, route, units, and the case's own fields."""
    case = CASES[name]
    route, mode = case["route"], case["mode"]
    n = case_n(case, cus)
    assert n is not None, "%s: no persistent plan at %d CUs" % (name, cus)
    seed = case_seed(name) % 1000
    if route in ("direct", "thin_in", "thin_out", "wino2"):
        c = E.make_case("A", mode, n, case["cin"], case["cout"], case["hi"], case["wi"], seed=seed)
    else:
        c = E.make_case("C", mode, n, case["cin"], case["cout"], case["hi"], case["wi"], seed=seed)
        g = torch.Generator().manual_seed(case_seed(name))
        m = torch.randint(-1, 2, c["w"].shape, generator=g).double()
        if case.get("keep"):
            m = m * (torch.rand(m.shape, generator=g) < float(case["keep"]) / case["cin"])
        c["w"] = m * W4_SCALE
        c["units"] = dict(c["units"], w=W4_UNIT)
    c.update(case)
    c["n"], c["name"] = n, name
    return c


def make_normal(name, cus=REFERENCE_CUS):
    """f32-representable standard-normal operands of the case's shape (weights scaled by 1 / sqrt(9 Cin)), as float64"""
    case = CASES[name]
    n = case_n(case, cus)
    g = torch.Generator().manual_seed(case_seed(name) + 1)
    ho, wo = out_hw(case["mode"], case["hi"], case["wi"])
    cin, cout = case["cin"], case["cout"]
    c = dict(case)
    c["x"] = torch.randn(n, cin, case["hi"], case["wi"], generator=g).double()
    c["w"] = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).double()
    c["b"] = torch.randn(cout, generator=g).double()
    c["res"] = torch.randn(n, cout, ho, wo, generator=g).double()
    c["dy"] = torch.randn(n, cout, ho, wo, generator=g).double()
    c["n"], c["name"] = n, name
    return c


# ------------------------------------------------------------------------------------------------------------------------------
# the precondition
# ------------------------------------------------------------------------------------------------------------------------------
def _assert_multiples(c):
    for name in ("x", "w", "dy", "res", "b"):
        t = c[name]
        if t is None:
            continue
        assert torch.equal(t.float().double(), t), "%s is not made of f32 numbers" % name
        u = c["units"][name]
        assert torch.equal(torch.round(t / u) * u, t), "%s is not made of multiples of %g" % (name, u)


def summability(c, route=None):
    """Per kind of sum the kernels of the route form: the largest sum of |terms| in units of that sum."""
    route = route or c["route"]
    mode, x, w, dy = c["mode"], c["x"], c["w"], c["dy"]
    u = c["units"]
    uy = min(u["x"] * u["w"], u["b"], u["res"])
    extra = c["b"].abs().view(1, -1, 1, 1) + c["res"].abs()
    out = {}
    if route in ("direct", "thin_in", "thin_out"):
        out["forward"] = (conv_ref(mode, x.abs(), w.abs()) + extra).max().item() / uy
        full = dgrad_full_ref(mode, dy.abs(), w.abs(), x.shape)
        out["dgrad"] = full.max().item() / (u["dy"] * u["w"])
        if mode == 2:       # mode 6 sums all sixteen taps of a low-resolution pixel; up_dense sum-pools the full-resolution gradient
            out["dgrad_pool"] = pool2x2(full).max().item() / (u["dy"] * u["w"])
        return out
    m = _wino_m(route)
    uU = u["w"] / 4.0 if m == 2 else u["w"]         # F(2x2): G has halves, so U has quarters of w's unit; F(4x4): w's unit is U's already
    xin = upsample2x(x) if mode == 2 else x
    uyw = min(u["x"] * uU, u["b"], u["res"])
    mac, outb = winograd_bounds(xin, w, m, extra=extra)
    out["forward_mac"] = mac / (u["x"] * uU)
    out["forward_out"] = outb / uyw
    mac, outb = winograd_bounds(dy, flipped(w), m)
    out["dgrad_mac"] = mac / (u["dy"] * uU)
    out["dgrad_out"] = outb / (u["dy"] * uU)
    if route in ("wino4_pool", "wino4_up"):
        out["dgrad_pool"] = winograd_bounds(dy, flipped(w), m, pooled=True)[1] / (u["dy"] * uU)
    if c.get("groups") and route in ("wino4_stats", "wino4_up"):
        # y = (9 k + 8 j) / 16 (w = 9 m / 16, bias and residual in halves): its own grid is 1/16, far coarser than the 2^-10 of the
        # transforms.  y * y and every partial sum of the squares are whole multiples of 1/256; the squares are non-negative, so
        # their total bounds every partial sum.
        y = conv_ref(mode, x, w, c["b"], c["res"])
        assert torch.equal(torch.round(y * 16.0) / 16.0, y), "y is not made of multiples of 1/16"
        sums = tile_group_sums(y, c["groups"], WINO_TILE[4])
        out["stats_sum"] = tile_group_sums(y.abs(), c["groups"], WINO_TILE[4])[..., 0].max().item() * 16.0
        out["stats_sumsq"] = sums[..., 1].max().item() * 256.0
        out["stats_square"] = (y.abs().max().item() * 16.0) ** 2          # one product y * y, in units of 1/256
    return out


def assert_exactly_summable(c, route=None):
    """The condition under which equality is the right assertion, on the very tensors a test uses: every operand is made of f32
    numbers and of whole multiples of its unit; every kind of sum the route's kernels form has its sum of |terms| below 2^24 units.
    For the F(4x4) routes also: U = G g G^T is dyadic (24 G is whole, w is a multiple of 576 * 2^-10)."""
    route = route or c["route"]
    _assert_multiples(c)
    if route.startswith("wino4"):
        mm = c["w"] / W4_SCALE
        assert torch.equal(torch.round(mm), mm), "F(4x4) weights are not of the form 576 m 2^-10"
        U = winograd_U(c["w"], 4)
        assert torch.equal(torch.round(U / W4_UNIT) * W4_UNIT, U) and torch.equal(U.float().double(), U), "U is not dyadic in f32"
    s = summability(c, route)
    for kind, units in s.items():
        assert units < LIMIT, "%s: %s: sum of |terms| is %.4g units, not below 2^24 = %.4g: f32 operations may round" % (c.get("name"), kind, units, LIMIT)
    return s
