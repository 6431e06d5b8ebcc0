"""Inputs, float64 reference and cases for the direct 3x3 weight-gradient kernels (csrc/conv3x3_wgrad_f32.hip), for
tests/test_wgrad_direct_inputs.py (host) and tests/test_wgrad_direct_exact_gpu.py.  Plain module: no fixtures, no device.

The kernels multiply in plain f32 on the matrix cores and add f32 partial sums: per tile, per split of the pixel range, then over the
splits' slabs.  On operands that are small whole numbers every product is a whole number, and as long as the sum of |x| |dy| over all
pixels of a (ci, co, tap) stays below 2^24 every partial sum of every subset of the terms, in any order, is a whole number below 2^24
and therefore exact in f32.  The device result must then equal the float64 gradient bit for bit: no tolerance.  `make_exact` makes such
operands and asserts the condition on them; `wgrad_f64` is the float64 gradient as nine [Cout x pixels] . [pixels x Cin] products;
`CASES` names the shapes, one per path of the kernels that one pixel tile per block never reaches, with the properties of the launch
plan (`odvae_conv3x3_wgrad_plan`) each case exists for.  All tensors are NCHW on the host.

    mode 0  stride 1, pad 1           mode 1  pad (0, 1, 0, 1), stride 2           mode 2  nearest 2x, then stride 1, pad 1
    mode 5  mode 2's mathematics, accumulated by output parity class (falls back to the dense form of mode 2 when a channel count is
            no multiple of 4)
"""
import torch
import torch.nn.functional as F

EXACT_LIMIT = float(2 ** 24)
MAGNITUDE = 7                   # operands are drawn from +-1 ... +-7: dense, never zero


def out_hw(mode, hi, wi):
    if mode == 0:
        return hi, wi
    if mode == 1:
        assert hi % 2 == 0 and wi % 2 == 0
        return hi // 2, wi // 2
    assert mode in (2, 5), mode
    return 2 * hi, 2 * wi


def small_integers(shape, generator):
    """float64 whole numbers from +-1 ... +-MAGNITUDE, every magnitude and both signs equally likely"""
    mag = torch.randint(1, MAGNITUDE + 1, shape, generator=generator)
    sign = 2 * torch.randint(0, 2, shape, generator=generator) - 1
    return (mag * sign).double()


def exact_bound(x, dy):
    """An upper bound of sum over pixels |xs| |dy| of the worst (ci, co, tap): every output pixel meets at most one input value per tap,
    so the sum is at most max |x| times the largest per-channel sum of |dy| (which also bounds the bias gradient's terms)."""
    return x.abs().max().item() * dy.abs().sum(dim=(0, 2, 3)).max().item()


def make_exact(mode, n, cin, cout, hi, wi, seed):
    """(x [n][cin][hi][wi], dy [n][cout][ho][wo]) float64 whole numbers on which the weight gradient is exact in f32 in any order"""
    ho, wo = out_hw(mode, hi, wi)
    g = torch.Generator().manual_seed(seed)
    x = small_integers((n, cin, hi, wi), g)
    dy = small_integers((n, cout, ho, wo), g)
    assert (x != 0).all() and (dy != 0).all()
    assert exact_bound(x, dy) < EXACT_LIMIT, "sum |x| |dy| of one output element can reach %g >= 2^24" % exact_bound(x, dy)
    return x, dy


def make_normal(mode, n, cin, cout, hi, wi, seed):
    """(x, dy) f32 standard normal, for the precision figures"""
    ho, wo = out_hw(mode, hi, wi)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, cin, hi, wi, generator=g), torch.randn(n, cout, ho, wo, generator=g)


def conv_input(mode, x):
    """(the padded / upsampled tensor the conv's taps slide over, stride)"""
    if mode == 0:
        return F.pad(x, (1, 1, 1, 1)), 1
    if mode == 1:
        return F.pad(x, (0, 1, 0, 1)), 2
    assert mode in (2, 5), mode
    return F.pad(x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3), (1, 1, 1, 1)), 1


def wgrad_f64(mode, x, dy):
    """(dw [cout][cin][3][3], db [cout]) in float64: dw[:, :, kh, kw] = dy [cout x pixels] . xs(kh, kw) [pixels x cin], xs the input
    value each output pixel's tap (kh, kw) reads -- nine products, no autograd"""
    x, dy = x.double(), dy.double()
    n, cout, ho, wo = dy.shape
    cin = x.shape[1]
    assert (ho, wo) == out_hw(mode, x.shape[2], x.shape[3]), "dy is not the output gradient of a mode %d conv of x" % mode
    xin, s = conv_input(mode, x)
    dym = dy.permute(1, 0, 2, 3).reshape(cout, -1)
    dw = torch.empty(cout, cin, 3, 3, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            xs = xin[:, :, kh:kh + s * (ho - 1) + 1:s, kw:kw + s * (wo - 1) + 1:s]
            dw[:, :, kh, kw] = dym @ xs.permute(0, 2, 3, 1).reshape(-1, cin)
    return dw, dy.sum(dim=(0, 2, 3))


# ------------------------------------------------------------------------------------------------------------------------------
# cases: name -> (mode passed to the C ABI, n, cin, cout, INPUT hi, wi, expectation).  The expectation holds properties of the plan
# the library reports (tests/test_wgrad_direct_inputs.py asserts them, so a retuned block budget makes a stale case fail there):
#   kind, effective_mode, ntiles, nsplit, tiles_per_split   equal to the plan's fields
#   last            tiles of the last split
#   crosses_images  some split's tile range holds tiles of two images
# thin:  blocks, waves, groups equal to the plan's; rows_per_wave_max = ceil(rows / waves); Cs = the thin side's channel count
# ------------------------------------------------------------------------------------------------------------------------------
CASES = {
    # v2 (LDS-DMA): 452 -> 324 is ragged on both channel axes (8 ci tiles of 64, 3 co tiles of 128)
    "v2-m0-3-per-block": (0, 2, 452, 324, 26, 24, dict(kind="v2", effective_mode=0, ntiles=28, nsplit=10, tiles_per_split=3, last=1, crosses_images=True)),
    "v2-m1-3-per-block": (1, 3, 452, 324, 12, 80, dict(kind="v2", effective_mode=1, ntiles=27, nsplit=9, tiles_per_split=3, last=3)),
    "v2-m2-3-per-block": (2, 3, 452, 324, 6, 20, dict(kind="v2", effective_mode=2, ntiles=27, nsplit=9, tiles_per_split=3, last=3)),
    "v2-m0-2-per-block": (0, 1, 512, 512, 20, 32, dict(kind="v2", effective_mode=0, ntiles=10, nsplit=5, tiles_per_split=2, last=2)),
    # v1: channel counts that are no multiples of 4 ...
    "v1-m0-short-last": (0, 3, 510, 510, 24, 40, dict(kind="v1", effective_mode=0, ntiles=27, nsplit=14, tiles_per_split=2, last=1, crosses_images=True)),
    "v1-m1": (1, 3, 510, 510, 24, 80, dict(kind="v1", effective_mode=1, ntiles=27, nsplit=14, tiles_per_split=2, last=1, crosses_images=True)),
    "v1-m5-falls-back-to-m2": (5, 3, 510, 510, 12, 20, dict(kind="v1", effective_mode=2, ntiles=27, nsplit=14, tiles_per_split=2, last=1, crosses_images=True)),
    # ... and multiples of 4 with Cout <= 64 (the other arm of the v2 condition); 129 tiles are the fewest with two per block
    "v1-m0-narrow-cout": (0, 3, 512, 64, 33, 129, dict(kind="v1", effective_mode=0, ntiles=135, nsplit=68, tiles_per_split=2, last=1, crosses_images=True)),
    # up (parity classes)
    "up-5-per-block": (5, 3, 452, 324, 6, 36, dict(kind="up", effective_mode=5, ntiles=27, nsplit=6, tiles_per_split=5, last=2, crosses_images=True)),
    "up-3-per-block": (5, 1, 512, 512, 10, 32, dict(kind="up", effective_mode=5, ntiles=10, nsplit=4, tiles_per_split=3, last=1)),
    # thin, several rows per wave: 825 rows over 816 waves, five channel groups, the last eight channels wide; waves 0 .. 8 own a row of
    # image 0 and one of image 2.  W = 16 is the single-chunk row, W = 48 has three chunks.
    "thin-in-2-rows-w16": (0, 3, 3, 520, 275, 16, dict(kind="thin", Cs=3, blocks=204, waves=816, groups=5, rows_per_wave_max=2)),
    "thin-out-2-rows-w48": (0, 3, 520, 2, 275, 48, dict(kind="thin", Cs=2, blocks=204, waves=816, groups=5, rows_per_wave_max=2)),
    # thin, few rows and many channels: fewer than 32 blocks, fewer slabs than the reduction has parts
    "thin-in-few-rows": (0, 2, 1, 160, 5, 16, dict(kind="thin", Cs=1, blocks=3, waves=12, groups=2, rows_per_wave_max=1)),
    "thin-out-few-rows": (0, 2, 160, 3, 5, 32, dict(kind="thin", Cs=3, blocks=3, waves=12, groups=2, rows_per_wave_max=1)),
    # thin, 140 slabs: one trip of the reduction's eight-wide loop, then its tail
    "thin-in-140-slabs": (0, 2, 2, 36, 70, 16, dict(kind="thin", Cs=2, blocks=35, waves=140, groups=1, rows_per_wave_max=1)),
    "thin-out-140-slabs": (0, 2, 36, 1, 70, 32, dict(kind="thin", Cs=1, blocks=35, waves=140, groups=1, rows_per_wave_max=1)),
}
KINDS = ("thin", "v1", "v2", "up")
# one multi-tile case per kind for the random-normal precision figures and for the argument contract
PRECISION_CASES = {"thin": "thin-in-2-rows-w16", "v1": "v1-m0-short-last", "v2": "v2-m0-3-per-block", "up": "up-5-per-block"}


def case_seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % (2 ** 31 - 1)


def split_ranges(plan):
    """[(first tile, one past the last)] of every split of a tiled plan"""
    tps = plan["tiles_per_split"]
    return [(s * tps, min(plan["ntiles"], (s + 1) * tps)) for s in range(plan["nsplit"])]


def plan_properties(plan, n, hi):
    """The properties an expectation may name, derived from a reported plan (a dict with the C ABI's field names, kind by name)."""
    if plan["kind"] == "thin":
        rows, waves = n * hi, plan["nsplit"]
        return dict(kind="thin", blocks=plan["ntiles"], waves=waves, groups=plan["tiles_per_split"], rows_per_wave_max=-(-rows // waves))
    ranges = split_ranges(plan)
    per_image = plan["ntiles"] // n
    return dict(kind=plan["kind"], effective_mode=plan["effective_mode"], ntiles=plan["ntiles"], nsplit=plan["nsplit"],
                tiles_per_split=plan["tiles_per_split"], last=ranges[-1][1] - ranges[-1][0],
                crosses_images=any(a // per_image != (b - 1) // per_image for a, b in ranges))
