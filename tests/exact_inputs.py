"""Exactly summable inputs for the bf16 convolution kernels: generators, float64 references, the bit-for-bit checker.

The bf16 kernels multiply bf16 numbers (exact in f32) and add in f32 only, with one rounding at the store.  If every partial sum a
kernel could form -- in any order -- is an integer multiple of one unit 2^-s and smaller than 2^24 units, no f32 addition rounds: an
f32 output must EQUAL the float64 reference, a bf16 output must equal the reference rounded once to nearest-even.  This module makes
such operands (recipes A-D), asserts the condition on the very tensors a test uses (`assert_exactly_summable`), builds references that
follow the rounding chain of `ops._ConvB`, and compares raw bits (`assert_bits_equal`).

recipe  operands                                                                                   forward unit
  A     x, dy integers in [-4, 4]; w multiples of 1/4 in [-2, 2]; bias multiples of 1/8 in [-2, 2];  2^-3   "deep": any Cin
        residual integers in [-8, 8]
  B     x odd integers |x| <= 255; w = k 2^-7, |k| <= 255 (all 8 significand bits of both in use);  2^-7   K = taps * Cin <= 258
        dy odd integers up to the largest of 255, 63, 15, 3 that keeps dx and dw summable
  C     x in {-1, 0, 1}; w in {-1/2, 0, 1/2}; bias multiples of 1/2 in [-1, 1]; residual multiples  2^-2   sums of y and y^2 per tile
        of 1/2 in [-2, 2]                                                                                  and group exact too
  D     x, dy integers in [-2, 2]; w multiples of 1/4 in [-2, 2]; bias multiples of 1/8              2^-3   dw over 2^21 pixels
Plain module: no fixtures, no device.  All tensors are float64 NCHW on the host.
"""
import torch
import torch.nn.functional as F

BF = torch.bfloat16
LIMIT = float(2 ** 24)      # an f32 holds every integer multiple of its unit below 2^24 units
RNE_GROWTH = 1.0 + 2.0 ** -8     # one rounding to bf16 moves a value by at most half an ulp <= 2^-8 of its magnitude
TILE = (8, 16)              # output tile of conv_bf16_kernel (rows, columns)


# ------------------------------------------------------------------------------------------------------------------------------
# generators
# ------------------------------------------------------------------------------------------------------------------------------
def out_hw(mode, h, w):
    if mode == 1:
        return h // 2, w // 2
    if mode == 2:
        return 2 * h, 2 * w
    return h, w


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _odd(g, shape, amax):
    """odd integers with |v| <= amax, both signs"""
    mag = 2 * torch.randint(0, (amax + 1) // 2, shape, generator=g) + 1
    sign = 2 * torch.randint(0, 2, shape, generator=g) - 1
    return (mag * sign).double()


def make_case(recipe, mode, n, cin, cout, h, w, bias=True, residual=True, seed=0, cx=None):
    """Operands of one conv case: dict x [n, cx or cin, h, w], w [cout, cin, k, k], b [cout] | None, res | None, dy, mode, units.
    cx > cin: the input carries zero channels beyond the weight's (the 3-channel image padded to 8).
    Recipe C past 8 input channels keeps 8 / cin of the weights (at random, so every channel stays live somewhere): the worst-case
    sum of y^2 over a tile and group must stay under 2^24 units."""
    g = torch.Generator().manual_seed(100003 * seed + 7919 * mode + 131 * cin + 17 * cout + 3 * h + w)
    k = 1 if mode == 4 else 3
    ho, wo = out_hw(mode, h, w)
    c = {"mode": mode, "recipe": recipe}
    if recipe in ("A", "D"):
        a = 4 if recipe == "A" else 2
        c["x"], c["dy"] = _ints(g, (n, cin, h, w), -a, a), _ints(g, (n, cout, ho, wo), -a, a)
        c["w"] = _ints(g, (cout, cin, k, k), -8, 8) / 4
        c["b"] = _ints(g, (cout,), -16, 16) / 8 if bias else None
        c["res"] = _ints(g, (n, cout, ho, wo), -8, 8) if residual else None
        c["units"] = {"x": 1.0, "w": 0.25, "dy": 1.0, "b": 0.125, "res": 1.0}
    elif recipe == "B":
        c["x"] = _odd(g, (n, cin, h, w), 255)
        c["w"] = _odd(g, (cout, cin, k, k), 255) / 128
        c["b"] = _ints(g, (cout,), -16, 16) / 8 if bias else None
        c["res"] = _ints(g, (n, cout, ho, wo), -8, 8) if residual else None
        c["units"] = {"x": 1.0, "w": 2.0 ** -7, "dy": 1.0, "b": 2.0 ** -3, "res": 1.0}
        seed_dy = int(torch.randint(0, 2 ** 31 - 1, (1,), generator=g).item())
        for amax in (255, 63, 15, 3):       # the widest upstream gradient that keeps dx and dw under 2^24 units (bounds from operands alone)
            c["dy"] = _odd(torch.Generator().manual_seed(seed_dy + amax), (n, cout, ho, wo), amax)
            s = summability(c)
            if max(s["dgrad"], s.get("dgrad_pool", 0.0), s["wgrad"]) < LIMIT:
                break
    elif recipe == "C":
        c["x"], c["dy"] = _ints(g, (n, cin, h, w), -1, 1), _ints(g, (n, cout, ho, wo), -1, 1)
        c["w"] = _ints(g, (cout, cin, k, k), -1, 1) / 2
        if cin > 8:
            c["w"] = c["w"] * (torch.rand(c["w"].shape, generator=g) < 8.0 / cin)
        c["b"] = _ints(g, (cout,), -2, 2) / 2 if bias else None
        c["res"] = _ints(g, (n, cout, ho, wo), -4, 4) / 2 if residual else None
        c["units"] = {"x": 1.0, "w": 0.5, "dy": 1.0, "b": 0.5, "res": 0.5}
    else:
        raise ValueError("recipe %r" % (recipe,))
    if cx is not None and cx != cin:
        c["x"] = torch.cat([c["x"], torch.zeros(n, cx - cin, h, w, dtype=torch.float64)], 1)
    return c


def f32_gradient(shape, seed=5):
    """(dy, unit): an f32 upstream gradient that is no bf16 tensor -- multiples of 2^-10 in [-4, 4], 13 significant bits"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4096, 4097, tuple(shape), generator=g).double() / 1024, 2.0 ** -10


# ------------------------------------------------------------------------------------------------------------------------------
# the float64 mathematics
# ------------------------------------------------------------------------------------------------------------------------------
def conv_f64(mode, x, w, b=None):
    if mode == 0:
        return F.conv2d(x, w, b, padding=1)
    if mode == 1:
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)
    if mode == 2:
        return F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, padding=1)
    return F.conv2d(x, w, b)


def dgrad_f64(mode, dy, w, x_shape):
    """d conv / d x applied to dy; for mode 2 the gradient w.r.t. the UPSAMPLED image [N, Cin, 2H, 2W]"""
    n, c, h, wd = x_shape
    shape = (n, c, 2 * h, 2 * wd) if mode == 2 else tuple(x_shape)
    x = torch.zeros(shape, dtype=dy.dtype, requires_grad=True)
    y = conv_f64(0 if mode == 2 else mode, x, w)
    return torch.autograd.grad(y, x, dy)[0]


def wgrad_f64(mode, x, dy, w_shape):
    w = torch.zeros(w_shape, dtype=x.dtype, requires_grad=True)
    return torch.autograd.grad(conv_f64(mode, x, w), w, dy)[0]


def pool2x2(t):
    return t[:, :, 0::2, 0::2] + t[:, :, 0::2, 1::2] + t[:, :, 1::2, 0::2] + t[:, :, 1::2, 1::2]


def rne(t):
    """float64 -> bf16, one rounding to nearest-even (the f32 stop in between is exact for every value these recipes produce)"""
    return t.float().to(BF)


def tile_group_sums(y, groups, tile=TILE):
    """[N][tiles][groups][2] = (sum, sum of squares) of y [N, C, H, W] over each output tile and channel group (float64)"""
    n, c, h, w = y.shape
    th, tw = tile
    ty, tx = -(-h // th), -(-w // tw)
    yp = F.pad(y, (0, tx * tw - w, 0, ty * th - h)).reshape(n, groups, c // groups, ty, th, tx, tw)
    s = yp.sum((2, 4, 6)).permute(0, 2, 3, 1).reshape(n, ty * tx, groups)
    q = (yp * yp).sum((2, 4, 6)).permute(0, 2, 3, 1).reshape(n, ty * tx, groups)
    return torch.stack([s, q], -1)


# ------------------------------------------------------------------------------------------------------------------------------
# the precondition
# ------------------------------------------------------------------------------------------------------------------------------
def forward_unit(c):
    """the unit every partial sum of conv + bias + residual is a multiple of"""
    u = c["units"]
    return min(u["x"] * u["w"], u["b"] if c["b"] is not None else 1e300, u["res"] if c["res"] is not None else 1e300)


def summability(c, dy_f32=None, dy_f32_unit=None, stats_groups=None):
    """Per kind of sum the kernels form: the sum of |terms| in units, from the float64 operands and the recipe's declared units alone.
    `worst` is the largest.  dy_f32: an f32 upstream gradient (its bf16 cast feeds the products, its own values the bias gradient)."""
    mode, x, w = c["mode"], c["x"], c["w"]
    u = c["units"]
    cin = w.shape[1]
    xa = x[:, :cin].abs()
    dy = rne(dy_f32).double() if dy_f32 is not None else c["dy"]
    udy = dy_f32_unit if dy_f32 is not None else u["dy"]     # rounding to bf16 only coarsens: rne(dy_f32) stays a multiple of the f32 unit
    out = {}
    fwd = conv_f64(mode, xa, w.abs(), c["b"].abs() if c["b"] is not None else None)
    if c["res"] is not None:
        fwd = fwd + c["res"].abs()
    uy = forward_unit(c)
    out["forward"] = fwd.max().item() / uy
    du = dgrad_f64(mode, dy.abs(), w.abs(), xa.shape)
    out["dgrad"] = du.max().item() / (udy * u["w"])
    if mode == 2:       # second stage: 2x2 sums of the ROUNDED du (rounding keeps multiples of the unit, and |rne(v)| <= (1 + 2^-8) |v|)
        out["dgrad_pool"] = RNE_GROWTH * pool2x2(du).max().item() / (udy * u["w"])
    out["wgrad"] = wgrad_f64(mode, xa, dy.abs(), w.shape).max().item() / (u["x"] * udy)
    out["bgrad"] = (dy_f32 if dy_f32 is not None else dy).abs().sum((0, 2, 3)).max().item() / udy
    if stats_groups:
        sums = tile_group_sums(RNE_GROWTH * fwd, stats_groups)       # |rne(y)| <= (1 + 2^-8) (conv(|x|, |w|) + |b| + |res|)
        out["stats_sum"] = sums[..., 0].max().item() / uy
        out["stats_sumsq"] = sums[..., 1].max().item() / (uy * uy)
    out["worst"] = max(out.values())
    return out


def assert_exactly_summable(c, dy_f32=None, dy_f32_unit=None, stats_groups=None):
    """The condition under which equality is the right assertion.  (1) every operand the kernels read as bf16 survives .to(bfloat16)
    unchanged (the bias and an f32 upstream gradient stay f32: they must survive .float()) and is made of whole multiples of its
    recipe's unit; (2) for every kind of sum, the sum of |terms| is below 2^24 units."""
    for name in ("x", "w", "dy", "res", "b"):
        t = c[name]
        if t is None:
            continue
        if name == "b":
            assert torch.equal(t.float().double(), t), "bias is not made of f32 numbers"
        else:
            assert torch.equal(t.float().to(BF).double(), t), "%s is not made of bf16 numbers" % name
        assert torch.equal(torch.round(t / c["units"][name]) * c["units"][name], t), "%s is not made of multiples of %g" % (name, c["units"][name])
    if dy_f32 is not None:
        assert torch.equal(dy_f32.float().double(), dy_f32), "f32 upstream gradient is not made of f32 numbers"
        assert torch.equal(torch.round(dy_f32 / dy_f32_unit) * dy_f32_unit, dy_f32), "f32 upstream gradient: not multiples of %g" % dy_f32_unit
    s = summability(c, dy_f32, dy_f32_unit, stats_groups)
    for kind, units in s.items():
        assert units < LIMIT, "%s: sum of |terms| is %.4g units, not below 2^24 = %.4g: f32 additions may round" % (kind, units, LIMIT)
    return s


# ------------------------------------------------------------------------------------------------------------------------------
# references that follow the rounding chain of ops._ConvB
# ------------------------------------------------------------------------------------------------------------------------------
def references(c, out_f32=False, dy_f32=None, stats_groups=None):
    """What ops._ConvB must produce for case c, bit for bit.
    y: conv + bias + residual, one rounding (none with out_f32).  dx: one rounding (modes 0, 1, 4); mode 2: du = rne(dgrad at
    2H x 2W), dx = rne(2x2 sums of du).  dy_f32: the f32 upstream gradient -- the products see rne(dy_f32) (cast_pad_bf16), the bias
    gradient sums the f32 values themselves.  dw, db: f32, no rounding.  dres: dy as the kernels see it."""
    mode, x, w = c["mode"], c["x"], c["w"]
    cin = w.shape[1]
    xw = x[:, :cin]
    y = conv_f64(mode, xw, w, c["b"])
    if c["res"] is not None:
        y = y + c["res"]
    dyb = rne(dy_f32).double() if dy_f32 is not None else c["dy"]
    du = dgrad_f64(mode, dyb, w, xw.shape)
    if mode == 2:
        dx = rne(pool2x2(rne(du).double()))
    else:
        dx = rne(du)
    r = {"y": y.float() if out_f32 else rne(y), "dx": dx, "dx_exact": du,
         "dw": wgrad_f64(mode, xw, dyb, w.shape).float(),
         "db": (dy_f32 if dy_f32 is not None else dyb).sum((0, 2, 3)).float(),
         "dres": rne(dyb), "y_exact": y}
    if stats_groups:
        r["partials"] = tile_group_sums(r["y"].double(), stats_groups).float()
    return r


def rounding_profile(exact):
    """share of the elements of a float64 tensor that are no bf16 numbers, and the share that lie exactly half way between two"""
    f = exact.float()
    bits = f.view(torch.int32)
    low = bits & 0xFFFF
    return (low != 0).double().mean().item(), (low == 0x8000).double().mean().item()


# ------------------------------------------------------------------------------------------------------------------------------
# the checker
# ------------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    if t.dtype == BF:
        return t.contiguous().view(torch.int16)
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    raise AssertionError("bit comparison wants bf16 or f32 tensors, got %s" % t.dtype)


def assert_bits_equal(got, want, what, summed=True, tile=TILE):
    """got and want agree in dtype, shape and every bit.  Compared as integers, so a NaN can hide behind neither == nor !=.
    summed=True (outputs that are sums): -0.0 counts as +0.0 on both sides -- the sign of a sum that is exactly zero depends on the
    order and on the start value.  summed=False (casts, packs): raw, the sign of zero included.
    A failure names the count, the first indices and -- for [N, C, H, W] tensors -- where the mismatches lie: image border, tile seam,
    channel tail."""
    assert got.dtype == want.dtype, "%s: dtype %s, expected %s" % (what, got.dtype, want.dtype)
    assert tuple(got.shape) == tuple(want.shape), "%s: shape %s, expected %s" % (what, tuple(got.shape), tuple(want.shape))
    want = want.to(got.device)
    if summed:
        got, want = got + 0.0, want + 0.0        # x + (+0.0) in round-to-nearest: -0.0 -> +0.0, every other value (NaN payloads included) kept
    bad = _bits(got) != _bits(want)
    nbad = int(bad.sum().item())
    if nbad == 0:
        return
    idx = bad.nonzero()
    first = ["(%s): got %r, want %r" % (", ".join(str(int(v)) for v in i), got[tuple(i)].item(), want[tuple(i)].item()) for i in idx[:6]]
    msg = "%s: %d of %d elements differ in bits; first %s" % (what, nbad, bad.numel(), "; ".join(first))
    if got.dim() == 4:
        _, c, h, w = got.shape
        ci, yi, xi = idx[:, 1], idx[:, 2], idx[:, 3]
        border = ((yi == 0) | (yi == h - 1) | (xi == 0) | (xi == w - 1)).sum().item()
        th, tw = tile
        seam = ((yi % th == 0) | (yi % th == th - 1) | (xi % tw == 0) | (xi % tw == tw - 1)).sum().item()
        tail = (ci >= (c - 1) // 8 * 8).sum().item()
        msg += " | of the mismatches: %d on the image border, %d on a tile seam (y %% %d, x %% %d), %d in the last 8-channel vector" % (
            border, seam, th, tw, tail)
    raise AssertionError(msg)
