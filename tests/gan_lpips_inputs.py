"""Inputs and float64 references for the PatchGAN / LPIPS support kernels (csrc/gan_f32.hip, csrc/lpips_f32.hip).

* index-built references of the data-movement kernels, written from the definitions in the kernels' comments (one strided slice per
  tap of the zero-padded image; col2im as the scatter that is im2col's adjoint, where the kernel gathers): `im2col4x4`, `col2im4x4`,
  `weight_to_gemm` / `weight_from_gemm`;
* an exactly summable recipe for the 4x4 convolution (recipe A of exact_inputs: x, dy integers in [-4, 4], w multiples of 1/4 in
  [-2, 2], bias multiples of 1/8 in [-2, 2]) with its precondition `assert_exactly_summable4x4`: every partial sum of the forward, dx, dw
  and db, formed in any order, is a multiple of one unit and stays below 2^24 units, so no f32 addition rounds and an f32 kernel must
  EQUAL the float64 reference;
* makers of max-pool inputs: ties, all-equal windows, all-negative windows, -inf, NaN.
Plain module: no fixtures, no device.  All tensors live on the host.
"""
import itertools

import torch
import torch.nn.functional as F

LIMIT = float(2 ** 24)      # an f32 holds every integer multiple of its unit below 2^24 units


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31 - 1))


# ------------------------------------------------------------------------------------------------------------------------------
# Conv2d(kernel 4, padding 1, stride 1 | 2): geometry and the data-movement references
# ------------------------------------------------------------------------------------------------------------------------------
def out4x4(h, stride):
    """output extent of kernel 4, padding 1; None where the padded image is smaller than the kernel (torch refuses it)"""
    if h < 2 or stride not in (1, 2):
        return None
    return (h - 2) // stride + 1


def im2col4x4(x, stride):
    """x [N, Hi, Wi, C] -> cols [N*Ho*Wo, 16*C]: cols[(n, oy, ox)][(kh*4 + kw)*C + c] = x[n][oy*S - 1 + kh][ox*S - 1 + kw][c], zero outside"""
    n, hi, wi, c = x.shape
    ho, wo = out4x4(hi, stride), out4x4(wi, stride)
    xp = torch.zeros(n, hi + 2, wi + 2, c, dtype=x.dtype)
    xp[:, 1:hi + 1, 1:wi + 1] = x
    cols = torch.zeros(n, ho, wo, 16, c, dtype=x.dtype)
    for kh, kw in itertools.product(range(4), range(4)):      # padded row of tap kh at output row oy: oy*S + kh
        cols[:, :, :, kh * 4 + kw] = xp[:, kh:kh + stride * (ho - 1) + 1:stride, kw:kw + stride * (wo - 1) + 1:stride]
    return cols.reshape(n * ho * wo, 16 * c)


def col2im4x4(dcols, n, hi, wi, c, stride):
    """the exact adjoint of im2col4x4: every element of dcols is added to the input pixel it was read from (those read from the padding
    are dropped); dcols [N*Ho*Wo, 16*C] -> dx [N, Hi, Wi, C]"""
    ho, wo = out4x4(hi, stride), out4x4(wi, stride)
    d = dcols.reshape(n, ho, wo, 16, c)
    dxp = torch.zeros(n, hi + 2, wi + 2, c, dtype=dcols.dtype)
    for kh, kw in itertools.product(range(4), range(4)):
        dxp[:, kh:kh + stride * (ho - 1) + 1:stride, kw:kw + stride * (wo - 1) + 1:stride] += d[:, :, :, kh * 4 + kw]
    return dxp[:, 1:hi + 1, 1:wi + 1].contiguous()


def weight_to_gemm(w):
    """OIHW [Cout, Cin, 4, 4] -> [Cout, (kh*4 + kw)*Cin + ci]"""
    cout, cin = w.shape[:2]
    return w.permute(0, 2, 3, 1).reshape(cout, 16 * cin).contiguous()


def weight_from_gemm(wg, cin):
    cout = wg.shape[0]
    return wg.reshape(cout, 4, 4, cin).permute(0, 3, 1, 2).contiguous()


# the cases of the data-movement kernels: (stride, (Hi, Wi)) that the geometry allows (Hi, Wi >= 2 is all it asks) x C x N
MOVE_HW = [(2, 2), (3, 5), (4, 4), (8, 8), (9, 7), (17, 33)]
MOVE_C = [1, 3, 4, 64, 130]
MOVE_N = [1, 3]
MOVE_CASES = [(s, hw, c, n) for s in (1, 2) for hw in MOVE_HW if out4x4(hw[0], s) and out4x4(hw[1], s) for c in MOVE_C for n in MOVE_N]
REORDER_CASES = [(1, 1), (4, 3), (64, 3), (1, 512), (130, 66)]


def distinct_integers(shape):
    """1, 2, 3, ... in memory order, as f32 (exact below 2^24): no two elements agree, so a transposed or shifted index cannot cancel"""
    numel = 1
    for v in shape:
        numel *= int(v)
    assert numel < LIMIT
    return torch.arange(1, numel + 1, dtype=torch.float32).reshape(shape)


# ------------------------------------------------------------------------------------------------------------------------------
# the exactly summable 4x4 convolution
# ------------------------------------------------------------------------------------------------------------------------------
UNITS = {"x": 1.0, "w": 0.25, "dy": 1.0, "b": 0.125}
CONV_GEOMETRY = [(2, (9, 7)), (2, (17, 33)), (2, (8, 16)), (1, (4, 4)), (1, (9, 7)), (1, (2, 2))]      # (stride, (Hi, Wi))
CONV_CIN = [3, 64, 72]
CONV_COUT = [1, 4, 64, 130]          # 1: zero-padded to 4 in ops.conv4x4; 130: a multiple of no GEMM tile
CONV_N = [1, 3]
CONV_CASES = [(s, hw, cin, cout, bias, n) for s, hw in CONV_GEOMETRY for cin in CONV_CIN for cout in CONV_COUT for bias in (True, False)
              for n in CONV_N]


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def make_conv_case(stride, hw, cin, cout, bias, n, seed=0):
    """float64 NCHW operands of one case: x, w, b | None, dy, stride"""
    h, w = hw
    g = gen(seed, stride, h, w, cin, cout, int(bias), n)
    ho, wo = out4x4(h, stride), out4x4(w, stride)
    return {"stride": stride, "x": _ints(g, (n, cin, h, w), -4, 4), "w": _ints(g, (cout, cin, 4, 4), -8, 8) / 4,
            "b": _ints(g, (cout,), -16, 16) / 8 if bias else None, "dy": _ints(g, (n, cout, ho, wo), -4, 4)}


def conv_references(c):
    """float64: y, dx, dw, db (None without bias) of F.conv2d(kernel 4, padding 1, the case's stride)"""
    x, w = c["x"].clone().requires_grad_(True), c["w"].clone().requires_grad_(True)
    b = c["b"].clone().requires_grad_(True) if c["b"] is not None else None
    y = F.conv2d(x, w, b, stride=c["stride"], padding=1)
    y.backward(c["dy"])
    return {"y": y.detach(), "dx": x.grad, "dw": w.grad, "db": b.grad if b is not None else None}


def conv_summability(c):
    """per kind of sum: the sum of |terms| in units of that sum, from the operands and the declared units alone"""
    a = {"stride": c["stride"], "x": c["x"].abs(), "w": c["w"].abs(), "b": c["b"].abs() if c["b"] is not None else None, "dy": c["dy"].abs()}
    r = conv_references(a)
    uy = min(UNITS["x"] * UNITS["w"], UNITS["b"]) if c["b"] is not None else UNITS["x"] * UNITS["w"]
    out = {"forward": r["y"].max().item() / uy, "dgrad": r["dx"].max().item() / (UNITS["dy"] * UNITS["w"]),
           "wgrad": r["dw"].max().item() / (UNITS["x"] * UNITS["dy"]), "bgrad": a["dy"].sum((0, 2, 3)).max().item() / UNITS["dy"]}
    out["worst"] = max(out.values())
    return out


def assert_exactly_summable4x4(c):
    """The condition under which equality is the right assertion (exact_inputs.assert_exactly_summable for this convolution):
    (1) every operand is made of f32 numbers and of whole multiples of its unit; (2) for every kind of sum the sum of |terms| is below
    2^24 units."""
    for name in ("x", "w", "dy", "b"):
        t = c[name]
        if t is None:
            continue
        assert torch.equal(t.float().double(), t), "%s is not made of f32 numbers" % name
        assert torch.equal(torch.round(t / UNITS[name]) * UNITS[name], t), "%s is not made of multiples of %g" % (name, UNITS[name])
    s = conv_summability(c)
    for kind, units in s.items():
        assert units < LIMIT, "%s: sum of |terms| is %.4g units, not below 2^24 = %.4g: f32 additions may round" % (kind, units, LIMIT)
    return s


# ------------------------------------------------------------------------------------------------------------------------------
# max-pool inputs, f32 [N, C, H, W]
# ------------------------------------------------------------------------------------------------------------------------------
POOL_HW = [(2, 2), (2, 3), (3, 2), (5, 7), (9, 9), (8, 6), (25, 12)]
POOL_C = [4, 64, 260]
POOL_N = [1, 3]
POOL_WRAP = (2, 128, 259, 517)      # [N, C, H, W]: 2 * 129 * 258 * 32 float4 items > 8192 * 256, H and W odd


def windows(t):
    """[N, C, H, W] -> [N, C, H//2, W//2, 4]: the 2x2 windows in row-major order (an odd last row / column belongs to none)"""
    n, c, h, w = t.shape
    ho, wo = h // 2, w // 2
    return t[:, :, :2 * ho, :2 * wo].reshape(n, c, ho, 2, wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, ho, wo, 4)


def from_windows(win, h, w, rest):
    """the inverse of `windows`; the pixels of an odd last row / column come from `rest` [N, C, H, W]"""
    n, c, ho, wo, _ = win.shape
    out = rest.clone()
    out[:, :, :2 * ho, :2 * wo] = win.reshape(n, c, ho, wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, 2 * ho, 2 * wo)
    return out


def _window_kind(shape, kinds):
    """[N, C, Ho, Wo] of 0 .. kinds-1, cycling over the windows in memory order: every kind occurs once there are `kinds` windows"""
    n, c, h, w = shape
    cnt = n * c * (h // 2) * (w // 2)
    return (torch.arange(cnt) % kinds).reshape(n, c, h // 2, w // 2)


def _plant(shape, seed, value, base):
    """`base` with `value` planted per window by kind: 0 none, 1 one element, 2 two or three elements, 3 all four"""
    g = gen(seed, *shape)
    kind = _window_kind(shape, 4)
    order = torch.rand(kind.shape + (4,), generator=g).argsort(-1)       # a random permutation of the window's four places
    count = torch.where(kind == 2, torch.randint(2, 4, kind.shape, generator=g), torch.where(kind == 3, 4, kind))
    mask = order < count.unsqueeze(-1)
    win = windows(base).clone()
    win[mask] = value
    return from_windows(win, shape[2], shape[3], base)


def pool_relu_ties(shape, seed=1):
    """post-ReLU integers: about half the elements are +0.0, the rest 1 .. 3, so most windows hold their maximum more than once"""
    return torch.relu(torch.randint(-3, 4, shape, generator=gen(seed, *shape)).float())


def pool_all_equal(shape, seed=2):
    """every window holds one value four times (another value per window)"""
    n, c, h, w = shape
    g = gen(seed, *shape)
    rest = torch.randint(-50, 51, shape, generator=g).float()
    v = torch.randint(-50, 51, (n, c, h // 2, w // 2, 1), generator=g).float()
    return from_windows(v.expand(-1, -1, -1, -1, 4), h, w, rest)


def pool_all_negative(shape, seed=3):
    """every element below zero: a maximum that started from 0 instead of the window's first element shows"""
    return -torch.randint(1, 100, shape, generator=gen(seed, *shape)).float()


def pool_neg_inf(shape, seed=4):
    """windows with none, one, two or three, and four -inf among negative numbers"""
    return _plant(shape, seed, float("-inf"), pool_all_negative(shape, seed + 100))


def pool_nan(shape, seed=5):
    """windows with none, one, two or three, and four NaN among numbers of both signs"""
    return _plant(shape, seed, float("nan"), torch.randint(-50, 51, shape, generator=gen(seed + 100, *shape)).float())


POOL_MAKERS = {"relu-ties": pool_relu_ties, "all-equal": pool_all_equal, "all-negative": pool_all_negative, "neg-inf": pool_neg_inf,
               "nan": pool_nan}


def pool_upstream_gradient(shape, seed=6):
    """dy [N, C, H//2, W//2]: non-zero integers of both signs, so the element that received it is the one that is not 0"""
    n, c, h, w = shape
    mag = torch.randint(1, 9, (n, c, h // 2, w // 2), generator=gen(seed, *shape))
    return (mag * (1 - 2 * (torch.arange(mag.numel()).reshape(mag.shape) % 2))).float()      # alternating signs in memory order


def pool_reference(x, dy):
    """(y, dx) of F.max_pool2d(x, 2, 2) and its autograd on the host, f32"""
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, 2, 2)
    y.backward(dy)
    return y.detach(), xr.grad


def check_pool(x, dy, y, dx, y_ref, dx_ref, what=""):
    """The rule for ops.maxpool2x2 against torch (all tensors on the host).  Forward: exact, NaN where torch has NaN.  Backward: where the
    window's maximum is a number, exactly torch's dx; in a window that holds a NaN all four elements are written, exactly one of them
    receives dy and that one is a NaN element of x (torch takes the last NaN; which one is not pinned); the dropped last row / column of
    an odd size is exactly 0."""
    assert tuple(y.shape) == tuple(y_ref.shape) and tuple(dx.shape) == tuple(x.shape), what
    nan = torch.isnan(y_ref)
    assert torch.equal(torch.isnan(y), nan), "%s: forward: NaN mask differs from torch (%d vs %d NaN)" % (what, int(torch.isnan(y).sum()), int(nan.sum()))
    assert torch.equal(torch.nan_to_num(y, nan=0.0), torch.nan_to_num(y_ref, nan=0.0)), "%s: forward differs from torch" % what
    assert not torch.isnan(dx).any(), "%s: backward: dx holds NaN (an element the kernel did not write?)" % what
    h, w = x.shape[2:]
    ho, wo = h // 2, w // 2
    assert (dx[:, :, 2 * ho:, :] == 0).all() and (dx[:, :, :, 2 * wo:] == 0).all(), "%s: backward: the dropped last row / column is not 0" % what
    assert torch.equal(dx[:, :, 2 * ho:, :], dx_ref[:, :, 2 * ho:, :]) and torch.equal(dx[:, :, :, 2 * wo:], dx_ref[:, :, :, 2 * wo:])
    dw, dw_ref, xw = windows(dx), windows(dx_ref), windows(x)
    assert torch.equal(dw[~nan], dw_ref[~nan]), "%s: backward differs from torch in %d windows without NaN" % (
        what, int((dw[~nan] != dw_ref[~nan]).any(-1).sum()))
    if nan.any():
        got, gx, g = dw[nan], xw[nan], dy[nan]
        assert (g != 0).all()
        hit = got != 0
        assert (hit.sum(-1) == 1).all(), "%s: backward: a NaN window with %s elements receiving a gradient" % (what, sorted(set(hit.sum(-1).tolist())))
        assert torch.equal(got.sum(-1), g), "%s: backward: the receiving element of a NaN window does not hold dy" % what
        assert torch.isnan(gx[hit]).all(), "%s: backward: dy of a NaN window went to an element that is no NaN" % what
