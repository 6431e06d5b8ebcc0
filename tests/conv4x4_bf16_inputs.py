"""Exactly summable inputs for the 16-tap PatchGAN convolutions on the bf16 kernels: generators, float64 host models, references.

Built on tests/exact_inputs.py (its condition, its checker): the kernels multiply bf16 numbers exactly and add in f32 with one rounding
at the store, so on operands whose every partial sum is a whole number of units below 2^24 units an f32 output must EQUAL the float64
reference and a bf16 output must equal it rounded once.

Recipe A here (as there): x, dy integers in [-4, 4]; w multiples of 1/4 in [-2, 2]; bias multiples of 1/8 in [-2, 2]; forward unit
2^-3.  It stays exact up to K = 16 * 512: 8192 products of magnitude at most 8 = 64 units sum to at most 2^19 units, under 2^24.  The
condition is asserted on the tensors a test uses (`assert_exactly_summable`), never assumed.
Recipe L (the fused LeakyReLU(0.2)): w multiples of 5/4, bias multiples of 5/8, so every accumulator is a multiple of 5 units and a
negative accumulator's fifth is exact; the reference divides by 5 (exact in float64) where the kernel multiplies by the f32 0.2 -- the
product k (1 + 1.5e-8) units rounds to k units in f32, since 1.5e-8 is under the half ulp 2^-25 ... 2^-24.

The host models below spell the kernels' index arithmetic out tap by tap (they do not call F.conv2d): forward, the stride-1 data
gradient as the forward form on the flipped, transposed weights with pad 2, the stride-2 data gradient by parity class, the weight
gradient per tap.  Each is checked against F.conv2d / torch.autograd in float64, and each takes a `fault` that plants one of the
mistakes such a kernel can make; the checker must reject those.
Plain module: no fixtures, no device.  All tensors are float64 NCHW on the host.
"""
import torch
import torch.nn.functional as F

import exact_inputs as E

BF = torch.bfloat16
SLOPE = 0.2

# the shapes of tests/test_disc_bf16_gpu.py: (name, stride, n, cin, cout, h, w, bias); cin = 3 comes to the kernel zero-padded to 8
CASES = [
    ("s2_odd_both", 2, 2, 3, 64, 9, 11, True),          # both sizes odd -> 4 x 5
    ("s2_pad_row", 2, 2, 3, 64, 10, 12, True),          # the last window reaches the pad row
    ("s2_tiles", 2, 1, 64, 128, 36, 44, False),         # 18 x 22: output tiles 8 + 8 + 2 by 16 + 6
    ("s2_ragged_cout", 2, 3, 16, 36, 7, 6, False),      # ragged Cout, several images in one tile range
    ("s1_ragged", 1, 2, 128, 36, 10, 19, False),        # 9 x 18: ragged tile and ragged Cout
    ("s1_head", 1, 1, 512, 1, 5, 6, True),              # the logit head, deep K, f32 logits
    ("s1_smallest", 1, 2, 8, 1, 2, 2, True),            # the smallest legal input -> 1 x 1
]
# a weight gradient split over several blocks with a short last one (asserted on the plan the library reports): 9 one-pixel tiles
WGRAD_SPLIT_CASE = ("s1_wgrad_split", 1, 9, 256, 512, 2, 2, False)


def out4(h, stride):
    return (h + 2 - 4) // stride + 1


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def make_case(stride, n, cin, cout, h, w, bias=True, seed=0, recipe="A"):
    """dict: x [n, cin, h, w], w [cout, cin, 4, 4], b [cout] | None, dy [n, cout, ho, wo], stride, units"""
    g = torch.Generator().manual_seed(100003 * seed + 7919 * stride + 131 * cin + 17 * cout + 3 * h + w)
    ho, wo = out4(h, stride), out4(w, stride)
    c = {"stride": stride, "recipe": recipe, "res": None}
    c["x"], c["dy"] = _ints(g, (n, cin, h, w), -4, 4), _ints(g, (n, cout, ho, wo), -4, 4)
    if recipe == "A":
        c["w"] = _ints(g, (cout, cin, 4, 4), -8, 8) / 4
        c["b"] = _ints(g, (cout,), -16, 16) / 8 if bias else None
        c["units"] = {"x": 1.0, "w": 0.25, "dy": 1.0, "b": 0.125, "res": 1.0}
    elif recipe == "L":
        c["w"] = 5 * _ints(g, (cout, cin, 4, 4), -8, 8) / 4
        c["b"] = 5 * _ints(g, (cout,), -16, 16) / 8 if bias else None
        c["units"] = {"x": 1.0, "w": 1.25, "dy": 1.0, "b": 0.625, "res": 1.0}
    else:
        raise ValueError("recipe %r" % (recipe,))
    return c


def as_exact_case(c):
    """The case in the vocabulary of exact_inputs: Conv2d(k=4, pad=1) at stride 1 is its mode 0 with a 4x4 weight (F.conv2d, padding
    1); at stride 2 it is its mode 1 -- pad (0, 1, 0, 1), stride 2 -- on x with one more zero row on top and zero column on the left.
    Zeros add nothing to a sum of |terms|, so the bounds are those of the 4x4 convolution itself."""
    d = dict(c)
    if c["stride"] == 1:
        d["mode"] = 0
    else:
        d["mode"] = 1
        d["x"] = F.pad(c["x"], (1, 0, 1, 0))
    return d


def assert_exactly_summable(c, dy_f32=None, dy_f32_unit=None):
    """exact_inputs.assert_exactly_summable on the tensors of c (forward, data gradient, weight gradient, bias gradient)"""
    d = as_exact_case(c)
    assert torch.equal(E.conv_f64(d["mode"], d["x"], d["w"], d["b"]), conv_f64(c["x"], c["w"], c["b"], c["stride"])), "as_exact_case"
    return E.assert_exactly_summable(d, dy_f32, dy_f32_unit)


# ------------------------------------------------------------------------------------------------------------------------------
# the float64 mathematics by torch (what the host models are checked against)
# ------------------------------------------------------------------------------------------------------------------------------
def conv_f64(x, w, b, stride):
    return F.conv2d(x, w, b, stride=stride, padding=1)


def dgrad_f64(dy, w, x_shape, stride):
    x = torch.zeros(tuple(x_shape), dtype=dy.dtype, requires_grad=True)
    return torch.autograd.grad(conv_f64(x, w, None, stride), x, dy)[0]


def wgrad_f64(x, dy, w_shape, stride):
    w = torch.zeros(tuple(w_shape), dtype=x.dtype, requires_grad=True)
    return torch.autograd.grad(conv_f64(x, w, None, stride), w, dy)[0]


# ------------------------------------------------------------------------------------------------------------------------------
# host models of the kernels, tap by tap, with planted faults
# ------------------------------------------------------------------------------------------------------------------------------
FAULTS = ("swap_taps", "pad2", "wrong_parity", "drop_last_row", "lrelu_after_round")
_P = 4      # the models pad generously and index from there


def _correlate(x, w, stride, pad, ho, wo, fault=None):
    """y[n, o, oy, ox] = sum_{c, kh, kw} x[n, c, stride oy - pad + kh, stride ox - pad + kw] w[o, c, kh, kw], zero outside x"""
    n, cin, h, wd = x.shape
    xp = F.pad(x, (_P, _P + 4, _P, _P + 4))
    y = torch.zeros(n, w.shape[0], ho, wo, dtype=x.dtype)
    for kh in range(4):
        for kw in range(4):
            wt = w[:, :, kh, kw]
            if fault == "swap_taps" and (kh, kw) in ((0, 1), (1, 0)):
                wt = w[:, :, kw, kh]
            r0, c0 = _P - pad + kh, _P - pad + kw
            patch = xp[:, :, r0:r0 + stride * (ho - 1) + 1:stride, c0:c0 + stride * (wo - 1) + 1:stride]
            y = y + torch.einsum("nchw,oc->nohw", patch, wt)
    return y


def forward_model(x, w, b, stride, fault=None):
    """the forward kernel's sum (float64, no rounding)"""
    h, wd = x.shape[2], x.shape[3]
    if fault == "drop_last_row" and h % 2 == 1:
        x = x.clone()
        x[:, :, h - 1] = 0          # an odd last row is read by the last window's fourth tap row: a kernel that stops at 2 * Ho rows loses it
    y = _correlate(x, w, stride, 2 if fault == "pad2" else 1, out4(h, stride), out4(wd, stride), fault)
    return y if b is None else y + b.reshape(1, -1, 1, 1)


def flipped_transposed(w):
    """W'[ci][co][kh][kw] = w[co][ci][3 - kh][3 - kw]: the data-gradient pack"""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def dgrad_s1_model(dy, w, x_shape, fault=None):
    """stride 1: the forward form on the flipped, transposed weights with pad 2: Hi = Ho + 1"""
    return _correlate(dy, flipped_transposed(w), 1, 1 if fault == "pad2" else 2, x_shape[2], x_shape[3], fault)


def dgrad_s2_model(dy, w, x_shape, fault=None):
    """stride 2, the transposed convolution by parity class: input pixel (iy, ix) with parities (py, px) takes the taps
    (py + 2a, px + 2b), a, b in {0, 1}, of the flipped weights, from dy[(iy + py) / 2 - 1 + a][(ix + px) / 2 - 1 + b]"""
    n, cin, h, wd = x_shape
    wf = flipped_transposed(w)
    dyp = F.pad(dy, (1, 3, 1, 3))           # index + 1; rows past Ho are zero (pixels no window reads get 0)
    dx = torch.zeros(n, cin, h, wd, dtype=dy.dtype)
    for py in range(2):
        for px in range(2):
            ni, nj = len(range(py, h, 2)), len(range(px, wd, 2))
            if ni == 0 or nj == 0:
                continue
            acc = torch.zeros(n, cin, ni, nj, dtype=dy.dtype)
            for a in range(2):
                for b in range(2):
                    qy, qx = (1 - py, 1 - px) if fault == "wrong_parity" else (py, px)
                    wt = wf[:, :, qy + 2 * a, qx + 2 * b]
                    patch = dyp[:, :, py + a:py + a + ni, px + b:px + b + nj]       # (i + py - 1 + a) + 1
                    acc = acc + torch.einsum("nohw,co->nchw", patch, wt)
            dx[:, :, py::2, px::2] = acc
    return dx


def dgrad_model(dy, w, x_shape, stride, fault=None):
    return dgrad_s1_model(dy, w, x_shape, fault) if stride == 1 else dgrad_s2_model(dy, w, x_shape, fault)


def wgrad_model(x, dy, stride, fault=None):
    """dw[o, c, kh, kw] = sum_{n, oy, ox} dy[n, o, oy, ox] x[n, c, stride oy - 1 + kh, stride ox - 1 + kw]"""
    n, cin, h, wd = x.shape
    ho, wo = dy.shape[2], dy.shape[3]
    if fault == "drop_last_row" and h % 2 == 1:
        x = x.clone()
        x[:, :, h - 1] = 0
    pad = 2 if fault == "pad2" else 1
    xp = F.pad(x, (_P, _P + 4, _P, _P + 4))
    dw = torch.zeros(dy.shape[1], cin, 4, 4, dtype=x.dtype)
    for kh in range(4):
        for kw in range(4):
            r0, c0 = _P - pad + kh, _P - pad + kw
            patch = xp[:, :, r0:r0 + stride * (ho - 1) + 1:stride, c0:c0 + stride * (wo - 1) + 1:stride]
            th, tw = (kw, kh) if (fault == "swap_taps" and (kh, kw) in ((0, 1), (1, 0))) else (kh, kw)
            dw[:, :, th, tw] = torch.einsum("nohw,nchw->oc", dy, patch)
    return dw


def lrelu_f64(acc, fault=None):
    """LeakyReLU(0.2) on accumulators that are multiples of 5 units, then the one rounding; a NaN stays a NaN.
    fault lrelu_after_round: round first, scale the rounded value, round again."""
    if fault == "lrelu_after_round":
        r = E.rne(acc).double()
        return E.rne(torch.where(r > 0, r, r / 5))
    return E.rne(torch.where(acc > 0, acc, acc / 5))


def rne(t):
    return E.rne(t)


def lrelu_bwd_f32(y, dy):
    """bf16 = round(dy * (y > 0 ? 1 : 0.2)) with the product taken in f32 against the f32 0.2, as the kernel takes it (dy: bf16 numbers)"""
    d = dy.float()
    return torch.where(y.float() > 0, d, d * SLOPE).to(BF)


# ------------------------------------------------------------------------------------------------------------------------------
# what the kernels must produce, bit for bit
# ------------------------------------------------------------------------------------------------------------------------------
def references(c, out_f32=False, dx_f32=False, lrelu=False, dy_f32=None):
    """y: conv + bias, one rounding (none with out_f32; with lrelu the LeakyReLU on the exact accumulator first).  dx: one rounding (none
    with dx_f32: the image layer).  dy_f32: an f32 upstream gradient (the head) -- the products see rne(dy_f32), the bias gradient sums
    the f32 values themselves.  With lrelu the upstream gradient is first multiplied by the LeakyReLU's derivative (1 or 0.2) and
    rounded once: the kernels see that.  dw, db: f32, no rounding."""
    x, w, s = c["x"], c["w"], c["stride"]
    acc = conv_f64(x, w, c["b"], s)
    dyb = rne(dy_f32).double() if dy_f32 is not None else c["dy"]
    r = {"y_exact": acc}
    if lrelu:
        r["y"] = lrelu_f64(acc)
        dyb = lrelu_bwd_f32(r["y"], dyb).double()
        r["g"] = dyb
    else:
        r["y"] = acc.float() if out_f32 else rne(acc)
    du = dgrad_f64(dyb, w, x.shape, s)
    r["dx_exact"] = du
    r["dx"] = du.float() if dx_f32 else rne(du)
    r["dw"] = wgrad_f64(x, dyb, w.shape, s).float()
    r["db"] = (dy_f32 if (dy_f32 is not None and not lrelu) else dyb).sum((0, 2, 3)).float()
    return r


def nan_footprint(shape_out, stride, iy, ix):
    """[ho, wo] bool: the outputs of Conv2d(k=4, pad=1, stride) whose 4x4 window holds input pixel (iy, ix)"""
    ho, wo = shape_out
    oy = torch.arange(ho).reshape(-1, 1) * stride - 1
    ox = torch.arange(wo).reshape(1, -1) * stride - 1
    return (oy <= iy) & (iy <= oy + 3) & (ox <= ix) & (ix <= ox + 3)
