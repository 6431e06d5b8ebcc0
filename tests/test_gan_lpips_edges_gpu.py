"""The PatchGAN / LPIPS support kernels (csrc/gan_f32.hip, csrc/lpips_f32.hip) at their edges: odd sizes, channel counts that are no
multiple of a vector or a tile, loops that wrap past their grid cap (8192 or 16384 blocks of 256), NaN / inf / signed zeros.

Every comparison is bit for bit unless a bound is named here:
  data movement (im2col, col2im, weight reorder)   equal to the index-built float64 references of tests/gan_lpips_inputs.py
  ops.conv4x4 forward, dx, dw, db                  equal to float64 F.conv2d on exactly summable operands (no f32 addition can round)
  ops.maxpool2x2                                   equal to F.max_pool2d(x, 2, 2) and its autograd; NaN windows by gan_lpips_inputs.check_pool
  ops.leaky_relu forward, backward                 equal to torch f32, the sign of zero and the NaN positions included
  ops.scale_shift                                  forward |err| <= 2^-23 |ref64| (one subtraction and one division, each rounded once: with
                                                   u = 2^-24 the relative error of a rounding is <= u / (1 + u), and two of them compound to
                                                   < 2u); backward <= 2^-24 |ref64| (one division).  Both are what a correctly rounded
                                                   division gives; equality with torch f32 is printed
  ops.lpips_layer_distance, zero feature vectors   forward 2e-5 against torch f32, gradient by the rule of test_lpips_layer_distance
  whole networks at sizes with odd layers          1e-3 forward, 5e-3 gradients, 1e-4 buffers: the figures of tests/test_gan_lpips_gpu.py
Outputs of direct C-ABI calls sit in canary_buffers.out_buf: pre-filled (NaN; a number where NaN is a legitimate result), canary behind.
"""
import pytest
import torch
import torch.nn.functional as F

import exact_inputs as E
import gan_lpips_inputs as I
from canary_buffers import DEV, assert_canary, call, out_buf, padded
from test_gan_lpips_gpu import _lpips_reference, close

pytestmark = pytest.mark.gpu
ERR_ARG = 1             # ODVAE_ERR_ARG
PREFILL = 777.0         # pre-fill of outputs for which NaN is a legitimate value; no input or gradient of those cases holds it


def equal_bits(got, want, what):
    """raw bits: data movement copies, it sums nothing that could turn out as -0.0"""
    E.assert_bits_equal(got.cpu(), want, what, summed=False)


# ---- im2col / col2im / weight reorder through the C ABI -----------------------------------------------------------------------------
def run_im2col(L, x, stride):
    n, hi, wi, c = x.shape
    ho, wo = I.out4x4(hi, stride), I.out4x4(wi, stride)
    xb, xd = padded(x)
    ob, cols = out_buf(n * ho * wo * 16 * c)
    call(L.odvae_im2col4x4_f32, xd.data_ptr(), cols.data_ptr(), n, hi, wi, c, ho, wo, stride)
    assert_canary(xb, ob)
    return cols.view(n * ho * wo, 16 * c)


def run_col2im(L, dcols, n, hi, wi, c, stride):
    ho, wo = I.out4x4(hi, stride), I.out4x4(wi, stride)
    db, dd = padded(dcols)
    ob, dx = out_buf(n * hi * wi * c)
    call(L.odvae_col2im4x4_f32, dd.data_ptr(), dx.data_ptr(), n, hi, wi, c, ho, wo, stride)
    assert_canary(db, ob)
    return dx.view(n, hi, wi, c)


def small_integers(shape, *key):
    """integers in [-8, 8]: a sum of up to 16 of them is exact in any order"""
    return torch.randint(-8, 9, shape, generator=I.gen(*key)).float()


MOVE_IDS = ["s%d-%dx%d-c%d-n%d" % (s, hw[0], hw[1], c, n) for s, hw, c, n in I.MOVE_CASES]


@pytest.mark.parametrize("stride,hw,c,n", I.MOVE_CASES, ids=MOVE_IDS)
def test_im2col_and_col2im(hip_lib, stride, hw, c, n):
    hi, wi = hw
    x = I.distinct_integers((n, hi, wi, c))
    equal_bits(run_im2col(hip_lib, x, stride), I.im2col4x4(x.double(), stride).float(), "im2col4x4")
    ho, wo = I.out4x4(hi, stride), I.out4x4(wi, stride)
    d = small_integers((n * ho * wo, 16 * c), 11, stride, hi, wi, c, n)
    want = I.col2im4x4(d.double(), n, hi, wi, c, stride).float()
    E.assert_bits_equal(run_col2im(hip_lib, d, n, hi, wi, c, stride).cpu(), want, "col2im4x4", summed=True)


def test_im2col_where_the_grid_wraps(hip_lib):
    """297 * 297 * 48 = 4 234 032 items: past 16384 * 256 = 4 194 304, and 48 past a multiple of 256 (a tail shorter than a wavefront)"""
    x = I.distinct_integers((1, 298, 298, 3))
    assert 297 * 297 * 48 > 16384 * 256 and (297 * 297 * 48) % 256 == 48
    equal_bits(run_im2col(hip_lib, x, 1), I.im2col4x4(x.double(), 1).float(), "im2col4x4 past the grid cap")


def test_col2im_where_the_grid_wraps(hip_lib):
    """2049 * 2049 = 4 198 401 items, an odd count past 16384 * 256; stride 2 on an odd size"""
    hi = wi = 2049
    ho = I.out4x4(hi, 2)
    d = small_integers((ho * ho, 16), 13)
    want = I.col2im4x4(d.double(), 1, hi, wi, 1, 2).float()
    E.assert_bits_equal(run_col2im(hip_lib, d, 1, hi, wi, 1, 2).cpu(), want, "col2im4x4 past the grid cap", summed=True)


@pytest.mark.parametrize("cout,cin", I.REORDER_CASES + [(257, 511)], ids=lambda v: str(v))
def test_weight_reorder(hip_lib, cout, cin):
    """both directions and the round trip; (257, 511): 2 101 232 items, past 8192 * 256 = 2 097 152 with a ragged tail"""
    w = I.distinct_integers((cout, cin, 4, 4))
    wb, wd = padded(w)
    gb, g = out_buf(w.numel())
    call(hip_lib.odvae_weight4x4_reorder_f32, wd.data_ptr(), g.data_ptr(), cout, cin, 1)
    assert_canary(wb, gb)
    equal_bits(g.view(cout, 16 * cin), I.weight_to_gemm(w), "OIHW -> GEMM layout")
    bb, back = out_buf(w.numel())
    call(hip_lib.odvae_weight4x4_reorder_f32, g.data_ptr(), back.data_ptr(), cout, cin, 0)
    assert_canary(gb, bb)
    equal_bits(back.view(w.shape), w, "round trip")
    src = I.distinct_integers((cout, 16 * cin)) + 0.5          # the inverse on its own, from values the forward direction never produced
    sb, sd = padded(src)
    ob, o = out_buf(w.numel())
    call(hip_lib.odvae_weight4x4_reorder_f32, sd.data_ptr(), o.data_ptr(), cout, cin, 0)
    assert_canary(sb, ob)
    equal_bits(o.view(w.shape), I.weight_from_gemm(src, cin), "GEMM layout -> OIHW")


@pytest.mark.parametrize("name", ["odvae_im2col4x4_f32", "odvae_col2im4x4_f32"])
def test_data_movement_refuses_a_wrong_geometry(hip_lib, name):
    """Ho / Wo that do not belong to (Hi, Wi, stride), a stride other than 1 or 2, an input under 2 pixels: an error code, a message,
    and an output that was not touched"""
    fn = getattr(hip_lib, name)
    n, hi, wi, c = 2, 9, 7, 4
    src = torch.ones(n * hi * wi * 16 * c, device=DEV)          # large enough for either direction
    ob, out = out_buf(n * hi * wi * 16 * c)
    for stride, ho, wo, h, w in [(2, 5, 3, hi, wi), (2, 4, 4, hi, wi), (2, 3, 3, hi, wi), (1, 8, 7, hi, wi), (1, 9, 6, hi, wi),
                                 (3, 3, 2, hi, wi), (0, 4, 3, hi, wi), (2, 1, 3, 1, wi), (2, 0, 3, 1, wi), (1, 8, 0, hi, 1)]:
        rc = fn(src.data_ptr(), out.data_ptr(), n, h, w, c, ho, wo, stride, 0)
        assert rc == ERR_ARG, "%s accepted Hi=%d Wi=%d Ho=%d Wo=%d stride=%d" % (name, h, w, ho, wo, stride)
        assert hip_lib.odvae_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all().item(), "a refused call wrote to its output"
    assert_canary(ob)
    assert fn(src.data_ptr(), out.data_ptr(), n, hi, wi, c, 4, 3, 2, 0) == 0        # the right geometry of the same arguments


# ---- ops.conv4x4 on exactly summable operands ---------------------------------------------------------------------------------------
CONV_SHAPES = [(s, hw, cin, cout) for s, hw in I.CONV_GEOMETRY for cin in I.CONV_CIN for cout in I.CONV_COUT]


@pytest.mark.parametrize("stride,hw,cin,cout", CONV_SHAPES, ids=["s%d-%dx%d-ci%d-co%d" % (s, hw[0], hw[1], ci, co) for s, hw, ci, co in CONV_SHAPES])
def test_conv4x4_exact(hip_lib, stride, hw, cin, cout):
    """Forward, dx, dw, db equal to the float64 reference, with and without bias, N = 1 and 3 (the cases of gan_lpips_inputs.CONV_CASES;
    tests/test_gan_lpips_inputs.py asserts the precondition on each)"""
    from odvae_amd import ops
    for bias in (True, False):
        for n in I.CONV_N:
            assert (stride, hw, cin, cout, bias, n) in I.CONV_CASES
            c = I.make_conv_case(stride, hw, cin, cout, bias, n)
            r = I.conv_references(c)
            what = "conv4x4 s%d %dx%d cin %d cout %d bias %s n %d: " % (stride, hw[0], hw[1], cin, cout, bias, n)
            xd, wd = c["x"].float().to(DEV).requires_grad_(True), c["w"].float().to(DEV).requires_grad_(True)
            bd = c["b"].float().to(DEV).requires_grad_(True) if bias else None
            y = ops.conv4x4(xd, wd, bd, stride)
            E.assert_bits_equal(y.detach().cpu(), r["y"].float(), what + "forward")
            y.backward(c["dy"].float().to(DEV))
            E.assert_bits_equal(xd.grad.cpu(), r["dx"].float(), what + "dx")
            E.assert_bits_equal(wd.grad.cpu(), r["dw"].float(), what + "dw")
            if bias:
                E.assert_bits_equal(bd.grad.cpu(), r["db"].float(), what + "db")


def test_conv4x4_refuses_what_torch_refuses(hip_lib):
    """before any launch: ValueError, not an error code that the Ho / Wo check happens to produce"""
    from odvae_amd import ops
    w = torch.zeros(4, 4, 4, 4, device=DEV)
    for shape, stride in [((1, 4, 1, 8), 1), ((1, 4, 1, 8), 2), ((1, 4, 8, 1), 2), ((1, 4, 1, 1), 1), ((1, 4, 8, 8), 3), ((1, 3, 8, 8), 1)]:
        with pytest.raises(ValueError):
            ops.conv4x4(torch.zeros(shape, device=DEV), w, None, stride)
        if stride in (1, 2):
            with pytest.raises(RuntimeError):
                F.conv2d(torch.zeros(shape), w.cpu(), None, stride=stride, padding=1)


# ---- ops.maxpool2x2 -----------------------------------------------------------------------------------------------------------------
def pool_through_the_abi(L, x, dy, fill):
    """forward and backward through the C ABI on NHWC buffers with canaries; (y, dx) as NCHW host tensors"""
    n, c, h, w = x.shape
    ho, wo = h // 2, w // 2
    xb, xd = padded(x.permute(0, 2, 3, 1).contiguous())
    gb, gd = padded(dy.permute(0, 2, 3, 1).contiguous())
    yb, y = out_buf(n * ho * wo * c, fill)
    call(L.odvae_maxpool2x2_f32, xd.data_ptr(), y.data_ptr(), n, h, w, c, ho, wo)
    assert_canary(xb, yb)
    db, dx = out_buf(n * h * w * c, fill)
    call(L.odvae_maxpool2x2_bwd_f32, xd.data_ptr(), y.data_ptr(), gd.data_ptr(), dx.data_ptr(), n, h, w, c, ho, wo)
    assert_canary(xb, yb, gb, db)
    assert not (dx == fill).any().item() and not (y == fill).any().item(), "an output element was not written"
    return y.view(n, ho, wo, c).permute(0, 3, 1, 2).cpu(), dx.view(n, h, w, c).permute(0, 3, 1, 2).cpu()


def check_pool_on_device(L, x, dy, what, abi=True):
    from odvae_amd import ops
    y_ref, dx_ref = I.pool_reference(x, dy)
    xd = x.to(DEV).requires_grad_(True)
    y = ops.maxpool2x2(xd)
    y.backward(dy.to(DEV))
    I.check_pool(x, dy, y.detach().cpu(), xd.grad.cpu(), y_ref, dx_ref, what + " (ops)")
    if abi:
        fill = PREFILL if torch.isnan(x).any() else float("nan")
        ya, dxa = pool_through_the_abi(L, x, dy, fill)
        I.check_pool(x, dy, ya, dxa, y_ref, dx_ref, what + " (C ABI)")


@pytest.mark.parametrize("maker", sorted(I.POOL_MAKERS))
@pytest.mark.parametrize("h,w", I.POOL_HW, ids=lambda v: str(v))
def test_maxpool2x2(hip_lib, h, w, maker):
    for c in I.POOL_C:
        for n in I.POOL_N:
            shape = (n, c, h, w)
            check_pool_on_device(hip_lib, I.POOL_MAKERS[maker](shape), I.pool_upstream_gradient(shape), "maxpool2x2 %s %s" % (maker, shape))


def test_maxpool2x2_where_the_grid_wraps(hip_lib):
    n, c, h, w = I.POOL_WRAP
    assert n * (h // 2) * (w // 2) * (c // 4) > 8192 * 256 and h % 2 == 1 and w % 2 == 1
    x = torch.randint(-1000, 1001, I.POOL_WRAP, generator=I.gen(17)).float()
    check_pool_on_device(hip_lib, x, I.pool_upstream_gradient(I.POOL_WRAP), "maxpool2x2 past the grid cap", abi=False)


def test_maxpool2x2_refusals(hip_lib):
    from odvae_amd import lib, ops
    for shape in [(1, 4, 1, 8), (1, 4, 8, 1), (2, 4, 1, 1)]:
        with pytest.raises(ValueError):
            ops.maxpool2x2(torch.zeros(shape, device=DEV))
        with pytest.raises(RuntimeError):
            F.max_pool2d(torch.zeros(shape), 2, 2)
    with pytest.raises(lib.HipLibraryError, match="C % 4"):
        ops.maxpool2x2(torch.zeros(1, 6, 4, 4, device=DEV))
    # the C ABI checks Ho == Hi / 2, Wo == Wi / 2 and leaves its outputs alone
    x = torch.ones(1 * 5 * 7 * 4, device=DEV)
    ob, out = out_buf(1 * 5 * 7 * 4)
    for ho, wo in [(3, 3), (2, 4), (2, 2), (1, 3)]:
        assert hip_lib.odvae_maxpool2x2_f32(x.data_ptr(), out.data_ptr(), 1, 5, 7, 4, ho, wo, 0) == ERR_ARG
        assert hip_lib.odvae_maxpool2x2_bwd_f32(x.data_ptr(), x.data_ptr(), x.data_ptr(), out.data_ptr(), 1, 5, 7, 4, ho, wo, 0) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(out).all().item()
    assert_canary(ob)


# ---- ScalingLayer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 3, 1, 1), (1, 3, 5, 17), (2, 3, 600, 600)], ids=["1px", "85px", "2x600x600"])
def test_scale_shift(hip_lib, shape):
    """2 * 600 * 600 * 3 = 2 160 000 items: past 8192 * 256"""
    from odvae_amd import ops
    g = I.gen(19, *shape)
    shift = torch.tensor([-.030, -.088, -.188])[None, :, None, None]
    scale = torch.tensor([.458, .448, .450])[None, :, None, None]
    x, dy = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    y = ops.scale_shift(xd, shift.to(DEV), scale.to(DEV))
    y.backward(dy.to(DEV))
    y, dx = y.detach().cpu(), xd.grad.cpu()
    ref = (x.double() - shift.double()) / scale.double()
    dref = dy.double() / scale.double()
    ferr, berr = ((y.double() - ref).abs() / ref.abs()).max().item(), ((dx.double() - dref).abs() / dref.abs()).max().item()
    print("scale_shift %s: forward max relative error %.3g x 2^-23, equal to torch f32: %s; backward %.3g x 2^-24, equal to torch f32: %s" % (
        shape, ferr * 2 ** 23, torch.equal(y, (x - shift) / scale), berr * 2 ** 24, torch.equal(dx, dy / scale)))
    assert ((y.double() - ref).abs() <= 2.0 ** -23 * ref.abs()).all(), "forward: %.3g x 2^-23" % (ferr * 2 ** 23)
    assert ((dx.double() - dref).abs() <= 2.0 ** -24 * dref.abs()).all(), "backward: %.3g x 2^-24" % (berr * 2 ** 24)


# ---- LeakyReLU ----------------------------------------------------------------------------------------------------------------------
SPECIALS = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e-40, -1e-40, 1.401298464324817e-45, -1.401298464324817e-45,
            1.1754942e-38, -1.1754942e-38, 3.4028234e38, -3.4028234e38]


def equal_with_nan(got, want, what):
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), "%s: NaN at other places than torch" % what
    gb, wb = got.contiguous().view(torch.int32)[~nan], want.contiguous().view(torch.int32)[~nan]
    bad = gb != wb
    assert not bad.any(), "%s: %d elements differ in bits, first got %r want %r" % (
        what, int(bad.sum()), got[~nan][bad][0].item(), want[~nan][bad][0].item())


@pytest.mark.parametrize("slope", [0.2, 0.0])
@pytest.mark.parametrize("n", [1, 255, 257, 8192 * 256 + 3])
def test_leaky_relu(hip_lib, n, slope):
    from odvae_amd import ops
    g = I.gen(23, n)
    x, dy = torch.randn(n, generator=g), torch.randn(n, generator=g)
    sp = torch.tensor(SPECIALS)
    pos = torch.arange(len(SPECIALS)) * max(1, (n - 1) // (len(SPECIALS) - 1))       # spread from the first to (about) the last element
    if n >= len(SPECIALS):
        x[pos] = sp
        x[n - 1] = -0.0
    else:
        x[0] = -0.0
    for xs in ([x] if n >= len(SPECIALS) else [x] + [torch.full((1,), v) for v in SPECIALS]):
        xr = xs.clone().requires_grad_(True)
        y_ref = F.leaky_relu(xr, slope)
        y_ref.backward(dy[:xs.numel()])
        xd = xs.view(1, -1, 1, 1).to(DEV).requires_grad_(True)
        y = ops.leaky_relu(xd, slope)
        y.backward(dy[:xs.numel()].view(1, -1, 1, 1).to(DEV))
        equal_with_nan(y.detach().cpu().reshape(-1), y_ref.detach(), "leaky_relu(%g) forward, n = %d" % (slope, n))
        equal_with_nan(xd.grad.cpu().reshape(-1), xr.grad, "leaky_relu(%g) backward, n = %d" % (slope, n))


# ---- LPIPS layer distance with all-zero feature vectors -----------------------------------------------------------------------------
def test_lpips_layer_distance_with_zero_feature_vectors(hip_lib):
    """Pixels 0-4 of f1 and pixels 3-8 of f0 are all zero (3 and 4 in both).  torch's own gradient is NaN at the zero pixels of f1: the term
    (sum_c gb_c f1_c) f1_k / (n1^2 |f1|) is 0 * 0 / 0 there, and the kernel takes it as 0 (csrc/lpips_f32.hip).  That choice is pinned:
    the gradient is finite everywhere, at the zero pixels it is the remaining term gs * gb_k / 1e-10 with gb = -2 w normalize(f0), and at
    all other pixels it meets the float64 reference under the rule of test_lpips_layer_distance."""
    import gn_offset_inputs as G
    from odvae_amd import ops
    c, h, w = 64, 6, 5
    g = I.gen(29)
    f0 = torch.relu(torch.randn(2, c, h, w, generator=g))
    f1 = torch.relu(torch.randn(2, c, h, w, generator=g))
    f1.view(2, c, h * w)[:, :, 0:5] = 0.0
    f0.view(2, c, h * w)[:, :, 3:9] = 0.0
    z1 = (f1.abs().sum(1) == 0)                                      # [2, h, w]
    assert int(z1.sum()) == 10 and int((f0.abs().sum(1) == 0).sum()) == 12
    wt = torch.rand(1, c, 1, 1, generator=g) / c
    gw = torch.randn(2, generator=g)
    ref, grad = _lpips_reference(f0, f1, wt, gw, torch.float32)
    ref64, grad64 = _lpips_reference(f0, f1, wt, gw, torch.float64)
    assert torch.isnan(grad).any() and torch.isfinite(ref).all()
    f1d = f1.to(DEV).requires_grad_(True)
    out = ops.lpips_layer_distance(f0.to(DEV), f1d, wt.to(DEV))
    close(out, ref, 2e-5, "lpips dist with zero pixels")
    (out * gw.to(DEV)).sum().backward()
    got = f1d.grad.cpu()
    assert torch.isfinite(got).all(), "the gradient holds %d non-finite values" % int((~torch.isfinite(got)).sum())
    live = (~z1).unsqueeze(1).expand_as(got)
    gmax = grad64[live].abs().max()
    G.check([G.figure("distance / d64", out.cpu().double() / ref64, torch.ones_like(ref64), ref.double() / ref64, G.FLOOR_FWD),
             G.figure("gradient / max |g64| off the zero pixels", got[live].double() / gmax, grad64[live] / gmax, grad[live].double() / gmax, G.FLOOR_DX)],
            "lpips layer distance with zero feature vectors")
    n0 = f0.double() / (f0.double().pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    at_zero = gw.double().view(2, 1, 1, 1) / (h * w) * (-2.0 * wt.double() * n0) / 1e-10
    dead = z1.unsqueeze(1).expand_as(got)
    close(got[dead], at_zero[dead], 5e-4, "gradient at the zero pixels of f1")
    both = (z1 & (f0.abs().sum(1) == 0)).unsqueeze(1).expand_as(got)
    assert (got[both] == 0).all()


# ---- whole networks at sizes whose inner layers are odd -------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(24, 40), (72, 72)], ids=lambda v: str(v))
def test_lpips_style_at_sizes_with_odd_pools(hip_lib, h, w):
    """24 x 40: the fourth pool sees 3 x 5; 72 x 72: 9 x 9.  An unwritten dropped row / column of the pool's dx shows as NaN / Inf or as a
    wrong input gradient."""
    from odvae_amd.gan import LPIPSStyle
    from oracle.losses import LPIPSStyle as RefL
    net, ref = LPIPSStyle(), RefL()
    res = ref.load_state_dict(net.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    net = net.to(DEV).eval(); ref.eval()
    g = I.gen(31, h, w)
    x0 = torch.rand(2, 3, h, w, generator=g) * 2 - 1
    x1 = (x0 + 0.3 * torch.randn(2, 3, h, w, generator=g)).clamp(-1, 1)
    x1r = x1.clone().requires_grad_(True)
    d_ref = ref(x0, x1r)
    d_ref.sum().backward()
    x1d = x1.to(DEV).requires_grad_(True)
    d = net(x0.to(DEV), x1d)
    close(d, d_ref, 1e-3, "lpips %dx%d fwd" % (h, w))
    d.sum().backward()
    assert torch.isfinite(x1d.grad).all().item(), "dx holds %d non-finite values" % int((~torch.isfinite(x1d.grad)).sum())
    close(x1d.grad, x1r.grad, 5e-3, "lpips %dx%d dx" % (h, w))


def test_discriminator_at_36x44(hip_lib):
    """36 x 44 -> 18 x 22 -> 9 x 11 -> 4 x 5 -> 3 x 4 -> 2 x 3: a stride-2 convolution on an odd 9 x 11 input, stride-1 ones on 4 x 5 and 3 x 4"""
    from odvae_amd.gan import NLayerDiscriminator, weights_init
    from oracle.losses import NLayerDiscriminator as RefD
    torch.manual_seed(5)
    ref = RefD().apply(weights_init)
    net = NLayerDiscriminator()
    res = net.load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    net = net.to(DEV)
    ref.train(); net.train()
    x = torch.randn(2, 3, 36, 44, generator=I.gen(37))
    xr = x.clone().requires_grad_(True)
    y_ref = ref(xr)
    assert tuple(y_ref.shape) == (2, 1, 2, 3)
    gy = torch.randn(y_ref.shape, generator=I.gen(41))
    y_ref.backward(gy)
    xd = x.to(DEV).requires_grad_(True)
    y = net(xd)
    close(y, y_ref, 1e-3, "D fwd")
    y.backward(gy.to(DEV))
    close(xd.grad, xr.grad, 5e-3, "D dx")
    refp = dict(ref.named_parameters())
    for name, p in net.named_parameters():
        close(p.grad, refp[name].grad, 5e-3, "D grad " + name)
    refb = dict(ref.named_buffers())
    for name, b in net.named_buffers():
        close(b.float(), refb[name].float(), 1e-4, "D buffer " + name)
