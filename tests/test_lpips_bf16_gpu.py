"""The opt-in bf16 perceptual net (gan.LPIPSStyle.set_precision("bf16")): conv_bf16.hip's ReLU / mask epilogues, lpips_bf16.hip.

Per kernel, bit for bit against float64 on exactly summable operands (tests/exact_inputs.py recipe A; tests/lpips_bf16_inputs.py):
  conv + ReLU forward, masked data gradient   N = 2 at 9 x 17 (2 x 2 tiles of 8 x 16, ragged both ways), 4 x 5 for 512 -> 512; pre-activations
                                              that are exactly 0 and negative; a planted NaN.  The eight new instantiations and who reaches them
                                              (KC = 64 where the padded reduction is a multiple of 64, else 32; W: more than 64 outputs, M: 33..64):
                                                RELU KC32 M  3(8) -> 64      RELU KC64 M  64 -> 64      RELU KC32 W  96 -> 136
                                                RELU KC64 W  64 -> 128, 128 -> 256, 256 -> 512, 512 -> 512, 40 -> 96 [reduce 40 pads to 64]
                                              data gradients (reduce = Cout, out = Cin):
                                                MASK KC64 M  of 64 -> 64, 64 -> 128      MASK KC64 W  of 128 -> 256, 256 -> 512, 512 -> 512
                                                MASK KC32 M  of 40 -> 96 [reduce 96]     MASK KC32 W  of 96 -> 136 [reduce 136 pads to 160]
  max-pool forward / backward                 9 x 11 -> 4 x 5 and 2 x 2 -> 1 x 1, C = 64 and 512: ties, -inf, NaN windows, a mask with zeros at the argmax
  distance forward / backward                 against the host model's f32 arithmetic: forward 2e-5 (the bound the f32 kernel's edge test holds its own
                                              arithmetic to), backward: the stored bf16 value is the rounding of SOME f32 within 2e-4 of max |g| of the
                                              model's f32 value (test_lpips_layer_distance's bound, then one rounding); HW = 1 and 35, C = 64 and 512,
                                              one all-zero feature vector, with and without the next slice's gradient, with and without the mask
  scaling layer                               (x - shift) / scale within one f32 rounding each of the subtraction and the division, then one bf16 rounding
A chain, bit for bit: scaling -> conv+ReLU -> conv+ReLU -> pool -> conv+ReLU -> tap, forward and backward, wired as LPIPSStyle wires its layers.
  (The distance's own gradient is not exactly summable -- it is a quotient of norms -- so the backward is seeded through the tap's
  pass-through output, which takes the same route through the tap's kernel: f32 sum with the distance gradient (0 here), mask, one rounding.)
The whole net against the f32 oracle by the rule of tests/test_bf16_model_gpu.py (no floors): N = 2 at 36 x 44, 24 x 40, 72 x 72.
The training step with the GAN on, precision bf16 + perceptual_precision bf16: that file's rule, run-to-run bit identity, and the switch
off again reproduces the values of a model that never had it on.
On the parent commit every test here that reaches ops.conv3x3(bf16, relu=True) fails (NotImplementedError / missing entry points).
"""
import pytest
import torch

import exact_inputs as E
import lpips_bf16_inputs as M
from test_lpips_bf16_inputs import CONV_CASES, dist_case, nan_at

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
CL = torch.channels_last


def dev_cl(t, dtype=BF):
    return t.to(dtype).to(DEV).contiguous(memory_format=CL)


def frozen(t):
    return torch.nn.Parameter(t.float().to(DEV), requires_grad=False)


# ------------------------------------------------------------------------------------------------------------------------------
# conv + ReLU, masked data gradient
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,n,h,w", CONV_CASES)
def test_conv_relu_and_masked_dgrad_exact(hip_lib, cin, cout, n, h, w):
    from odvae_amd import ops
    c = M.conv_case(cin, cout, n, h, w)
    E.assert_exactly_summable(c)
    ref = M.conv_case_references(c)
    wt, b = frozen(c["w"]), frozen(c["b"])
    x = dev_cl(c["x"])
    # the public op: a true gradient (ReLU mask in a pass of its own, plain data gradient)
    y = ops.conv3x3(x, wt, b, relu=True)
    assert y.dtype == BF
    E.assert_bits_equal(y.cpu(), ref["y"], "conv + ReLU y")
    if cin == 3:
        return      # the image layer's gradient has 3 f32 channels: the stem, below
    pre_dy = torch.where(ref["y"].double() > 0, c["dy"], torch.zeros_like(c["dy"]))
    xg = dev_cl(c["x"]).requires_grad_(True)
    ops.conv3x3(xg, wt, b, relu=True).backward(dev_cl(c["dy"]))
    E.assert_bits_equal(xg.grad.cpu(), M.conv_dgrad(pre_dy, c["w"]).float().to(BF), "conv + ReLU dx (self-contained)")
    # the VGG wiring: the incoming gradient is already masked, the outgoing one is masked with the layer's input
    xg = dev_cl(c["x"]).requires_grad_(True)
    ops.conv3x3_relu_bf16(xg, wt, b, mask_input=True, grad_premasked=True).backward(dev_cl(c["dy"]))
    E.assert_bits_equal(xg.grad.cpu(), ref["dx_masked"], "masked data gradient")
    xg = dev_cl(c["x"]).requires_grad_(True)
    ops.conv3x3_relu_bf16(xg, wt, b, mask_input=False, grad_premasked=True).backward(dev_cl(c["dy"]))
    E.assert_bits_equal(xg.grad.cpu(), ref["dx_plain"], "plain data gradient of a premasked layer")


@pytest.mark.parametrize("cin,cout,n,h,w", [(64, 64, 2, 9, 17), (128, 256, 2, 9, 17), (512, 512, 2, 4, 5)])
def test_conv_relu_keeps_a_nan(hip_lib, cin, cout, n, h, w):
    """A NaN in x: the 3 x 3 neighbourhood of y is NaN in every channel (the ReLU does not drop it), every other element is exact; in the
    masked data gradient a NaN mask is `not > 0`: zero there, exact elsewhere."""
    from odvae_amd import ops
    c = M.conv_case(cin, cout, n, h, w, nan_at=nan_at(h, w))
    ref = M.conv_case_references(c)
    assert 4 * cout <= int(torch.isnan(ref["y"]).sum()) <= 9 * cout
    wt, b = frozen(c["w"]), frozen(c["b"])
    xg = dev_cl(c["x"]).requires_grad_(True)
    y = ops.conv3x3_relu_bf16(xg, wt, b, mask_input=True, grad_premasked=True)
    M.nan_equal_bits(y.detach().cpu(), ref["y"], "conv + ReLU with a NaN input")
    y.backward(dev_cl(c["dy"]))
    E.assert_bits_equal(xg.grad.cpu(), ref["dx_masked"], "masked data gradient with a NaN in the mask")


def test_vgg_stem_exact(hip_lib):
    """scaling + image layer: forward bf16, the gradient back at the image in f32 with 3 channels"""
    from odvae_amd import ops
    c = M.conv_case(3, 64, 2, 9, 17)
    shift, scale = torch.tensor([0.5, -1.0, 0.0], dtype=torch.float64), torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)
    img = c["x"][:, :3] * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)        # exact: the scaled image is c["x"]
    ref = M.conv_case_references(c)
    xg = img.float().to(DEV).requires_grad_(True)
    y = ops.vgg_stem_bf16(xg, shift.float().to(DEV), scale.float().to(DEV), frozen(c["w"]), frozen(c["b"]), grad_premasked=True)
    E.assert_bits_equal(y.detach().cpu(), ref["y"], "stem y")
    y.backward(dev_cl(c["dy"]))
    assert xg.grad.dtype == torch.float32 and tuple(xg.grad.shape) == (2, 3, 9, 17)
    E.assert_bits_equal(xg.grad.cpu(), (ref["dx_f32"].double() / scale.view(1, -1, 1, 1)).float(), "stem dx")
    # self-contained form: the ReLU's own mask in a pass of its own
    xg2 = img.float().to(DEV).requires_grad_(True)
    ops.vgg_stem_bf16(xg2, shift.float().to(DEV), scale.float().to(DEV), frozen(c["w"]), frozen(c["b"])).backward(dev_cl(c["dy"]))
    pre_dy = torch.where(ref["y"].double() > 0, c["dy"], torch.zeros_like(c["dy"]))
    E.assert_bits_equal(xg2.grad.cpu(), (M.conv_dgrad(pre_dy, c["w"]) / scale.view(1, -1, 1, 1)).float(), "stem dx (self-contained)")


# ------------------------------------------------------------------------------------------------------------------------------
# max-pool
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(9, 11), (2, 2)], ids=lambda v: str(v))
@pytest.mark.parametrize("c", [64, 512])
def test_maxpool_bf16(hip_lib, h, w, c):
    from odvae_amd import ops
    x, dy, mask = M.pool_case(2, c, h, w)
    y_ref, dx_ref = M.pool_fwd(x), M.pool_bwd(x, dy)
    xg = dev_cl(x).requires_grad_(True)
    y = ops.maxpool2x2(xg)
    assert y.dtype == BF and tuple(y.shape) == (2, c, h // 2, w // 2)
    M.nan_equal_bits(y.detach().cpu(), y_ref.float().to(BF), "maxpool y")
    y.backward(dev_cl(dy))
    E.assert_bits_equal(xg.grad.cpu(), dx_ref.float().to(BF), "maxpool dx")
    # relu_mask: the mask is the input itself
    xg = dev_cl(x).requires_grad_(True)
    ops.maxpool2x2(xg, relu_mask=True).backward(dev_cl(dy))
    E.assert_bits_equal(xg.grad.cpu(), M.pool_bwd(x, dy, mask=x).float().to(BF), "maxpool dx masked with its input")
    # through the C ABI with a mask of its own: zeros at argmax positions that carry a gradient
    xd, dyd, md = dev_cl(x), dev_cl(dy), dev_cl(mask)
    dx = torch.full((2, h, w, c), float("nan"), dtype=BF, device=DEV)
    rc = hip_lib.odvae_maxpool2x2_bwd_bf16(xd.data_ptr(), dyd.data_ptr(), md.data_ptr(), dx.data_ptr(), 2, h, w, c, h // 2, w // 2, 0)
    assert rc == 0
    torch.cuda.synchronize()
    E.assert_bits_equal(dx.permute(0, 3, 1, 2).cpu(), M.pool_bwd(x, dy, mask=mask).float().to(BF), "maxpool dx with a mask (C ABI)")


# ------------------------------------------------------------------------------------------------------------------------------
# distance
# ------------------------------------------------------------------------------------------------------------------------------
def rounded_within(got, ref, tol, what):
    """got (bf16) is the rounding of some value within tol of ref (f32): rne is monotone, so rne(ref - tol) <= got <= rne(ref + tol)"""
    g = got.float().cpu().double()
    lo, hi = (ref.double() - tol).float().to(BF).double(), (ref.double() + tol).float().to(BF).double()
    bad = (g < lo) | (g > hi) | torch.isnan(g)
    assert not bad.any(), "%s: %d of %d elements outside; first got %r, reference %r +- %.3g" % (
        what, int(bad.sum()), bad.numel(), g[bad][0].item(), ref[bad][0].item(), tol)


@pytest.mark.parametrize("c,hw", [(64, 1), (64, 35), (512, 1), (512, 35), (128, 35), (256, 35)])
def test_lpips_distance_bf16(hip_lib, c, hw):
    from odvae_amd import ops
    from test_gan_lpips_gpu import close
    f0, f1, w, gw, dnext = dist_case(c, hw)
    zero = (f1.abs().sum(1, keepdim=True) == 0).expand_as(f1)
    assert int(zero.sum()) == c
    lin = frozen(w.view(1, c, 1, 1))
    d_ref = M.dist_fwd(f0, f1, w)
    for use_next in (False, True):
        for use_mask in (False, True):
            f1d = dev_cl(f1).requires_grad_(True)
            if use_next or use_mask:
                out = ops.lpips_tap_bf16(dev_cl(f0), f1d, lin, passthrough=use_next, relu_mask=use_mask)
                d, hp = out if use_next else (out, None)
            else:
                d, hp = ops.lpips_layer_distance(dev_cl(f0), f1d, lin), None
            assert d.dtype == torch.float32
            close(d, d_ref, 2e-5, "distance forward")
            if use_next:
                torch.autograd.backward([d, hp], [gw.to(DEV), dev_cl(dnext)])
            else:
                d.backward(gw.to(DEV))
            got = f1d.grad
            assert got.dtype == BF
            ref32 = _dist_bwd_f32(f0, f1, w, gw, dnext if use_next else None, f1 if use_mask else None)
            what = "distance backward C=%d HW=%d next=%s mask=%s" % (c, hw, use_next, use_mask)
            if use_mask:       # zero where f1 is zero -- at the all-zero feature vector everywhere -- and nowhere a huge value
                assert (got.cpu()[f1 == 0] == 0).all(), what + ": not zero where the mask is zero"
                live = ~zero
            else:              # at the all-zero vector the remaining term gs * gb / 1e-10 is of size 1e8: its own bound (5e-4 of the largest, the f32 edge test's, + one rounding: half a bf16 ulp <= 2^-8 |v|)
                gz, rz = got.float().cpu()[zero].double(), ref32[zero].double()
                assert torch.isfinite(gz).all() and ((gz - rz).abs() <= 5e-4 * rz.abs().max() + 2.0 ** -8 * rz.abs()).all(), what + ": at the zero vector"
                live = ~zero
            gmax = ref32[live].abs().max().item()
            rounded_within(got.cpu()[live], ref32[live], 2e-4 * gmax, what)


def _dist_bwd_f32(f0, f1, w, g, dnext, mask):
    """the host model's f32 value in front of its rounding (M.dist_bwd without the rne at its end)"""
    hw = f1.shape[2] * f1.shape[3]
    gs = (g / hw).view(-1, 1, 1, 1)
    s1 = torch.sqrt((f1 * f1).sum(1, keepdim=True))
    n1 = s1 + 1e-10
    ia, ib = 1.0 / (torch.sqrt((f0 * f0).sum(1, keepdim=True)) + 1e-10), 1.0 / n1
    gb = -2.0 * w.view(1, -1, 1, 1) * (f0 * ia - f1 * ib)
    dot = (gb * f1).sum(1, keepdim=True)
    coef = torch.where(s1 > 0, dot / (n1 * n1 * torch.where(s1 > 0, s1, torch.ones_like(s1))), torch.zeros_like(s1))
    o = gs * (gb * ib - coef * f1)
    if dnext is not None:
        o = o + dnext
    if mask is not None:
        o = M.apply_mask(o, mask)
    assert o.dtype == torch.float32
    return o


def test_distance_model_value_in_front_of_its_rounding():
    """(no device) _dist_bwd_f32 above is M.dist_bwd without its last line"""
    f0, f1, w, gw, dnext = dist_case(64, 35)
    assert torch.equal(M.rne(_dist_bwd_f32(f0, f1, w, gw, dnext, f1)), M.dist_bwd(f0, f1, w, gw, dnext=dnext, mask=f1))


# ------------------------------------------------------------------------------------------------------------------------------
# scaling layer
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 3, 1, 1), (2, 3, 9, 17), (1, 3, 1450, 1450)], ids=["1px", "2x9x17", "past-the-grid"])
def test_scaling_layer_bf16(hip_lib, shape):
    """y = bf16((x - shift) / scale), channels 3..7 zero.  Two f32 roundings in front of the bf16 one: the f32 value lies within
    (2^-24 |x - shift| / scale + 2^-24 |q|) of the float64 quotient q (half an ulp each), and the stored value is the rounding of such a
    value.  1450 x 1450 = 2 102 500 pixels, one thread each: past the grid cap of 8192 * 256."""
    from odvae_amd import ops
    g = M.gen(19, *shape)
    shift = torch.tensor([-.030, -.088, -.188])
    scale = torch.tensor([.458, .448, .450])
    x = torch.randn(shape, generator=g)
    y = ops.scale_shift(x.to(DEV), shift.view(1, 3, 1, 1).to(DEV), scale.view(1, 3, 1, 1).to(DEV), out_dtype=BF)
    assert y.dtype == BF and tuple(y.shape) == (shape[0], 8, shape[2], shape[3]) and y.stride(1) == 1
    y = y.cpu()
    assert (y[:, 3:] == 0).all()
    diff = x.double() - shift.double().view(1, 3, 1, 1)
    q = diff / scale.double().view(1, 3, 1, 1)
    tol = 2.0 ** -24 * diff.abs() / scale.double().view(1, 3, 1, 1) + 2.0 ** -24 * q.abs()
    g_ = y[:, :3].double()
    lo, hi = (q - tol).float().to(BF).double(), (q + tol).float().to(BF).double()
    assert ((g_ >= lo) & (g_ <= hi)).all(), "scaling layer: %d elements outside the two roundings" % int(((g_ < lo) | (g_ > hi)).sum())
    # and the model's own f32 arithmetic, which the whole-net comparison relies on
    same = torch.equal(y[:, :3], M.scaling_fwd(x, shift, scale).to(BF))
    print("scaling_layer_bf16 %s: equal to the host model's f32 arithmetic: %s" % (shape, same))


# ------------------------------------------------------------------------------------------------------------------------------
# the chain
# ------------------------------------------------------------------------------------------------------------------------------
def test_chain_exact(hip_lib):
    from odvae_amd import ops
    from test_gan_lpips_gpu import close
    c = M.chain_case()
    M.assert_chain_summable(c)
    ref = M.net(c["x0"], c["x1"], c["shift"], c["scale"], c["convs"], c["lins"], c["g"], c["g_pass"], dt=torch.float64)
    sh, sc = c["shift"].float().to(DEV), c["scale"].float().to(DEV)
    (w1, b1), (w2, b2) = [(frozen(w), frozen(b)) for w, b in c["convs"][0]]
    w3, b3 = [frozen(t) for t in c["convs"][1][0]]
    lin = frozen(c["lins"][1].view(1, -1, 1, 1))

    def branch(x, grad):
        h1 = ops.vgg_stem_bf16(x, sh, sc, w1, b1, grad_premasked=grad)
        h2 = ops.conv3x3_relu_bf16(h1, w2, b2, mask_input=grad, grad_premasked=grad)
        h3 = ops.maxpool2x2(h2, relu_mask=grad)          # no tap below: the pool carries the mask of the ReLU output it reads
        return h2, ops.conv3x3_relu_bf16(h3, w3, b3, mask_input=False, grad_premasked=grad)

    with torch.no_grad():
        _, f0 = branch(c["x0"].float().to(DEV), False)
    x1 = c["x1"].float().to(DEV).requires_grad_(True)
    t1, t2 = branch(x1, True)
    E.assert_bits_equal(t1.detach().cpu(), ref["taps"][0].float().to(BF), "chain: features in front of the pool")
    E.assert_bits_equal(t2.detach().cpu(), ref["taps"][1].float().to(BF), "chain: tap features")
    seen = {}
    t2.register_hook(lambda g: seen.__setitem__("dtap", g.detach().clone()))
    d, hp = ops.lpips_tap_bf16(f0, t2, lin, passthrough=True, relu_mask=True)
    close(d, ref["d"].float(), 2e-5, "chain: distance")
    torch.autograd.backward([d, hp], [c["g"].float().to(DEV), dev_cl(c["g_pass"])])
    E.assert_bits_equal(seen["dtap"].cpu(), ref["dtaps"][1].float().to(BF), "chain: gradient stored at the tap")
    assert x1.grad.dtype == torch.float32
    E.assert_bits_equal(x1.grad.cpu(), ref["dx"].float(), "chain: image gradient")


# ------------------------------------------------------------------------------------------------------------------------------
# the whole net
# ------------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_lpips(h, w):
    """d and d/dx1 from the CPU oracle in f32 and under autocast, once per size"""
    if (h, w) not in _ORACLE:
        from oracle.losses import LPIPSStyle as RefL
        from odvae_amd.gan import LPIPSStyle
        net = LPIPSStyle()
        ref = RefL()
        res = ref.load_state_dict(net.state_dict(), strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        ref.eval()
        g = M.gen(31, h, w)
        x0 = torch.rand(2, 3, h, w, generator=g) * 2 - 1
        x1 = (x0 + 0.3 * torch.randn(2, 3, h, w, generator=g)).clamp(-1, 1)
        out = {}
        for name, ac in (("f32", False), ("autocast", True)):
            x1r = x1.clone().requires_grad_(True)
            if ac:
                with torch.autocast("cpu", dtype=torch.bfloat16):
                    d = ref(x0, x1r)
            else:
                d = ref(x0, x1r)
            d.float().sum().backward()
            out[name] = (d.detach().float().reshape(-1), x1r.grad.float())
        _ORACLE[(h, w)] = (net, x0, x1, out)
    return _ORACLE[(h, w)]


@pytest.mark.parametrize("h,w", [(36, 44), (24, 40), (72, 72)], ids=lambda v: str(v))
def test_lpips_bf16_is_as_close_to_f32_as_autocast(hip_lib, h, w):
    """err_hip <= 2 err_autocast for the value (max over the batch, relative) and for the gradient (relative L2); gradient cosine with
    the f32 gradient >= min(0.98, cos_autocast - 0.01).  No floors."""
    net, x0, x1, out = oracle_lpips(h, w)
    net = net.to(DEV).eval().set_precision("bf16")
    assert net.compute_dtype == BF and net.scaling_layer.compute_dtype == BF
    assert all(v.dtype == torch.float32 for v in net.state_dict().values())
    x1d = x1.to(DEV).requires_grad_(True)
    d = net(x0.to(DEV), x1d)
    assert d.dtype == torch.float32 and tuple(d.shape) == (2, 1, 1, 1)
    d.sum().backward()
    grad = x1d.grad.cpu()
    assert grad.dtype == torch.float32 and torch.isfinite(grad).all()
    (d32, g32), (dac, gac) = out["f32"], out["autocast"]
    relv = lambda a: ((a - d32).abs() / d32.abs()).max().item()
    rell2 = lambda a: ((a - g32).norm() / g32.norm()).item()
    cos = lambda a: (a.flatten().double() @ g32.flatten().double() / (a.double().norm() * g32.double().norm())).item()
    dh = d.detach().cpu().reshape(-1)
    print("lpips bf16 %dx%d: value error hip %.3e autocast %.3e | gradient rel. L2 hip %.3e autocast %.3e | cosine hip %.5f autocast %.5f" % (
        h, w, relv(dh), relv(dac), rell2(grad), rell2(gac), cos(grad), cos(gac)))
    assert relv(dh) <= 2 * relv(dac), "value: hip %.3e, autocast %.3e" % (relv(dh), relv(dac))
    assert rell2(grad) <= 2 * rell2(gac), "gradient: hip %.3e, autocast %.3e" % (rell2(grad), rell2(gac))
    assert cos(grad) >= min(0.98, cos(gac) - 0.01), "gradient cosine: hip %.5f, autocast %.5f" % (cos(grad), cos(gac))
    # the no-gradient form (both branches without a graph) computes the same value
    with torch.no_grad():
        d2 = net(x0.to(DEV), x1.to(DEV))
    assert torch.equal(d2, d.detach())
    net.set_precision(32)
    assert net.compute_dtype == torch.float32 and net.scaling_layer.compute_dtype == torch.float32


def count_packs(monkeypatch, ops):
    """-> list that receives id(weight) of every weight-pack launch from now on"""
    seen, real = [], ops._pack_conv3x3_now

    def counted(weight, *a, **k):
        seen.append(id(weight))
        return real(weight, *a, **k)
    monkeypatch.setattr(ops.packs, "_pack_conv3x3_now", counted)     # where the pack cache looks it up
    return seen


def test_frozen_packs_are_built_once(hip_lib, monkeypatch):
    """The VGG weights are frozen: their bf16 packs are made at the first forward that needs them and never again, whatever the optimizer
    epoch does; load_weights makes them stale."""
    from odvae_amd import ops
    from odvae_amd.gan import LPIPSStyle, VGG16_SLICES
    net = LPIPSStyle().to(DEV).eval().set_precision("bf16")
    g = M.gen(7)
    x0 = (torch.rand(1, 3, 16, 16, generator=g) * 2 - 1).to(DEV)
    x1 = (torch.rand(1, 3, 16, 16, generator=g) * 2 - 1).to(DEV).requires_grad_(True)
    net(x0, x1).sum().backward()
    convs = [m for m in net.net.modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == 13
    before = {id(m): ops.PACK_CACHE.get(m.weight, True, "bf16")[0].clone() for m in convs}
    seen = count_packs(monkeypatch, ops)
    for _ in range(3):
        ops.PACK_CACHE.bump()           # an optimizer step of the trainable networks
        x1.grad = None
        net(x0, x1).sum().backward()
    assert not seen, "%d pack launches for frozen weights after the first step" % len(seen)
    sd = {}
    for name, layers in VGG16_SLICES:
        for idx, _, _ in layers:
            conv = getattr(getattr(net.net, name), str(idx))
            sd["features.%d.weight" % idx] = conv.weight.detach().cpu() * 0.5
            sd["features.%d.bias" % idx] = conv.bias.detach().cpu()
    net.load_weights(vgg16=sd)
    f, _ = ops.PACK_CACHE.get(convs[0].weight, True, "bf16")
    assert seen == [id(convs[0].weight)] and not torch.equal(f, before[id(convs[0])]), "load_weights left a stale pack"


# ------------------------------------------------------------------------------------------------------------------------------
# the training step
# ------------------------------------------------------------------------------------------------------------------------------
def _gan_step(model, batch, noise):
    model.zero_grad(set_to_none=True)
    model._global_step = 1
    model.injected_noise = noise
    loss = model.training_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}, 0, 0)
    loss.backward()
    logs = {k: float(v) for k, v in model.logged_metrics.items() if k.startswith("train/") and (not torch.is_tensor(v) or v.numel() == 1)}
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    return loss.detach().clone(), logs, grads


def test_gan_step_with_bf16_perceptual_net(hip_lib):
    """ch = 32 at 64 x 64, B = 2, perceptual_weight 1, discriminator on, generator step.  The logged terms and the parameter gradients by
    the rule of tests/test_bf16_model_gpu.py against the f32 oracle; two runs bit-identical; with the switch off again, the values of a
    model that never had it on, bit for bit."""
    from test_model_gpu import build_pair
    from test_bf16_model_gpu import rel, run_oracle, flat
    from odvae_amd import synthetic
    model, ref = build_pair(perceptual_weight=1.0, disc_factor=1.0, ch=32, latent_hw=4)
    plain, _ = build_pair(perceptual_weight=1.0, disc_factor=1.0, ch=32, latent_hw=4)
    model.train(); ref.train(); plain.train()
    ref.loss.perceptual_loss.eval()          # (the product pins its perceptual net to eval mode: tests/test_model_gpu.py)
    ref.global_step = 1
    batch = synthetic.make_batch(2, 64, seed=5)
    noise = synthetic.make_noise(2, 4, dropout_p=0.7, seed=6)
    l32, log32, _, g32 = run_oracle(ref, batch, noise, False)
    lac, logac, _, gac = run_oracle(ref, batch, noise, True)

    plain.set_precision("bf16")
    assert plain.loss.perceptual_loss.compute_dtype == torch.float32
    base = _gan_step(plain, batch, noise)

    model.set_precision("bf16", perceptual_precision="bf16")
    assert model.loss.perceptual_loss.compute_dtype == BF and model.encoder.compute_dtype == BF
    run1 = _gan_step(model, batch, noise)
    run2 = _gan_step(model, batch, noise)
    assert torch.equal(run1[0], run2[0]) and run1[1] == run2[1]
    assert set(run1[2]) == set(run2[2]) and all(torch.equal(run1[2][k], run2[2][k]) for k in run1[2])

    loss, logs, grads = run1
    report, failed = [], []
    def check(name, got, want, ac, floor, base_value=None):
        e, eac = rel(got, want), rel(ac, want)
        line = "%s: hip %.3e autocast %.3e" % (name, e, eac)
        if base_value is not None:
            line += " (perceptual net in f32: %.3e)" % rel(base_value, want)
        report.append(line)
        if not e <= 2 * eac + floor:
            failed.append("%s: bf16 HIP path %.3e from the f32 oracle, autocast oracle %.3e (floor %.0e)" % (name, e, eac, floor))
    check("total loss", loss, l32, lac, 1e-2, base[0])
    # d_weight is no loss term: it is the quotient of two gradient norms at the last layer (contperceptual.py calculate_adaptive_weight),
    # so it is held to that file's floor for gradients, 5e-2, the loss terms to its floor for loss terms, 1e-2.  (Measured: 4.07e-2 from the
    # f32 oracle, autocast 1.16e-2 -- and 4.07e-2 just the same with the perceptual net in f32: the figure is the bf16 Decoder's.)
    for key in sorted(k for k in log32 if k in logs and k in logac):
        check(key, torch.as_tensor(logs[key]), torch.as_tensor(log32[key]), torch.as_tensor(logac[key]),
              5e-2 if key == "train/d_weight" else 1e-2, torch.as_tensor(base[1][key]))
    print("\n".join(report))
    assert not failed, "; ".join(failed)
    assert {"train/nll_loss", "train/rec_loss", "train/g_loss", "train/d_weight"} <= {k for k in log32 if k in logs}
    keys = [k for k in g32 if k in grads]
    assert {k.split(".")[0] for k in keys} >= {"encoder", "decoder", "quant_conv_obj", "post_quant_conv"}
    ghip = {k: grads[k].cpu().float() for k in keys}
    for k in keys:
        assert torch.isfinite(ghip[k]).all(), k
    v32, vhip, vac = flat(g32, keys), flat(ghip, keys), flat(gac, keys)
    cos = lambda a, b: (a @ b / (a.norm() * b.norm())).item()
    c_hip, c_ac = cos(vhip, v32), cos(vac, v32)
    report.append("gradient cosine: hip %.5f autocast %.5f" % (c_hip, c_ac))
    print(report[-1])
    assert c_hip >= min(0.98, c_ac - 0.01), report[-1]
    energy = v32.pow(2).sum().item()
    for k in keys:
        if g32[k].double().pow(2).sum().item() < 1e-3 * energy:
            continue
        e, eac = rel(ghip[k], g32[k]), rel(gac[k], g32[k])
        assert e <= 2 * eac + 5e-2, "grad %s: hip %.3e autocast %.3e" % (k, e, eac)

    model.set_precision("bf16", perceptual_precision=32)
    assert model.loss.perceptual_loss.compute_dtype == torch.float32
    off = _gan_step(model, batch, noise)
    assert torch.equal(off[0], base[0]) and off[1] == base[1], "switch off: the step differs from a model that never had the switch on"
    assert set(off[2]) == set(base[2]) and all(torch.equal(off[2][k], base[2][k]) for k in base[2])
    assert any(not torch.equal(run1[2][k], base[2][k]) for k in base[2]), "the switch changes nothing"     # (the total, ~1e6, need not move by an f32 ulp)


def test_gan_batch_with_bf16_perceptual_net_never_synchronises_the_host(hip_lib, monkeypatch):
    """As tests/test_model_gpu.py::test_training_batch_never_synchronises_the_host, with the perceptual net on its bf16 kernels: after
    two warm-up batches (packs, workspaces) a whole generator + discriminator batch issues without one host synchronisation, and the
    frozen VGG weights are not packed again, whatever the two optimizer steps in between do to the pack cache's epoch."""
    import warnings
    from test_model_gpu import YAML
    from odvae_amd import ops, synthetic
    from odvae_amd.trainer import Trainer
    torch.manual_seed(23)
    model = synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=4, ch=32, perceptual_weight=1.0, disc_factor=1.0, disc_start=0).to(DEV).train()
    model._global_step = 1
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1), precision="bf16", perceptual_precision="bf16")
    batch = synthetic.make_batch(2, 64, seed=23)
    batch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}

    def step(i):
        b = dict(batch)
        b["pose_6d"] = batch["pose_6d"].clone()
        return trainer.training_batch(b, i)
    convs = [m for m in model.loss.perceptual_loss.net.modules() if isinstance(m, torch.nn.Conv2d)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(2):
            step(i)
        torch.cuda.synchronize()
        seen = count_packs(monkeypatch, ops)
        torch.cuda.set_sync_debug_mode("error")
        try:
            losses = step(2)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert all(torch.isfinite(l).all() for l in losses)
    vgg = {id(m.weight) for m in convs}
    assert len(seen) > 0 and not vgg & set(seen), "%d pack launches for frozen VGG weights in a steady-state batch" % len(vgg & set(seen))


def test_precision_switch_plumbing(hip_lib, monkeypatch):
    from test_model_gpu import build_pair
    from odvae_amd import ops
    from odvae_amd.trainer import Trainer
    model, _ = build_pair(perceptual_weight=1.0, disc_factor=1.0)
    lp = model.loss.perceptual_loss
    assert lp.compute_dtype == torch.float32
    model.set_precision("bf16")
    assert lp.compute_dtype == torch.float32, "precision: bf16 alone must leave the perceptual net f32"
    Trainer(model, precision="bf16", perceptual_precision="bf16")
    assert lp.compute_dtype == BF
    Trainer(model, precision="bf16")
    assert lp.compute_dtype == BF, "perceptual_precision=None leaves the perceptual net alone"
    model.set_precision(32, perceptual_precision=32)
    assert lp.compute_dtype == torch.float32
    monkeypatch.setattr(ops, "LPIPS_BF16", True)       # ODVAE_LPIPS_BF16=1
    model.set_precision("bf16")
    assert lp.compute_dtype == BF
    model.set_precision(32)
    assert lp.compute_dtype == torch.float32
    with pytest.raises(ValueError):
        lp.set_precision(16)
