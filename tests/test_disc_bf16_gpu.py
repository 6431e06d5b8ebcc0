"""The opt-in bf16 PatchGAN discriminator (gan.NLayerDiscriminator.set_precision("bf16")): the 16-tap implicit-GEMM convolutions of
conv_bf16.hip (modes 5 / 6 / 7) and conv_wgrad_bf16.hip (modes 5 / 6), BatchNorm + LeakyReLU of gan_norm.hip.

Per kernel, bit for bit against float64 on exactly summable operands (tests/conv4x4_bf16_inputs.py, recipe A; recipe L for the fused
LeakyReLU): forward, data gradient, weight gradient and bias gradient at every shape of M.CASES -- an f32 output equals the reference,
a bf16 output the reference rounded once.  The 3-channel image comes to the kernels zero-padded to 8 channels; a ragged Cout (36, 1)
comes to the data- and weight-gradient kernels as a dy zero-padded to the next multiple of 8, as ops._Conv4x4B pads an f32 dy.
One weight-gradient case runs several pixel splits with a short last one (asserted on the library's plan).  A planted NaN reaches
exactly the outputs whose window holds it.  BatchNorm + LeakyReLU: see the bound derived at `bn_bounds`.
Whole net, GAN batch, plumbing: the rule of tests/test_bf16_model_gpu.py.
On the parent commit everything here fails: there is no odvae_conv4x4_bf16 and no NLayerDiscriminator.set_precision.
"""
import pytest
import torch

import exact_inputs as E
import conv4x4_bf16_inputs as M
import gn_offset_inputs as G
import bn_offset_inputs as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
CL = torch.channels_last


def dev_cl(t, dtype=BF):
    return t.to(dtype).to(DEV).contiguous(memory_format=CL)


def pad_channels(t, mult=8):
    c = t.shape[1]
    cp = (c + mult - 1) // mult * mult
    return t if cp == c else torch.cat([t, torch.zeros(t.shape[0], cp - c, t.shape[2], t.shape[3], dtype=t.dtype)], 1)


def run_kernels(c, out_f32, dx_f32, slope=0.0, dy=None):
    """The four kernels on case c through the op layer's raw launchers and the C ABI: (y, dx, dw, db) on the host.
    dy: the upstream gradient the data- and weight-gradient kernels read (default c["dy"])."""
    from odvae_amd import lib, ops
    L = lib.load()
    s = c["stride"]
    n, cin, h, w = c["x"].shape
    cout = c["w"].shape[0]
    ho, wo = M.out4(h, s), M.out4(w, s)
    xd = dev_cl(pad_channels(c["x"]))
    wt = c["w"].float().to(DEV)
    b = c["b"].float().to(DEV) if c["b"] is not None else None
    fwd, dgr = ops._pack_conv3x3_now(wt, True, True, "bf16")
    y = ops._conv4x4_b_raw(s, False, xd, fwd, cout, b, ho, wo, out_f32, slope)
    dyd = dev_cl(pad_channels(c["dy"] if dy is None else dy))
    dx = ops._conv4x4_b_raw(s, True, dyd, dgr, cin, None, h, w, dx_f32)
    cx, cp = xd.shape[1], dyd.shape[1]
    mode = 5 if s == 1 else 6
    dw = torch.full((cp, cx, 4, 4), float("nan"), device=DEV)
    db = torch.full((cp,), float("nan"), device=DEV)
    need = L.odvae_conv_wgrad_bf16_workspace_bytes(mode, n, ho, wo, cx, cp)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    lib.check(L.odvae_conv_wgrad_bf16(mode, xd.data_ptr(), dyd.data_ptr(), n, h, w, cx, ho, wo, cp, dw.data_ptr(), db.data_ptr(),
                                      ws.data_ptr(), need, lib.stream_ptr()), "conv_wgrad_bf16")
    dw, db = dw.cpu(), db.cpu()
    assert not dw[cout:].any() and not dw[:, cin:].any() and not db[cout:].any(), "padding channels of dw / db are not zero"
    return y.cpu(), dx.cpu(), dw[:cout, :cin].contiguous(), db[:cout].contiguous()


def check_case(c, what, lrelu=False):
    cin, cout = c["w"].shape[1], c["w"].shape[0]
    out_f32, dx_f32 = cout % 4 != 0, cin % 4 != 0
    ref = M.references(c, out_f32=out_f32, dx_f32=dx_f32, lrelu=lrelu)
    cc = c
    if lrelu:     # the backward kernels read g = round(dy * lrelu'): multiples of 2^-10 (bf16(0.2) = 205 * 2^-10 times an integer)
        cc = dict(c, dy=ref["g"], units=dict(c["units"], dy=2.0 ** -10))
    s = M.assert_exactly_summable(cc)
    y, dx, dw, db = run_kernels(c, out_f32, dx_f32, M.SLOPE if lrelu else 0.0, dy=ref["g"] if lrelu else None)
    print("%s: worst sum %.3g of 2^24 units; y off the bf16 grid %.2f, ties %.3f" % ((what, s["worst"]) + E.rounding_profile(ref["y_exact"])))
    E.assert_bits_equal(y, ref["y"], what + " y")
    E.assert_bits_equal(dx, ref["dx"], what + " dx")
    E.assert_bits_equal(dw, ref["dw"], what + " dw")
    E.assert_bits_equal(db, ref["db"], what + " db")
    return ref


@pytest.mark.parametrize("case", M.CASES, ids=[c[0] for c in M.CASES])
def test_conv4x4_kernels_exact(hip_lib, case):
    name, stride, n, cin, cout, h, w, bias = case
    check_case(M.make_case(stride, n, cin, cout, h, w, bias=bias), name)


def test_wgrad_with_several_splits_and_a_short_last_one(hip_lib):
    from odvae_amd import lib
    name, stride, n, cin, cout, h, w, bias = M.WGRAD_SPLIT_CASE
    plan = lib.conv_wgrad_bf16_plan(5, n, M.out4(h, stride), M.out4(w, stride), cin, cout)
    print(plan)
    assert plan["nsplit"] >= 2 and plan["ntiles"] > plan["nsplit"] and plan["ntiles"] % plan["nsplit"] != 0, plan
    check_case(M.make_case(stride, n, cin, cout, h, w, bias=bias), name)


@pytest.mark.parametrize("n,cin,cout,h,w", [(2, 3, 64, 9, 11), (1, 8, 128, 36, 44)], ids=["image-64", "8-128-tiles"])
def test_fused_lrelu_epilogue_exact(hip_lib, n, cin, cout, h, w):
    """LeakyReLU(0.2) on the f32 accumulator, then the one rounding: accumulators are multiples of 5 units, negative ones included, and a
    kernel that rounded first would differ (asserted on the reference itself)"""
    c = M.make_case(2, n, cin, cout, h, w, bias=True, recipe="L")
    ref = check_case(c, "lrelu %d->%d" % (cin, cout), lrelu=True)
    acc = ref["y_exact"]
    assert (acc < 0).any() and torch.equal(torch.round(acc / 0.625) * 0.625, acc)
    assert not torch.equal(M.lrelu_f64(acc, "lrelu_after_round"), ref["y"]), "these inputs cannot tell the two orders apart"
    # the elementwise backward of the epilogue
    from odvae_amd import lib
    L = lib.load()
    yd, dyd = dev_cl(ref["y"]), dev_cl(c["dy"])
    g = torch.empty_like(dyd)
    lib.check(L.odvae_leaky_relu_bwd_bf16(yd.data_ptr(), dyd.data_ptr(), g.data_ptr(), M.SLOPE, dyd.numel(), lib.stream_ptr()), "lrelu bwd")
    E.assert_bits_equal(g.cpu(), M.lrelu_bwd_f32(ref["y"], c["dy"]), "leaky_relu_bwd_bf16", summed=False)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("where", ["interior", "corner"])
def test_a_nan_reaches_exactly_its_windows(hip_lib, stride, where):
    from odvae_amd import ops
    n, cin, cout, h, w = 2, 16, 40, 11, 19
    c = M.make_case(stride, n, cin, cout, h, w, bias=True)
    iy, ix = (5, 9) if where == "interior" else (h - 1, w - 1)
    ref = M.references(c)
    x = c["x"].clone()
    x[1, 3, iy, ix] = float("nan")
    wt = c["w"].float().to(DEV)
    fwd, _ = ops._pack_conv3x3_now(wt, True, False, "bf16")
    ho, wo = M.out4(h, stride), M.out4(w, stride)
    for slope in ((0.0, M.SLOPE) if stride == 2 else (0.0,)):
        y = ops._conv4x4_b_raw(stride, False, dev_cl(x), fwd, cout, c["b"].float().to(DEV), ho, wo, False, slope).cpu()
        foot = M.nan_footprint((ho, wo), stride, iy, ix)
        assert 1 <= int(foot.sum()) <= 16
        nan = torch.isnan(y.float())
        assert torch.equal(nan[1], foot.unsqueeze(0).expand(cout, ho, wo)) and not nan[0].any(), "NaN footprint (slope %g)" % slope
        if slope == 0.0:
            keep = ~nan
            E.assert_bits_equal(torch.where(keep, y, torch.zeros_like(y)), torch.where(keep, ref["y"], torch.zeros_like(y)), "y beside the NaN")


def test_conv4x4_bf16_op_first_layer_and_head(hip_lib):
    """The autograd Function: the f32 image in, LeakyReLU fused, the f32 3-channel gradient out; the head's f32 logits and f32 upstream
    gradient (cast once; the bias gradient sums the f32 values)."""
    from odvae_amd import ops
    c = M.make_case(2, 2, 3, 64, 9, 11, bias=True, recipe="L")
    ref = M.references(c, dx_f32=True, lrelu=True)
    M.assert_exactly_summable(dict(c, dy=ref["g"], units=dict(c["units"], dy=2.0 ** -10)))
    wt = torch.nn.Parameter(c["w"].float().to(DEV)); bs = torch.nn.Parameter(c["b"].float().to(DEV))
    x = c["x"].float().to(DEV).requires_grad_(True)
    y = ops.conv4x4_bf16(x, wt, bs, 2, lrelu=M.SLOPE)
    assert y.dtype == BF and [tuple(t.shape) for t in y.grad_fn.saved_tensors if t is not None and t.dtype == BF][0] == (2, 8, 9, 11)
    y.backward(dev_cl(c["dy"]))
    E.assert_bits_equal(y.detach().cpu(), ref["y"], "first layer y")
    assert x.grad.dtype == torch.float32 and tuple(x.grad.shape) == (2, 3, 9, 11)
    E.assert_bits_equal(x.grad.cpu(), ref["dx"], "first layer dx")
    E.assert_bits_equal(wt.grad.cpu(), ref["dw"], "first layer dw")
    E.assert_bits_equal(bs.grad.cpu(), ref["db"], "first layer db")

    c = M.make_case(1, 1, 512, 1, 5, 6, bias=True)
    dy32, unit = E.f32_gradient(c["dy"].shape)
    M.assert_exactly_summable(c, dy32, unit)
    ref = M.references(c, out_f32=True, dy_f32=dy32)
    wt = torch.nn.Parameter(c["w"].float().to(DEV)); bs = torch.nn.Parameter(c["b"].float().to(DEV))
    x = dev_cl(c["x"]).requires_grad_(True)
    y = ops.conv4x4_bf16(x, wt, bs, 1)
    assert y.dtype == torch.float32
    y.backward(dy32.float().to(DEV))
    E.assert_bits_equal(y.detach().cpu(), ref["y"], "head y")
    E.assert_bits_equal(x.grad.cpu(), ref["dx"], "head dx")
    E.assert_bits_equal(wt.grad.cpu(), ref["dw"], "head dw")
    E.assert_bits_equal(bs.grad.cpu(), ref["db"], "head db")


# ------------------------------------------------------------------------------------------------------------------------------
# BatchNorm + LeakyReLU on bf16 activations
# ------------------------------------------------------------------------------------------------------------------------------
EPS24 = 2.0 ** -24
WRAP_ROWS = 1024 * 128 + 1      # bn_colstats: at most 1024 blocks of rows / 128 rows; one row more and every block walks 129


def bn_input(rows, c, r):
    """[1, c, rows, 1] of bf16 numbers.  r = 0: randn rounded.  r = 1000: 1000 sign_c + 4 t, t in {-1, 0, 1} with P(+-1) = 1/32 each --
    1000 +- 4 are neighbouring bf16 numbers, the spread's standard deviation is 4 sqrt(2/32) = 1: the mean lies 1000 standard
    deviations from zero IN the stored values."""
    g = torch.Generator().manual_seed(G.seed_of((1, c, rows, 1), r, 1.0, 29))
    if r == 0:
        x = torch.randn(1, c, rows, 1, generator=g)
    else:
        u = torch.rand(1, c, rows, 1, generator=g)
        t = (u < 1 / 32).float() - (u > 31 / 32).float()
        x = r * B.channel_signs(c).view(1, c, 1, 1) + 4 * t
    x = x.to(BF).float()
    assert torch.equal(x.to(BF).float(), x)
    return x


def bn_bounds(x, gamma, beta, mean, rstd, dy, sum_g, sum_gxh, train):
    """float64 evaluation of the kernels' formulas on the stored bf16 x, dy with the DEVICE's f32 mean, rstd (and, backward, its f32 sums),
    and the bound on |stored bf16 - that|.  e = 2^-24 (one f32 rounding, relative); every f32 operation rounds once.
    forward  t = ((x - mean) rstd) gamma: 3 roundings, |err| <= 4 e |t| (first order, 3 e, rounded up for the second-order terms);
             u = t + beta: + e |u|; y = u or 0.2f u (0.2f is within e of 0.2, the product rounds once: 2 e |y|, LeakyReLU is 1-Lipschitz,
             so a sign of u that differs between the two evaluations costs no more): E_y = e (4 |t| + 3 |u|).
             The store rounds once to bf16: at most half an ulp, 2^-8 of the f32 value's magnitude: bound = E_y + 2^-8 (|y64| + E_y).
    backward xh: 2 roundings; g = dy or 0.2f dy: 2 e |g|; p = xh sum_gxh: 3 e |p|; q = sum_g + p: e more on each; (q) inv_m with
             inv_m = fl(1 / M): 2 more; v = g - q / M: 1 more; dx = (gamma rstd) v: 2 more.  No term passes more than 10 roundings:
             E_dx = 10 e |gamma rstd| (|g| + (|sum_g| + |xh sum_gxh|) / M); eval mode has only the g term.
             bound = E_dx + 2^-8 (|dx64| + E_dx)."""
    c = x.shape[1]
    v = lambda t: t.double().view(1, c, 1, 1)
    xd, m = x.double(), float(x.numel() // c)
    xh = (xd - v(mean)) * v(rstd)
    t = xh * v(gamma)
    u = t + v(beta)
    y = torch.where(u > 0, u, u * 0.2)
    e_y = EPS24 * (4 * t.abs() + 3 * u.abs())
    out = {"y": y, "y_bound": e_y + 2.0 ** -8 * (y.abs() + e_y), "u": u}
    if dy is not None:
        g = dy.double() * torch.where(u > 0, 1.0, 0.2)
        if train:
            q = (v(sum_g) + xh * v(sum_gxh)) / m
            mag = g.abs() + (v(sum_g).abs() + (xh * v(sum_gxh)).abs()) / m
        else:
            q, mag = 0.0, g.abs()
        dx = v(gamma) * v(rstd) * (g - q)
        e_dx = 10 * EPS24 * (v(gamma) * v(rstd)).abs() * mag
        out.update({"dx": dx, "dx_bound": e_dx + 2.0 ** -8 * (dx.abs() + e_dx)})
    return out


def inside(got, want, bound, what):
    err = (got.detach().cpu().double() - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print("%s: max |err| %.3e, max err / bound %.3f" % (what, err.max().item(), worst))
    assert torch.isfinite(got).all() and bool((err <= bound).all()), "%s: err / bound up to %.3f" % (what, worst)


# (63, 7): odd C, one element per thread in every pass; (63, 263): odd C past one 256-channel pass; (63, 520): C / 2 = 260 pairs, a second
# pass 4 pairs wide, 8-element apply
BN_SHAPES = [(1, 8), (1, 36), (1, 512), (63, 8), (63, 36), (63, 512), (WRAP_ROWS, 8), (63, 7), (63, 263), (63, 520)]


@pytest.mark.parametrize("r", [0, 1000])
@pytest.mark.parametrize("rows,c", BN_SHAPES, ids=lambda v: str(v))
def test_batchnorm_lrelu_bf16_training(hip_lib, rows, c, r):
    from odvae_amd import ops
    from test_batchnorm_offset_gpu import holder, backward_figures
    x = bn_input(rows, c, r)
    gamma, beta = B.affine(c)
    rm0, rv0 = B.running_start(c)
    mean64, var64, rstd64 = B.stats64(x)
    if rows > 1:
        _, rm64, rv64 = B.ref64(x, gamma, beta, rm0, rv0)
        _, rm32, rv32, mean32, rstd32 = B.ref32(x, gamma, beta, rm0, rv0)
    else:             # one row (torch refuses one value per channel in training mode): mean = x, var = 0, by hand
        mean32, rstd32 = B.rows_of(x)[0].clone(), torch.full((c,), float(1.0 / torch.sqrt(torch.tensor(B.EPS, dtype=torch.float32))))
    bn = holder(c, gamma, beta, rm0, rv0, True)
    xd = x.to(BF).to(DEV).requires_grad_(True)
    y = ops.batchnorm_lrelu(xd, bn, B.SLOPE)
    assert y.dtype == BF and int(bn.num_batches_tracked) == 1
    mean, rstd = (t.cpu() for t in y.grad_fn.saved_tensors[3:5])
    assert mean.dtype == torch.float32 and rstd.dtype == torch.float32
    what = "bn bf16 rows %d C %d r %d" % (rows, c, r)
    figs = G.stat_figures(mean, rstd, mean64, rstd64, mean32, rstd32)
    if rows > 1:      # (one row: the unbiased variance is 0 / 0 in torch's reference)
        std64 = (var64 + B.EPS).sqrt()
        figs.append(G.figure("running_mean / std64", bn.running_mean.cpu().double() / std64, rm64 / std64, rm32.double() / std64, G.FLOOR_FWD))
        figs.append(G.figure("running_var / var64", bn.running_var.cpu().double() / (var64 + B.EPS), rv64 / (var64 + B.EPS), rv32.double() / (var64 + B.EPS), G.FLOOR_FWD))
        # the f32 path on the same (bf16-valued) inputs moves the running statistics to the same place, by the same rule
        bn32 = holder(c, gamma, beta, rm0, rv0, True)
        ops.batchnorm_lrelu(x.to(DEV), bn32, B.SLOPE)
        figs.append(G.figure("running_mean vs f32 path / std64", bn.running_mean.cpu().double() / std64, bn32.running_mean.cpu().double() / std64, rm32.double() / std64 + (bn32.running_mean.cpu().double() - rm64) / std64, G.FLOOR_FWD))
        figs.append(G.figure("running_var vs f32 path / var64", bn.running_var.cpu().double() / (var64 + B.EPS), bn32.running_var.cpu().double() / (var64 + B.EPS), rv32.double() / (var64 + B.EPS) + (bn32.running_var.cpu().double() - rv64) / (var64 + B.EPS), G.FLOOR_FWD))
    pre = bn_bounds(x, gamma, beta, mean, rstd, None, None, None, True)
    dy = B.kink_free_dy(pre["u"], G.seed_of(x.shape, 0, 1.0, 19)).to(BF).float()
    y.backward(dy.to(BF).to(DEV))
    dgamma, dbeta = bn.weight.grad.cpu(), bn.bias.grad.cpu()
    assert xd.grad.dtype == BF and dgamma.dtype == torch.float32
    if rows > 1:
        figs += backward_figures((xd.grad.float(), dgamma, dbeta), B.backward_refs(x, gamma, beta, dy))[1:]
    else:             # one row: dbeta is the one g, dgamma = g xhat with xhat = 0 up to the rounding of the mean (here exact)
        g1 = (B.rows_of(dy)[0] * torch.where(B.rows_of(pre["u"])[0] > 0, 1.0, 0.2).float())
        assert torch.equal(dbeta, g1) and not dgamma.any()
    G.check(figs, what)
    bd = bn_bounds(x, gamma, beta, mean, rstd, dy, dbeta, dgamma, True)
    inside(y.float(), bd["y"], bd["y_bound"], what + " y")
    inside(xd.grad.float(), bd["dx"], bd["dx_bound"], what + " dx")


@pytest.mark.parametrize("rows,c", [(63, 36), (63, 512), (1, 8)], ids=lambda v: str(v))
def test_batchnorm_lrelu_bf16_eval(hip_lib, rows, c):
    from odvae_amd import ops
    from test_batchnorm_offset_gpu import holder, backward_figures
    x = bn_input(rows, c, 0)
    gamma, beta = B.affine(c)
    rm0, rv0 = B.running_start(c)
    bn = holder(c, gamma, beta, rm0, rv0, False)
    xd = x.to(BF).to(DEV).requires_grad_(True)
    y = ops.batchnorm_lrelu(xd, bn, B.SLOPE)
    assert int(bn.num_batches_tracked) == 0 and torch.equal(bn.running_mean.cpu(), rm0) and torch.equal(bn.running_var.cpu(), rv0)
    mean, rstd = (t.cpu() for t in y.grad_fn.saved_tensors[3:5])
    assert torch.equal(mean, rm0)
    assert (rstd.double() - 1 / torch.sqrt(rv0.double() + B.EPS)).abs().max().item() <= 4 * EPS24 * rstd.abs().max().item()
    pre = bn_bounds(x, gamma, beta, mean, rstd, None, None, None, False)
    dy = B.kink_free_dy(pre["u"], 31).to(BF).float()
    y.backward(dy.to(BF).to(DEV))
    what = "bn bf16 eval rows %d C %d" % (rows, c)
    refs = B.backward_refs(x, gamma, beta, dy, (rm0, rv0))
    G.check(backward_figures((xd.grad.float(), bn.weight.grad.cpu(), bn.bias.grad.cpu()), refs, "eval: ")[1:], what)
    bd = bn_bounds(x, gamma, beta, mean, rstd, dy, None, None, False)
    inside(y.float(), bd["y"], bd["y_bound"], what + " y")
    inside(xd.grad.float(), bd["dx"], bd["dx_bound"], what + " dx")


# ------------------------------------------------------------------------------------------------------------------------------
# the whole discriminator against the f32 oracle, by the rule of tests/test_bf16_model_gpu.py
# ------------------------------------------------------------------------------------------------------------------------------
def _oracle_pass(ref, x, gy, autocast):
    import copy
    ref = copy.deepcopy(ref)
    xr = x.clone().requires_grad_(True)
    if autocast:
        with torch.autocast("cpu", dtype=BF):
            y = ref(xr)
    else:
        y = ref(xr)
    y.float().backward(gy)
    return y.detach().float(), xr.grad.detach().float(), {k: p.grad.detach().float() for k, p in ref.named_parameters()}


@pytest.mark.parametrize("h,w", [(36, 44), (24, 40), (72, 72)], ids=lambda v: str(v))
def test_whole_discriminator_is_as_close_to_f32_as_autocast(hip_lib, h, w):
    """N = 4: logits, input gradient and every parameter gradient no further from the f32 oracle than twice the CPU-autocast oracle
    is, plus that file's floors (2e-2 outputs, 5e-2 per gradient tensor); all gradients concatenated: cosine >= min(0.98, autocast - 0.01)"""
    from test_bf16_model_gpu import rel, flat
    from odvae_amd.gan import NLayerDiscriminator, weights_init
    from oracle.losses import NLayerDiscriminator as RefD
    torch.manual_seed(11)
    ref = RefD().apply(weights_init).train()
    net = NLayerDiscriminator()
    res = net.load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    net = net.to(DEV).train().set_precision("bf16")
    g = torch.Generator().manual_seed(100 * h + w)
    x = torch.rand(4, 3, h, w, generator=g) * 2 - 1
    shape = tuple(_oracle_buffers_and_shape(ref, x)[1])
    gy = torch.randn(shape, generator=g)
    y32, dx32, g32 = _oracle_pass(ref, x, gy, False)
    yac, dxac, gac = _oracle_pass(ref, x, gy, True)
    xd = x.to(DEV).requires_grad_(True)
    y = net(xd)
    assert y.dtype == torch.float32 and tuple(y.shape) == shape
    y.backward(gy.to(DEV))
    assert xd.grad.dtype == torch.float32
    ghip = {k: p.grad.detach().cpu().float() for k, p in net.named_parameters()}
    assert set(ghip) == set(g32) and all(torch.isfinite(v).all() for v in ghip.values())
    report, failed = [], []

    def check(name, got, want, ac, floor):
        e, eac = rel(got, want), rel(ac, want)
        report.append("%s: hip %.3e autocast %.3e" % (name, e, eac))
        if not e <= 2 * eac + floor:
            failed.append("%s: hip %.3e from the f32 oracle, autocast %.3e (floor %.0e)" % (name, e, eac, floor))
    check("logits", y, y32, yac, 2e-2)
    check("input gradient", xd.grad, dx32, dxac, 5e-2)
    keys = sorted(g32)
    for k in keys:
        check("grad " + k, ghip[k], g32[k], gac[k], 5e-2)
    v32, vhip, vac = flat(g32, keys), flat(ghip, keys), flat(gac, keys)
    cos = lambda a, b: (a @ b / (a.norm() * b.norm())).item()
    c_hip, c_ac = cos(vhip, v32), cos(vac, v32)
    cx_hip, cx_ac = cos(xd.grad.cpu().flatten().double(), dx32.flatten().double()), cos(dxac.flatten().double(), dx32.flatten().double())
    report.append("parameter-gradient cosine: hip %.5f autocast %.5f | input-gradient cosine: hip %.5f autocast %.5f" % (c_hip, c_ac, cx_hip, cx_ac))
    print("discriminator bf16 %dx%d\n  " % (h, w) + "\n  ".join(report))
    assert not failed, "; ".join(failed)
    assert c_hip >= min(0.98, c_ac - 0.01) and cx_hip >= min(0.98, cx_ac - 0.01), report[-1]
    # the running statistics moved as the f32 oracle's did (bf16 activations in front of them: the rule for outputs)
    refb = _oracle_buffers_and_shape(ref, x)[0]
    for name, b in net.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(b) == 1
        else:
            e = rel(b, refb[name])
            assert e <= 2e-2, "buffer %s: %.3e" % (name, e)


def _oracle_buffers_and_shape(ref, x):
    import copy
    r = copy.deepcopy(ref)
    y = r(x)
    return dict(r.named_buffers()), y.shape


# ------------------------------------------------------------------------------------------------------------------------------
# the training step, the steady state, the switch
# ------------------------------------------------------------------------------------------------------------------------------
def _step(model, batch, noise, optimizer_idx):
    model.zero_grad(set_to_none=True)
    model._global_step = 1
    model.injected_noise = noise
    loss = model.training_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}, 0, optimizer_idx)
    loss.backward()
    logs = {k: float(v) for k, v in model.logged_metrics.items() if k.startswith("train/") and (not torch.is_tensor(v) or v.numel() == 1)}
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    return loss.detach().clone(), logs, grads


def _oracle_step(ref, batch, noise, optimizer_idx, autocast):
    import copy
    ref = copy.deepcopy(ref)         # (each pass starts from the same BatchNorm running statistics)
    ref.zero_grad()
    if autocast:
        with torch.autocast("cpu", dtype=BF):
            loss, log, _ = ref.training_step(batch, optimizer_idx, noise)
    else:
        loss, log, _ = ref.training_step(batch, optimizer_idx, noise)
    loss.backward()
    grads = {k: p.grad.detach().clone().float() for k, p in ref.named_parameters() if p.grad is not None}
    return loss.detach().float(), {k: float(v) for k, v in log.items() if not torch.is_tensor(v) or v.numel() == 1}, grads


@pytest.mark.parametrize("optimizer_idx", [0, 1], ids=["generator-step", "discriminator-step"])
def test_gan_step_with_bf16_discriminator(hip_lib, optimizer_idx):
    """ch = 32 at 64 x 64, B = 2, perceptual_weight 1, discriminator on; the generator step (with the adaptive weight) and the
    discriminator step.  The rule of test_gan_step_with_bf16_perceptual_net (tests/test_lpips_bf16_gpu.py) against the f32 oracle, with the
    same model with the switch off on the same seeded batch beside it; both d_weight values are printed."""
    from test_model_gpu import build_pair
    from test_bf16_model_gpu import rel, flat
    from odvae_amd import synthetic
    model, ref = build_pair(perceptual_weight=1.0, disc_factor=1.0, ch=32, latent_hw=4)
    plain, _ = build_pair(perceptual_weight=1.0, disc_factor=1.0, ch=32, latent_hw=4)
    model.train(); ref.train(); plain.train()
    ref.loss.perceptual_loss.eval()
    ref.global_step = 1
    batch = synthetic.make_batch(2, 64, seed=5)
    noise = synthetic.make_noise(2, 4, dropout_p=0.7, seed=6)
    l32, log32, g32 = _oracle_step(ref, batch, noise, optimizer_idx, False)
    lac, logac, gac = _oracle_step(ref, batch, noise, optimizer_idx, True)
    plain.set_precision("bf16")
    assert plain.loss.discriminator.compute_dtype == torch.float32
    base = _step(plain, batch, noise, optimizer_idx)
    model.set_precision("bf16", discriminator_precision="bf16")
    assert model.loss.discriminator.compute_dtype == BF and model.encoder.compute_dtype == BF
    state0 = {k: v.clone() for k, v in model.loss.discriminator.state_dict().items()}
    run1 = _step(model, batch, noise, optimizer_idx)
    model.loss.discriminator.load_state_dict(state0)         # (the running statistics moved; the outputs do not read them in training mode)
    run2 = _step(model, batch, noise, optimizer_idx)
    assert torch.equal(run1[0], run2[0]) and run1[1] == run2[1]
    assert set(run1[2]) == set(run2[2]) and all(torch.equal(run1[2][k], run2[2][k]) for k in run1[2])
    loss, logs, grads = run1
    report, failed = [], []

    def check(name, got, want, ac, floor, base_value):
        e, eac = rel(got, want), rel(ac, want)
        report.append("%s: hip %.3e autocast %.3e (switch off: %.3e)" % (name, e, eac, rel(base_value, want)))
        if not e <= 2 * eac + floor:
            failed.append("%s: bf16 HIP path %.3e from the f32 oracle, autocast oracle %.3e (floor %.0e)" % (name, e, eac, floor))
    check("total loss", loss, l32, lac, 1e-2, base[0])
    shared = sorted(k for k in log32 if k in logs and k in logac)
    for key in shared:      # d_weight: a quotient of gradient norms, held to the gradient floor (tests/test_lpips_bf16_gpu.py)
        check(key, torch.as_tensor(logs[key]), torch.as_tensor(log32[key]), torch.as_tensor(logac[key]),
              5e-2 if key == "train/d_weight" else 1e-2, torch.as_tensor(base[1][key]))
    if optimizer_idx == 0:
        assert {"train/g_loss", "train/d_weight", "train/nll_loss"} <= set(shared)
        report.append("d_weight: switch on %.6e, switch off %.6e, f32 oracle %.6e, autocast oracle %.6e" % (
            logs["train/d_weight"], base[1]["train/d_weight"], log32["train/d_weight"], logac["train/d_weight"]))
    else:
        assert {"train/disc_loss", "train/logits_real", "train/logits_fake"} <= set(shared)
    keys = [k for k in g32 if k in grads]
    want_nets = {"encoder", "decoder"} if optimizer_idx == 0 else {"loss"}
    assert {k.split(".")[0] for k in keys} >= want_nets
    ghip = {k: grads[k].cpu().float() for k in keys}
    assert all(torch.isfinite(ghip[k]).all() for k in keys)
    v32, vhip, vac = flat(g32, keys), flat(ghip, keys), flat(gac, keys)
    cos = lambda a, b: (a @ b / (a.norm() * b.norm())).item()
    c_hip, c_ac = cos(vhip, v32), cos(vac, v32)
    report.append("gradient cosine: hip %.5f autocast %.5f" % (c_hip, c_ac))
    print("\n".join(report))
    assert not failed, "; ".join(failed)
    assert c_hip >= min(0.98, c_ac - 0.01), report[-1]
    energy = v32.pow(2).sum().item()
    for k in keys:
        if g32[k].double().pow(2).sum().item() < 1e-3 * energy:
            continue
        e, eac = rel(ghip[k], g32[k]), rel(gac[k], g32[k])
        assert e <= 2 * eac + 5e-2, "grad %s: hip %.3e autocast %.3e" % (k, e, eac)
    # switch off again: the values of a model that never had it on, bit for bit
    model.set_precision("bf16", discriminator_precision=32)
    model.loss.discriminator.load_state_dict(state0)
    off = _step(model, batch, noise, optimizer_idx)
    assert torch.equal(off[0], base[0]) and off[1] == base[1], "switch off: the step differs from a model that never had the switch on"
    assert set(off[2]) == set(base[2]) and all(torch.equal(off[2][k], base[2][k]) for k in base[2])
    assert any(not torch.equal(run1[2][k], base[2][k]) for k in base[2]), "the switch changes nothing"


class _Recorder:
    """the loaded library with every odvae_* call noted by name"""

    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if not name.startswith("odvae_"):
            return f
        log = self._log

        def noted(*a):
            log.append(name)
            return f(*a)
        return noted


NEW_ENTRY_POINTS = {"odvae_conv4x4_bf16", "odvae_batchnorm_lrelu_fwd_bf16", "odvae_batchnorm_lrelu_bwd_bf16", "odvae_leaky_relu_bwd_bf16"}


def _trainer_and_batch(disc_precision, seed=23):
    from test_model_gpu import YAML
    from odvae_amd import synthetic
    from odvae_amd.trainer import Trainer
    torch.manual_seed(seed)
    model = synthetic.build_model(YAML, batch_size_for_lr=12, latent_hw=4, ch=32, perceptual_weight=1.0, disc_factor=1.0, disc_start=0).to(DEV).train()
    model._global_step = 1
    trainer = Trainer(model, gradient_clip_val=1.0, optimizer_indices=(0, 1), precision="bf16", discriminator_precision=disc_precision)
    batch = synthetic.make_batch(2, 64, seed=seed)
    batch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}

    def step(i):
        b = dict(batch)
        b["pose_6d"] = batch["pose_6d"].clone()
        return trainer.training_batch(b, i)
    return model, trainer, step


def test_gan_batch_with_bf16_discriminator_never_synchronises_the_host(hip_lib, monkeypatch):
    """After two warm-up batches a whole generator + discriminator batch issues without one host synchronisation, and each discriminator
    weight is packed exactly once per weight version -- once per batch, as its optimizer steps once per batch -- although three
    discriminator forwards (generator side, real, fake) read it."""
    import warnings
    from test_lpips_bf16_gpu import count_packs
    from odvae_amd import ops
    from odvae_amd.gan import Conv4x4
    model, trainer, step = _trainer_and_batch("bf16")
    assert model.loss.discriminator.compute_dtype == BF
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
    convs = [m for m in model.loss.discriminator.main if isinstance(m, Conv4x4)]
    assert len(convs) == 5
    for m in convs:
        assert seen.count(id(m.weight)) == 1, "discriminator weight %s packed %d times in one batch" % (tuple(m.weight.shape), seen.count(id(m.weight)))


def test_switch_off_makes_the_launches_of_a_model_that_never_had_it(hip_lib, monkeypatch):
    """The sequence of C-ABI calls of a GAN batch: with the switch off (after having been on) it is the sequence of a model that was
    never switched, none of the new entry points in it; with the switch on the f32 im2col / col2im / BatchNorm calls are gone."""
    import warnings
    from odvae_amd import lib
    from odvae_amd.trainer import Trainer

    def record(step, i):
        log = []
        with monkeypatch.context() as mp:
            rec = _Recorder(lib.load(), log)
            mp.setattr(lib, "load", lambda: rec)
            step(i)
        return log
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, _, step_plain = _trainer_and_batch(None)
        model, trainer, step = _trainer_and_batch("bf16")
        for i in range(2):
            step_plain(i); step(i)
        plain = record(step_plain, 2)
        on = record(step, 2)
        model.loss.discriminator.set_precision(32)
        off = record(step, 3)
    f32_disc = {"odvae_im2col4x4_f32", "odvae_col2im4x4_f32", "odvae_batchnorm_lrelu_fwd_f32", "odvae_batchnorm_lrelu_bwd_f32", "odvae_weight4x4_reorder_f32"}
    assert not NEW_ENTRY_POINTS & set(plain) and f32_disc <= set(plain)
    assert off == plain, "switch off: %d calls against %d; first difference at %s" % (
        len(off), len(plain), next((i, a, b) for i, (a, b) in enumerate(zip(off + [None], plain + [None])) if a != b))
    assert NEW_ENTRY_POINTS <= set(on) and not f32_disc & set(on)
    # three forwards of five layers; data gradients: five on the generator side (down to the image), four each for real and fake (their
    # inputs are detached); weight gradients: the discriminator step's two branches
    assert on.count("odvae_conv4x4_bf16") == 3 * 5 + 5 + 2 * 4 and on.count("odvae_conv_wgrad_bf16") - plain.count("odvae_conv_wgrad_bf16") == 2 * 5


def test_trainer_argument(hip_lib):
    from test_model_gpu import build_pair
    from odvae_amd.trainer import Trainer
    model, _ = build_pair(perceptual_weight=1.0, disc_factor=1.0)
    disc = model.loss.discriminator
    Trainer(model, precision="bf16")
    assert disc.compute_dtype == torch.float32
    Trainer(model, precision="bf16", discriminator_precision="bf16")
    assert disc.compute_dtype == BF and model.loss.perceptual_loss.compute_dtype == torch.float32
    Trainer(model, precision="bf16")
    assert disc.compute_dtype == BF, "discriminator_precision=None leaves the discriminator alone"
    Trainer(model, discriminator_precision=32)
    assert disc.compute_dtype == torch.float32
