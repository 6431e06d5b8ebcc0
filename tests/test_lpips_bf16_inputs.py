"""The host model of the bf16 perceptual net and its references must be able to fail (CPU only).

tests/lpips_bf16_inputs.py holds the model the GPU tests (tests/test_lpips_bf16_gpu.py) compare the HIP path with.  Here, on the host:
  * the model in float32 equals the model in float64 bit for bit on the exactly summable chain (so the float64 references are what f32
    accumulators must give), and the per-kernel references agree with torch's own autograd where torch computes the same thing;
  * each planted fault -- ReLU after the rounding that drops a NaN, mask from the wrong layer, mask >= 0, the tap gradient rounded
    twice, a pool tie broken the other way -- is REJECTED by the bit comparison on the inputs the GPU tests use;
  * the model stands where the issue's table puts it against the f32 oracle: no further than autocast on the gradient, far below it
    on the value.
"""
import pytest
import torch
import torch.nn.functional as F

import exact_inputs as E
import lpips_bf16_inputs as M

BF = torch.bfloat16


def run_chain(c, dt, fault=None):
    return M.net(c["x0"], c["x1"], c["shift"], c["scale"], c["convs"], c["lins"], c["g"], c["g_pass"], dt=dt, fault=fault)


def chain_bits(r):
    return [r["dx"].float()] + [t.float().to(BF) for t in r["taps"]] + [t.float().to(BF) for t in r["dtaps"]]


@pytest.fixture(scope="module")
def chain():
    c = M.chain_case()
    M.assert_chain_summable(c)
    return c, run_chain(c, torch.float64)


def test_chain_f32_equals_f64(chain):
    c, ref = chain
    got = run_chain(c, torch.float32)
    for a, b, name in zip(chain_bits(got), chain_bits(ref), ("dx", "tap 1", "tap 2", "d tap 1", "d tap 2")):
        E.assert_bits_equal(a, b, "chain " + name)
    # the case is worth something: zeros at ReLU outputs, both signs in the gradient, rounding at the stores, a live image gradient
    assert 0.2 < (ref["taps"][0] == 0).double().mean() < 0.8 and 0.2 < (ref["taps"][1] == 0).double().mean() < 0.8
    assert ref["taps"][0].max() > 256 * 0.5, "no feature is wide enough to be rounded at its store"
    assert (ref["dx"] > 0).any() and (ref["dx"] < 0).any()


@pytest.mark.parametrize("fault", ["mask_wrong_layer", "mask_ge", "pool_tie_other"])
def test_chain_rejects(chain, fault):
    c, ref = chain
    bad = run_chain(c, torch.float64, fault)
    with pytest.raises(AssertionError, match="differ in bits"):
        E.assert_bits_equal(bad["dx"].float(), ref["dx"].float(), "chain dx with " + fault)


CONV_CASES = [(3, 64, 2, 9, 17), (64, 64, 2, 9, 17), (64, 128, 2, 9, 17), (128, 256, 2, 9, 17), (256, 512, 2, 9, 17), (512, 512, 2, 4, 5),
              (40, 96, 1, 9, 17), (96, 136, 1, 9, 17)]
NAN_AT = (1, 2, 4, 9)      # image 1, channel 2, row 4, column 9 (row 1, column 2 at 4 x 5)


def nan_at(h, w):
    return NAN_AT if h > 4 else (1, 2, 1, 2)


@pytest.mark.parametrize("cin,cout,n,h,w", CONV_CASES)
def test_conv_cases_are_exactly_summable_and_cover_the_edges(cin, cout, n, h, w):
    c = M.conv_case(cin, cout, n, h, w)
    E.assert_exactly_summable(c)
    r = M.conv_case_references(c)
    assert (r["y_exact"] == 0).any() and (r["y_exact"] < 0).any() and (r["y_exact"] > 0).any(), "pre-activations: no exact zero / no negative value"
    x = c["x"][:, :cin]
    assert (x == 0).any() and (x < 0).any() and (x > 0).any(), "the mask holds no zero / no negative value"
    assert not torch.equal(r["dx_masked"], r["dx_plain"])
    # torch's own autograd computes the same two things
    xr = x.clone().requires_grad_(True)
    y = torch.relu(F.conv2d(xr, c["w"], c["b"], padding=1))
    assert torch.equal(y.detach().float().to(BF), r["y"])
    pre = F.conv2d(xr, c["w"], c["b"], padding=1)
    (du,) = torch.autograd.grad(pre, xr, c["dy"])
    assert torch.equal(du.float(), r["dx_f32"])


def test_relu_after_the_rounding_of_a_nan_is_rejected():
    c = M.conv_case(64, 64, 2, 9, 17, nan_at=NAN_AT)
    ref = M.conv_case_references(c)["y"]
    assert int(torch.isnan(ref).sum()) == 9 * 64
    good = M.conv_relu_fwd(c["x"], c["w"], c["b"]).float().to(BF)
    M.nan_equal_bits(good, ref, "conv + ReLU with a NaN")
    bad = M.conv_relu_fwd(c["x"], c["w"], c["b"], fault="relu_after_round").float().to(BF)
    with pytest.raises(AssertionError, match="NaN at"):
        M.nan_equal_bits(bad, ref, "conv + ReLU with a NaN, ReLU after the rounding")


def dist_case(c, hw, seed=0, zero_pixel=True):
    """bf16 ReLU-like features [2, c, 1, hw], one all-zero feature vector in f1, lin weights, upstream gradient, next-slice gradient"""
    g = M.gen(41, c, hw, seed)
    f0 = torch.relu(torch.randn(2, c, 1, hw, generator=g)).to(BF).float()
    f1 = torch.relu(torch.randn(2, c, 1, hw, generator=g)).to(BF).float()
    if zero_pixel:
        f1[1, :, 0, hw // 2] = 0.0
    w = torch.rand(c, generator=g) / c
    gw = torch.randn(2, generator=g)
    dnext = (torch.randn(2, c, 1, hw, generator=g) * 1e-3).to(BF).float()
    return f0, f1, w, gw, dnext


def test_tap_gradient_rounded_twice_is_rejected():
    f0, f1, w, gw, dnext = dist_case(64, 35)
    good = M.dist_bwd(f0, f1, w, gw, dnext=dnext, mask=f1).to(BF)
    bad = M.dist_bwd(f0, f1, w, gw, dnext=dnext, mask=f1, fault="tap_round_twice").to(BF)
    with pytest.raises(AssertionError, match="differ in bits"):
        E.assert_bits_equal(bad, good, "tap gradient rounded twice")


@pytest.mark.parametrize("c,hw", [(64, 1), (64, 35), (512, 35)])
def test_distance_model_against_autograd(c, hw):
    """off the zero feature vector and without mask / next-slice gradient, dist_bwd is the gradient of dist_fwd (float64)"""
    f0, f1, w, gw, _ = dist_case(c, hw, zero_pixel=False)
    f0, f1, w, gw = f0.double(), f1.double(), w.double(), gw.double()
    f1r = f1.clone().requires_grad_(True)
    (M.dist_fwd(f0, f1r, w) * gw).sum().backward()
    n0 = f0 / (torch.sqrt((f0 ** 2).sum(1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt((f1 ** 2).sum(1, keepdim=True)) + 1e-10)
    assert torch.allclose(M.dist_fwd(f0, f1, w), F.conv2d((n0 - n1) ** 2, w.view(1, -1, 1, 1)).mean((1, 2, 3)), rtol=1e-12, atol=0)
    got = M.dist_bwd(f0, f1, w, gw)
    ref = f1r.grad
    assert (got - ref).abs().max() <= 2.0 ** -8 * ref.abs().max(), "beyond one bf16 rounding of the autograd gradient"
    assert torch.equal(got, M.rne(got))


@pytest.mark.parametrize("h,w,c", [(9, 11, 64), (2, 2, 64), (9, 11, 512), (2, 2, 512)])
def test_pool_model_against_torch(h, w, c):
    """off NaN windows the model's pool is F.max_pool2d and its autograd (first maximum in row-major order); the other tie order differs"""
    x, dy, mask = M.pool_case(2, c, h, w)
    clean = torch.where(torch.isnan(x), torch.zeros_like(x), x)
    xr = clean.clone().requires_grad_(True)
    y = F.max_pool2d(xr, 2, 2)
    y.backward(dy)
    assert torch.equal(M.pool_fwd(clean), y.detach())
    assert torch.equal(M.pool_bwd(clean, dy), xr.grad)
    assert not torch.equal(M.pool_bwd(clean, dy, fault="pool_tie_other"), xr.grad)
    if h >= 4:
        assert torch.isnan(M.pool_fwd(x)[:, 0, 1, 1]).all() and torch.isnan(M.pool_fwd(x)[:, c - 1, 1, 1]).all()
        dx = M.pool_bwd(x, dy)
        assert torch.equal(dx[:, 0, 2, 2], dy[:, 0, 1, 1]) and torch.equal(dx[:, c - 1, 3, 3], dy[:, c - 1, 1, 1])      # to the window's NaN
        assert (dx[:, :, 8, :] == 0).all() and (dx[:, :, :, 10] == 0).all()                                            # dropped row / column
    masked = M.pool_bwd(x, dy, mask=mask)
    plain = M.pool_bwd(x, dy)
    assert ((plain != 0) & (mask <= 0)).any(), "the mask is never zero at an argmax that carries a gradient"
    assert torch.equal(masked, torch.where(mask > 0, plain, torch.zeros_like(plain)))


def test_host_model_against_the_oracle_at_36x44():
    """The model's arithmetic alone: value error far below autocast's, gradient no worse than 1.25 x autocast's (the issue's table has it at
    about 1.0 x), cosine as autocast's.  The figures are printed."""
    from odvae_amd.gan import VGG16_SLICES
    from oracle.losses import LPIPSStyle as RefL
    torch.manual_seed(0)
    ref = RefL().eval()
    g = M.gen(31, 36, 44)
    x0 = torch.rand(2, 3, 36, 44, generator=g) * 2 - 1
    x1 = (x0 + 0.3 * torch.randn(2, 3, 36, 44, generator=g)).clamp(-1, 1)

    def oracle(autocast):
        x1r = x1.clone().requires_grad_(True)
        if autocast:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                d = ref(x0, x1r)
        else:
            d = ref(x0, x1r)
        d.float().sum().backward()
        return d.detach().float().reshape(-1), x1r.grad.float()

    d32, g32 = oracle(False)
    dac, gac = oracle(True)
    shift, scale, convs, lins = M.net_params(ref.state_dict(), VGG16_SLICES)
    r = M.net(x0, x1, shift, scale, convs, lins, torch.ones(2))
    relv = lambda a: ((a - d32).abs() / d32.abs()).max().item()
    rell2 = lambda a: ((a - g32).norm() / g32.norm()).item()
    cos = lambda a: (a.flatten() @ g32.flatten() / (a.norm() * g32.norm())).item()
    print("value error: model %.3e autocast %.3e | gradient rel. L2: model %.3e autocast %.3e | cosine: model %.5f autocast %.5f" % (
        relv(r["d"]), relv(dac), rell2(r["dx"]), rell2(gac), cos(r["dx"]), cos(gac)))
    assert relv(r["d"]) <= relv(dac)
    assert rell2(r["dx"]) <= 1.25 * rell2(gac)
    assert cos(r["dx"]) >= min(0.98, cos(gac) - 0.01)
