"""Host checks of tests/conv_f32_exact_inputs.py: every case is exactly summable, every float64 reference agrees with
torch.nn.functional, the host-made F(4x4) pack evaluates to the direct convolution exactly, and the mirrored persistent-form rule
gives persistent, uneven plans at the MI355X's 256 CUs.  No device."""
import pytest
import torch
import torch.nn.functional as F

import conv_f32_exact_inputs as C
import exact_inputs as E


@pytest.mark.parametrize("name", list(C.CASES))
def test_every_case_is_exactly_summable(name):
    c = C.make_exact(name)
    s = C.assert_exactly_summable(c)
    assert max(s.values()) < C.LIMIT
    for t in ("x", "w", "dy"):
        assert c[t].abs().max().item() > 0
    if c["route"].startswith("wino4"):
        assert set((c["w"] / C.W4_SCALE).unique().tolist()) <= {-1.0, 0.0, 1.0}
        assert set(c["x"].unique().tolist()) <= {-1.0, 0.0, 1.0}
    if c.get("groups") and c["route"] != "wino4_gnbwd":
        assert s["stats_sumsq"] < C.LIMIT and s["stats_sumsq"] > 0


def test_the_summability_assertion_refuses_operands_that_can_round():
    c = C.make_exact("w4-16x32")
    c["w"] = c["w"] * 3.0 / 576.0          # multiples of 3 * 2^-10: G g G^T is no longer dyadic
    with pytest.raises(AssertionError):
        C.assert_exactly_summable(c)
    c = C.make_exact("m0-wide-ragged")
    c["x"] = c["x"] * 2.0 ** 16             # sums past 2^24 units
    with pytest.raises(AssertionError):
        C.assert_exactly_summable(c)
    c = C.make_exact("w2-4wave")
    c["w"] = c["w"] + 2.0 ** -30
    with pytest.raises(AssertionError):
        C.assert_exactly_summable(c)


@pytest.mark.parametrize("name", ["m0-wide-ragged", "m0-cin3-off-thin-in-narrow", "m1-narrow", "m2-narrow", "m5-cin24", "thin-in-5x32",
                                  "thin-out-c2-9x33", "w2-4wave", "w4-20x36-ragged", "w4-pool-20x36"])
@pytest.mark.parametrize("relu", [False, True])
def test_references_agree_with_torch_in_float64(name, relu):
    c = C.make_exact(name)
    mode, x, w, b, res, dy = c["mode"], c["x"], c["w"], c["b"], c["res"], c["dy"]
    xr = x.clone().requires_grad_(True)
    y = E.conv_f64(mode, xr, w, b) + res
    want = F.relu(y) if relu else y
    assert torch.equal(C.conv_ref(mode, x, w, b, res, relu=relu), want.detach())      # whole multiples of a unit: float64 is exact in any order
    assert torch.equal(C.conv_ref(mode, x, w), E.conv_f64(mode, x, w))
    dx, = torch.autograd.grad(E.conv_f64(mode, xr, w), xr, dy)
    assert torch.equal(C.dgrad_ref(mode, dy, w, x.shape), dx)
    if mode == 2:
        xu = C.upsample2x(x).requires_grad_(True)
        du, = torch.autograd.grad(F.conv2d(xu, w, padding=1), xu, dy)
        assert torch.equal(C.dgrad_full_ref(mode, dy, w, x.shape), du)
        assert torch.equal(C.pool2x2(du), dx)
    else:
        assert torch.equal(C.dgrad_full_ref(mode, dy, w, x.shape), dx)
    assert (want.detach() < 0).any().item() != relu and (want.detach() > 0).any().item()


def _eval_pack(pack, x, red_c, out_c):
    """F(4x4) of x [n, red_c, h, w] with a flat pack [36][redP / 4][outP][4], float64"""
    redP, outP = -(-red_c // 8) * 8, -(-out_c // 64) * 64
    U = pack.reshape(36, redP // 4, outP, 4).permute(0, 2, 1, 3).reshape(6, 6, outP, redP)
    d = F.pad(F.pad(x, (0, 0, 0, 0, 0, redP - red_c)), (1, 1, 1, 1)).unfold(2, 6, 4).unfold(3, 6, 4)
    V = torch.einsum("ai,nctuij,bj->nctuab", C.BT4, d, C.BT4)
    M = torch.einsum("nctuab,aboc->notuab", V, U)
    return C._output_transform(M, C.AT4)[:, :out_c], U


@pytest.mark.parametrize("name", ["w4-20x36-ragged", "w4-16x32", "w4-pool-20x36"])
def test_host_wino4_pack_reproduces_the_direct_convolution_exactly(name):
    c = C.make_exact(name)
    cin, cout = c["cin"], c["cout"]
    fwd, dgr = C.wino4_pack_f64(c["w"])
    assert fwd.numel() == 36 * (-(-cin // 8) * 8) * (-(-cout // 64) * 64) and dgr.numel() == 36 * (-(-cout // 8) * 8) * (-(-cin // 64) * 64)
    assert torch.equal(fwd.float().double(), fwd) and torch.equal(dgr.float().double(), dgr)        # f32 holds the pack exactly
    x = C.upsample2x(c["x"]) if c["mode"] == 2 else c["x"]
    y, U = _eval_pack(fwd, x, cin, cout)
    assert torch.equal(y, C.conv_ref(0, x, c["w"]))
    assert (U[:, :, cout:] == 0).all() and (U[:, :, :, cin:] == 0).all()                             # padding is zero
    dx, U = _eval_pack(dgr, c["dy"], cout, cin)
    assert torch.equal(dx, C.dgrad_full_ref(c["mode"], c["dy"], c["w"], c["x"].shape))
    assert (U[:, :, cin:] == 0).all() and (U[:, :, :, cout:] == 0).all()
    # and the evaluation the bounds are taken from is the same mathematics
    assert torch.equal(C.winograd(x, c["w"], 4)["y"], y)
    # the scale of the device pack's error has the pack's layout and bounds it entry by entry
    af, ad = C.wino4_pack_abs_f64(c["w"])
    assert af.shape == fwd.shape and (af >= fwd.abs()).all() and (ad >= dgr.abs()).all() and (fwd[af == 0] == 0).all()


def test_f2x2_on_the_host_is_exact_too():
    c = C.make_exact("w2-4wave")
    assert torch.equal(C.winograd(c["x"], c["w"], 2)["y"], C.conv_ref(0, c["x"], c["w"]))
    assert torch.equal(C.winograd(c["dy"], C.flipped(c["w"]), 2)["y"], C.dgrad_ref(0, c["dy"], c["w"], c["x"].shape))


@pytest.mark.parametrize("name", [k for k, v in C.CASES.items() if v.get("persistent")])
def test_persistent_cases_plan_persistent_and_uneven_at_256_cus(name):
    case = C.CASES[name]
    m = 2 if case["route"] == "wino2" else 4
    n = C.case_n(case, 256)
    assert n is not None
    p = C.persistent_plan(m, 256, n, case["hi"], case["wi"], case["cin"], case["cout"])
    assert p["persistent"] and p["uneven"]
    assert p["tiles"] >= 2 * p["blocks_per_co"] and p["tiles"] % p["blocks_per_co"] != 0
    assert not C.persistent_plan(m, 256, 1, case["hi"], case["wi"], case["cin"], case["cout"])["persistent"]      # fewer than two tiles per block
    if m == 2:      # the chunk condition of F(2x2): three chunks, and an odd count, stay on the one-tile form
        assert not C.persistent_plan(2, 256, n, case["hi"], case["wi"], 48, case["cout"])["persistent"]
        assert not C.persistent_plan(2, 256, n, case["hi"], case["wi"], 80, case["cout"])["persistent"]
        assert not C.persistent_plan(2, 256, n, case["hi"], case["wi"], case["cin"], case["cout"] + 64)["persistent"]
    assert not C.persistent_plan(m, 256, 4096, case["hi"], case["wi"], case["cin"], 3 * C.WINO_BN[m])["persistent"]   # 256 % (8 * 3) != 0


def test_no_other_case_plans_persistent_at_256_cus():
    for name, case in C.CASES.items():
        if case.get("persistent") or not case["route"].startswith("wino"):
            continue
        m = 2 if case["route"] == "wino2" else 4
        ho, wo = C.out_hw(case["mode"], case["hi"], case["wi"])
        for cin, cout in ((case["cin"], case["cout"]), (case["cout"], case["cin"])):
            assert not C.persistent_plan(m, 256, case["n"], ho, wo, cin, cout)["persistent"], name


def test_thin_in_wrap_case_wraps():
    case = C.CASES["thin-in-wraps"]
    assert case["n"] * case["hi"] * (case["wi"] // 32) > 4096 and case["wi"] % 32 == 0
