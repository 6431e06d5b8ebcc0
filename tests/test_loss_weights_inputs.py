"""CPU checks of what the `weights` / `cond` GPU tests rest on: ops.loss_weights_layout on every class of shape, the float64 restatements of
tests/loss_weights_ref.py against the element-wise formulas upstream writes, the exact inputs' precondition, and the acceptance rules
against planted faults in a host model of the kernels."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loss_weights_ref as R  # noqa: E402


# ---- ops.loss_weights_layout -----------------------------------------------------------------------------------------------------
N, C, H, W = 4, 3, 6, 5


@pytest.mark.parametrize("weights,layout,shape", [
    (0.5, "scalar", ()), (2, "scalar", ()), (torch.tensor(0.5), "scalar", ()), (torch.ones(1, 1, 1, 1), "scalar", ()),
    (torch.ones(N), "sample", (N,)), (torch.ones(N, 1, 1, 1), "sample", (N,)),
    (torch.ones(N, 1, H, W), "pixel", (N, 1, H, W)), (torch.ones(1, 1, H, W), "pixel", (N, 1, H, W)), (torch.ones(H, W), "pixel", (N, 1, H, W)),
    (torch.ones(N, C, H, W), "element", (N, C, H, W)), (torch.ones(1, C, H, W), "element", (N, C, H, W)), (torch.ones(C, 1, 1), "element", (N, C, H, W)),
    (torch.ones(N, C, 1, 1), "element", (N, C, H, W)), (torch.ones(W), "element", (N, C, H, W)), (torch.ones(N, 1, H, 1), "element", (N, C, H, W)),
    (torch.ones(N, 1, H, W, dtype=torch.bool), "pixel", (N, 1, H, W)),
])
def test_layout_classes(weights, layout, shape):
    from odvae_amd import ops
    got, t = ops.loss_weights_layout(weights, N, C, H, W)
    assert got == layout and got in ops.WEIGHT_LAYOUTS and tuple(t.shape) == shape
    if torch.is_tensor(weights) and layout in ("pixel", "element"):      # the view broadcasts as torch would
        assert torch.equal(t, weights.expand(shape) if weights.dim() == 4 else torch.broadcast_to(weights, (N, C, H, W))[:, :shape[1]])


def test_layout_reads_a_one_d_tensor_of_batch_length_as_per_sample():
    """[N] is this project's reading of one weight per sample, also where N == W would let torch broadcast it along the width"""
    from odvae_amd import ops
    w = torch.arange(5.0)
    assert ops.loss_weights_layout(w, 5, 3, 6, 5)[0] == "sample"
    assert ops.loss_weights_layout(w, 4, 3, 6, 5)[0] == "element"


@pytest.mark.parametrize("bad", [torch.ones(N + 3), torch.ones(N, 2, H, W), torch.ones(N, 1, H + 1, W), torch.ones(2, 1, H, W),
                                 torch.ones(1, N, C, H, W), torch.ones(N, C, H)])
def test_layout_refuses_a_shape_that_does_not_broadcast(bad):
    from odvae_amd import ops
    with pytest.raises(ValueError) as e:
        ops.loss_weights_layout(bad, N, C, H, W)
    assert str(tuple(bad.shape)) in str(e.value) and str((N, C, H, W)) in str(e.value)      # both shapes are named


def test_layout_refuses_weights_that_require_grad():
    from odvae_amd import ops
    with pytest.raises(ValueError, match="requires grad"):
        ops.loss_weights_layout(torch.ones(N, 1, H, W, requires_grad=True), N, C, H, W)


# ---- the restatements against the element-wise formulas -------------------------------------------------------------------------------
def _nchw(t, h, w):
    return t.reshape(t.shape[0], h, w, -1).permute(0, 3, 1, 2)


@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("with_box", [False, True])
@pytest.mark.parametrize("eps", [0.0, 1e-8])
def test_three_sums_give_the_elementwise_weighted_nll(per_channel, with_box, eps):
    """Per sample, sum over (c,h,w) of weights * (rec_loss / (exp(logvar) + eps) + logvar) with rec_loss = |x m - xr m| + pw p[n], written
    out on [N,C,H,W] as upstream does, equals (WL1 + pw p W) / (exp(logvar) + eps) + logvar W -- in float64 to a few ulps."""
    g = torch.Generator().manual_seed(3)
    n, h, w, c = 3, 5, 7, 3
    x, xr = torch.randn(n, h * w, c, generator=g, dtype=torch.float64), torch.randn(n, h * w, c + 1, generator=g, dtype=torch.float64)
    wgt = torch.randn(n, h * w, c, generator=g, dtype=torch.float64) if per_channel else torch.rand(n, h * w, generator=g, dtype=torch.float64)
    box = (torch.rand(n, h * w, generator=g) < 0.6).double() if with_box else None
    p, logvar, pw = torch.rand(n, generator=g, dtype=torch.float64), 0.3, 0.7
    l1, wl1, ws = R.l1_weighted_sums_f64(x, xr, box, wgt, per_channel)
    got = R.weighted_nll_from_sums(l1, wl1, ws, p, pw, logvar, eps)
    m = torch.ones(n, 1, h, w, dtype=torch.float64) if box is None else box.reshape(n, 1, h, w)
    rec_loss = (_nchw(x, h, w) * m - _nchw(xr, h, w)[:, :c] * m).abs() + pw * p.reshape(n, 1, 1, 1)
    nll = rec_loss / (np.exp(logvar) + eps) + logvar
    weights = _nchw(wgt, h, w) if per_channel else wgt.reshape(n, 1, h, w)
    want = (weights * nll).sum(dim=(1, 2, 3))
    assert float(((got - want).abs() / want.abs().clamp(min=1.0)).max()) < 1e-13
    unweighted = R.weighted_nll_from_sums(l1, l1, torch.full((n,), float(c * h * w), dtype=torch.float64), p, pw, logvar, eps)
    assert float(((unweighted - nll.sum(dim=(1, 2, 3))).abs() / nll.sum(dim=(1, 2, 3)).abs().clamp(min=1.0)).max()) < 1e-13
    # the weight sums alone (the pixel term off): the same W
    assert torch.equal(R.l1_weighted_sums_f64(None if per_channel else c, None, None, wgt, per_channel)[2], ws)


def test_backward_restatement_is_the_derivative():
    """d/dxr of sum_n (g_l1[n] l1[n] + g_wl1[n] wl1[n]) by autograd on the element-wise formula, away from ties"""
    g = torch.Generator().manual_seed(4)
    n, hw, c, cr = 2, 11, 3, 4
    x, wgt = torch.randn(n, hw, c, generator=g, dtype=torch.float64), torch.randn(n, hw, generator=g, dtype=torch.float64)
    xr = torch.randn(n, hw, cr, generator=g, dtype=torch.float64).requires_grad_()
    box = torch.rand(n, hw, generator=g, dtype=torch.float64)
    g_l1, g_wl1 = torch.randn(n, generator=g, dtype=torch.float64), torch.randn(n, generator=g, dtype=torch.float64)
    t = (x * box[..., None] - xr[..., :c] * box[..., None]).abs()
    ((g_l1 * t.sum(dim=(1, 2))).sum() + (g_wl1 * (wgt[..., None] * t).sum(dim=(1, 2))).sum()).backward()
    want = R.l1_weighted_bwd_f64(x, xr.detach(), box, wgt, False, g_l1, g_wl1)
    assert float((xr.grad - want).abs().max()) < 1e-14 and float(want[..., c:].abs().max()) == 0.0
    only = R.l1_weighted_bwd_f64(x, xr.detach(), box, wgt, False, g_l1, None)
    assert torch.equal(only, R.l1_weighted_bwd_f64(x, xr.detach(), box, wgt, False, g_l1, torch.zeros(n, dtype=torch.float64)))


def test_weighted_plain_loss_is_the_elementwise_formula_and_plain_loss_without_the_arguments():
    """WeightedPlainLoss with weights = None, cond = None is tests/plain_vae_ref.PlainLoss to the bit; with a weight map its total moves by
    exactly sum((weights - 1) * nll) / N; with cond the discriminator sees the concatenation (a 5-channel first layer takes it)."""
    import plain_vae_ref as P
    from oracle.distributions import DiagonalGaussianDistribution as DG
    kw = dict(disc_start=0, kl_weight=0.3, disc_weight=0.5, perceptual_weight=0.0, disc_factor=1.0)
    torch.manual_seed(1)
    a = P.PlainLoss(**kw).double()
    b = R.WeightedPlainLoss(**kw).double()
    b.load_state_dict(a.state_dict())
    g = torch.Generator().manual_seed(2)
    x = torch.rand(2, 3, 32, 32, generator=g, dtype=torch.float64)
    gain = torch.ones(3, dtype=torch.float64, requires_grad=True)
    xr = (x + 0.1 * torch.randn(2, 3, 32, 32, generator=g, dtype=torch.float64)) * gain.view(1, 3, 1, 1)
    mom = torch.randn(2, 8, 4, 4, generator=g, dtype=torch.float64)
    la, _ = a(x, xr, DG(mom), 0, 5, last_layer=gain)
    lb, logb = b(x, xr, DG(mom), 0, 5, last_layer=gain)
    assert torch.equal(la, lb)
    wmap = torch.rand(2, 1, 32, 32, generator=g, dtype=torch.float64)
    lw, logw = b(x, xr, DG(mom), 0, 5, last_layer=gain, weights=wmap)
    nll = (x - xr).abs() / torch.exp(b.logvar) + b.logvar
    assert abs(float((lw - lb).detach()) - float(((wmap - 1) * nll).sum().detach() / 2)) < 1e-9 * abs(float(lb.detach()))
    assert torch.equal(logw["train/nll_loss"], logb["train/nll_loss"])
    per_sample = torch.tensor([0.5, 1.75], dtype=torch.float64)
    assert torch.equal(b(x, xr, DG(mom), 0, 5, last_layer=gain, weights=per_sample)[0],
                       b(x, xr, DG(mom), 0, 5, last_layer=gain, weights=per_sample.reshape(2, 1, 1, 1))[0])
    with pytest.raises(AssertionError):
        b(x, xr, DG(mom), 0, 5, last_layer=gain, cond=x[:, :2])
    torch.manual_seed(1)
    c5 = R.WeightedPlainLoss(disc_in_channels=5, disc_conditional=True, **kw).double()
    with pytest.raises(AssertionError):
        c5(x, xr, DG(mom), 0, 5, last_layer=gain)
    cond = torch.rand(2, 2, 32, 32, generator=g, dtype=torch.float64)
    l5, log5 = c5(x, xr, DG(mom), 0, 5, last_layer=gain, cond=cond)
    want_g = -c5.discriminator(torch.cat((xr, cond), dim=1)).mean()
    assert abs(float(log5["train/g_loss"]) - float(want_g)) < 1e-12 and bool(torch.isfinite(l5))
    d5, _ = c5(x, xr, DG(mom), 1, 5, cond=cond)
    assert bool(torch.isfinite(d5))


# ---- the exact inputs and the acceptance rules -----------------------------------------------------------------------------------------
CASES = [(1, 1, 1, 1, False), (3, 63, 3, 3, False), (3, 257, 3, 4, False), (1, 1000, 4, 4, True), (3, 255, 3, 4, True), (1, 256, 3, 3, True)]


@pytest.mark.parametrize("n,hw,c,cr,per_channel", CASES)
def test_exact_inputs_meet_their_precondition_and_the_clean_model_is_accepted(n, hw, c, cr, per_channel):
    for with_box in (False, True):
        x, xr, box, wgt = R.exact_inputs(n, hw, c, cr, per_channel, seed=hw + n, with_box=with_box)
        assert R.sums_are_exact(x, xr, box, wgt, per_channel)
        g_l1, g_wl1 = R.exact_grads(n, seed=hw)
        l1, wl1, w, dxr = R.host_model(x, xr, box, wgt, per_channel, g_l1, g_wl1)
        assert R.accept_sums((l1, wl1, w), x, xr, box, wgt, per_channel)
        assert R.accept_bwd(dxr, x, xr, box, wgt, per_channel, g_l1, g_wl1)
        assert R.accept_sums((None, wl1, None), x, xr, box, wgt, per_channel)      # each output may be absent


def test_the_size_past_the_grid_cap_meets_the_precondition():
    x, xr, box, wgt = R.exact_inputs(1, R.PAST_CAP, 3, 4, False, seed=1)
    assert R.sums_are_exact(x, xr, box, wgt, False)
    big = R.exact_inputs(1, R.PAST_CAP, 3, 4, False, seed=1, q=64, wq=64, a=4)
    assert not R.sums_are_exact(*big[:2], big[2], big[3], False)      # the precondition is a real one: finer grids at this size fail it
    assert not R.sums_are_exact(x + 1e-3, xr, box, wgt, False)


@pytest.mark.parametrize("fault", ["weight_before_abs", "w_sum_boxed", "pixel_weight_once", "dxr_channel3", "sign_at_tie"])
def test_acceptance_rules_reject_a_planted_fault_in_the_weighted_sums(fault):
    per_channel = False
    x, xr, box, wgt = R.exact_inputs(3, 257, 3, 4, per_channel, seed=9, with_box=True)
    g_l1, g_wl1 = R.exact_grads(3, seed=10)
    assert bool((g_l1 != 0).all())
    l1, wl1, w, dxr = R.host_model(x, xr, box, wgt, per_channel, g_l1, g_wl1, fault=fault)
    ok_sums = R.accept_sums((l1, wl1, w), x, xr, box, wgt, per_channel)
    ok_bwd = R.accept_bwd(dxr, x, xr, box, wgt, per_channel, g_l1, g_wl1)
    assert not (ok_sums and ok_bwd), fault
    assert ok_sums == (fault in ("dxr_channel3", "sign_at_tie")) and ok_bwd == (fault not in ("dxr_channel3", "sign_at_tie"))


@pytest.mark.parametrize("fault", ["cond_times_box", "grad_to_cond"])
def test_acceptance_rules_reject_a_planted_fault_in_cat_mask(fault):
    x, box, cond, dy = R.exact_cat_inputs(3, 63, 3, 2, seed=11)
    assert R.accept_cat(*R.host_cat_model(x, box, cond, dy), x, box, cond, dy)
    assert not R.accept_cat(*R.host_cat_model(x, box, cond, dy, fault=fault), x, box, cond, dy)


def test_every_fault_is_covered():
    assert set(R.FAULTS) == {"weight_before_abs", "w_sum_boxed", "pixel_weight_once", "cond_times_box", "grad_to_cond", "dxr_channel3", "sign_at_tie"}


def test_synthetic_side_inputs_leave_every_other_entry_alone():
    from odvae_amd import synthetic
    a = synthetic.make_batch(3, 16, seed=7, mask_key="mask")
    b = synthetic.make_batch(3, 16, seed=7, mask_key="mask", cond_key="cond", cond_channels=2, weights_key="wts")
    assert set(b) - set(a) == {"cond", "wts"} and tuple(b["cond"].shape) == (3, 2, 16, 16) and tuple(b["wts"].shape) == (3, 1, 16, 16)
    for k in a:
        assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k
    ia, ib = synthetic.make_image_batch(2, 16, seed=7), synthetic.make_image_batch(2, 16, seed=7, cond_key="cond", cond_channels=5)
    assert torch.equal(ia["image"], ib["image"]) and tuple(ib["cond"].shape) == (2, 5, 16, 16) and set(ib) == {"image", "cond"}
    assert float(b["wts"].min()) >= 0.25 and float(b["wts"].max()) <= 2.0
