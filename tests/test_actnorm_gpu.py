"""ActNorm + LeakyReLU(0.2) on the HIP kernels (csrc/gan_norm.hip: an_*_kernel, odvae_actnorm_*).

* forward and backward of an initialised layer against torch f32 on the host (tests/actnorm_ref.py) at test_batchnorm_lrelu's
  tolerances -- 2e-4 forward, 5e-4 for dx, dloc, dscale, relative to max|ref| -- over the shapes of bn_offset_inputs (they reach every
  branch of the row-lane / channel-pass geometry the kernels share with bn_colstats_kernel) plus (2,6,5,3), whose channel count is no
  multiple of 4 and takes the scalar path; the dx-only kernel with both parameters frozen;
* the data-dependent initialisation against float64 on the offset ladder of bn_offset_inputs (|mean| / std up to 1000, scales 1 and
  0.01), the figures loc * scale_64 and scale / scale_64 under the acceptance rule of gn_offset_inputs (at most 8x torch f32's own
  error, or the forward floor);
* the flags: `initialized`, loc, scale over training / eval forwards, a state_dict round trip, fewer than 2 rows;
* no host synchronisation, in the initialising forward or afterwards.
"""
import pytest
import torch
import torch.nn.functional as F

import actnorm_ref as A
import bn_offset_inputs as B
import gn_offset_inputs as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = B.SHAPES + [(2, 6, 5, 3)]
FWD_TOL, BWD_TOL = 2e-4, 5e-4


def close(a, b, tol, what=""):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    assert a.shape == b.shape, "%s: shape %s vs %s" % (what, tuple(a.shape), tuple(b.shape))
    err = (a - b).abs().max().item()
    ref = max(1e-6, b.abs().max().item())
    print("%-28s err %.3e  bound %.1e * %.3e" % (what, err, tol, ref))
    assert err <= tol * ref, "%s: max err %.3e > %.1e * %.3e" % (what, err, tol, ref)


def initialised_layer(c, loc, scale, requires_grad=True):
    from odvae_amd.gan import ActNormLReLU
    m = ActNormLReLU(c)
    with torch.no_grad():
        m.loc.copy_(loc.view(1, c, 1, 1)); m.scale.copy_(scale.view(1, c, 1, 1)); m.initialized.fill_(1)
    m.refresh_initialized()
    m.loc.requires_grad_(requires_grad); m.scale.requires_grad_(requires_grad)
    return m.to(DEV).train()


def case(shape):
    """x, loc, scale, a kink-free dy and torch f32's (y, dx, dloc, dscale) for one shape"""
    n, c, h, w = shape
    x = B.make_input(shape, 2, 1.0)
    loc, scale = B.affine(c)                      # randn: scales of both signs
    loc, scale = loc.view(1, c, 1, 1), scale.view(1, c, 1, 1)
    u64 = scale.double() * (x.double() + loc.double())
    dy = B.kink_free_dy(u64, G.seed_of(shape, 0, 1.0, 29))
    y32 = F.leaky_relu(scale * (x + loc), A.SLOPE)
    return x, loc, scale, dy, y32, A.autograd_backward(x, loc, scale, dy)


@pytest.mark.parametrize("shape", SHAPES, ids=B.shape_id)
def test_forward_and_backward_match_torch_f32(hip_lib, shape):
    x, loc, scale, dy, y32, (dx32, dloc32, dscale32) = case(shape)
    m = initialised_layer(shape[1], loc, scale)
    xd = x.to(DEV).requires_grad_(True)
    y = m(xd)
    close(y, y32, FWD_TOL, "actnorm fwd")
    y.backward(dy.to(DEV))
    close(xd.grad, dx32, BWD_TOL, "actnorm dx")
    close(m.loc.grad, dloc32, BWD_TOL, "actnorm dloc")
    close(m.scale.grad, dscale32, BWD_TOL, "actnorm dscale")
    # the closed forms the kernels evaluate, in float64, say the same
    dx64, dloc64, dscale64 = A.closed_form_backward(x.double(), loc.double(), scale.double(), dy.double())
    close(xd.grad, dx64, BWD_TOL, "actnorm dx (f64)")
    close(m.loc.grad, dloc64, BWD_TOL, "actnorm dloc (f64)")
    close(m.scale.grad, dscale64, BWD_TOL, "actnorm dscale (f64)")
    assert torch.equal(m.loc.detach().cpu(), loc) and torch.equal(m.scale.detach().cpu(), scale) and int(m.initialized) == 1


@pytest.mark.parametrize("shape", SHAPES, ids=B.shape_id)
def test_dx_only_backward_with_frozen_parameters(hip_lib, shape):
    x, loc, scale, dy, y32, (dx32, _, _) = case(shape)
    m = initialised_layer(shape[1], loc, scale, requires_grad=False)
    xd = x.to(DEV).requires_grad_(True)
    y = m(xd)
    close(y, y32, FWD_TOL, "actnorm fwd (frozen)")
    y.backward(dy.to(DEV))
    close(xd.grad, dx32, BWD_TOL, "actnorm dx (dx-only kernel)")
    assert m.loc.grad is None and m.scale.grad is None
    # same values as the kernel that also forms the partial sums: both evaluate scale * (dy * lrelu'(h))
    m2 = initialised_layer(shape[1], loc, scale)
    xd2 = x.to(DEV).requires_grad_(True)
    m2(xd2).backward(dy.to(DEV))
    assert torch.equal(xd.grad, xd2.grad)


# ---- initialisation on the offset ladder ---------------------------------------------------------------------------------------------
def init_figures(x):
    """loc * scale_64 and scale / scale_64 of the layer initialised from the host tensor x; a measuring script can call this too"""
    from odvae_amd.gan import ActNormLReLU
    c = x.shape[1]
    ref64, ref32 = A.ActNorm(c).double().train(), A.ActNorm(c).train()
    ref64(x.double()); ref32(x)
    loc64, scale64 = ref64.loc.detach().view(c), ref64.scale.detach().view(c)
    loc32, scale32 = ref32.loc.detach().view(c).double(), ref32.scale.detach().view(c).double()
    m = ActNormLReLU(c).to(DEV).train()
    y = m(x.to(DEV))
    assert int(m.initialized) == 1 and m._initialized_host
    loc, scale = m.loc.detach().cpu().view(c).double(), m.scale.detach().cpu().view(c).double()
    figs = [G.figure("loc * scale64", loc * scale64, loc64 * scale64, loc32 * scale64, G.FLOOR_FWD),
            G.figure("scale / scale64", scale / scale64, torch.ones_like(scale64), scale32 / scale64, G.FLOOR_FWD)]
    # the same forward already used the new values
    want = F.leaky_relu(m.scale.detach().cpu() * (x + m.loc.detach().cpu()), A.SLOPE)
    return figs, y.detach().cpu(), want


@pytest.mark.parametrize("rung", B.RUNGS, ids=G.rung_id)
@pytest.mark.parametrize("shape", B.MODEL_SHAPES, ids=B.shape_id)
def test_initialisation_on_the_ladder(hip_lib, shape, rung):
    figs, y, want = init_figures(B.make_input(shape, *rung))
    G.check(figs, "actnorm init %s %s" % (B.shape_id(shape), G.rung_id(rung)))
    close(y, want, FWD_TOL, "initialising forward")


# ---- flags ---------------------------------------------------------------------------------------------------------------------------
def test_flags_over_training_and_eval_forwards(hip_lib):
    from odvae_amd.gan import ActNormLReLU
    shape = (2, 64, 16, 16)
    x = B.make_input(shape, 4, 1.0)
    c = shape[1]
    # eval: a fresh layer stays uninitialised and applies loc = 0, scale = 1
    m = ActNormLReLU(c).to(DEV).eval()
    y = m(x.to(DEV))
    assert int(m.initialized) == 0 and not m._initialized_host
    assert torch.equal(m.loc.detach().cpu(), torch.zeros(1, c, 1, 1)) and torch.equal(m.scale.detach().cpu(), torch.ones(1, c, 1, 1))
    assert torch.equal(y.detach().cpu(), F.leaky_relu(x, A.SLOPE))
    # first training forward: every channel of h = scale (x + loc) has mean 0 and unbiased std 1 (f32 parameters: to a few ulps of them)
    m.train()
    m(x.to(DEV))
    assert int(m.initialized) == 1 and m._initialized_host
    loc, scale = m.loc.detach().cpu().double(), m.scale.detach().cpu().double()
    flat = (scale * (x.double() + loc)).permute(1, 0, 2, 3).reshape(c, -1)
    assert flat.mean(1).abs().max().item() < 1e-5 and (flat.std(1, unbiased=True) - 1).abs().max().item() < 1e-5
    # second training forward, other data: bit-identical parameters
    keep = (m.loc.detach().clone(), m.scale.detach().clone())
    m(B.make_input(shape, 16, 0.01).to(DEV))
    assert torch.equal(m.loc.detach(), keep[0]) and torch.equal(m.scale.detach(), keep[1]) and int(m.initialized) == 1
    # a state_dict round trip into a fresh training-mode layer: the next forward does not initialise again
    fresh = ActNormLReLU(c)
    res = fresh.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys and fresh._initialized_host
    fresh = fresh.to(DEV).train()
    fresh(B.make_input(shape, 16, 0.01).to(DEV))
    assert torch.equal(fresh.loc.detach(), keep[0]) and torch.equal(fresh.scale.detach(), keep[1])
    # ... and into a layer that already lives on the device
    on_dev = ActNormLReLU(c).to(DEV).train()
    on_dev.load_state_dict(m.state_dict(), strict=True)
    on_dev(B.make_input(shape, 16, 0.01).to(DEV))
    assert torch.equal(on_dev.loc.detach(), keep[0]) and torch.equal(on_dev.scale.detach(), keep[1])


def test_fewer_than_two_rows_is_an_error(hip_lib):
    from odvae_amd import lib
    from odvae_amd.gan import ActNormLReLU
    m = ActNormLReLU(8).to(DEV).train()
    with pytest.raises(lib.HipLibraryError, match="at least 2 rows"):
        m(torch.randn(1, 8, 1, 1).to(DEV))
    assert int(m.initialized) == 0 and not m._initialized_host
    m(torch.randn(1, 8, 2, 1).to(DEV))          # two rows are enough
    assert int(m.initialized) == 1 and torch.isfinite(m.scale).all().item()


def test_no_host_synchronisation(hip_lib):
    """Upstream's `self.initialized.item()` waits for the device on every forward; here neither the initialising forward nor the
    steady state does (torch.cuda.set_sync_debug_mode("error") raises at the first synchronisation)."""
    from odvae_amd.gan import ActNormLReLU
    shape = (2, 64, 16, 16)
    warm = ActNormLReLU(shape[1]).to(DEV).train()
    m = ActNormLReLU(shape[1]).to(DEV).train()
    x = B.make_input(shape, 4, 1.0).to(DEV)
    dy = torch.randn(shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    warm(x.clone().requires_grad_(True)).backward(dy)      # workspaces exist from here on
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x1 = x.clone().requires_grad_(True)
        m(x1).backward(dy)                                  # the initialising forward
        x2 = x.clone().requires_grad_(True)
        m(x2).backward(dy)                                  # steady state
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(m.initialized) == 1 and torch.isfinite(x2.grad).all().item() and torch.equal(x1.grad, x2.grad)
