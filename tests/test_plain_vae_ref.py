"""tests/plain_vae_ref.py held to what it restates.  Host only: the float64 restatement of the upstream plain loss against values worked
out by hand on a 2 x 1 x 2 x 2 case, validation_step / log_images against their own parts, the float64 model of the six GAN logit terms
against torch's float64 autograd, the planted faults it must reject, and the precondition of the bit-for-bit inputs."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import plain_vae_ref as R
from oracle.distributions import DiagonalGaussianDistribution

LN2 = math.log(2.0)


# ------------------------------------------------------------------------------------------------------------------------------
# the loss, by hand
# ------------------------------------------------------------------------------------------------------------------------------
def hand_case(**kw):
    """x, x_rec [2,1,2,2]; |x - x_rec| sums to 1.5 and 3.5 per sample; logvar = ln 2; posterior mean (1, -2), logvar (0, ln 4).  The
    discriminator is the identity, so the logits are the images themselves."""
    loss = R.PlainLoss(disc_start=0, logvar_init=LN2, perceptual_weight=0.0, disc_in_channels=1, **kw).double()
    loss.discriminator = nn.Identity()
    loss.logvar.data.fill_(LN2)       # (the constructor made it in f32)
    x = torch.tensor([[1.0, 2.0, 3.0, 4.0], [0.0, -1.0, 0.5, 2.0]], dtype=torch.float64).reshape(2, 1, 2, 2)
    base = torch.tensor([[1.5, 2.0, 2.0, 4.0], [0.0, 0.0, 0.0, 0.0]], dtype=torch.float64).reshape(2, 1, 2, 2)
    gain = torch.ones((), dtype=torch.float64, requires_grad=True)       # the "last layer": x_rec = gain * base
    moments = torch.tensor([[1.0, 0.0], [-2.0, 2 * LN2]], dtype=torch.float64).reshape(2, 2, 1, 1)
    return loss, x, gain * base, gain, DiagonalGaussianDistribution(moments)


def test_generator_phase_by_hand():
    loss, x, xr, gain, post = hand_case(kl_weight=0.5, disc_factor=0.0)
    total, log = loss(x, xr, post, 0, 5, last_layer=gain)
    want = {"train/nll_loss": 1.25 + 4 * LN2, "train/kl_loss": 2.0 - 0.5 * LN2, "train/rec_loss": 0.625, "train/g_loss": -1.1875,
            "train/d_weight": 0.0, "train/disc_factor": 0.0, "train/logvar": LN2, "train/total_loss": 2.25 + 3.75 * LN2}
    assert set(log) == set(want)
    for k, v in want.items():
        assert float(log[k]) == pytest.approx(v, abs=1e-14), k
    assert total.item() == pytest.approx(2.25 + 3.75 * LN2, abs=1e-14)


def test_adaptive_weight_and_per_sample_weights_by_hand():
    loss, x, xr, gain, post = hand_case(kl_weight=0.5, disc_factor=1.0, disc_weight=0.5)
    loss.train()
    # d nll / d gain = sum sign(x_rec - x) base / (exp(logvar) N) = (1.5 - 2) / 4; d g_loss / d gain = -mean(base) = -9.5 / 8
    d_weight = 0.5 * 0.125 / (1.1875 + 1e-4)
    total, log = loss(x, xr, post, 0, 5, last_layer=gain, weights=torch.tensor([1.0, 3.0], dtype=torch.float64))
    assert float(log["train/d_weight"]) == pytest.approx(d_weight, abs=1e-14) and float(log["train/disc_factor"]) == 1.0
    # weighted: (1 (0.75 + 4 ln 2) + 3 (1.75 + 4 ln 2)) / 2; the logged nll_loss stays unweighted
    assert float(log["train/nll_loss"]) == pytest.approx(1.25 + 4 * LN2, abs=1e-14)
    assert float(total) == pytest.approx(3.0 + 8 * LN2 + 0.5 * (2.0 - 0.5 * LN2) + d_weight * -1.1875, abs=1e-13)
    # before disc_start the adaptive weight is still evaluated, the factor is 0
    loss.discriminator_iter_start = 6
    total, log = loss(x, xr, post, 0, 5, last_layer=gain)
    assert float(log["train/disc_factor"]) == 0.0 and float(log["train/d_weight"]) == pytest.approx(d_weight, abs=1e-14)
    assert float(total) == pytest.approx(1.25 + 4 * LN2 + 0.5 * (2.0 - 0.5 * LN2), abs=1e-14)
    # a last layer the graph does not reach: RuntimeError -> only outside training
    stray = torch.ones((), dtype=torch.float64, requires_grad=True)
    with pytest.raises(AssertionError):
        loss(x, xr, post, 0, 5, last_layer=stray)
    loss.eval()
    assert float(loss(x, xr, post, 0, 5, last_layer=stray)[1]["train/d_weight"]) == 0.0
    with pytest.raises(AssertionError):
        loss(x, xr, post, 0, 5, last_layer=gain, cond=x)


@pytest.mark.parametrize("kind,want", [("hinge", 0.5 * (0.4375 + 2.1875)), ("vanilla", None)])
def test_discriminator_phase_by_hand(kind, want):
    loss, x, xr, gain, post = hand_case(disc_loss=kind)
    if want is None:      # 0.5 (mean softplus(-real) + mean softplus(fake)), term by term
        sp = lambda v: math.log1p(math.exp(v))
        want = 0.5 * (sum(sp(-v) for v in x.flatten().tolist()) + sum(sp(v) for v in xr.flatten().tolist())) / 8
    d_loss, log = loss(x, xr, post, 1, 5, split="val")
    assert set(log) == {"val/disc_loss", "val/logits_real", "val/logits_fake"}
    assert float(d_loss) == pytest.approx(want, abs=1e-14) and float(log["val/disc_loss"]) == pytest.approx(want, abs=1e-14)
    assert float(log["val/logits_real"]) == 1.4375 and float(log["val/logits_fake"]) == 1.1875
    assert not d_loss.requires_grad or torch.autograd.grad(d_loss, gain, allow_unused=True)[0] is None       # the reconstruction is detached
    loss.discriminator_iter_start = 6
    assert float(loss(x, xr, post, 1, 5)[0]) == 0.0


def test_model_methods_are_their_parts():
    """validation_step = one forward + the loss at optimizer_idx 0 and 1 with split "val"; log_images = inputs, forward, decode(eps)"""
    torch.manual_seed(3)
    model = R.PlainAutoencoder(R.small_ddconfig(4), dict(disc_start=0, kl_weight=1e-6, disc_weight=0.5), 4).eval()
    batch = {"image": torch.rand(2, 32, 32, 3) * 2 - 1}
    noise = {"posterior_eps": torch.randn(2, 4, 16, 16), "samples_eps": torch.randn(2, 4, 16, 16)}
    with torch.no_grad():
        logs = model.validation_step(batch, noise)
        x = model.get_input(batch, "image")
        xrec, post = model(x, noise["posterior_eps"])
        want = dict(model.loss(x, xrec, post, 0, 0, last_layer=model.decoder.conv_out.weight, split="val")[1])
        want.update(model.loss(x, xrec, post, 1, 0, split="val")[1])
    assert len(logs) == 11 and set(logs) == set(want) and "val/rec_loss" in logs
    for k in want:
        assert torch.equal(logs[k], want[k]), k
    assert x.shape == (2, 3, 32, 32) and torch.equal(x[0, :, 5, 7], batch["image"][0, 5, 7])
    imgs = model.log_images(batch, noise)
    assert list(imgs) == ["samples", "reconstructions", "inputs"] and all(v.shape == (2, 3, 32, 32) for v in imgs.values())
    assert torch.equal(imgs["inputs"], x) and torch.equal(imgs["reconstructions"], xrec)
    assert torch.equal(imgs["samples"], model.decode(noise["samples_eps"]).detach())
    assert list(model.log_images(batch, noise, only_inputs=True)) == ["inputs"]
    assert torch.equal(model(x, None, sample_posterior=False)[0], model.decode(post.mode()))
    model.learning_rate = 1e-4
    owned = {id(q) for o in model.configure_optimizers() for g in o.param_groups for q in g["params"]}
    assert id(model.loss.logvar) not in owned and id(model.decoder.conv_out.weight) in owned      # logvar is in neither optimizer


# ------------------------------------------------------------------------------------------------------------------------------
# the six logit terms
# ------------------------------------------------------------------------------------------------------------------------------
def test_logit_model_by_hand():
    real, fake = np.array([1.0, 2.0, 0.0, -3.0]), np.array([-1.0, 0.5])
    out = R.logit_terms_f64(real, fake)
    assert out[:4].tolist() == [0.0, -0.25, (0 + 0 + 1 + 4) / 4, (0 + 1.5) / 2]
    sp = lambda v: math.log1p(math.exp(v))
    assert out[4] == pytest.approx((sp(-1) + sp(-2) + sp(0) + sp(3)) / 4, abs=1e-15) and out[5] == pytest.approx((sp(-1) + sp(0.5)) / 2, abs=1e-15)
    dreal, dfake = R.logit_terms_grad_f64(real, fake, [1.0, 2.0, 4.0, 8.0, 0.0, 0.0])
    assert dreal.tolist() == [0.25, 0.25, -0.75, -0.75] and dfake.tolist() == [1.0, 5.0]      # relu'(0) = 0 at real = 1 and fake = -1
    assert R.logit_terms_f64(None, fake)[[0, 2, 4]].tolist() == [0.0, 0.0, 0.0] and R.logit_terms_grad_f64(None, fake, np.ones(6))[0] is None


@pytest.mark.parametrize("n_real,n_fake", [(1, 1), (65, 65), (257, 900), (900, 63)])
def test_logit_model_is_torch_in_float64(n_real, n_fake):
    for make, dout in ((R.dyadic_logits, R.DOUT_HINGE), (R.softplus_logits, R.DOUT_FULL)):
        real, fake = make(n_real, 1), make(n_fake, 2)
        out, dr, df = R.torch_logit_terms(real, fake, dout, torch.float64)
        want = R.logit_terms_f64(real, fake)
        wr, wf = R.logit_terms_grad_f64(real, fake, dout)
        # torch's softplus switches to the identity past 20: e^-20 = 2e-9 of the value there, far below f32
        assert np.abs(out.numpy() - want).max() <= 3e-9 * max(1.0, np.abs(want).max())
        assert np.abs(dr.numpy() - wr).max() <= 3e-9 / n_real * 2 and np.abs(df.numpy() - wf).max() <= 3e-9 / n_fake * 2
    assert np.isfinite(R.logit_terms_f64(np.array([100.0, -100.0]), np.array([100.0, -100.0]))).all()
    nan = R.logit_terms_f64(np.array([1.0, np.nan]), np.array([1.0, 2.0]))
    assert np.isnan(nan[[0, 2, 4]]).all() and np.isfinite(nan[[1, 3, 5]]).all()


def test_logit_model_rejects_the_planted_faults():
    real, fake = R.dyadic_logits(65, 1), R.dyadic_logits(257, 2)
    assert (real == 1.0).any() and (fake == -1.0).any()
    good = R.logit_terms_f64(real, fake)
    gr, gf = R.logit_terms_grad_f64(real, fake, R.DOUT_HINGE)
    f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32)
    seen = []
    for fault in R.FAULTS:
        out = R.logit_terms_f64(real, fake, fault=fault)
        dr, df = R.logit_terms_grad_f64(real, fake, R.DOUT_HINGE, fault=fault)
        # the hinge terms, the means and their gradients are compared bit for bit: any change at all is a rejection
        hinge = not np.array_equal(f32(out[:4]), f32(good[:4])) or not np.array_equal(f32(dr), f32(gr)) or not np.array_equal(f32(df), f32(gf))
        # the softplus terms at +-100: the naive log(1 + exp(x)) overflows
        sp = R.logit_terms_f64(R.softplus_logits(64, 1), R.softplus_logits(64, 2), fault=fault)
        if hinge or not np.isfinite(sp).all():
            seen.append(fault)
    assert seen == R.FAULTS, "unnoticed: %s" % sorted(set(R.FAULTS) - set(seen))
    # each for its own reason
    dr, df = R.logit_terms_grad_f64(real, fake, R.DOUT_HINGE, fault="le_for_lt")
    assert (dr != gr).sum() == (real == 1.0).sum() and (df != gf).sum() == (fake == -1.0).sum()
    assert np.array_equal(R.logit_terms_f64(real, real, fault="wrong_n"), R.logit_terms_f64(real, real))       # n_real = n_fake hides it
    assert not np.isfinite(R.logit_terms_f64(None, np.array([100.0]), fault="naive_softplus")[5])


@pytest.mark.parametrize("n", R.SIZES + [R.PAST_CAP])
def test_dyadic_inputs_keep_every_partial_sum_exact_in_f32(n):
    for seed in (1, 2):
        x = R.dyadic_logits(n, seed)
        assert x.dtype == np.float32
        R.assert_partial_sums_exact(x)
        for t in (x, np.maximum(1 - x, 0), np.maximum(1 + x, 0)):
            assert np.array_equal(np.cumsum(t, dtype=np.float32).astype(np.float64), np.cumsum(t.astype(np.float64)))
    if n >= 9:
        assert (x == 1.0).any() and (x == -1.0).any() and x.min() == -4.0 and x.max() == 4.0
    with pytest.raises(AssertionError):
        R.assert_partial_sums_exact(np.array([1.0 / 3.0]))
    assert R.PAST_CAP > R.GRID_CAP_BLOCKS * 256


def test_torch_softplus_figures_are_the_recorded_ones():
    """torch's f32 F.softplus / mean and autograd on this host against the float64 model, on the logits the GPU test uses: the recorded
    figures (the kernel is held to 4x of them) are not below what is measured here; a result rounded once from float64 is inside them"""
    worst, once = {}, {}
    for n_real, n_fake in R.SOFTPLUS_CASES:
        real, fake = R.softplus_logits(n_real, 1), R.softplus_logits(n_fake, 2)
        out, dr, df = R.torch_logit_terms(real, fake, R.DOUT_FULL, torch.float32)
        for k, f in R.softplus_figures(out.numpy(), dr.numpy(), df.numpy(), real, fake, R.DOUT_FULL).items():
            worst[k] = max(worst.get(k, 0.0), f)
        want, (wr, wf) = R.logit_terms_f64(real, fake), R.logit_terms_grad_f64(real, fake, R.DOUT_FULL)
        for k, f in R.softplus_figures(want.astype(np.float32), wr.astype(np.float32), wf.astype(np.float32), real, fake, R.DOUT_FULL).items():
            once[k] = max(once.get(k, 0.0), f)
    print("torch f32 softplus terms: %s; rounded once from float64: %s" % (worst, once))
    assert set(worst) == set(R.TORCH_SOFTPLUS_FIGURES)
    for k, f in worst.items():
        assert f <= R.TORCH_SOFTPLUS_FIGURES[k] <= 1.25 * f, (k, f)
        assert once[k] <= 1.0 < R.SOFTPLUS_MARGIN * R.TORCH_SOFTPLUS_FIGURES[k], (k, once[k])


def test_softplus_inputs_hold_the_named_points():
    x = R.softplus_logits(900, 1)
    for v in (0.0, 1e-8, 1.0, 20.0, 20.5, 100.0):
        assert (x == np.float32(v)).any() and (x == np.float32(-v)).any()
