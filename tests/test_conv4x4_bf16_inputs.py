"""Host tests (no device) of tests/conv4x4_bf16_inputs.py -- the generators, the float64 host models of the 16-tap kernels, the planted
faults the checker must reject -- and of the precision plumbing of the bf16 discriminator that needs no device.
On the parent commit the plumbing tests fail: NLayerDiscriminator has no set_precision."""
import pytest
import torch

import exact_inputs as E
import conv4x4_bf16_inputs as M

BF = torch.bfloat16


def case_of(entry, **kw):
    name, stride, n, cin, cout, h, w, bias = entry
    return M.make_case(stride, n, cin, cout, h, w, bias=bias, **kw)


@pytest.mark.parametrize("entry", M.CASES + [M.WGRAD_SPLIT_CASE], ids=lambda e: e[0])
def test_cases_are_exactly_summable(entry):
    c = case_of(entry)
    s = M.assert_exactly_summable(c)
    assert s["worst"] < E.LIMIT
    ho, wo = M.out4(entry[5], entry[1]), M.out4(entry[6], entry[1])
    assert tuple(c["dy"].shape) == (entry[2], entry[4], ho, wo) and ho >= 1 and wo >= 1


def test_recipe_a_stays_exact_at_the_deepest_reduction():
    """K = 16 * 512: 8192 products of magnitude at most 8 = 64 units of 2^-3 -> at most 2^19 units, under 2^24; asserted on the tensors"""
    c = M.make_case(1, 1, 512, 8, 5, 6, bias=True)
    assert c["x"].abs().max() <= 4 and c["w"].abs().max() <= 2
    s = M.assert_exactly_summable(c)
    assert s["forward"] <= 16 * 512 * 64 + 16 <= 2 ** 19 + 16 < E.LIMIT
    # and the condition does refuse operands that are too large for it
    big = dict(c, x=c["x"] * 64, units=dict(c["units"]))
    with pytest.raises(AssertionError):
        M.assert_exactly_summable(dict(big, w=c["w"] * 128))


def test_recipe_l_accumulators_are_multiples_of_five_units():
    c = M.make_case(2, 2, 3, 64, 9, 11, bias=True, recipe="L")
    M.assert_exactly_summable(c)
    acc = M.conv_f64(c["x"], c["w"], c["b"], 2)
    assert torch.equal(torch.round(acc / 0.625) * 0.625, acc) and (acc < 0).any()
    fifth = torch.where(acc > 0, acc, acc / 5)
    assert torch.equal(torch.round(fifth / 0.125) * 0.125, fifth), "a negative accumulator's fifth is a whole number of units"
    # the kernel multiplies by the f32 0.2: the f32 product of an exact multiple of 5 units is the exact fifth
    assert torch.equal((acc.float() * 0.2).double()[acc < 0], (acc / 5)[acc < 0])


@pytest.mark.parametrize("entry", M.CASES, ids=lambda e: e[0])
def test_host_models_agree_with_torch(entry):
    c = case_of(entry)
    x, w, b, dy, s = c["x"], c["w"], c["b"], c["dy"], c["stride"]
    assert torch.equal(M.forward_model(x, w, b, s), M.conv_f64(x, w, b, s))
    assert torch.equal(M.dgrad_model(dy, w, x.shape, s), M.dgrad_f64(dy, w, x.shape, s))
    assert torch.equal(M.wgrad_model(x, dy, s), M.wgrad_f64(x, dy, w.shape, s))


def test_both_dgrad_models_on_random_float64():
    g = torch.Generator().manual_seed(3)
    for stride, h, w in ((1, 6, 7), (2, 9, 11), (2, 10, 12), (2, 2, 3)):
        x_shape = (2, 5, h, w)
        wt = torch.randn(7, 5, 4, 4, generator=g, dtype=torch.float64)
        dy = torch.randn(2, 7, M.out4(h, stride), M.out4(w, stride), generator=g, dtype=torch.float64)
        torch.testing.assert_close(M.dgrad_model(dy, wt, x_shape, stride), M.dgrad_f64(dy, wt, x_shape, stride), rtol=1e-12, atol=1e-12)


def rejected(got64, want64, what):
    with pytest.raises(AssertionError):
        E.assert_bits_equal(E.rne(got64), E.rne(want64), what)


def test_planted_faults_are_rejected():
    """each fault in a host model of the kernel it belongs to; the checker (bit equality after the one rounding) must refuse every one"""
    c2 = M.make_case(2, 2, 8, 16, 9, 11, bias=True)       # stride 2, both sizes odd
    c1 = M.make_case(1, 2, 8, 16, 6, 7, bias=True)
    for c in (c1, c2):
        x, w, b, dy, s = c["x"], c["w"], c["b"], c["dy"], c["stride"]
        y, dx, dw = M.conv_f64(x, w, b, s), M.dgrad_f64(dy, w, x.shape, s), M.wgrad_f64(x, dy, w.shape, s)
        E.assert_bits_equal(E.rne(M.forward_model(x, w, b, s)), E.rne(y), "sound forward model")
        rejected(M.forward_model(x, w, b, s, "swap_taps"), y, "forward: swapped tap pair")
        rejected(M.forward_model(x, w, b, s, "pad2"), y, "forward: pad 1 taken as pad 2")
        rejected(M.dgrad_model(dy, w, x.shape, s, "swap_taps" if s == 1 else "wrong_parity"), dx, "dgrad fault")
        rejected(M.wgrad_model(x, dy, s, "swap_taps"), dw, "wgrad: swapped tap pair")
        rejected(M.wgrad_model(x, dy, s, "pad2"), dw, "wgrad: pad 1 taken as pad 2")
    x, w, b, dy = c2["x"], c2["w"], c2["b"], c2["dy"]
    rejected(M.dgrad_s1_model(c1["dy"], c1["w"], c1["x"].shape, "pad2"), M.dgrad_f64(c1["dy"], c1["w"], c1["x"].shape, 1), "dgrad: pad 2 taken as pad 1")
    rejected(M.dgrad_s2_model(dy, w, x.shape, "wrong_parity"), M.dgrad_f64(dy, w, x.shape, 2), "dgrad: wrong parity class")
    assert x.shape[2] % 2 == 1
    rejected(M.forward_model(x, w, b, 2, "drop_last_row"), M.conv_f64(x, w, b, 2), "forward: dropped last odd row")
    rejected(M.wgrad_model(x, dy, 2, "drop_last_row"), M.wgrad_f64(x, dy, w.shape, 2), "wgrad: dropped last odd row")
    # LeakyReLU after the rounding instead of before
    cl = M.make_case(2, 2, 3, 64, 9, 11, bias=True, recipe="L")
    acc = M.conv_f64(cl["x"], cl["w"], cl["b"], 2)
    with pytest.raises(AssertionError):
        E.assert_bits_equal(M.lrelu_f64(acc, "lrelu_after_round"), M.lrelu_f64(acc), "LeakyReLU after the rounding")


def test_nan_footprint_matches_torch():
    for stride, (iy, ix) in ((1, (5, 9)), (2, (5, 9)), (1, (10, 18)), (2, (10, 18)), (2, (0, 0))):
        x = torch.zeros(1, 1, 11, 19, dtype=torch.float64)
        x[0, 0, iy, ix] = float("nan")
        y = M.conv_f64(x, torch.ones(1, 1, 4, 4, dtype=torch.float64), None, stride)
        assert torch.equal(torch.isnan(y)[0, 0], M.nan_footprint(y.shape[2:], stride, iy, ix))


# ------------------------------------------------------------------------------------------------------------------------------
# plumbing that needs no device
# ------------------------------------------------------------------------------------------------------------------------------
def test_discriminator_set_precision_values():
    from odvae_amd.gan import NLayerDiscriminator, Conv4x4, LeakyReLU
    d = NLayerDiscriminator()
    assert d.compute_dtype == torch.float32 and all(m.compute_dtype == torch.float32 for m in d.main if isinstance(m, Conv4x4))
    before = {k: (v.dtype, tuple(v.shape)) for k, v in d.state_dict().items()}
    for p in ("bf16", "bf16-mixed"):
        assert d.set_precision(p) is d and d.compute_dtype == BF
        convs = [m for m in d.main if isinstance(m, Conv4x4)]
        assert all(m.compute_dtype == BF for m in convs)
        assert convs[0].fused_lrelu == pytest.approx(0.2) and all(m.fused_lrelu is None for m in convs[1:])
        assert [m.fused for m in d.main if isinstance(m, LeakyReLU)] == [True]
        assert {k: (v.dtype, tuple(v.shape)) for k, v in d.state_dict().items()} == before
        assert all(q.dtype == torch.float32 for q in d.parameters()) and all(q.dtype in (torch.float32, torch.int64) for q in d.buffers())
    for p in (32, "32", "32-true", "fp32"):
        d.set_precision(p)
        assert d.compute_dtype == torch.float32 and all(m.compute_dtype == torch.float32 and m.fused_lrelu is None for m in d.main if isinstance(m, Conv4x4))
        assert [m.fused for m in d.main if isinstance(m, LeakyReLU)] == [False]
    for bad in (16, "16", "fp16", "bf", None):
        with pytest.raises(ValueError, match="the discriminator computes in 32"):
            d.set_precision(bad)
    assert d.compute_dtype == torch.float32
    # checkpoints interchange: a state_dict of one loads into the other, strictly
    e = NLayerDiscriminator().set_precision("bf16")
    res = e.load_state_dict(d.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_actnorm_discriminator_refuses_bf16():
    from odvae_amd.gan import NLayerDiscriminator
    d = NLayerDiscriminator(use_actnorm=True)
    with pytest.raises(ValueError, match="ActNorm"):
        d.set_precision("bf16")
    assert d.compute_dtype == torch.float32
    assert d.set_precision(32) is d


def _model(disc=True):
    import os
    from odvae_amd import synthetic
    yaml = os.path.join(os.path.dirname(__file__), "golden", "autoencoder_kl_16x16x16.yaml")
    return synthetic.build_model(yaml, batch_size_for_lr=12, latent_hw=4, ch=32, perceptual_weight=0.0, disc_factor=1.0 if disc else 0.0)


def test_model_plumbing(monkeypatch):
    """(the Trainer's argument needs a device for its optimizers: tests/test_disc_bf16_gpu.py)"""
    from odvae_amd import ops
    model = _model()
    disc = model.loss.discriminator
    assert disc.compute_dtype == torch.float32
    model.set_precision("bf16")
    assert disc.compute_dtype == torch.float32, "precision: bf16 alone must leave the discriminator f32"
    model.set_precision("bf16", discriminator_precision="bf16")
    assert disc.compute_dtype == BF and model.loss.perceptual_loss.compute_dtype == torch.float32
    model.set_precision("bf16")
    assert disc.compute_dtype == BF, "discriminator_precision=None leaves the discriminator alone"
    model.set_precision(32, discriminator_precision=32)
    assert disc.compute_dtype == torch.float32
    monkeypatch.setattr(ops, "DISC_BF16", True)        # ODVAE_DISC_BF16=1
    model.set_precision("bf16")
    assert disc.compute_dtype == BF
    model.set_precision(32)
    assert disc.compute_dtype == torch.float32
    with pytest.raises(ValueError):
        model.set_precision("bf16", discriminator_precision="fp16")


def test_discriminator_precision_without_a_discriminator_raises():
    model = _model()
    del model.loss.discriminator
    with pytest.raises(ValueError, match="no discriminator"):
        model.set_precision("bf16", discriminator_precision="bf16")
