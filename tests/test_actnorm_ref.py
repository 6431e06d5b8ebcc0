"""`use_actnorm` on the host: the restatement tests/actnorm_ref.py does what the published algorithm says, the closed forms the HIP
backward evaluates equal autograd in float64, and the product's modules construct with the restatement's state layout."""
import os

import pytest
import torch

import actnorm_ref as A

YAML = os.path.join(os.path.dirname(__file__), "golden", "autoencoder_kl_16x16x16.yaml")


def _x(shape=(3, 6, 7, 5), seed=1, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    c = shape[1]
    return (torch.randn(shape, generator=g, dtype=dtype) * (0.5 + torch.arange(c, dtype=dtype)).view(1, c, 1, 1)
            + torch.linspace(-3, 3, c, dtype=dtype).view(1, c, 1, 1))


def test_first_training_forward_standardises_every_channel():
    x = _x()
    layer = A.ActNorm(6).double().train()
    h = layer(x)
    flat = h.detach().permute(1, 0, 2, 3).reshape(6, -1)
    assert int(layer.initialized) == 1
    assert flat.mean(1).abs().max().item() < 1e-12
    # scale = 1 / (std + 1e-6): the output's std is std / (std + 1e-6)
    std = x.permute(1, 0, 2, 3).reshape(6, -1).std(1, unbiased=True)
    assert torch.allclose(flat.std(1, unbiased=True), std / (std + A.EPS), rtol=0, atol=1e-12)
    assert (flat.std(1, unbiased=True) - 1).abs().max().item() < 4e-6


def test_second_training_forward_leaves_the_parameters_bit_identical():
    layer = A.ActNorm(6).double().train()
    layer(_x(seed=1))
    loc, scale = layer.loc.detach().clone(), layer.scale.detach().clone()
    layer(_x(seed=2) * 3 + 1)
    assert torch.equal(layer.loc.detach(), loc) and torch.equal(layer.scale.detach(), scale) and int(layer.initialized) == 1


def test_eval_forward_of_a_fresh_layer_stays_uninitialised():
    x = _x()
    layer = A.ActNorm(6).double().eval()
    h = layer(x)
    assert int(layer.initialized) == 0
    assert torch.equal(h, x) and torch.equal(layer.loc.detach(), torch.zeros(1, 6, 1, 1, dtype=torch.float64))


def test_weights_init_leaves_loc_and_scale_alone():
    from odvae_amd import gan
    for net, init in ((A.NLayerDiscriminator(), A.weights_init), (gan.NLayerDiscriminator(use_actnorm=True), gan.weights_init)):
        net.apply(init)
        layers = A.actnorm_layers(net)
        assert len(layers) == 3
        for m in layers:
            assert torch.equal(m.loc.detach(), torch.zeros_like(m.loc)) and torch.equal(m.scale.detach(), torch.ones_like(m.scale))
        assert net.main[2].bias is not None and net.main[2].weight.std().item() < 0.03


def test_closed_forms_equal_autograd_in_float64():
    g = torch.Generator().manual_seed(3)
    x = _x((2, 5, 4, 3))
    loc = torch.randn(1, 5, 1, 1, generator=g, dtype=torch.float64)
    scale = torch.randn(1, 5, 1, 1, generator=g, dtype=torch.float64)       # both signs: lrelu' follows the sign of h, not of x + loc
    dy = torch.randn(x.shape, generator=g, dtype=torch.float64)
    for got, want in zip(A.closed_form_backward(x, loc, scale, dy), A.autograd_backward(x, loc, scale, dy)):
        assert got.shape == want.shape
        assert torch.allclose(got, want, rtol=1e-13, atol=1e-13)


def test_product_discriminator_has_the_restatements_state():
    from odvae_amd import gan
    for n_layers in (3, 2):
        ref = A.NLayerDiscriminator(n_layers=n_layers).apply(A.weights_init)
        net = gan.NLayerDiscriminator(n_layers=n_layers, use_actnorm=True).apply(gan.weights_init)
        sd, ref_sd = net.state_dict(), ref.state_dict()
        assert list(sd) == list(ref_sd)
        if n_layers == 3:
            want = ["main.%d.%s" % (i, k) for i in (0, 2, 5, 8, 11) for k in ("weight", "bias")]
            want += ["main.%d.%s" % (i, k) for i in (3, 6, 9) for k in ("loc", "scale", "initialized")]
            assert sorted(sd) == sorted(want)
        for k in sd:
            assert sd[k].shape == ref_sd[k].shape and sd[k].dtype == ref_sd[k].dtype, k
        assert sd["main.3.initialized"].dtype == torch.uint8 and tuple(sd["main.3.loc"].shape) == (1, 128, 1, 1)
        # both directions, strict; an "initialised" flag arrives in the product's host-side mirror
        ref.main[3].initialized.fill_(1)
        res = net.load_state_dict(ref.state_dict(), strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        assert net.main[3]._initialized_host and not net.main[6]._initialized_host
        res = ref.load_state_dict(net.state_dict(), strict=True)
        assert not res.missing_keys and not res.unexpected_keys
    # the default stays the BatchNorm PatchGAN
    assert sorted(gan.NLayerDiscriminator().state_dict()) == sorted(__import__("oracle.losses", fromlist=["x"]).NLayerDiscriminator().state_dict())


def test_pose_loss_constructs_with_use_actnorm():
    from odvae_amd import gan, synthetic
    from odvae_amd.config import instantiate_from_config
    mcfg, _ = synthetic.model_config(YAML, latent_hw=4, ch=32)
    mcfg.params.lossconfig.params["use_actnorm"] = True
    loss = instantiate_from_config(mcfg.params.lossconfig)
    layers = loss.discriminator.actnorm_layers()
    assert len(layers) == 3 and all(isinstance(m, gan.ActNormLReLU) for m in layers)
    assert loss.discriminator.actnorm_uninitialized()
    assert "discriminator.main.3.loc" in loss.state_dict() and "discriminator.main.3.running_mean" not in loss.state_dict()
    with pytest.raises(NotImplementedError):
        gan.ActNormLReLU(8, logdet=True)


def test_new_symbols_are_declared():
    from odvae_amd import lib
    names = lib.header_symbols()
    for name in ("odvae_actnorm_workspace_bytes", "odvae_actnorm_init_f32", "odvae_actnorm_lrelu_fwd_f32", "odvae_actnorm_lrelu_bwd_f32"):
        assert name in names and name in lib.PROTOTYPES
