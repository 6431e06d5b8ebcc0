"""The VQ family's public surface without a GPU: the yaml instantiates, the checkpoint keys, the optimizers, what raises, and the C ABI
declarations of csrc/vq_f32.hip."""
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
VQ_YAML = os.path.join(GOLDEN, "autoencoder_vq_plain.yaml")
VQ_SYMBOLS = ["odvae_vq_plan", "odvae_vq_assign_workspace_bytes", "odvae_vq_assign_f32", "odvae_vq_loss_finalize",
              "odvae_vq_backward_workspace_bytes", "odvae_vq_backward_f32", "odvae_vq_gather_f32", "odvae_vq_usage"]


def load(overrides=()):
    from odvae_amd.config import Config, instantiate_from_config
    config = Config.merge(Config.load(VQ_YAML), Config.from_dotlist(list(overrides)))
    return config, instantiate_from_config(config.model)


def test_yaml_instantiates_with_the_checkpoint_layout():
    from odvae_amd.autoencoder import VQModel
    from odvae_amd.losses import VQLPIPSWithDiscriminator
    config, model = load()
    assert type(model) is VQModel and type(model.loss) is VQLPIPSWithDiscriminator
    p = config.model.params
    sd = model.state_dict()
    assert tuple(sd["quantize.embedding.weight"].shape) == (p.n_embed, p.embed_dim)
    assert tuple(sd["quant_conv.weight"].shape) == (p.embed_dim, p.ddconfig.z_channels, 1, 1)
    assert tuple(sd["post_quant_conv.weight"].shape) == (p.ddconfig.z_channels, p.embed_dim, 1, 1)
    assert tuple(sd["encoder.conv_out.weight"].shape)[0] == p.ddconfig.z_channels          # double_z: False
    assert not any("logvar" in k for k in sd), "the VQ loss has no logvar"
    w = sd["quantize.embedding.weight"]
    assert w.abs().max().item() <= 1.0 / p.n_embed and w.abs().max().item() > 0.5 / p.n_embed      # uniform(-1/n_e, 1/n_e)
    assert model.quantize.beta == 0.25 and model.quantize.legacy is True and model.image_key == "image"


def test_optimizers_hold_what_upstream_gives_them():
    _, model = load(["model.params.lr_g_factor=0.5"])
    model.learning_rate = 2e-4
    (opt_ae, opt_disc), sched = model.configure_optimizers()
    assert sched == []
    ids = lambda opt: {id(p) for g in opt.param_groups for p in g["params"]}
    code = model.quantize.embedding.weight
    assert id(code) in ids(opt_ae) and id(code) not in ids(opt_disc)
    want_ae = {id(p) for m in (model.encoder, model.decoder, model.quantize, model.quant_conv, model.post_quant_conv) for p in m.parameters()}
    assert ids(opt_ae) == want_ae
    assert ids(opt_disc) == {id(p) for p in model.loss.discriminator.parameters()}
    assert opt_ae.param_groups[0]["lr"] == 1e-4 and opt_disc.param_groups[0]["lr"] == 2e-4       # lr_g_factor on the generator only
    assert tuple(opt_ae.param_groups[0]["betas"]) == (0.5, 0.9) and tuple(opt_disc.param_groups[0]["betas"]) == (0.5, 0.9)


@pytest.mark.parametrize("override", ["model.params.remap=used.npy", "model.params.batch_resize_range=[128,256]",
                                      "model.params.scheduler_config={target: x}", "model.params.lossconfig.params.pixel_loss=l2",
                                      "model.params.lossconfig.params.perceptual_loss=clips"])
def test_unreachable_options_are_loud(override):
    with pytest.raises(NotImplementedError):
        load([override])


def test_quantizer_surface():
    from odvae_amd.quantize import VectorQuantizer
    q = VectorQuantizer(16, 4, 0.25, sane_index_shape=True, legacy=False)
    assert list(q.state_dict()) == ["embedding.weight"] and q.sane_index_shape and not q.legacy
    with pytest.raises(NotImplementedError):
        VectorQuantizer(16, 4, 0.25, remap="used.npy")
    from odvae_amd import lib
    with pytest.raises(lib.HipLibraryError):      # no CPU fallback
        q(torch.zeros(1, 4, 2, 2))


def test_interface_and_use_ema_build():
    from odvae_amd.autoencoder import VQModel, VQModelInterface
    config, _ = load()
    p = config.model.params.to_container()
    m = VQModelInterface(p["embed_dim"], p["ddconfig"], p["lossconfig"], p["n_embed"], use_ema=True)
    assert isinstance(m, VQModel) and m.use_ema and m.embed_dim == p["embed_dim"]
    assert float(m.model_ema.decay) == pytest.approx(0.9999)
    assert any(k.startswith("model_ema.") for k in m.state_dict())


def test_header_declares_the_vq_entry_points_and_the_binding_follows():
    from odvae_amd import lib
    names = lib.header_symbols()
    for s in VQ_SYMBOLS:
        assert s in names and s in lib.PROTOTYPES, s
    import ctypes
    res, args = lib.PROTOTYPES["odvae_vq_usage"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    res, args = lib.PROTOTYPES["odvae_vq_assign_workspace_bytes"]
    assert res is ctypes.c_size_t and args == [ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    assert len(lib.PROTOTYPES["odvae_vq_assign_f32"][1]) == 17 and len(lib.PROTOTYPES["odvae_vq_backward_f32"][1]) == 19
    assert lib.ABI_VERSION == 4
    src = open(os.path.join(os.path.dirname(lib.HEADER_PATH), "..", "generative-detection_amd", "csrc", "vq_f32.hip")).read()
    for s in VQ_SYMBOLS:
        assert s + "(" in src, s


def test_plan_is_a_host_function():
    from odvae_amd import lib, ops
    lib.load()
    p = ops.vq_plan(131072, 8192, 3)
    assert p["tile_rows"] == 64 and p["chunk"] == 64 and p["slab_depth"] == 4 and p["nsplit"] == 1
    p = ops.vq_plan(8192, 16384, 8)
    assert p["nsplit"] > 1 and p["nsplit"] * p["codes_per_split"] >= 16384 and p["codes_per_split"] % p["chunk"] == 0
    assert ops.vq_plan(100, 300, 64)["nslabs"] == 2
    with pytest.raises(lib.HipLibraryError):
        ops.vq_plan(100, 300, 513)
    with pytest.raises(lib.HipLibraryError):
        ops.vq_plan(100, (1 << 20) + 1, 4)
