"""Host logic: the reference's target:/params: config surface, learning-rate rule and module tree (CPU only)."""
import hashlib
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "tests", "golden", "autoencoder_kl_16x16x16.yaml")
REF_DIGEST = os.path.join(ROOT, "tests", "golden", "reference_config.json")   # size and SHA-256 of the reference's own yaml


def test_yaml_fixture_is_the_untouched_reference_config():
    ref = json.load(open(REF_DIGEST))
    data = open(YAML, "rb").read()
    assert ref["file"].endswith(os.path.basename(YAML))
    assert len(data) == ref["bytes"] and hashlib.sha256(data).hexdigest() == ref["sha256"]


def test_config_load_merge_dotlist():
    from odvae_amd.config import Config
    cfg = Config.load(YAML)
    assert cfg.model.target == "src.models.autoencoder.PoseAutoencoder"
    assert cfg.model.params.ddconfig.ch_mult == [1, 1, 2, 2, 4]
    cli = Config.from_dotlist(["model.params.ddconfig.ch=32", "data.params.batch_size=2", "model.params.feat_dims=[16,4,4]"])
    merged = Config.merge(cfg, cli)
    assert merged.model.params.ddconfig.ch == 32 and merged.model.params.ddconfig.z_channels == 16
    assert merged.data.params.batch_size == 2 and merged.model.params.feat_dims == [16, 4, 4]
    assert cfg.model.params.ddconfig.ch == 128  # inputs untouched
    lightning = merged.pop("lightning")
    assert lightning.trainer.gradient_clip_val == 1.0 and "lightning" not in merged


def test_instantiate_from_config_contract():
    from odvae_amd.config import instantiate_from_config
    with pytest.raises(KeyError, match="Expected key `target` to instantiate."):
        instantiate_from_config({"params": {}})
    lin = instantiate_from_config({"target": "torch.nn.Linear", "params": {"in_features": 3, "out_features": 2}})
    assert isinstance(lin, torch.nn.Linear)


def test_learning_rate_rule():
    from odvae_amd.config import Config, configure_learning_rate
    cfg = Config.load(YAML)

    class M:
        pass
    m = configure_learning_rate(cfg, M(), cfg.lightning.trainer, scale_lr=True, ngpu=1)
    assert abs(m.learning_rate - 12 * 4.5e-6) < 1e-12  # 1 * 1 * 12 * 4.5e-6 = 5.4e-5 (train.py:383)
    m = configure_learning_rate(cfg, M(), cfg.lightning.trainer, scale_lr=False)
    assert m.learning_rate == 4.5e-6


def test_untouched_yaml_targets_resolve_and_state_dict_keys():
    """Every `target:` of the model section resolves to the HIP-backed classes; parameter counts and checkpoint key
    scheme are the reference's."""
    from odvae_amd import synthetic
    from odvae_amd.autoencoder import PoseAutoencoder
    from odvae_amd.losses import PoseLoss
    model = synthetic.build_model(YAML, phase="asis", perceptual_weight=1.0, disc_factor=1.0, disc_start=30000)
    assert isinstance(model, PoseAutoencoder) and isinstance(model.loss, PoseLoss)
    assert abs(model.learning_rate - 5.4e-5) < 1e-12
    n = lambda m: sum(p.numel() for p in m.parameters())
    assert n(model.encoder) + n(model.quant_conv_obj) + n(model.quant_conv_pose) == 26691408
    assert n(model.decoder) + n(model.post_quant_conv) == 38980243
    assert n(model.pose_encoder) == 3089984 and n(model.pose_decoder) == 2312527
    assert n(model.loss.discriminator) == 2765633
    keys = set(model.state_dict().keys())
    for k in ["encoder.conv_in.weight", "encoder.down.0.block.1.norm2.bias", "encoder.down.2.attn.1.proj_out.weight",
              "encoder.down.3.downsample.conv.weight", "encoder.mid.attn_1.q.weight", "encoder.norm_out.weight",
              "decoder.up.4.upsample.conv.bias", "decoder.up.1.block.0.nin_shortcut.weight", "decoder.up.2.attn.2.k.bias",
              "decoder.conv_out.weight", "quant_conv_obj.weight", "quant_conv_pose.bias", "post_quant_conv.weight",
              "pose_encoder.coord_linear.weight", "pose_encoder.latent_linear.weight", "pose_encoder.layers.3.bias",
              "pose_decoder.layers.4.weight", "loss.logvar", "loss.discriminator.main.0.bias",
              "loss.discriminator.main.3.running_mean", "loss.discriminator.main.11.weight"]:
        assert k in keys, k
    assert tuple(model.get_last_layer().shape) == (3, 128, 3, 3)       # autoencoder.py:311
    assert "encoder.down.4.downsample.conv.weight" not in keys and "decoder.up.0.upsample.conv.weight" not in keys
    opts, scheds = model.configure_optimizers()
    assert scheds == [] and len(opts) == 2
    n_ae = sum(p.numel() for g in opts[0].param_groups for p in g["params"])
    assert n_ae == 26691408 + 38980243 + 3089984 + 2312527           # 71 074 162: loss.logvar is in no optimizer
    assert opts[0].param_groups[0]["betas"] == (0.5, 0.9) and opts[0].param_groups[0]["lr"] == model.learning_rate


def test_dropout_schedule_and_global_step_thresholds():
    from odvae_amd import synthetic
    model = synthetic.build_model(YAML, phase="asis", ch=32)
    pre, gen, warm = 30000, 45000, 45000
    assert model.encoder_pretrain_steps == pre and model.pose_conditioned_generation_steps == gen
    for step, want in [(0, 1.0), (pre + gen - 1, 1.0), (pre + gen + warm, 0.7),
                       (pre + gen, 1.0 - 0.3 * gen / warm)]:   # QUIRK: ramp measured from `pre`, autoencoder.py:200
        model._global_step = step
        assert abs(model._get_dropout_prob() - want) < 1e-12, step
    # the loss keeps its own default of 7000 pose-conditioned steps (contperceptual.py:31; lossconfig omits the key)
    assert model.loss.pose_conditioned_generation_steps == 7000
