"""Synthetic batches and config overrides for benchmarks, smoke and tests: there is no network for
nuScenes, the reference's dataset-stats pickle is not shipped, and the reference's dataloader is out of scope."""
import copy
import math

import torch

from .config import Config, instantiate_from_config

LABELS = ['car', 'truck', 'trailer', 'bus', 'construction_vehicle', 'bicycle', 'motorcycle', 'pedestrian',
          'traffic_cone', 'barrier', 'background']  # yaml:89


def dataset_stats_standin():
    """{label: {"t3","l","h","w": tensor([mean, logvar])}} with mean 0 / logvar 0 (contperceptual.py:84-104 layout)."""
    return {lab: {k: torch.tensor([0.0, 0.0]) for k in ("t3", "l", "h", "w")} for lab in LABELS}


def _loss_side_inputs(batch_size, height, width, seed, cond_key, cond_channels, weights_key):
    """The entries behind the models' cond_key / loss_weights_key, each from a generator of its own (every other entry keeps its bits):
    cond ~ U[0,1) [B,cond_channels,H,W] (a side channel of the conditional discriminator), weights in {0.25, 0.5, ..., 2} [B,1,H,W] (a
    per-pixel weight on the NLL)."""
    extra = {}
    if cond_key is not None:
        gc = torch.Generator().manual_seed(seed + 1299709)
        extra[cond_key] = torch.rand(batch_size, int(cond_channels), height, width, generator=gc)
    if weights_key is not None:
        gw = torch.Generator().manual_seed(seed + 15485863)
        extra[weights_key] = torch.randint(1, 9, (batch_size, 1, height, width), generator=gw).float() / 4
    return extra


def make_batch(batch_size, height, width=None, seed=23, class_id=0, mask_key=None, cond_key=None, cond_channels=2, weights_key=None):
    """The batch dict PoseAutoencoder.training_step reads; `patch` ~ U[0,1) NCHW like ToTensor output.
    mask_key (the model's image_mask_key): a seeded {0,1} alpha mask [B,1,H,W] under that key, drawn from a generator of its own so that
    the other entries are the ones a batch without it holds.  cond_key / weights_key (the model's cond_key / loss_weights_key): the same
    for a [B,cond_channels,H,W] side channel and a per-pixel weight map [B,1,H,W]."""
    width = width or height
    g = torch.Generator().manual_seed(seed)
    extra = _loss_side_inputs(batch_size, height, width, seed, cond_key, cond_channels, weights_key)
    if mask_key is not None:
        gm = torch.Generator().manual_seed(seed + 104729)
        extra[mask_key] = (torch.rand(batch_size, 1, height, width, generator=gm) < 0.5).float()
    return {
        **extra,
        "patch": torch.rand(batch_size, 3, height, width, generator=g),
        "pose_6d": torch.randn(batch_size, 4, generator=g),
        "yaw": (torch.rand(batch_size, generator=g) * 2 - 1) * math.pi,
        "class_id": torch.full((batch_size,), class_id, dtype=torch.int64),
        "class_name": [LABELS[class_id]] * batch_size,
        "bbox_sizes": torch.randn(batch_size, 3, generator=g),
        "fill_factor": torch.rand(batch_size, generator=g),
        "mask_2d_bbox": torch.ones(batch_size, 1, height, width),
        "pose_6d_perturbed": torch.randn(batch_size, 1, 4, generator=g),
        "yaw_perturbed": (torch.rand(batch_size, generator=g) * 2 - 1) * math.pi,
    }


def make_image_batch(batch_size, height, width=None, seed=23, image_key="image", cond_key=None, cond_channels=2):
    """The batch dict AutoencoderKL.training_step reads: `image` ~ U[-1,1) as [N, H, W, 3] (get_input permutes it to NCHW).
    cond_key: as in make_batch (NCHW; the plain model has no loss_weights_key)."""
    width = width or height
    g = torch.Generator().manual_seed(seed)
    return {**_loss_side_inputs(batch_size, height, width, seed, cond_key, cond_channels, None),
            image_key: torch.rand(batch_size, height, width, 3, generator=g) * 2 - 1}


def make_noise(batch_size, latent_hw, z_channels=16, dropout_p=0.7, seed=99):
    """The four host RNG draws of one forward pass, made explicit so HIP path and oracle can share them."""
    g = torch.Generator().manual_seed(seed)
    shape = (batch_size, z_channels, latent_hw, latent_hw)
    if dropout_p >= 1.0:
        mask = torch.zeros(shape)
    elif dropout_p <= 0.0:
        mask = torch.ones(shape)
    else:
        mask = (torch.rand(shape, generator=g) >= dropout_p).float() / (1.0 - dropout_p)
    return {"posterior_eps": torch.randn(shape, generator=g), "dropout_mask": mask,
            "z_noise": torch.randn(shape, generator=g), "bbox_eps": torch.randn(batch_size, 8, generator=g)}


def model_config(yaml_path, latent_hw=16, ch=None, phase="vae", perceptual_weight=0.0, disc_factor=0.0, disc_start=0, cond_key=None,
                 cond_channels=2, loss_weights_key=None):
    """The model section of the reference yaml with the benchmark overrides of SURVEY.md 8(d):
    phase "vae": encoder_pretrain_steps = 0 and pose_conditioned_generation_steps = 0 on both the model and the loss, so
    the decoder runs, L1 is on and dropout sits at its final value from step 0 (the regime the metric is quoted on);
    phase "asis": thresholds untouched.  perceptual_weight / disc_factor 0 = "rec+KL only".  latent_hw adapts the pose
    MLPs when the input is not 256x256 (latent = H/16); ch narrows the network for tests.  cond_key (with cond_channels) / loss_weights_key:
    the model's params of those names; a cond_key also makes the discriminator conditional (disc_conditional, disc_in_channels + cond_channels)."""
    cfg = Config.load(yaml_path)
    model = copy.deepcopy(cfg.model)
    p = model.params
    lp = p.lossconfig.params
    lp["dataset_stats"] = dataset_stats_standin()
    lp["perceptual_weight"] = perceptual_weight
    lp["disc_factor"] = disc_factor
    lp["disc_start"] = disc_start
    if phase == "vae":
        lp["encoder_pretrain_steps"] = 0
        lp["pose_conditioned_generation_steps"] = 0
        p["pose_conditioned_generation_steps"] = 0
        p["dropout_warmup_steps"] = 0
    if latent_hw != 16:
        for key in ("pose_decoder_config", "pose_encoder_config"):
            p[key].params["n"] = latent_hw
            p[key].params["m"] = latent_hw
        p["feat_dims"] = [16, latent_hw, latent_hw]
    if ch is not None:
        p.ddconfig["ch"] = ch
    if cond_key is not None:
        p["cond_key"] = cond_key
        lp["disc_conditional"] = True
        lp["disc_in_channels"] = int(lp.get("disc_in_channels", 3)) + int(cond_channels)
    if loss_weights_key is not None:
        p["loss_weights_key"] = loss_weights_key
    return model, cfg


def build_model(yaml_path, batch_size_for_lr=None, **kw):
    """instantiate_from_config on the (overridden) yaml + the reference's learning-rate rule."""
    model_cfg, cfg = model_config(yaml_path, **kw)
    model = instantiate_from_config(model_cfg)
    bs = batch_size_for_lr if batch_size_for_lr is not None else cfg.data.params.batch_size
    model.learning_rate = 1 * 1 * bs * cfg.model.base_learning_rate  # accumulate * ngpu * bs * base_lr (train.py:383)
    return model


def fill_state_procedural(module, seed=23):
    """Deterministic weights that depend only on (seed, state_dict key, shape) -- not on torch's init routines or on the
    construction order of a module tree -- so committed fixtures (tests/golden/make_op_fixtures.py) can name their weights
    without storing them.  Matrices ~ N(0, 1/fan_in), norm scales ~ 1 + 0.1 N, biases ~ 0.05 N; integer buffers untouched."""
    import zlib
    sd = module.state_dict()
    with torch.no_grad():
        for key in sorted(sd.keys()):
            t = sd[key]
            if not t.is_floating_point() or key.startswith("loss.perceptual_loss.scaling_layer"):
                continue
            g = torch.Generator().manual_seed((zlib.crc32(key.encode()) + 7919 * seed) % (2 ** 31))
            r = torch.randn(t.shape, generator=g)
            if key.endswith("running_var"):
                v = 1.0 + 0.1 * r.abs()
            elif t.dim() >= 2:
                v = r / float(max(1, t[0].numel())) ** 0.5
            elif "norm" in key and key.endswith("weight"):
                v = 1.0 + 0.1 * r
            elif t.dim() == 0:
                v = torch.zeros(())
            else:
                v = 0.05 * r
            t.copy_(v.to(t.dtype))
    return module
