"""Thin runner for the hot path with the reference launcher's config surface (train.py:18-55,134-148,356-392,433):
`-b/--base` yaml files merged left to right, trailing `key=value` dotlist overrides, `-s/--seed` (default 23), the
learning-rate rule, then the PL-1.9-semantics loop of trainer.py on synthetic batches (the nuScenes pipeline, loggers,
checkpoint callbacks and the rest of train.py are out of scope).

    python -m odvae_amd.run -b tests/golden/autoencoder_kl_16x16x16.yaml --steps 4 --height 256 \
        model.params.lossconfig.params.disc_start=0 data.params.batch_size=8
"""
import argparse
import os
import random
import sys

import numpy as np
import torch

from . import synthetic
from .config import Config, configure_learning_rate, instantiate_from_config
from .trainer import Trainer


def seed_everything(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    os.environ["PL_GLOBAL_SEED"] = str(seed)


def parse(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-b", "--base", nargs="*", default=[], metavar="base_config.yaml")
    ap.add_argument("-s", "--seed", type=int, default=23)
    ap.add_argument("--scale_lr", type=lambda v: str(v).lower() in ("1", "true", "yes"), default=True)
    ap.add_argument("--steps", type=int, default=2, help="batches to run")
    ap.add_argument("--height", type=int, default=256, help="synthetic crop size (the yaml's patch_height)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("-l", "--logdir", default=None, help="if given, the yaml's lightning.callbacks run and ImageLogger writes below it")
    ap.add_argument("--checkpoint", default=None, help="with model.params.ema_decay or model.params.image_mask_key: write a Lightning-layout checkpoint "
                    "(weights, model_ema.* if any, optimizer states) here after the run; default <logdir>/checkpoints/last.ckpt when --logdir is given")
    ap.add_argument("--float32_matmul_precision", default=None, choices=("highest", "high", "medium", "torch"),
                    help="what the reference's launcher sets with torch.set_float32_matmul_precision (train.py:521: medium); default: "
                    "leave ODVAE_FLOAT32_MATMUL_PRECISION (highest) alone")
    return ap.parse_known_args(argv)


def trainer_kwargs(trainer_cfg):
    """The `lightning.trainer` keys of the yaml this Trainer honours: gradient_clip_val, precision, detect_anomaly (yaml:138; absent
    = None, which leaves the choice to ODVAE_DETECT_ANOMALY), accumulate_grad_batches (yaml:134; passed on only when it is not 1) and sync_batchnorm (passed on only when the yaml sets it); gradient_clip_algorithm ('norm' / 'value') and track_grad_norm (-1, a
    number > 0 or 'inf'), the two PL-1.9 Trainer arguments of the gradient path, likewise only when the yaml or a dotlist override
    (lightning.trainer.track_grad_norm=2) sets them."""
    kw = {"gradient_clip_val": trainer_cfg.get("gradient_clip_val", None), "precision": trainer_cfg.get("precision", None),
          "detect_anomaly": trainer_cfg.get("detect_anomaly", None)}
    accumulate = trainer_cfg.get("accumulate_grad_batches", 1)
    if accumulate != 1:      # (yaml:134; configure_learning_rate already multiplies the learning rate by it)
        kw["accumulate_grad_batches"] = accumulate
    if "sync_batchnorm" in trainer_cfg:      # (PL: SyncBatchNorm over the discriminator's BatchNorm layers; Trainer refuses a non-bool)
        kw["sync_batchnorm"] = trainer_cfg["sync_batchnorm"]
    for key in ("gradient_clip_algorithm", "track_grad_norm"):      # (Trainer validates both)
        if key in trainer_cfg:
            kw[key] = trainer_cfg[key]
    return kw


def main(argv=None):
    opt, unknown = parse(sys.argv[1:] if argv is None else argv)
    seed_everything(opt.seed)
    config = Config.merge(*[Config.load(p) for p in opt.base], Config.from_dotlist(unknown))
    lightning = config.pop("lightning", Config.create())
    trainer_cfg = lightning.get("trainer", Config.create())
    params = config.model.params
    if "pose_decoder_config" in params:      # the pose model's keys; a plain AutoencoderKL / Autoencoder yaml has none of them
        lp = params.lossconfig.params
        if "dataset_stats" not in lp and not os.path.exists(lp.get("dataset_stats_path", "dataset_stats/combined/all.pkl")):
            lp["dataset_stats"] = synthetic.dataset_stats_standin()   # the reference does not ship its stats pickle
        latent = opt.height // 2 ** (len(params.ddconfig.ch_mult) - 1)
        if latent != params.pose_decoder_config.params.n:
            for key in ("pose_decoder_config", "pose_encoder_config"):
                params[key].params["n"] = latent
                params[key].params["m"] = latent
            params["feat_dims"] = [params.embed_dim, latent, latent]
    model = instantiate_from_config(config.model)
    configure_learning_rate(config, model, trainer_cfg, scale_lr=opt.scale_lr, ngpu=1)
    model = model.to(opt.device).train()
    callbacks, logger = [], None
    if opt.logdir:   # the callbacks section of the yaml (train.py:452-463 instantiates them the same way)
        class _Logger:
            save_dir = opt.logdir
        logger = _Logger()
        for name, cb_cfg in lightning.get("callbacks", Config.create()).items():
            callbacks.append(instantiate_from_config(cb_cfg))
    trainer = Trainer(model, callbacks=callbacks, logger=logger, float32_matmul_precision=opt.float32_matmul_precision,
                      **trainer_kwargs(trainer_cfg))
    bs = config.data.params.batch_size

    # model.params.cond_key: the synthetic batch carries a side channel of disc_in_channels - out_ch channels under that key; the pose
    # model's loss_weights_key: a per-pixel weight map
    side = dict(cond_key=getattr(model, "cond_key", None),
                cond_channels=model.loss.discriminator.main[0].in_channels - model.decoder.conv_out.out_channels)

    def make(step):
        if hasattr(model, "image_key"):      # AutoencoderKL / Autoencoder: images alone
            return synthetic.make_image_batch(bs, opt.height, seed=opt.seed + step, image_key=model.image_key, **side)
        return synthetic.make_batch(bs, opt.height, seed=opt.seed + step, mask_key=getattr(model, "image_mask_key", None),
                                    weights_key=getattr(model, "loss_weights_key", None), **side)
    for step in range(opt.steps):
        batch = make(step)
        losses = trainer.training_batch(batch, step, last_in_epoch=step == opt.steps - 1)   # (closes an accumulation window)
        print("batch %d  global_step %d  aeloss %.4f  discloss %.4f  lr %.2e" %
              (step, model.global_step, losses[0].item(), losses[1].item(), model.learning_rate), flush=True)
    if hasattr(model, "quantize"):     # VQModel: one validation batch (and the same under the averaged weights with model.params.use_ema)
        metrics = trainer.validate([make(opt.steps)])
        line = "validation  val/rec_loss %.4f  val/aeloss %.4f  val/quant_loss %.4f" % (
            metrics["val/rec_loss"].item(), metrics["val/aeloss"].item(), metrics["val/quant_loss"].item())
        if getattr(model, "use_ema", False):
            line += "  val_ema/rec_loss %.4f" % metrics["val_ema/rec_loss"].item()
        print(line, flush=True)
        ckpt = opt.checkpoint or (os.path.join(opt.logdir, "checkpoints", "last.ckpt") if opt.logdir else None)
        if ckpt:
            print("checkpoint  %s" % trainer.save_checkpoint(ckpt), flush=True)
    elif getattr(model, "use_ema", False):     # model.params.ema_decay: one validation batch under the trained and the averaged weights
        metrics = trainer.validate([make(opt.steps)])
        print("validation  val/rec_loss %.4f  val_ema/rec_loss %.4f  ema updates %d" %
              (metrics["val/rec_loss"].item(), metrics["val_ema/rec_loss"].item(), int(model.model_ema.num_updates)), flush=True)
        ckpt = opt.checkpoint or (os.path.join(opt.logdir, "checkpoints", "last.ckpt") if opt.logdir else None)
        if ckpt:
            print("checkpoint  %s (%d model_ema.* keys)" % (trainer.save_checkpoint(ckpt), len(model.model_ema.state_dict())), flush=True)
    elif getattr(model, "image_mask_key", None) is not None:     # model.params.image_mask_key: one validation batch with the alpha mask
        metrics = trainer.validate([make(opt.steps)])
        print("validation  val/rec_loss %.4f  val/mask_loss %.4f" % (metrics["val/rec_loss"].item(), metrics["val/mask_loss"].item()), flush=True)
        ckpt = opt.checkpoint or (os.path.join(opt.logdir, "checkpoints", "last.ckpt") if opt.logdir else None)
        if ckpt:
            print("checkpoint  %s" % trainer.save_checkpoint(ckpt), flush=True)
    return model


if __name__ == "__main__":
    main()
