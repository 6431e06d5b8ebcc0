"""AutoencoderKL / Autoencoder / PoseAutoencoder on the HIP kernels, with the reference's LightningModule surface.

Mirrors src/models/autoencoder.py (PoseAutoencoder :34-443, Autoencoder :29-32) and the [UPSTREAM]
ldm/models/autoencoder.py AutoencoderKL it derives from (encode / decode / get_input / get_last_layer /
init_from_ckpt / configure_optimizers).  Constructor signature, attribute names, state_dict keys, batch-dict keys,
global_step thresholds and logged names are the reference's; the arithmetic is in generative-detection_amd/ops/.
"""
import contextlib
import logging

import torch
import torch.nn as nn

from . import lib as _lib
from . import ops
from .config import instantiate_from_config
from .distributions import DiagonalGaussianDistribution
from .ema import LitEma
from .latent_noise import CallCounter, make_draw, with_stream
from .lightning import LightningModule
from .modules import Conv1x1, Decoder, Encoder
from .optim import make_adam
from .quantize import VectorQuantizer

POSE_6D_DIM = 4
FILL_FACTOR_DIM = 1
LHW_DIM = 3
BBOX_DIM = POSE_6D_DIM + LHW_DIM + FILL_FACTOR_DIM


class FeatEncoder(Encoder):
    """src/modules/autoencodermodules/feat_encoder.py:4-6"""


class FeatDecoder(Decoder):
    """src/modules/autoencodermodules/feat_decoder.py:4-6"""


class AutoencoderKL(LightningModule):
    """[UPSTREAM] ldm.models.autoencoder.AutoencoderKL (the plain KL autoencoder BASELINE.json names)."""

    def __init__(self, ddconfig, lossconfig, embed_dim, ckpt_path=None, ignore_keys=[], image_key="image",
                 colorize_nlabels=None, monitor=None, ema_decay=None, learn_logvar=False, device_noise=None, cond_key=None):
        """cond_key: an extension (upstream's steps never pass the loss's `cond`).  When set, batch[key] (NCHW) goes to the loss as cond=
        (the conditional discriminator's side channel: lossconfig disc_conditional, disc_in_channels) in the training and validation
        steps.  (PoseAutoencoder has loss_weights_key beside it: a weight map is PoseLoss's, the plain loss takes none.)
        device_noise: an extension (neither upstream nor the reference has it).  None = the noise is drawn with the host RNG and
        uploaded, as the reference does; an integer is the seed of the device-side draws (latent_noise.py): no host RNG, no upload."""
        super().__init__()
        self._init_image_model(image_key, cond_key, learn_logvar, device_noise)
        self.encoder = Encoder(**ddconfig)
        self.decoder = Decoder(**ddconfig)
        self.loss = instantiate_from_config(lossconfig)
        assert ddconfig["double_z"]
        self.quant_conv = Conv1x1(2 * ddconfig["z_channels"], 2 * embed_dim)
        self.post_quant_conv = Conv1x1(embed_dim, ddconfig["z_channels"])
        self.embed_dim = embed_dim
        self._init_colorize_and_monitor(colorize_nlabels, monitor)
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys=ignore_keys)
        self._init_ema(ema_decay)

    def _init_image_model(self, image_key, cond_key=None, learn_logvar=False, device_noise=None):
        """The state every method of this class reads, whatever the latent stage: AutoencoderKL and VQModel both start here, so a method
        that comes to need a new attribute gets it in both."""
        self.learn_logvar = learn_logvar
        self.image_key = image_key
        self.cond_key = cond_key
        # test hook: {"posterior_eps", "samples_eps"} tensors replace the host RNG draws of forward and log_images
        self.injected_noise = None
        self._init_device_noise(device_noise)
        self.use_ema = False
        self._in_ema_scope = False

    def _init_colorize_and_monitor(self, colorize_nlabels, monitor):
        if colorize_nlabels is not None:
            assert type(colorize_nlabels) == int
            self.register_buffer("colorize", torch.randn(3, colorize_nlabels, 1, 1))
        if monitor is not None:
            self.monitor = monitor

    def _noise(self, key):
        noise = getattr(self, "injected_noise", None)
        return None if noise is None else noise.get(key)

    # ---- device-side noise (latent_noise.py: the draw; csrc/latent_noise.hip: the kernels) ------------------------------------------
    def _init_device_noise(self, device_noise):
        self.device_noise = None if device_noise is None else int(device_noise)
        self.noise_rank = 0      # the key's rank: trainer.Trainer sets it where it hands out the process group
        self._noise_calls = CallCounter()
        self._last_draw = None

    def _next_draw(self):
        """The draw descriptor of one forward (None with device_noise off): a pure function of seed, rank, global_step, training and the
        number of forwards since the last two changed -- nothing of it is in the state_dict, and a resumed run draws what the
        uninterrupted one drew."""
        if self.device_noise is None:
            return None
        call = self._noise_calls.next(self.global_step, self.training)
        self._last_draw = make_draw(self.device_noise, self.noise_rank, self.global_step, self.training, call)
        return self._last_draw

    def _drawn(self, key, shape, draw, stream, kind=0, p=0.0):
        """injected_noise[key] where a test set it, else the stream's elements from the device fill ([N, C, H, W]: in NHWC order)"""
        t = self._noise(key)
        if t is not None:
            return _lib.upload(t, self.device)
        return ops.noise_fill(shape, with_stream(draw, stream), self.device, kind=kind, p=p, nhwc=len(shape) == 4)

    # ---- exponential moving average of the weights ([UPSTREAM] the stable-diffusion revision of this class; ema.LitEma) -------------
    def _init_ema(self, ema_decay, use_ema=None):
        """Last in __init__ (after init_from_ckpt): the shadows start as clones of the weights the model starts with.  use_ema=True with
        ema_decay None (VQModel): LitEma's own default decay, as upstream."""
        self.use_ema = ema_decay is not None if use_ema is None else bool(use_ema)
        self._in_ema_scope = False
        if self.use_ema:
            assert ema_decay is None or 0. < ema_decay < 1.
            self.model_ema = LitEma(self) if ema_decay is None else LitEma(self, decay=ema_decay)
            print(f"Keeping EMAs of {len(list(self.model_ema.buffers()))}.")

    @contextlib.contextmanager
    def ema_scope(self, context=None):
        """Inside, the parameters hold the averaged weights; on the way out -- by an exception too -- they hold exactly what they held
        before.  One exchange kernel per parameter arena each way (upstream: store / copy_to / restore, three copies of every parameter).
        The exchange writes parameters behind torch's version counters, so the weight packs are marked stale both times; a graph built
        outside the scope cannot be back-propagated inside it (and the reverse)."""
        if self.use_ema:
            if self._in_ema_scope:
                raise RuntimeError("ema_scope: already inside one (the parameters hold the averaged weights; a second exchange would bring the trained ones back)")
            self.model_ema.swap(self)
            ops.PACK_CACHE.bump()
            self._in_ema_scope = True
            if context is not None:
                print(f"{context}: Switched to EMA weights")
        try:
            yield None
        finally:
            if self.use_ema:
                self.model_ema.swap(self)
                ops.PACK_CACHE.bump()
                self._in_ema_scope = False
                if context is not None:
                    print(f"{context}: Restored training weights")

    def on_train_batch_end(self, *args, **kwargs):
        """One update of the average per training BATCH (PL calls this hook per batch, not per optimizer step)"""
        if self.use_ema:
            self.model_ema(self)

    def set_precision(self, precision, perceptual_precision=None, discriminator_precision=None):
        """The trainer's `precision` (configs/autoencoder/pose/autoencoder_kl_16x16x16.yaml:139; PL-1.9 accepts 32, "32", 16, "bf16"):
        32 = f32 everywhere; "bf16" = mixed precision -- bf16 activations inside Encoder / Decoder on the bf16 MFMA kernels, f32
        master weights, gradients, statistics, latent, reconstruction and losses.  fp16 is not offered (no loss scaler here).
        perceptual_precision: 32 or "bf16" for the LPIPS-style net of the loss (LPIPSStyle.set_precision); None leaves it as it is -- f32
        unless ODVAE_LPIPS_BF16=1, with which `precision` takes the perceptual net along.
        discriminator_precision: the same for the loss's PatchGAN discriminator (NLayerDiscriminator.set_precision) and ODVAE_DISC_BF16=1."""
        p = str(precision).lower()
        if p in ("32", "32-true", "fp32"):
            dt = torch.float32
        elif p in ("bf16", "bf16-mixed"):
            dt = torch.bfloat16
        else:
            raise ValueError("precision %r: this build computes in 32 (f32) or bf16 (mixed precision)" % (precision,))
        self.encoder.compute_dtype = dt
        self.decoder.compute_dtype = dt
        lpips = getattr(getattr(self, "loss", None), "perceptual_loss", None)
        if perceptual_precision is not None:
            if not hasattr(lpips, "set_precision"):
                raise ValueError("perceptual_precision=%r: the loss has no perceptual net" % (perceptual_precision,))
            lpips.set_precision(perceptual_precision)
        elif ops.LPIPS_BF16 and hasattr(lpips, "set_precision"):
            lpips.set_precision(precision)
        disc = getattr(getattr(self, "loss", None), "discriminator", None)
        if discriminator_precision is not None:
            if not hasattr(disc, "set_precision"):
                raise ValueError("discriminator_precision=%r: the loss has no discriminator" % (discriminator_precision,))
            disc.set_precision(discriminator_precision)
        elif ops.DISC_BF16 and hasattr(disc, "set_precision"):
            disc.set_precision(precision)
        return self

    def init_from_ckpt(self, path, ignore_keys=list()):
        sd = torch.load(path, map_location="cpu")["state_dict"]
        for k in list(sd.keys()):
            if any(k.startswith(ik) for ik in ignore_keys):
                print("Deleting key {} from state_dict.".format(k))
                del sd[k]
        self.load_state_dict(sd, strict=False)
        print(f"Restored from {path}")

    def encode(self, x):
        moments = self.quant_conv(self.encoder(x))
        return DiagonalGaussianDistribution(moments)

    def decode(self, z):
        return self.decoder(self.post_quant_conv(z))

    def forward(self, input, sample_posterior=True):
        posterior = self.encode(input)
        draw = self._next_draw()
        z = posterior.sample(self._noise("posterior_eps"), draw=draw) if sample_posterior else posterior.mode()
        return self.decode(z), posterior

    def _samples_eps(self, shape):
        """The N(0, 1) latent that log_images decodes as `samples`: injected, stream 4 of the last forward's draw, or a host draw"""
        eps = self._noise("samples_eps")
        if eps is None and self.device_noise is not None:
            return ops.noise_fill(shape, with_stream(self._last_draw, "samples_eps"), self.device)
        if eps is None:
            eps = torch.randn(shape)      # drawn on the host, as DiagonalGaussianDistribution.sample does
        return _lib.upload(eps.float(), self.device)

    def _loss_extras(self, batch):
        """cond= and weights= of the loss call: batch[cond_key] and (PoseAutoencoder alone has that key) batch[loss_weights_key], both NCHW,
        where the keys are set, else nothing"""
        extras = {}
        if getattr(self, "cond_key", None) is not None:
            extras["cond"] = batch[self.cond_key]
        if getattr(self, "loss_weights_key", None) is not None:
            extras["weights"] = batch[self.loss_weights_key]
        return extras

    def get_input(self, batch, k):
        """[N, H, W, C] (or [N, H, W]) of the batch -> f32 NCHW on the model's device"""
        x = batch[k]
        if len(x.shape) == 3:
            x = x[..., None]
        return _lib.upload(x.permute(0, 3, 1, 2).to(memory_format=torch.contiguous_format).float(), self.device)

    def training_step(self, batch, batch_idx, optimizer_idx):
        inputs = self.get_input(batch, self.image_key)
        reconstructions, posterior = self(inputs)
        if optimizer_idx == 0:
            aeloss, log_dict_ae = self.loss(inputs, reconstructions, posterior, optimizer_idx, self.global_step,
                                            last_layer=self.get_last_layer(), split="train", **self._loss_extras(batch))
            self.log("aeloss", aeloss, prog_bar=True, logger=True, on_step=True, on_epoch=True)
            self.log_dict(log_dict_ae, prog_bar=False, logger=True, on_step=True, on_epoch=False)
            return aeloss
        discloss, log_dict_disc = self.loss(inputs, reconstructions, posterior, optimizer_idx, self.global_step,
                                            last_layer=self.get_last_layer(), split="train", **self._loss_extras(batch))
        self.log("discloss", discloss, prog_bar=True, logger=True, on_step=True, on_epoch=True)
        self.log_dict(log_dict_disc, prog_bar=False, logger=True, on_step=True, on_epoch=False)
        return discloss

    def validation_step(self, batch, batch_idx):
        log_dict = self._validation_step(batch, batch_idx)
        if self.use_ema:      # the same batch again under the averaged weights: val_ema/rec_loss and the rest
            with self.ema_scope():
                self._validation_step(batch, batch_idx, postfix="_ema")
        return log_dict

    def _validation_step(self, batch, batch_idx, postfix=""):
        inputs = self.get_input(batch, self.image_key)
        reconstructions, posterior = self(inputs)
        _, log_dict_ae = self.loss(inputs, reconstructions, posterior, 0, self.global_step,
                                   last_layer=self.get_last_layer(), split="val" + postfix, **self._loss_extras(batch))
        _, log_dict_disc = self.loss(inputs, reconstructions, posterior, 1, self.global_step,
                                     last_layer=self.get_last_layer(), split="val" + postfix, **self._loss_extras(batch))
        self.log(f"val{postfix}/rec_loss", log_dict_ae[f"val{postfix}/rec_loss"])
        self.log_dict(log_dict_ae)
        self.log_dict(log_dict_disc)
        return self.log_dict

    @torch.no_grad()
    def log_images(self, batch, only_inputs=False, log_ema=False, **kwargs):
        log = dict()
        x = self.get_input(batch, self.image_key)
        if not only_inputs:
            x_in = x
            xrec, posterior = self(x)
            if x.shape[1] > 3:      # more than three channels (label maps): both sides go through the fixed `colorize` projection
                assert xrec.shape[1] == x.shape[1], "reconstruction has %d channels, input %d" % (xrec.shape[1], x.shape[1])
                x, xrec = self.to_rgb(x), self.to_rgb(xrec)
            log["samples"] = self.decode(self._samples_eps(tuple(posterior.mean.shape)))
            log["reconstructions"] = xrec
            if log_ema or self.use_ema:
                with self.ema_scope():
                    xrec_ema, posterior_ema = self(x_in)
                    if x_in.shape[1] > 3:
                        assert xrec_ema.shape[1] == x_in.shape[1]
                        xrec_ema = self.to_rgb(xrec_ema)
                    log["samples_ema"] = self.decode(self._samples_eps(tuple(posterior_ema.mean.shape)))      # the shape of the EMA pass's posterior
                    log["reconstructions_ema"] = xrec_ema
        log["inputs"] = x
        return log

    def configure_optimizers(self):
        lr = self.learning_rate
        ae_params = (list(self.encoder.parameters()) + list(self.decoder.parameters())
                     + list(self.quant_conv.parameters()) + list(self.post_quant_conv.parameters()))
        if self.learn_logvar:
            print(f"{self.__class__.__name__}: Learning logvar")
            ae_params.append(self.loss.logvar)
        opt_ae = make_adam(ae_params, lr=lr, betas=(0.5, 0.9))
        opt_disc = make_adam(self.loss.discriminator.parameters(), lr=lr, betas=(0.5, 0.9))
        return [opt_ae, opt_disc], []

    def get_last_layer(self):
        return self.decoder.conv_out.weight

    def to_rgb(self, x):
        """Random fixed 1x1 projection of a C-channel map to three channels, rescaled to [-1, 1] over the batch
        (src/models/autoencoder.py:438-443; [UPSTREAM] AutoencoderKL.to_rgb, used when `colorize_nlabels` is given).
        `colorize` is a buffer drawn once, as in the reference."""
        if not hasattr(self, "colorize"):
            self.register_buffer("colorize", torch.randn(3, x.shape[1], 1, 1).to(x))
        return ops.rescale_minmax(ops.conv1x1(x, self.colorize))


class Autoencoder(AutoencoderKL):
    """src/models/autoencoder.py:29-32"""


class VQModel(AutoencoderKL):
    """[UPSTREAM] ldm.models.autoencoder.VQModel: the family's second member (vq-f4, vq-f8, vq-f16; taming's VQGAN).  Encoder without the
    doubled latent, quant_conv to embed_dim, VectorQuantizer, post_quant_conv, Decoder; loss VQLPIPSWithDiscriminator.  What it shares
    with AutoencoderKL (get_input, get_last_layer, init_from_ckpt, to_rgb, ema_scope, on_train_batch_end, set_precision) is inherited;
    under precision "bf16" the quantiser still runs in f32 (the encoder hands quant_conv an f32 latent)."""

    def __init__(self, ddconfig, lossconfig, n_embed, embed_dim, ckpt_path=None, ignore_keys=[], image_key="image",
                 colorize_nlabels=None, monitor=None, batch_resize_range=None, scheduler_config=None, lr_g_factor=1.0,
                 remap=None, sane_index_shape=False, use_ema=False):
        LightningModule.__init__(self)      # (AutoencoderKL.__init__ builds the doubled quant_conv and the KL loss)
        if batch_resize_range is not None:
            raise NotImplementedError("VQModel(batch_resize_range=%r): random batch resizing is not implemented" % (batch_resize_range,))
        if scheduler_config is not None:
            raise NotImplementedError("VQModel(scheduler_config=...): learning-rate schedulers are not implemented")
        self._init_image_model(image_key)
        self.embed_dim = embed_dim
        self.n_embed = n_embed
        self.encoder = Encoder(**ddconfig)
        self.decoder = Decoder(**ddconfig)
        self.loss = instantiate_from_config(lossconfig)
        self.quantize = VectorQuantizer(n_embed, embed_dim, beta=0.25, remap=remap, sane_index_shape=sane_index_shape)
        self.quant_conv = Conv1x1(ddconfig["z_channels"], embed_dim)
        self.post_quant_conv = Conv1x1(embed_dim, ddconfig["z_channels"])
        self._init_colorize_and_monitor(colorize_nlabels, monitor)
        self.batch_resize_range = batch_resize_range
        self.scheduler_config = scheduler_config
        self.lr_g_factor = lr_g_factor
        self._init_ema(None, use_ema=use_ema)      # upstream's default decay
        if ckpt_path is not None:      # (upstream loads after the EMA is built: a checkpoint's model_ema.* keys land in it)
            self.init_from_ckpt(ckpt_path, ignore_keys=ignore_keys)

    def encode(self, x):
        h = self.quant_conv(self.encoder(x))
        quant, emb_loss, info = self.quantize(h)
        return quant, emb_loss, info

    def encode_to_prequant(self, x):
        return self.quant_conv(self.encoder(x))

    def decode(self, quant):
        return self.decoder(self.post_quant_conv(quant))

    def decode_code(self, code_b):
        """code_b int64 [N, H, W] -> images"""
        n, h, w = code_b.shape
        return self.decode(self.quantize.get_codebook_entry(code_b.reshape(-1), (n, h, w, self.embed_dim)))

    def forward(self, input, return_pred_indices=False):
        quant, diff, (_, _, ind) = self.encode(input)
        dec = self.decode(quant)
        if return_pred_indices:
            return dec, diff, ind
        return dec, diff

    def training_step(self, batch, batch_idx, optimizer_idx):
        x = self.get_input(batch, self.image_key)
        xrec, qloss, ind = self(x, return_pred_indices=True)
        if optimizer_idx == 0:
            aeloss, log_dict_ae = self.loss(qloss, x, xrec, optimizer_idx, self.global_step, last_layer=self.get_last_layer(),
                                            split="train", predicted_indices=ind)
            self.log_dict(log_dict_ae, prog_bar=False, logger=True, on_step=True, on_epoch=True)
            return aeloss
        if optimizer_idx == 1:
            discloss, log_dict_disc = self.loss(qloss, x, xrec, optimizer_idx, self.global_step, last_layer=self.get_last_layer(),
                                                split="train")
            self.log_dict(log_dict_disc, prog_bar=False, logger=True, on_step=True, on_epoch=True)
            return discloss

    def validation_step(self, batch, batch_idx):
        log_dict = self._validation_step(batch, batch_idx)
        if self.use_ema:
            with self.ema_scope():
                self._validation_step(batch, batch_idx, suffix="_ema")
        return log_dict

    def _validation_step(self, batch, batch_idx, suffix=""):
        x = self.get_input(batch, self.image_key)
        xrec, qloss, ind = self(x, return_pred_indices=True)
        aeloss, log_dict_ae = self.loss(qloss, x, xrec, 0, self.global_step, last_layer=self.get_last_layer(), split="val" + suffix,
                                        predicted_indices=ind)
        discloss, log_dict_disc = self.loss(qloss, x, xrec, 1, self.global_step, last_layer=self.get_last_layer(), split="val" + suffix,
                                            predicted_indices=ind)
        rec_loss = log_dict_ae[f"val{suffix}/rec_loss"]
        self.log(f"val{suffix}/rec_loss", rec_loss, prog_bar=True, logger=True, on_step=False, on_epoch=True, sync_dist=True)
        self.log(f"val{suffix}/aeloss", aeloss, prog_bar=True, logger=True, on_step=False, on_epoch=True, sync_dist=True)
        del log_dict_ae[f"val{suffix}/rec_loss"]
        self.log_dict(log_dict_ae)
        self.log_dict(log_dict_disc)
        return self.log_dict

    def configure_optimizers(self):
        lr_d = self.learning_rate
        lr_g = self.lr_g_factor * self.learning_rate
        print("lr_d", lr_d)
        print("lr_g", lr_g)
        opt_ae = make_adam(list(self.encoder.parameters()) + list(self.decoder.parameters()) + list(self.quantize.parameters())
                           + list(self.quant_conv.parameters()) + list(self.post_quant_conv.parameters()), lr=lr_g, betas=(0.5, 0.9))
        opt_disc = make_adam(self.loss.discriminator.parameters(), lr=lr_d, betas=(0.5, 0.9))
        return [opt_ae, opt_disc], []

    @torch.no_grad()
    def log_images(self, batch, only_inputs=False, plot_ema=False, **kwargs):
        log = dict()
        x = self.get_input(batch, self.image_key)
        if only_inputs:
            log["inputs"] = x
            return log
        xrec, _ = self(x)
        x_in = x
        if x.shape[1] > 3:      # more than three channels (label maps): both sides go through the fixed `colorize` projection
            assert xrec.shape[1] > 3
            x, xrec = self.to_rgb(x), self.to_rgb(xrec)
        log["inputs"] = x
        log["reconstructions"] = xrec
        if plot_ema:
            with self.ema_scope():
                xrec_ema, _ = self(x_in)
                if x_in.shape[1] > 3:
                    xrec_ema = self.to_rgb(xrec_ema)
                log["reconstructions_ema"] = xrec_ema
        return log


class VQModelInterface(VQModel):
    """[UPSTREAM] ldm VQModelInterface: the face a latent-diffusion model sees -- encode stops before the quantiser, decode quantises."""

    def __init__(self, embed_dim, *args, **kwargs):
        super().__init__(embed_dim=embed_dim, *args, **kwargs)
        self.embed_dim = embed_dim

    def encode(self, x):
        return self.quant_conv(self.encoder(x))

    def decode(self, h, force_not_quantize=False):
        if not force_not_quantize:
            quant, emb_loss, info = self.quantize(h)
        else:
            quant = h
        return self.decoder(self.post_quant_conv(quant))


class PoseAutoencoder(AutoencoderKL):
    def __init__(self, ddconfig, lossconfig, embed_dim, euler_convention, ckpt_path=None, ignore_keys=[],
                 image_mask_key=None, image_rgb_key="patch", pose_key="pose_6d", fill_factor_key="fill_factor",
                 pose_perturbed_key="pose_6d_perturbed", class_key="class_id", bbox_key="bbox_sizes",
                 colorize_nlabels=None, monitor=None, activation="relu", feat_dims=[16, 16, 16],
                 pose_decoder_config=None, pose_encoder_config=None, dropout_prob_init=1.0, dropout_prob_final=0.7,
                 dropout_warmup_steps=5000, pose_conditioned_generation_steps=10000, add_noise_to_z_obj=True,
                 train_on_yaw=True, ema_decay=None, learn_logvar=False, device_noise=None, cond_key=None, loss_weights_key=None):
        """cond_key, loss_weights_key: extensions (the reference's steps never pass the loss's `cond` / `weights`).  When set, batch[key]
        (NCHW) goes to PoseLoss as cond= (the conditional discriminator's side channel: lossconfig disc_conditional, disc_in_channels) or
        weights= (a weight on the NLL: scalar, per sample, per pixel or per element) in the training and validation steps.
        ema_decay, learn_logvar: an extension (the reference's PoseAutoencoder has neither): the two keys of the stable-diffusion
        revision of AutoencoderKL, off by default -- None / False reproduce the reference.
        device_noise: an extension too.  None = posterior_eps, the dropout mask, z_noise and bbox_eps come from the host RNG, as in the
        reference; an integer seeds the device-side draws and the latent stage runs as one launch each way (_forward_device_noise)."""
        LightningModule.__init__(self)  # the reference skips AutoencoderKL.__init__ as well (:66)
        self.learn_logvar = learn_logvar
        self.encoder_pretrain_steps = lossconfig["params"]["encoder_pretrain_steps"]
        self.train_on_yaw = train_on_yaw
        self.dropout_prob_final, self.dropout_prob_init = dropout_prob_final, dropout_prob_init
        self.dropout_prob = dropout_prob_init
        self.dropout_warmup_steps = dropout_warmup_steps
        self.pose_conditioned_generation_steps = pose_conditioned_generation_steps
        self.add_noise_to_z_obj = add_noise_to_z_obj
        self.feature_dims = feat_dims
        self.image_rgb_key, self.image_mask_key = image_rgb_key, image_mask_key
        self.cond_key, self.loss_weights_key = cond_key, loss_weights_key
        self.pose_key, self.pose_perturbed_key = pose_key, pose_perturbed_key
        self.class_key, self.bbox_key, self.fill_factor_key = class_key, bbox_key, fill_factor_key
        self.encoder = FeatEncoder(**ddconfig)
        self.decoder = FeatDecoder(**ddconfig)
        lossconfig["params"]["train_on_yaw"] = self.train_on_yaw
        self.loss = instantiate_from_config(lossconfig)
        assert ddconfig["double_z"]
        zc = ddconfig["z_channels"]
        self.quant_conv_obj = Conv1x1(2 * zc, 2 * embed_dim)
        self.quant_conv_pose = Conv1x1(2 * zc, embed_dim)
        self.post_quant_conv = Conv1x1(embed_dim, zc)
        self.embed_dim = embed_dim
        if colorize_nlabels is not None:
            assert type(colorize_nlabels) == int
            self.register_buffer("colorize", torch.randn(3, colorize_nlabels, 1, 1))
        if monitor is not None:
            self.monitor = monitor
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys=ignore_keys)
        self.num_classes = lossconfig["params"]["num_classes"]
        self.pose_decoder = instantiate_from_config(pose_decoder_config)
        self.pose_encoder = instantiate_from_config(pose_encoder_config)
        self.z_channels = zc
        self.euler_convention = euler_convention
        self.feat_dims = feat_dims
        # test hook: {"posterior_eps", "dropout_mask", "z_noise", "bbox_eps"} tensors replace the host RNG draws
        self.injected_noise = None
        self._init_device_noise(device_noise)
        self._init_ema(ema_decay)

    # ---- pose head (:126-174) ---------------------------------------------------------------------------------
    def _decode_pose_to_distribution(self, z, sample_posterior=True):
        c_pred = z[..., -self.num_classes:]
        bbox_moments = z[..., :2 * BBOX_DIM].to(self.device)
        return DiagonalGaussianDistribution(bbox_moments), c_pred

    def _decode_pose(self, x, sample_posterior=True, draw=None):
        flat = x.reshape(x.size(0), -1)  # logical NCHW order, as x.view(B,-1) in the reference
        z = self.pose_decoder(flat)
        bbox_posterior, c_pred = self._decode_pose_to_distribution(z)
        if sample_posterior:
            bbox_pred = bbox_posterior.sample(self._noise("bbox_eps"), draw=None if draw is None else with_stream(draw, "bbox_eps"))
        else:
            bbox_pred = bbox_posterior.mode()
        return torch.cat([bbox_pred, c_pred], dim=-1), bbox_posterior

    def _encode_pose(self, x):
        flat = self.pose_encoder(x)
        return flat.view(flat.size(0), self.feature_dims[0], self.feature_dims[1], self.feature_dims[2])

    def _noise(self, key):
        return None if self.injected_noise is None else self.injected_noise.get(key)

    # ---- encode / forward (:176-257) -------------------------------------------------------------------------
    def encode(self, x):
        x = x.to(self.device)
        h = self.encoder(x)
        moments_obj = self.quant_conv_obj(h)
        pose_feat = self.quant_conv_pose(h)
        return DiagonalGaussianDistribution(moments_obj), pose_feat

    def _get_dropout_prob(self):
        step, pre, gen = self.global_step, self.encoder_pretrain_steps, self.pose_conditioned_generation_steps
        if step < pre + gen:
            return self.dropout_prob_init
        if step < self.dropout_warmup_steps + pre + gen:
            # QUIRK (:200): the ramp is measured from encoder_pretrain_steps, not from pre+gen
            return self.dropout_prob_init - (self.dropout_prob_init - self.dropout_prob_final) * (step - pre) / self.dropout_warmup_steps
        return self.dropout_prob_final

    def _dropout(self, z, p):
        """nn.Dropout(p) keeps with prob 1-p and scales by 1/(1-p); p = 1 zeroes z.  QUIRK kept (autoencoder.py:233-235):
        the reference builds a fresh nn.Dropout inside forward, and a fresh module is in training mode, so the dropout
        is active in validation and log_images too."""
        mask = self._noise("dropout_mask")
        if mask is None:
            if p >= 1.0:
                mask = torch.zeros(z.shape)
            else:
                mask = (torch.rand(z.shape) >= p).float() / (1.0 - p)
        return ops.latent_combine(z, _lib.upload(mask, z.device), None)

    def _latent_device_noise(self, posterior_obj, draw, sample_posterior, enc_pose):
        """z_obj -> dropout -> + noise -> + enc_pose with the draws of `draw`: one launch (ops.latent_stage).  Where a test injected one of
        the three tensors, the chain of launches the host path runs, fed the injected tensors and the fill's for the rest."""
        p = min(float(self.dropout_prob), 1.0)
        if all(self._noise(k) is None for k in ("posterior_eps", "dropout_mask", "z_noise")):
            return ops.latent_stage(posterior_obj.parameters, draw, add=enc_pose, sample=sample_posterior, dropout_p=p,
                                    noise=self.add_noise_to_z_obj)
        n, c2, h, w = posterior_obj.parameters.shape
        shape = (n, c2 // 2, h, w)
        z = posterior_obj.sample(self._drawn("posterior_eps", shape, draw, "posterior_eps")) if sample_posterior else posterior_obj.mode()
        if p > 0:
            z = ops.latent_combine(z, self._drawn("dropout_mask", shape, draw, "dropout", kind=1, p=p), None)
        if self.add_noise_to_z_obj:
            z = ops.latent_combine(z, None, self._drawn("z_noise", shape, draw, "z_noise"))
        return z if enc_pose is None else ops.latent_combine(z, None, enc_pose)

    def _pretrain_channels(self, input_im):
        """Channels of the all-zero stand-in reconstruction before encoder_pretrain_steps: the input's, as in the reference
        (zeros_like(input_im), :247).  DEVIATION with image_mask_key: the decoder's out_ch, so that the loss and its 4-channel discriminator
        see the shape the decoder will deliver -- the reference's 3-channel zeros die in its discriminator call there."""
        return input_im.shape[1] if self.image_mask_key is None else self.decoder.conv_out.out_channels

    def _forward_device_noise(self, posterior_obj, pose_feat, input_im, sample_posterior):
        """forward with device_noise on: no torch.randn / torch.rand, no upload.  The pose head runs first, so that enc_pose is there
        when the one latent launch wants it as `add` (neither depends on the other's draws)."""
        draw = self._next_draw()
        self.dropout_prob = self._get_dropout_prob()
        dec_pose, bbox_posterior = self._decode_pose(pose_feat, sample_posterior, draw=draw)
        if self.global_step < self.encoder_pretrain_steps:      # z_obj feeds nothing here: not computed
            n, _, h, w = input_im.shape
            dec_obj = torch.zeros((n, h, w, self._pretrain_channels(input_im)), device=self.device).permute(0, 3, 1, 2)
        else:
            enc_pose = self._encode_pose(dec_pose)
            zshape = (posterior_obj.parameters.shape[0], posterior_obj.parameters.shape[1] // 2) + tuple(posterior_obj.parameters.shape[2:])
            assert zshape == tuple(enc_pose.shape), f"z_obj shape: {zshape}, enc_pose shape: {enc_pose.shape}"
            dec_obj = self.decode(self._latent_device_noise(posterior_obj, draw, sample_posterior, enc_pose))
        return dec_obj, dec_pose, posterior_obj, bbox_posterior

    def forward(self, input_im, sample_posterior=True):
        posterior_obj, pose_feat = self.encode(input_im)
        if self.device_noise is not None:
            return self._forward_device_noise(posterior_obj, pose_feat, input_im, sample_posterior)
        z_obj = posterior_obj.sample(self._noise("posterior_eps")) if sample_posterior else posterior_obj.mode()
        self.dropout_prob = self._get_dropout_prob()
        if self.dropout_prob > 0:
            z_obj = self._dropout(z_obj, self.dropout_prob)
        if self.add_noise_to_z_obj:
            z_noise = self._noise("z_noise")
            if z_noise is None:
                z_noise = torch.randn(tuple(z_obj.shape))  # Normal(0,1).sample(...) on the host, as the reference (:239-240)
            z_obj = ops.latent_combine(z_obj, None, _lib.upload(z_noise, self.device))
        dec_pose, bbox_posterior = self._decode_pose(pose_feat, sample_posterior)
        if self.global_step < self.encoder_pretrain_steps:
            n, _, h, w = input_im.shape
            dec_obj = torch.zeros((n, h, w, self._pretrain_channels(input_im)), device=self.device).permute(0, 3, 1, 2)
        else:
            enc_pose = self._encode_pose(dec_pose)
            assert z_obj.shape == enc_pose.shape, f"z_obj shape: {z_obj.shape}, enc_pose shape: {enc_pose.shape}"
            dec_obj = self.decode(ops.latent_combine(z_obj, None, enc_pose))
        return dec_obj, dec_pose, posterior_obj, bbox_posterior

    # ---- batch access (:259-293) ---------------------------------------------------------------------------------
    def get_pose_input(self, batch, k):
        x = batch[k]
        if self.train_on_yaw:
            x[:, 3] = batch["yaw"]
        return x.to(memory_format=torch.contiguous_format).float()

    def get_mask_input(self, batch, k):
        return None if k is None else batch[k]

    def get_class_input(self, batch, k):
        return batch[k]

    def get_bbox_input(self, batch, k):
        return batch[k]

    def get_fill_factor_input(self, batch, k):
        return batch[k]

    def _get_perturbed_pose(self, batch, k):
        x = batch[k].squeeze(1)
        if self.train_on_yaw:
            x = torch.zeros_like(x)
            x[:, -1] = batch["yaw_perturbed"]
        return x

    def _rgb_input(self, batch):
        """get_input(...).permute(0,2,3,1) is the identity on an NCHW `patch` (:296); _rescale on the device."""
        x = batch[self.image_rgb_key]
        if x.dim() == 3:
            x = x[..., None]
        return self._rescale(x.float().to(self.device))

    def _unpack(self, batch):
        rgb_gt = self._rgb_input(batch)
        pose_gt = self.get_pose_input(batch, self.pose_key).to(self.device)
        mask_gt = self.get_mask_input(batch, self.image_mask_key)
        mask_gt = mask_gt.to(self.device) if mask_gt is not None else None
        class_gt = self.get_class_input(batch, self.class_key).to(self.device)
        bbox_gt = self.get_bbox_input(batch, self.bbox_key).to(self.device)
        fill_factor_gt = self.get_fill_factor_input(batch, self.fill_factor_key).to(self.device).float()
        return rgb_gt, mask_gt, pose_gt, class_gt, batch["class_name"], bbox_gt, fill_factor_gt, batch["mask_2d_bbox"]

    # ---- steps (:295-363) ---------------------------------------------------------------------------------------------
    def training_step(self, batch, batch_idx, optimizer_idx):
        rgb_gt, mask_gt, pose_gt, class_gt, class_gt_label, bbox_gt, fill_factor_gt, mask_2d_bbox = self._unpack(batch)
        dec_obj, dec_pose, posterior_obj, bbox_posterior = self.forward(rgb_gt)
        self.log("dropout_prob", self.dropout_prob, prog_bar=True, logger=True, on_step=True, on_epoch=True)
        loss, log_dict = self.loss(rgb_gt, mask_gt, pose_gt, dec_obj, dec_pose, class_gt, class_gt_label, bbox_gt,
                                   fill_factor_gt, posterior_obj, bbox_posterior, optimizer_idx, self.global_step,
                                   mask_2d_bbox, last_layer=self.get_last_layer(), split="train", **self._loss_extras(batch))
        name = "aeloss" if optimizer_idx == 0 else "discloss"
        self.log(name, loss, prog_bar=True, logger=True, on_step=True, on_epoch=True)
        self.log_dict(log_dict, prog_bar=False, logger=True, on_step=True, on_epoch=False)
        return loss

    def _validation_step(self, batch, batch_idx, postfix=""):
        rgb_gt, mask_gt, pose_gt, class_gt, class_gt_label, bbox_gt, fill_factor_gt, mask_2d_bbox = self._unpack(batch)
        dec_obj, dec_pose, posterior_obj, bbox_posterior = self.forward(rgb_gt)
        logs = []
        for optimizer_idx in (0, 1):
            _, log = self.loss(rgb_gt, mask_gt, pose_gt, dec_obj, dec_pose, class_gt, class_gt_label, bbox_gt,
                               fill_factor_gt, posterior_obj, bbox_posterior, optimizer_idx, self.global_step,
                               mask_2d_bbox, last_layer=self.get_last_layer(), split="val" + postfix, **self._loss_extras(batch))
            logs.append(log)
        log_dict_ae, log_dict_disc = logs
        self.log(f"val{postfix}/rec_loss", log_dict_ae[f"val{postfix}/rec_loss"], sync_dist=True)
        del log_dict_ae[f"val{postfix}/rec_loss"]
        self.log_dict(log_dict_ae)
        self.log_dict(log_dict_disc)
        return self.log_dict

    def configure_optimizers(self):
        lr = self.learning_rate
        ae_params = (list(self.encoder.parameters()) + list(self.decoder.parameters())
                     + list(self.quant_conv_obj.parameters()) + list(self.quant_conv_pose.parameters())
                     + list(self.post_quant_conv.parameters()) + list(self.pose_encoder.parameters())
                     + list(self.pose_decoder.parameters()))  # loss.logvar is in no optimizer, as in the reference
        if self.learn_logvar:
            ae_params.append(self.loss.logvar)
        opt_ae = make_adam(ae_params, lr=lr, betas=(0.5, 0.9))
        opt_disc = make_adam(self.loss.discriminator.parameters(), lr=lr, betas=(0.5, 0.9))
        return [opt_ae, opt_disc], []

    # ---- image logging (:379-432) ---------------------------------------------------------------------------------------
    def _perturb_poses(self, batch, dec_pose):
        yaw = self._get_perturbed_pose(batch, self.pose_perturbed_key).squeeze()[:, -1]
        out = dec_pose.clone()
        out[:, 3] = yaw
        assert out.shape == dec_pose.shape
        return out.to(self.device)

    def _perturbed_pose_forward(self, posterior_obj, dec_pose, batch, sample_posterior=True):
        draw = self._next_draw()      # a call of its own: a second sample of the same posterior
        if draw is not None and sample_posterior and self._noise("posterior_eps_perturbed") is None:
            enc_pose = self._encode_pose(self._perturb_poses(batch, dec_pose))
            return self.decode(ops.latent_stage(posterior_obj.parameters, draw, add=enc_pose))
        z_obj = posterior_obj.sample(self._noise("posterior_eps_perturbed")) if sample_posterior else posterior_obj.mode()
        enc_pose = self._encode_pose(self._perturb_poses(batch, dec_pose))
        return self.decode(ops.latent_combine(z_obj, None, enc_pose))

    @torch.no_grad()
    def log_images(self, batch, only_inputs=False, **kwargs):
        log = dict()
        x_rgb = self._rgb_input(batch)
        if not only_inputs:
            xrec, poserec, posterior_obj, _ = self.forward(x_rgb)
            xrec_perturbed = self._perturbed_pose_forward(posterior_obj, poserec, batch)
            log["reconstructions_rgb"] = xrec[:, :3, :, :].clone().detach()
            log["perturbed_pose_reconstruction_rgb"] = xrec_perturbed[:, :3, :, :].clone().detach()
            if kwargs.get("log_ema", False) or self.use_ema:
                with self.ema_scope():
                    log["reconstructions_rgb_ema"] = self.forward(x_rgb)[0][:, :3, :, :].clone().detach()
        log["inputs_rgb"] = x_rgb.clone().detach()
        return log

    def _rescale(self, x):
        return ops.rescale_minmax(x)
