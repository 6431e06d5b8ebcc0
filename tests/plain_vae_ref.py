"""Host references for the plain AutoencoderKL path (tests/test_plain_vae_ref.py holds them to hand-computed values; the GPU tests
compare the HIP path against them).  Two parts:

  * the six GAN logit terms of odvae_gan_logit_terms_f32 and their gradient as a float64 numpy model, with the inputs the GPU test feeds
    the kernel (dyadic logits whose every partial sum is exact in f32; softplus logits at the points where a naive form breaks);
  * a restatement in plain torch of the three upstream methods the plain model needs -- [UPSTREAM] ldm LPIPSWithDiscriminator.forward,
    AutoencoderKL.validation_step and AutoencoderKL.log_images -- on oracle.ldm_model.Encoder / Decoder and oracle.losses' discriminator
    and LPIPS-style net, run in float64.  ldm is not vendored; the semantics are the ones written out in DESIGN.md 7.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.distributions import DiagonalGaussianDistribution
from oracle.ldm_model import Decoder, Encoder
from oracle.losses import LPIPSStyle, NLayerDiscriminator, adopt_weight, hinge_d_loss, weights_init

# ------------------------------------------------------------------------------------------------------------------------------
# the six logit terms
# ------------------------------------------------------------------------------------------------------------------------------
GRID_CAP_BLOCKS = 1024                      # kLogitBlocks of gan_f32.hip: blocks of 256 threads, a thread loops past the cap
PAST_CAP = GRID_CAP_BLOCKS * 256 + 257      # one size at which 257 threads take a second logit
SIZES = [1, 63, 64, 65, 256, 257, 900, 28800]
PLANTED_DYADIC = [1.0, -1.0, 0.0, 4.0, -4.0, 0.875, -0.875, 1.125, -1.125]
PLANTED_SOFTPLUS = [s * v for v in (0.0, 1e-8, 1.0, 20.0, 20.5, 100.0) for s in (1.0, -1.0)]
FAULTS = ["le_for_lt", "wrong_n", "naive_softplus", "swapped"]
# dout6 with power-of-two entries and the two softplus entries off: the hinge / mean gradients are then exact f32 numbers divided by n once
DOUT_HINGE = np.array([0.5, -2.0, 0.25, 1.0, 0.0, 0.0], dtype=np.float32)
DOUT_FULL = np.array([0.5, -2.0, 0.25, 1.0, -0.75, 1.5], dtype=np.float32)


def dyadic_logits(n, seed):
    """n f32 logits that are multiples of 1/8 in [-4, 4]; the first entries are the planted ones (exact +-1: the hinge's kink)"""
    rng = np.random.RandomState(seed)
    x = rng.randint(-32, 33, size=n).astype(np.float32) / 8.0
    k = min(n, len(PLANTED_DYADIC))
    x[:k] = np.roll(np.array(PLANTED_DYADIC, dtype=np.float32), -(seed % 2))[:k]     # n = 1: +1 for one seed, -1 for the other
    return x


def softplus_logits(n, seed):
    rng = np.random.RandomState(seed)
    x = (rng.randn(n) * 4.0).astype(np.float32)
    k = min(n, len(PLANTED_SOFTPLUS))
    x[:k] = np.array(PLANTED_SOFTPLUS, dtype=np.float32)[:k]
    return x


def assert_partial_sums_exact(x):
    """Every partial sum of the logits and of relu(1 -+ x), in any order, is exact in f32: all are multiples of 1/8 and none can pass
    2^24 / 8 in magnitude."""
    x = np.asarray(x, dtype=np.float64)
    assert np.array_equal(x * 8.0, np.round(x * 8.0)) and np.abs(x).max() <= 4.0
    assert (1.0 + np.abs(x)).sum() * 8.0 < 2.0 ** 24, "a partial sum could round in f32"


def _softplus(x, naive=False):
    if naive:      # as an f32 kernel would evaluate it: exp(100) is past f32's range
        with np.errstate(over="ignore"):
            x32 = np.asarray(x, dtype=np.float32)
            return np.log(np.float32(1.0) + np.exp(x32)).astype(np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def logit_terms_f64(real, fake, fault=None):
    """[mean real, mean fake, mean relu(1 - real), mean relu(1 + fake), mean softplus(-real), mean softplus(fake)] in float64; real may be
    None (its three terms are 0).  `fault` plants one of FAULTS."""
    fake = np.asarray(fake, dtype=np.float64)
    real = None if real is None else np.asarray(real, dtype=np.float64)
    if fault == "swapped" and real is not None:
        real, fake = fake, real
    naive = fault == "naive_softplus"
    out = np.zeros(6, dtype=np.float64)
    n_real, n_fake = (0 if real is None else real.size), fake.size
    if fault == "wrong_n" and real is not None:
        n_real, n_fake = n_fake, n_real
    if real is not None:
        out[0] = real.sum() / n_real
        out[2] = np.maximum(1.0 - real, 0.0).sum() / n_real
        out[4] = _softplus(-real, naive).sum() / n_real
    out[1] = fake.sum() / n_fake
    out[3] = np.maximum(1.0 + fake, 0.0).sum() / n_fake
    out[5] = _softplus(fake, naive).sum() / n_fake
    return out


def logit_terms_grad_f64(real, fake, dout6, fault=None):
    """(dreal, dfake) in float64 for the upstream gradient dout6; strict inequalities (relu'(0) = 0, as torch)"""
    d = np.asarray(dout6, dtype=np.float64)
    fake = np.asarray(fake, dtype=np.float64)
    real = None if real is None else np.asarray(real, dtype=np.float64)
    n_real, n_fake = (0 if real is None else real.size), fake.size
    if fault == "wrong_n" and real is not None:
        n_real, n_fake = n_fake, n_real
    if fault == "swapped" and real is not None:      # each tensor gets the other's expression
        dr, df = logit_terms_grad_f64(fake, real, dout6)
        return df, dr
    lt = (lambda a, b: a <= b) if fault == "le_for_lt" else (lambda a, b: a < b)
    dreal = None
    if real is not None:
        dreal = (d[0] - d[2] * lt(real, 1.0) - d[4] * _sigmoid(-real)) / n_real
    dfake = (d[1] + d[3] * lt(-1.0, fake) + d[5] * _sigmoid(fake)) / n_fake
    return dreal, dfake


def torch_logit_terms(real, fake, dout6, dtype):
    """The six terms as the strings of torch ops they replace (F.relu, F.softplus, mean), with autograd, in `dtype` on the CPU"""
    r = torch.tensor(np.asarray(real), dtype=dtype, requires_grad=True)
    f = torch.tensor(np.asarray(fake), dtype=dtype, requires_grad=True)
    out = torch.stack([r.mean(), f.mean(), F.relu(1.0 - r).mean(), F.relu(1.0 + f).mean(), F.softplus(-r).mean(), F.softplus(f).mean()])
    (out * torch.tensor(np.asarray(dout6), dtype=dtype)).sum().backward()
    return out.detach(), r.grad, f.grad


UNEQUAL = [(63, 257), (900, 64)]            # n_real != n_fake, either way round
SOFTPLUS_CASES = [(n, n) for n in SIZES] + UNEQUAL


def ulp_distance(got, ref64):
    """|got - ref| in ulps of the f32 format at ref; inf where got is not finite"""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref64), 2.0 ** -126))) - 23)
    return np.where(np.isfinite(got), np.abs(got - ref64) / ulp, np.inf)


def softplus_figures(out, dreal, dfake, real, fake, dout6):
    """How far an f32 evaluation of the softplus terms is from the float64 model at the same f32 logits:
      out_ulp    worst ulp distance of out[4], out[5]
      grad_abs   worst |d - d64| over both gradients in units of 2^-24 max|dout6| / n: the gradient is a sum of three terms of that order,
                 and where they cancel a ulp distance of the sum says little"""
    want = logit_terms_f64(real, fake)
    wr, wf = logit_terms_grad_f64(real, fake, dout6)
    unit = 2.0 ** -24 * np.abs(np.asarray(dout6, dtype=np.float64)).max()
    g = max((np.abs(np.asarray(dreal, dtype=np.float64) - wr) * len(real)).max(), (np.abs(np.asarray(dfake, dtype=np.float64) - wf) * len(fake)).max())
    if not (np.isfinite(np.asarray(dreal)).all() and np.isfinite(np.asarray(dfake)).all()):
        g = np.inf
    return {"out_ulp": float(ulp_distance(np.asarray(out)[4:6], want[4:6]).max()), "grad_abs": float(g / unit)}


# worst figures of torch's own f32 F.softplus / mean and their autograd backward on the host, over SOFTPLUS_CASES with DOUT_FULL
# (tests/test_plain_vae_ref.py measures them again and holds them to these); the kernel gets 4x
TORCH_SOFTPLUS_FIGURES = {"out_ulp": 1.3, "grad_abs": 2.3}
SOFTPLUS_MARGIN = 4.0


# ------------------------------------------------------------------------------------------------------------------------------
# the upstream methods, restated
# ------------------------------------------------------------------------------------------------------------------------------
def vanilla_d_loss(logits_real, logits_fake):
    return 0.5 * (torch.mean(F.softplus(-logits_real)) + torch.mean(F.softplus(logits_fake)))


class PlainLoss(nn.Module):
    """[UPSTREAM] ldm LPIPSWithDiscriminator"""

    def __init__(self, disc_start, logvar_init=0.0, kl_weight=1.0, pixelloss_weight=1.0, disc_num_layers=3, disc_in_channels=3,
                 disc_factor=1.0, disc_weight=1.0, perceptual_weight=1.0, use_actnorm=False, disc_conditional=False, disc_loss="hinge"):
        super().__init__()
        assert disc_loss in ["hinge", "vanilla"] and not use_actnorm
        self.kl_weight, self.pixel_weight = kl_weight, pixelloss_weight
        self.perceptual_loss = LPIPSStyle().eval()
        self.perceptual_weight = perceptual_weight
        self.logvar = nn.Parameter(torch.ones(size=()) * logvar_init)
        self.discriminator = NLayerDiscriminator(input_nc=disc_in_channels, n_layers=disc_num_layers).apply(weights_init)
        self.discriminator_iter_start = disc_start
        self.disc_loss = hinge_d_loss if disc_loss == "hinge" else vanilla_d_loss
        self.disc_factor, self.discriminator_weight, self.disc_conditional = disc_factor, disc_weight, disc_conditional

    def train(self, mode=True):
        super().train(mode)
        self.perceptual_loss.eval()      # the metric is a fixed function (upstream LPIPS overrides train() the same way)
        return self

    def calculate_adaptive_weight(self, nll_loss, g_loss, last_layer):
        nll_grads = torch.autograd.grad(nll_loss, last_layer, retain_graph=True)[0]
        g_grads = torch.autograd.grad(g_loss, last_layer, retain_graph=True)[0]
        d_weight = torch.norm(nll_grads) / (torch.norm(g_grads) + 1e-4)
        d_weight = torch.clamp(d_weight, 0.0, 1e4).detach()
        return d_weight * self.discriminator_weight

    def forward(self, inputs, reconstructions, posteriors, optimizer_idx, global_step, last_layer=None, cond=None, split="train",
                weights=None):
        rec_loss = torch.abs(inputs.contiguous() - reconstructions.contiguous())
        if self.perceptual_weight > 0:
            p_loss = self.perceptual_loss(inputs.contiguous(), reconstructions.contiguous())
            rec_loss = rec_loss + self.perceptual_weight * p_loss
        nll_loss = rec_loss / torch.exp(self.logvar) + self.logvar
        weighted_nll_loss = nll_loss
        if weights is not None:
            if torch.is_tensor(weights) and weights.dim() == 1:
                weights = weights.reshape(-1, 1, 1, 1)       # one weight per sample
            weighted_nll_loss = weights * nll_loss
        weighted_nll_loss = torch.sum(weighted_nll_loss) / weighted_nll_loss.shape[0]
        nll_loss = torch.sum(nll_loss) / nll_loss.shape[0]
        kl_loss = posteriors.kl()
        kl_loss = torch.sum(kl_loss) / kl_loss.shape[0]
        if optimizer_idx == 0:
            assert cond is None and not self.disc_conditional
            logits_fake = self.discriminator(reconstructions.contiguous())
            g_loss = -torch.mean(logits_fake)
            if self.disc_factor > 0.0:
                try:
                    d_weight = self.calculate_adaptive_weight(nll_loss, g_loss, last_layer=last_layer)
                except RuntimeError:
                    assert not self.training
                    d_weight = torch.tensor(0.0)
            else:
                d_weight = torch.tensor(0.0)
            disc_factor = adopt_weight(self.disc_factor, global_step, threshold=self.discriminator_iter_start)
            loss = weighted_nll_loss + self.kl_weight * kl_loss + d_weight * disc_factor * g_loss
            log = {"{}/total_loss".format(split): loss.clone().detach().mean(), "{}/logvar".format(split): self.logvar.detach(),
                   "{}/kl_loss".format(split): kl_loss.detach().mean(), "{}/nll_loss".format(split): nll_loss.detach().mean(),
                   "{}/rec_loss".format(split): rec_loss.detach().mean(), "{}/d_weight".format(split): d_weight.detach(),
                   "{}/disc_factor".format(split): torch.tensor(disc_factor), "{}/g_loss".format(split): g_loss.detach().mean()}
            return loss, log
        if optimizer_idx == 1:
            assert cond is None
            logits_real = self.discriminator(inputs.contiguous().detach())
            logits_fake = self.discriminator(reconstructions.contiguous().detach())
            disc_factor = adopt_weight(self.disc_factor, global_step, threshold=self.discriminator_iter_start)
            d_loss = disc_factor * self.disc_loss(logits_real, logits_fake)
            log = {"{}/disc_loss".format(split): d_loss.clone().detach().mean(), "{}/logits_real".format(split): logits_real.detach().mean(),
                   "{}/logits_fake".format(split): logits_fake.detach().mean()}
            return d_loss, log


class PlainAutoencoder(nn.Module):
    """[UPSTREAM] ldm AutoencoderKL: forward, training_step, validation_step, log_images; the random draws are arguments"""

    def __init__(self, ddconfig, loss_kwargs, embed_dim, image_key="image"):
        super().__init__()
        self.image_key = image_key
        self.encoder, self.decoder = Encoder(**ddconfig), Decoder(**ddconfig)
        self.loss = PlainLoss(**loss_kwargs)
        assert ddconfig["double_z"]
        self.quant_conv = nn.Conv2d(2 * ddconfig["z_channels"], 2 * embed_dim, 1)
        self.post_quant_conv = nn.Conv2d(embed_dim, ddconfig["z_channels"], 1)
        self.global_step, self.learning_rate = 0, None

    def encode(self, x):
        return DiagonalGaussianDistribution(self.quant_conv(self.encoder(x)))

    def decode(self, z):
        return self.decoder(self.post_quant_conv(z))

    def forward(self, x, eps, sample_posterior=True):
        posterior = self.encode(x)
        z = posterior.sample(eps) if sample_posterior else posterior.mode()
        return self.decode(z), posterior

    def get_input(self, batch, k):
        x = batch[k]
        if len(x.shape) == 3:
            x = x[..., None]
        return x.permute(0, 3, 1, 2).contiguous().to(self.quant_conv.weight.dtype)

    def training_step(self, batch, optimizer_idx, noise):
        inputs = self.get_input(batch, self.image_key)
        reconstructions, posterior = self(inputs, noise["posterior_eps"].to(inputs.dtype))
        loss, log = self.loss(inputs, reconstructions, posterior, optimizer_idx, self.global_step, last_layer=self.decoder.conv_out.weight,
                              split="train")
        return loss, log, dict(inputs=inputs, reconstructions=reconstructions, posterior=posterior)

    def validation_step(self, batch, noise):
        inputs = self.get_input(batch, self.image_key)
        reconstructions, posterior = self(inputs, noise["posterior_eps"].to(inputs.dtype))
        logs = {}
        for optimizer_idx in (0, 1):
            _, log = self.loss(inputs, reconstructions, posterior, optimizer_idx, self.global_step, last_layer=self.decoder.conv_out.weight,
                               split="val")
            logs.update(log)
        return logs

    @torch.no_grad()
    def log_images(self, batch, noise, only_inputs=False):
        log = dict()
        x = self.get_input(batch, self.image_key)
        if not only_inputs:
            xrec, posterior = self(x, noise["posterior_eps"].to(x.dtype))
            log["samples"] = self.decode(noise["samples_eps"].to(x.dtype))       # decode(randn_like(posterior.sample()))
            log["reconstructions"] = xrec
        log["inputs"] = x
        return log

    def configure_optimizers(self):
        lr = self.learning_rate
        ae = (list(self.encoder.parameters()) + list(self.decoder.parameters()) + list(self.quant_conv.parameters())
              + list(self.post_quant_conv.parameters()))
        return [torch.optim.Adam(ae, lr=lr, betas=(0.5, 0.9)), torch.optim.Adam(self.loss.discriminator.parameters(), lr=lr, betas=(0.5, 0.9))]


def train_batch(model, optimizers, batch, noise_per_opt, clip=1.0):
    """One PL-1.9 style batch on the restatement: per optimizer forward, zero_grad, backward, clip, step; global_step += 1 each"""
    out = []
    for idx in (0, 1):
        opt = optimizers[idx]
        others = [p for j, o in enumerate(optimizers) if j != idx for g in o.param_groups for p in g["params"]]
        for p in others:
            p.requires_grad = False
        loss, log, aux = model.training_step(batch, idx, noise_per_opt[idx])
        opt.zero_grad()
        loss.backward()
        if clip:
            torch.nn.utils.clip_grad_norm_([p for g in opt.param_groups for p in g["params"]], clip)
        opt.step()
        for p in others:
            p.requires_grad = True
        model.global_step += 1
        out.append((loss.detach(), log, aux))
    return out


# the test geometry: the smallest at which the discriminator's five 4x4 layers and the VGG stack's four pools still have output
def small_ddconfig(z_channels):
    return dict(double_z=True, z_channels=z_channels, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2], num_res_blocks=1,
                attn_resolutions=[16], dropout=0.0)
