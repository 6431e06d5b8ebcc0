"""PoseLoss / LPIPSWithDiscriminator with the reference's interface and log keys.

Mirrors src/modules/losses/contperceptual.py (PoseLoss :26-375) on top of [UPSTREAM]
ldm/modules/losses/contperceptual.py LPIPSWithDiscriminator (constructor arguments, logvar parameter,
calculate_adaptive_weight) and taming/modules/losses/vqperceptual.py (adopt_weight, hinge_d_loss, vanilla_d_loss).

Hot-path arithmetic (the per-pixel masked L1 term and its gradient, the image-posterior KL, the PatchGAN and the
LPIPS-style network) runs in HIP kernels; the O(B) scalar assembly and the pose-head losses use torch ops on
[B]-sized tensors.  Reference quirks are kept on purpose and marked QUIRK.
"""
import math
import pickle as pkl

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import anomaly
from . import lib as _lib
from . import ops
from .distributions import DiagonalGaussianDistribution
from .gan import LPIPSStyle, NLayerDiscriminator, weights_init

POSE_6D_DIM = 4
LHW_DIM = 3
FILL_FACTOR_DIM = 1
PROB_THRESHOLD_OBJ = 0.2
BACKGROUND_CLASS_IDX = 1  # QUIRK (contperceptual.py:17,228): masks class id 1 ("truck"), not "background" (id 10)
BBOX_DIM = POSE_6D_DIM + LHW_DIM + FILL_FACTOR_DIM


def adopt_weight(weight, global_step, threshold=0, value=0.0):
    return value if global_step < threshold else weight


def hinge_d_loss(logits_real, logits_fake):
    return 0.5 * (torch.mean(F.relu(1.0 - logits_real)) + torch.mean(F.relu(1.0 + logits_fake)))


def vanilla_d_loss(logits_real, logits_fake):
    return 0.5 * (torch.mean(F.softplus(-logits_real)) + torch.mean(F.softplus(logits_fake)))


class SigmoidFocalLoss(nn.Module):
    """mmdet.models.losses.FocalLoss() defaults (use_sigmoid, gamma 2, alpha 0.25, mean over B*classes) restated in
    torch ops for class-index targets (contperceptual.py:11,70,179)."""

    def __init__(self, gamma=2.0, alpha=0.25, loss_weight=1.0):
        super().__init__()
        self.gamma, self.alpha, self.loss_weight = gamma, alpha, loss_weight

    def forward(self, pred, target):
        num_classes = pred.size(1)
        onehot = F.one_hot(target.long(), num_classes=num_classes + 1)[:, :num_classes].type_as(pred)
        p = pred.sigmoid()
        pt = (1 - p) * onehot + p * (1 - onehot)
        focal = (self.alpha * onehot + (1 - self.alpha) * (1 - onehot)) * pt.pow(self.gamma)
        loss = F.binary_cross_entropy_with_logits(pred, onehot, reduction="none") * focal
        return self.loss_weight * loss.mean()


def _elementwise_loss(name, what):
    if name == "l1":
        return nn.L1Loss(reduction="none")
    if name in ("l2", "mse"):
        return nn.MSELoss(reduction="none")
    raise ValueError("Invalid %s loss function. Please provide a valid %s loss function in ['l1', 'l2', 'mse']." % (what, what))


class LPIPSWithDiscriminator(nn.Module):
    """[UPSTREAM] ldm LPIPSWithDiscriminator: owns logvar, the LPIPS-style net and the PatchGAN."""

    def __init__(self, disc_start, logvar_init=0.0, kl_weight=1.0, pixelloss_weight=1.0, disc_num_layers=3,
                 disc_in_channels=3, disc_factor=1.0, disc_weight=1.0, perceptual_weight=1.0, use_actnorm=False,
                 disc_conditional=False, disc_loss="hinge"):
        super().__init__()
        assert disc_loss in ["hinge", "vanilla"]
        self.kl_weight = kl_weight
        self.pixel_weight = pixelloss_weight
        self.perceptual_loss = LPIPSStyle().eval()
        self.perceptual_weight = perceptual_weight
        self.logvar = nn.Parameter(torch.ones(size=()) * logvar_init)
        self.discriminator = NLayerDiscriminator(input_nc=disc_in_channels, n_layers=disc_num_layers,
                                                 use_actnorm=use_actnorm).apply(weights_init)
        self.discriminator_iter_start = disc_start
        self.disc_loss = hinge_d_loss if disc_loss == "hinge" else vanilla_d_loss
        self.disc_factor = disc_factor
        self.discriminator_weight = disc_weight
        self.disc_conditional = disc_conditional
        # With the discriminator off (disc_factor == 0) upstream still evaluates D(x_rec), logs g_loss = -mean D(x_rec) and multiplies it by an
        # exact 0 in the total.  True reproduces that logged value (one discriminator forward without a graph); False (default) skips the pass
        # and logs 0.  Total loss, every other logged term and all gradients are the same either way.
        self.log_exact_g_loss = False

    def _check_perceptual_weights(self):
        """Once per loss object: the reference cannot even be constructed without the real LPIPS weights ([UPSTREAM]
        LPIPS.__init__ downloads them); here a run with perceptual_weight > 0 on the construction-time stand-ins is
        allowed (benchmarks, tests) but never silent."""
        if getattr(self, "_perceptual_checked", False):
            return
        self._perceptual_checked = True
        if self.perceptual_loss.has_synthetic_weights():
            import warnings
            warnings.warn("perceptual_weight = %g but loss.perceptual_loss still holds its seeded SYNTHETIC weights: the "
                          "perceptual term is LPIPS-shaped, not LPIPS. Load a checkpoint carrying loss.perceptual_loss.* or call "
                          "loss.perceptual_loss.load_weights(vgg16=..., lins=...) (torchvision vgg16 + taming vgg.pth)."
                          % self.perceptual_weight, RuntimeWarning, stacklevel=3)

    # The reference takes two partial backward passes (nll_loss and g_loss, each down to the decoder's last layer) for the adaptive weight
    # and then a full one through the same graph: the LPIPS-style VGG stack and the discriminator are back-propagated TWICE per generator
    # step.  Backpropagation is linear in the incoming gradient, so one traversal is enough: take d nll / d x_rec and d g_loss / d x_rec
    # once, get the two last-layer gradients from them (only conv_out's own weight-gradient launch runs: ops.weight_gradient_only), and hand the main backward pass the combined
    # gradient at x_rec through a surrogate term -- same values, same parameter gradients (to summation order), one VGG and one
    # discriminator backward less (≈ 5 % of a configs[3] step).  ODVAE_ADAPTIVE_WEIGHT_ONE_PASS=0 keeps the reference's three passes.
    ONE_PASS = os.environ.get("ODVAE_ADAPTIVE_WEIGHT_ONE_PASS", "1") != "0"

    def adaptive_weight_one_pass(self, nll_loss, g_loss, reconstructions, last_layer):
        """(d_weight, g_nll, g_g): the adaptive weight of calculate_adaptive_weight and the two gradients w.r.t. the reconstruction."""
        anomaly.watch((nll_loss, g_loss))      # torch's anomaly mode checks these backward passes too (no-op when it is off)
        g_nll = torch.autograd.grad(nll_loss, reconstructions, retain_graph=True)[0]
        g_g = torch.autograd.grad(g_loss, reconstructions, retain_graph=True)[0]
        with ops.weight_gradient_only():      # (needs_input_grad is fixed at forward time: without this each probe also runs conv_out's data gradient)
            nll_grads = torch.autograd.grad(reconstructions, last_layer, grad_outputs=g_nll, retain_graph=True)[0]
            g_grads = torch.autograd.grad(reconstructions, last_layer, grad_outputs=g_g, retain_graph=True)[0]
        d_weight = torch.norm(nll_grads) / (torch.norm(g_grads) + 1e-4)
        d_weight = torch.clamp(d_weight, 0.0, 1e4).detach()
        return d_weight * self.discriminator_weight, g_nll, g_g

    def calculate_adaptive_weight(self, nll_loss, g_loss, last_layer=None):
        if last_layer is None:
            last_layer = self.last_layer[0]
        anomaly.watch((nll_loss, g_loss))
        nll_grads = torch.autograd.grad(nll_loss, last_layer, retain_graph=True)[0]
        g_grads = torch.autograd.grad(g_loss, last_layer, retain_graph=True)[0]
        d_weight = torch.norm(nll_grads) / (torch.norm(g_grads) + 1e-4)
        d_weight = torch.clamp(d_weight, 0.0, 1e4).detach()
        return d_weight * self.discriminator_weight

    # ---- the plain loss ([UPSTREAM] ldm contperceptual.py LPIPSWithDiscriminator.forward) ---------------------------------------------
    def _weights_layout(self, weights, shape):
        """(layout, tensor) of ops.loss_weights_layout, (None, None) without weights; `map` layouts ("pixel", "element") take the weighted
        sums of ops.l1_weighted_sums, the other two scale the per-sample sums."""
        if weights is None:
            return None, None
        return ops.loss_weights_layout(weights, *shape)

    def _checked_cond(self, cond, d_input):
        """`cond` of the conditional discriminator as f32 [B,Cc,H,W] on the device of the tensor it is concatenated to (float, bool or
        uint8 in; values as they are, never box-masked, never differentiated); None stays None."""
        if cond is None:
            return None
        want = (d_input.shape[0], d_input.shape[2], d_input.shape[3])
        if not torch.is_tensor(cond) or cond.dim() != 4 or (cond.shape[0], cond.shape[2], cond.shape[3]) != want or cond.shape[1] < 1:
            raise ValueError("cond must be [B,Cc,H,W] = [%d,Cc,%d,%d] for a discriminator input %s, got %s"
                             % (want + (tuple(d_input.shape), tuple(cond.shape) if torch.is_tensor(cond) else type(cond))))
        input_nc = self.discriminator.main[0].in_channels
        if d_input.shape[1] + cond.shape[1] != input_nc:
            raise ValueError("cond has %d channels and the discriminator input %d, but the discriminator was built with disc_in_channels: %d "
                             "(set lossconfig.params.disc_in_channels: %d)" % (cond.shape[1], d_input.shape[1], input_nc, d_input.shape[1] + cond.shape[1]))
        return cond.detach().to(d_input.device).float()

    def _plain_nll(self, rec_sums, chw, weights=None):
        """(nll_loss, weighted_nll_loss) = sum over everything / N of rec_loss / exp(logvar) + logvar, from the per-sample sums of rec_loss.
        No +1e-8 beside exp(logvar) here (PoseLoss has one)."""
        n = rec_sums.numel()
        nll_sums = rec_sums / torch.exp(self.logvar) + self.logvar * chw
        nll_loss = torch.sum(nll_sums) / n
        if weights is None:
            return nll_loss, nll_loss
        w = torch.as_tensor(weights, dtype=nll_sums.dtype, device=nll_sums.device)
        if w.numel() not in (1, n):
            raise NotImplementedError("weights of shape %s: a per-pixel weight map is not on the HIP path (the L1 term arrives as per-sample "
                                      "sums); a scalar or one weight per sample is" % (tuple(w.shape),))
        return nll_loss, torch.sum(w.reshape(-1) * nll_sums) / n

    def forward(self, inputs, reconstructions, posteriors, optimizer_idx, global_step, last_layer=None, cond=None, split="train",
                weights=None):
        if optimizer_idx == 1:
            # the discriminator phase returns d_loss and the two logit means only: as in PoseLoss, the reconstruction (incl. LPIPS) and KL
            # terms upstream evaluates first have no consumer and are not evaluated
            return self._plain_discriminator_phase(inputs, reconstructions, global_step, cond, split)
        if optimizer_idx != 0:
            return None      # (upstream falls off the end of forward as well)
        if cond is None:
            assert not self.disc_conditional
        else:
            assert self.disc_conditional
        cond = self._checked_cond(cond, reconstructions)
        n, c, h, w = inputs.shape
        chw = float(c * h * w)
        rec_sums = ops.l1_masked_sum(inputs, reconstructions, None)      # per-sample sums of |x - x_rec|
        if self.perceptual_weight > 0:
            self._check_perceptual_weights()
            p_loss = self.perceptual_loss(inputs, reconstructions)
            rec_sums = rec_sums + self.perceptual_weight * p_loss.reshape(n) * chw
        nll_loss, weighted_nll_loss = self._plain_nll(rec_sums, chw, weights)
        rec_mean = rec_sums.detach().sum() / (n * chw)
        kl_loss = torch.sum(posteriors.kl()) / n
        g_loss, d_weight, one_pass = self._generator_gan_terms(nll_loss, reconstructions, cond, last_layer, weights)
        disc_factor = adopt_weight(self.disc_factor, global_step, threshold=self.discriminator_iter_start)

        if one_pass is None:
            loss = weighted_nll_loss + self.kl_weight * kl_loss + d_weight * disc_factor * g_loss
        else:
            # the reconstruction-dependent terms enter by VALUE (same expression, same order of additions) and their gradient through
            # `surrogate`, whose derivative w.r.t. the reconstruction is d nll / d x_rec + d_weight * disc_factor * d g_loss / d x_rec; the
            # value added is an exact 0.  logvar keeps its gradient through the same trick on the per-sample sums.
            loss = weighted_nll_loss.detach() + self.kl_weight * kl_loss + d_weight * disc_factor * g_loss.detach()
            grad_at_rec = (one_pass[0] + (d_weight * disc_factor) * one_pass[1]).detach()
            surrogate = (reconstructions * grad_at_rec).sum()
            nll_lv = self._plain_nll(rec_sums.detach(), chw)[0]
            loss = loss + (surrogate - surrogate.detach()) + (nll_lv - nll_lv.detach())

        log = {"{}/total_loss".format(split): loss.clone().detach().mean(),
               "{}/logvar".format(split): self.logvar.detach(),
               "{}/kl_loss".format(split): kl_loss.detach().mean(),
               "{}/nll_loss".format(split): nll_loss.detach().mean(),
               "{}/rec_loss".format(split): rec_mean,
               "{}/d_weight".format(split): d_weight.detach(),
               "{}/disc_factor".format(split): torch.tensor(disc_factor),
               "{}/g_loss".format(split): g_loss.detach().mean()}
        return loss, log

    def _generator_gan_terms(self, nll_loss, reconstructions, cond, last_layer, weights=None):
        """(g_loss, d_weight, one_pass) of the generator phase: g_loss = -mean D(x_rec) (or the disc_factor == 0 shortcut), the adaptive
        weight, and (g_nll, g_g) when the main backward is to start from the combined gradient at the reconstruction (else None).
        Shared by LPIPSWithDiscriminator and VQLPIPSWithDiscriminator."""
        dev = reconstructions.device
        if self.disc_factor > 0.0:
            g_loss = -ops.gan_logit_terms(None, self.discriminator(ops.cat_mask(reconstructions, None, cond)))[1]
        elif self.log_exact_g_loss or (self.discriminator.training and self.discriminator.actnorm_uninitialized()):
            # discriminator off: upstream still evaluates D(x_rec) (BatchNorm running statistics move, ActNorm layers initialise from this
            # tensor on the first training batch) and multiplies the term by an exact 0; the forward runs here without a graph
            with torch.no_grad():
                g_loss = -ops.gan_logit_terms(None, self.discriminator(ops.cat_mask(reconstructions.detach(), None, cond)))[1]
            if not self.log_exact_g_loss:     # the forward ran for the initialisation alone: the logged value stays the shortcut's 0
                g_loss = torch.zeros((), device=dev)
        else:
            g_loss = torch.zeros((), device=dev)
        one_pass = None      # (g_nll, g_g) when the main backward is to start from the combined gradient at the reconstruction
        if self.disc_factor > 0.0:
            ll = last_layer if last_layer is not None else (self.last_layer[0] if getattr(self, "last_layer", None) else None)
            if (self.ONE_PASS and weights is None and ll is not None and torch.is_grad_enabled() and reconstructions.requires_grad
                    and not reconstructions.is_leaf):
                try:
                    d_weight, g_nll, g_g = self.adaptive_weight_one_pass(nll_loss, g_loss, reconstructions, ll)
                    one_pass = (g_nll, g_g)
                except RuntimeError:      # (a last layer the reconstruction's graph does not reach: upstream's fallback, as below)
                    assert not self.training
                    d_weight = torch.zeros((), device=dev)
            else:
                try:
                    d_weight = self.calculate_adaptive_weight(nll_loss, g_loss, last_layer=last_layer)
                except RuntimeError:
                    assert not self.training
                    d_weight = torch.zeros((), device=dev)
        else:
            d_weight = torch.zeros((), device=dev)
        return g_loss, d_weight, one_pass

    def _plain_discriminator_phase(self, inputs, reconstructions, global_step, cond, split):
        """optimizer_idx == 1: hinge / vanilla loss of the discriminator on the target and the detached reconstruction; the two loss terms
        and the two logged logit means come from one kernel (ops.gan_logit_terms)."""
        # A None cond means no concatenation, as upstream.  DEVIATION: upstream has no assert in this phase; here a cond without
        # disc_conditional is refused as in the generator phase (which every training step passes first, and where upstream asserts it).
        assert cond is None or self.disc_conditional
        cond = self._checked_cond(cond, inputs)
        logits_real = self.discriminator(ops.cat_mask(inputs.detach(), None, cond))
        logits_fake = self.discriminator(ops.cat_mask(reconstructions.detach(), None, cond))
        disc_factor = adopt_weight(self.disc_factor, global_step, threshold=self.discriminator_iter_start)
        terms = ops.gan_logit_terms(logits_real, logits_fake)
        pair = (terms[2], terms[3]) if self.disc_loss is hinge_d_loss else (terms[4], terms[5])
        d_loss = disc_factor * (0.5 * (pair[0] + pair[1]))
        log = {"{}/disc_loss".format(split): d_loss.clone().detach().mean(),
               "{}/logits_real".format(split): terms[0].detach(),
               "{}/logits_fake".format(split): terms[1].detach()}
        return d_loss, log


class VQLPIPSWithDiscriminator(LPIPSWithDiscriminator):
    """[UPSTREAM] ldm.modules.losses.vqperceptual.VQLPIPSWithDiscriminator (a superset of taming's): the loss of VQModel.  No logvar and
    no KL term: nll_loss = mean(|x - x_rec| + perceptual_weight * p_loss), plus the adaptive GAN term and codebook_weight times the
    quantiser's loss.  The GAN terms, the one-pass adaptive weight, the disc_factor == 0 shortcut and the discriminator phase are
    LPIPSWithDiscriminator's own code."""

    def __init__(self, disc_start, codebook_weight=1.0, pixelloss_weight=1.0, disc_num_layers=3, disc_in_channels=3, disc_factor=1.0,
                 disc_weight=1.0, perceptual_weight=1.0, use_actnorm=False, disc_conditional=False, disc_ndf=64, disc_loss="hinge",
                 n_classes=None, perceptual_loss="lpips", pixel_loss="l1"):
        nn.Module.__init__(self)      # (LPIPSWithDiscriminator.__init__ would add the logvar parameter, which this loss does not have)
        assert disc_loss in ["hinge", "vanilla"]
        if perceptual_loss != "lpips":
            raise NotImplementedError("VQLPIPSWithDiscriminator(perceptual_loss=%r): only 'lpips' is implemented" % (perceptual_loss,))
        if pixel_loss != "l1":
            raise NotImplementedError("VQLPIPSWithDiscriminator(pixel_loss=%r): only 'l1' is implemented" % (pixel_loss,))
        self.codebook_weight = codebook_weight
        self.pixel_weight = pixelloss_weight
        self.perceptual_loss = LPIPSStyle().eval()
        self.perceptual_weight = perceptual_weight
        self.discriminator = NLayerDiscriminator(input_nc=disc_in_channels, n_layers=disc_num_layers, use_actnorm=use_actnorm,
                                                 ndf=disc_ndf).apply(weights_init)
        self.discriminator_iter_start = disc_start
        self.disc_loss = hinge_d_loss if disc_loss == "hinge" else vanilla_d_loss
        print(f"VQLPIPSWithDiscriminator running with {disc_loss} loss.")
        self.disc_factor = disc_factor
        self.discriminator_weight = disc_weight
        self.disc_conditional = disc_conditional
        self.n_classes = n_classes
        self.log_exact_g_loss = False      # (as in LPIPSWithDiscriminator: with disc_factor == 0, log the exact -mean D(x_rec) instead of 0)

    def forward(self, codebook_loss, inputs, reconstructions, optimizer_idx, global_step, last_layer=None, cond=None, split="train",
                predicted_indices=None):
        if optimizer_idx == 1:
            return self._plain_discriminator_phase(inputs, reconstructions, global_step, cond, split)
        if optimizer_idx != 0:
            return None
        if cond is None:
            assert not self.disc_conditional
        else:
            assert self.disc_conditional
        cond = self._checked_cond(cond, reconstructions)
        n, c, h, w = inputs.shape
        chw = float(c * h * w)
        rec_sums = ops.l1_masked_sum(inputs, reconstructions, None)      # per-sample sums of |x - x_rec|
        if self.perceptual_weight > 0:
            self._check_perceptual_weights()
            p_loss = self.perceptual_loss(inputs, reconstructions)
            rec_sums = rec_sums + self.perceptual_weight * p_loss.reshape(n) * chw
            p_mean = p_loss.detach().mean()
        else:
            p_mean = torch.zeros((), device=inputs.device)
        nll_loss = torch.sum(rec_sums) / (n * chw)      # mean(rec_loss): no logvar here
        g_loss, d_weight, one_pass = self._generator_gan_terms(nll_loss, reconstructions, cond, last_layer)
        disc_factor = adopt_weight(self.disc_factor, global_step, threshold=self.discriminator_iter_start)
        quant_loss = codebook_loss.mean()
        if one_pass is None:
            loss = nll_loss + d_weight * disc_factor * g_loss + self.codebook_weight * quant_loss
        else:      # (the surrogate of LPIPSWithDiscriminator.forward: values by value, the gradient at the reconstruction in one traversal)
            loss = nll_loss.detach() + d_weight * disc_factor * g_loss.detach() + self.codebook_weight * quant_loss
            grad_at_rec = (one_pass[0] + (d_weight * disc_factor) * one_pass[1]).detach()
            surrogate = (reconstructions * grad_at_rec).sum()
            loss = loss + (surrogate - surrogate.detach())
        log = {"{}/total_loss".format(split): loss.clone().detach().mean(),
               "{}/quant_loss".format(split): codebook_loss.detach().mean(),
               "{}/nll_loss".format(split): nll_loss.detach().mean(),
               "{}/rec_loss".format(split): nll_loss.detach().mean(),
               "{}/p_loss".format(split): p_mean,
               "{}/d_weight".format(split): d_weight.detach(),
               "{}/disc_factor".format(split): torch.tensor(disc_factor),
               "{}/g_loss".format(split): g_loss.detach().mean()}
        if predicted_indices is not None and self.n_classes is not None:
            # DEVIATION: upstream asserts n_classes whenever indices arrive (and VQModel always sends them); here the two figures are logged
            # when n_classes is set and skipped otherwise
            with torch.no_grad():
                _, perplexity, cluster_usage = ops.vq_usage(predicted_indices, self.n_classes)
            log["{}/perplexity".format(split)] = perplexity
            log["{}/cluster_usage".format(split)] = cluster_usage
        return loss, log


class PoseLoss(LPIPSWithDiscriminator):
    def __init__(self, train_on_yaw=True, kl_weight_obj=1.0, kl_weight_bbox=1e-6, pose_weight=1.0, mask_weight=0.0,
                 class_weight=1.0, bbox_weight=1.0, fill_factor_weight=1.0, pose_loss_fn=None, mask_loss_fn=None,
                 encoder_pretrain_steps=0, pose_conditioned_generation_steps=7000, use_mask_loss=True,
                 use_class_loss=False, use_bbox_loss=False, num_classes=1,
                 dataset_stats_path="dataset_stats/combined/all.pkl", dataset_stats=None, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.pose_conditioned_generation_steps = pose_conditioned_generation_steps
        self.encoder_pretrain_steps = encoder_pretrain_steps
        self.pose_weight, self.mask_weight = pose_weight, mask_weight
        self.fill_factor_weight, self.class_weight, self.bbox_weight = fill_factor_weight, class_weight, bbox_weight
        self.use_mask_loss = use_mask_loss
        self.num_classes = num_classes
        self.kl_weight_obj, self.kl_weight_bbox = kl_weight_obj, kl_weight_bbox
        self.train_on_yaw = train_on_yaw
        assert pose_loss_fn is not None, "Please provide a pose loss function."
        assert mask_loss_fn is not None, "Please provide a mask loss function."
        assert pose_loss_fn in ["l1", "l2", "mse"], "Please provide a valid pose loss function in ['l1', 'l2', 'mse']."
        self.pose_loss = _elementwise_loss(pose_loss_fn, "pose")
        self.mask_loss = _elementwise_loss(mask_loss_fn, "mask")
        if self.train_on_yaw:
            self.rot_loss_fn = nn.SmoothL1Loss(reduction="none")
        self.class_loss_fn = SigmoidFocalLoss()
        # True: every pose-head term from one HIP kernel (ops.pose_losses); False keeps the per-term torch-op methods below (same
        # values; tests compare the two)
        self.fused_pose_terms = True
        # With the discriminator off (disc_factor == 0) the reference still evaluates D(x_rec), logs g_loss = -mean D(x_rec) (:285-292,331)
        # and multiplies it by an exact 0 in the total.  True reproduces that logged value (one discriminator forward without a graph:
        # 5.5 ms per B=32 step at 256x256, 2 % of the f32 step and 6.5 % of the bf16 one); False (default) skips the pass and logs 0.
        # Total loss, every other logged term and all gradients are the same either way.
        self.log_exact_g_loss = False
        self.bbox_loss_fn = nn.MSELoss(reduction="none")
        self.fill_factor_loss_fn = nn.MSELoss(reduction="none")
        # `dataset_stats` (a dict) is an extension for runs without the pickle, which the reference does not ship
        if dataset_stats is None:
            with open(dataset_stats_path, "rb") as handle:
                dataset_stats = pkl.load(handle)
        self.bbox_distribution_dict = self._create_distribution_from_dataset_stats(dataset_stats)

    # ---- priors over the pose-head posterior (contperceptual.py:82-109) -----------------------------------
    def _create_distribution_from_dataset_stats(self, dataset_stats):
        fixed = {"yaw": (0.0, math.pi), "t1": (0.0, 1.0), "t2": (0.0, 1.0), "fill_factor": (0.5, math.sqrt(2))}
        rot_param = "yaw" if self.train_on_yaw else "v3"
        out = {}
        for label, stats in dataset_stats.items():
            means, logvars = torch.zeros(BBOX_DIM), torch.zeros(BBOX_DIM)
            for idx, key in enumerate(["t1", "t2", "t3", rot_param, "l", "h", "w", "fill_factor"]):
                if key in fixed:
                    mean, std_dev = fixed[key]
                    logvar = 2 * torch.log(torch.tensor(std_dev))
                else:
                    mean, logvar = stats[key]
                means[idx], logvars[idx] = mean, logvar
            out[label] = DiagonalGaussianDistribution(torch.cat((means.unsqueeze(1), logvars.unsqueeze(1)), dim=1))
        return out

    @staticmethod
    def _masked_mean(values, mask_bg):
        # sum / sum(mask) if sum(mask) > 0 else 0 -- evaluated on the device: the reference's host-side `if` would
        # stall the queue once per term (7 syncs per loss evaluation); values and gradients are identical
        denom = torch.sum(mask_bg)
        return torch.sum(values) / torch.clamp(denom, min=1) * (denom > 0)

    # ---- pose-head terms (contperceptual.py:111-132,176-212) ------------------------------------------------
    def compute_pose_loss(self, pred, gt, mask_bg):
        assert pred.shape == gt.shape, "Prediction and ground truth shapes do not match."
        assert pred.shape[1] == POSE_6D_DIM, "Invalid pose dimensionality."
        t1, t2, t3 = (self.pose_loss(pred[:, i], gt[:, i]) for i in range(3))
        if self.train_on_yaw:
            v3 = self.rot_loss_fn(torch.sin(pred[:, 3]), torch.sin(gt[:, 3]))
        else:
            v3 = self.pose_loss(pred[:, 3], gt[:, 3])
        pose_loss = self._masked_mean((t1 + t2 + t3 + v3) * mask_bg, mask_bg)
        return pose_loss, self.pose_weight * pose_loss, t1, t2, t3, v3

    def compute_class_loss(self, class_gt, class_probs, eps=1e-8):
        class_loss = self.class_loss_fn(class_probs, class_gt)
        return class_loss, self.class_weight * class_loss

    def compute_bbox_loss(self, bbox_gt, bbox_pred, mask_bg):
        bbox_loss = self._masked_mean(self.bbox_loss_fn(bbox_gt, bbox_pred) * mask_bg.unsqueeze(1), mask_bg)
        return bbox_loss, self.bbox_weight * bbox_loss

    def compute_fill_factor_loss(self, fill_factor_gt, fill_factor_pred, mask_bg):
        loss = self._masked_mean(self.fill_factor_loss_fn(fill_factor_gt, fill_factor_pred) * mask_bg, mask_bg)
        return loss, self.fill_factor_weight * loss

    def get_mask_loss(self, mask1, mask2, mask_bg):
        if self.use_mask_loss:
            mask_loss = self.mask_loss(mask1, mask2)
            return mask_loss, self.mask_weight * mask_loss
        zero = torch.zeros((), device=mask_bg.device)   # the reference's CPU torch.tensor(0.0), made where it is consumed
        return zero, zero

    def _prior_table(self, device):
        """Per-label prior moments stacked once: {label: row}, mean/var/logvar [L, 8] on `device`."""
        cache = getattr(self, "_prior_cache", None)
        if cache is None or cache[1].device != device:
            labels = list(self.bbox_distribution_dict.keys())
            rows = {lab: i for i, lab in enumerate(labels)}
            stack = lambda attr: torch.stack([getattr(self.bbox_distribution_dict[l], attr).squeeze() for l in labels]).to(device)
            cache = (rows, stack("mean"), stack("var"), stack("logvar"))
            self._prior_cache = cache
        return cache

    def _fused_pose_terms(self, dec_pose, pose_gt, bbox_gt, fill_factor_gt, class_gt, class_gt_label, bbox_posterior):
        """out[9] of ops.pose_losses: the translation / yaw / class / box-size / fill-factor terms and the box-posterior KL of
        compute_pose_loss, compute_class_loss, compute_bbox_loss, compute_fill_factor_loss and compute_pose_kl_loss in one launch."""
        dev = dec_pose.device
        cache = getattr(self, "_prior_pack", None)
        if cache is None or cache[1].device != dev:
            rows, p_mean, p_var, p_logvar = self._prior_table(dev)
            cache = (rows, torch.stack([p_mean, p_var, p_logvar], dim=1).contiguous())     # [L, 3, 8]
            self._prior_pack = cache
        rows, prior = cache
        idx = _lib.upload(torch.tensor([rows[l] if l != "background" else -1 for l in class_gt_label], dtype=torch.int32), dev)
        return ops.pose_losses(dec_pose, bbox_posterior.parameters, pose_gt, bbox_gt, fill_factor_gt.reshape(-1), class_gt, prior, idx,
                               bg_idx=BACKGROUND_CLASS_IDX, l2=not isinstance(self.pose_loss, nn.L1Loss), yaw=self.train_on_yaw,
                               gamma=self.class_loss_fn.gamma, alpha=self.class_loss_fn.alpha)

    def compute_pose_kl_loss(self, bbox_posterior, mask_bg, class_gt):
        """The reference loops over the batch on the host (:196-203), calling kl(other) on [8,1] moments against
        [1,8] prior moments.  QUIRK kept: that broadcast makes entry i of a sample's row the sum over ALL prior
        dimensions j of the (i, j) cross term.  Evaluated here for the whole batch at once (same arithmetic, ~500
        fewer tiny launches per step): [B,8,1] against [B,1,8] -> sum over j."""
        mean, logvar = bbox_posterior.mean, bbox_posterior.logvar           # [B, 8]
        rows, p_mean, p_var, p_logvar = self._prior_table(mean.device)
        # built on the host, sent through the pinned staging ring: a plain torch.tensor(..., device=...) is a pageable
        # copy that makes the host wait for every queued kernel
        idx = _lib.upload(torch.tensor([rows[l] if l != "background" else 0 for l in class_gt]), mean.device)
        keep = _lib.upload(torch.tensor([0.0 if l == "background" else 1.0 for l in class_gt]), mean.device)
        om, ov, ol = p_mean[idx].unsqueeze(1), p_var[idx].unsqueeze(1), p_logvar[idx].unsqueeze(1)   # [B, 1, 8]
        m, lv = mean.unsqueeze(2), logvar.unsqueeze(2)                                               # [B, 8, 1]
        kl = 0.5 * torch.sum(torch.pow(m - om, 2) / (ov + 1e-5) + torch.exp(lv) / (ov + 1e-5) - 1.0 - lv + ol, dim=2)
        return self._masked_mean(kl * keep.unsqueeze(1), mask_bg)

    # ---- reconstruction / KL terms on the image (contperceptual.py:134-164) ----------------------------------
    def _weighted_l1(self, inputs_rgb, reconstructions, mask_2d_bbox, use_pixel_loss, wmap, want_l1):
        """(l1_sums | None, wl1_sums, w_sums) of a weight map per sample; reconstructions may carry more channels than inputs_rgb (read in
        place).  With the pixel term off only w_sums comes from the kernel: it still multiplies the perceptual and the logvar term."""
        if use_pixel_loss:
            return ops.l1_weighted_sums(inputs_rgb, reconstructions, mask_2d_bbox, wmap, want_l1=want_l1)
        w_sums = ops.l1_weighted_sums(None, None, None, wmap, shape=tuple(inputs_rgb.shape), device=inputs_rgb.device)[2]
        zeros = torch.zeros(inputs_rgb.shape[0], device=inputs_rgb.device)
        return (zeros if want_l1 else None), zeros, w_sums

    def _rec_sums(self, inputs_rgb, recon_rgb, mask_2d_bbox, use_pixel_loss, wmap=None, reconstructions=None):
        """(rec_sums, chw, weighted): the per-sample sum over (c,h,w) of rec_loss = |x*m - xr*m| (+ perceptual_weight * p_loss); weighted =
        None, or under a weight map `wmap` (sum of weights * rec_loss, sum of weights) per sample."""
        n, c, h, w = inputs_rgb.shape
        chw = float(c * h * w)
        weighted = None
        if wmap is not None:
            s, ws, w_sums = self._weighted_l1(inputs_rgb, recon_rgb if reconstructions is None else reconstructions, mask_2d_bbox,
                                              use_pixel_loss, wmap, True)
        elif use_pixel_loss:
            s = ops.l1_masked_sum(inputs_rgb, recon_rgb, mask_2d_bbox)
        else:
            s = torch.zeros(n, device=inputs_rgb.device)
        if self.perceptual_weight > 0:
            self._check_perceptual_weights()
            p_loss = self.perceptual_loss(ops.mul_mask(inputs_rgb, mask_2d_bbox), ops.mul_mask(recon_rgb, mask_2d_bbox))
            s = s + self.perceptual_weight * p_loss.reshape(n) * chw
            if wmap is not None:
                ws = ws + self.perceptual_weight * p_loss.reshape(n) * w_sums
        if wmap is not None:
            weighted = (ws, w_sums)
        return s, chw, weighted

    @staticmethod
    def _checked_mask(mask_gt, rgb_gt, dec_obj):
        """The alpha target of image_mask_key as f32 [B,1,H,W] on the images' device (float, bool or uint8 in; values as they are)."""
        if not torch.is_tensor(mask_gt) or mask_gt.dim() != 4 or tuple(mask_gt.shape) != (rgb_gt.shape[0], 1) + tuple(rgb_gt.shape[2:]):
            raise ValueError("mask_gt must be [B,1,H,W] = %s for rgb_gt %s, got %s" % ((rgb_gt.shape[0], 1) + tuple(rgb_gt.shape[2:]),
                             tuple(rgb_gt.shape), tuple(mask_gt.shape) if torch.is_tensor(mask_gt) else type(mask_gt)))
        if dec_obj.dim() != 4 or dec_obj.shape[1] != 4 or dec_obj.shape[0] != rgb_gt.shape[0] or dec_obj.shape[2:] != rgb_gt.shape[2:]:
            # (the reference dies here with a shape error in its discriminator call: cat(rgb_gt, mask_gt) has four channels)
            raise ValueError("image_mask_key needs a 4-channel reconstruction (ddconfig.out_ch: 4, disc_in_channels: 4), got dec_obj %s"
                             % (tuple(dec_obj.shape),))
        return mask_gt.to(rgb_gt.device).float()

    def _rgba_rec_sums(self, rgb_gt, mask_gt, reconstructions, mask_2d_bbox, use_pixel_loss, need_d_input, wmap=None):
        """(rec_sums, chw, mask_sums, rec_rgba_m, weighted): _rec_sums on the RGB part of a 4-channel reconstruction, the per-sample sums of the
        element-wise mask loss |mask_gt*m - rec[:, 3:]*m| (or its square) and reconstructions * m for the discriminator (None unless asked).
        Under a weight map the unweighted sums and the masked copies still come from ops.rgba_terms; the weighted sums from
        ops.l1_weighted_sums on the 4-channel reconstruction in place."""
        n, _, h, w = rgb_gt.shape
        chw = float(3 * h * w)
        perceptual = self.perceptual_weight > 0
        l1_sums, mask_sums, rec_rgb_m, gt_rgb_m, rec_rgba_m, _ = ops.rgba_terms(
            reconstructions, rgb_gt, mask_gt, mask_2d_bbox, l2=not isinstance(self.mask_loss, nn.L1Loss), rec_rgb_m=perceptual,
            gt_rgb_m=perceptual, rec_rgba_m=need_d_input)
        s = l1_sums if use_pixel_loss else torch.zeros(n, device=rgb_gt.device)
        weighted = None
        if wmap is not None:
            _, ws, w_sums = self._weighted_l1(rgb_gt, reconstructions, mask_2d_bbox, use_pixel_loss, wmap, False)
        if perceptual:
            self._check_perceptual_weights()
            p_loss = self.perceptual_loss(gt_rgb_m, rec_rgb_m)
            s = s + self.perceptual_weight * p_loss.reshape(n) * chw
            if wmap is not None:
                ws = ws + self.perceptual_weight * p_loss.reshape(n) * w_sums
        if wmap is not None:
            weighted = (ws, w_sums)
        return s, chw, mask_sums, rec_rgba_m, weighted

    def _mask_loss_mean(self, mask_sums, count):
        """(mask_loss, weighted_mask_loss) of get_mask_loss as scalars: the mean over B*H*W of the element-wise mask loss -- what the
        reference logs -- and mask_weight times it.  QUIRK (:169): NOT multiplied by mask_bg (the reference computes that product and drops it)."""
        if self.use_mask_loss:
            mask_loss = torch.sum(mask_sums) / float(count)
            return mask_loss, self.mask_weight * mask_loss
        zero = torch.zeros((), device=mask_sums.device)
        return zero, zero

    def _get_nll_loss(self, rec_sums, chw, mask_bg, weights=None, weighted=None):
        """weights: a scalar or a [B] tensor (they scale the per-sample sums; a [B,1,1,1] weight arrives here as [B]: multiplied as it
        came it would broadcast against the [B] sums to [B,1,1,B]).  weighted = (sum of weights * rec_loss, sum of weights) per sample for a
        weight map: per sample sum w * nll = wrec / (exp(logvar) + eps) + logvar * wsum (contperceptual.py:147-158)."""
        eps = 1e-8
        nll_sums = rec_sums / (torch.exp(self.logvar) + eps) + self.logvar * chw
        nll_loss = self._masked_mean(nll_sums * mask_bg, mask_bg)
        if weighted is not None:
            wrec_sums, w_sums = weighted
            wnll_sums = wrec_sums / (torch.exp(self.logvar) + eps) + self.logvar * w_sums
            return nll_loss, self._masked_mean(wnll_sums * mask_bg, mask_bg)
        weighted = nll_loss if weights is None else self._masked_mean(weights * nll_sums * mask_bg, mask_bg)
        return nll_loss, weighted

    def _get_kl_loss(self, posteriors, mask_bg):
        return self._masked_mean(posteriors.kl() * mask_bg, mask_bg)

    # ---- forward (contperceptual.py:214-375) -------------------------------------------------------------------
    def forward(self, rgb_gt, mask_gt, pose_gt, dec_obj, dec_pose, class_gt, class_gt_label, bbox_gt, fill_factor_gt,
                posterior_obj, bbox_posterior, optimizer_idx, global_step, mask_2d_bbox, last_layer=None, cond=None,
                split="train", weights=None):
        if mask_2d_bbox is not None:
            mask_2d_bbox = mask_2d_bbox.to(rgb_gt.device)
        use_pixel_loss = global_step >= (self.encoder_pretrain_steps + self.pose_conditioned_generation_steps)
        class_gt = class_gt.to(rgb_gt.device)
        mask_bg = torch.zeros_like(class_gt, device=rgb_gt.device)
        mask_bg[class_gt != BACKGROUND_CLASS_IDX] = 1
        if mask_gt is not None:
            mask_gt = self._checked_mask(mask_gt, rgb_gt, dec_obj)      # image_mask_key: gt_obj = cat(rgb_gt, mask_gt) (:235)
        else:
            self.use_mask_loss = False  # QUIRK (:232,248): no mask channel on either side -- and sticky: a later call WITH a mask finds it off
        rgba = mask_gt is not None
        reconstructions = dec_obj
        recon_rgb = reconstructions[:, :3, :, :] if reconstructions.shape[1] != 3 else reconstructions
        cond = self._checked_cond(cond, reconstructions)
        if optimizer_idx == 1:
            # The discriminator phase returns d_loss and three logit statistics only (contperceptual.py:352-375).  The reference
            # evaluates the pose, reconstruction (incl. LPIPS: 16 VGG convs on two image sets) and KL terms first and then does not use
            # them; they have no consumer here either, so they are not evaluated: same outputs, 11 ms of a 113 ms step.
            return self._discriminator_phase(rgb_gt, reconstructions, mask_2d_bbox, mask_bg, global_step, cond, split, mask_gt=mask_gt)

        pose_rec = dec_pose[:, :POSE_6D_DIM]
        lhw_rec = dec_pose[:, POSE_6D_DIM:POSE_6D_DIM + LHW_DIM]
        fill_factor_rec = dec_pose[:, POSE_6D_DIM + LHW_DIM:BBOX_DIM]
        class_probs = dec_pose[:, BBOX_DIM:]
        fused = self.fused_pose_terms and dec_pose.is_cuda and dec_pose.dim() == 2 and bbox_posterior.parameters.shape == (dec_pose.shape[0], 2 * BBOX_DIM)
        if fused:
            # all pose-head terms (and their gradients) from one kernel: pose_f32.hip
            terms = self._fused_pose_terms(dec_pose, pose_gt, bbox_gt, fill_factor_gt, class_gt, class_gt_label, bbox_posterior)
            pose_loss, class_loss, bbox_loss, fill_factor_loss, kl_loss_obj_bbox = terms[0], terms[1], terms[2], terms[3], terms[4]
            t1_loss, t2_loss, t3_loss, v3_loss = terms[5], terms[6], terms[7], terms[8]
            weighted_pose_loss, weighted_class_loss = self.pose_weight * pose_loss, self.class_weight * class_loss
            weighted_bbox_loss, weighted_fill_factor_loss = self.bbox_weight * bbox_loss, self.fill_factor_weight * fill_factor_loss
        else:
            class_loss, weighted_class_loss = self.compute_class_loss(class_gt, class_probs)
            bbox_loss, weighted_bbox_loss = self.compute_bbox_loss(bbox_gt, lhw_rec, mask_bg)
            # QUIRK (:269): (gt, pred) are passed into the (pred, gt) slots; symmetric for l1/l2
            pose_loss, weighted_pose_loss, t1_loss, t2_loss, t3_loss, v3_loss = self.compute_pose_loss(pose_gt, pose_rec, mask_bg)
            fill_factor_loss, weighted_fill_factor_loss = self.compute_fill_factor_loss(fill_factor_gt, fill_factor_rec.squeeze(), mask_bg)
        layout, wt = self._weights_layout(weights, tuple(rgb_gt.shape))
        wmap = wt if layout in ("pixel", "element") else None
        if layout == "sample":
            weights = wt.to(rgb_gt.device)      # [B], however it was shaped
        if rgba:
            # one pass over the 4-channel reconstruction: the L1 sums over RGB, the mask-loss sums over alpha, the masked RGB pair of the
            # LPIPS-style net and D's masked RGBA input (ops.rgba_terms) in place of l1_masked_sum + three mul_mask + the channel slice
            need_d_input = optimizer_idx == 0 and (self.disc_factor > 0.0 or self.log_exact_g_loss
                                                   or (self.discriminator.training and self.discriminator.actnorm_uninitialized()))
            rec_sums, chw, mask_sums, rec_rgba_m, weighted = self._rgba_rec_sums(rgb_gt, mask_gt, reconstructions, mask_2d_bbox, use_pixel_loss,
                                                                                 need_d_input, wmap)
            mask_loss, weighted_mask_loss = self._mask_loss_mean(mask_sums, mask_gt.numel())
        else:
            mask_loss, weighted_mask_loss = self.get_mask_loss(None, None, mask_bg)
            rec_sums, chw, weighted = self._rec_sums(rgb_gt, recon_rgb, mask_2d_bbox, use_pixel_loss, wmap, reconstructions)
        nll_loss, weighted_nll_loss = self._get_nll_loss(rec_sums, chw, mask_bg, weights, weighted)
        rec_mean = rec_sums.detach().sum() / (rec_sums.numel() * chw)
        kl_loss_obj = self._get_kl_loss(posterior_obj, mask_bg)
        if not fused:
            kl_loss_obj_bbox = self.compute_pose_kl_loss(bbox_posterior, mask_bg, class_gt_label)
        bg4 = mask_bg.reshape(-1, 1, 1, 1)

        if optimizer_idx == 0:
            if cond is None:
                assert not self.disc_conditional
            else:
                assert self.disc_conditional
            if self.disc_factor > 0.0:
                logits_fake = self.discriminator(ops.cat_mask(rec_rgba_m, None, cond) if rgba else ops.cat_mask(reconstructions, mask_2d_bbox, cond))
                g_loss = -torch.mean(logits_fake * bg4)
            elif self.log_exact_g_loss or (self.discriminator.training and self.discriminator.actnorm_uninitialized()):
                # discriminator off: the reference still evaluates D(x_rec) (its BatchNorm running statistics move too) and
                # multiplies the term by an exact 0 (:285-292,305).  The forward runs here without a graph, so the logged
                # `g_loss` and the discriminator's buffers are the reference's; the all-zero backward through D is skipped.
                # use_actnorm: the reference's ActNorm layers initialise from THIS tensor on the first training batch, so the
                # forward also runs while any of them is uninitialised; afterwards the shortcut below applies again.
                with torch.no_grad():
                    d_in = ops.cat_mask(rec_rgba_m.detach(), None, cond) if rgba else ops.cat_mask(reconstructions.detach(), mask_2d_bbox, cond)
                    g_loss = -torch.mean(self.discriminator(d_in) * bg4)
                if not self.log_exact_g_loss:     # the forward ran for the initialisation alone: the logged value stays the shortcut's 0
                    g_loss = torch.zeros((), device=rgb_gt.device)
            else:
                g_loss = torch.zeros((), device=rgb_gt.device)
            one_pass = None      # (g_nll, g_g) when the main backward is to start from the combined gradient at the reconstruction
            if self.disc_factor > 0.0 and global_step > self.encoder_pretrain_steps:
                ll = last_layer if last_layer is not None else (self.last_layer[0] if getattr(self, "last_layer", None) else None)
                if (self.ONE_PASS and weights is None and ll is not None and torch.is_grad_enabled() and reconstructions.requires_grad
                        and not reconstructions.is_leaf and self.encoder_pretrain_steps != -1):
                    d_weight, g_nll, g_g = self.adaptive_weight_one_pass(nll_loss, g_loss, reconstructions, ll)
                    one_pass = (g_nll, g_g)
                else:
                    try:
                        d_weight = self.calculate_adaptive_weight(nll_loss, g_loss, last_layer=last_layer)
                    except RuntimeError:
                        assert not self.training
                        d_weight = torch.zeros((), device=rgb_gt.device)
            else:
                d_weight = torch.zeros((), device=rgb_gt.device)
            disc_factor = adopt_weight(self.disc_factor, global_step, threshold=self.discriminator_iter_start)

            pose_only = (weighted_pose_loss + weighted_class_loss + weighted_bbox_loss + weighted_fill_factor_loss
                         + self.kl_weight_bbox * kl_loss_obj_bbox)
            if self.encoder_pretrain_steps != -1 and global_step > self.encoder_pretrain_steps:
                # one pass: the reconstruction-dependent terms enter by VALUE (same expression, same order of additions) ...
                wn = weighted_nll_loss.detach() if one_pass is not None else weighted_nll_loss
                gl = g_loss.detach() if one_pass is not None else g_loss
                # DEVIATION (image_mask_key with use_mask_loss): the reference leaves weighted_mask_loss unreduced here
                # (:168-170), so its `loss` is a [B,1,H,W] tensor no trainer can back-propagate; weighted_mask_loss is mask_weight * the MEAN
                # of the element-wise mask loss instead -- the value the reference logs as total_loss, with its gradient.  The term keeps its
                # own graph under the one-pass adaptive weight (not detached, not in the surrogate).
                loss = (weighted_pose_loss + weighted_mask_loss.to(rgb_gt.device) + wn + weighted_class_loss
                        + weighted_bbox_loss + weighted_fill_factor_loss + self.kl_weight_obj * kl_loss_obj
                        + self.kl_weight_bbox * kl_loss_obj_bbox + d_weight.to(rgb_gt.device) * disc_factor * gl)
                if one_pass is not None:
                    # ... and their gradient through `surrogate`, whose derivative w.r.t. the reconstruction is d nll / d x_rec + d_weight *
                    # disc_factor * d g_loss / d x_rec -- what a second traversal of the VGG stack and the discriminator would have delivered
                    # there; the value added is an exact 0.  (logvar keeps its gradient through the same trick on the per-sample sums.)
                    grad_at_rec = (one_pass[0] + (d_weight * disc_factor) * one_pass[1]).detach()
                    surrogate = (reconstructions * grad_at_rec).sum()
                    nll_lv = self._get_nll_loss(rec_sums.detach(), chw, mask_bg)[0]
                    loss = loss + (surrogate - surrogate.detach()) + (nll_lv - nll_lv.detach())
            else:
                loss = pose_only

            log = {
                "{}/total_loss".format(split): loss.clone().detach().mean(),
                "{}/logvar".format(split): self.logvar.detach(),
                "{}/kl_loss_obj".format(split): kl_loss_obj.detach().mean(),
                "{}/nll_loss".format(split): nll_loss.detach().mean(),
                "{}/weighted_nll_loss".format(split): weighted_nll_loss.detach().mean(),
                "{}/rec_loss".format(split): rec_mean,
                "{}/d_weight".format(split): d_weight.detach(),
                "{}/disc_factor".format(split): torch.tensor(disc_factor),
                "{}/g_loss".format(split): g_loss.detach().mean(),
                "{}/pose_loss".format(split): pose_loss.detach().mean(),
                "{}/weighted_pose_loss".format(split): weighted_pose_loss.detach().mean(),
                "{}/mask_loss".format(split): mask_loss.detach().mean(),
                "{}/weighted_mask_loss".format(split): weighted_mask_loss.detach().mean(),
                "{}/class_loss".format(split): class_loss.detach(),
                "{}/weighted_class_loss".format(split): weighted_class_loss.detach(),
                "{}/bbox_loss".format(split): bbox_loss.detach(),
                "{}/weighted_bbox_loss".format(split): weighted_bbox_loss.detach(),
                "{}/t1_loss".format(split): t1_loss.detach().mean(),
                "{}/t2_loss".format(split): t2_loss.detach().mean(),
                "{}/t3_loss".format(split): t3_loss.detach().mean(),
                "{}/v3_loss".format(split): v3_loss.detach().mean(),
                "{}/kl_loss_bbox".format(split): kl_loss_obj_bbox.detach().mean(),
                "{}/weighted_kl_loss_bbox".format(split): self.kl_weight_bbox * kl_loss_obj_bbox.detach().mean(),
                "{}/weighted_kl_loss_obj".format(split): self.kl_weight_obj * kl_loss_obj.detach().mean(),
                "{}/fill_factor_loss".format(split): fill_factor_loss.detach().mean(),
                "{}/weighted_fill_factor_loss".format(split): weighted_fill_factor_loss.detach().mean(),
            }
            return loss, log

        return None      # (any other optimizer_idx: the reference falls off the end of forward as well)

    def _discriminator_phase(self, rgb_gt, reconstructions, mask_2d_bbox, mask_bg, global_step, cond, split, mask_gt=None):
        """optimizer_idx == 1 (contperceptual.py:352-375): hinge / vanilla loss of the discriminator on the masked target and the masked,
        detached reconstruction; background samples (mask_bg == 0) drop out of the logits.  mask_gt (image_mask_key): the target is
        cat(rgb_gt, mask_gt) and both masked 4-channel inputs come from one pass (ops.rgba_terms)."""
        bg4 = mask_bg.reshape(-1, 1, 1, 1)      # (cond: checked by forward; None means no concatenation, and there is no assert in this phase)
        if mask_gt is not None:
            terms = ops.rgba_terms(reconstructions.detach(), rgb_gt, mask_gt, mask_2d_bbox, rec_rgba_m=True, gt_rgba_m=True, sums=False)
            logits_real = self.discriminator(ops.cat_mask(terms[5], None, cond))
            logits_fake = self.discriminator(ops.cat_mask(terms[4], None, cond))
        else:
            logits_real = self.discriminator(ops.cat_mask(rgb_gt, mask_2d_bbox, cond).detach())
            logits_fake = self.discriminator(ops.cat_mask(reconstructions, mask_2d_bbox, cond).detach())
        disc_factor = adopt_weight(self.disc_factor, global_step, threshold=self.discriminator_iter_start)
        logits_real = logits_real * bg4
        logits_fake = logits_fake * bg4
        d_loss = disc_factor * self.disc_loss(logits_real, logits_fake)
        log = {"{}/disc_loss".format(split): d_loss.clone().detach().mean(),
               "{}/logits_real".format(split): logits_real.detach().mean(),
               "{}/logits_fake".format(split): logits_fake.detach().mean()}
        return d_loss, log
