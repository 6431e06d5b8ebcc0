"""Host references for the losses' `weights` and `cond` arguments (tests/test_loss_weights_inputs.py holds them to the element-wise
formulas and shows that their acceptance rules reject planted faults; the GPU tests compare the kernels and the losses against them).

  * float64 restatements of the three kernels on [N][HW][C] arrays: the weighted L1 sums (odvae_l1_weighted_sums_f32), their backward
    (odvae_l1_weighted_bwd_f32) and the masked concatenation with its backward (odvae_cat_mask_f32 / _bwd_f32);
  * inputs on a coarse binary grid and `sums_are_exact`, the host-side precondition under which every partial sum of the kernels is
    exact in f32 -- sums and elements are then bit for bit the float64 answer, whatever the order of the additions;
  * `host_model`: the kernels' arithmetic in f32 numpy with one planted fault at a time (FAULTS), and the `accept_*` rules the GPU tests
    apply to the device's outputs;
  * `WeightedPlainLoss`: [UPSTREAM] ldm LPIPSWithDiscriminator.forward with `weights` and `cond` honoured as upstream writes them
    (weights * nll_loss on [N,C,H,W]; torch.cat((x, cond), dim=1) in front of the discriminator), on tests/plain_vae_ref.PlainLoss.
"""
import numpy as np
import torch

import plain_vae_ref as P

GRID_CAP_BLOCKS = 256      # kL1wBlocks of csrc/elementwise.hip: a sample's pixels go over at most this many 256-thread blocks
PAST_CAP = GRID_CAP_BLOCKS * 256 + 259
FAULTS = ("weight_before_abs", "w_sum_boxed", "pixel_weight_once", "cond_times_box", "grad_to_cond", "dxr_channel3", "sign_at_tie")


# ------------------------------------------------------------------------------------------------------------------------------
# float64 restatements
# ------------------------------------------------------------------------------------------------------------------------------
def _full_weight(wgt, per_channel, c):
    return wgt if per_channel else wgt[..., None].expand(*wgt.shape, c)


def l1_weighted_sums_f64(x, xr, box, wgt, per_channel):
    """(l1, wl1, w), each [N] float64.  x [N,HW,C], xr [N,HW,Cr >= C], box [N,HW] or None, wgt [N,HW] or [N,HW,C]; x = xr = None: the
    weight sums alone (l1 and wl1 None), for which the channel count comes from a per-channel wgt or must be given as `x` = int."""
    if x is None or isinstance(x, int):
        c = wgt.shape[-1] if per_channel else int(x)
        return None, None, _full_weight(wgt.double(), per_channel, c).sum(dim=(1, 2))
    x, xr, wgt = x.double(), xr.double(), wgt.double()
    c = x.shape[-1]
    b = torch.ones_like(x[..., 0]) if box is None else box.double()
    t = (x * b[..., None] - xr[..., :c] * b[..., None]).abs()
    w = _full_weight(wgt, per_channel, c)
    return t.sum(dim=(1, 2)), (w * t).sum(dim=(1, 2)), w.sum(dim=(1, 2))


def l1_weighted_bwd_f64(x, xr, box, wgt, per_channel, g_l1, g_wl1):
    """dxr [N,HW,Cr] float64: ((g_l1 + g_wl1 * wgt) * sign(rm - xm)) * box for c < C, 0 beyond; a None gradient is a zero."""
    x, xr, wgt = x.double(), xr.double(), wgt.double()
    n, hw, c = x.shape
    b = (torch.ones_like(x[..., 0]) if box is None else box.double())[..., None]
    w = _full_weight(wgt, per_channel, c)
    gl = torch.zeros(n, dtype=torch.float64) if g_l1 is None else g_l1.double()
    gw = torch.zeros(n, dtype=torch.float64) if g_wl1 is None else g_wl1.double()
    out = torch.zeros_like(xr)
    out[..., :c] = ((gl[:, None, None] + gw[:, None, None] * w) * torch.sign(xr[..., :c] * b - x * b)) * b
    return out


def cat_mask_f64(x, box, cond):
    x, cond = x.double(), cond.double()
    b = (torch.ones_like(x[..., 0]) if box is None else box.double())[..., None]
    return torch.cat((x * b, cond), dim=-1)


def cat_mask_bwd_f64(dy, box, cx):
    dy = dy.double()
    b = (torch.ones_like(dy[..., 0]) if box is None else box.double())[..., None]
    return dy[..., :cx] * b


# ------------------------------------------------------------------------------------------------------------------------------
# exact inputs
# ------------------------------------------------------------------------------------------------------------------------------
def exact_inputs(n, hw, c, cr, per_channel, seed, with_box=True, q=8, wq=4, a=1):
    """(x, xr, box, wgt) float64: images multiples of 1/q in [-a, a], weights multiples of 1/wq in [-1, 2] (a negative
    weight is legal, and it is what tells weights * |d| from |weights * d|), box {0,1} or None.  A tenth of
    the reconstruction's elements equal the target's (ties of the L1 term); the channels of xr past C hold values that must not be read."""
    g = torch.Generator().manual_seed(seed)
    draw = lambda *shape: torch.randint(-a * q, a * q + 1, shape, generator=g).double() / q
    x, xr = draw(n, hw, c), draw(n, hw, cr)
    tie = torch.rand(n, hw, c, generator=g) < 0.1
    xr[..., :c] = torch.where(tie, x, xr[..., :c])
    if cr > c:
        xr[..., c:] = 1000.0 + draw(n, hw, cr - c)
    wgt = torch.randint(-wq, 2 * wq + 1, (n, hw, c) if per_channel else (n, hw), generator=g).double() / wq
    box = torch.randint(0, 2, (n, hw), generator=g).double() if with_box else None
    return x, xr, box, wgt


def sums_are_exact(x, xr, box, wgt, per_channel):
    """True when every partial sum of the three per-sample sums, in ANY order and grouping, is exact in f32 (and so is the f32 result):
    the terms of a sum are multiples of one power of two g, and the magnitudes of a whole sample's terms add up to less than 2^24 g --
    every partial sum is then a multiple of g below 2^24 g in magnitude, an f32 number.  The element-wise products and differences must be exact too: checked
    by evaluating them in f32 and in f64."""
    c = x.shape[-1]
    b = (torch.ones_like(x[..., 0]) if box is None else box)[..., None]
    t64 = (x * b - xr[..., :c] * b).abs()
    w64 = _full_weight(wgt, per_channel, c)
    t32 = (x.float() * b.float() - xr[..., :c].float() * b.float()).abs()
    if not (torch.equal(t32.double(), t64) and torch.equal((w64.float() * t32).double(), w64 * t64)):
        return False

    def grain(v):      # the largest power of two every element is a multiple of (down to 2^-20)
        for k in range(0, 21):
            if torch.equal(v * 2.0 ** k, torch.round(v * 2.0 ** k)):
                return 2.0 ** -k
        return None
    for terms in (t64, w64 * t64, w64):
        g = grain(terms)
        if g is None or not bool((terms.abs().sum(dim=(1, 2)) < 2.0 ** 24 * g).all()):
            return False
    return True


def exact_grads(n, seed):
    """(g_l1, g_wl1): multiples of 1/4 of magnitude <= 2; times a weight that is a multiple of 1/4 <= 2 every product and sum is exact"""
    g = torch.Generator().manual_seed(seed)
    q = lambda: torch.randint(-8, 9, (n,), generator=g).double() / 4.0
    return q(), q()


def exact_cat_inputs(n, hw, cx, cc, seed, with_box=True):
    g = torch.Generator().manual_seed(seed)
    draw = lambda *shape: torch.randint(-16, 17, shape, generator=g).double() / 8
    x, cond, dy = draw(n, hw, cx), draw(n, hw, cc), draw(n, hw, cx + cc)
    box = torch.randint(0, 2, (n, hw), generator=g).double() if with_box else None
    return x, box, cond, dy


# ------------------------------------------------------------------------------------------------------------------------------
# a host model of the kernels with planted faults, and the acceptance rules
# ------------------------------------------------------------------------------------------------------------------------------
def host_model(x, xr, box, wgt, per_channel, g_l1=None, g_wl1=None, fault=None):
    """(l1, wl1, w, dxr) as an f32 evaluation of the kernels' arithmetic (numpy, float32 throughout); `fault` plants one of FAULTS"""
    f = np.float32
    X, XR, W = x.numpy().astype(f), xr.numpy().astype(f), wgt.numpy().astype(f)
    n, hw, c = X.shape
    cr = XR.shape[-1]
    B = np.ones((n, hw), dtype=f) if box is None else box.numpy().astype(f)
    Wf = W if per_channel else np.repeat(W[..., None], c, axis=-1)
    xm, rm = X * B[..., None], XR[..., :c] * B[..., None]
    if fault == "weight_before_abs":
        t = np.abs(xm - rm)
        wt = np.abs(Wf * xm - Wf * rm)
    else:
        t = np.abs(xm - rm)
        wt = Wf * t
    wsum_terms = Wf * B[..., None] if fault == "w_sum_boxed" else Wf
    if fault == "pixel_weight_once" and not per_channel:
        wsum_terms = wsum_terms[..., :1]
    l1, wl1, w = t.sum(axis=(1, 2), dtype=np.float64), wt.sum(axis=(1, 2), dtype=np.float64), wsum_terms.sum(axis=(1, 2), dtype=np.float64)
    gl = np.zeros(n, dtype=f) if g_l1 is None else g_l1.numpy().astype(f)
    gw = np.zeros(n, dtype=f) if g_wl1 is None else g_wl1.numpy().astype(f)
    d = rm - xm
    sg = np.where(d > 0, f(1), np.where(d < 0, f(-1), f(1) if fault == "sign_at_tie" else f(0)))
    dxr = np.zeros((n, hw, cr), dtype=f)
    dxr[..., :c] = ((gl[:, None, None] + gw[:, None, None] * Wf) * sg) * B[..., None]
    if fault == "dxr_channel3" and cr > c:
        dxr[..., c] = gl[:, None]
    return (torch.from_numpy(l1.astype(f)), torch.from_numpy(wl1.astype(f)), torch.from_numpy(w.astype(f)), torch.from_numpy(dxr))


def host_cat_model(x, box, cond, dy, fault=None):
    """(y, dx, dcond): cat_mask and its backward in f32 numpy; dcond is what a kernel would leave in cond's gradient (None = nothing)"""
    f = np.float32
    X, C, DY = x.numpy().astype(f), cond.numpy().astype(f), dy.numpy().astype(f)
    B = (np.ones(X.shape[:2], dtype=f) if box is None else box.numpy().astype(f))[..., None]
    y = np.concatenate((X * B, C * B if fault == "cond_times_box" else C), axis=-1)
    dx = DY[..., :X.shape[-1]] * B
    dcond = torch.from_numpy(DY[..., X.shape[-1]:]) if fault == "grad_to_cond" else None
    return torch.from_numpy(y), torch.from_numpy(dx), dcond


def same(got, want):
    """bit for bit the float64 answer (an f32 tensor whose every element, widened, equals the float64 value)"""
    return got is not None and got.dtype == torch.float32 and torch.equal(got.double().cpu(), want)


def accept_sums(got, x, xr, box, wgt, per_channel):
    """The rule of the exact tests for (l1, wl1, w): each given sum is bit for bit the float64 answer"""
    want = l1_weighted_sums_f64(x, xr, box, wgt, per_channel)
    return all(g is None or same(g, w) for g, w in zip(got, want))


def accept_bwd(got, x, xr, box, wgt, per_channel, g_l1, g_wl1):
    """... and for dxr: every element, the channels past C included (they are zeros), is the float64 answer"""
    return same(got, l1_weighted_bwd_f64(x, xr, box, wgt, per_channel, g_l1, g_wl1))


def accept_cat(got_y, got_dx, got_dcond, x, box, cond, dy):
    """... and for cat_mask: y and dx are the float64 answers and nothing arrives at cond"""
    return same(got_y, cat_mask_f64(x, box, cond)) and same(got_dx, cat_mask_bwd_f64(dy, box, x.shape[-1])) and got_dcond is None


# ------------------------------------------------------------------------------------------------------------------------------
# upstream's plain loss with weights and cond
# ------------------------------------------------------------------------------------------------------------------------------
class WeightedPlainLoss(P.PlainLoss):
    """[UPSTREAM] ldm LPIPSWithDiscriminator.forward as it is written, `weights` and `cond` included: weighted_nll_loss = weights *
    nll_loss on [N,C,H,W] (a 1-D [N] weight read as one per sample, this project's reading), both reduced as sum / N; the generator phase
    asserts `cond is None => not disc_conditional` / `cond given => disc_conditional` and feeds cat((x_rec, cond), 1) to the
    discriminator; the discriminator phase feeds cat((x, cond), 1) and cat((x_rec.detach(), cond), 1), without an assert."""

    def forward(self, inputs, reconstructions, posteriors, optimizer_idx, global_step, last_layer=None, cond=None, split="train", weights=None):
        rec_loss = torch.abs(inputs.contiguous() - reconstructions.contiguous())
        if self.perceptual_weight > 0:
            rec_loss = rec_loss + self.perceptual_weight * self.perceptual_loss(inputs.contiguous(), reconstructions.contiguous())
        nll_loss = rec_loss / torch.exp(self.logvar) + self.logvar
        weighted_nll_loss = nll_loss
        if weights is not None:
            if torch.is_tensor(weights) and weights.dim() == 1 and weights.numel() == nll_loss.shape[0]:
                weights = weights.reshape(-1, 1, 1, 1)
            weighted_nll_loss = weights * nll_loss
        weighted_nll_loss = torch.sum(weighted_nll_loss) / weighted_nll_loss.shape[0]
        nll_loss = torch.sum(nll_loss) / nll_loss.shape[0]
        kl_loss = posteriors.kl()
        kl_loss = torch.sum(kl_loss) / kl_loss.shape[0]
        if optimizer_idx == 0:
            if cond is None:
                assert not self.disc_conditional
                logits_fake = self.discriminator(reconstructions.contiguous())
            else:
                assert self.disc_conditional
                logits_fake = self.discriminator(torch.cat((reconstructions.contiguous(), cond), dim=1))
            g_loss = -torch.mean(logits_fake)
            if self.disc_factor > 0.0:
                d_weight = self.calculate_adaptive_weight(nll_loss, g_loss, last_layer=last_layer)
            else:
                d_weight = torch.tensor(0.0)
            disc_factor = P.adopt_weight(self.disc_factor, global_step, threshold=self.discriminator_iter_start)
            loss = weighted_nll_loss + self.kl_weight * kl_loss + d_weight * disc_factor * g_loss
            log = {"{}/total_loss".format(split): loss.clone().detach().mean(), "{}/logvar".format(split): self.logvar.detach(),
                   "{}/kl_loss".format(split): kl_loss.detach().mean(), "{}/nll_loss".format(split): nll_loss.detach().mean(),
                   "{}/rec_loss".format(split): rec_loss.detach().mean(), "{}/d_weight".format(split): d_weight.detach(),
                   "{}/disc_factor".format(split): torch.tensor(disc_factor), "{}/g_loss".format(split): g_loss.detach().mean()}
            return loss, log
        if optimizer_idx == 1:
            if cond is None:
                logits_real = self.discriminator(inputs.contiguous().detach())
                logits_fake = self.discriminator(reconstructions.contiguous().detach())
            else:
                logits_real = self.discriminator(torch.cat((inputs.contiguous().detach(), cond), dim=1))
                logits_fake = self.discriminator(torch.cat((reconstructions.contiguous().detach(), cond), dim=1))
            disc_factor = P.adopt_weight(self.disc_factor, global_step, threshold=self.discriminator_iter_start)
            d_loss = disc_factor * self.disc_loss(logits_real, logits_fake)
            log = {"{}/disc_loss".format(split): d_loss.clone().detach().mean(), "{}/logits_real".format(split): logits_real.detach().mean(),
                   "{}/logits_fake".format(split): logits_fake.detach().mean()}
            return d_loss, log


def weighted_nll_from_sums(l1, wl1, w, p_loss, perceptual_weight, logvar, eps):
    """Per sample sum over (c,h,w) of weights * nll from the three sums: (WL1 + pw p W) / (exp(logvar) + eps) + logvar W -- the identity
    the losses use (tests/test_loss_weights_inputs.py holds it to the element-wise formula)"""
    return (wl1 + perceptual_weight * p_loss * w) / (np.exp(logvar) + eps) + logvar * w
