"""CPU restatement of the VQ family, written literally as upstream writes it -- [UPSTREAM] taming VectorQuantizer2 (distance matrix, argmin,
embedding lookup, detach arithmetic), ldm VQLPIPSWithDiscriminator and ldm VQModel -- on oracle.ldm_model.Encoder / Decoder and
oracle.losses' discriminator and LPIPS-style net.  tests/test_vq_ref.py holds it to the closed forms of tests/vq_inputs.py; the GPU
tests compare the HIP path against it.  ldm and taming are not vendored; the formulas are the ones of INTEGRATION.md."""
import torch
import torch.nn as nn

from oracle.ldm_model import Decoder, Encoder
from oracle.losses import LPIPSStyle, NLayerDiscriminator, adopt_weight, hinge_d_loss, weights_init
from plain_vae_ref import vanilla_d_loss


class VectorQuantizerRef(nn.Module):
    """VectorQuantizer2.forward, line by line"""

    def __init__(self, n_e, e_dim, beta, sane_index_shape=False, legacy=True):
        super().__init__()
        self.n_e, self.e_dim, self.beta, self.legacy, self.sane_index_shape = n_e, e_dim, beta, legacy, sane_index_shape
        self.embedding = nn.Embedding(n_e, e_dim)
        self.embedding.weight.data.uniform_(-1.0 / n_e, 1.0 / n_e)
        self.forced_indices = None      # test hook: int64 [M] taken in place of the argmin (the reference AT given indices)

    def distances(self, z):
        zp = z.permute(0, 2, 3, 1).contiguous()
        z_flattened = zp.view(-1, self.e_dim)
        return (torch.sum(z_flattened ** 2, dim=1, keepdim=True) + torch.sum(self.embedding.weight ** 2, dim=1)
                - 2 * torch.einsum("bd,dn->bn", z_flattened, self.embedding.weight.t()))

    def forward(self, z):
        zp = z.permute(0, 2, 3, 1).contiguous()
        d = self.distances(z)
        self.natural_indices = torch.argmin(d, dim=1)
        min_encoding_indices = self.natural_indices if self.forced_indices is None else self.forced_indices.reshape(-1)
        z_q = self.embedding(min_encoding_indices).view(zp.shape)
        if not self.legacy:
            loss = self.beta * torch.mean((z_q.detach() - zp) ** 2) + torch.mean((z_q - zp.detach()) ** 2)
        else:
            loss = torch.mean((z_q.detach() - zp) ** 2) + self.beta * torch.mean((z_q - zp.detach()) ** 2)
        z_q = zp + (z_q - zp).detach()
        z_q = z_q.permute(0, 3, 1, 2).contiguous()
        if self.sane_index_shape:
            min_encoding_indices = min_encoding_indices.reshape(z_q.shape[0], z_q.shape[2], z_q.shape[3])
        return z_q, loss, (None, None, min_encoding_indices)

    def get_codebook_entry(self, indices, shape):
        z_q = self.embedding(indices)
        if shape is not None:
            z_q = z_q.view(shape).permute(0, 3, 1, 2).contiguous()
        return z_q


def measure_perplexity(predicted_indices, n_embed):
    encodings = torch.nn.functional.one_hot(predicted_indices, n_embed).to(torch.float64).reshape(-1, n_embed)
    avg_probs = encodings.mean(0)
    perplexity = (-(avg_probs * torch.log(avg_probs + 1e-10)).sum()).exp()
    cluster_use = torch.sum(avg_probs > 0)
    return perplexity, cluster_use


class VQLossRef(nn.Module):
    """ldm VQLPIPSWithDiscriminator.forward (pixel_loss l1, perceptual_loss lpips)"""

    def __init__(self, disc_start, codebook_weight=1.0, pixelloss_weight=1.0, disc_num_layers=3, disc_in_channels=3, disc_factor=1.0,
                 disc_weight=1.0, perceptual_weight=1.0, use_actnorm=False, disc_conditional=False, disc_ndf=64, disc_loss="hinge",
                 n_classes=None, perceptual_loss="lpips", pixel_loss="l1"):
        super().__init__()
        assert disc_loss in ["hinge", "vanilla"] and perceptual_loss == "lpips" and pixel_loss == "l1" and not use_actnorm
        self.codebook_weight, self.pixel_weight = codebook_weight, pixelloss_weight
        self.perceptual_loss = LPIPSStyle().eval()
        self.perceptual_weight = perceptual_weight
        self.discriminator = NLayerDiscriminator(input_nc=disc_in_channels, n_layers=disc_num_layers, ndf=disc_ndf).apply(weights_init)
        self.discriminator_iter_start = disc_start
        self.disc_loss = hinge_d_loss if disc_loss == "hinge" else vanilla_d_loss
        self.disc_factor, self.discriminator_weight, self.disc_conditional = disc_factor, disc_weight, disc_conditional
        self.n_classes = n_classes

    def train(self, mode=True):
        super().train(mode)
        self.perceptual_loss.eval()
        return self

    def calculate_adaptive_weight(self, nll_loss, g_loss, last_layer):
        nll_grads = torch.autograd.grad(nll_loss, last_layer, retain_graph=True)[0]
        g_grads = torch.autograd.grad(g_loss, last_layer, retain_graph=True)[0]
        d_weight = torch.norm(nll_grads) / (torch.norm(g_grads) + 1e-4)
        d_weight = torch.clamp(d_weight, 0.0, 1e4).detach()
        return d_weight * self.discriminator_weight

    def forward(self, codebook_loss, inputs, reconstructions, optimizer_idx, global_step, last_layer=None, cond=None, split="train",
                predicted_indices=None):
        rec_loss = torch.abs(inputs.contiguous() - reconstructions.contiguous())
        if self.perceptual_weight > 0:
            p_loss = self.perceptual_loss(inputs.contiguous(), reconstructions.contiguous())
            rec_loss = rec_loss + self.perceptual_weight * p_loss
        else:
            p_loss = torch.tensor([0.0])
        nll_loss = torch.mean(rec_loss)
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
            loss = nll_loss + d_weight * disc_factor * g_loss + self.codebook_weight * codebook_loss.mean()
            log = {"{}/total_loss".format(split): loss.clone().detach().mean(), "{}/quant_loss".format(split): codebook_loss.detach().mean(),
                   "{}/nll_loss".format(split): nll_loss.detach().mean(), "{}/rec_loss".format(split): rec_loss.detach().mean(),
                   "{}/p_loss".format(split): p_loss.detach().mean(), "{}/d_weight".format(split): d_weight.detach(),
                   "{}/disc_factor".format(split): torch.tensor(disc_factor), "{}/g_loss".format(split): g_loss.detach().mean()}
            if predicted_indices is not None and self.n_classes is not None:
                with torch.no_grad():
                    perplexity, cluster_usage = measure_perplexity(predicted_indices, self.n_classes)
                log["{}/perplexity".format(split)] = perplexity
                log["{}/cluster_usage".format(split)] = cluster_usage
            return loss, log
        if optimizer_idx == 1:
            logits_real = self.discriminator(inputs.contiguous().detach())
            logits_fake = self.discriminator(reconstructions.contiguous().detach())
            disc_factor = adopt_weight(self.disc_factor, global_step, threshold=self.discriminator_iter_start)
            d_loss = disc_factor * self.disc_loss(logits_real, logits_fake)
            log = {"{}/disc_loss".format(split): d_loss.clone().detach().mean(), "{}/logits_real".format(split): logits_real.detach().mean(),
                   "{}/logits_fake".format(split): logits_fake.detach().mean()}
            return d_loss, log


class VQModelRef(nn.Module):
    """ldm VQModel: encode, decode, forward, the two steps, log_images, configure_optimizers"""

    def __init__(self, ddconfig, loss_kwargs, n_embed, embed_dim, image_key="image", lr_g_factor=1.0, sane_index_shape=False):
        super().__init__()
        self.image_key, self.embed_dim, self.lr_g_factor = image_key, embed_dim, lr_g_factor
        self.encoder, self.decoder = Encoder(**ddconfig), Decoder(**ddconfig)
        self.loss = VQLossRef(**loss_kwargs)
        self.quantize = VectorQuantizerRef(n_embed, embed_dim, beta=0.25, sane_index_shape=sane_index_shape)
        self.quant_conv = nn.Conv2d(ddconfig["z_channels"], embed_dim, 1)
        self.post_quant_conv = nn.Conv2d(embed_dim, ddconfig["z_channels"], 1)
        self.global_step, self.learning_rate = 0, None

    def encode_to_prequant(self, x):
        return self.quant_conv(self.encoder(x))

    def encode(self, x):
        return self.quantize(self.encode_to_prequant(x))

    def decode(self, quant):
        return self.decoder(self.post_quant_conv(quant))

    def decode_code(self, code_b):
        n, h, w = code_b.shape
        return self.decode(self.quantize.get_codebook_entry(code_b.reshape(-1), (n, h, w, self.embed_dim)))

    def forward(self, x):
        quant, diff, (_, _, ind) = self.encode(x)
        return self.decode(quant), diff, ind

    def get_input(self, batch, k):
        x = batch[k]
        if len(x.shape) == 3:
            x = x[..., None]
        return x.permute(0, 3, 1, 2).contiguous().to(self.quant_conv.weight.dtype)

    def training_step(self, batch, optimizer_idx, noise=None):
        x = self.get_input(batch, self.image_key)
        xrec, qloss, ind = self(x)
        loss, log = self.loss(qloss, x, xrec, optimizer_idx, self.global_step, last_layer=self.decoder.conv_out.weight, split="train",
                              predicted_indices=ind)
        return loss, log, dict(inputs=x, reconstructions=xrec, indices=ind, qloss=qloss)

    def validation_step(self, batch, suffix=""):
        x = self.get_input(batch, self.image_key)
        xrec, qloss, ind = self(x)
        logs = {}
        for optimizer_idx in (0, 1):
            loss, log = self.loss(qloss, x, xrec, optimizer_idx, self.global_step, last_layer=self.decoder.conv_out.weight,
                                  split="val" + suffix, predicted_indices=ind)
            logs.update(log)
            if optimizer_idx == 0:
                logs["val%s/aeloss" % suffix] = loss.detach()
        return logs

    @torch.no_grad()
    def log_images(self, batch):
        x = self.get_input(batch, self.image_key)
        xrec, _, _ = self(x)
        return {"inputs": x, "reconstructions": xrec}

    def configure_optimizers(self):
        ae = (list(self.encoder.parameters()) + list(self.decoder.parameters()) + list(self.quantize.parameters())
              + list(self.quant_conv.parameters()) + list(self.post_quant_conv.parameters()))
        return [torch.optim.Adam(ae, lr=self.lr_g_factor * self.learning_rate, betas=(0.5, 0.9)),
                torch.optim.Adam(self.loss.discriminator.parameters(), lr=self.learning_rate, betas=(0.5, 0.9))]


def small_vq_ddconfig(z_channels=4):
    """plain_vae_ref.small_ddconfig with double_z off"""
    from plain_vae_ref import small_ddconfig
    return dict(small_ddconfig(z_channels), double_z=False)


def min_gap(quantizer, h):
    """smallest best-to-second distance gap over the rows of the pre-quantisation latent h, and the largest |h|"""
    d = quantizer.distances(h.double())
    two = torch.topk(d, 2, dim=1, largest=False).values
    return (two[:, 1] - two[:, 0]).min().item(), h.abs().max().item()


# ---- the model-level pair of the GPU tests ---------------------------------------------------------------------------------------------
MODEL_SEED = 23            # tests/test_vq_ref.py checks that no row of this seed's latents sits near a decision boundary
# quant_conv and the codebook of the pair are the procedural draws times 4: the latent and the codes grow by exactly 4 (a power of two: the
# same indices, bit for bit the same mantissas), every distance and every best-to-second gap by 16.  A squared-distance gap measured
# against a relative deviation of the latent depends on that scale; the scale-free form is held beside it in tests/test_vq_ref.py.
LATENT_SCALE = 4.0
N_EMBED, EMBED_DIM = 64, 4
LOSS_KW = dict(disc_start=0, disc_weight=0.5, codebook_weight=1.0, n_classes=N_EMBED)


def build_pair(seed=MODEL_SEED, dtype=torch.float64, loss_kw=(), **model_kw):
    """(odvae_amd VQModel on the CPU with procedural weights, the restatement holding the same weights in `dtype`)"""
    from odvae_amd import synthetic
    from odvae_amd.autoencoder import VQModel
    kw = dict(LOSS_KW, **dict(loss_kw))
    dd = small_vq_ddconfig(EMBED_DIM)
    model = VQModel(dict(dd), {"target": "odvae_amd.losses.VQLPIPSWithDiscriminator", "params": dict(kw)}, N_EMBED, EMBED_DIM, **model_kw)
    synthetic.fill_state_procedural(model, seed=seed)
    with torch.no_grad():      # BatchNorm scales of 1 + 0.05 N: logits spread over several units, the adaptive weight inside (0, 1e4)
        for name, p in model.loss.discriminator.named_parameters():
            if p.dim() == 1 and name.endswith("weight"):
                p.add_(1.0)
    with torch.no_grad():
        for p in (model.quant_conv.weight, model.quant_conv.bias, model.quantize.embedding.weight):
            p.mul_(LATENT_SCALE)
    if model.use_ema:      # (the procedural fill reached the shadows too: start them again as clones of the weights, as the constructor does)
        from odvae_amd.ema import LitEma
        model.model_ema = LitEma(model)
    model.learning_rate = 1e-4
    ref = VQModelRef(dd, kw, N_EMBED, EMBED_DIM, lr_g_factor=model_kw.get("lr_g_factor", 1.0),
                     sane_index_shape=model_kw.get("sane_index_shape", False)).to(dtype)
    sd = {k: v for k, v in model.state_dict().items() if not k.startswith("model_ema.")}
    res = ref.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    ref.learning_rate = model.learning_rate
    return model, ref
