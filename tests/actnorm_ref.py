"""ActNorm and the ActNorm PatchGAN in plain torch: the yardstick of the `use_actnorm` tests.

The taming sources (taming/modules/util.py ActNorm, taming/modules/discriminator/model.py NLayerDiscriminator) are not at hand; this
is the published algorithm restated, as odvae_amd/gan.py restates it for the HIP path, and parity for this layer is "unpinned" in
the sense of DESIGN.md 5.  The oracle package ignores `use_actnorm`.

ActNorm(num_features, logdet=False, affine=True, allow_reverse_init=False): parameters loc = zeros, scale = ones [1,C,1,1], uint8
buffer `initialized` = 0; h = scale * (x + loc).  In training mode, while `initialized` == 0, the layer first sets, without a graph,
loc = -mean_c, scale = 1 / (std_c + 1e-6) with the unbiased (n - 1) standard deviation over N*H*W, and `initialized` = 1; the same
forward already uses the new values.  In eval mode an uninitialised layer stays so and applies loc = 0, scale = 1.

NLayerDiscriminator(use_actnorm=True): the pix2pix PatchGAN with ActNorm at main.{3,6,9} and a bias on the convolutions at
main.{2,5,8}.  `weights_init` matches on the class names "Conv" and "BatchNorm": loc and scale stay at 0 and 1.

Everything follows the module's dtype (`.double()` gives the float64 reference).  Plain module: no fixtures, no device.
"""
import torch
import torch.nn as nn

SLOPE = 0.2
EPS = 1e-6


class ActNorm(nn.Module):
    def __init__(self, num_features, logdet=False, affine=True, allow_reverse_init=False):
        assert affine
        super().__init__()
        if logdet or allow_reverse_init:
            raise NotImplementedError("logdet / reverse are not on the discriminator's path")
        self.loc = nn.Parameter(torch.zeros(1, num_features, 1, 1))
        self.scale = nn.Parameter(torch.ones(1, num_features, 1, 1))
        self.register_buffer("initialized", torch.tensor(0, dtype=torch.uint8))

    def initialize(self, x):
        with torch.no_grad():
            flat = x.permute(1, 0, 2, 3).reshape(x.shape[1], -1)
            mean = flat.mean(1).view(1, -1, 1, 1)
            std = flat.std(1, unbiased=True).view(1, -1, 1, 1)
            self.loc.data.copy_(-mean)
            self.scale.data.copy_(1.0 / (std + EPS))

    def forward(self, x):
        if self.training and self.initialized.item() == 0:
            self.initialize(x)
            self.initialized.fill_(1)
        return self.scale * (x + self.loc)


def weights_init(m):
    classname = m.__class__.__name__
    if classname.find("Conv") != -1:
        nn.init.normal_(m.weight.data, 0.0, 0.02)
    elif classname.find("BatchNorm") != -1:
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0)


class NLayerDiscriminator(nn.Module):
    def __init__(self, input_nc=3, ndf=64, n_layers=3, use_actnorm=True):
        super().__init__()
        assert use_actnorm, "the BatchNorm variant is oracle.losses.NLayerDiscriminator"
        layers = [nn.Conv2d(input_nc, ndf, 4, 2, 1), nn.LeakyReLU(SLOPE, True)]
        mult = 1
        for n in range(1, n_layers + 1):
            prev, mult = mult, min(2 ** n, 8)
            stride = 2 if n < n_layers else 1
            layers += [nn.Conv2d(ndf * prev, ndf * mult, 4, stride, 1, bias=True), ActNorm(ndf * mult), nn.LeakyReLU(SLOPE, True)]
        layers += [nn.Conv2d(ndf * mult, 1, 4, 1, 1)]
        self.main = nn.Sequential(*layers)

    def forward(self, input):
        return self.main(input)


def actnorm_layers(net):
    return [m for m in net.modules() if type(m).__name__.startswith("ActNorm")]


# ---- closed forms of the backward (what the HIP kernels evaluate) ----------------------------------------------------------------------
def closed_form_backward(x, loc, scale, dy, slope=SLOPE):
    """(dx, dloc, dscale) of y = lrelu(scale * (x + loc)): with g = dy * lrelu'(h), dx = scale * g, dloc = scale * sum g,
    dscale = sum g (x + loc), the sums over N, H, W; dloc / dscale shaped [1,C,1,1]"""
    t = x + loc
    h = scale * t
    g = dy * torch.where(h > 0, torch.ones_like(h), torch.full_like(h, slope))
    return scale * g, scale * g.sum((0, 2, 3), keepdim=True), (g * t).sum((0, 2, 3), keepdim=True)


def autograd_backward(x, loc, scale, dy, slope=SLOPE):
    xr, lr, sr = (t.detach().clone().requires_grad_(True) for t in (x, loc, scale))
    torch.nn.functional.leaky_relu(sr * (xr + lr), slope).backward(dy)
    return xr.grad, lr.grad, sr.grad
