"""PatchGAN discriminator and the LPIPS-style perceptual network.

* NLayerDiscriminator / weights_init: [UPSTREAM] taming/modules/discriminator/model.py (pix2pix PatchGAN):
  Conv(4x4,s2,p1)+LeakyReLU(0.2), two Conv(4x4,s2,p1,no bias)+BatchNorm2d+LeakyReLU, one Conv(4x4,s1,p1,no bias)+BN+
  LeakyReLU, Conv(4x4,s1,p1) -> logits [B,1,30,30] at 256x256 (src/modules/losses/contperceptual.py:285).
  state_dict keys main.{0,2,3,5,6,8,9,11} as in the reference checkpoint layout.
* ActNormLReLU / NLayerDiscriminator(use_actnorm=True): [UPSTREAM] taming/modules/util.py ActNorm and the `use_actnorm` branch of the
  same NLayerDiscriminator.  The taming sources are not at hand: this is the published algorithm restated (parity "unpinned",
  DESIGN.md 5).  ActNorm(num_features, logdet=False, affine=True, allow_reverse_init=False): parameters loc (zeros) and scale (ones)
  [1,C,1,1], uint8 buffer `initialized`; h = scale * (x + loc); on the first TRAINING forward, without a graph, loc = -mean_c and
  scale = 1 / (std_c + 1e-6) with the unbiased std over N*H*W, `initialized` = 1, and that same forward already uses the new values; in
  eval mode an uninitialised layer stays uninitialised.  ActNorm stands at main.{3,6,9}, the convolutions at main.{2,5,8} get a bias,
  weights_init leaves loc / scale alone (it matches "Conv" and "BatchNorm").
* LPIPSStyle: [UPSTREAM] taming/modules/losses/lpips.py structure (ScalingLayer, VGG16 feature slices relu1_2 ... relu5_3,
  channel-unit-normalise, squared difference, 1x1 "lin" heads, spatial mean, sum over the five taps).  The real LPIPS
  weights are downloads (torchvision VGG16 + vgg.pth) that do not exist offline, so the weights here are seeded
  synthetic and frozen unless `LPIPSStyle.load_weights()` is given the two files or a checkpoint carrying
  `loss.perceptual_loss.*` is loaded over them: "LPIPS-style", as BASELINE.json words it.
"""
import torch
import torch.nn as nn

from . import ops


def weights_init(m):
    classname = m.__class__.__name__
    if classname.find("Conv") != -1:
        nn.init.normal_(m.weight.data, 0.0, 0.02)
    elif classname.find("BatchNorm") != -1:
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0)


class Conv4x4(nn.Conv2d):
    """4x4 convolution parameter holder, forward through the HIP k x k kernel."""

    def __init__(self, cin, cout, stride, bias=True):
        super().__init__(cin, cout, kernel_size=4, stride=stride, padding=1, bias=bias)
        self.compute_dtype = torch.float32     # NLayerDiscriminator.set_precision
        self.fused_lrelu = None                # bf16 only: slope of the LeakyReLU that rides in this conv's epilogue

    def forward(self, x):
        if self.compute_dtype == torch.bfloat16:
            return ops.conv4x4_bf16(x, self.weight, self.bias, self.stride[0], lrelu=self.fused_lrelu)
        return ops.conv4x4(x, self.weight, self.bias, self.stride[0])


class BatchNormLReLU(nn.BatchNorm2d):
    """BatchNorm2d (batch statistics in training, running statistics in eval) fused with the LeakyReLU(0.2) that follows it in the
    PatchGAN.  `dist_group` = None: the statistics are this rank's own, as under the reference's default `sync_batchnorm: False`.
    A process group of more than one rank (set by Trainer(sync_batchnorm=True)): every training-mode forward takes mean and variance
    over all ranks' rows and the backward the two gradient sums, what torch.nn.SyncBatchNorm computes; the running estimates then
    hold the same bits on every rank.  The attribute is no parameter and no buffer: the state_dict does not change."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.dist_group = None          # set by the Trainer in a data-parallel run with sync_batchnorm

    def forward(self, x):
        return ops.batchnorm_lrelu(x, self, 0.2)


class ActNormLReLU(nn.Module):
    """[UPSTREAM] taming ActNorm (logdet=False, the discriminator's form) fused with the LeakyReLU(0.2) that follows it in the PatchGAN.
    State under the upstream names and shapes: loc, scale [1,C,1,1], initialized (uint8 scalar).

    Upstream reads `self.initialized.item()` on every forward: a device synchronisation per layer per call.  Here a host-side mirror of
    the flag decides, so the steady-state forward never reads the buffer; the mirror is refreshed where the buffer can change behind it
    (`_load_from_state_dict`, the data-parallel broadcast), one read each.

    DELIBERATE DEVIATION: upstream initialises per rank and the replicas then keep different loc / scale for the whole
    run.  When the Trainer has handed the layer a process group (`dist_group`), rank 0's values are broadcast right after initialising."""

    EPS = 1e-6

    def __init__(self, num_features, logdet=False, affine=True, allow_reverse_init=False):
        assert affine
        super().__init__()
        if logdet or allow_reverse_init:
            raise NotImplementedError("ActNorm logdet / reverse are not on the discriminator's path")
        self.logdet = logdet
        self.loc = nn.Parameter(torch.zeros(1, num_features, 1, 1))
        self.scale = nn.Parameter(torch.ones(1, num_features, 1, 1))
        self.register_buffer("initialized", torch.tensor(0, dtype=torch.uint8))
        self._initialized_host = False
        self.dist_group = None          # set by the Trainer in a data-parallel run

    def refresh_initialized(self):
        """Re-read the flag from the buffer (one device read): after anything that wrote the buffer behind the mirror."""
        self._initialized_host = bool(int(self.initialized.item()))
        return self._initialized_host

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        self.refresh_initialized()

    def initialize(self, x):
        """loc, scale from the statistics of `x`, on the device, without a graph and without a value coming back to the host"""
        ops.actnorm_init(x, self.loc, self.scale, self.EPS)
        with torch.no_grad():
            self.initialized.fill_(1)
        self._initialized_host = True
        if self.dist_group is not None:
            from .parallel import broadcast_actnorm
            broadcast_actnorm([self], self.dist_group)

    def forward(self, x, reverse=False):
        if reverse:
            raise NotImplementedError("ActNorm reverse is not on the discriminator's path")
        if self.training and not self._initialized_host:
            self.initialize(x)
        return ops.actnorm_lrelu(x, self, 0.2)


class LeakyReLU(nn.LeakyReLU):
    fused = False      # bf16 discriminator: applied in the epilogue of the conv in front (NLayerDiscriminator.set_precision)

    def forward(self, x):
        if self.fused:
            return x
        return ops.leaky_relu(x, self.negative_slope)


class _Fused(nn.Identity):
    """Placeholder keeping nn.Sequential indices equal to upstream where an activation was fused away."""


class NLayerDiscriminator(nn.Module):
    def __init__(self, input_nc=3, ndf=64, n_layers=3, use_actnorm=False):
        super().__init__()
        # [UPSTREAM]: BatchNorm2d and bias-free convolutions in front of it, or ActNorm and use_bias=True
        norm, use_bias = (ActNormLReLU, True) if use_actnorm else (BatchNormLReLU, False)
        seq = [Conv4x4(input_nc, ndf, 2, bias=True), LeakyReLU(0.2, True)]
        mult = 1
        for n in range(1, n_layers):
            prev, mult = mult, min(2 ** n, 8)
            seq += [Conv4x4(ndf * prev, ndf * mult, 2, bias=use_bias), norm(ndf * mult), _Fused()]
        prev, mult = mult, min(2 ** n_layers, 8)
        seq += [Conv4x4(ndf * prev, ndf * mult, 1, bias=use_bias), norm(ndf * mult), _Fused()]
        seq += [Conv4x4(ndf * mult, 1, 1, bias=True)]
        self.main = nn.Sequential(*seq)
        self.use_actnorm = bool(use_actnorm)
        self.compute_dtype = torch.float32     # see set_precision

    def forward(self, input):
        return self.main(input)

    def set_precision(self, precision):
        """32 (default) or "bf16": the 4x4 convolutions as implicit GEMMs on the bf16 MFMA kernels (no cols matrix), bf16 activations, the
        first layer's LeakyReLU in its conv's epilogue, BatchNorm + LeakyReLU on the bf16 kernels with f32 statistics, f32 logits -- what
        torch.autocast makes of the discriminator under the reference's `precision: bf16`.  The f32 image goes in and its f32 gradient
        comes out.  Parameters, buffers and the state_dict stay f32."""
        p = str(precision).lower()
        if p in ("32", "32-true", "fp32"):
            dt = torch.float32
        elif p in ("bf16", "bf16-mixed"):
            dt = torch.bfloat16
        else:
            raise ValueError("precision %r: the discriminator computes in 32 (f32) or bf16" % (precision,))
        if dt == torch.bfloat16 and self.use_actnorm:
            raise ValueError("precision %r with use_actnorm=True: there are no bf16 ActNorm + LeakyReLU kernels (only the BatchNorm "
                             "discriminator runs in bf16); keep this discriminator at 32" % (precision,))
        mods = list(self.main)
        for i, m in enumerate(mods):
            if isinstance(m, Conv4x4):
                nxt = mods[i + 1] if i + 1 < len(mods) else None
                fuse = dt == torch.bfloat16 and isinstance(nxt, LeakyReLU) and m.stride[0] == 2 and m.out_channels % 8 == 0
                m.compute_dtype = dt
                m.fused_lrelu = nxt.negative_slope if fuse else None
                if isinstance(nxt, LeakyReLU):
                    nxt.fused = fuse
        self.compute_dtype = dt
        return self

    def actnorm_layers(self):
        return [m for m in self.main if isinstance(m, ActNormLReLU)]

    def batchnorm_layers(self):
        """The BatchNorm layers (main.3/6/9; none under use_actnorm): what `sync_batchnorm` synchronises"""
        return [m for m in self.main if isinstance(m, BatchNormLReLU)]

    def actnorm_uninitialized(self):
        """True while an ActNorm layer still waits for its first training forward (host-side flags only)"""
        return any(not m._initialized_host for m in self.actnorm_layers())


class _VggConv(nn.Conv2d):
    def __init__(self, cin, cout):
        super().__init__(cin, cout, kernel_size=3, padding=1)

    def forward(self, x, mask_input=False, grad_premasked=False):
        """f32 or bf16 by the input's dtype; the two flags are the bf16 net's ReLU-mask wiring (ops.conv3x3_relu_bf16)"""
        if x.dtype == torch.bfloat16:
            return ops.conv3x3_relu_bf16(x, self.weight, self.bias, mask_input, grad_premasked)
        return ops.conv3x3(x, self.weight, self.bias, None, 0, relu=True)


# [UPSTREAM] taming/modules/losses/lpips.py `vgg16`: torchvision's vgg16().features split at the five taps
# relu1_2 / relu2_2 / relu3_3 / relu4_3 / relu5_3; each conv keeps its torchvision feature index as its module name
# (slice1 = features[0:4], slice2 = [4:9], slice3 = [9:16], slice4 = [16:23], slice5 = [23:30]; ReLU and MaxPool carry no
# parameters), so the keys read net.slice{k}.{idx}.{weight,bias}.
VGG16_SLICES = [
    ("slice1", [(0, 3, 64), (2, 64, 64)]),
    ("slice2", [(5, 64, 128), (7, 128, 128)]),
    ("slice3", [(10, 128, 256), (12, 256, 256), (14, 256, 256)]),
    ("slice4", [(17, 256, 512), (19, 512, 512), (21, 512, 512)]),
    ("slice5", [(24, 512, 512), (26, 512, 512), (28, 512, 512)]),
]
LPIPS_CHNS = [64, 128, 256, 512, 512]


class ScalingLayer(nn.Module):
    """[UPSTREAM] lpips.ScalingLayer: (x - shift) / scale with the two buffers in the state_dict."""

    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer("scale", torch.tensor([.458, .448, .450])[None, :, None, None])
        self.compute_dtype = torch.float32   # torch.bfloat16: hand the bf16 net its 8-channel bf16 image in the same pass

    def forward(self, x):
        return ops.scale_shift(x, self.shift, self.scale, out_dtype=self.compute_dtype)


class _Vgg16Features(nn.Module):
    def __init__(self):
        super().__init__()
        for name, convs in VGG16_SLICES:
            sl = nn.Module()
            for idx, cin, cout in convs:
                sl.add_module(str(idx), _VggConv(cin, cout))
            self.add_module(name, sl)

    def forward(self, h):
        outs = []
        for k, (name, convs) in enumerate(VGG16_SLICES):
            if k > 0:
                h = ops.maxpool2x2(h)     # features[4], [9], [16], [23] open slices 2..5
            sl = getattr(self, name)
            for idx, _, _ in convs:
                h = getattr(sl, str(idx))(h)   # conv + the ReLU that follows it (fused epilogue)
            outs.append(h)
        return outs


class NetLinLayer(nn.Module):
    """[UPSTREAM] lpips.NetLinLayer: Sequential(Dropout, Conv2d(chn_in, 1, 1, bias=False)) -> key lin{k}.model.1.weight.
    The Dropout holds the key index; it never drops anything here: LPIPSStyle pins itself to eval mode (see its `train`), and
    the 1x1 conv is folded into ops.lpips_layer_distance."""

    def __init__(self, chn_in, chn_out=1, use_dropout=True):
        super().__init__()
        layers = [nn.Dropout()] if use_dropout else []
        layers += [nn.Conv2d(chn_in, chn_out, 1, stride=1, padding=0, bias=False)]
        self.model = nn.Sequential(*layers)

    @property
    def weight(self):
        return self.model[-1].weight


class LPIPSStyle(nn.Module):
    """d(x, y) = sum_k mean_hw lin_k( (normalize(f_k(x)) - normalize(f_k(y)))^2 ), shape [B,1,1,1].

    Module tree = [UPSTREAM] taming LPIPS (`scaling_layer`, `net.slice{1..5}.{idx}`, `lin{0..4}.model.1`), so the
    `loss.perceptual_loss.*` entries of a reference checkpoint load with strict=True.  Construction fills seeded synthetic
    weights (the real ones are two downloads that do not exist offline); `load_weights` takes the two upstream files."""

    def __init__(self, seed=1234, use_dropout=True):
        super().__init__()
        self.scaling_layer = ScalingLayer()
        self.chns = list(LPIPS_CHNS)
        self.compute_dtype = torch.float32     # see set_precision
        self.net = _Vgg16Features()
        gen = torch.Generator().manual_seed(seed)
        with torch.no_grad():   # He-normal stand-in for the pretrained VGG16 weights (no network here)
            for name, convs in VGG16_SLICES:
                for idx, cin, cout in convs:
                    conv = getattr(getattr(self.net, name), str(idx))
                    conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * (2.0 / (9 * cin)) ** 0.5)
                    conv.bias.zero_()
        for k, chn in enumerate(self.chns):
            lin = NetLinLayer(chn, use_dropout=use_dropout)
            with torch.no_grad():
                lin.weight.copy_(torch.rand(lin.weight.shape, generator=gen) / chn)  # non-negative, like LPIPS lins
            self.add_module("lin%d" % k, lin)
        for p in self.parameters():
            p.requires_grad = False
        self._synthetic_mark = self._fingerprint()

    def train(self, mode=True):
        """DELIBERATE DEVIATION: the perceptual net stays in eval mode whatever the parent module is switched to.
        [UPSTREAM] builds it as `LPIPS().eval()` but defines no `train` override, so a Lightning fit's recursive `model.train()`
        re-arms the `Dropout(0.5)` in front of every lin layer and the reference's training-time LPIPS value is that of a random
        half of the feature channels, doubled -- an unbiased, noisy estimate of the eval-mode distance computed here (and by
        every LPIPS evaluation outside training).  The metric is frozen (`requires_grad = False`), so nothing else depends on
        the mode."""
        return super().train(False)

    # ---- weights ---------------------------------------------------------------------------------------------------------------
    def _fingerprint(self):
        with torch.no_grad():
            return (float(self.lin0.weight.double().sum()), float(self.net.slice1._modules["0"].weight.double().sum()))

    def has_synthetic_weights(self):
        """True while the construction-time stand-in weights are still in place (nothing was loaded over them)."""
        now = self._fingerprint()   # summation order differs between host and device: compare with a tolerance
        return all(abs(a - b) <= 1e-6 * max(1.0, abs(b)) for a, b in zip(now, self._synthetic_mark))

    def load_weights(self, vgg16=None, lins=None):
        """The two files [UPSTREAM] LPIPS.__init__ fetches: `vgg16` = torchvision vgg16 state_dict (keys features.{idx}.*;
        classifier.* ignored) and `lins` = taming's vgg.pth (keys lin{k}.model.1.weight).  Each may be a path or a dict.
        Raises KeyError / RuntimeError when a tensor is missing or has the wrong shape."""
        def _sd(x):
            return torch.load(x, map_location="cpu") if isinstance(x, (str, bytes)) or hasattr(x, "__fspath__") else x
        with torch.no_grad():
            if vgg16 is not None:
                sd = _sd(vgg16)
                for name, convs in VGG16_SLICES:
                    for idx, _, _ in convs:
                        conv = getattr(getattr(self.net, name), str(idx))
                        conv.weight.copy_(sd["features.%d.weight" % idx])
                        conv.bias.copy_(sd["features.%d.bias" % idx])
            if lins is not None:
                sd = _sd(lins)
                for k in range(len(self.chns)):
                    getattr(self, "lin%d" % k).weight.copy_(sd["lin%d.model.1.weight" % k])
        ops.PACK_CACHE.bump()
        return self

    def set_precision(self, precision):
        """32 (default) or "bf16": the 13 VGG layers on the bf16 MFMA conv kernels with the ReLU in their epilogue, bf16 features, the
        pools and the distance taps on the bf16 kernels of lpips_bf16.hip -- what torch.autocast makes of LPIPS under the reference's
        `precision: bf16`.  Parameters, buffers and the state_dict stay f32."""
        p = str(precision).lower()
        if p in ("32", "32-true", "fp32"):
            dt = torch.float32
        elif p in ("bf16", "bf16-mixed"):
            dt = torch.bfloat16
        else:
            raise ValueError("precision %r: the perceptual net computes in 32 (f32) or bf16" % (precision,))
        self.compute_dtype = dt
        self.scaling_layer.compute_dtype = dt
        return self

    def features(self, x):
        return self.net(self.scaling_layer(x))

    def _forward_bf16(self, input, target):
        """The bf16 net.  The input branch needs no gradient: nothing of it is saved and no data-gradient pack is built.  The target
        (reconstruction) branch is wired so that every ReLU's backward rides in the epilogue of the kernel that produces its incoming
        gradient (ops: "Where the ReLU masks go"): each layer runs with grad_premasked, each conv behind a conv masks its data gradient
        with its own input, each tap masks the sum of its own gradient and the one arriving from the next slice's pool."""
        if input.requires_grad:
            raise NotImplementedError("LPIPSStyle: gradient w.r.t. the first (input) branch is not on the OD-VAE path")
        with torch.no_grad():
            f0 = self.features(input)
        sl = self.scaling_layer
        if not target.requires_grad:
            f1 = self.features(target)
            ds = [ops.lpips_layer_distance(f0[k], f1[k], getattr(self, "lin%d" % k).weight) for k in range(len(self.chns))]
        else:
            ds, h, last = [], target, len(VGG16_SLICES) - 1
            for k, (name, convs) in enumerate(VGG16_SLICES):
                if k > 0:
                    h = ops.maxpool2x2(h)          # reads the tap's pass-through: the tap masks
                s = getattr(self.net, name)
                for j, (idx, _, _) in enumerate(convs):
                    conv = getattr(s, str(idx))
                    if k == 0 and j == 0:
                        h = ops.vgg_stem_bf16(h, sl.shift, sl.scale, conv.weight, conv.bias, grad_premasked=True)
                    else:
                        h = conv(h, mask_input=j > 0, grad_premasked=True)
                lin_w = getattr(self, "lin%d" % k).weight
                if k < last:
                    d, h = ops.lpips_tap_bf16(f0[k], h, lin_w, passthrough=True, relu_mask=True)
                else:
                    d = ops.lpips_tap_bf16(f0[k], h, lin_w, relu_mask=True)
                ds.append(d)
        total = ds[0]
        for d in ds[1:]:
            total = total + d
        return total.reshape(-1, 1, 1, 1)

    def forward(self, input, target):
        if self.compute_dtype == torch.bfloat16:
            return self._forward_bf16(input, target)
        f0, f1 = self.features(input), self.features(target)
        total = None
        for k in range(len(self.chns)):
            d = ops.lpips_layer_distance(f0[k], f1[k], getattr(self, "lin%d" % k).weight)  # [B]
            total = d if total is None else total + d
        return total.reshape(-1, 1, 1, 1)
