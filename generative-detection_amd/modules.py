"""Encoder / Decoder of the KL autoencoder, built from the HIP ops.

Module tree, parameter names, shapes and initialisation follow [UPSTREAM] CompVis latent-diffusion
ldm/modules/diffusionmodules/model.py (Encoder, Decoder, ResnetBlock, AttnBlock, Normalize, Upsample,
Downsample) as the reference subclasses them in src/modules/autoencodermodules/feat_encoder.py:4-6 and
feat_decoder.py:4-6, so a reference checkpoint's state_dict loads unchanged.
torch.nn.Conv2d / GroupNorm objects are used as parameter containers only (default init, OIHW weights);
their forward is never called -- all arithmetic goes through generative-detection_amd/ops/.
"""
import contextlib

import torch
import torch.nn as nn
import torch.utils.checkpoint

from . import ops


class Normalize(nn.GroupNorm):
    """GroupNorm(32 groups, eps 1e-6, affine); swish=True fuses nonlinearity(x) = x*sigmoid(x)."""

    def __init__(self, channels, num_groups=32):
        super().__init__(num_groups=num_groups, num_channels=channels, eps=1e-6, affine=True)

    def forward(self, x, swish=False, skip=False, drop_p=0.0, drop_seed=None):
        """skip=True also returns x for the block's skip connection; its gradient is then summed inside this node's
        backward pass (ops.group_norm_skip).  drop_p > 0 (not with skip): the ResnetBlock dropout on the result, its mask made
        from (drop_seed, element index, drop_p) inside the kernel (ops.group_norm)."""
        if skip:
            return ops.group_norm_skip(x, self.weight, self.bias, self.num_groups, self.eps, swish)
        if drop_p > 0.0:
            return ops.group_norm(x, self.weight, self.bias, self.num_groups, self.eps, swish, drop_p=drop_p, drop_seed=drop_seed)
        return ops.group_norm(x, self.weight, self.bias, self.num_groups, self.eps, swish)


class Conv3x3(nn.Conv2d):
    """3x3 convolution; mode 0 = stride 1 pad 1, 1 = Downsample form, 2 = Upsample form."""

    def __init__(self, cin, cout, mode=0):
        stride, pad = (2, 0) if mode == 1 else (1, 1)
        super().__init__(cin, cout, kernel_size=3, stride=stride, padding=pad)
        self.mode = mode

    def forward(self, x, residual=None, out_f32=False, gn_stats=False):
        """gn_stats=True: a Normalize() reads the result next -- where the kernel can, the conv's epilogue leaves the GroupNorm statistics
        with the tensor (ops.conv3x3) and that layer skips its statistics pass."""
        return ops.conv3x3(x, self.weight, self.bias, residual, self.mode, out_f32=out_f32, gn_stats=gn_stats)


class Conv1x1(nn.Conv2d):
    def __init__(self, cin, cout, bias=True):
        super().__init__(cin, cout, kernel_size=1, stride=1, padding=0, bias=bias)

    def forward(self, x, residual=None):
        return ops.conv1x1(x, self.weight, self.bias, residual)


class Upsample(nn.Module):
    def __init__(self, channels, with_conv=True):
        super().__init__()
        self.with_conv = with_conv
        if with_conv:
            self.conv = Conv3x3(channels, channels, mode=2)

    def forward(self, x):
        if not self.with_conv:      # (no parameters, as upstream) nearest 2x; the statistics of the result from the same pass
            return ops.upsample2x(x, gn_stats=True)
        # nearest 2x is folded into the conv's input gather; a ResnetBlock's norm1 reads the result: statistics from the conv's epilogue
        return self.conv(x, gn_stats=True)


class Downsample(nn.Module):
    def __init__(self, channels, with_conv=True):
        super().__init__()
        self.with_conv = with_conv
        if with_conv:
            self.conv = Conv3x3(channels, channels, mode=1)

    def forward(self, x):
        if not self.with_conv:      # F.avg_pool2d(x, 2, 2); a ResnetBlock's norm1 reads the result: statistics from the same pass
            return ops.avg_pool2x2(x, gn_stats=True)
        return self.conv(x)  # pad (0,1,0,1) + stride 2 inside the kernel


def _remake(module, a):
    """Saved-tensor hooks of the "norm" activation-checkpoint policy around the conv that consumes a = act(GroupNorm(.)): that conv keeps
    what re-makes `a` (the GroupNorm's input and statistics) instead of `a` (ops.remake_from_norm); a null context otherwise."""
    if getattr(module, "recompute_norm", False) and torch.is_grad_enabled() and a.requires_grad:
        return ops.remake_from_norm(a)
    return contextlib.nullcontext()


class ResnetBlock(nn.Module):
    def __init__(self, *, in_channels, out_channels=None, conv_shortcut=False, dropout=0.0, temb_channels=512):
        super().__init__()
        out_channels = in_channels if out_channels is None else out_channels
        if temb_channels > 0:
            raise NotImplementedError("timestep embedding is not part of the autoencoder path (temb_ch = 0)")
        self.in_channels, self.out_channels = in_channels, out_channels
        # whether a Normalize() reads this block's output (the next ResnetBlock's norm1, an AttnBlock's norm, norm_out): conv2 then
        # leaves the GroupNorm statistics with its result.  Encoder / Decoder clear it on the blocks in front of a Down / Upsample.
        self.gn_stats_out = True
        self.use_conv_shortcut = conv_shortcut
        self.norm1 = Normalize(in_channels)
        self.conv1 = Conv3x3(in_channels, out_channels)
        self.norm2 = Normalize(out_channels)
        # ddconfig.dropout.  nn.Dropout validates 0 <= p <= 1 (ValueError) and keeps the module tree / state_dict of the reference; its
        # forward is never called: in training with p > 0 norm2's kernels apply the mask (forward below)
        self.dropout = nn.Dropout(dropout)
        self.last_dropout_seed = None      # the seed of the latest training forward with dropout (tests, debugging; nothing reads it)
        self.conv2 = Conv3x3(out_channels, out_channels)
        if in_channels != out_channels:
            if conv_shortcut:
                self.conv_shortcut = Conv3x3(in_channels, out_channels)
            else:
                self.nin_shortcut = Conv1x1(in_channels, out_channels)

    recompute_norm = False      # "norm" activation-checkpoint policy (Decoder): the convs do not keep their normalised + activated inputs

    def forward(self, x, temb=None):
        h, x = self.norm1(x, swish=True, skip=True)
        with _remake(self, h):
            h1 = self.conv1(h, gn_stats=True)
        if self.training and self.dropout.p > 0:
            # conv2(dropout(swish(norm2(h)))): the seed comes from torch's default CPU generator (no device work, no sync), so
            # torch.manual_seed reproduces a run and torch.utils.checkpoint's restored generator state re-draws it in a recompute
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
            self.last_dropout_seed = seed
            h = self.norm2(h1, swish=True, drop_p=float(self.dropout.p), drop_seed=seed)
        else:
            h = self.norm2(h1, swish=True)
        del h1
        if self.in_channels != self.out_channels:
            x = self.conv_shortcut(x) if self.use_conv_shortcut else self.nin_shortcut(x)
        # x + h in the conv epilogue
        with _remake(self, h):
            return self.conv2(h, residual=x, gn_stats=self.gn_stats_out)


class AttnBlock(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.in_channels = in_channels
        self.norm = Normalize(in_channels)
        self.q = Conv1x1(in_channels, in_channels)
        self.k = Conv1x1(in_channels, in_channels)
        self.v = Conv1x1(in_channels, in_channels)
        self.proj_out = Conv1x1(in_channels, in_channels)

    recompute_norm = False

    def forward(self, x):
        h, x = self.norm(x, skip=True)
        # one [C -> 3C] projection instead of three reads of h
        w = torch.cat([self.q.weight, self.k.weight, self.v.weight], dim=0)
        b = torch.cat([self.q.bias, self.k.bias, self.v.bias], dim=0)
        with _remake(self, h):
            qkv = ops.conv1x1(h, w, b)
        del h
        o = ops.attention_qkv(qkv)
        return self.proj_out(o, residual=x)


class LinAttnBlock(nn.Module):
    """[UPSTREAM] LinAttnBlock(in_channels) = LinearAttention(dim=C, heads=1, dim_head=C): to_out(q ctx) with ctx = softmax(k over the
    tokens)^T v.  No GroupNorm, no residual add, no softmax over q, no C^-0.5 scale; state_dict: to_qkv.weight, to_out.weight, to_out.bias.
    Under compute_dtype = bfloat16 the two 1x1 convs run on the bf16 kernels; the projection leaves its conv in f32 (its f32-output
    form), the attention core runs in f32 (ops.linear_attention_qkv) and one ops.to_bf16 hands the result to to_out."""

    def __init__(self, in_channels):
        super().__init__()
        self.in_channels = in_channels
        self.to_qkv = Conv1x1(in_channels, 3 * in_channels, bias=False)
        self.to_out = Conv1x1(in_channels, in_channels)

    def forward(self, x):
        if x.dtype == torch.bfloat16:
            qkv = ops.conv1x1(x, self.to_qkv.weight, None, out_f32=True)
            return self.to_out(ops.to_bf16(ops.linear_attention_qkv(qkv)))
        return self.to_out(ops.linear_attention_qkv(self.to_qkv(x)))


def make_attn(in_channels, attn_type="vanilla"):
    if attn_type == "none":
        return nn.Identity()
    if attn_type == "linear":
        return LinAttnBlock(in_channels)
    if attn_type != "vanilla":
        raise NotImplementedError("attn_type %r: 'vanilla', 'linear' and 'none' are on the OD-VAE path" % attn_type)
    return AttnBlock(in_channels)


class Encoder(nn.Module):
    def __init__(self, *, ch, out_ch, ch_mult=(1, 2, 4, 8), num_res_blocks, attn_resolutions, dropout=0.0,
                 resamp_with_conv=True, in_channels, resolution, z_channels, double_z=True, use_linear_attn=False,
                 attn_type="vanilla", **ignore_kwargs):
        super().__init__()
        if use_linear_attn:
            attn_type = "linear"
        self.ch, self.temb_ch = ch, 0
        self.num_resolutions = len(ch_mult)
        self.num_res_blocks = num_res_blocks
        self.resolution, self.in_channels = resolution, in_channels
        # torch.float32, or torch.bfloat16 = the trainer's `precision: bf16` (configs[4]): bf16 activations, f32 master weights
        self.compute_dtype = torch.float32
        self.conv_in = Conv3x3(in_channels, ch)
        curr_res = resolution
        widths = [ch * m for m in (1,) + tuple(ch_mult)]
        self.in_ch_mult = (1,) + tuple(ch_mult)
        self.down = nn.ModuleList()
        block_in = ch
        for level in range(self.num_resolutions):
            block_in, block_out = widths[level], widths[level + 1]
            stage = nn.Module()
            stage.block, stage.attn = nn.ModuleList(), nn.ModuleList()
            for _ in range(num_res_blocks):
                stage.block.append(ResnetBlock(in_channels=block_in, out_channels=block_out,
                                               temb_channels=self.temb_ch, dropout=dropout))
                block_in = block_out
                if curr_res in attn_resolutions:
                    stage.attn.append(make_attn(block_in, attn_type))
            if level != self.num_resolutions - 1:
                stage.downsample = Downsample(block_in, resamp_with_conv)
                if len(stage.attn) == 0:
                    stage.block[-1].gn_stats_out = False      # its output feeds the Downsample conv, not a Normalize
                curr_res //= 2
            self.down.append(stage)
        self.mid = nn.Module()
        self.mid.block_1 = ResnetBlock(in_channels=block_in, out_channels=block_in, temb_channels=self.temb_ch, dropout=dropout)
        self.mid.attn_1 = make_attn(block_in, attn_type)
        self.mid.block_2 = ResnetBlock(in_channels=block_in, out_channels=block_in, temb_channels=self.temb_ch, dropout=dropout)
        self.norm_out = Normalize(block_in)
        self.conv_out = Conv3x3(block_in, 2 * z_channels if double_z else z_channels)

    def forward(self, x):
        if self.compute_dtype == torch.bfloat16:
            x = ops.to_bf16(x, pad_channels_to=8)   # 3-channel image -> 16-byte channel vectors (the extra channels are zero)
        h = self.conv_in(x)
        for level, stage in enumerate(self.down):
            for i, block in enumerate(stage.block):
                h = block(h)
                if len(stage.attn) > 0:
                    h = stage.attn[i](h)
            if level != self.num_resolutions - 1:
                h = stage.downsample(h)
        h = self.mid.block_2(self.mid.attn_1(self.mid.block_1(h)))
        return self.conv_out(self.norm_out(h, swish=True), out_f32=True)   # the moments leave the encoder in f32


class Decoder(nn.Module):
    def __init__(self, *, ch, out_ch, ch_mult=(1, 2, 4, 8), num_res_blocks, attn_resolutions, dropout=0.0,
                 resamp_with_conv=True, in_channels, resolution, z_channels, give_pre_end=False, tanh_out=False,
                 use_linear_attn=False, attn_type="vanilla", activation_checkpoint=False, **ignorekwargs):
        super().__init__()
        # activation_checkpoint (not an upstream key; upstream swallows unknown keys through **ignorekwargs): True / "unit" = keep only
        # the input of each ResnetBlock(+AttnBlock) unit and recompute its interior in backward -- torch.utils.checkpoint per unit
        # (BASELINE.json config 5; what bench.py --ckpt-decoder measures).  "norm" = keep the conv outputs, drop only the normalised +
        # activated tensors between a Normalize and the conv that reads it, and re-make them with one GroupNorm apply pass in the
        # backward (ops.remake_from_norm): half of the decoder's activation memory for ~2 % of its work instead of all of it for ~1/3.
        self.activation_checkpoint = activation_checkpoint if activation_checkpoint in ("unit", "norm") else bool(activation_checkpoint)
        self.compute_dtype = torch.float32   # see Encoder
        if use_linear_attn:
            attn_type = "linear"
        self.ch, self.temb_ch = ch, 0
        self.num_resolutions = len(ch_mult)
        self.num_res_blocks = num_res_blocks
        self.resolution, self.in_channels = resolution, in_channels
        self.give_pre_end, self.tanh_out = give_pre_end, tanh_out
        block_in = ch * ch_mult[-1]
        curr_res = resolution // 2 ** (self.num_resolutions - 1)
        self.z_shape = (1, z_channels, curr_res, curr_res)
        self.conv_in = Conv3x3(z_channels, block_in)
        self.mid = nn.Module()
        self.mid.block_1 = ResnetBlock(in_channels=block_in, out_channels=block_in, temb_channels=self.temb_ch, dropout=dropout)
        self.mid.attn_1 = make_attn(block_in, attn_type)
        self.mid.block_2 = ResnetBlock(in_channels=block_in, out_channels=block_in, temb_channels=self.temb_ch, dropout=dropout)
        stages = []
        for level in reversed(range(self.num_resolutions)):
            block_out = ch * ch_mult[level]
            stage = nn.Module()
            stage.block, stage.attn = nn.ModuleList(), nn.ModuleList()
            for _ in range(num_res_blocks + 1):
                stage.block.append(ResnetBlock(in_channels=block_in, out_channels=block_out,
                                               temb_channels=self.temb_ch, dropout=dropout))
                block_in = block_out
                if curr_res in attn_resolutions:
                    stage.attn.append(make_attn(block_in, attn_type))
            if level != 0:
                stage.upsample = Upsample(block_in, resamp_with_conv)
                if len(stage.attn) == 0:
                    stage.block[-1].gn_stats_out = False      # its output feeds the Upsample conv, not a Normalize
                curr_res *= 2
            stages.insert(0, stage)  # index == resolution level, as upstream
        self.up = nn.ModuleList(stages)
        self.norm_out = Normalize(block_in)
        self.conv_out = Conv3x3(block_in, out_ch)

    def forward(self, z):
        self.last_z_shape = z.shape
        if self.compute_dtype == torch.bfloat16 and z.shape[1] % 8 == 0:
            z = ops.to_bf16(z)
        h = self.conv_in(z)
        if self.compute_dtype == torch.bfloat16:
            # a latent whose channel count is no multiple of 8 (kl-f4: 3, this repository's small test geometry: 4) cannot enter the bf16 kernels
            # (16-byte channel vectors, and the encoder needs the gradient of every latent channel back): conv_in then reads it in f32 and its
            # output is handed to the bf16 network.  (to_bf16 returns a bf16 tensor as it is.)
            h = ops.to_bf16(h)
        norm_policy = self.activation_checkpoint == "norm"
        for m in self.modules():
            if isinstance(m, (ResnetBlock, AttnBlock)):      # (a LinAttnBlock has no norm to re-make)
                m.recompute_norm = norm_policy
        recompute = bool(self.activation_checkpoint) and not norm_policy and torch.is_grad_enabled() and h.requires_grad
        def ckpt(f, t):      # (no GroupNorm-backward links inside a checkpointed unit: ops.GN_FUSED_BWD_SUSPENDED)
            with ops.gn_fused_bwd_suspended():
                return torch.utils.checkpoint.checkpoint(f, t, use_reentrant=False)
        run = ckpt if recompute else (lambda f, t: f(t))
        # With the fused (bf16) attention an AttnBlock keeps only qkv, o and one f32 per row for its backward, so it stays OUTSIDE
        # the recomputed units: re-running the T x T products would cost far more than those tensors (3 of 8 attention forwards
        # per step at configs[4]).  The f32 path materialises P ([N, T, T]) and keeps attention inside the unit.
        attn_outside = recompute and self.compute_dtype == torch.bfloat16
        if attn_outside:
            h = run(self.mid.block_2, self.mid.attn_1(run(self.mid.block_1, h)))
        else:
            h = run(lambda t: self.mid.block_2(self.mid.attn_1(self.mid.block_1(t))), h)
        for level in reversed(range(self.num_resolutions)):
            stage = self.up[level]
            for i, block in enumerate(stage.block):
                if len(stage.attn) > 0 and attn_outside:
                    h = stage.attn[i](run(block, h))
                    continue
                unit = (lambda t, b=block, a=stage.attn[i]: a(b(t))) if len(stage.attn) > 0 else block
                h = run(unit, h)
            if level != 0:
                h = stage.upsample(h)
        if self.give_pre_end:
            return h
        h = self.norm_out(h, swish=True)
        self.recompute_norm = norm_policy
        with _remake(self, h):
            h = self.conv_out(h, out_f32=True)   # the reconstruction (and the losses on it) stay f32
        return ops.tanh(h) if self.tanh_out else h
