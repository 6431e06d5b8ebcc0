"""PatchGAN discriminator pieces: the 4x4 conv (f32: gan_f32.hip; bf16: conv_bf16.hip), BatchNorm+LeakyReLU and ActNorm (gan_norm.hip),
LeakyReLU, the scalar terms of the GAN losses over the logits (gan_f32.hip)."""
import weakref

import torch
from torch.autograd import Function

from .. import ops as _ops      # the package: switches and run-time state are read and written there (ops/__init__.py)
from .. import lib as _lib
from ._base import BF16, KERNEL_EVENTS, _L, _cl, _new_cl, _ws
from .packs import pack_conv3x3
from .gemm import _colsum, gemm
from .conv_bf16 import _pad8, cast_pad_bf16


# ------------------------------------------------------------------------------------------------------
# PatchGAN discriminator pieces (gan_f32.hip, gan_norm.hip)
# ------------------------------------------------------------------------------------------------------
def _conv4x4_out(h, stride):
    return (h + 2 - 4) // stride + 1


class _Conv4x4(Function):
    """Conv2d(k=4, pad=1, stride 1|2) = im2col + MFMA GEMM; weight OIHW [Cout][Cin][4][4]."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride):
        L = _L()
        x = _cl(x)
        n, cin, hi, wi = x.shape
        cout = weight.shape[0]
        ho, wo = _conv4x4_out(hi, stride), _conv4x4_out(wi, stride)
        m, k = n * ho * wo, 16 * cin
        st = _lib.stream_ptr()
        wg = torch.empty(cout, k, dtype=torch.float32, device=x.device)
        _lib.check(L.odvae_weight4x4_reorder_f32(weight.detach().contiguous().data_ptr(), wg.data_ptr(), cout, cin, 1, st), "weight4x4_reorder")
        cols = torch.empty(m, k, dtype=torch.float32, device=x.device)
        _lib.check(L.odvae_im2col4x4_f32(x.data_ptr(), cols.data_ptr(), n, hi, wi, cin, ho, wo, stride, st), "im2col4x4")
        y = _new_cl(n, cout, ho, wo, x)
        b = bias.detach().contiguous() if bias is not None else None
        gemm(0, 1, m, cout, k, 1.0, cols, k, 0, wg, k, 0, y, cout, 0, b)
        ctx.stride, ctx.has_bias, ctx.xshape = stride, bias is not None, (n, cin, hi, wi)
        ctx.save_for_backward(cols, wg)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _L()
        cols, wg = ctx.saved_tensors
        dy = _cl(dy)
        n, cin, hi, wi = ctx.xshape
        _, cout, ho, wo = dy.shape
        m, k = n * ho * wo, 16 * cin
        st = _lib.stream_ptr()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dcols = torch.empty(m, k, dtype=torch.float32, device=dy.device)
            gemm(0, 0, m, k, cout, 1.0, dy, cout, 0, wg, k, 0, dcols, k, 0)
            dx = _new_cl(n, cin, hi, wi, dy)
            _lib.check(L.odvae_col2im4x4_f32(dcols.data_ptr(), dx.data_ptr(), n, hi, wi, cin, ho, wo, ctx.stride, st), "col2im4x4")
        if ctx.needs_input_grad[1]:
            dwg = torch.empty(cout, k, dtype=torch.float32, device=dy.device)
            gemm(1, 0, cout, k, m, 1.0, dy, cout, 0, cols, k, 0, dwg, k, 0)
            dw = torch.empty(cout, cin, 4, 4, dtype=torch.float32, device=dy.device)
            _lib.check(L.odvae_weight4x4_reorder_f32(dwg.data_ptr(), dw.data_ptr(), cout, cin, 0, st), "weight4x4_reorder")
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = _colsum(dy, m, cout)
        return dx, dw, db, None


def _conv4x4_i_raw(stride, dgrad, x, pack, cout, bias, ho, wo):
    """One odvae_conv4x4_f32 call: x f32 [N, C, H, W] -> [N, cout, ho, wo]"""
    L = _L()
    n, cx, hi, wi = x.shape
    y = _new_cl(n, cout, ho, wo, x)
    tag = KERNEL_EVENTS.begin(secondary=True)
    _lib.check(L.odvae_conv4x4_f32(stride, int(dgrad), x.data_ptr(), n, hi, wi, cx, pack.data_ptr(), cout, _lib.ptr(bias), y.data_ptr(),
                                   ho, wo, _lib.stream_ptr()), "conv4x4_f32(stride=%d, dgrad=%d)" % (stride, dgrad))
    px = (hi * wi) if dgrad else (ho * wo)      # 16 taps per pixel of the conv's OUTPUT, forward and transposed alike
    KERNEL_EVENTS.end("conv4x4_f32", 2.0 * 16 * cx * cout * n * px, tag,
                      4.0 * n * hi * wi * cx + 4.0 * n * ho * wo * cout + 4.0 * 16 * cx * cout)
    return y


def _check_pack_current(ctx, op):
    """The data-gradient pack a 4x4 conv's forward cached (ctx.dpack) is keyed by its weight's tag: refuse a backward after the weight was written"""
    wnow = ctx.wref()
    if wnow is None or _ops.PACK_CACHE.weight_tag(wnow) != ctx.pack_tag:
        raise RuntimeError("%s backward: the weight was updated between this graph's forward and its backward; the "
                           "cached data-gradient pack now holds the new weights" % op)


class _Conv4x4I(Function):
    """Conv2d(k=4, pad=1, stride 1|2) as an implicit GEMM in exact f32 (opt-in: ops.DISC_F32_IMPLICIT; conv3x3_f32.hip modes 6 - 9,
    conv4x4_wgrad_f32.hip).  No cols matrix: what is saved is the input, which is the previous layer's output anyway.  Any Cout
    (the logit head needs no padding round trip).  weight OIHW [Cout][Cin][4][4]."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride):
        x = _cl(x)
        n, cin, hi, wi = x.shape
        cout = weight.shape[0]
        ho, wo = _conv4x4_out(hi, stride), _conv4x4_out(wi, stride)
        need_dx = bool(ctx.needs_input_grad[0])
        # tagged per weight, as "bf16v": the three discriminator forwards of a GAN batch and the generator's optimizer step between
        # them read one pack; the data-gradient pack's tap order depends on the stride, hence one kind per stride
        fwd_pack, dpack = pack_conv3x3(weight, True, need_dx, "c4x4s%d" % stride)
        b = bias.detach().contiguous() if bias is not None else None
        y = _conv4x4_i_raw(stride, False, x, fwd_pack, cout, b, ho, wo)
        ctx.stride, ctx.has_bias, ctx.dpack = stride, bias is not None, dpack
        ctx.pack_tag, ctx.wref = _ops.PACK_CACHE.weight_tag(weight), weakref.ref(weight)
        ctx.wshape = tuple(weight.shape)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _L()
        (x,) = ctx.saved_tensors
        dy = _cl(dy)
        cout, cin = ctx.wshape[0], ctx.wshape[1]
        n, _, hi, wi = x.shape
        _, _, ho, wo = dy.shape
        stride = ctx.stride
        dx = dw = db = None
        if ctx.needs_input_grad[0] and not _ops.WEIGHT_GRADIENT_ONLY:
            _check_pack_current(ctx, "conv4x4")
            dx = _conv4x4_i_raw(stride, True, dy, ctx.dpack, cin, None, hi, wi)
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            dw = torch.empty((cout, cin, 4, 4), dtype=torch.float32, device=x.device)
            if want_db:
                db = torch.empty(cout, dtype=torch.float32, device=x.device)
            wp, wn = _ws(L.odvae_conv4x4_wgrad_workspace_bytes(stride, n, ho, wo, cin, cout), x)
            tag = KERNEL_EVENTS.begin(secondary=True)
            _lib.check(L.odvae_conv4x4_wgrad_f32(stride, x.data_ptr(), dy.data_ptr(), n, hi, wi, cin, ho, wo, cout, dw.data_ptr(), _lib.ptr(db),
                                                 wp, wn, _lib.stream_ptr()), "conv4x4_wgrad_f32(stride=%d)" % stride)
            KERNEL_EVENTS.end("conv4x4_wgrad_f32", 2.0 * 16 * cin * cout * n * ho * wo, tag, 4.0 * n * (hi * wi * cin + ho * wo * cout))
        elif want_db:
            db = _colsum(dy, n * ho * wo, cout)
        return dx, dw, db, None


def conv4x4(x, weight, bias, stride):
    """PatchGAN convolution.  Cout = 1 (the logit head) is zero-padded to 4 output channels for the GEMM's
    float4 staging and sliced back (torch cat/slice on [4,C,4,4] / [B,4,30,30]-sized tensors).
    An input under 2 pixels high or wide is refused here, as torch refuses it (the padded image is smaller than the kernel).
    With ops.DISC_F32_IMPLICIT on, shapes odvae_conv4x4_f32_supported takes run as an implicit GEMM instead (_Conv4x4I)."""
    if stride not in (1, 2):
        raise ValueError("conv4x4: stride must be 1 or 2, got %r" % (stride,))
    if x.dim() != 4 or x.shape[2] < 2 or x.shape[3] < 2:
        raise ValueError("conv4x4: needs an [N, C, H, W] input with H, W >= 2 (kernel 4, padding 1), got %s" % (tuple(x.shape),))
    if tuple(weight.shape[1:]) != (x.shape[1], 4, 4):
        raise ValueError("conv4x4: weight %s does not fit an input with %d channels" % (tuple(weight.shape), x.shape[1]))
    cout = weight.shape[0]
    if _ops.DISC_F32_IMPLICIT and _L().odvae_conv4x4_f32_supported(int(stride), x.shape[0], x.shape[2], x.shape[3], x.shape[1], cout):
        return _Conv4x4I.apply(x, weight, bias, int(stride))
    if cout % 4 == 0:
        return _Conv4x4.apply(x, weight, bias, stride)
    pad = 4 - cout % 4
    wp = torch.cat([weight, weight.new_zeros((pad,) + tuple(weight.shape[1:]))], dim=0)
    bp = torch.cat([bias, bias.new_zeros(pad)]) if bias is not None else None
    return _Conv4x4.apply(x, wp, bp, stride)[:, :cout]


class _BatchNormLReLU(Function):
    """BatchNorm2d + LeakyReLU on f32 or bf16 activations (x, y, dy, dx in x's dtype); statistics, running estimates and parameter
    gradients f32 either way (gan_norm.hip)"""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, slope, train):
        L = _L()
        bf = x.dtype == BF16
        dt = BF16 if bf else torch.float32
        x = _cl(x, dt)
        n, c, h, w = x.shape
        rows = n * h * w
        y = _new_cl(n, c, h, w, x, dtype=dt)
        if train:
            mean = torch.empty(c, dtype=torch.float32, device=x.device)
            rstd = torch.empty(c, dtype=torch.float32, device=x.device)
        else:  # eval: running estimates (tiny [C] torch ops)
            mean = running_mean.detach().clone()
            rstd = torch.rsqrt(running_var.detach() + eps)
        wp, wn = _ws(L.odvae_batchnorm_workspace_bytes(rows, c), x)
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        _lib.check(getattr(L, "odvae_batchnorm_lrelu_fwd_" + ("bf16" if bf else "f32"))(x.data_ptr(), rows, c, g.data_ptr(), b.data_ptr(), float(eps), float(momentum),
                                                                   float(slope), int(train), mean.data_ptr(), rstd.data_ptr(),
                                                                   _lib.ptr(running_mean) if train else None,
                                                                   _lib.ptr(running_var) if train else None, y.data_ptr(), wp, wn,
                                                                   _lib.stream_ptr()), "batchnorm_lrelu_fwd" + ("_bf16" if bf else ""))
        ctx.slope, ctx.train = float(slope), int(train)
        ctx.save_for_backward(x, gamma, beta, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _L()
        x, gamma, beta, mean, rstd = ctx.saved_tensors
        bf = x.dtype == BF16
        dy = _cl(dy, x.dtype)
        n, c, h, w = x.shape
        rows = n * h * w
        dx = _new_cl(n, c, h, w, x, dtype=x.dtype)
        dg = torch.empty(c, dtype=torch.float32, device=x.device)
        db = torch.empty(c, dtype=torch.float32, device=x.device)
        wp, wn = _ws(L.odvae_batchnorm_workspace_bytes(rows, c), x)
        _lib.check(getattr(L, "odvae_batchnorm_lrelu_bwd_" + ("bf16" if bf else "f32"))(x.data_ptr(), dy.data_ptr(), rows, c, gamma.detach().contiguous().data_ptr(),
                                                                       beta.detach().contiguous().data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                                                       ctx.slope, ctx.train, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), wp, wn,
                                                                       _lib.stream_ptr()), "batchnorm_lrelu_bwd" + ("_bf16" if bf else ""))
        return dx, dg, db, None, None, None, None, None, None


def _gather_f64(local, group, world):
    """[world, *local.shape]: every rank's `local` (f64, device), rank-major, the same bits on every rank.  A zero-filled tensor in
    which the rank fills its own slot, summed over the group: adding zeros is exact, so this is an all-gather that runs on gloo (which
    has no all_gather of device tensors) and on nccl alike, and on nccl it stays on the stream (no host synchronisation)."""
    import torch.distributed as dist
    buf = torch.zeros((world,) + tuple(local.shape), dtype=torch.float64, device=local.device)
    buf[dist.get_rank(group)].copy_(local)
    dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
    return buf


class _SyncBatchNormLReLU(Function):
    """Training-mode BatchNorm + LeakyReLU with the statistics of all ranks of `group` (torch.nn.SyncBatchNorm: BatchNorm2d on the
    concatenated batch), f32 or bf16 activations.  Forward: local record -> one exchange -> merge (mean, rstd, running estimates, the
    same bits on every rank) -> the eval-form apply.  Backward: local sums -> one exchange -> dx; dgamma, dbeta stay the local sums (the
    gradient all-reduce adds them like every other parameter gradient)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, slope, group, world):
        L = _L()
        bf = x.dtype == BF16
        sfx = "bf16" if bf else "f32"
        x = _cl(x, BF16) if bf else _cl(x)
        n, c, h, w = x.shape
        rows = n * h * w
        dev = x.device
        st = _lib.stream_ptr()
        wp, wn = _ws(L.odvae_batchnorm_workspace_bytes(rows, c), x)
        record = torch.empty(c, 3, dtype=torch.float64, device=dev)
        _lib.check(getattr(L, "odvae_batchnorm_sync_stats_record_" + sfx)(x.data_ptr(), rows, c, record.data_ptr(), record.numel() * 8, wp, wn, st),
                   "batchnorm_sync_stats_record_" + sfx)
        records = _gather_f64(record, group, world)
        mean = torch.empty(c, dtype=torch.float32, device=dev)
        rstd = torch.empty(c, dtype=torch.float32, device=dev)
        total = torch.empty(1, dtype=torch.float64, device=dev)
        _lib.check(L.odvae_batchnorm_sync_stats_merge(records.data_ptr(), records.numel() * 8, world, c, float(eps), float(momentum),
                                                      mean.data_ptr(), rstd.data_ptr(), _lib.ptr(running_mean), _lib.ptr(running_var),
                                                      total.data_ptr(), st), "batchnorm_sync_stats_merge")
        y = _new_cl(n, c, h, w, x, dtype=BF16 if bf else torch.float32)
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        _lib.check(getattr(L, "odvae_batchnorm_lrelu_fwd_" + sfx)(x.data_ptr(), rows, c, g.data_ptr(), b.data_ptr(), float(eps), float(momentum),
                                                                   float(slope), 0, mean.data_ptr(), rstd.data_ptr(), None, None,
                                                                   y.data_ptr(), None, 0, st), "batchnorm_lrelu_fwd_" + sfx)
        ctx.slope, ctx.group, ctx.world, ctx.total, ctx.sfx = float(slope), group, world, total, sfx
        ctx.save_for_backward(x, gamma, beta, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _L()
        x, gamma, beta, mean, rstd = ctx.saved_tensors
        sfx, world = ctx.sfx, ctx.world
        bf = sfx == "bf16"
        dy = _cl(dy, BF16) if bf else _cl(dy)
        n, c, h, w = x.shape
        rows = n * h * w
        dev = x.device
        st = _lib.stream_ptr()
        g, b = gamma.detach().contiguous(), beta.detach().contiguous()
        dg = torch.empty(c, dtype=torch.float32, device=dev)
        db = torch.empty(c, dtype=torch.float32, device=dev)
        sums = torch.empty(2, c, dtype=torch.float64, device=dev)
        wp, wn = _ws(L.odvae_batchnorm_workspace_bytes(rows, c), x)
        _lib.check(getattr(L, "odvae_batchnorm_sync_bwd_sums_" + sfx)(x.data_ptr(), dy.data_ptr(), rows, c, g.data_ptr(), b.data_ptr(),
                                                                       mean.data_ptr(), rstd.data_ptr(), ctx.slope, sums.data_ptr(), sums.numel() * 8,
                                                                       dg.data_ptr(), db.data_ptr(), wp, wn, st), "batchnorm_sync_bwd_sums_" + sfx)
        sums_all = _gather_f64(sums, ctx.group, world)
        dx = _new_cl(n, c, h, w, x, dtype=BF16 if bf else torch.float32)
        _lib.check(getattr(L, "odvae_batchnorm_sync_bwd_dx_" + sfx)(x.data_ptr(), dy.data_ptr(), rows, c, g.data_ptr(), b.data_ptr(),
                                                                     mean.data_ptr(), rstd.data_ptr(), ctx.slope, sums_all.data_ptr(),
                                                                     sums_all.numel() * 8, world, ctx.total.data_ptr(), dx.data_ptr(), wp, wn, st),
                   "batchnorm_sync_bwd_dx_" + sfx)
        return dx, dg, db, None, None, None, None, None, None, None


def _sync_group(bn):
    """(group, world) when `bn` is to take its training statistics over a process group of more than one rank, else (None, 1):
    torch.nn.SyncBatchNorm's own condition -- a training-mode module with a group; eval never exchanges anything."""
    group = getattr(bn, "dist_group", None)
    if group is None or not bn.training:
        return None, 1
    world = torch.distributed.get_world_size(group)
    return (group, world) if world > 1 else (None, 1)


def batchnorm_lrelu(x, bn, slope):
    """BatchNorm2d `bn` (parameter/buffer holder) + LeakyReLU(slope); updates running stats in training mode.  With `bn.dist_group` a
    process group of more than one rank, the training statistics are those of all its ranks' rows (_SyncBatchNormLReLU)."""
    train = bn.training or not bn.track_running_stats
    if train and bn.track_running_stats and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    momentum = 0.1 if bn.momentum is None else bn.momentum
    group, world = _sync_group(bn)
    if group is not None:
        return _SyncBatchNormLReLU.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, momentum, slope, group, world)
    return _BatchNormLReLU.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, momentum, slope, train)


class _ActNormLReLU(Function):
    @staticmethod
    def forward(ctx, x, loc, scale, slope):
        L = _L()
        x = _cl(x)
        _lib.require_device(loc, scale)
        n, c, h, w = x.shape
        y = _new_cl(n, c, h, w, x)
        _lib.check(L.odvae_actnorm_lrelu_fwd_f32(x.data_ptr(), n * h * w, c, loc.detach().contiguous().data_ptr(),
                                                 scale.detach().contiguous().data_ptr(), float(slope), y.data_ptr(), _lib.stream_ptr()),
                   "actnorm_lrelu_fwd")
        ctx.slope = float(slope)
        ctx.save_for_backward(x, loc, scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _L()
        x, loc, scale = ctx.saved_tensors
        dy = _cl(dy)
        n, c, h, w = x.shape
        rows = n * h * w
        dx = _new_cl(n, c, h, w, x)
        dloc = dscale = None
        wp, wn = None, 0
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:   # neither: the dx-only kernel, no partial sums
            dloc = torch.empty(1, c, 1, 1, dtype=torch.float32, device=x.device)
            dscale = torch.empty(1, c, 1, 1, dtype=torch.float32, device=x.device)
            wp, wn = _ws(L.odvae_actnorm_workspace_bytes(rows, c), x)
        _lib.check(L.odvae_actnorm_lrelu_bwd_f32(x.data_ptr(), dy.data_ptr(), rows, c, loc.detach().contiguous().data_ptr(),
                                                 scale.detach().contiguous().data_ptr(), ctx.slope, dx.data_ptr(), _lib.ptr(dloc),
                                                 _lib.ptr(dscale), wp, wn, _lib.stream_ptr()), "actnorm_lrelu_bwd")
        return dx, dloc, dscale, None


def actnorm_init(x, loc, scale, eps=1e-6):
    """ActNorm's data-dependent initialisation: loc = -mean_c(x), scale = 1 / (std_c(x) + eps), unbiased std over N*H*W, written into
    the two parameters' storage on the device (no graph, nothing comes back to the host).  Needs N*H*W >= 2."""
    L = _L()
    x = _cl(x.detach())
    _lib.require_device(loc, scale)
    n, c, h, w = x.shape
    if loc.numel() != c or scale.numel() != c or not (loc.is_contiguous() and scale.is_contiguous()):
        raise ValueError("actnorm_init: loc / scale must be contiguous with %d elements" % c)
    rows = n * h * w
    wp, wn = _ws(L.odvae_actnorm_workspace_bytes(rows, c), x)
    _lib.check(L.odvae_actnorm_init_f32(x.data_ptr(), rows, c, float(eps), loc.data_ptr(), scale.data_ptr(), wp, wn, _lib.stream_ptr()),
               "actnorm_init")


def actnorm_lrelu(x, an, slope):
    """ActNorm `an` (holder of loc, scale [1,C,1,1]) + LeakyReLU(slope): lrelu(scale * (x + loc)); gradients dx, dloc, dscale."""
    return _ActNormLReLU.apply(x, an.loc, an.scale, slope)


class _LeakyReLU(Function):
    @staticmethod
    def forward(ctx, x, slope):
        L = _L()
        x = _cl(x)
        y = _new_cl(*x.shape, x)
        _lib.check(L.odvae_leaky_relu_f32(x.data_ptr(), y.data_ptr(), float(slope), x.numel(), _lib.stream_ptr()), "leaky_relu")
        ctx.slope = float(slope)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _L()
        (x,) = ctx.saved_tensors
        dy = _cl(dy)
        dx = _new_cl(*x.shape, x)
        _lib.check(L.odvae_leaky_relu_bwd_f32(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), ctx.slope, x.numel(), _lib.stream_ptr()),
                   "leaky_relu_bwd")
        return dx, None


def leaky_relu(x, slope):
    return _LeakyReLU.apply(x, slope)


class _GanLogitTerms(Function):
    """The six scalar terms of the GAN losses over the discriminator's logits, one launch pair forward and one launch backward."""

    @staticmethod
    def forward(ctx, real, fake):
        L = _L()
        _lib.require_device(real, fake)
        fake_c = fake.detach().contiguous()
        real_c = None if real is None else real.detach().contiguous()
        n_real = 0 if real_c is None else real_c.numel()
        out = torch.empty(6, dtype=torch.float32, device=fake.device)
        wp, wn = _ws(L.odvae_gan_logit_terms_workspace_bytes(n_real, fake_c.numel()), fake)
        _lib.check(L.odvae_gan_logit_terms_f32(_lib.ptr(real_c), n_real, fake_c.data_ptr(), fake_c.numel(), out.data_ptr(), wp, wn,
                                               _lib.stream_ptr()), "gan_logit_terms")
        ctx.has_real = real_c is not None
        ctx.save_for_backward(fake_c, *(() if real_c is None else (real_c,)))
        return out

    @staticmethod
    def backward(ctx, dout):
        L = _L()
        fake, real = ctx.saved_tensors[0], (ctx.saved_tensors[1] if ctx.has_real else None)
        dout = dout.contiguous()
        _lib.require_device(dout)
        dreal = torch.empty_like(real) if ctx.has_real and ctx.needs_input_grad[0] else None
        dfake = torch.empty_like(fake) if ctx.needs_input_grad[1] else None
        if dreal is None and dfake is None:
            return None, None
        _lib.check(L.odvae_gan_logit_terms_bwd_f32(_lib.ptr(real), 0 if real is None else real.numel(), fake.data_ptr(), fake.numel(),
                                                   dout.data_ptr(), _lib.ptr(dreal), _lib.ptr(dfake), _lib.stream_ptr()),
                   "gan_logit_terms_bwd")
        return dreal, dfake


def gan_logit_terms(real, fake):
    """[mean real, mean fake, mean relu(1 - real), mean relu(1 + fake), mean softplus(-real), mean softplus(fake)] as six f32 on the device;
    `real` may be None (generator phase: its three terms are 0).  hinge_d_loss = 0.5 (t[2] + t[3]), vanilla_d_loss = 0.5 (t[4] + t[5]),
    g_loss = -t[1].  The logits may have any shape and different element counts."""
    return _GanLogitTerms.apply(real, fake)


# ---- the PatchGAN discriminator on bf16 activations (opt-in: NLayerDiscriminator.set_precision("bf16"); conv_bf16.hip modes 5 / 6 / 7,
# conv_wgrad_bf16.hip modes 5 / 6; its BatchNorm + LeakyReLU is _BatchNormLReLU above) ----
def _conv4x4_b_raw(stride, dgrad, x, pack, cout, bias, ho, wo, out_f32, slope=0.0, cin_alg=None):
    """One odvae_conv4x4_bf16 call: x bf16 [N, C, H, W] -> [N, cout, ho, wo] in bf16 or f32"""
    L = _L()
    n, cx, hi, wi = x.shape
    y = _new_cl(n, cout, ho, wo, x, dtype=torch.float32 if out_f32 else BF16)
    tag = KERNEL_EVENTS.begin(secondary=True)
    _lib.check(L.odvae_conv4x4_bf16(stride, int(dgrad), x.data_ptr(), n, hi, wi, cx, pack.data_ptr(), cout, _lib.ptr(bias), y.data_ptr(),
                                    ho, wo, int(out_f32), float(slope), _lib.stream_ptr()),
               "conv4x4_bf16(stride=%d, dgrad=%d)" % (stride, dgrad))
    ca = cin_alg or cx
    px = (hi * wi) if dgrad else (ho * wo)      # 16 taps per pixel of the conv's OUTPUT, forward and transposed alike
    KERNEL_EVENTS.end("conv4x4_bf16", 2.0 * 16 * ca * cout * n * px, tag,
                      2.0 * n * hi * wi * ca + (4 if out_f32 else 2) * n * ho * wo * cout + 2.0 * 16 * ca * cout)
    return y


class _Conv4x4B(Function):
    """Conv2d(k=4, pad=1, stride 1|2) as an implicit GEMM on bf16 NHWC activations (no cols matrix; what is saved is the bf16 input).
    weight / bias are the f32 master parameters (OIHW), their gradients come back in f32.
    x f32 (the image; any channel count): cast and zero-padded to a multiple of 8 channels here, and its gradient comes back in f32
    on the image's channels (the kernel's f32 output form), so it feeds an f32 backward unchanged.
    Output: bf16, or f32 when cout is no multiple of 8 (the logit head).
    slope: LeakyReLU(slope) in the conv's epilogue (stride 2, bf16 output), one rounding."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, slope):
        L = _L()
        cout, cin = weight.shape[0], weight.shape[1]
        from_f32 = x.dtype != BF16
        if from_f32:
            x = _cl(x)
            if x.shape[1] != cin:
                raise ValueError("conv4x4_bf16: input has %d channels, weight expects %d" % (x.shape[1], cin))
            xb = cast_pad_bf16(x, _pad8(cin))
        else:
            xb = _cl(x, BF16)
            if xb.shape[1] != cin:
                raise ValueError("conv4x4_bf16: input has %d channels, weight expects %d" % (xb.shape[1], cin))
            if cin % 8:
                raise ValueError("conv4x4_bf16: a bf16 input needs a multiple of 8 channels, got %d" % cin)
        n, cx, hi, wi = xb.shape
        ho, wo = _conv4x4_out(hi, stride), _conv4x4_out(wi, stride)
        out_f32 = cout % 8 != 0
        if slope and (out_f32 or stride != 2):
            raise NotImplementedError("conv4x4_bf16: the LeakyReLU epilogue is built for the stride-2 conv with a bf16 output")
        need_dx = bool(ctx.needs_input_grad[0])
        # "bf16v": a pack is rebuilt when THIS weight was written (its optimizer's step, a load_state_dict), not at every optimizer
        # step: the generator's step between the two phases of a GAN batch leaves the discriminator's packs valid, and the three
        # discriminator forwards of a batch (generator side, real, fake) read one pack
        fwd_pack, dpack = pack_conv3x3(weight, True, need_dx, "bf16v")
        b = bias.detach().contiguous() if bias is not None else None
        y = _conv4x4_b_raw(stride, False, xb, fwd_pack, cout, b, ho, wo, out_f32, slope or 0.0, cin_alg=cin)
        ctx.stride, ctx.slope, ctx.has_bias, ctx.from_f32, ctx.dpack = stride, float(slope or 0.0), bias is not None, from_f32, dpack
        ctx.pack_tag, ctx.wref = _ops.PACK_CACHE.weight_tag(weight), weakref.ref(weight)
        ctx.wshape = tuple(weight.shape)
        ctx.save_for_backward(xb, y if slope else None)     # (y is the next layer's saved input anyway)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _L()
        xb, y = ctx.saved_tensors
        cout, cin = ctx.wshape[0], ctx.wshape[1]
        n, cx, hi, wi = xb.shape
        _, _, ho, wo = dy.shape
        stride = ctx.stride
        f32_dy = dy.dtype != BF16
        if f32_dy:                       # the head's f32 upstream gradient: one cast (+ channel pad) pass
            cp = _pad8(cout)
            dyb = cast_pad_bf16(_cl(dy), cp)
        else:
            cp = cout
            dyb = _cl(dy, BF16)
            if ctx.slope:
                g = torch.empty_like(dyb)
                _lib.check(L.odvae_leaky_relu_bwd_bf16(y.data_ptr(), dyb.data_ptr(), g.data_ptr(), ctx.slope, dyb.numel(), _lib.stream_ptr()),
                           "leaky_relu_bwd_bf16")
                dyb = g
        dx = dw = db = None
        if ctx.needs_input_grad[0] and not _ops.WEIGHT_GRADIENT_ONLY:
            _check_pack_current(ctx, "conv4x4_bf16")
            dx = _conv4x4_b_raw(stride, True, dyb, ctx.dpack, cin, None, hi, wi, ctx.from_f32, cin_alg=cout)
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        fold_db = want_db and not f32_dy and ctx.needs_input_grad[1]
        if ctx.needs_input_grad[1]:
            mode = 5 if stride == 1 else 6
            dwf = torch.empty((cp, cx, 4, 4), dtype=torch.float32, device=xb.device)
            dbf = torch.empty(cp, dtype=torch.float32, device=xb.device) if fold_db else None
            wp, wn = _ws(L.odvae_conv_wgrad_bf16_workspace_bytes(mode, n, ho, wo, cx, cp), xb)
            tag = KERNEL_EVENTS.begin(secondary=True)
            _lib.check(L.odvae_conv_wgrad_bf16(mode, xb.data_ptr(), dyb.data_ptr(), n, hi, wi, cx, ho, wo, cp, dwf.data_ptr(), _lib.ptr(dbf),
                                               wp, wn, _lib.stream_ptr()), "conv_wgrad_bf16(mode=%d)" % mode)
            KERNEL_EVENTS.end("conv4x4_wgrad_bf16", 2.0 * 16 * cx * cp * n * ho * wo, tag, 2.0 * n * (hi * wi * cx + ho * wo * cp))
            dw = dwf if (cp == cout and cx == cin) else dwf[:cout, :cin].contiguous()
            if fold_db:
                db = dbf
        if want_db and not fold_db:
            if f32_dy:                   # sum the f32 values themselves
                db = _colsum(_cl(dy), n * ho * wo, cout)
            else:
                db = torch.empty(cout, dtype=torch.float32, device=xb.device)
                rows = n * ho * wo
                wp, wn = _ws(L.odvae_colsum_bf16_workspace_bytes(rows, cout), xb)
                _lib.check(L.odvae_colsum_bf16(dyb.data_ptr(), rows, cout, db.data_ptr(), wp, wn, _lib.stream_ptr()), "colsum_bf16")
        return dx, dw, db, None, None


def conv4x4_bf16(x, weight, bias, stride, lrelu=None):
    """PatchGAN convolution on the bf16 MFMA kernels (see _Conv4x4B).  lrelu: slope of a LeakyReLU fused into the epilogue, or None."""
    if stride not in (1, 2):
        raise ValueError("conv4x4_bf16: stride must be 1 or 2, got %r" % (stride,))
    if x.dim() != 4 or x.shape[2] < 2 or x.shape[3] < 2:
        raise ValueError("conv4x4_bf16: needs an [N, C, H, W] input with H, W >= 2 (kernel 4, padding 1), got %s" % (tuple(x.shape),))
    if tuple(weight.shape[2:]) != (4, 4):
        raise ValueError("conv4x4_bf16: weight %s is no 4x4 kernel" % (tuple(weight.shape),))
    return _Conv4x4B.apply(x, weight, bias, int(stride), float(lrelu) if lrelu else 0.0)
