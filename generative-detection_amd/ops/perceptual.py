"""LPIPS-style perceptual network pieces: scaling layer, max-pool, distance in f32 (lpips_f32.hip) and the bf16 net
(conv_bf16.hip RELU / MASK, lpips_bf16.hip)."""
import torch
from torch.autograd import Function

from .. import ops as _ops      # the package: switches and run-time state are read and written there (ops/__init__.py)
from .. import lib as _lib
from ._base import BF16, KERNEL_EVENTS, _L, _cl, _new_cl, _ws
from .packs import pack_conv3x3
from .conv_bf16 import _conv_b_raw


# ------------------------------------------------------------------------------------------------------
# LPIPS-style perceptual network pieces (lpips_f32.hip)
# ------------------------------------------------------------------------------------------------------
class _ScalingLayer(Function):
    @staticmethod
    def forward(ctx, x, shift, scale):
        L = _L()
        x = _cl(x)
        n, c, h, w = x.shape
        sh, sc = shift.detach().reshape(-1).contiguous(), scale.detach().reshape(-1).contiguous()
        y = _new_cl(n, c, h, w, x)
        _lib.check(L.odvae_scaling_layer_f32(x.data_ptr(), sh.data_ptr(), sc.data_ptr(), y.data_ptr(), n * h * w, c, 0,
                                             _lib.stream_ptr()), "scaling_layer")
        ctx.save_for_backward(sh, sc)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _L()
        sh, sc = ctx.saved_tensors
        dy = _cl(dy)
        n, c, h, w = dy.shape
        dx = _new_cl(n, c, h, w, dy)
        _lib.check(L.odvae_scaling_layer_f32(dy.data_ptr(), sh.data_ptr(), sc.data_ptr(), dx.data_ptr(), n * h * w, c, 1,
                                             _lib.stream_ptr()), "scaling_layer bwd")
        return dx, None, None


def scale_shift(x, shift, scale, out_dtype=None):
    """lpips.ScalingLayer.  out_dtype=torch.bfloat16: the hand-off into the bf16 perceptual net in the same pass -- bf16, channels
    zero-padded to 8 (see _ScalingLayerB)."""
    if out_dtype == BF16:
        return _ScalingLayerB.apply(x, shift, scale)
    return _ScalingLayer.apply(x, shift, scale)


class _MaxPool2x2(Function):
    @staticmethod
    def forward(ctx, x):
        L = _L()
        x = _cl(x)
        n, c, h, w = x.shape
        y = _new_cl(n, c, h // 2, w // 2, x)
        _lib.check(L.odvae_maxpool2x2_f32(x.data_ptr(), y.data_ptr(), n, h, w, c, h // 2, w // 2, _lib.stream_ptr()), "maxpool2x2")
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _L()
        x, y = ctx.saved_tensors
        dy = _cl(dy)
        n, c, h, w = x.shape
        dx = _new_cl(n, c, h, w, x)
        _lib.check(L.odvae_maxpool2x2_bwd_f32(x.data_ptr(), y.data_ptr(), dy.data_ptr(), dx.data_ptr(), n, h, w, c, h // 2, w // 2,
                                              _lib.stream_ptr()), "maxpool2x2_bwd")
        return dx


def maxpool2x2(x, relu_mask=False):
    """torch.nn.MaxPool2d(2, 2): floors, so an odd last row / column is dropped and gets a zero gradient; NaN propagates.
    bf16 input: the bf16 kernels; relu_mask=True there says x is a ReLU output whose producer was told `grad_premasked` -- the backward
    then writes the gradient at that ReLU's pre-activation (x > 0 ? dx : 0)."""
    if x.dim() != 4 or x.shape[2] < 2 or x.shape[3] < 2:
        raise ValueError("maxpool2x2: needs an [N, C, H, W] input with H, W >= 2, got %s" % (tuple(x.shape),))
    if x.dtype == BF16:
        return _MaxPool2x2B.apply(x, bool(relu_mask))
    if relu_mask:
        raise NotImplementedError("maxpool2x2(relu_mask=True) is the bf16 perceptual net's (the f32 layers mask in a pass of their own)")
    return _MaxPool2x2.apply(x)


class _LpipsDistance(Function):
    """[B] spatial mean of lin_w . (normalize(f0) - normalize(f1))^2; differentiable w.r.t. f1 (the reconstruction)."""

    @staticmethod
    def forward(ctx, f0, f1, lin_w):
        L = _L()
        f0, f1 = _cl(f0), _cl(f1)
        n, c, h, w = f0.shape
        wv = lin_w.detach().reshape(-1).contiguous()
        out = torch.empty(n, dtype=torch.float32, device=f0.device)
        wp, wn = _ws(n * 1024, f0)
        _lib.check(L.odvae_lpips_distance_f32(f0.data_ptr(), f1.data_ptr(), wv.data_ptr(), out.data_ptr(), n, h * w, c, wp, wn,
                                              _lib.stream_ptr()), "lpips_distance")
        ctx.save_for_backward(f0, f1, wv)
        return out

    @staticmethod
    def backward(ctx, g):
        L = _L()
        f0, f1, wv = ctx.saved_tensors
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("lpips_layer_distance: gradient w.r.t. the first (input) branch is not on the OD-VAE path")
        n, c, h, w = f1.shape
        df1 = None
        if ctx.needs_input_grad[1]:
            df1 = _new_cl(n, c, h, w, f1)
            _lib.check(L.odvae_lpips_distance_bwd_f32(f0.data_ptr(), f1.data_ptr(), wv.data_ptr(), g.contiguous().data_ptr(),
                                                      df1.data_ptr(), n, h * w, c, _lib.stream_ptr()), "lpips_distance_bwd")
        return None, df1, None


def lpips_layer_distance(f0, f1, lin_w):
    if f1.dtype == BF16:
        return _LpipsTapB.apply(f0, f1, lin_w, False, False)
    return _LpipsDistance.apply(f0, f1, lin_w)


# ---- the LPIPS-style perceptual net on bf16 features (opt-in: LPIPSStyle.set_precision("bf16"); conv_bf16.hip RELU / MASK, lpips_bf16.hip) ----

# Where the ReLU masks go.  The backward of y = relu(conv(x)) is dy * (y > 0).  In this net every tensor that consumes a ReLU output y --
# the next conv, a pool, a distance tap -- has y as its own saved input, so its backward can write `y > 0 ? gradient : 0` from the
# epilogue of the kernel that computes the gradient: what arrives at the producing layer is already the gradient at its pre-activation and
# no dy * (y > 0) pass runs (the f32 path spends one per layer).  The producer has to be told (`grad_premasked=True`) and then applies no
# mask of its own; the consumer is told that its input is such a ReLU output (`mask_input` / `relu_mask`).  LPIPSStyle wires its layers
# that way; every op's default is the plain, self-contained gradient.


def _conv_relu_b_raw(x, pack, cout, bias, cin_alg):
    L = _L()
    n, cx, h, w = x.shape
    y = _new_cl(n, cout, h, w, x, dtype=BF16)
    tag = KERNEL_EVENTS.begin()
    _lib.check(L.odvae_conv_bf16_relu(x.data_ptr(), n, h, w, cx, pack.data_ptr(), cout, _lib.ptr(bias), y.data_ptr(), _lib.stream_ptr()),
               "conv_bf16_relu")
    KERNEL_EVENTS.end("conv_bf16", 2.0 * 9 * cin_alg * cout * n * h * w, tag, 2.0 * n * h * w * (cin_alg + cout) + 2.0 * 9 * cin_alg * cout,
                      variant="ReLU epilogue (VGG)")
    return y


def _conv_masked_b_raw(dy, dpack, cin, mask):
    """Data gradient of a stride-1 3x3 conv, masked by the ReLU output that was the conv's input"""
    L = _L()
    n, cout, h, w = dy.shape
    dx = _new_cl(n, cin, h, w, dy, dtype=BF16)
    tag = KERNEL_EVENTS.begin()
    _lib.check(L.odvae_conv_bf16_masked(dy.data_ptr(), n, h, w, cout, dpack.data_ptr(), cin, mask.data_ptr(), dx.data_ptr(),
                                        _lib.stream_ptr()), "conv_bf16_masked")
    KERNEL_EVENTS.end("conv_bf16", 2.0 * 9 * cin * cout * n * h * w, tag, 2.0 * n * h * w * (2 * cin + cout) + 2.0 * 9 * cin * cout,
                      variant="masked data gradient (VGG)")
    return dx


def _relu_bwd_b(y, dy):
    g = torch.empty_like(dy)
    _lib.check(_L().odvae_relu_bwd_bf16(y.data_ptr(), dy.data_ptr(), g.data_ptr(), dy.numel(), _lib.stream_ptr()), "relu_bwd_bf16")
    return g


class _ConvReluB(Function):
    """relu(conv3x3(x) + bias) on bf16 NHWC activations in one launch; the weights are frozen f32 master parameters (no weight gradient:
    the VGG stack of the perceptual loss).  mask_input: x is a ReLU output whose producer runs with grad_premasked.  grad_premasked: every
    consumer of the result masks the gradient it sends back with (result > 0).  A forward that needs no gradient w.r.t. x (the target
    branch) builds no data-gradient pack and saves nothing."""

    @staticmethod
    def forward(ctx, x, weight, bias, mask_input, grad_premasked):
        L = _L()
        x = _cl(x, BF16)
        cout, cin = weight.shape[0], weight.shape[1]
        if weight.requires_grad or (bias is not None and bias.requires_grad):
            raise NotImplementedError("conv3x3(bf16, relu=True): frozen weights only (no weight gradient on this path)")
        if x.shape[1] != cin and L.odvae_conv_bf16_reduce_pad(x.shape[1]) != L.odvae_conv_bf16_reduce_pad(cin):
            raise ValueError("conv_bf16: input has %d channels, weight expects %d" % (x.shape[1], cin))
        need_dx = bool(ctx.needs_input_grad[0])
        fwd_pack, dpack = pack_conv3x3(weight, True, need_dx, "bf16")
        y = _conv_relu_b_raw(x, fwd_pack, cout, bias.detach().contiguous() if bias is not None else None, cin)
        ctx.need_dx = need_dx
        if need_dx:
            ctx.dpack, ctx.cin, ctx.mask_input, ctx.premasked = dpack, cin, bool(mask_input), bool(grad_premasked)
            ctx.padded = x.shape[1] != cin
            ctx.save_for_backward(x if mask_input else None, None if grad_premasked else y)
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.need_dx or _ops.WEIGHT_GRADIENT_ONLY:
            return None, None, None, None, None
        if ctx.padded:
            raise NotImplementedError("data gradient through a channel-padded input (the image layer of the VGG stack goes through "
                                      "_VggStemB, which returns the 3-channel f32 gradient)")
        x, y = ctx.saved_tensors
        dy = _cl(dy, BF16)
        if not ctx.premasked:
            dy = _relu_bwd_b(y, dy)
        if ctx.mask_input:
            dx = _conv_masked_b_raw(dy, ctx.dpack, ctx.cin, x)
        else:
            dx = _conv_b_raw(0, dy, ctx.dpack, ctx.cin, None, None, False)
        return dx, None, None, None, None


def conv3x3_relu_bf16(x, weight, bias, mask_input=False, grad_premasked=False):
    """A VGG layer of the bf16 perceptual net (see "Where the ReLU masks go" above)."""
    return _ConvReluB.apply(x, weight, bias, bool(mask_input), bool(grad_premasked))


def _scaling_b_raw(x, sh, sc):
    n, c, h, w = x.shape
    y = _new_cl(n, 8, h, w, x, dtype=BF16)
    _lib.check(_L().odvae_scaling_layer_bf16(x.data_ptr(), sh.data_ptr(), sc.data_ptr(), y.data_ptr(), n * h * w, c, _lib.stream_ptr()),
               "scaling_layer_bf16")
    return y


def _scaling_bwd_raw(dy, sh, sc):
    n, c, h, w = dy.shape
    dx = _new_cl(n, c, h, w, dy)
    _lib.check(_L().odvae_scaling_layer_f32(dy.data_ptr(), sh.data_ptr(), sc.data_ptr(), dx.data_ptr(), n * h * w, c, 1, _lib.stream_ptr()),
               "scaling_layer bwd")
    return dx


class _ScalingLayerB(Function):
    """f32 image [N, C <= 8, H, W] -> bf16 [N, 8, H, W] = (x - shift) / scale, padding channels zero: one pass instead of a scale pass plus
    a cast + pad pass.  The gradient (8 channels, bf16 or f32) is cut back to the C image channels and scaled in f32."""

    @staticmethod
    def forward(ctx, x, shift, scale):
        x = _cl(x)
        sh, sc = shift.detach().reshape(-1).contiguous(), scale.detach().reshape(-1).contiguous()
        ctx.c = x.shape[1]
        ctx.save_for_backward(sh, sc)
        return _scaling_b_raw(x, sh, sc)

    @staticmethod
    def backward(ctx, dy):
        sh, sc = ctx.saved_tensors
        d = _cl(dy[:, :ctx.c].float())
        return _scaling_bwd_raw(d, sh, sc), None, None


class _VggStemB(Function):
    """ScalingLayer + the first VGG layer of the bf16 perceptual net: f32 image -> relu(conv3x3((x - shift) / scale)) in bf16.  Two
    launches (odvae_scaling_layer_bf16 writes the 8-channel bf16 image, the conv reads it); one autograd node, because the conv's data
    gradient comes back with the image's 3 channels in f32 (the kernel's f32 output form, as decoder.conv_out) and goes through the f32
    scaling backward -- it never has the padded input's shape."""

    @staticmethod
    def forward(ctx, x, shift, scale, weight, bias, grad_premasked):
        x = _cl(x)
        cout, cin = weight.shape[0], weight.shape[1]
        if weight.requires_grad or (bias is not None and bias.requires_grad):
            raise NotImplementedError("vgg_stem_bf16: frozen weights only")
        if x.shape[1] != cin:
            raise ValueError("vgg_stem_bf16: image has %d channels, weight expects %d" % (x.shape[1], cin))
        sh, sc = shift.detach().reshape(-1).contiguous(), scale.detach().reshape(-1).contiguous()
        need_dx = bool(ctx.needs_input_grad[0])
        fwd_pack, dpack = pack_conv3x3(weight, True, need_dx, "bf16")
        y = _conv_relu_b_raw(_scaling_b_raw(x, sh, sc), fwd_pack, cout, bias.detach().contiguous() if bias is not None else None, cin)
        ctx.need_dx = need_dx
        if need_dx:
            ctx.dpack, ctx.cin, ctx.premasked = dpack, cin, bool(grad_premasked)
            ctx.save_for_backward(sh, sc, None if grad_premasked else y)
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.need_dx or _ops.WEIGHT_GRADIENT_ONLY:
            return None, None, None, None, None, None
        sh, sc, y = ctx.saved_tensors
        dy = _cl(dy, BF16)
        if not ctx.premasked:
            dy = _relu_bwd_b(y, dy)
        d = _conv_b_raw(0, dy, ctx.dpack, ctx.cin, None, None, True)     # f32, the image's channels
        return _scaling_bwd_raw(d, sh, sc), None, None, None, None, None


def vgg_stem_bf16(x, shift, scale, weight, bias, grad_premasked=False):
    return _VggStemB.apply(x, shift, scale, weight, bias, bool(grad_premasked))


class _MaxPool2x2B(Function):
    """MaxPool2d(2, 2) on bf16; the backward recomputes the window maxima from x.  relu_mask: see maxpool2x2."""

    @staticmethod
    def forward(ctx, x, relu_mask):
        L = _L()
        x = _cl(x, BF16)
        n, c, h, w = x.shape
        y = _new_cl(n, c, h // 2, w // 2, x, dtype=BF16)
        _lib.check(L.odvae_maxpool2x2_bf16(x.data_ptr(), y.data_ptr(), n, h, w, c, h // 2, w // 2, _lib.stream_ptr()), "maxpool2x2_bf16")
        ctx.relu_mask = bool(relu_mask)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _L()
        (x,) = ctx.saved_tensors
        dy = _cl(dy, BF16)
        n, c, h, w = x.shape
        dx = _new_cl(n, c, h, w, x, dtype=BF16)
        _lib.check(L.odvae_maxpool2x2_bwd_bf16(x.data_ptr(), dy.data_ptr(), x.data_ptr() if ctx.relu_mask else None, dx.data_ptr(),
                                               n, h, w, c, h // 2, w // 2, _lib.stream_ptr()), "maxpool2x2_bwd_bf16")
        return dx, None


class _LpipsTapB(Function):
    """A distance tap of the bf16 perceptual net: d [B] = spatial mean of lin_w . (normalize(f0) - normalize(f1))^2 on bf16 features,
    f32 inside; differentiable w.r.t. f1 (the reconstruction).
    passthrough=True also returns f1 itself for the next slice to read: the tap then receives BOTH gradients of f1 -- its own and the one
    arriving from the next slice's pool -- in one backward call, and one kernel sums them in f32, masks and rounds once (autograd's own
    accumulation would round the two bf16 gradients separately and add them in a pass of its own).
    relu_mask=True: f1 is a ReLU output whose producer runs with grad_premasked; the gradient is masked with (f1 > 0)."""

    @staticmethod
    def forward(ctx, f0, f1, lin_w, passthrough, relu_mask):
        L = _L()
        f0, f1 = _cl(f0, BF16), _cl(f1, BF16)
        n, c, h, w = f0.shape
        if tuple(f1.shape) != (n, c, h, w):
            raise ValueError("lpips tap: feature shapes differ: %s vs %s" % (tuple(f0.shape), tuple(f1.shape)))
        wv = lin_w.detach().reshape(-1).contiguous()
        out = torch.empty(n, dtype=torch.float32, device=f0.device)
        wp, wn = _ws(n * 1024, f0)
        _lib.check(L.odvae_lpips_distance_bf16(f0.data_ptr(), f1.data_ptr(), wv.data_ptr(), out.data_ptr(), n, h * w, c, wp, wn,
                                               _lib.stream_ptr()), "lpips_distance_bf16")
        ctx.relu_mask = bool(relu_mask)
        if ctx.needs_input_grad[1]:
            ctx.save_for_backward(f0, f1, wv)
        ctx.set_materialize_grads(False)
        if passthrough:
            return out, f1     # (an input handed back as it is: autograd makes it a view whose gradient comes to this node)
        return out

    @staticmethod
    def backward(ctx, g, dnext=None):
        L = _L()
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("lpips_layer_distance: gradient w.r.t. the first (input) branch is not on the OD-VAE path")
        if not ctx.needs_input_grad[1] or (g is None and dnext is None):
            return None, None, None, None, None
        f0, f1, wv = ctx.saved_tensors
        n, c, h, w = f1.shape
        if g is None:
            g = torch.zeros(n, dtype=torch.float32, device=f1.device)
        dn = _cl(dnext, BF16) if dnext is not None else None
        df1 = _new_cl(n, c, h, w, f1, dtype=BF16)
        _lib.check(L.odvae_lpips_distance_bwd_bf16(f0.data_ptr(), f1.data_ptr(), wv.data_ptr(), g.contiguous().data_ptr(), _lib.ptr(dn),
                                                   f1.data_ptr() if ctx.relu_mask else None, df1.data_ptr(), n, h * w, c,
                                                   _lib.stream_ptr()), "lpips_distance_bwd_bf16")
        return None, df1, None, None, None


def lpips_tap_bf16(f0, f1, lin_w, passthrough=False, relu_mask=False):
    """-> d, or (d, f1 for the next slice) with passthrough (see _LpipsTapB)"""
    return _LpipsTapB.apply(f0, f1, lin_w, bool(passthrough), bool(relu_mask))
