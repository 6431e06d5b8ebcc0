"""The f32 3x3 conv family (direct, Winograd F(2x2) / F(4x4), their routes), the 1x1 conv, and the dispatchers `conv3x3` /
`conv1x1` that hand bf16 activations to conv_bf16.py / perceptual.py."""
import contextlib

import torch
from torch.autograd import Function

from .. import ops as _ops      # the package: switches and run-time state are read and written there (ops/__init__.py)
from .. import lib as _lib
from ._base import BF16, KERNEL_EVENTS, _L, _cl, _new_cl, _stamp, _ws
from .packs import pack_conv3x3
from .gn_link import GN_GROUPS, _gn_bwd_link_of, _gn_stats_ok, _tag_gn_partials
from .gemm import _colsum, gemm
from .conv_bf16 import _ConvB
from .perceptual import _ConvReluB


# ------------------------------------------------------------------------------------------------------
# 3x3 convolution family
# ------------------------------------------------------------------------------------------------------
def _conv3x3_raw(mode, x, pack, cin, cout, bias, residual, act=0):
    L = _L()
    n, _, hi, wi = x.shape
    if mode == 0:
        ho, wo = hi, wi
    elif mode in (1, 6):
        ho, wo = hi // 2, wi // 2
    else:
        ho, wo = 2 * hi, 2 * wi
    y = _new_cl(n, cout, ho, wo, x)
    tag = KERNEL_EVENTS.begin() if (mode == 0 and cout > 32 and cin > 3) else None   # the 128-wide v2 kernel only
    _lib.check(L.odvae_conv3x3_f32(mode, x.data_ptr(), n, hi, wi, cin, pack.data_ptr(), cout,
                                   _lib.ptr(bias), _lib.ptr(residual), y.data_ptr(), ho, wo, int(act), _lib.stream_ptr()),
               "conv3x3(mode=%d)" % mode)
    KERNEL_EVENTS.end("conv3x3_128x128", 2.0 * 9 * cin * cout * n * ho * wo, tag,
                      4.0 * (n * hi * wi * cin + n * ho * wo * cout * (2 if residual is not None else 1) + 9 * cin * cout),
                      issued=_conv_issued(mode, n, hi, wi, ho, wo, cin, cout))
    return y


def _conv_issued(mode, n, hi, wi, ho, wo, cin, cout):
    """Multiply-add FLOP the direct kernels issue: modes 0/1/2 nine taps per output pixel; mode 3 (transposed stride-2
    data gradient, inserted zeros skipped) nine per LOW-res pixel; modes 5/6 (Upsample conv by parity class) sixteen
    pre-summed taps per low-res pixel."""
    if mode in (5, 6, 3):
        lo = n * min(hi, ho) * min(wi, wo)
        return 2.0 * (9 if mode == 3 else 16) * cin * cout * lo
    return 2.0 * 9 * cin * cout * n * ho * wo


@contextlib.contextmanager
def weight_gradient_only():
    prev, _ops.WEIGHT_GRADIENT_ONLY = _ops.WEIGHT_GRADIENT_ONLY, True
    try:
        yield
    finally:
        _ops.WEIGHT_GRADIENT_ONLY = prev


def _wino_ok(h, w, cin, cout):
    # both the forward (reduce over cin) and the data gradient (reduce over cout) need channel counts in whole quads
    return _ops.WINOGRAD and h % 2 == 0 and w % 2 == 0 and cin % 4 == 0 and cout % 4 == 0 and cin >= 16 and cout >= 16


def _wino4_ok(h, w, cin, cout):
    return _ops.WINOGRAD and _ops.WINOGRAD4 and bool(_L().odvae_conv3x3_wino4_supported(h, w, cin, cout))


def _conv3x3_wino_raw(x, pack, cin, cout, bias, residual, act=0, f4=False, stats=False, upsample=False):
    """stats=True (F(4x4) only): returns (y, partials [N][tiles][32][2]) -- the GroupNorm statistics of y per output tile.
    upsample=True (F(4x4) only): x is the low-resolution input of an Upsample conv, y has twice its height and width."""
    L = _L()
    n, _, h, w = x.shape
    if upsample:
        h, w = 2 * h, 2 * w
    y = _new_cl(n, cout, h, w, x)
    tag = KERNEL_EVENTS.begin() if cout > 32 else None
    partial = None
    if stats:
        partial = torch.empty(n, L.odvae_conv3x3_wino4_stats_chunks(h, w), GN_GROUPS, 2, dtype=torch.float32, device=x.device)
    if upsample:
        _lib.check(L.odvae_conv3x3_wino4_up_f32(x.data_ptr(), n, h, w, cin, pack.data_ptr(), cout, _lib.ptr(bias), _lib.ptr(residual),
                                                y.data_ptr(), _lib.ptr(partial), GN_GROUPS if stats else 0, _lib.stream_ptr()), "conv3x3_wino4_up")
    elif stats:
        _lib.check(L.odvae_conv3x3_wino4_stats_f32(x.data_ptr(), n, h, w, cin, pack.data_ptr(), cout, _lib.ptr(bias), _lib.ptr(residual),
                                                   y.data_ptr(), partial.data_ptr(), GN_GROUPS, _lib.stream_ptr()), "conv3x3_wino4_stats")
    else:
        fn = L.odvae_conv3x3_wino4_f32 if f4 else L.odvae_conv3x3_wino_f32
        _lib.check(fn(x.data_ptr(), n, h, w, cin, pack.data_ptr(), cout, _lib.ptr(bias), _lib.ptr(residual),
                      y.data_ptr(), int(act), _lib.stream_ptr()), "conv3x3_wino4" if f4 else "conv3x3_wino")
    # issued multiply-adds per output pixel and (ci, co): F(2x2,3x3) 16 per 2x2 tile = 4, F(4x4,3x3) 36 per 4x4 tile = 2.25
    KERNEL_EVENTS.end("conv3x3_wino4" if f4 else "conv3x3_128x128", 2.0 * 9 * cin * cout * n * h * w, tag,
                      4.0 * (n * h * w * cin // (4 if upsample else 1) + n * h * w * cout * (2 if residual is not None else 1) + 9 * cin * cout),
                      issued=2.0 * (2.25 if f4 else 4.0) * cin * cout * n * h * w,
                      variant=(("upsample" if upsample else "plain") + (" + GroupNorm statistics" if stats else "")) if f4 else None)
    return (y, partial) if stats else y


# The kernels one f32 3x3 conv call runs, by route (_conv3x3_route picks it).  Each entry: (pack kind, forward mode, data-gradient mode,
# weight-gradient mode) of the direct kernels odvae_conv3x3_f32 / odvae_conv3x3_wgrad_f32; None where a Winograd kernel runs instead.
# (Stride-1 layers may take the Winograd-domain weight gradient in place of the direct one: that depends on N too, see _Conv3x3.backward.)
CONV3X3_ROUTES = {
    "direct":    ("direct", 0, 0, 0),
    "down":      ("direct", 1, 3, 1),         # data gradient: the transposed stride-2 conv
    "up_dense":  ("direct", 2, 0, 2),         # data gradient at full resolution, then odvae_upsample2x_bwd_f32 (2x2 sum-pool)
    "up_parity": ("up", 5, 6, 5),             # 16 pre-summed taps per low-res pixel instead of 36
    "wino2":     ("wino", None, None, 0),     # odvae_conv3x3_wino_f32, F(2x2,3x3), both ways
    "wino4":     ("wino4", None, None, 0),    # odvae_conv3x3_wino4_f32 / _stats_f32; data gradient: _wino4_f32, or _wino4_gnbwd_f32 with a live GroupNorm link
    "wino4_up":  ("wino4", None, None, 5),    # odvae_conv3x3_wino4_up_f32; data gradient: _wino4_pool_f32 (UPCONV_POOLED_DGRAD off: _wino4_f32, then upsample2x_bwd)
}


def _conv3x3_route(mode, hi, wi, cin, cout, relu):
    """The route (a key of CONV3X3_ROUTES) of one f32 3x3 conv call; hi, wi: the INPUT height and width."""
    if mode == 1:
        return "down"
    if mode == 2:
        if not _ops.UPCONV_BY_PARITY:
            return "up_dense"
        # the Upsample conv on the F(4x4) kernel: the halo of the (never formed) upsampled image is read from x[iy >> 1][ix >> 1]
        return "wino4_up" if _ops.UPCONV_WINOGRAD4 and not relu and _wino4_ok(2 * hi, 2 * wi, cin, cout) else "up_parity"
    if mode != 0:
        raise ValueError("conv3x3: mode %r (0: stride 1, 1: Downsample, 2: Upsample)" % (mode,))
    if not _wino_ok(hi, wi, cin, cout):
        return "direct"
    # (not with a fused ReLU, i.e. not in the frozen VGG stack of the perceptual loss: F(4x4)'s ~1e-5 output error flips ten times
    # more ReLU masks than F(2x2)'s ~1e-6, and the input gradient of LPIPS then leaves the 5e-3 the parity tests hold it to)
    return "wino4" if not relu and _wino4_ok(hi, wi, cin, cout) else "wino2"


class _Conv3x3(Function):
    """mode 0: stride 1 pad 1; mode 1: Downsample (pad (0,1,0,1), stride 2); mode 2: Upsample (nearest 2x) + conv."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, mode, relu, gn_stats=False, gn_link=None):
        """gn_stats=True: returns (y, partials) when the F(4x4) kernel takes the layer (partials: GroupNorm statistics of y per output
        tile, not differentiable), (y, None) otherwise.  gn_link: x is swish(GroupNorm(.)) and this is its link (_GnBwdLink)."""
        x = _cl(x)
        res = _cl(residual) if residual is not None else None
        cout, cin = weight.shape[0], weight.shape[1]
        route = _conv3x3_route(mode, x.shape[2], x.shape[3], cin, cout, relu)
        kind, fwd_mode, _, _ = CONV3X3_ROUTES[route]
        fwd_pack, _ = pack_conv3x3(weight, True, bool(ctx.needs_input_grad[0]), kind)  # both packs in one launch
        b = bias.detach().contiguous() if bias is not None else None
        partial = None
        if fwd_mode is not None:
            y = _conv3x3_raw(fwd_mode, x, fwd_pack, cin, cout, b, res, act=1 if relu else 0)
        else:
            f4 = route != "wino2"
            stats = bool(f4 and gn_stats and _gn_stats_ok(cout))
            out = _conv3x3_wino_raw(x, fwd_pack, cin, cout, b, res, act=1 if relu else 0, f4=f4, stats=stats, upsample=route == "wino4_up")
            y, partial = out if stats else (out, None)
        ctx.mode, ctx.route = mode, route
        ctx.gn_link = gn_link if (route == "wino4" and gn_link is not None and ctx.needs_input_grad[0]) else None
        ctx.pack_epoch = _ops.PACK_CACHE.epoch
        ctx.relu = bool(relu)
        ctx.has_bias = bias is not None
        ctx.has_res = residual is not None
        ctx.save_for_backward(x, weight, y if relu else None)
        if gn_stats:
            if partial is not None:
                ctx.mark_non_differentiable(partial)
            ctx.set_materialize_grads(False)   # the statistics output has no gradient: not a tensor of zeros per backward (a fill launch each)
            return y, partial
        return y

    @staticmethod
    def backward(ctx, dy, _dpartial=None):
        L = _L()
        if dy is None:
            return None, None, None, None, None, None, None, None
        x, weight, y_act = ctx.saved_tensors
        mode, route = ctx.mode, ctx.route
        kind, _, dgrad_mode, wgrad_mode = CONV3X3_ROUTES[route]
        dy = _cl(dy)
        if ctx.relu:  # gradient through the fused ReLU: dy * (y > 0)
            g = _new_cl(*[dy.shape[i] for i in (0, 1, 2, 3)], dy)
            _lib.check(L.odvae_leaky_relu_bwd_f32(y_act.data_ptr(), dy.data_ptr(), g.data_ptr(), 0.0, dy.numel(),
                                                  _lib.stream_ptr()), "relu_bwd")
            dy = g
        cout, cin = weight.shape[0], weight.shape[1]
        n, _, hi, wi = x.shape
        _, _, ho, wo = dy.shape
        dx = dw = db = None
        if ctx.needs_input_grad[0] and not _ops.WEIGHT_GRADIENT_ONLY:
            _ops.PACK_CACHE.check_epoch(ctx.pack_epoch, "conv3x3 backward")
            _, dgr = pack_conv3x3(weight, False, True, kind)
            pooled = route == "wino4_up" and _ops.UPCONV_POOLED_DGRAD
            if pooled:
                # gradient w.r.t. the upsampled image on the F(4x4) kernel, 2x2-summed in its output transform (never stored at full size)
                dx = _new_cl(n, cin, hi, wi, x)
                tag = KERNEL_EVENTS.begin()
                _lib.check(L.odvae_conv3x3_wino4_pool_f32(dy.data_ptr(), n, ho, wo, cout, dgr.data_ptr(), cin, dx.data_ptr(), _lib.stream_ptr()),
                           "conv3x3_wino4_pool")
                KERNEL_EVENTS.end("conv3x3_wino4", 2.0 * 9 * cin * cout * n * ho * wo, tag, 4.0 * (n * ho * wo * cout + n * hi * wi * cin + 9 * cin * cout),
                                  issued=2.0 * 2.25 * cin * cout * n * ho * wo, variant="data gradient, 2x2-summed (Upsample)")
            elif route == "wino4" and ctx.gn_link is not None and (gn_ops := ctx.gn_link.operands()) is not None:
                # da and, from the same output transform, the first pass of the backward of the GroupNorm that produced this conv's input
                lk = ctx.gn_link
                gx, gmean, grstd, ggamma, gbeta = gn_ops
                dx = _new_cl(n, cin, hi, wi, x)
                sums = torch.empty(n, L.odvae_conv3x3_wino4_stats_chunks(hi, wi), 2, cin, dtype=torch.float32, device=x.device)
                tag = KERNEL_EVENTS.begin()
                _lib.check(L.odvae_conv3x3_wino4_gnbwd_f32(dy.data_ptr(), n, hi, wi, cout, dgr.data_ptr(), cin, dx.data_ptr(), _cl(gx).data_ptr(),
                                                           gmean.data_ptr(), grstd.data_ptr(), ggamma.data_ptr(), gbeta.data_ptr(),
                                                           lk.groups, sums.data_ptr(), _lib.stream_ptr()), "conv3x3_wino4_gnbwd")
                KERNEL_EVENTS.end("conv3x3_wino4", 2.0 * 9 * cin * cout * n * hi * wi, tag, 4.0 * (n * hi * wi * (2 * cin + cout) + 9 * cin * cout),
                                  issued=2.0 * 2.25 * cin * cout * n * hi * wi, variant="data gradient + GroupNorm-backward sums")
                lk.sums = (sums, _stamp(dx))
            elif dgrad_mode is None:
                dx = _conv3x3_wino_raw(dy, dgr, cout, cin, None, None, f4=route != "wino2")
            else:
                dx = _conv3x3_raw(dgrad_mode, dy, dgr, cout, cin, None, None)   # (mode 6: 4x4-tap stride-2 conv over dy, pre-summed weights)
            if route in ("up_dense", "wino4_up") and not pooled:   # that was the gradient w.r.t. the upsampled image: its 2x2 sum-pool
                du, dx = dx, _new_cl(n, cin, hi, wi, x)
                _lib.check(L.odvae_upsample2x_bwd_f32(du.data_ptr(), dx.data_ptr(), n, hi, wi, cin, _lib.stream_ptr()), "upsample2x_bwd")
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw = torch.empty_like(weight, memory_format=torch.contiguous_format)
            db = torch.empty(cout, dtype=torch.float32, device=x.device) if ctx.has_bias else None
            if mode == 0 and _ops.WGRAD_WINOGRAD and L.odvae_conv3x3_wgrad_wino_supported(n, hi, wi, cin, cout):
                need = L.odvae_conv3x3_wgrad_wino_workspace_bytes(n, hi, wi, cin, cout)
                wp, wn = _ws(need, x)
                tag = KERNEL_EVENTS.begin(secondary=True)
                _lib.check(L.odvae_conv3x3_wgrad_wino_f32(x.data_ptr(), dy.data_ptr(), n, hi, wi, cin, cout,
                                                          dw.data_ptr(), _lib.ptr(db), wp, wn, _lib.stream_ptr()),
                           "conv3x3_wgrad_wino")
                KERNEL_EVENTS.end("conv3x3_wgrad_wino", 2.0 * 9 * cin * cout * n * hi * wi, tag,
                                  4.0 * (n * hi * wi * (cin + cout) + 9 * cin * cout),
                                  issued=2.0 * 4 * cin * cout * n * hi * wi)
            else:
                need = L.odvae_conv3x3_wgrad_workspace_bytes(wgrad_mode, n, ho, wo, cin, cout)
                wp, wn = _ws(need, x)
                _lib.check(L.odvae_conv3x3_wgrad_f32(wgrad_mode, x.data_ptr(), dy.data_ptr(), n, hi, wi, cin, ho, wo, cout,
                                                     dw.data_ptr(), _lib.ptr(db), wp, wn, _lib.stream_ptr()),
                           "conv3x3_wgrad(mode=%d)" % wgrad_mode)
                KERNEL_EVENTS.end("conv3x3_wgrad", 2.0 * 9 * cin * cout * n * ho * wo, None,
                                  issued=_conv_issued(wgrad_mode, n, hi, wi, ho, wo, cin, cout))
        dres = dy if ctx.has_res and ctx.needs_input_grad[3] else None
        return dx, dw, db, dres, None, None, None, None


def conv3x3(x, weight, bias=None, residual=None, mode=0, relu=False, out_f32=False, gn_stats=False):
    """bf16 activations take the mixed-precision kernels (conv_bf16.hip); out_f32 makes that path hand back f32 (the f32 ends of
    the network: encoder.conv_out -> moments, decoder.conv_out -> reconstruction).
    gn_stats=True: the caller says a GroupNorm(32) reads the result next.  Where the F(4x4) kernel takes the layer, its output transform
    then also writes the GroupNorm statistics of y per tile; they travel as the attribute `_gn_partials` of the returned tensor (the
    Python object, so a copy or a view does not carry them) and `group_norm` / `group_norm_skip` use them instead of a statistics pass."""
    if x.dtype == BF16:
        if relu:   # the VGG layers of the bf16 perceptual net (opt-in): conv + ReLU in one launch, a true gradient w.r.t. x
            if residual is not None or mode != 0 or out_f32 or gn_stats:
                raise NotImplementedError("conv3x3(bf16, relu=True): stride 1, no residual, bf16 output (the VGG layer shape)")
            return _ConvReluB.apply(x, weight, bias, False, False)
        if gn_stats and mode == 0 and not out_f32:
            return _tag_gn_partials(*_ConvB.apply(x, weight, bias, residual, mode, False, True))
        return _ConvB.apply(x, weight, bias, residual, mode, bool(out_f32))
    link = _gn_bwd_link_of(x, weight.shape[1]) if (mode == 0 and not relu) else None
    if gn_stats and not relu and mode in (0, 2):
        return _tag_gn_partials(*_Conv3x3.apply(x, weight, bias, residual, mode, relu, True, link))
    return _Conv3x3.apply(x, weight, bias, residual, mode, relu, False, link)


class _Conv1x1(Function):
    """y[M][Cout] = x[M][Cin] . W[Cout][Cin]^T + b (+ residual), M = N*H*W pixels (NHWC)."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual):
        x = _cl(x)
        res = _cl(residual) if residual is not None else None
        n, cin, h, w = x.shape
        cout = weight.shape[0]
        wt = weight.detach().reshape(cout, cin).contiguous()
        b = bias.detach().contiguous() if bias is not None else None
        y = _new_cl(n, cout, h, w, x)
        m = n * h * w
        gemm(0, 1, m, cout, cin, 1.0, x, cin, 0, wt, cin, 0, y, cout, 0, b, res)
        ctx.has_bias = bias is not None
        ctx.has_res = residual is not None
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = _cl(dy)
        n, cin, h, w = x.shape
        cout = weight.shape[0]
        m = n * h * w
        wt = weight.detach().reshape(cout, cin).contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _new_cl(n, cin, h, w, x)
            gemm(0, 0, m, cin, cout, 1.0, dy, cout, 0, wt, cin, 0, dx, cin, 0)
        if ctx.needs_input_grad[1]:
            dw2 = torch.empty(cout, cin, dtype=torch.float32, device=x.device)
            gemm(1, 0, cout, cin, m, 1.0, dy, cout, 0, x, cin, 0, dw2, cin, 0)
            dw = dw2.view(cout, cin, 1, 1)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = _colsum(dy, m, cout)
        dres = dy if ctx.has_res and ctx.needs_input_grad[3] else None
        return dx, dw, db, dres


def conv1x1(x, weight, bias=None, residual=None, out_f32=False):
    """out_f32: bf16 input only -- the result leaves the conv in f32 (no residual then)."""
    if x.dtype == BF16:
        return _ConvB.apply(x, weight, bias, residual, 4, bool(out_f32))
    # (a forward-only call with output channels that are no multiple of 4 -- AutoencoderKL.to_rgb's 3 -- has always run on the GEMM and stays there)
    needs_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, bias, residual))
    if weight.shape[1] % 4 or (weight.shape[0] % 4 and needs_grad):
        # The f32 GEMM stages float4 vectors along the contiguous axis of both operands: the input channels in the forward, the output
        # channels too in the two backward products.  A layer it cannot take (the kl-f4 layout: quant_conv on 6-channel moments,
        # post_quant_conv on the 3-channel latent) runs on the direct 3x3 kernel, which has no such rule, with the weight in the centre tap
        # of an otherwise zero 3x3 stencil: the same sums, and nine times the multiplies of a layer that has a few dozen of them per pixel.
        return conv3x3(x, torch.nn.functional.pad(weight, (1, 1, 1, 1)), bias, residual)
    return _Conv1x1.apply(x, weight, bias, residual)
