"""2x2 average pool and nearest 2x upsample, f32 and bf16 (the conv-less resamplers)."""
import collections

import torch
from torch.autograd import Function

from .. import lib as _lib
from ._base import BF16, CL, KERNEL_EVENTS, _L, _cl, _new_cl
from .gn_link import GN_GROUPS, _gn_stats_ok, _tag_gn_partials


# ------------------------------------------------------------------------------------------------------
# conv-less resamplers (ddconfig.resamp_with_conv = False) and the decoder's tanh_out
# ------------------------------------------------------------------------------------------------------
# Per-dtype description of the resampler Functions: dtype, bytes per element, entry points (by name), the chunk count _gn_partials_of expects
# for a tensor of this dtype
_RsKind = collections.namedtuple("_RsKind", "dtype esz pool pool_bwd up up_bwd chunks suffix")
_RS_F32 = _RsKind(torch.float32, 4.0, "odvae_avgpool2x2_f32", "odvae_avgpool2x2_bwd_f32", "odvae_upsample2x_f32", "odvae_upsample2x_bwd_f32",
                  "odvae_conv3x3_wino4_stats_chunks", "")
_RS_BF16 = _RsKind(BF16, 2.0, "odvae_avgpool2x2_bf16", "odvae_avgpool2x2_bwd_bf16", "odvae_upsample2x_bf16", "odvae_upsample2x_bwd_bf16",
                   "odvae_conv_bf16_stats_chunks", "_bf16")


def _rs_in(kind, t):
    """NHWC view with the 16-byte aligned base the resamplers' vector accesses need."""
    t = _cl(t, kind.dtype)
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=CL)


def _rs_forward(kind, ctx, x, up, gn_stats):
    """up: nearest 2x, else 2x2 average pool.  gn_stats: returns (y, partials [N][chunks][32][2]) -- the GroupNorm statistics of y from the
    same pass, not differentiable -- where _gn_stats_ok(C), (y, None) otherwise."""
    L = _L()
    x = _rs_in(kind, x)
    n, c, h, w = x.shape
    ho, wo = (2 * h, 2 * w) if up else (h // 2, w // 2)
    y = _new_cl(n, c, ho, wo, x, dtype=kind.dtype)
    partial = None
    if gn_stats and _gn_stats_ok(c):
        partial = torch.empty(n, getattr(L, kind.chunks)(ho, wo), GN_GROUPS, 2, dtype=torch.float32, device=x.device)
    tag = KERNEL_EVENTS.begin(secondary=True)
    _lib.check(getattr(L, kind.up if up else kind.pool)(x.data_ptr(), y.data_ptr(), n, h, w, c, _lib.ptr(partial), GN_GROUPS if partial is not None else 0,
                                                        int(partial.shape[1]) if partial is not None else 0, _lib.stream_ptr()),
               ("upsample2x" if up else "avgpool2x2") + kind.suffix)
    # algorithmic traffic: every input vector the result depends on read once, the result written once
    KERNEL_EVENTS.end("upsample2x" if up else "avgpool2x2", 0.0, tag, kind.esz * n * c * (h * w + ho * wo if up else 5 * ho * wo), issued=0.0)
    ctx.in_hw = (h, w)
    if gn_stats:
        if partial is not None:
            ctx.mark_non_differentiable(partial)
        ctx.set_materialize_grads(False)
        return y, partial
    return y


def _rs_backward(kind, ctx, dy, up):
    L = _L()
    if dy is None:
        return None
    dy = _rs_in(kind, dy)
    n, c = dy.shape[0], dy.shape[1]
    h, w = ctx.in_hw
    dx = _new_cl(n, c, h, w, dy, dtype=kind.dtype)
    tag = KERNEL_EVENTS.begin(secondary=True)
    _lib.check(getattr(L, kind.up_bwd if up else kind.pool_bwd)(dy.data_ptr(), dx.data_ptr(), n, h, w, c, _lib.stream_ptr()),
               ("upsample2x_bwd" if up else "avgpool2x2_bwd") + kind.suffix)
    KERNEL_EVENTS.end("upsample2x" if up else "avgpool2x2", 0.0, tag, kind.esz * (dy.numel() + dx.numel()), issued=0.0)
    return dx


class _AvgPool2x2(Function):
    @staticmethod
    def forward(ctx, x, gn_stats=False):
        return _rs_forward(_RS_F32, ctx, x, False, gn_stats)

    @staticmethod
    def backward(ctx, dy, _dpartial=None):
        return _rs_backward(_RS_F32, ctx, dy, False), None


class _AvgPool2x2B(Function):
    """On bf16 activations: f32 arithmetic, one rounding on the way out."""

    @staticmethod
    def forward(ctx, x, gn_stats=False):
        return _rs_forward(_RS_BF16, ctx, x, False, gn_stats)

    @staticmethod
    def backward(ctx, dy, _dpartial=None):
        return _rs_backward(_RS_BF16, ctx, dy, False), None


class _Upsample2x(Function):
    @staticmethod
    def forward(ctx, x, gn_stats=False):
        return _rs_forward(_RS_F32, ctx, x, True, gn_stats)

    @staticmethod
    def backward(ctx, dy, _dpartial=None):
        return _rs_backward(_RS_F32, ctx, dy, True), None


class _Upsample2xB(Function):
    @staticmethod
    def forward(ctx, x, gn_stats=False):
        return _rs_forward(_RS_BF16, ctx, x, True, gn_stats)

    @staticmethod
    def backward(ctx, dy, _dpartial=None):
        return _rs_backward(_RS_BF16, ctx, dy, True), None


def avg_pool2x2(x, gn_stats=False):
    """F.avg_pool2d(x, 2, 2) (Downsample(with_conv=False)); an odd last row / column is dropped.  gn_stats=True: the caller says a
    GroupNorm(32) reads the result next -- where _gn_stats_ok(C), the same pass leaves the GroupNorm statistics of the result, which travel
    as `_gn_partials` on the returned tensor the way conv3x3(gn_stats=True) leaves them."""
    fn = _AvgPool2x2B if x.dtype == BF16 else _AvgPool2x2
    if gn_stats:
        return _tag_gn_partials(*fn.apply(x, True))
    return fn.apply(x)


def upsample2x(x, gn_stats=False):
    """F.interpolate(x, scale_factor=2.0, mode="nearest") (Upsample(with_conv=False)); gn_stats as avg_pool2x2 (the statistics of the
    upsampled tensor are four times those of x: the kernel sums its input once)."""
    fn = _Upsample2xB if x.dtype == BF16 else _Upsample2x
    if gn_stats:
        return _tag_gn_partials(*fn.apply(x, True))
    return fn.apply(x)
