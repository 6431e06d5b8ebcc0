"""3x3 / 1x1 convolutions on bf16 activations (conv_bf16.hip, conv_wgrad_bf16.hip) and the f32 -> bf16 hand-off."""
import torch
from torch.autograd import Function

from .. import ops as _ops      # the package: switches and run-time state are read and written there (ops/__init__.py)
from .. import lib as _lib
from ._base import BF16, KERNEL_EVENTS, _L, _cl, _new_cl, _ws
from .packs import pack_conv3x3
from .gn_link import GN_GROUPS
from .gemm import _colsum


# ------------------------------------------------------------------------------------------------------
# bf16 mixed-precision path (BASELINE.json configs[4]): bf16 activations in HBM, f32 master weights / gradients / statistics
# ------------------------------------------------------------------------------------------------------
_I31 = 0x7FFFFFF0


def _conv_b_raw(mode, x, pack, cout, bias, residual, out_f32, cin_alg=None, stats=False):
    """One odvae_conv_bf16 call.  mode 4 (1x1) flattens the pixels to [1][M/wi][wi]; images are processed in groups small enough
    for the 2 GiB buffer descriptors.  cin_alg: the reduction width the algorithm has (3 for conv_in, whose image is zero-padded to
    8 channels): the FLOP / byte figures handed to KERNEL_EVENTS are the direct-form work of SURVEY.md 8(d), not the padded work."""
    L = _L()
    n, cx, hi, wi = x.shape
    if mode in (0, 4):
        ho, wo = hi, wi
    elif mode == 1:
        ho, wo = hi // 2, wi // 2
    else:
        ho, wo = 2 * hi, 2 * wi
    y = _new_cl(n, cout, ho, wo, x, dtype=torch.float32 if out_f32 else BF16)
    esz = 4 if out_f32 else 2
    if mode != 4:
        tag = KERNEL_EVENTS.begin()
        partial = None
        if stats:     # (mode 0, bf16 output) the epilogue also leaves the GroupNorm statistics of y per output tile
            partial = torch.empty(n, L.odvae_conv_bf16_stats_chunks(ho, wo), GN_GROUPS, 2, dtype=torch.float32, device=x.device)
            _lib.check(L.odvae_conv_bf16_stats(x.data_ptr(), n, hi, wi, cx, pack.data_ptr(), cout, _lib.ptr(bias), _lib.ptr(residual),
                                               y.data_ptr(), partial.data_ptr(), GN_GROUPS, _lib.stream_ptr()), "conv_bf16_stats")
        else:
            _lib.check(L.odvae_conv_bf16(mode, x.data_ptr(), n, hi, wi, cx, pack.data_ptr(), cout, _lib.ptr(bias), _lib.ptr(residual),
                                         y.data_ptr(), ho, wo, int(out_f32), _lib.stream_ptr()), "conv_bf16(mode=%d)" % mode)
        ca = cin_alg or cx
        px = hi * wi if mode == 3 else ho * wo     # mode 3 (data gradient of the stride-2 conv): nine taps per LOW-res pixel
        KERNEL_EVENTS.end("conv_bf16", 2.0 * 9 * ca * cout * n * px, tag,
                          2.0 * n * hi * wi * ca + esz * n * ho * wo * cout * (2 if residual is not None else 1) + 2.0 * 9 * ca * cout)
        return (y, partial) if stats else y
    per = hi * wi
    grp = max(1, min(n, _ops.CONV_1X1_GROUP or _I31 // max(per * cx * 2, per * cout * esz)))
    for a in range(0, n, grp):
        b = min(n, a + grp)
        m = (b - a) * per
        w16 = next(d for d in (16, 8, 4, 2, 1) if m % d == 0)
        tag = KERNEL_EVENTS.begin(secondary=True)
        _lib.check(L.odvae_conv_bf16(4, x.data_ptr() + a * per * cx * 2, 1, m // w16, w16, cx, pack.data_ptr(), cout, _lib.ptr(bias),
                                     None if residual is None else residual.data_ptr() + a * per * cout * 2,
                                     y.data_ptr() + a * per * cout * esz, m // w16, w16, int(out_f32), _lib.stream_ptr()), "conv_bf16(1x1)")
        KERNEL_EVENTS.end("conv1x1_bf16", 2.0 * cx * cout * m, tag, 2.0 * m * cx + esz * m * cout)
    return y


def _pad8(c):
    return (c + 7) // 8 * 8


class _ConvB(Function):
    """3x3 (modes 0 / 1 / 2) or 1x1 (mode 4) convolution on bf16 NHWC activations; weight / bias are the f32 master parameters
    (OIHW), their gradients come back in f32.  x may carry zero channels beyond weight.shape[1] (the 3-channel image padded to 8)."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, mode, out_f32, gn_stats=False):
        """gn_stats=True: returns (y, partials) -- partials [N][tiles][32][2], the GroupNorm statistics of y from the conv's own epilogue
        (not differentiable), or None where the kernel does not offer them."""
        L = _L()
        x = _cl(x, BF16)
        res = _cl(residual, BF16) if residual is not None else None
        cout, cin = weight.shape[0], weight.shape[1]
        if x.shape[1] != cin and L.odvae_conv_bf16_reduce_pad(x.shape[1]) != L.odvae_conv_bf16_reduce_pad(cin):
            raise ValueError("conv_bf16: input has %d channels, weight expects %d" % (x.shape[1], cin))
        fwd_pack, dpack = pack_conv3x3(weight, True, bool(ctx.needs_input_grad[0]), "bf16")
        b = bias.detach().contiguous() if bias is not None else None
        partial = None
        if gn_stats and mode == 0 and not out_f32 and _ops.GN_FUSED_STATS and L.odvae_conv_bf16_stats_supported(cout, GN_GROUPS):
            y, partial = _conv_b_raw(mode, x, fwd_pack, cout, b, res, out_f32, cin_alg=cin, stats=True)
        else:
            y = _conv_b_raw(mode, x, fwd_pack, cout, b, res, out_f32, cin_alg=cin)
        ctx.mode, ctx.has_bias, ctx.has_res, ctx.dpack = mode, bias is not None, residual is not None, dpack
        ctx.pack_epoch = _ops.PACK_CACHE.epoch
        ctx.wshape = tuple(weight.shape)
        ctx.save_for_backward(x)
        if gn_stats:
            if partial is not None:
                ctx.mark_non_differentiable(partial)
            ctx.set_materialize_grads(False)   # (as _Conv3x3: no tensor of zeros for the statistics output)
            return y, partial
        return y

    @staticmethod
    def backward(ctx, dy, _dpartial=None):
        L = _L()
        if dy is None:
            return None, None, None, None, None, None, None
        (x,) = ctx.saved_tensors
        mode = ctx.mode
        cout, cin = ctx.wshape[0], ctx.wshape[1]
        n, cx, hi, wi = x.shape
        _, _, ho, wo = dy.shape
        dyb, cp = dy, cout
        if dy.dtype != BF16:                 # f32 upstream gradient (reconstruction / moments): one cast (+ channel pad) pass
            cp = _pad8(cout)
            dyb = cast_pad_bf16(_cl(dy), cp)
        else:
            dyb = _cl(dy, BF16)
        dx = dw = db = None
        if ctx.needs_input_grad[0] and not _ops.WEIGHT_GRADIENT_ONLY:
            if cx != cin:
                raise NotImplementedError("data gradient through a channel-padded input")
            _ops.PACK_CACHE.check_epoch(ctx.pack_epoch, "conv_bf16 backward")
            if mode == 0:
                dx = _conv_b_raw(0, dyb, ctx.dpack, cin, None, None, False)
            elif mode == 1:
                dx = _conv_b_raw(3, dyb, ctx.dpack, cin, None, None, False)
            elif mode == 4:
                dx = _conv_b_raw(4, dyb, ctx.dpack, cin, None, None, False)
            else:                            # Upsample: gradient w.r.t. the upsampled image, then its 2x2 sum-pool
                du = _conv_b_raw(0, dyb, ctx.dpack, cin, None, None, False)
                dx = _new_cl(n, cin, hi, wi, x, dtype=BF16)
                _lib.check(L.odvae_upsample2x_bwd_bf16(du.data_ptr(), dx.data_ptr(), n, hi, wi, cin, _lib.stream_ptr()), "upsample2x_bwd_bf16")
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        fold_db = want_db and dy.dtype == BF16 and ctx.needs_input_grad[1]   # bias gradient rides in the weight-gradient pass over dy
        if ctx.needs_input_grad[1]:
            taps = ctx.wshape[2] * ctx.wshape[3]
            dwf = torch.empty((cp, cx) + tuple(ctx.wshape[2:]), dtype=torch.float32, device=x.device)
            dbf = torch.empty(cp, dtype=torch.float32, device=x.device) if fold_db else None
            def _wgrad(xg, dyg, geo, ng, dw_out, db_out):
                need = L.odvae_conv_wgrad_bf16_workspace_bytes(mode, geo[0], geo[4], geo[5], cx, cp)
                wp, wn = _ws(need, x)
                tag = KERNEL_EVENTS.begin(secondary=True)
                _lib.check(L.odvae_conv_wgrad_bf16(mode, xg.data_ptr(), dyg.data_ptr(), *geo, dw_out.data_ptr(), _lib.ptr(db_out), wp, wn,
                                                   _lib.stream_ptr()), "conv_wgrad_bf16(mode=%d)" % mode)
                KERNEL_EVENTS.end("conv_wgrad_bf16", 2.0 * taps * cx * cp * ng * ho * wo, tag, 2.0 * ng * (hi * wi * cx + ho * wo * cp))

            if mode == 4:
                # a 1x1 conv is one [pixels x cx]^T [pixels x cp] product; the kernel addresses with 32-bit offsets, so image groups
                # of under 2 GiB are reduced one after the other (the same split the forward / data-gradient take in _conv_b_raw)
                per = hi * wi
                grp = max(1, min(n, _ops.WGRAD_1X1_GROUP or _I31 // (per * max(cx, cp) * 2)))
                for g0 in range(0, n, grp):
                    ng = min(grp, n - g0)
                    m = ng * per
                    w16 = next(d for d in (16, 8, 4, 2, 1) if m % d == 0)
                    geo = (1, m // w16, w16, cx, m // w16, w16, cp)
                    if g0 == 0:
                        _wgrad(x[g0:g0 + ng], dyb[g0:g0 + ng], geo, ng, dwf, dbf)
                    else:
                        dw_part = torch.empty_like(dwf)
                        db_part = torch.empty_like(dbf) if fold_db else None
                        _wgrad(x[g0:g0 + ng], dyb[g0:g0 + ng], geo, ng, dw_part, db_part)
                        dwf += dw_part
                        if fold_db:
                            dbf += db_part
            else:
                _wgrad(x, dyb, (n, hi, wi, cx, ho, wo, cp), n, dwf, dbf)
            dw = dwf if (cp == cout and cx == cin) else dwf[:cout, :cin].contiguous()
            if fold_db:
                db = dbf if cp == cout else dbf[:cout].contiguous()
        if want_db and not fold_db:
            if dy.dtype != BF16:   # f32 upstream gradient (reconstruction / moments): sum the f32 values themselves
                db = _colsum(_cl(dy), n * ho * wo, cout)
            else:
                db = torch.empty(cout, dtype=torch.float32, device=x.device)
                rows = n * ho * wo
                wp, wn = _ws(L.odvae_colsum_bf16_workspace_bytes(rows, cout), x)
                _lib.check(L.odvae_colsum_bf16(dyb.data_ptr(), rows, cout, db.data_ptr(), wp, wn, _lib.stream_ptr()), "colsum_bf16")
        dres = dyb if ctx.has_res and ctx.needs_input_grad[3] else None
        return dx, dw, db, dres, None, None, None


def cast_pad_bf16(x, cp=None):
    """bf16 NHWC copy of an f32 NHWC tensor, channels zero-padded to cp (raw, no autograd)."""
    L = _L()
    n, c, h, w = x.shape
    cp = c if cp is None else cp
    y = _new_cl(n, cp, h, w, x, dtype=BF16)
    _lib.check(L.odvae_cast_pad_bf16(x.data_ptr(), n * h * w, c, cp, y.data_ptr(), _lib.stream_ptr()), "cast_pad_bf16")
    return y


class _ToBF16(Function):
    """f32 -> bf16 hand-off into the mixed-precision network (optionally zero-padding the channels to a multiple of 8); the
    gradient comes back as f32 on the original channels."""

    @staticmethod
    def forward(ctx, x, cp):
        x = _cl(x)
        ctx.c = x.shape[1]
        return cast_pad_bf16(x, cp)

    @staticmethod
    def backward(ctx, dy):
        L = _L()
        dy = _cl(dy, BF16)
        n, cp, h, w = dy.shape
        dx = _new_cl(n, cp, h, w, dy)
        _lib.check(L.odvae_cast_f32_from_bf16(dy.data_ptr(), dy.numel(), dx.data_ptr(), _lib.stream_ptr()), "cast_f32_from_bf16")
        return (dx if cp == ctx.c else dx[:, :ctx.c]), None


def to_bf16(x, pad_channels_to=None):
    if x.dtype == BF16:
        return x
    c = x.shape[1]
    cp = c if pad_channels_to is None else max(c, (c + pad_channels_to - 1) // pad_channels_to * pad_channels_to)
    return _ToBF16.apply(x, cp)
