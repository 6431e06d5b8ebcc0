"""Streaming ops: tanh, input rescale, Gaussian sample / KL, masked L1, layout copy, masks, the pose losses and the pose MLPs' dense layer."""
import torch
from torch.autograd import Function

from .. import lib as _lib
from ._base import CL, KERNEL_EVENTS, _L, _cl, _new_cl, _ws
from .gemm import _colsum


class _Tanh(Function):
    """Decoder(tanh_out=True): elementwise on the f32 reconstruction, any layout (the kernels see a flat array); the backward keeps y only."""

    @staticmethod
    def forward(ctx, x):
        L = _L()
        _lib.require_device(x)
        if not (x.is_contiguous() or (x.dim() == 4 and x.is_contiguous(memory_format=CL))):
            x = x.contiguous()
        y = torch.empty_like(x)      # (preserve_format: the same dense layout as x)
        if y.stride() != x.stride():
            x = x.contiguous()
            y = torch.empty_like(x)
        tag = KERNEL_EVENTS.begin(secondary=True)
        _lib.check(L.odvae_tanh_f32(x.data_ptr(), y.data_ptr(), x.numel(), _lib.stream_ptr()), "tanh")
        KERNEL_EVENTS.end("tanh", 0.0, tag, 8.0 * x.numel(), issued=0.0)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _L()
        (y,) = ctx.saved_tensors
        _lib.require_device(dy)
        if dy.stride() != y.stride():
            dy = torch.empty_like(y).copy_(dy)
        dx = torch.empty_like(y)
        tag = KERNEL_EVENTS.begin(secondary=True)
        _lib.check(L.odvae_tanh_bwd_f32(y.data_ptr(), dy.data_ptr(), dx.data_ptr(), y.numel(), _lib.stream_ptr()), "tanh_bwd")
        KERNEL_EVENTS.end("tanh", 0.0, tag, 12.0 * y.numel(), issued=0.0)
        return dx


def tanh(x):
    return _Tanh.apply(x)


# ------------------------------------------------------------------------------------------------------
# input rescale, posterior, reconstruction term
# ------------------------------------------------------------------------------------------------------
def rescale_minmax(x_nchw):
    """2(x-min)/(max-min)-1 over the whole local batch (src/models/autoencoder.py:434-436); returns NHWC memory."""
    L = _L()
    _lib.require_device(x_nchw)
    x = x_nchw.detach().contiguous()
    n, c, h, w = x.shape
    y = _new_cl(n, c, h, w, x)
    mm = torch.empty(2, dtype=torch.float32, device=x.device)
    wp, wn = _ws(16384, x)
    _lib.check(L.odvae_rescale_minmax_f32(x.data_ptr(), y.data_ptr(), n, c, h * w, mm.data_ptr(), wp, wn,
                                          _lib.stream_ptr()), "rescale_minmax")
    return y


class _GaussianSample(Function):
    @staticmethod
    def forward(ctx, moments, eps):
        L = _L()
        moments = _cl(moments)
        eps = _cl(eps)
        n, c2, h, w = moments.shape
        cz = c2 // 2
        z = _new_cl(n, cz, h, w, moments)
        _lib.check(L.odvae_gaussian_sample_f32(moments.data_ptr(), eps.data_ptr(), z.data_ptr(), n, h * w, cz,
                                               _lib.stream_ptr()), "gaussian_sample")
        ctx.save_for_backward(moments, eps)
        return z

    @staticmethod
    def backward(ctx, dz):
        L = _L()
        moments, eps = ctx.saved_tensors
        dz = _cl(dz)
        n, c2, h, w = moments.shape
        dm = _new_cl(n, c2, h, w, moments)
        _lib.check(L.odvae_gaussian_bwd_f32(moments.data_ptr(), eps.data_ptr(), dz.data_ptr(), None, dm.data_ptr(),
                                            n, h * w, c2 // 2, _lib.stream_ptr()), "gaussian_bwd(sample)")
        return dm, None


class _GaussianKL(Function):
    @staticmethod
    def forward(ctx, moments):
        L = _L()
        moments = _cl(moments)
        n, c2, h, w = moments.shape
        kl = torch.empty(n, dtype=torch.float32, device=moments.device)
        _lib.check(L.odvae_gaussian_kl_f32(moments.data_ptr(), kl.data_ptr(), n, h * w, c2 // 2, _lib.stream_ptr()),
                   "gaussian_kl")
        ctx.save_for_backward(moments)
        return kl

    @staticmethod
    def backward(ctx, dkl):
        L = _L()
        (moments,) = ctx.saved_tensors
        n, c2, h, w = moments.shape
        dkl = dkl.contiguous()
        dm = _new_cl(n, c2, h, w, moments)
        _lib.check(L.odvae_gaussian_bwd_f32(moments.data_ptr(), None, None, dkl.data_ptr(), dm.data_ptr(),
                                            n, h * w, c2 // 2, _lib.stream_ptr()), "gaussian_bwd(kl)")
        return dm


def gaussian_sample(moments, eps):
    return _GaussianSample.apply(moments, eps)


def gaussian_kl(moments):
    return _GaussianKL.apply(moments)


class _L1MaskedSum(Function):
    """per-sample sum |x*m - xr*m| (contperceptual.py:137 with the mask_2d_bbox products of :252-255 folded in)."""

    @staticmethod
    def forward(ctx, x, xr, mask):
        L = _L()
        x = _cl(x)
        xr = _cl(xr)
        n, c, h, w = x.shape
        m = mask.detach().reshape(n, h * w).contiguous() if mask is not None else None
        _lib.require_device(m)
        out = torch.empty(n, dtype=torch.float32, device=x.device)
        wp, wn = _ws(n * 1024, x)
        _lib.check(L.odvae_l1_masked_sum_f32(x.data_ptr(), xr.data_ptr(), _lib.ptr(m), out.data_ptr(), n, h * w, c,
                                             wp, wn, _lib.stream_ptr()), "l1_masked_sum")
        ctx.save_for_backward(x, xr, m)
        return out

    @staticmethod
    def backward(ctx, g):
        L = _L()
        x, xr, m = ctx.saved_tensors
        n, c, h, w = x.shape
        g = g.contiguous()
        dxr = _new_cl(n, c, h, w, x)
        _lib.check(L.odvae_l1_masked_bwd_f32(x.data_ptr(), xr.data_ptr(), _lib.ptr(m), g.data_ptr(), dxr.data_ptr(),
                                             n, h * w, c, _lib.stream_ptr()), "l1_masked_bwd")
        return None, dxr, None


def l1_masked_sum(x, xr, mask=None):
    return _L1MaskedSum.apply(x, xr, mask)


def _aligned16(t):
    """`t` itself, or a copy of the same strides where its base is not 16-byte aligned (a view into a larger buffer)."""
    return t if t.data_ptr() % 16 == 0 else torch.empty_like(t).copy_(t)


class _RgbaTerms(Function):
    """image_mask_key: every reconstruction-side term of PoseLoss on a 4-channel reconstruction from one pass (contperceptual.py:230-257):
    the per-sample L1 sums over RGB, the per-sample mask-loss sums over alpha, and the box-masked copies the LPIPS-style net (RGB) and the
    discriminator (RGBA) read.  Differentiable w.r.t. `rec` alone; the backward is one pass as well."""

    @staticmethod
    def forward(ctx, rec, rgb_gt, mask_gt, box, l2, want, sums):
        L = _L()
        rec = _aligned16(_cl(rec))
        rgb = _cl(rgb_gt.detach())
        n, c, h, w = rec.shape
        if c != 4 or tuple(rgb.shape) != (n, 3, h, w) or mask_gt.numel() != n * h * w or (box is not None and box.numel() != n * h * w):
            raise ValueError("rgba_terms: rec %s, rgb_gt %s, mask_gt %s, box %s" % (tuple(rec.shape), tuple(rgb.shape), tuple(mask_gt.shape),
                                                                                    None if box is None else tuple(box.shape)))
        a = mask_gt.detach().to(rec.device).float().reshape(n, h * w).contiguous()
        m = box.detach().to(rec.device).float().reshape(n, h * w).contiguous() if box is not None else None
        _lib.require_device(a, *(() if m is None else (m,)))
        l1_sums = torch.empty(n, dtype=torch.float32, device=rec.device) if sums else None
        mask_sums = torch.empty(n, dtype=torch.float32, device=rec.device) if sums else None
        outs = [(_new_cl(n, cc, h, w, rec) if flag else None) for flag, cc in zip(want, (3, 3, 4, 4))]
        wp, wn = _ws(L.odvae_rgba_terms_workspace_bytes(n), rec) if sums else (None, 0)
        _lib.check(L.odvae_rgba_terms_f32(rec.data_ptr(), rgb.data_ptr(), a.data_ptr(), _lib.ptr(m), int(l2), _lib.ptr(l1_sums),
                                          _lib.ptr(mask_sums), _lib.ptr(outs[0]), _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.ptr(outs[3]),
                                          n, h * w, wp, wn, _lib.stream_ptr()), "rgba_terms")
        ctx.save_for_backward(rec, rgb, a, m)
        ctx.l2 = int(l2)
        ctx.set_materialize_grads(False)      # an output nobody differentiated arrives as None, and its term is skipped
        ctx.mark_non_differentiable(*[t for t in (outs[1], outs[3]) if t is not None])      # the target's copies (one call: a second replaces it)
        return (l1_sums, mask_sums) + tuple(outs)

    @staticmethod
    def backward(ctx, g_l1, g_mask, g_rgb, _g_gt_rgb, g_rgba, _g_gt_rgba):
        L = _L()
        rec, rgb, a, m = ctx.saved_tensors
        n, c, h, w = rec.shape
        g_l1 = None if g_l1 is None else g_l1.contiguous()
        g_mask = None if g_mask is None else g_mask.contiguous()
        g_rgb = None if g_rgb is None else _cl(g_rgb)
        g_rgba = None if g_rgba is None else _aligned16(_cl(g_rgba))
        d_rec = _new_cl(n, 4, h, w, rec)
        _lib.check(L.odvae_rgba_terms_bwd_f32(rec.data_ptr(), rgb.data_ptr(), a.data_ptr(), _lib.ptr(m), ctx.l2, _lib.ptr(g_l1), _lib.ptr(g_mask),
                                              _lib.ptr(g_rgb), _lib.ptr(g_rgba), d_rec.data_ptr(), n, h * w, _lib.stream_ptr()), "rgba_terms_bwd")
        return d_rec, None, None, None, None, None, None


def rgba_terms(rec, rgb_gt, mask_gt, box=None, l2=False, rec_rgb_m=False, gt_rgb_m=False, rec_rgba_m=False, gt_rgba_m=False, sums=True):
    """(l1_sums [N], mask_sums [N], rec_rgb_m, gt_rgb_m, rec_rgba_m, gt_rgba_m) of a 4-channel reconstruction: sum |rgb_gt*box - rec[:, :3]*box|
    and sum of |mask_gt*box - rec[:, 3:]*box| (or its square, l2) per sample, and those of the four box-masked tensors that were asked for
    (None otherwise): rec[:, :3]*box, rgb_gt*box, rec*box, cat(rgb_gt, mask_gt)*box, all NHWC in memory.  sums=False: the two sums are
    None and not computed (no reduction, no second launch)."""
    return _RgbaTerms.apply(rec, rgb_gt, mask_gt, box, l2, (bool(rec_rgb_m), bool(gt_rgb_m), bool(rec_rgba_m), bool(gt_rgba_m)), bool(sums))


WEIGHT_LAYOUTS = ("scalar", "sample", "pixel", "element")


def loss_weights_layout(weights, n, c, h, w):
    """(layout, tensor) of a loss's `weights` argument against rec_loss [n, c, h, w] -- the one place that classifies it.  layout:
    "scalar" (a number or a one-element tensor; tensor: 0-d), "sample" (a 1-D [n] tensor -- this project's reading of one weight per
    sample -- or anything that broadcasts as [n,1,1,1]; tensor: [n]), "pixel" ([n or 1, 1, h, w]; tensor: a [n,1,h,w] view) or "element"
    (anything else that broadcasts to exactly [n,c,h,w]; tensor: a [n,c,h,w] view).  Needs no device.  A shape that does not broadcast to
    [n,c,h,w], or weights that require grad, raise ValueError."""
    target = (int(n), int(c), int(h), int(w))
    t = weights if torch.is_tensor(weights) else torch.as_tensor(weights, dtype=torch.float32)
    if t.requires_grad:
        raise ValueError("weights requires grad: the losses treat weights as a constant (detach it, or scale the loss instead)")
    if t.numel() == 1:
        return "scalar", t.reshape(())
    shape = tuple(t.shape)
    if shape == (target[0],):
        return "sample", t
    refuse = ValueError("weights of shape %s do not broadcast to the reconstruction loss's %s" % (shape, target))
    if len(shape) > 4:
        raise refuse
    padded = (1,) * (4 - len(shape)) + shape
    if any(p not in (1, q) for p, q in zip(padded, target)):
        raise refuse
    if padded == (target[0], 1, 1, 1):
        return "sample", t.reshape(target[0])
    t4 = t.reshape(padded)
    if padded[1] == 1 and padded[2:] == target[2:]:
        return "pixel", t4.expand(target[0], 1, target[2], target[3])
    return "element", t4.expand(target)


class _L1WeightedSums(Function):
    """Per-sample sums of |x*box - xr*box|, of weights * that and of the weights themselves from one pass (odvae_l1_weighted_sums_f32).
    wgt arrives flat: [N][HW] or, per_channel, [N][HW][C].  Differentiable w.r.t. xr alone; the backward is one launch."""

    @staticmethod
    def forward(ctx, x, xr, box, wgt, per_channel, want_l1, shape):
        L = _L()
        n, c, h, w = shape
        _lib.require_device(wgt)
        dev = wgt.device
        w_sums = torch.empty(n, dtype=torch.float32, device=dev)
        wp, wn = _ws(L.odvae_l1_weighted_workspace_bytes(n), wgt)
        if x is None:      # the pixel term is off: the weight sums alone
            _lib.check(L.odvae_l1_weighted_sums_f32(None, None, None, wgt.data_ptr(), int(per_channel), None, None, w_sums.data_ptr(),
                                                    n, h * w, c, c, wp, wn, _lib.stream_ptr()), "l1_weighted_sums")
            ctx.mark_non_differentiable(w_sums)
            return None, None, w_sums
        x = _cl(x.detach())
        xr = _cl(xr)
        cr = xr.shape[1]
        if tuple(x.shape) != (n, c, h, w) or cr < c or (xr.shape[0], xr.shape[2], xr.shape[3]) != (n, h, w) or (box is not None and box.numel() != n * h * w):
            raise ValueError("l1_weighted_sums: x %s, xr %s, box %s" % (tuple(x.shape), tuple(xr.shape), None if box is None else tuple(box.shape)))
        m = box.detach().to(dev).float().reshape(n, h * w).contiguous() if box is not None else None
        _lib.require_device(m)
        l1_sums = torch.empty(n, dtype=torch.float32, device=dev) if want_l1 else None
        wl1_sums = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.check(L.odvae_l1_weighted_sums_f32(x.data_ptr(), xr.data_ptr(), _lib.ptr(m), wgt.data_ptr(), int(per_channel), _lib.ptr(l1_sums),
                                                wl1_sums.data_ptr(), w_sums.data_ptr(), n, h * w, c, cr, wp, wn, _lib.stream_ptr()),
                   "l1_weighted_sums")
        ctx.save_for_backward(x, xr, m, wgt)
        ctx.per_channel = int(per_channel)
        ctx.set_materialize_grads(False)      # a sum nobody differentiated arrives as None, and its term is skipped
        ctx.mark_non_differentiable(w_sums)
        return l1_sums, wl1_sums, w_sums

    @staticmethod
    def backward(ctx, g_l1, g_wl1, _g_w):
        L = _L()
        if g_l1 is None and g_wl1 is None:
            return (None,) * 7
        x, xr, m, wgt = ctx.saved_tensors
        n, c, h, w = x.shape
        cr = xr.shape[1]
        g_l1 = None if g_l1 is None else g_l1.contiguous()
        g_wl1 = None if g_wl1 is None else g_wl1.contiguous()
        dxr = _new_cl(n, cr, h, w, xr)
        _lib.check(L.odvae_l1_weighted_bwd_f32(x.data_ptr(), xr.data_ptr(), _lib.ptr(m), wgt.data_ptr(), ctx.per_channel, _lib.ptr(g_l1),
                                               _lib.ptr(g_wl1), dxr.data_ptr(), n, h * w, c, cr, _lib.stream_ptr()), "l1_weighted_bwd")
        return None, dxr, None, None, None, None, None


def l1_weighted_sums(x, xr, box, weights, want_l1=True, shape=None, device=None):
    """(l1_sums | None, wl1_sums, w_sums), each [N]: per sample, sum |x*box - xr*box|, sum weights * |x*box - xr*box| and sum weights
    (broadcast against [N,C,H,W], NOT box-masked).  weights: a per-pixel or per-element map in the sense of loss_weights_layout.  xr may
    have more channels than x: only its first C are read, in place.  x = xr = None with shape=(n, c, h, w) and the device to compute on
    (default: the weights'): (None, None, w_sums)."""
    n, c, h, w = tuple(x.shape) if x is not None else tuple(shape)
    layout, wt = loss_weights_layout(weights, n, c, h, w)
    if layout not in ("pixel", "element"):
        raise ValueError("l1_weighted_sums: %s weights need no weight map (scale the per-sample sums instead)" % layout)
    dev = x.device if x is not None else (wt.device if device is None else torch.device(device))
    wt = wt.detach().to(dev).float()
    wgt = wt.reshape(n, h * w).contiguous() if layout == "pixel" else wt.permute(0, 2, 3, 1).contiguous()
    if x is None:
        xr = box = None
    return _L1WeightedSums.apply(x, xr, box, wgt, layout == "element", bool(want_l1), (n, c, h, w))


class _CatMask(Function):
    """cat(x * box, cond) along the channels in one pass (odvae_cat_mask_f32); gradient to x only."""

    @staticmethod
    def forward(ctx, x, box, cond):
        L = _L()
        x = _cl(x)
        n, cx, h, w = x.shape
        cc = cond.shape[1]
        cond = _cl(cond)
        m = box.detach().to(x.device).float().reshape(n, h * w).contiguous() if box is not None else None
        _lib.require_device(m)
        y = _new_cl(n, cx + cc, h, w, x)
        _lib.check(L.odvae_cat_mask_f32(x.data_ptr(), _lib.ptr(m), cond.data_ptr(), y.data_ptr(), n, h * w, cx, cc, _lib.stream_ptr()), "cat_mask")
        ctx.save_for_backward(m)
        ctx.dims = (n, cx, cc, h, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _L()
        (m,) = ctx.saved_tensors
        n, cx, cc, h, w = ctx.dims
        dy = _cl(dy)
        dx = _new_cl(n, cx, h, w, dy)
        _lib.check(L.odvae_cat_mask_bwd_f32(dy.data_ptr(), _lib.ptr(m), dx.data_ptr(), n, h * w, cx, cc, _lib.stream_ptr()), "cat_mask_bwd")
        return dx, None, None


def cat_mask(x, box, cond):
    """torch.cat((x * box, cond), dim=1) for the conditional discriminator: x [N,Cx,H,W], box [N,1,H,W] or None (= 1), cond [N,Cc,H,W]
    (float, bool or uint8, any device; never multiplied by box, never differentiated).  cond None: ops.mul_mask(x, box)."""
    if cond is None:
        return mul_mask(x, box)
    if not torch.is_tensor(cond) or cond.dim() != 4 or x.dim() != 4 or (cond.shape[0], cond.shape[2], cond.shape[3]) != (x.shape[0], x.shape[2], x.shape[3]) or cond.shape[1] < 1:
        raise ValueError("cond must be [B,Cc,H,W] matching the discriminator input %s, got %s"
                         % (tuple(x.shape), tuple(cond.shape) if torch.is_tensor(cond) else type(cond)))
    if cond.requires_grad:
        raise ValueError("cond requires grad: the conditional discriminator's side channel is not differentiated (detach it)")
    if box is not None and box.numel() != x.shape[0] * x.shape[2] * x.shape[3]:
        raise ValueError("cat_mask: box %s does not match x %s" % (tuple(box.shape), tuple(x.shape)))
    return _CatMask.apply(x, box, cond.to(x.device).float())


def nhwc_to_nchw(x):
    """Contiguous NCHW copy of an NHWC-in-memory tensor (hand-off to NCHW consumers)."""
    L = _L()
    x = _cl(x)
    n, c, h, w = x.shape
    y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    _lib.check(L.odvae_nhwc_to_nchw_f32(x.data_ptr(), y.data_ptr(), n, c, h * w, _lib.stream_ptr()), "nhwc_to_nchw")
    return y


class _MulMask(Function):
    @staticmethod
    def forward(ctx, x, mask):
        L = _L()
        x = _cl(x)
        n, c, h, w = x.shape
        m = mask.detach().to(x.device).float().reshape(n, h * w).contiguous()
        y = _new_cl(n, c, h, w, x)
        _lib.check(L.odvae_mul_mask_f32(x.data_ptr(), m.data_ptr(), y.data_ptr(), n * h * w, c, _lib.stream_ptr()), "mul_mask")
        ctx.save_for_backward(m)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = _L()
        (m,) = ctx.saved_tensors
        dy = _cl(dy)
        n, c, h, w = dy.shape
        dx = _new_cl(n, c, h, w, dy)
        _lib.check(L.odvae_mul_mask_f32(dy.data_ptr(), m.data_ptr(), dx.data_ptr(), n * h * w, c, _lib.stream_ptr()), "mul_mask bwd")
        return dx, None


def mul_mask(x, mask):
    """x * mask_2d_bbox ([B,1,H,W]); identity when mask is None."""
    return x if mask is None else _MulMask.apply(x, mask)


class _LatentCombine(Function):
    """z * mask + add on the latent (dropout keep-mask already scaled by 1/(1-p); noise or enc_pose as `add`)."""

    @staticmethod
    def forward(ctx, z, mask, add):
        L = _L()
        z = _cl(z)
        m = _cl(mask) if mask is not None else None
        a = _cl(add) if add is not None else None
        n, c, h, w = z.shape
        out = _new_cl(n, c, h, w, z)
        _lib.check(L.odvae_latent_combine_f32(z.data_ptr(), _lib.ptr(m), _lib.ptr(a), out.data_ptr(), z.numel(),
                                              _lib.stream_ptr()), "latent_combine")
        ctx.save_for_backward(m)
        ctx.has_add = add is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        L = _L()
        (m,) = ctx.saved_tensors
        dout = _cl(dout)
        dz = dout
        if m is not None and ctx.needs_input_grad[0]:
            n, c, h, w = dout.shape
            dz = _new_cl(n, c, h, w, dout)
            _lib.check(L.odvae_latent_combine_f32(dout.data_ptr(), m.data_ptr(), None, dz.data_ptr(), dout.numel(),
                                                  _lib.stream_ptr()), "latent_combine bwd")
        return dz, None, (dout if ctx.has_add and ctx.needs_input_grad[2] else None)


def latent_combine(z, mask=None, add=None):
    return _LatentCombine.apply(z, mask, add)


# ------------------------------------------------------------------------------------------------------
# device-side latent noise (latent_noise.hip; latent_noise.py is the draw's numpy mirror)
# ------------------------------------------------------------------------------------------------------
LATENT_SAMPLE, LATENT_DROPOUT, LATENT_NOISE = 1, 2, 4      # flags of odvae_latent_stage_f32


def noise_fill(shape, draw, device, kind=0, p=0.0, first=0, nhwc=False):
    """A new f32 tensor of `shape` (contiguous: element = flat index) holding elements first .. of the stream in draw.tag: kind 0 =
    standard normals, 1 = dropout multipliers of probability p.  draw = latent_noise.Draw(key, step, tag); no host RNG, no upload.
    nhwc: shape is a logical [N, C, H, W] and the tensor comes in channels_last memory -- element = flat NHWC index, the latent's order."""
    L = _L()
    if nhwc:
        n, c, h, w = shape
        return noise_fill((n, h, w, c), draw, device, kind=kind, p=p, first=first).permute(0, 3, 1, 2)
    out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
    _lib.require_device(out)
    if out.numel():
        _lib.check(L.odvae_noise_fill_f32(out.data_ptr(), out.numel(), int(first), draw.key, draw.step, draw.tag, int(kind), float(p),
                                          _lib.stream_ptr()), "noise_fill")
    return out


class _LatentStage(Function):
    """z = ((mean + std * eps) * m + noise) + add in one launch; eps, m and noise are streams 0, 1, 2 of `draw`, made in registers.
    The backward keeps the moments alone and draws eps and m again; the gradient of `add` is dz itself."""

    @staticmethod
    def forward(ctx, moments, add, draw, flags, p):
        L = _L()
        moments = _cl(moments)
        a = _cl(add) if add is not None else None
        n, c2, h, w = moments.shape
        cz = c2 // 2
        if a is not None and tuple(a.shape) != (n, cz, h, w):
            raise ValueError("latent_stage: add %s does not have the latent's shape %s" % (tuple(a.shape), (n, cz, h, w)))
        z = _new_cl(n, cz, h, w, moments)
        _lib.check(L.odvae_latent_stage_f32(moments.data_ptr(), _lib.ptr(a), z.data_ptr(), n, h * w, cz, draw.key, draw.step, draw.tag,
                                            flags, p, _lib.stream_ptr()), "latent_stage")
        ctx.save_for_backward(moments)
        ctx.draw, ctx.flags, ctx.p, ctx.has_add = draw, flags, p, add is not None
        return z

    @staticmethod
    def backward(ctx, dz):
        L = _L()
        (moments,) = ctx.saved_tensors
        dz = _cl(dz)
        dm = None
        if ctx.needs_input_grad[0]:
            n, c2, h, w = moments.shape
            dm = _new_cl(n, c2, h, w, moments)
            _lib.check(L.odvae_latent_stage_bwd_f32(moments.data_ptr(), dz.data_ptr(), dm.data_ptr(), n, h * w, c2 // 2, ctx.draw.key,
                                                    ctx.draw.step, ctx.draw.tag, ctx.flags, ctx.p, _lib.stream_ptr()), "latent_stage_bwd")
        return dm, (dz if ctx.has_add and ctx.needs_input_grad[1] else None), None, None, None


def latent_stage(moments, draw, add=None, sample=True, dropout_p=0.0, noise=False):
    """The latent stage of one forward: sample (or mode), dropout of probability dropout_p (0 = off, >= 1 zeroes), + N(0,1) noise, + add.
    draw = latent_noise.Draw of the forward (stream 0's tag: the kernel adds the stream ids)."""
    p = min(float(dropout_p), 1.0)
    flags = (LATENT_SAMPLE if sample else 0) | (LATENT_DROPOUT if p > 0.0 else 0) | (LATENT_NOISE if noise else 0)
    return _LatentStage.apply(moments, add, draw, flags, max(p, 0.0))


# ------------------------------------------------------------------------------------------------------
# exponential moving average of the weights (ema.LitEma): raw launches on flat f32 storage, no autograd
# ------------------------------------------------------------------------------------------------------
def _flat_f32(*tensors):
    _lib.require_device(*tensors)
    for t in tensors:
        if not t.is_contiguous():
            raise ValueError("ema: needs contiguous storage, got strides %s for shape %s" % (t.stride(), tuple(t.shape)))


def ema_tick(decay, num_updates, state):
    """LitEma's counter step and decay schedule on the device: num_updates (int32, in place) += 1 unless negative, state <- [1 - d, d]."""
    L = _L()
    _lib.require_device(decay, state)
    _lib.require_device(num_updates, dtypes=(torch.int32,))
    if decay.numel() != 1 or num_updates.numel() != 1 or state.numel() != 2 or not state.is_contiguous():
        raise ValueError("ema_tick: decay and num_updates are scalars, state holds two floats")
    tag = KERNEL_EVENTS.begin(secondary=True)
    _lib.check(L.odvae_ema_tick(decay.data_ptr(), num_updates.data_ptr(), state.data_ptr(), _lib.stream_ptr()), "ema_tick")
    KERNEL_EVENTS.end("ema_tick", 0.0, tag, 20.0, issued=0.0)


def ema_update(param, shadow, state, numel=None):
    """shadow <- shadow - state[0] * (shadow - param) over `numel` floats (default: all of them) of two flat f32 tensors, in place."""
    L = _L()
    _flat_f32(param, shadow, state)
    n = min(param.numel(), shadow.numel()) if numel is None else int(numel)
    if n > param.numel() or n > shadow.numel():
        raise ValueError("ema_update: %d floats asked of tensors holding %d and %d" % (n, param.numel(), shadow.numel()))
    tag = KERNEL_EVENTS.begin(secondary=True)
    _lib.check(L.odvae_ema_update_f32(param.data_ptr(), shadow.data_ptr(), n, state.data_ptr(), _lib.stream_ptr()), "ema_update")
    KERNEL_EVENTS.end("ema_update", 0.0, tag, 12.0 * n, issued=0.0)


def ema_swap(a, b, numel=None):
    """Exchange the contents of two flat f32 tensors in one pass, in place (behind torch's version counters: the caller bumps PACK_CACHE)."""
    L = _L()
    _flat_f32(a, b)
    n = min(a.numel(), b.numel()) if numel is None else int(numel)
    if n > a.numel() or n > b.numel():
        raise ValueError("ema_swap: %d floats asked of tensors holding %d and %d" % (n, a.numel(), b.numel()))
    tag = KERNEL_EVENTS.begin(secondary=True)
    _lib.check(L.odvae_ema_swap_f32(a.data_ptr(), b.data_ptr(), n, _lib.stream_ptr()), "ema_swap")
    KERNEL_EVENTS.end("ema_swap", 0.0, tag, 16.0 * n, issued=0.0)


# ------------------------------------------------------------------------------------------------------
# pose head: every loss term in one launch (pose_f32.hip)
# ------------------------------------------------------------------------------------------------------
class _PoseLosses(Function):
    """out[9] = pose, class, bbox, fill, kl_bbox losses + the logged per-component means (t1, t2, t3, v3) of
    src/modules/losses/contperceptual.py:111-132,176-212.  Differentiable w.r.t. dec_pose and the box-posterior moments through
    out[0:5] only: the reference logs out[5:9] (the means of t1, t2, t3, v3) and never trains on them, so the backward kernel ignores
    their upstream gradient -- a non-zero one changes neither gradient (tests/test_pose_exact_gpu.py)."""

    @staticmethod
    def forward(ctx, dec_pose, moments, pose_gt, bbox_gt, fill_gt, class_gt, prior, prior_idx, bg_idx, l2, yaw, gamma, alpha):
        L = _L()
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        dec_pose, moments, pose_gt, bbox_gt, fill_gt, prior = (f32(t) for t in (dec_pose, moments, pose_gt, bbox_gt, fill_gt, prior))
        _lib.require_device(dec_pose, moments, pose_gt, bbox_gt, fill_gt, prior)
        class_gt = class_gt.detach().to(torch.int64).contiguous()
        prior_idx = prior_idx.detach().to(torch.int32).contiguous()
        b, w = dec_pose.shape
        nc = w - 8
        if moments.shape != (b, 16) or pose_gt.shape != (b, 4) or bbox_gt.shape != (b, 3) or fill_gt.numel() != b or prior.shape[1:] != (3, 8):
            raise ValueError("pose_losses: unexpected shapes %s %s %s %s %s %s" % tuple(tuple(t.shape) for t in (dec_pose, moments, pose_gt, bbox_gt, fill_gt, prior)))
        out = torch.empty(9, dtype=torch.float32, device=dec_pose.device)
        jac_pose = torch.empty(4, b, w, dtype=torch.float32, device=dec_pose.device)
        jac_mom = torch.empty(b, 16, dtype=torch.float32, device=dec_pose.device)
        _lib.check(L.odvae_pose_losses_f32(dec_pose.data_ptr(), pose_gt.data_ptr(), bbox_gt.data_ptr(), fill_gt.data_ptr(), class_gt.data_ptr(),
                                           moments.data_ptr(), prior.data_ptr(), prior_idx.data_ptr(), b, nc, prior.shape[0], int(bg_idx), int(l2),
                                           int(yaw), float(gamma), float(alpha), out.data_ptr(), jac_pose.data_ptr(), jac_mom.data_ptr(),
                                           _lib.stream_ptr()), "pose_losses")
        ctx.save_for_backward(jac_pose, jac_mom)
        ctx.dims = (b, nc)
        return out

    @staticmethod
    def backward(ctx, g):
        L = _L()
        jac_pose, jac_mom = ctx.saved_tensors
        b, nc = ctx.dims
        g = g.contiguous()
        d_pose = torch.empty(b, 8 + nc, dtype=torch.float32, device=g.device)
        d_mom = torch.empty(b, 16, dtype=torch.float32, device=g.device)
        _lib.check(L.odvae_pose_losses_bwd_f32(g.data_ptr(), jac_pose.data_ptr(), jac_mom.data_ptr(), b, nc, d_pose.data_ptr(), d_mom.data_ptr(),
                                               _lib.stream_ptr()), "pose_losses_bwd")
        return (d_pose, d_mom) + (None,) * 11


def pose_losses(dec_pose, moments, pose_gt, bbox_gt, fill_gt, class_gt, prior, prior_idx, bg_idx=1, l2=False, yaw=True, gamma=2.0, alpha=0.25):
    return _PoseLosses.apply(dec_pose, moments, pose_gt, bbox_gt, fill_gt, class_gt, prior, prior_idx, bg_idx, l2, yaw, gamma, alpha)


# ------------------------------------------------------------------------------------------------------
# pose head MLPs: skinny dense layers (linear_f32.hip)
# ------------------------------------------------------------------------------------------------------
LINEAR_ACTS = {None: 0, "none": 0, "tanh": 1, "swish": 2, "silu": 2, "relu": 3}


class _LinearAct(Function):
    """y = act(x . W^T + b) for the batch-sized rows of the pose MLPs (pose_encoder.py:59-131, pose_decoder.py:60-97); the
    epilogue kernel fuses the split-K sum, the bias and the activation and keeps the pre-activation for the backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, act):
        L = _L()
        x2 = x.detach().to(torch.float32).reshape(-1, x.shape[-1]).contiguous()
        w = weight.detach().contiguous()
        b = None if bias is None else bias.detach().contiguous()
        _lib.require_device(x2, w, *(() if b is None else (b,)))
        m, k = x2.shape
        n = w.shape[0]
        if w.shape[1] != k or (b is not None and b.numel() != n):
            raise ValueError("linear_act: x %s, weight %s, bias %s" % (tuple(x.shape), tuple(w.shape), None if b is None else tuple(b.shape)))
        y = torch.empty(m, n, dtype=torch.float32, device=x2.device)
        pre = torch.empty_like(y) if act else None
        wp, wn = _ws(L.odvae_linear_workspace_bytes(m, n, k), y)
        _lib.check(L.odvae_linear_fwd_f32(x2.data_ptr(), w.data_ptr(), _lib.ptr(b), m, n, k, act, y.data_ptr(), _lib.ptr(pre), wp, wn,
                                          _lib.stream_ptr()), "linear_fwd")
        ctx.save_for_backward(x2, w, pre)
        ctx.act, ctx.has_bias, ctx.x_shape = act, b is not None, x.shape
        return y.reshape(x.shape[:-1] + (n,))

    @staticmethod
    def backward(ctx, dy):
        L = _L()
        x2, w, pre = ctx.saved_tensors
        m, k = x2.shape
        n = w.shape[0]
        dy = dy.to(torch.float32).reshape(m, n).contiguous()
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dpre = torch.empty_like(dy)
        dx = torch.empty(m, k, dtype=torch.float32, device=dy.device) if need_x else None
        dw = torch.empty(n, k, dtype=torch.float32, device=dy.device) if need_w else None
        wp, wn = _ws(L.odvae_linear_workspace_bytes(m, n, k), dy)
        _lib.check(L.odvae_linear_bwd_f32(x2.data_ptr(), w.data_ptr(), _lib.ptr(pre), dy.data_ptr(), m, n, k, ctx.act, dpre.data_ptr(),
                                          _lib.ptr(dx), _lib.ptr(dw), wp, wn, _lib.stream_ptr()), "linear_bwd")
        db = _colsum(dpre, m, n) if need_b else None
        return (dx.reshape(ctx.x_shape) if need_x else None), dw, db, None


def linear_act(x, weight, bias=None, act=None):
    """act(x @ weight.T + bias) on the small-batch MFMA kernel; act in LINEAR_ACTS."""
    return _LinearAct.apply(x, weight, bias, LINEAR_ACTS[act])
