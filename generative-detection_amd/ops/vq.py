"""The vector quantiser of ldm's VQModel (csrc/vq_f32.hip): fused nearest-code search, deterministic codebook gradient."""
import ctypes

import torch
from torch.autograd import Function

from .. import lib as _lib
from ._base import _L, _ws

VQ_PLAN_FIELDS = ("tile_rows", "chunk", "slab_depth", "nslabs", "nsplit", "codes_per_split", "search_grid", "search_grid_cap",
                  "finish_blocks", "finish_cap", "sort_codes_per_block", "sort_code_ranges", "sort_row_segments", "sort_rows_per_segment",
                  "stream_grid_cap", "reserved")


def vq_plan(m, n_codes, dim):
    """odvae_vq_plan as a dict: the launch rule of the quantiser for M rows, K codes of dimension D; host only, needs no device."""
    out = (ctypes.c_int * 16)()
    _lib.check(_L().odvae_vq_plan(int(m), int(n_codes), int(dim), out), "odvae_vq_plan")
    return dict(zip(VQ_PLAN_FIELDS, out))


def _row_strides(t):
    """(sn, sc, sp) of a logical [N, D, H, W] tensor whose H and W collapse into one position axis (NCHW-contiguous and the NHWC memory
    of the conv kernels both do), else None"""
    n, d, h, w = t.shape
    sn, sc, sh, sw = t.stride()
    if w == 1:
        sp = sh if h > 1 else 1
    elif h == 1 or sh == w * sw:
        sp = sw
    else:
        return None
    if d == 1:
        sc = 1      # (the stride of an axis of one element is never used)
    if n == 1:
        sn = 0
    if sp < 1 or sc < 1 or sn < 0 or (n > 1 and sn < 1):
        return None
    return sn, sc, sp


def _rows_view(t):
    """`t` itself where the kernels can address it by (sn, sc, sp), else an NCHW-contiguous copy; with its strides"""
    s = _row_strides(t)
    if s is None or not _dense(t):
        t = t.contiguous()
        s = _row_strides(t)
    return t, s


def _dense(t):
    """no two elements share memory and none is skipped: what the kernels may write through the same strides"""
    return t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last)


def _codebook(codebook):
    if codebook.dim() != 2:
        raise ValueError("codebook must be [n_codes, dim], got %s" % (tuple(codebook.shape),))
    return codebook.detach().contiguous()


class _VqQuantize(Function):
    """(z_q, loss, indices) of VectorQuantizer2.forward; the straight-through estimator and both loss terms in one backward call."""

    @staticmethod
    def forward(ctx, z, codebook, beta, legacy):
        L = _L()
        _lib.require_device(z, codebook)
        if z.dim() != 4 or z.shape[1] != codebook.shape[1]:
            raise ValueError("z must be [N, %d, H, W] for a codebook %s, got %s" % (codebook.shape[1], tuple(codebook.shape), tuple(z.shape)))
        zd, zs = _rows_view(z.detach())
        e = _codebook(codebook)
        n, d, h, w = zd.shape
        k = e.shape[0]
        m = n * h * w
        zq = torch.empty_like(zd)
        if zq.stride() != zd.stride():
            zq = torch.empty_strided(zd.shape, zd.stride(), dtype=zd.dtype, device=zd.device)
        idx = torch.empty(m, dtype=torch.int64, device=z.device)
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        nbytes = L.odvae_vq_assign_workspace_bytes(m, k, d)
        if nbytes == 0:
            raise ValueError("vq_quantize: unsupported sizes M=%d K=%d D=%d (1 <= D <= 512, 1 <= K <= 2^20, M < 2^31)" % (m, k, d))
        wp, wn = _ws(nbytes, z)
        st = _lib.stream_ptr()
        _lib.check(L.odvae_vq_assign_f32(zd.data_ptr(), zs[0], zs[1], zs[2], n, h * w, d, e.data_ptr(), k, idx.data_ptr(), zq.data_ptr(),
                                         zs[0], zs[1], zs[2], wp, wn, st), "vq_assign")
        _lib.check(L.odvae_vq_loss_finalize(wp, wn, m, k, d, float(beta), loss.data_ptr(), st), "vq_loss_finalize")
        ctx.beta, ctx.legacy, ctx.zs = float(beta), bool(legacy), zs
        ctx.save_for_backward(zd, e, idx)
        ctx.mark_non_differentiable(idx)
        return zq, loss, idx

    @staticmethod
    def backward(ctx, gq, gl, _gidx):
        L = _L()
        zd, e, idx = ctx.saved_tensors
        n, d, h, w = zd.shape
        k = e.shape[0]
        m = n * h * w
        want_dz, want_de = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_dz or want_de):
            return None, None, None, None
        if gq is not None:
            _lib.require_device(gq)
            if gq.stride() != zd.stride():
                g = torch.empty_strided(zd.shape, zd.stride(), dtype=zd.dtype, device=zd.device)
                g.copy_(gq)
                gq = g
        if gl is not None:
            _lib.require_device(gl)
            gl = gl.contiguous()
        dz = torch.empty_strided(zd.shape, zd.stride(), dtype=zd.dtype, device=zd.device) if want_dz else None
        de = torch.empty_like(e) if want_de else None
        wp, wn = (None, 0)
        if want_de:
            wp, wn = _ws(L.odvae_vq_backward_workspace_bytes(m, k, d), zd)
        zs = ctx.zs
        _lib.check(L.odvae_vq_backward_f32(zd.data_ptr(), _lib.ptr(gq), _lib.ptr(dz), zs[0], zs[1], zs[2], n, h * w, d, e.data_ptr(), k,
                                           idx.data_ptr(), _lib.ptr(gl), ctx.beta, int(ctx.legacy), _lib.ptr(de), wp, wn,
                                           _lib.stream_ptr()), "vq_backward")
        return dz, de, None, None


def vq_quantize(z, codebook, beta, legacy=True):
    """z f32 [N, D, H, W] (NCHW or channels_last memory, read in place), codebook f32 [K, D] -> (z_q like z, loss f32 scalar,
    indices int64 [N*H*W]).  idx = argmin_k |e_k|^2 - 2 z.e_k, ties to the lowest k; loss = (1 + beta) mean (z_q - z)^2; the gradient
    of z_q passes straight through to z, the loss reaches z and the codebook with beta on the term `legacy` selects."""
    return _VqQuantize.apply(z, codebook, beta, legacy)


def vq_gather(indices, codebook, shape):
    """codebook[indices] as [N, D, H, W] (channels_last memory) for shape = (N, H, W, D) -- taming's (batch, height, width, channel).
    An index outside [0, K) is clamped to the nearest valid code.  No gradient."""
    L = _L()
    _lib.require_device(indices, dtypes=(torch.int64,))
    _lib.require_device(codebook)
    e = _codebook(codebook)
    n, h, w, d = (int(v) for v in shape)
    if d != e.shape[1] or indices.numel() != n * h * w:
        raise ValueError("vq_gather: %d indices and a codebook %s do not fill shape %s" % (indices.numel(), tuple(e.shape), tuple(shape)))
    idx = indices.detach().reshape(-1).contiguous()
    out = torch.empty((n, h, w, d), dtype=torch.float32, device=e.device).permute(0, 3, 1, 2)
    _lib.check(L.odvae_vq_gather_f32(idx.data_ptr(), n, h * w, e.data_ptr(), e.shape[0], d, out.data_ptr(), h * w * d, 1, d,
                                     _lib.stream_ptr()), "vq_gather")
    return out


def vq_usage(indices, n_codes):
    """(counts int32 [n_codes], perplexity, cluster_usage) of the indices, the two scalars f32 on the device:
    perplexity = exp(-sum p log(p + 1e-10)), p = count / M; cluster_usage = number of codes used."""
    L = _L()
    _lib.require_device(indices, dtypes=(torch.int64,))
    idx = indices.detach().reshape(-1).contiguous()
    counts = torch.empty(int(n_codes), dtype=torch.int32, device=idx.device)
    out = torch.empty(2, dtype=torch.float32, device=idx.device)
    _lib.check(L.odvae_vq_usage(idx.data_ptr(), idx.numel(), int(n_codes), counts.data_ptr(), out.data_ptr(), _lib.stream_ptr()), "vq_usage")
    return counts, out[0], out[1]
