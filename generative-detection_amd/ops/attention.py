"""Attention over T = H*W tokens from a packed qkv tensor: the GEMM path (scores in HBM), its recompute form, linear attention,
and the fused (flash) kernels in bf16 and f32."""
import collections

import torch
from torch.autograd import Function

from .. import ops as _ops      # the package: switches and run-time state are read and written there (ops/__init__.py)
from .. import lib as _lib
from ._base import BF16, CL, KERNEL_EVENTS, _L, _cl, _new_cl, _ws
from .gemm import gemm
from .precision import _sync_precision


def _qkv_views(t, c):
    """q, k, v of a packed NHWC [N, 3C, H, W] tensor as pointer-carrying views: channel offsets 0, C, 2C of its first pixel (the kernels
    take the pixel stride 3C as the leading dimension)."""
    off = t.storage_offset()
    return tuple(t.as_strided((1,), (1,), off + i * c) for i in range(3))


class _Attention(Function):
    """Single-head attention over T = H*W tokens from a packed qkv tensor [N, 3C, H, W]:
    softmax(q k^T * C^-0.5) v  ([UPSTREAM] AttnBlock.forward).  Scores live in HBM (T x T per image)."""

    @staticmethod
    def forward(ctx, qkv):
        L = _L()
        _sync_precision(L)      # the T x T products below call the library directly
        qkv = _cl(qkv)
        n, c3, h, w = qkv.shape
        c = c3 // 3
        t = h * w
        scale = float(c) ** -0.5
        p = torch.empty(n, t, t, dtype=torch.float32, device=qkv.device)
        o = _new_cl(n, c, h, w, qkv)
        q, k, v = _qkv_views(qkv, c)
        sq = t * c3
        rinv = None
        if _ops.ATTN_FOLDED_SOFTMAX and L.odvae_gemm_f32_workspace_bytes(t, t, c, n) == 0 and L.odvae_gemm_f32_workspace_bytes(t, c, t, n) == 0:
            st = _lib.stream_ptr()
            bound = torch.empty(2, n * t, dtype=torch.float32, device=qkv.device)      # [0]: the bounds, [1]: scratch (|k_j|)
            rinv = torch.empty(n * t, dtype=torch.float32, device=qkv.device)
            flag = torch.empty(1, dtype=torch.int32, device=qkv.device)
            _lib.check(L.odvae_attn_row_bound_f32(q.data_ptr(), n, t, c, bound.data_ptr(), bound[1].data_ptr(), flag.data_ptr(), st), "attn_row_bound")
            tag = KERNEL_EVENTS.begin(secondary=True)
            _lib.check(L.odvae_gemm_exp_bound_f32(t, t, c, scale, q.data_ptr(), c3, sq, k.data_ptr(), c3, sq, bound.data_ptr(), t,
                                                  p.data_ptr(), t, t * t, n, st), "gemm_exp_bound")
            KERNEL_EVENTS.end("gemm_f32", 2.0 * t * t * c * n, tag, 4.0 * n * (2 * t * c + t * t))
            tag = KERNEL_EVENTS.begin(secondary=True)
            _lib.check(L.odvae_gemm_rownorm_f32(t, c, t, p.data_ptr(), t, t * t, v.data_ptr(), c3, sq, o.data_ptr(), c, t * c,
                                                rinv.data_ptr(), t, flag.data_ptr(), n, st), "gemm_rownorm")
            KERNEL_EVENTS.end("gemm_f32", 2.0 * t * t * c * n, tag, 4.0 * n * (2 * t * c + t * t))
            # fallback under the device-side flag (three launches that return at once when it is 0): exact softmax, row factors 1
            _lib.check(L.odvae_gemm_pred_f32(0, 1, t, t, c, 1.0, q.data_ptr(), c3, sq, k.data_ptr(), c3, sq, p.data_ptr(), t, t * t, n,
                                             flag.data_ptr(), st), "gemm_pred(QK^T)")
            _lib.check(L.odvae_softmax_rows_pred_f32(p.data_ptr(), p.data_ptr(), n * t, t, scale, flag.data_ptr(), rinv.data_ptr(), st), "softmax_rows_pred")
            _lib.check(L.odvae_gemm_pred_f32(0, 0, t, c, t, 1.0, p.data_ptr(), t, t * t, v.data_ptr(), c3, sq, o.data_ptr(), c, t * c, n,
                                             flag.data_ptr(), st), "gemm_pred(PV)")
            _ops._ATTN_LAST_FLAG = flag      # (diagnostics / tests: 1 after a forward whose bound underflowed and whose fallback ran)
        else:
            gemm(0, 1, t, t, c, 1.0, q, c3, sq, k, c3, sq, p, t, t * t, batch=n)
            _lib.check(L.odvae_softmax_rows_f32(p.data_ptr(), p.data_ptr(), n * t, t, scale, _lib.stream_ptr()), "softmax_rows")
            gemm(0, 0, t, c, t, 1.0, p, t, t * t, v, c3, sq, o, c, t * c, batch=n)
        ctx.folded = rinv is not None
        if rinv is not None:
            ctx.save_for_backward(qkv, p, o, rinv)
        else:
            ctx.save_for_backward(qkv, p, o)
        return o

    @staticmethod
    def backward(ctx, do):
        L = _L()
        _sync_precision(L)
        if ctx.folded:
            qkv, p, o, rinv = ctx.saved_tensors      # p holds E = exp(scale (s - bound)), P = E * rinv[row]
        else:
            (qkv, p, o), rinv = ctx.saved_tensors, None
        do = _cl(do)
        n, c3, h, w = qkv.shape
        c = c3 // 3
        t = h * w
        scale = float(c) ** -0.5
        sq = t * c3
        q, k, v = _qkv_views(qkv, c)
        dqkv = _new_cl(n, c3, h, w, qkv)
        dq, dk, dv = _qkv_views(dqkv, c)
        if rinv is not None:
            # D_i = dO_i . O_i and dO_i / l_i in one pass over dO; dV = E^T (dO / l); dS = scale E rinv (dO V^T - D)
            drow = torch.empty(n * t, dtype=torch.float32, device=p.device)
            dos = torch.empty_like(do)
            _lib.check(L.odvae_rowdot_scale_f32(do.data_ptr(), o.data_ptr(), rinv.data_ptr(), n * t, c, drow.data_ptr(), dos.data_ptr(),
                                                _lib.stream_ptr()), "rowdot_scale")
            gemm(1, 0, t, c, t, 1.0, p, t, t * t, dos, c, t * c, dv, c3, sq, batch=n)
            del dos
            dp = torch.empty_like(p)
            tag = KERNEL_EVENTS.begin(secondary=True)
            _lib.check(L.odvae_gemm_softmax_bwd_scaled_f32(t, t, c, scale, do.data_ptr(), c, t * c, v.data_ptr(), c3, sq, p.data_ptr(),
                                                           drow.data_ptr(), rinv.data_ptr(), t, dp.data_ptr(), t, t * t, n, _lib.stream_ptr()),
                       "gemm_softmax_bwd_scaled")
            KERNEL_EVENTS.end("gemm_f32", 2.0 * t * t * c * n, tag, 4.0 * n * (2 * t * c + 2 * t * t))
            gemm(0, 0, t, c, t, 1.0, dp, t, t * t, k, c3, sq, dq, c3, sq, batch=n)
            gemm(1, 0, t, c, t, 1.0, dp, t, t * t, q, c3, sq, dk, c3, sq, batch=n)
            return dqkv
        # dV = P^T dO
        gemm(1, 0, t, c, t, 1.0, p, t, t * t, do, c, t * c, dv, c3, sq, batch=n)
        # dS = scale * P .* (dO V^T - D), D[i] = sum_j P[i][j] dP[i][j] = dO[i] . O[i]: the softmax backward rides in the
        # epilogue of the dP product (no dP round trip through HBM, no separate softmax-backward pass)
        dp = torch.empty_like(p)
        if _ops.FUSED_SOFTMAX_BWD:
            drow = torch.empty(n * t, dtype=torch.float32, device=p.device)
            _lib.check(L.odvae_rowdot_f32(do.data_ptr(), o.data_ptr(), n * t, c, drow.data_ptr(), _lib.stream_ptr()), "rowdot")
            tag = KERNEL_EVENTS.begin(secondary=True)
            _lib.check(L.odvae_gemm_softmax_bwd_f32(t, t, c, scale, do.data_ptr(), c, t * c, v.data_ptr(), c3, sq, p.data_ptr(),
                                                    drow.data_ptr(), t, dp.data_ptr(), t, t * t, n, _lib.stream_ptr()),
                       "gemm_softmax_bwd")
            KERNEL_EVENTS.end("gemm_f32", 2.0 * t * t * c * n, tag, 4.0 * n * (2 * t * c + 2 * t * t))
        else:
            gemm(0, 1, t, t, c, 1.0, do, c, t * c, v, c3, sq, dp, t, t * t, batch=n)
            _lib.check(L.odvae_softmax_rows_bwd_f32(p.data_ptr(), dp.data_ptr(), dp.data_ptr(), n * t, t, scale,
                                                    _lib.stream_ptr()), "softmax_rows_bwd")
        # dQ = dS K ; dK = dS^T Q
        gemm(0, 0, t, c, t, 1.0, dp, t, t * t, k, c3, sq, dq, c3, sq, batch=n)
        gemm(1, 0, t, c, t, 1.0, dp, t, t * t, q, c3, sq, dk, c3, sq, batch=n)
        return dqkv


class _AttentionRecompute(Function):
    """softmax(q k^T * C^-0.5) v as _Attention, with the T x T scores living in a scratch buffer of at most ATTN_SCORE_BUDGET bytes."""

    @staticmethod
    def _probabilities(L, qkv, g0, g, t, c, scale, p):
        c3, sq = 3 * c, t * 3 * c
        q, k, _ = _qkv_views(qkv[g0:g0 + g], c)
        gemm(0, 1, t, t, c, 1.0, q, c3, sq, k, c3, sq, p, t, t * t, batch=g)
        _lib.check(L.odvae_softmax_rows_f32(p.data_ptr(), p.data_ptr(), g * t, t, scale, _lib.stream_ptr()), "softmax_rows")

    @staticmethod
    def forward(ctx, qkv, group):
        L = _L()
        qkv = _cl(qkv)
        n, c3, h, w = qkv.shape
        c, t = c3 // 3, h * w
        scale = float(c) ** -0.5
        o = _new_cl(n, c, h, w, qkv)
        p = torch.empty(min(group, n), t, t, dtype=torch.float32, device=qkv.device)
        for g0 in range(0, n, group):
            g = min(group, n - g0)
            _AttentionRecompute._probabilities(L, qkv, g0, g, t, c, scale, p)
            v = _qkv_views(qkv[g0:g0 + g], c)[2]
            gemm(0, 0, t, c, t, 1.0, p, t, t * t, v, c3, t * c3, o[g0:g0 + g], c, t * c, batch=g)
        ctx.group = group
        ctx.save_for_backward(qkv, o)
        return o

    @staticmethod
    def backward(ctx, do):
        L = _L()
        _sync_precision(L)
        qkv, o = ctx.saved_tensors
        do = _cl(do)
        n, c3, h, w = qkv.shape
        c, t = c3 // 3, h * w
        scale = float(c) ** -0.5
        sq = t * c3
        group = max(1, ctx.group // 2)          # two score-sized buffers live here (P and dS)
        dqkv = _new_cl(n, c3, h, w, qkv)
        p = torch.empty(min(group, n), t, t, dtype=torch.float32, device=qkv.device)
        dp = torch.empty_like(p)
        drow = torch.empty(n * t, dtype=torch.float32, device=qkv.device)
        _lib.check(L.odvae_rowdot_f32(do.data_ptr(), o.data_ptr(), n * t, c, drow.data_ptr(), _lib.stream_ptr()), "rowdot")
        for g0 in range(0, n, group):
            g = min(group, n - g0)
            _AttentionRecompute._probabilities(L, qkv, g0, g, t, c, scale, p)
            q, k, v = _qkv_views(qkv[g0:g0 + g], c)
            dq, dk, dv = _qkv_views(dqkv[g0:g0 + g], c)
            dog = do[g0:g0 + g]
            gemm(1, 0, t, c, t, 1.0, p, t, t * t, dog, c, t * c, dv, c3, sq, batch=g)                       # dV = P^T dO
            tag = KERNEL_EVENTS.begin(secondary=True)
            _lib.check(L.odvae_gemm_softmax_bwd_f32(t, t, c, scale, dog.data_ptr(), c, t * c, v.data_ptr(), c3, sq, p.data_ptr(),
                                                    drow.data_ptr() + 4 * g0 * t, t, dp.data_ptr(), t, t * t, g, _lib.stream_ptr()),
                       "gemm_softmax_bwd")                                                                 # dS = scale P (dO V^T - D)
            KERNEL_EVENTS.end("gemm_f32", 2.0 * t * t * c * g, tag, 4.0 * g * (2 * t * c + 2 * t * t))
            gemm(0, 0, t, c, t, 1.0, dp, t, t * t, k, c3, sq, dq, c3, sq, batch=g)                          # dQ = dS K
            gemm(1, 0, t, c, t, 1.0, dp, t, t * t, q, c3, sq, dk, c3, sq, batch=g)                          # dK = dS^T Q
        return dqkv, None


def attention_qkv(qkv):
    if qkv.dtype == BF16:
        return _FlashAttention.apply(qkv)
    n, c3, h, w = qkv.shape
    if _ops.ATTN_F32_FUSED and qkv.dtype == torch.float32 and _L().odvae_flash_attn_f32_supported(n, h * w, c3 // 3):
        return _FlashAttentionF32.apply(qkv)
    per_image = (h * w) ** 2 * 4
    if n * per_image > _ops.ATTN_SCORE_BUDGET:
        return _AttentionRecompute.apply(qkv, max(1, _ops.ATTN_SCORE_BUDGET // per_image))
    return _Attention.apply(qkv)


class _LinearAttention(Function):
    """Linear attention over T = H*W tokens from a packed projection [N, 3C, H, W] ([UPSTREAM] LinearAttention, heads = 1):
    k' = softmax(k over the tokens, per image and channel), ctx = k'^T v [N, C, C], out = q ctx.  No scale, no softmax over q.
    Work 4 T C^2 per image (the vanilla block: 4 T^2 C).  Kept for the backward: qkv, ctx and the column statistics (max, 1 / sum)
    of k -- neither out nor k' (linattn_f32.hip re-makes k' from k and the statistics in its loaders)."""

    @staticmethod
    def forward(ctx_, qkv):
        L = _L()
        qkv = _aligned_cl(qkv)
        n, c3, h, w = qkv.shape
        c, t = c3 // 3, h * w
        if c3 != 3 * c or c % 32 != 0 or t < 1:
            raise _lib.HipLibraryError("linear attention: needs [N, 3C, H, W] with C a multiple of 32, got %s" % (tuple(qkv.shape),))
        q, k, v = _qkv_views(qkv, c)
        sq, st = t * c3, _lib.stream_ptr()
        stats = torch.empty(2, n, c, dtype=torch.float32, device=qkv.device)       # [0]: column maxima of k, [1]: 1 / sum exp(k - max)
        cx = torch.empty(n, c, c, dtype=torch.float32, device=qkv.device)
        wp, wn = _ws(L.odvae_linattn_colstats_workspace_bytes(n, t, c), qkv)
        tag = KERNEL_EVENTS.begin(secondary=True)
        _lib.check(L.odvae_linattn_colstats_f32(k.data_ptr(), c3, sq, n, t, c, stats[0].data_ptr(), stats[1].data_ptr(), wp, wn, st),
                   "linattn_colstats")
        KERNEL_EVENTS.end("linattn_colstats", 0.0, tag, 4.0 * n * t * c, issued=0.0)
        wp, wn = _ws(L.odvae_linattn_ctx_workspace_bytes(n, t, c), qkv)
        tag = KERNEL_EVENTS.begin(secondary=True)
        _lib.check(L.odvae_linattn_ctx_f32(k.data_ptr(), v.data_ptr(), c3, sq, stats[0].data_ptr(), stats[1].data_ptr(), n, t, c,
                                           cx.data_ptr(), wp, wn, st), "linattn_ctx")
        KERNEL_EVENTS.end("linattn_ctx", 2.0 * t * c * c * n, tag, 4.0 * n * (2 * t * c + c * c))
        o = _new_cl(n, c, h, w, qkv)
        gemm(0, 0, t, c, c, 1.0, q, c3, sq, cx, c, c * c, o, c, t * c, batch=n)                           # out = q ctx
        ctx_.save_for_backward(qkv, cx, stats)
        return o

    @staticmethod
    def backward(ctx_, do):
        L = _L()
        qkv, cx, stats = ctx_.saved_tensors
        do = _cl(do)
        n, c3, h, w = qkv.shape
        c, t = c3 // 3, h * w
        sq = t * c3
        q, k, v = _qkv_views(qkv, c)
        dqkv = _new_cl(n, c3, h, w, qkv)
        dq, dk, dv = _qkv_views(dqkv, c)
        dcx = torch.empty_like(cx)
        gemm(1, 0, c, c, t, 1.0, q, c3, sq, do, c, t * c, dcx, c, c * c, batch=n)                         # dctx = q^T dOut
        gemm(0, 1, t, c, c, 1.0, do, c, t * c, cx, c, c * c, dq, c3, sq, batch=n)                         # dq = dOut ctx^T
        # g[d] = ctx[d] . dctx[d] = sum_n k'[n][d] dk'[n][d]: the softmax backward's reduction over the tokens, from two C x C tensors
        g = torch.empty(n, c, dtype=torch.float32, device=qkv.device)
        _lib.check(L.odvae_rowdot_f32(cx.data_ptr(), dcx.data_ptr(), n * c, c, g.data_ptr(), _lib.stream_ptr()), "rowdot")
        tag = KERNEL_EVENTS.begin(secondary=True)
        _lib.check(L.odvae_linattn_dkv_f32(k.data_ptr(), v.data_ptr(), c3, sq, stats[0].data_ptr(), stats[1].data_ptr(), dcx.data_ptr(),
                                           g.data_ptr(), n, t, c, dk.data_ptr(), dv.data_ptr(), c3, sq, _lib.stream_ptr()), "linattn_dkv")
        KERNEL_EVENTS.end("linattn_dkv", 4.0 * t * c * c * n, tag, 4.0 * n * (4 * t * c + c * c))
        return dqkv


def linear_attention_qkv(qkv):
    """out [N, C, H, W] f32 of the linear attention on a packed f32 projection [N, 3C, H, W] (q | k | v channel thirds); any strides."""
    _lib.require_device(qkv)
    return _LinearAttention.apply(qkv)


# Tokens per workgroup of the context product (CTX_SPLIT of linattn_f32.hip, odvae_linattn_ctx_split()): from T = this + 1 on the product
# adds partial tiles from workspace.  Named here so that tests can place T around it; tests/test_linattn_gpu.py holds it to the library's.
LINATTN_CTX_SPLIT = 1024


def _aligned_cl(t):
    """_cl(t) with a 16-byte aligned base (the fused f32 kernels load float4 rows)."""
    t = _cl(t)
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=CL)


# Per-dtype description of the fused-attention Functions: dtype, bytes per element, input preparation, entry points (by name), the name in
# error messages and the suffix of the launch labels, and the issued-FLOP factor of a backward as a function of C:
# seven products (S and dP are formed in both backward kernels); f32 at C = 512: eight, the dK and dV launches each form S
_FlashKind = collections.namedtuple("_FlashKind", "dtype esz prep supported fwd bwd what suffix issued")
_FLASH_BF16 = _FlashKind(BF16, 2.0, lambda t: _cl(t, BF16), "odvae_flash_attn_supported", "odvae_flash_attn_fwd_bf16",
                         "odvae_flash_attn_bwd_bf16", "flash attention", "", lambda c: 14.0)
_FLASH_F32 = _FlashKind(torch.float32, 4.0, _aligned_cl, "odvae_flash_attn_f32_supported", "odvae_flash_attn_fwd_f32",
                        "odvae_flash_attn_bwd_f32", "flash attention f32", "_f32", lambda c: 16.0 if c == 512 else 14.0)


def _flash_forward(kind, ctx, qkv):
    L = _L()
    qkv = kind.prep(qkv)
    n, c3, h, w = qkv.shape
    c, t = c3 // 3, h * w
    if not getattr(L, kind.supported)(n, t, c):
        raise _lib.HipLibraryError("%s: unsupported shape N=%d T=%d C=%d" % (kind.what, n, t, c))
    o = _new_cl(n, c, h, w, qkv, dtype=kind.dtype)
    lse = torch.empty(n, t, dtype=torch.float32, device=qkv.device)
    tag = KERNEL_EVENTS.begin(secondary=True)
    _lib.check(getattr(L, kind.fwd)(qkv.data_ptr(), n, t, c, float(c) ** -0.5, o.data_ptr(), lse.data_ptr(), _lib.stream_ptr()),
               "flash_attn_fwd" + kind.suffix)
    KERNEL_EVENTS.end("flash_attn", 4.0 * t * t * c * n, tag, kind.esz * n * t * 4 * c)
    ctx.save_for_backward(qkv, o, lse)
    return o


def _flash_backward(kind, ctx, do):
    L = _L()
    qkv, o, lse = ctx.saved_tensors
    do = kind.prep(do)
    n, c3, h, w = qkv.shape
    c, t = c3 // 3, h * w
    dqkv = _new_cl(n, c3, h, w, qkv, dtype=kind.dtype)
    delta = torch.empty(n * t, dtype=torch.float32, device=qkv.device)
    tag = KERNEL_EVENTS.begin(secondary=True)
    _lib.check(getattr(L, kind.bwd)(qkv.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), n, t, c, float(c) ** -0.5,
                                    dqkv.data_ptr(), delta.data_ptr(), _lib.stream_ptr()), "flash_attn_bwd" + kind.suffix)
    # algorithmic: the five products of the backward (S, dP, dV, dK, dQ)
    KERNEL_EVENTS.end("flash_attn", 10.0 * t * t * c * n, tag, kind.esz * n * t * 8 * c, issued=kind.issued(c) * t * t * c * n)
    return dqkv


class _FlashAttention(Function):
    """softmax(q k^T C^-1/2) v from the packed bf16 projection [N, 3C, H, W]; the T x T scores stay on the CU (flash_attn_bf16.hip);
    only o and the per-row log-sum-exp are kept for the backward."""

    @staticmethod
    def forward(ctx, qkv):
        return _flash_forward(_FLASH_BF16, ctx, qkv)

    @staticmethod
    def backward(ctx, do):
        return _flash_backward(_FLASH_BF16, ctx, do)


class _FlashAttentionF32(Function):
    """softmax(q k^T C^-1/2) v from the packed f32 projection [N, 3C, H, W] with the T x T scores on the CU (flash_attn_f32.hip);
    only qkv, o and the per-row base-2 log-sum-exp are kept for the backward."""

    @staticmethod
    def forward(ctx, qkv):
        return _flash_forward(_FLASH_F32, ctx, qkv)

    @staticmethod
    def backward(ctx, do):
        return _flash_backward(_FLASH_F32, ctx, do)
